"""Shared checks of Deflate strips in pylinac_amd.tiff (Compression 8 / 32946: load_frames(deflate=True), decode_tiff_strips
with mask bit 8, pl_tiff_decode_ex / pl_tiff_work_bytes_ex): tests/test_emulated_tiff_deflate.py on the CPU emulator,
tests/test_gpu_tiff_deflate.py on the MI355X.  Every pixel comparison is EQUALITY with ``np.asarray(PIL.Image.open(f))``
(libtiff + zlib), as in tests/tiff_checks.py, whose writer, oracle and frames are used here.

The files come from PIL (``tiff_adobe_deflate`` = Compression 8, ``tiff_deflate`` = 32946) and from ``deflate_file``:
``tiff_checks.write_tiff`` with a ``mangle`` that compresses every strip with zlib -- any encoder setting, either byte order,
damaged streams.  PIL is asked first in every case: a sound fixture must read back equal to its source, a damaged one must
raise ``OSError`` there.  The rows of "accepted oddities" are asserted against the SOURCE array (a PIL linked against another
inflate could refuse a cut trailer; the device follows libtiff + zlib)."""
from __future__ import annotations

import re
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import tiff_checks as tc
from pylinac_amd import tiff
from tiff_checks import SHAPES, pil_array, pil_file, ridge, strip_table, to_np, write_tiff  # noqa: F401

PIL_NAMES = {"tiff_adobe_deflate": tiff.COMPRESSION_DEFLATE, "tiff_deflate": tiff.COMPRESSION_DEFLATE_OLD}


# ---- files ----------------------------------------------------------------------------------------------------------------
def packer(level=-1, wbits=15, strategy=zlib.Z_DEFAULT_STRATEGY):
    def pack(raw: bytes) -> bytes:
        c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
        return c.compress(raw) + c.flush()
    return pack


def deflate_file(a: np.ndarray, compression: int = 8, pack=zlib.compress, damage=None, **kw) -> bytes:
    """write_tiff with every strip as a zlib stream; ``damage(k, stream, raw) -> stream`` edits strip k's"""
    raws = []

    def mangle(k, raw):
        raws.append(raw)
        z = pack(raw)
        return damage(k, z, raw) if damage else z

    return write_tiff(a, compression=compression, mangle=mangle, **kw)


def sound(a: np.ndarray, **kw) -> bytes:
    """deflate_file, with PIL reading the file back equal to the source first"""
    data = deflate_file(a, **kw)
    want = a if a.ndim == 2 else np.asarray(Image.fromarray(a).convert("I"))
    assert np.array_equal(pil_array(data), want), kw
    return data


def load(dev, files, **kw):
    return tc.load(dev, files, deflate=True, **kw)


def same_as_pil(dev, files, **kw):
    got, stack = tc.same_as_pil(dev, files, deflate=True, **kw)
    assert stack.status.cpu().tolist() == [0] * len(files)
    return got, stack


# ---- 1: sound files ---------------------------------------------------------------------------------------------------------
def check_pil_written(dev, name, predictor):
    """ridge() 160 x 257 uint16 in three strip layouts: PIL's default strips (the first is as many rows as fit 64 KiB: twice
    the 32 KiB ring), ONE strip of 82 240 bytes (beyond 64 KiB), and 7 rows a strip = 3 598 bytes (below the 4 KiB flush), whose
    destinations fall on many alignments modulo 16.  (PIL's libtiff writes Compression 8 under both names; the hand-written
    files carry 32946.)"""
    a = ridge()
    default = pil_file(a, name, predictor=predictor)
    info = tiff.read_tiff(default)
    assert info.compression in PIL_NAMES.values() and info.predictor == predictor
    assert 32768 < info.strips[0][3] * 257 * 2 <= 65536 and len(info.strips) == 2
    one = pil_file(a, name, predictor=predictor, rows_per_strip=160)
    assert [s[3] * 257 * 2 for s in tiff.read_tiff(one).strips] == [82240]
    many = pil_file(a, name, predictor=predictor, rows_per_strip=7)
    strips = tiff.read_tiff(many).strips
    assert len(strips) == 23 and strips[0][3] * 257 * 2 == 3598
    assert len({(r0 * 257 * 2) % 16 for _, _, r0, _ in strips}) == 8
    assert all(many[o:o + 2] == b"\x78\x9c" for o, _, _, _ in strips)
    got, _ = same_as_pil(dev, [default, one, many])
    assert got.dtype == np.uint16


def check_shape(dev, rows, cols):
    """odd row_bytes, strips shorter than a dword, destinations at every alignment: the inflate's byte-store flush"""
    rng = np.random.default_rng(rows * 1000 + cols)
    files = []
    for dtype in (np.uint8, np.uint16):
        smooth = (rng.integers(0, 3, (rows, cols)).cumsum(axis=1) * 97 + 65000).astype(dtype)     # (wraps: the predictor's modulus)
        for a in (smooth, rng.integers(0, np.iinfo(dtype).max, (rows, cols)).astype(dtype)):
            mine = [pil_file(a, "tiff_adobe_deflate", rows_per_strip=1), pil_file(a, "tiff_deflate", predictor=2, rows_per_strip=2),
                    sound(a, order=">", predictor=2, rows_per_strip=1, shift=1)]
            assert len(tiff.read_tiff(mine[0]).strips) == rows
            same_as_pil(dev, mine)
            files.append(mine)
    for f in files[0] + files[2]:                                                  # (one at a time: the smallest stacks)
        same_as_pil(dev, [f])


def check_hand_written(dev):
    a = ridge(50, (20, 37))
    files = [sound(a, compression=c, order=o, predictor=p, rows_per_strip=7)
             for c in (8, 32946) for o in ("<", ">") for p in (1, 2)]
    infos = [tiff.read_tiff(f) for f in files]
    assert {(x.compression, x.byte_order, x.predictor) for x in infos} == {(c, o, p) for c in (8, 32946) for o in ("II", "MM") for p in (1, 2)}
    same_as_pil(dev, files)
    for f in files[:2]:
        same_as_pil(dev, [f])


def check_encoder_settings(dev):
    """stored blocks (level 0), fixed codes, literal-only dynamic codes, run-length matches, small and full windows"""
    a = ridge(51, (48, 150))
    settings = [dict(level=0), dict(level=1), dict(level=6), dict(level=9), dict(strategy=zlib.Z_FIXED), dict(strategy=zlib.Z_HUFFMAN_ONLY),
                dict(strategy=zlib.Z_RLE), dict(wbits=9), dict(wbits=15, level=9)]
    files = [sound(a, pack=packer(**kw), predictor=1 + k % 2, rows_per_strip=16) for k, kw in enumerate(settings)]
    o, n, _, _ = tiff.read_tiff(files[0]).strips[0]
    assert files[0][o + 2] & 6 == 0 and n > 16 * 300                               # level 0: block type 0, nothing saved
    o = tiff.read_tiff(files[4]).strips[0][0]
    assert files[4][o + 2] & 6 == 2                                                # Z_FIXED: block type 1
    o = tiff.read_tiff(files[7]).strips[0][0]
    assert files[7][o] >> 4 == 1                                                   # wbits 9: CINFO 1
    same_as_pil(dev, files)


def far_match_stream(raw: bytes) -> bytes:
    """a zlib stream of `raw` (whose bytes from 32 768 on repeat the bytes 32 768 before them): the first 32 768 bytes as a
    stored block, the rest as length-258 matches at distance 32 768 with the fixed codes -- zlib's own encoder never looks
    further back than 32 506 bytes"""
    assert len(raw) > 32768 and raw[32768:] == raw[:len(raw) - 32768]
    out, acc, n = bytearray(b"\x78\x01"), 0, 0

    def put(v, bits):
        nonlocal acc, n
        acc |= v << n
        n += bits
        while n >= 8:
            out.append(acc & 255)
            acc >>= 8
            n -= 8

    def code(c, bits):                                                             # Huffman codes go first bit first
        put(int(format(c, f"0{bits}b")[::-1], 2), bits)

    put(0, 3)                                                                      # BFINAL 0, BTYPE 0
    put(0, (8 - n) % 8)
    put(32768, 16), put(32768 ^ 0xFFFF, 16)
    out += raw[:32768]
    put(1, 1), put(1, 2)                                                           # BFINAL 1, BTYPE 1
    left = len(raw) - 32768
    while left:
        length = min(left, 258)
        assert length == 258 or 3 <= length <= 10
        if length == 258:
            code(0b11000000 + 285 - 280, 8)
        else:
            code(length - 3 + 1, 7)                                                # symbols 257 .. 264: lengths 3 .. 10, no extra bits
        code(29, 5), put(32768 - 24577, 13)
        left -= length
    code(0, 7)                                                                     # end of block
    put(0, (8 - n) % 8)
    z = bytes(out) + zlib.adler32(raw).to_bytes(4, "big")
    assert zlib.decompress(z) == raw
    return z


def check_content(dev):
    flat = np.full((tc.H, tc.W), 513, dtype=np.uint16)
    f = sound(flat, pack=packer(9), rows_per_strip=64)
    assert flat.nbytes > 200 * len(f)                                              # length-258 matches at distance 1 or 2
    same_as_pil(dev, [f])
    same_as_pil(dev, [sound(np.full((70, 200), 9, dtype=np.uint8), pack=packer(9))])   # ... at distance 1
    noise = np.random.default_rng(7).integers(0, 65536, (96, 130)).astype(np.uint16)
    g = pil_file(noise, "tiff_adobe_deflate", rows_per_strip=32)
    assert sum(s[1] for s in tiff.read_tiff(g).strips) > noise.nbytes              # grows under Deflate
    same_as_pil(dev, [g])
    # ONE strip of 12 rows of 8 192 bytes whose rows k and k + 4 are the same random row: matches at distance exactly 32 768
    base = np.random.default_rng(8).integers(0, 65536, (4, 4096)).astype(np.uint16)
    far = np.concatenate([base, base, base])
    h = sound(far, pack=far_match_stream)
    assert len(tiff.read_tiff(h).strips) == 1 and tiff.read_tiff(h).strips[0][1] < 32768 + 1200
    same_as_pil(dev, [h])


def check_uint8_and_rgb(dev):
    a8 = (ridge(52, (33, 131)) >> 8).astype(np.uint8)
    got, _ = same_as_pil(dev, [pil_file(a8, "tiff_adobe_deflate", predictor=2, rows_per_strip=8), sound(a8, compression=32946, rows_per_strip=5)])
    assert got.dtype == np.uint8
    rng = np.random.default_rng(5)
    rgb = np.clip(rng.integers(0, 40, (33, 131, 3)) + np.linspace(0, 215, 131)[None, :, None], 0, 255).astype(np.uint8)
    files = [pil_file(rgb, "tiff_adobe_deflate", predictor=2, rows_per_strip=8), pil_file(rgb, "tiff_deflate"),
             sound(rgb, order=">", predictor=2, rows_per_strip=5)]
    got, _ = same_as_pil(dev, files)
    assert got.dtype == np.int32 and np.array_equal(got[0], np.asarray(Image.fromarray(rgb).convert("I")))
    assert np.array_equal(load(dev, files[:2], dtype=np.float64)[0], got[:2].astype(np.float64))


def check_mixed_stack(dev):
    a = [ridge(60 + k, (48, 150)) for k in range(5)]
    files = [pil_file(a[0]), pil_file(a[1], "packbits", rows_per_strip=10), pil_file(a[2], "tiff_lzw", predictor=2, rows_per_strip=16),
             pil_file(a[3], "tiff_adobe_deflate", predictor=2, rows_per_strip=9), sound(a[4], order=">", compression=32946, rows_per_strip=11, shift=1)]
    got, stack = same_as_pil(dev, files)
    assert [x.compression for x in stack.images] == [1, 32773, 5, 8, 32946] and stack.images[4].byte_order == "MM"
    assert np.array_equal(got, np.stack(a))
    aba = [files[3], files[4], files[3]]
    got3, _ = same_as_pil(dev, aba)
    assert np.array_equal(got3, np.stack([a[3], a[4], a[3]]))
    for dt in (np.float64, np.uint16):
        conv, _ = load(dev, files, dtype=dt)
        assert conv.dtype == dt and np.array_equal(conv, np.stack(a).astype(dt))
    # the derived mask of decode_tiff_strips maps descriptors 8 and 32946 to bit 8
    buf, off, ln, desc, flags = strip_table(files)
    frames, status = tiff.decode_tiff_strips(buf, off, ln, desc, flags, width=150, height=48, bits=16, device=dev)
    assert status.cpu().tolist() == [0] * 5 and np.array_equal(to_np(frames), np.stack(a))


# ---- 2: what libtiff accepts ------------------------------------------------------------------------------------------------
ODD_SHAPE = (20, 37)                                                               # strips of 7 rows: 7, 7, 6


def check_accepted_oddities(dev):
    a = ridge(70, ODD_SHAPE)
    more = ridge(71, (9, 37))

    def longer(k, z, raw):                                                         # the stream yields two rows more than the strip holds
        return zlib.compress(raw + more[:2].tobytes()) if k == 1 else z

    files = [deflate_file(a, rows_per_strip=7, damage=lambda k, z, raw: z + b"\x00\x01junk\xff" if k == 1 else z),
             deflate_file(a, rows_per_strip=7, predictor=2, damage=lambda k, z, raw: z[:-4] if k == 1 else z),
             deflate_file(a, rows_per_strip=7, order=">", damage=longer),
             deflate_file(a, rows_per_strip=7, pack=packer(0), damage=lambda k, z, raw: z[:-4])]
    got, stack = load(dev, files)                                                  # check=True: nothing is raised
    assert stack.status.cpu().tolist() == [0] * 4
    for k in range(4):
        assert np.array_equal(got[k], a), k


# ---- 3: damaged files -------------------------------------------------------------------------------------------------------
def damaged_files():
    """-> (sources, files, expected status): sound files at 0, 3 and 7, one damaged file per row of the table"""
    a = [ridge(80 + k, ODD_SHAPE) for k in range(11)]
    row = 37 * 2

    def only(strip, f):
        return lambda k, z, raw: f(z, raw) if k == strip else z

    def stored_flip(z, raw):                                                       # inside a level-0 stored block: only the checksum notices
        assert z[2] == 1 and len(z) == len(raw) + 11
        return z[:40] + bytes([z[40] ^ 0x10]) + z[41:]

    cases = [
        (None, 0, {}),
        (only(1, lambda z, raw: z[:-1] + bytes([z[-1] ^ 1])), tiff.STATUS_ADLER, {}),
        (only(1, lambda z, raw: z[:len(z) // 2]), tiff.STATUS_SHORT, {}),
        (None, 0, dict(predictor=2, order=">")),
        (only(1, lambda z, raw: zlib.compress(raw[:6 * row])), tiff.STATUS_SHORT, {}),
        (only(0, lambda z, raw: z[:2] + b"\x07" + z[3:]), tiff.STATUS_CORRUPT_DEFLATE, {}),
        (only(2, lambda z, raw: b"\x79" + z[1:]), tiff.STATUS_CORRUPT_DEFLATE, {}),
        (None, 0, dict(compression=32946)),
        (only(1, lambda z, raw: z[2:-4]), tiff.STATUS_CORRUPT_DEFLATE, {}),
        (only(1, stored_flip), tiff.STATUS_ADLER, dict(pack=packer(0))),
        (only(1, lambda z, raw: b"\x78\x20" + z[2:]), tiff.STATUS_CORRUPT_DEFLATE, {}),
    ]
    files, want = [], []
    for k, (damage, status, kw) in enumerate(cases):
        f = deflate_file(a[k], rows_per_strip=7, damage=damage, **kw)
        if status:
            with pytest.raises(OSError):
                pil_array(f)
        else:
            assert np.array_equal(pil_array(f), a[k])
        files.append(f), want.append(status)
    assert (0x7820 % 31, 0x20 & 0x20) == (0, 0x20)                                 # a valid header check with FDICT set
    return a, files, want


def check_damage(dev, monkeypatch):
    a, files, want = damaged_files()
    stack = tiff.load_frames(files, device=dev, check=False, deflate=True)
    assert stack.status.cpu().tolist() == want
    got = to_np(stack.frames)
    for k, w in enumerate(want):
        if w == 0:
            assert np.array_equal(got[k], a[k]), k
    assert np.array_equal(got[5][7:], a[5][7:]) and np.array_equal(got[2][:7], a[2][:7])      # the sound strips of a flagged frame
    with pytest.raises(OSError, match=r"file 1: the Adler-32 of a strip differs"):
        tiff.load_frames(files, device=dev, deflate=True)
    with pytest.raises(OSError, match=r"file 2: corrupt Deflate data"):
        tiff.load_frames([files[0], files[3], files[5]], device=dev, deflate=True)
    with pytest.raises(OSError, match=r"file 1: a strip decodes to fewer bytes"):
        tiff.load_frames([files[0], files[4]], device=dev, deflate=True)
    with pytest.raises(OSError, match=r"file 0: corrupt Deflate data"):
        tiff.load_frames([files[10]], device=dev, deflate=True)
    # check=False transfers nothing back: no tensor of the call is copied to the host
    calls = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *x, **k: (calls.append(self.data_ptr()), real(self, *x, **k))[1])
    stack = tiff.load_frames(files, device=dev, check=False, deflate=True)
    assert not calls
    stack = tiff.load_frames([files[0], files[7]], device=dev, check=True, deflate=True)
    assert set(calls) == {stack.status.data_ptr()}                                 # check=True: the status, and nothing else
    monkeypatch.undo()


def check_window_outside_the_buffer(dev):
    a = [ridge(90 + k, (24, 100)) for k in range(3)]
    files = [pil_file(a[0], "tiff_adobe_deflate", rows_per_strip=8), pil_file(a[1], "tiff_lzw", rows_per_strip=8),
             sound(a[2], compression=32946, order=">", predictor=2, rows_per_strip=8)]
    buf, off, ln, desc, flags = strip_table(files)
    assert len(off) == 9
    kw = dict(width=100, height=24, bits=16, device=dev, max_strip_bytes=int(ln.max()))
    cases = {(1, "off", -1): 0, (0, "off", len(buf) - 3): 0, (2, "len", 1 << 40): 0, (7, "len", -5): 2, (6, "off", 1 << 50): 2,
             (8, "off", len(buf)): 2, (8, "len", int(ln.max()) + 1): 2, (2, "row", 20): 0, (6, "row", -1): 2, (1, "comp", 7): 0,
             (4, "len", -1): 1}
    for (s, what, value), frame in cases.items():
        o2, l2, d2 = off.copy(), ln.copy(), desc.copy()
        if what == "off":
            o2[s] = value
        elif what == "len":
            l2[s] = value
        else:
            d2[s, 1 if what == "row" else 3] = value
        out = torch.from_numpy(np.full((3, 24, 100), 0x5A5A, dtype=np.uint16).view(np.int16)).view(torch.uint16).to(dev)
        frames, status = tiff.decode_tiff_strips(buf, o2, l2, d2, flags, out=out, compressions=15, **kw)
        assert status.cpu().tolist() == [int(k == frame) for k in range(3)], (s, what)
        got = to_np(frames)
        for k in range(3):
            assert np.array_equal(got[k], a[k]) if k != frame else (got[k] == 0x5A5A).all(), (s, what, k)
    # under a mask without bit 8 a Deflate strip is a strip of a compression outside the mask
    frames, status = tiff.decode_tiff_strips(buf, off, ln, desc, flags, compressions=7, **kw)
    assert status.cpu().tolist() == [1, 0, 1] and np.array_equal(to_np(frames)[1], a[1])


# ---- 4: refusals, the C ABI -------------------------------------------------------------------------------------------------
def check_refusals(dev):
    a = ridge(40, (16, 40))
    a8 = (a >> 8).astype(np.uint8)
    good = pil_file(a, "tiff_adobe_deflate")
    cases = [
        (deflate_file(a, tags=[(322, 3, [16]), (323, 3, [16])]), "tiled"),
        (pil_file(a8, "jpeg"), "Compression 7 "),
        (deflate_file(a, tags=[(317, 3, [3])]), "Predictor 3"),
        (write_tiff(a, predictor=2), "Predictor 2 with Compression 1"),
        (write_tiff(a, compression=32773, predictor=2), "Predictor 2 with Compression 32773"),
    ]
    for data, text in cases:
        with pytest.raises(ValueError, match=r"file 1: .*(" + text + ")"):
            tiff.load_frames([good, data], device=dev, deflate=True)
    for data in (good, pil_file(a, "tiff_deflate")):
        with pytest.raises(ValueError, match=r"file 1: .*Compression (8|32946) "):
            tiff.load_frames([pil_file(a), data], device=dev)
        with pytest.raises(ValueError, match=r"file 0: .*Compression (8|32946) "):
            tiff.load_frames([data], device=dev, deflate=False)


def check_c_abi_argument_checks(dev):
    """pl_tiff_decode_ex: the argument checks of pl_tiff_decode with masks 1 .. 15 (the pointers below are never dereferenced
    by a refused call); pl_tiff_decode goes on refusing mask 8"""
    from pylinac_amd import _lib

    lib = _lib.load()
    buf = torch.zeros(256, dtype=torch.uint8, device=dev)
    idx = torch.zeros(8, dtype=torch.int64, device=dev)
    st = torch.zeros(4, dtype=torch.int32, device=dev)
    p, q, s = buf.data_ptr(), idx.data_ptr(), st.data_ptr()

    def call(n=1, n_strips=1, bits=16, spp=1, mask=8, kind=0, bytes_=p, out=p, work=p, flags=s, w=4, h=4, max_strip=64, fn=lib.pl_tiff_decode_ex):
        return fn(bytes_, 256, q, q, s, n_strips, max_strip, flags, n, w, h, bits, spp, mask, out, kind, s, work, None)

    for bits, spp in ((12, 1), (1, 1), (4, 1), (32, 1), (16, 3), (8, 4), (8, 2)):
        assert call(bits=bits, spp=spp) == 2 and b"pl_tiff_decode_ex: unsupported samples" in lib.pl_last_error()
        assert lib.pl_tiff_work_bytes_ex(1, 1, 64, 4, 4, bits, spp, 8) == -1
    assert call(mask=0) == 1 and call(mask=16) == 1 and b"8 (Deflate)" in lib.pl_last_error()
    for mask in (8, 15):                                                           # these pass the mask check: the NEXT check refuses
        assert call(mask=mask, kind=3) == 1 and b"out_kind" in lib.pl_last_error()
        assert lib.pl_tiff_work_bytes_ex(1, 1, 64, 4, 4, 16, 1, mask) > 0
    assert call(n=0) == 1 and call(n=65536) == 1 and call(n_strips=0) == 1 and call(w=0) == 1 and call(h=0) == 1
    assert call(bytes_=None) == 1 and call(out=None) == 1 and call(work=None) == 1 and call(flags=None) == 1
    assert call(kind=-1) == 1 and call(max_strip=-1) == 1
    assert call(bytes_=p + 1) == 1 and b"4-byte" in lib.pl_last_error()
    assert call(work=p + 4) == 1 and b"16-byte" in lib.pl_last_error()
    assert call(n_strips=65536, mask=10) == 1                                      # PackBits: the stream is a grid axis
    assert call(mask=8, fn=lib.pl_tiff_decode) == 1 and b"pl_tiff_decode: " in lib.pl_last_error()
    assert lib.pl_tiff_work_bytes(3, 9, 64, 100, 24, 16, 1, 8) == -1 and lib.pl_tiff_work_bytes_ex(3, 9, 64, 100, 24, 16, 1, 16) == -1
    assert lib.pl_tiff_work_bytes_ex(3, 9, 64, 100, 24, 16, 1, 7) == lib.pl_tiff_work_bytes(3, 9, 64, 100, 24, 16, 1, 7)
    assert lib.pl_tiff_work_bytes_ex(3, 9, 64, 100, 24, 16, 1, 15) > lib.pl_tiff_work_bytes(3, 9, 64, 100, 24, 16, 1, 7)
    assert lib.pl_tiff_work_bytes_ex(1, 1, 64, 32768, 32768, 8, 1, 8) == -1        # a frame above 65535 x 16 KiB: the Adler tiles
    assert lib.pl_tiff_work_bytes_ex(1, 1, 64, 32768, 32768, 8, 1, 7) > 0
    header = (Path(__file__).resolve().parent.parent / "include" / "pylinac_hip.h").read_text()
    assert re.search(r"int pl_tiff_decode_ex\(", header) and re.search(r"int64_t pl_tiff_work_bytes_ex\(", header)
