"""Shared checks of the checked Deflate path: pl_adler32 (zipstack.adler32), pl_inflate_checked (png.inflate(verify=True)) and
pl_png_decode_checked (png.load_frames(verify=True)) -- tests/test_emulated_verify.py on the CPU emulator,
tests/test_gpu_verify.py on the MI355X.  Every comparison is EQUALITY: ``adler32`` against ``zlib.adler32``, the checked
inflate against ``zlib.decompress`` / ``decompressobj`` (their output, their ``unused_data``, and which streams they refuse),
PNG frames against ``np.asarray(PIL.Image.open(f))``; a damaged file's status is asserted next to what PIL does with the same
bytes.  The PNG files are written by PIL; damage is made by patching bytes.  A stream's output stays below about 100 KiB (the
emulator runs a fiber per work-item)."""
from __future__ import annotations

import re
import struct
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

import png_checks as pc
from pylinac_amd import dicom, png, zipstack

to_np = dicom._to_numpy
TILE = 16384
ADLER_LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 256, 257, 258, 5551, 5552, 5553, TILE - 1, TILE, TILE + 1, 2 * TILE + 17, 3 * TILE]


def u32(t: torch.Tensor) -> list:
    return [int(v) & 0xFFFFFFFF for v in t.cpu().view(torch.int32).tolist()]


# ---- 1: pl_adler32 against zlib.adler32 -----------------------------------------------------------------------------------
def adler_layout(fill):
    """every length of ADLER_LENGTHS at source offsets 0, 1, 2 and 3 mod 4; the gaps between the ranges (and both ends of the
    buffer) hold 0xA5 bytes, which belong to no range -> (buffer, offsets, lengths)"""
    total = sum(ADLER_LENGTHS) * 4 + 16 * len(ADLER_LENGTHS) * 4 + 64
    buf = np.full(total, 0xA5, dtype=np.uint8)
    off, ln, pos = [], [], 5
    for n in ADLER_LENGTHS:
        for a in range(4):
            pos += (a - pos) % 4 + 4                                               # a gap, then the alignment wanted
            off.append(pos), ln.append(n)
            buf[pos:pos + n] = fill(n)
            pos += n
    assert pos < total and {o % 4 for o in off} == {0, 1, 2, 3}
    return buf, off, ln


def check_adler_random(dev):
    rng = np.random.default_rng(61)
    buf, off, ln = adler_layout(lambda n: rng.integers(0, 256, n, dtype=np.uint8))
    adler, status = zipstack.adler32(buf, off, ln, device=dev)
    want = [zlib.adler32(buf[o:o + n].tobytes()) for o, n in zip(off, ln)]
    assert status.cpu().tolist() == [0] * len(off)
    got = u32(adler)
    assert got == want, [(o, n) for o, n, g, w in zip(off, ln, got, want) if g != w]
    # device tensors are used in place
    some = slice(40, 52)
    adler2, _ = zipstack.adler32(torch.from_numpy(buf).to(dev), torch.tensor(off[some]).to(dev), torch.tensor(ln[some]).to(dev), device=dev)
    assert u32(adler2) == want[some]


def check_adler_constant(dev, value):
    """all 0xFF: the largest sums there are -- A crosses 65521 for the first time at 257 bytes, and the weighted sum of a tile
    (3.4e10) overflows 32 bits; all 0x00: A stays 1 and B = n mod 65521, which fails if a tile is given its own "1" or the
    fold forgets the len2 x (A1 - 1) term"""
    buf, off, ln = adler_layout(lambda n: np.full(n, value, dtype=np.uint8))
    adler, status = zipstack.adler32(buf, off, ln, device=dev)
    want = [zlib.adler32(bytes([value]) * n) for n in ln]
    assert status.cpu().tolist() == [0] * len(off)
    got = u32(adler)
    assert got == want, [(o, n, hex(g), hex(w)) for o, n, g, w in zip(off, ln, got, want) if g != w]
    if value == 0:
        assert want == [((n % 65521) << 16) | 1 for n in ln]
    else:
        assert 255 * 256 < 65521 < 255 * 257 and 255 * TILE * (TILE + 1) // 2 > 1 << 32


def check_adler_edges(dev):
    rng = np.random.default_rng(62)
    buf = rng.integers(0, 256, TILE + 39, dtype=np.uint8)                          # (the buffer's size: odd, no multiple of 4)
    n = len(buf)
    # ranges ending at the buffer's last byte at odd lengths, the whole buffer, an empty range at its end
    off = [n - 1, n - 7, n - 33, 3, 0, n]
    ln = [1, 7, 33, n - 3, n, 0]
    adler, status = zipstack.adler32(buf, off, ln, device=dev)
    assert status.cpu().tolist() == [0] * 6
    assert u32(adler) == [zlib.adler32(buf[o:o + m].tobytes()) for o, m in zip(off, ln)]
    # windows outside the buffer: status 1, the word keeps its sentinel; the neighbours are computed
    off = [0, n - 4, -1, 5, n + 1, 7, 9]
    ln = [10, 5, 4, -2, 0, 1 << 40, 3]
    out = torch.from_numpy(np.full(7, 0x5A5A5A5A, dtype=np.int32)).view(torch.uint32).to(dev)
    adler, status = zipstack.adler32(buf, off, ln, device=dev, out=out)
    assert status.cpu().tolist() == [0, 1, 1, 1, 1, 1, 0]
    assert u32(adler) == [zlib.adler32(buf[:10].tobytes())] + [0x5A5A5A5A] * 5 + [zlib.adler32(buf[9:12].tobytes())]


# ---- 2: pl_inflate_checked against zlib.decompress / decompressobj ---------------------------------------------------------
_PAYLOADS = None


def payloads():
    """name -> (payload, zlib level); the 70 000 bytes of text go beyond the 32 KiB ring and beyond two tiles of the Adler
    kernel, and levels 1 / 6 / 9 give fixed and dynamic blocks, level 0 stored ones"""
    global _PAYLOADS
    if _PAYLOADS is None:
        text = b"".join(b"leaf %d picket %d offset %.3f mm; " % (k % 60, k % 10, (k * 37 % 100) / 250) for k in range(3000))[:70000]
        assert len(text) == 70000
        _PAYLOADS = {"empty": (b"", 6), "one_byte": (b"Q", 6), "text_level1": (text, 1), "text_level6": (text, 6),
                     "text_level9": (text[::-1], 9), "text_stored": (text, 0), "short_stored": (text[:3000], 0)}
        types = {name: pc.inflate_trace(zlib.compress(p, lv)[2:-4])[1]["types"] for name, (p, lv) in _PAYLOADS.items()}
        assert types["text_stored"] == {0} and types["short_stored"] == {0} and 2 in types["text_level6"] | types["text_level9"]
        assert 1 in set().union(*types.values())
    return _PAYLOADS


def stream(name: str) -> tuple:
    p, level = payloads()[name]
    return zlib.compress(p, level), p


def run_checked(dev, streams, caps, shift=1):
    """streams laid one after the other behind `shift` foreign bytes (odd offsets), foreign bytes after the last one too"""
    buf, off = bytearray(b"\xAA" * shift), []
    for s in streams:
        off.append(len(buf))
        buf += s
    buf += b"\xAA" * 7
    out, out_len, status, in_used = png.inflate(np.frombuffer(bytes(buf), dtype=np.uint8), off, [len(s) for s in streams], caps,
                                                device=dev, verify=True)
    room = (np.clip(np.asarray(caps, dtype=np.int64), 0, None) + 15) & ~15
    oo = np.concatenate([[0], np.cumsum(room)[:-1]])
    flat = to_np(out)
    return ([flat[o:o + n].tobytes() for o, n in zip(oo, out_len.cpu().tolist())], status.cpu().tolist(), in_used.cpu().tolist())


def zlib_verdict(data: bytes):
    """what zlib makes of the bytes: (output, bytes used) or the error's number"""
    d = zlib.decompressobj()
    try:
        out = d.decompress(data)
    except zlib.error as e:
        return int(re.search(r"Error (-\d)", str(e)).group(1))
    if not d.eof:
        return -5                                                                  # what zlib.decompress raises for it
    return out, len(data) - len(d.unused_data)


def check_inflate_sound(dev):
    names = list(payloads())
    zs = [stream(n) for n in names]
    for tail in (b"", b"xyz"):                                                     # bytes after the trailer are ignored
        data = [z + tail for z, _ in zs]
        for d, (z, p) in zip(data, zs):
            assert zlib_verdict(d) == (p, len(z))
        got, status, used = run_checked(dev, data, [len(p) for _, p in zs], shift=1 + len(tail))
        assert status == [0] * len(names), dict(zip(names, status))
        assert used == [len(z) for z, _ in zs]
        for n, g, (_, p) in zip(names, got, zs):
            assert g == p, n


def check_inflate_trailer_flipped(dev):
    names = list(payloads())
    zs = [stream(n) for n in names]
    bad = [z[:-1] + bytes([z[-1] ^ 0x40]) for z, _ in zs]
    for b in bad:
        assert zlib_verdict(b) == -3
    got, status, used = run_checked(dev, bad, [len(p) for _, p in zs])
    assert status == [png.INFLATE_ADLER] * len(names), dict(zip(names, status))
    assert used == [len(z) for z, _ in zs]
    for n, g, (_, p) in zip(names, got, zs):
        assert g == p, n                                                           # the output is stored all the same


def check_inflate_stored_byte_flipped(dev):
    """a payload byte flipped inside a stored block: the Deflate layer cannot notice it, only the checksum does.  pl_inflate
    (verify=False) returns status 0 for it: the baseline this pull request leaves in place"""
    for name in ("short_stored", "text_stored"):
        z, p = stream(name)
        at = 2 + 5 + len(p) // 3                                                   # zlib header, the block's header and LEN / NLEN
        assert z[at] == p[len(p) // 3]
        bad = z[:at] + bytes([z[at] ^ 0x04]) + z[at + 1:]
        assert zlib_verdict(bad) == -3
        with pytest.raises(zlib.error, match="incorrect data check"):
            zlib.decompress(bad)
        want = p[:len(p) // 3] + bytes([p[len(p) // 3] ^ 0x04]) + p[len(p) // 3 + 1:]
        got, status, used = run_checked(dev, [bad], [len(p)], shift=3)
        assert status == [png.INFLATE_ADLER] and got[0] == want and used == [len(z)], (name, status)
        out, _, out_len, st0 = png.inflate(np.frombuffer(bad, dtype=np.uint8), [0], [len(bad)], [len(p)], device=dev)
        assert st0.cpu().tolist() == [0] and to_np(out)[:len(p)].tobytes() == want  # verify=False: as before


def check_inflate_trailer_cut(dev):
    names = ["empty", "one_byte", "text_level6", "short_stored"]
    for cut in (1, 2, 3, 4):
        zs = [stream(n) for n in names]
        data = [z[:-cut] for z, _ in zs]
        for d in data:
            assert zlib_verdict(d) == -5
        got, status, used = run_checked(dev, data, [len(p) for _, p in zs], shift=cut)
        assert all(s & png.STATUS_SHORT and not s & (png.INFLATE_ADLER | png.INFLATE_OVERFLOW | 4 | 1) for s in status), (cut, status)
        for g, (_, p) in zip(got, zs):
            assert g == p
    # ... and a stream cut inside its last block, whose output is complete by then: zlib says incomplete, and so does this
    z, p = stream("short_stored")
    assert zlib_verdict(z[:-5]) == -5
    _, status, _ = run_checked(dev, [z[:-5]], [len(p) - 1])
    assert status[0] & png.STATUS_SHORT


def check_inflate_capacity(dev):
    names = ["one_byte", "text_level6", "text_level9", "short_stored"]
    zs = [stream(n) for n in names]
    below = [len(p) - 1 for _, p in zs]
    got, status, _ = run_checked(dev, [z for z, _ in zs], below)
    assert status == [png.INFLATE_OVERFLOW] * len(names), status
    for g, c, (_, p) in zip(got, below, zs):
        assert len(g) == c and g == p[:c]
    above = [len(p) + 1 for _, p in zs]
    got, status, used = run_checked(dev, [z for z, _ in zs], above)
    assert status == [png.STATUS_SHORT] * len(names), status
    assert used == [len(z) for z, _ in zs]
    for g, (_, p) in zip(got, zs):
        assert g == p


def check_inflate_one_damaged_among_several(dev):
    names = ["text_level1", "one_byte", "short_stored", "empty", "text_level6"]
    zs = [stream(n) for n in names]
    data = [z for z, _ in zs]
    z, p = zs[2]
    data[2] = z[:500] + bytes([z[500] ^ 1]) + z[501:]
    assert zlib_verdict(data[2]) == -3
    got, status, used = run_checked(dev, data, [len(p) for _, p in zs])
    assert status == [0, 0, png.INFLATE_ADLER, 0, 0]
    for k in (0, 1, 3, 4):
        assert got[k] == zs[k][1] and used[k] == len(zs[k][0])
    with pytest.raises(ValueError, match="verify=True needs wrapper=True"):
        png.inflate(np.zeros(8, dtype=np.uint8), [0], [8], [8], wrapper=False, verify=True, device=dev)


# ---- 3: png.load_frames(verify=True) against PIL ---------------------------------------------------------------------------
def pil_refuses(data: bytes):
    with pytest.raises(OSError):                                                   # (UnidentifiedImageError is an OSError)
        pc.pil_array(data)


def rechunked(data: bytes, parts: int = 3) -> bytes:
    """the file with its zlib stream cut into `parts` IDAT chunks of about equal size"""
    info = png.read_png(data)
    z = pc.zlib_stream(data)
    cuts = [len(z) * k // parts for k in range(parts + 1)]
    first = info.idat[0][0] - 8
    out = data[:first] + b"".join(pc.chunk(b"IDAT", z[a:b]) for a, b in zip(cuts[:-1], cuts[1:])) + pc.chunk(b"IEND", b"")
    assert len(png.read_png(out).idat) == parts
    return out


def flip(data: bytes, at: int, bit: int = 1) -> bytes:
    return data[:at] + bytes([data[at] ^ bit]) + data[at + 1:]


def bad_ihdr_crc(data: bytes) -> bytes:
    return flip(data, 8 + 8 + 13 + 3)


def bad_text_chunk(data: bytes) -> bytes:
    first = png.read_png(data).idat[0][0] - 8
    text = pc.chunk(b"tEXt", b"Comment\0scanned 2026-10-19")
    return data[:first] + flip(text, len(text) - 2, 0x10) + data[first:]


def bad_idat_crc(data: bytes, which: int = 1) -> bytes:
    o, c = png.read_png(data).idat[which]
    return flip(data, o + c + 1, 0x08)


def bad_adler(data: bytes) -> bytes:
    """the stream's last byte flipped, the chunk's CRC repaired"""
    o, c = png.read_png(data).idat[-1]
    assert c >= 1
    payload = data[o:o + c - 1] + bytes([data[o + c - 1] ^ 0x20])
    return data[:o - 8] + pc.chunk(b"IDAT", payload) + data[o + c + 4:]


_PNG = None


def png_files():
    """(frames, files): 40 x 33 grey of 16 bits and RGB of 8 bits, written by PIL; file 2 of each kind re-chunked into three
    IDAT chunks"""
    global _PNG
    if _PNG is None:
        grey = [pc.ridge(70 + k, (33, 40)) for k in range(3)]
        rgb = [pc.rgb_frame(80 + k, (33, 40)) for k in range(3)]
        out = {}
        for kind, frames in (("grey16", grey), ("rgb8", rgb)):
            files = [pc.pil_file(a) for a in frames]
            files[2] = rechunked(files[2])
            for f, a in zip(files, frames):
                assert np.array_equal(pc.pil_array(f), pc.expected(a))
            out[kind] = (frames, files)
        _PNG = out
    return _PNG


def statuses(dev, files, **kw):
    stack = png.load_frames(files, device=dev, check=False, **kw)
    return stack.status.cpu().tolist(), to_np(stack.frames)


def check_png_sound(dev, kind):
    frames, files = png_files()[kind]
    st, got = statuses(dev, files, verify=True)
    assert st == [0, 0, 0]
    for k, f in enumerate(files):
        assert np.array_equal(got[k], pc.pil_array(f)) and np.array_equal(got[k], pc.expected(frames[k]))
    st0, got0 = statuses(dev, files)
    assert st0 == [0, 0, 0] and np.array_equal(got0, got)


def damaged(kind):
    """name -> (file, status with verify=True, whether PIL refuses it); every file is the three-IDAT one with ONE damage"""
    frames, files = png_files()[kind]
    base = files[2]
    second = bad_idat_crc(base, 1)
    o, c = png.read_png(base).idat[1]
    stored = struct.unpack(">I", second[o + c:o + c + 4])[0]
    assert stored != zlib.crc32(b"IDAT" + base[o:o + c]) == struct.unpack(">I", base[o + c:o + c + 4])[0]   # the expected verdict,
    return {                                                                                              # from zlib.crc32
        "IHDR CRC": (bad_ihdr_crc(base), png.STATUS_CHUNK_CRC, True),
        "tEXt CRC": (bad_text_chunk(base), png.STATUS_CHUNK_CRC, True),
        "second IDAT CRC": (second, png.STATUS_CHUNK_CRC, False),
        "Adler-32": (bad_adler(base), png.STATUS_ADLER, True),
    }


def check_png_damage(dev, kind):
    frames, files = png_files()[kind]
    want2 = pc.expected(frames[2])
    for name, (bad, flag, refused) in damaged(kind).items():
        if refused:
            pil_refuses(bad)
        else:
            assert np.array_equal(pc.pil_array(bad), want2), name                  # PIL does not verify IDAT CRCs: libpng does
        st, got = statuses(dev, [bad], verify=True)
        assert st == [flag], (name, st)
        assert np.array_equal(got[0], want2), name                                 # the pixels are stored all the same
        st, got = statuses(dev, [bad])                                             # verify=False: as before
        assert st == [0] and np.array_equal(got[0], want2), name
        # a stack with only file 1 damaged
        st, got = statuses(dev, [files[0], bad, files[1]], verify=True)
        assert st == [0, flag, 0], (name, st)
        assert np.array_equal(got[0], pc.pil_array(files[0])) and np.array_equal(got[2], pc.pil_array(files[1])), name


def check_png_raises(dev, monkeypatch):
    frames, files = png_files()["grey16"]
    cases = damaged("grey16")
    texts = {"IHDR CRC": r"file 1: chunk 'IHDR' at byte 8: CRC-32 0x[0-9a-f]{8} computed, 0x[0-9a-f]{8} stored",
             "tEXt CRC": r"file 1: chunk 'tEXt' at byte \d+: CRC-32",
             "second IDAT CRC": r"file 1: chunk 'IDAT' at byte \d+: CRC-32",
             "Adler-32": r"file 1: Adler-32 of the pixel data"}
    for name, text in texts.items():
        with pytest.raises(OSError, match=text):
            png.load_frames([files[0], cases[name][0], files[1]], device=dev, verify=True)
        png.load_frames([files[0], cases[name][0], files[1]], device=dev)           # the default does not look
    # a chunk whose declared length runs past the file stays the ValueError it is
    with pytest.raises(ValueError, match="runs past the end of the file"):
        png.load_frames([files[0][:-20]], device=dev, verify=True)
    # a stream that goes on beyond the frame is no error for a PNG, and its checksum is not judged; a cut trailer is bit 2
    a = frames[0]
    rows = pc.filtered(a, (1,))
    longer = pc.write_png(a, stream=zlib.compress(rows + b"\0" * 9))
    assert np.array_equal(pc.pil_array(longer), a)
    cut = pc.write_png(a, stream=zlib.compress(rows)[:-2])
    st, got = statuses(dev, [longer, cut, files[0]], verify=True)
    assert st == [0, png.STATUS_SHORT, 0] and np.array_equal(got[0], a) and np.array_equal(got[1], a)
    # check=False transfers nothing back
    calls = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *x, **k: (calls.append(self.data_ptr()), real(self, *x, **k))[1])
    png.load_frames(files, device=dev, check=False, verify=True)
    assert not calls
    stack = png.load_frames(files, device=dev, verify=True)
    assert set(calls) == {stack.status.data_ptr()}
    monkeypatch.undo()


# ---- 4: the C ABI ---------------------------------------------------------------------------------------------------------
def check_c_abi_argument_checks(dev):
    """pl_adler32 (the list of pl_crc32's test), pl_inflate_checked, pl_png_decode_checked: invalid argument (1) before any
    launch (the pointers below are never dereferenced); the work sizes: -1 for the same"""
    from pylinac_amd import _lib

    lib = _lib.load()
    buf = torch.zeros(256, dtype=torch.uint8, device=dev)
    idx = torch.zeros(8, dtype=torch.int64, device=dev)
    st = torch.zeros(4, dtype=torch.int32, device=dev)
    p, q, s = buf.data_ptr(), idx.data_ptr(), st.data_ptr()

    def adler(**kw):
        a = dict(bytes_=p, nbytes=256, off=q, len_=q, n=1, max_len=64, adler=s, status=s, work=p)
        a.update(kw)
        return lib.pl_adler32(a["bytes_"], a["nbytes"], a["off"], a["len_"], a["n"], a["max_len"], a["adler"], a["status"], a["work"], None)

    for name in ("bytes_", "off", "len_", "adler", "status", "work"):
        assert adler(**{name: None}) == 1 and b"null pointer" in lib.pl_last_error(), name
    assert adler(n=0) == 1 and adler(n=-1) == 1 and adler(max_len=-1) == 1 and adler(nbytes=-1) == 1 and adler(max_len=65535 * TILE + 1) == 1
    assert adler(bytes_=p + 1) == 1 and b"4-byte" in lib.pl_last_error()
    assert adler(work=p + 4) == 1 and b"8-byte" in lib.pl_last_error()
    assert lib.pl_adler32_work_bytes(0, 64) == -1 and lib.pl_adler32_work_bytes(1, -1) == -1
    assert lib.pl_adler32_work_bytes(3, 0) == 32 and lib.pl_adler32_work_bytes(3, 2 * TILE + 1) == 80 and lib.pl_adler32_work_bytes(1, TILE) == 16

    def inflate(**kw):
        a = dict(bytes_=p, nbytes=256, in_off=q, in_len=q, n=1, out=p, out_off=q, out_cap=q, max_out=64, out_len=q, in_used=q,
                 status=s, work=p)
        a.update(kw)
        return lib.pl_inflate_checked(a["bytes_"], a["nbytes"], a["in_off"], a["in_len"], a["n"], a["out"], a["out_off"], a["out_cap"],
                                      a["max_out"], a["out_len"], a["in_used"], a["status"], a["work"], None)

    for name in ("bytes_", "in_off", "in_len", "out", "out_off", "out_cap", "out_len", "in_used", "status", "work"):
        assert inflate(**{name: None}) == 1 and b"null pointer" in lib.pl_last_error(), name
    assert inflate(n=0) == 1 and inflate(max_out=-1) == 1 and inflate(max_out=65535 * TILE + 1) == 1 and inflate(nbytes=-1) == 1
    assert inflate(bytes_=p + 2) == 1 and inflate(out=p + 1) == 1 and b"4-byte" in lib.pl_last_error()
    assert inflate(work=p + 8) == 1 and b"16-byte" in lib.pl_last_error()
    assert lib.pl_inflate_checked_work_bytes(0, 64) == -1 and lib.pl_inflate_checked_work_bytes(1, -1) == -1
    assert lib.pl_inflate_checked_work_bytes(3, 2 * TILE + 1) == 16 + 16 + 80

    def decode(n=1, n_seg=1, bits=16, spp=1, n_chunks=1, max_chunk=64, table=q, crc=s, work=p):
        return lib.pl_png_decode_checked(p, 256, q, q, s, n_seg, n, 4, 4, bits, spp, p, 0, s, work, table, q, crc, s, n_chunks, max_chunk, None)

    assert decode(bits=12) == 2 and b"unsupported samples" in lib.pl_last_error()
    assert decode(n=0) == 1 and decode(n_seg=0) == 1 and decode(n_chunks=0) == 1 and decode(max_chunk=-1) == 1
    assert decode(table=None) == 1 and decode(crc=None) == 1 and b"chunk table" in lib.pl_last_error()
    assert decode(work=p + 4) == 1 and b"16-byte" in lib.pl_last_error()
    plain = lib.pl_png_work_bytes(3, 9, 6400, 100, 24, 16, 1)
    checked = lib.pl_png_checked_work_bytes(3, 9, 6400, 100, 24, 16, 1, 12, 5000)
    assert checked > plain and checked % 16 == 0 and lib.pl_png_checked_work_bytes(3, 9, 6400, 100, 24, 16, 1, 0, 5000) == -1
    assert lib.pl_png_checked_work_bytes(3, 9, 6400, 100, 24, 12, 1, 12, 5000) == -1
    header = (Path(__file__).resolve().parent.parent / "include" / "pylinac_hip.h").read_text()
    for entry in (r"int pl_adler32\(", r"int64_t pl_adler32_work_bytes\(", r"int pl_inflate_checked\(", r"int64_t pl_inflate_checked_work_bytes\(",
                  r"int pl_png_decode_checked\(", r"int64_t pl_png_checked_work_bytes\("):
        assert re.search(entry, header), entry
    assert lib.pl_abi_version() == 3
