"""Shared checks of pylinac_amd.tiff: read_tiff's IFD walk, load_frames, decode_tiff_strips and pl_tiff_decode
(tests/test_emulated_tiff.py on the CPU emulator, tests/test_gpu_tiff.py on the MI355X).  Every pixel comparison is EQUALITY
with ``np.asarray(PIL.Image.open(f))`` (libtiff), what the reference's FileImage hands its analyzers; RGB files against PIL's
``convert("I")``.

The files come from PIL (``Image.save(..., compression=, tiffinfo={317: predictor, 278: rows per strip})``, little-endian
only) and from ``write_tiff`` below -- big-endian files, strips at odd offsets, hand-made and damaged streams -- with its own
LZW encoder (libtiff's early-change rule).  ``pil_array`` is asked first in every case: PIL must read the file back equal to
the source array, so that no check is green because a fixture and the device err alike.  ``lzw_walk`` is a plain
table-building decoder kept for its counters (code widths, Clears inside a strip, KwKwK codes, string lengths): the cases
assert that the branch they are named for occurred."""
from __future__ import annotations

import io
import re
import struct
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

from pylinac_amd import dicom, tiff

to_np = dicom._to_numpy


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def pil_array(data: bytes) -> np.ndarray:
    img = Image.open(io.BytesIO(data))
    if img.mode == "RGB":
        return np.asarray(img.convert("I"))
    a = np.asarray(img)
    return a.astype(a.dtype.newbyteorder("="))                                     # (big-endian files come back as '>u2': the same values)


def pil_file(a: np.ndarray, compression=None, predictor=None, rows_per_strip=None, **kw) -> bytes:
    info = {}
    if predictor is not None:
        info[317] = predictor
    if rows_per_strip is not None:
        info[278] = rows_per_strip
    out = io.BytesIO()
    Image.fromarray(a).save(out, format="TIFF", **({"compression": compression} if compression else {}), tiffinfo=info, **kw)
    data = out.getvalue()
    want = a if a.ndim == 2 else np.asarray(Image.fromarray(a).convert("I"))
    assert np.array_equal(pil_array(data), want)                                   # the oracle validates the fixture
    return data


# ---- a TIFF writer (test files only) --------------------------------------------------------------------------------------
def lzw_encode(data: bytes, eoi: bool = True) -> bytes:
    """TIFF LZW, new style: MSB-first codes, Clear first, the width grows when the next free entry reaches 512 / 1024 / 2048
    on the encoder's side (one code ahead of the decoder's 511 / 1023 / 2047), Clear at 4094 entries (tif_lzw.c)"""
    acc = nacc = 0
    out = bytearray()
    width, nxt, table = 9, 258, {}

    def emit(code):
        nonlocal acc, nacc
        acc, nacc = (acc << width) | code, nacc + width
        while nacc >= 8:
            out.append((acc >> (nacc - 8)) & 0xFF)
            nacc -= 8
        acc &= (1 << nacc) - 1

    def grow():
        nonlocal width, nxt, table
        nxt += 1
        if nxt == 4094:
            emit(256)
            width, nxt, table = 9, 258, {}
        elif nxt in (512, 1024, 2048):
            width += 1

    emit(256)
    w = b""
    for b in data:
        wc = w + bytes([b])
        if len(wc) == 1 or wc in table:
            w = wc
            continue
        emit(w[0] if len(w) == 1 else table[w])
        table[wc] = nxt
        grow()
        w = bytes([b])
    if w:
        emit(w[0] if len(w) == 1 else table[w])
        grow()
    if eoi:
        emit(257)
    if nacc:
        out.append((acc << (8 - nacc)) & 0xFF)
    return bytes(out)


def lzw_walk(strip: bytes):
    """a table-building decoder -> (bytes, counters): widths seen, Clears after the first code, KwKwK codes, longest string"""
    table, out = {}, bytearray()
    seen = dict(widths=set(), clears=0, kwkwk=0, longest=0)
    pos, width, nxt, old, first = 0, 9, 258, None, True
    nbits = len(strip) * 8
    acc = int.from_bytes(strip, "big")
    while pos + width <= nbits:
        c = (acc >> (nbits - pos - width)) & ((1 << width) - 1)
        pos += width
        seen["widths"].add(width)
        if c == 257:
            break
        if c == 256:
            seen["clears"] += 0 if first else 1
            table, width, nxt, old, first = {}, 9, 258, None, False
            continue
        first = False
        if c < 256:
            s = bytes([c])
        elif c in table:
            s = table[c]
        else:
            assert old is not None and c == nxt, "corrupt"
            s = old + old[:1]
            seen["kwkwk"] += 1
        seen["longest"] = max(seen["longest"], len(s))
        out += s
        if old is not None:
            table[nxt] = old + s[:1]
            nxt += 1
            if nxt in (511, 1023, 2047):
                width += 1
        old = s
    return bytes(out), seen


def strip_bytes(a: np.ndarray, order: str, predictor: int) -> bytes:
    """rows of one strip -> the bytes the compressor sees: horizontal differencing per channel in the sample width, then the
    file's byte order"""
    rows = a.reshape(a.shape[0], a.shape[1], -1)
    if predictor == 2:
        rows = np.concatenate([rows[:, :1], rows[:, 1:] - rows[:, :-1]], axis=1)   # (wraps in a's unsigned dtype)
    return rows.astype(rows.dtype.newbyteorder(order)).tobytes()


def write_tiff(a: np.ndarray, order: str = "<", compression: int = 1, predictor: int = 1, rows_per_strip: int | None = None,
               shift: int = 0, resolution=None, tags=(), drop=(), mangle=None, magic: int = 42) -> bytes:
    """[H, W] uint8 / uint16 or [H, W, 3] uint8 -> a classic TIFF: header, ``shift`` pad bytes, the strips back to back, the
    value arrays, the IFD.  ``resolution`` = (numerator, denominator, unit); ``tags`` = extra (tag, type, values) entries
    (they replace the writer's own); ``drop`` = tags left out; ``mangle(k, strip) -> strip`` edits compressed strip k."""
    h, w = a.shape[:2]
    spp = 1 if a.ndim == 2 else a.shape[2]
    bits = 8 * a.dtype.itemsize
    rps = h if rows_per_strip is None else rows_per_strip
    strips = []
    for r0 in range(0, h, min(rps, h)):
        raw = strip_bytes(a[r0:r0 + rps], order, predictor)
        s = lzw_encode(raw) if compression == 5 else raw
        strips.append(mangle(len(strips), s) if mangle else s)
    body = bytearray(b"\0" * shift)
    offs = []
    for s in strips:
        offs.append(8 + len(body))
        body += s
    entries = {256: (3, [w]), 257: (3, [h]), 258: (3, [bits] * spp), 259: (3, [compression]), 262: (3, [2 if spp == 3 else 1]),
               273: (4, offs), 277: (3, [spp]), 278: (4, [rps]), 279: (4, [len(s) for s in strips])}
    if predictor != 1:
        entries[317] = (3, [predictor])
    if resolution is not None:
        entries.update({282: (5, [resolution[:2]]), 283: (5, [resolution[:2]]), 296: (3, [resolution[2]])})
    for tag, typ, vals in tags:
        entries[tag] = (typ, list(vals))
    for tag in drop:
        entries.pop(tag, None)
    ifd = bytearray()
    for tag in sorted(entries):
        typ, vals = entries[tag]
        code = {3: "H", 4: "I"}.get(typ)
        packed = b"".join(struct.pack(order + "II", *v) for v in vals) if typ == 5 else struct.pack(order + code * len(vals), *vals)
        if len(packed) > 4:
            if len(body) % 2:
                body += b"\0"
            at = 8 + len(body)
            body += packed
            packed = struct.pack(order + "I", at)
        ifd += struct.pack(order + "HHI", tag, typ, len(vals)) + packed.ljust(4, b"\0")
    if len(body) % 2:
        body += b"\0"
    head = (b"II" if order == "<" else b"MM") + struct.pack(order + "HI", magic, 8 + len(body))
    return head + bytes(body) + struct.pack(order + "H", len(entries)) + bytes(ifd) + struct.pack(order + "I", 0)


def checked(a: np.ndarray, **kw) -> bytes:
    """write_tiff, with PIL reading the file back equal to the source first"""
    data = write_tiff(a, **kw)
    want = a if a.ndim == 2 else np.asarray(Image.fromarray(a).convert("I"))
    assert np.array_equal(pil_array(data), want), kw
    return data


# ---- frames ---------------------------------------------------------------------------------------------------------------
H, W = 160, 257


def ridge(seed: int = 0, shape=(H, W)) -> np.ndarray:
    rng = np.random.default_rng(seed)
    x = np.arange(shape[1], dtype=np.float64)
    return (30000 + 20000 * np.exp(-(x - 128) ** 2 / 200)[None, :] + rng.integers(0, 48, shape)).astype(np.uint16)


def load(dev, files, **kw):
    stack = tiff.load_frames(files, device=dev, **kw)
    return to_np(stack.frames), stack


def same_as_pil(dev, files, **kw):
    got, stack = load(dev, files, **kw)
    for k, f in enumerate(files):
        want = pil_array(f)
        assert got[k].dtype == want.dtype and np.array_equal(got[k], want), k
    return got, stack


def counters(data: bytes) -> dict:
    """lzw_walk over every strip of a file, its output pinned to the strip's size -> the merged counters"""
    info = tiff.read_tiff(data)
    row_bytes = info.width * info.samples * info.bits // 8
    merged = dict(widths=set(), clears=[], kwkwk=0, longest=0)
    for off, n, _, rows in info.strips:
        out, seen = lzw_walk(data[off:off + n])
        assert len(out) == rows * row_bytes
        merged["widths"] |= seen["widths"]
        merged["clears"].append(seen["clears"])
        merged["kwkwk"] += seen["kwkwk"]
        merged["longest"] = max(merged["longest"], seen["longest"])
    return merged


# ---- 1: LZW ---------------------------------------------------------------------------------------------------------------
def check_ridge(dev, predictor):
    a = ridge()
    f = pil_file(a, "tiff_lzw", predictor=predictor, rows_per_strip=64)
    info = tiff.read_tiff(f)
    assert [s[2:] for s in info.strips] == [(0, 64), (64, 64), (128, 32)] and info.predictor == predictor
    seen = counters(f)
    assert 12 in seen["widths"] and min(seen["clears"][:2]) >= 2 and seen["kwkwk"] >= 1, seen
    got, stack = same_as_pil(dev, [f])
    assert got.dtype == np.uint16 and stack.status.cpu().tolist() == [0]


def check_constant(dev):
    a = np.full((H, W), 513, dtype=np.uint16)
    f = pil_file(a, "tiff_lzw", rows_per_strip=64)
    seen = counters(f)
    assert seen["longest"] > 180 and seen["kwkwk"] > 100 and a.nbytes > 50 * len(f), seen
    same_as_pil(dev, [f])
    # the writer's own encoder makes the same kind of stream (KwKwK chains), from a big-endian file
    g = checked(a, order=">", compression=5, rows_per_strip=64)
    assert counters(g)["kwkwk"] > 100
    same_as_pil(dev, [g])


def check_uint8(dev):
    a = (ridge() >> 8).astype(np.uint8)
    for predictor in (1, 2):
        f = pil_file(a, "tiff_lzw", predictor=predictor, rows_per_strip=64)
        seen = counters(f)
        if predictor == 1:
            assert 11 in seen["widths"] and seen["longest"] > 64, seen
        got, _ = same_as_pil(dev, [f])
        assert got.dtype == np.uint8


def check_random(dev):
    a = np.random.default_rng(7).integers(0, 65536, (96, 130)).astype(np.uint16)
    f = pil_file(a, "tiff_lzw", rows_per_strip=32)
    info = tiff.read_tiff(f)
    assert sum(s[1] for s in info.strips) > a.nbytes and counters(f)["longest"] <= 2
    same_as_pil(dev, [f])


SHAPES = [(1, 1), (1, 300), (3, 65), (5, 63), (5, 64), (4, 127), (4, 129)]


def check_shape(dev, rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    for dtype in (np.uint8, np.uint16):
        smooth = (rng.integers(0, 3, (rows, cols)).cumsum(axis=1) * 97 + 65000).astype(dtype)     # (wraps: the predictor's modulus)
        for a in (smooth, rng.integers(0, np.iinfo(dtype).max, (rows, cols)).astype(dtype)):
            files = [pil_file(a), pil_file(a, "tiff_lzw"), pil_file(a, "tiff_lzw", predictor=2), pil_file(a, "packbits"),
                     checked(a, order=">", compression=5, predictor=2)]
            for f in files:                                                        # (one at a time: the smallest stacks)
                same_as_pil(dev, [f])
            same_as_pil(dev, files)


# ---- 2: strips, byte order, PackBits, RGB ---------------------------------------------------------------------------------
def check_strip_geometry(dev):
    a = ridge(1, (37, 131))
    for rps in (1, 37, 50, 7):
        for comp in (None, "tiff_lzw", "packbits"):
            f = pil_file(a, comp, rows_per_strip=rps)
            info = tiff.read_tiff(f)
            assert len(info.strips) == -(-37 // min(info.tags[278][0], 37))
            if comp:                                                               # (PIL lays uncompressed strips out itself)
                assert len(info.strips) == -(-37 // min(rps, 37))
            same_as_pil(dev, [f])
    absent = checked(a, compression=5, predictor=2, drop=(278,))
    assert 278 not in tiff.read_tiff(absent).tags and len(tiff.read_tiff(absent).strips) == 1
    same_as_pil(dev, [absent])
    # strips at odd file offsets, for every compression the writer knows, in a stack whose files start anywhere mod 4
    files = [checked(a, compression=c, rows_per_strip=5, shift=s) for c in (1, 5) for s in (1, 2, 3)]
    assert sum(tiff.read_tiff(f).strips[0][0] % 2 for f in files) == 4 and len({len(f) % 4 for f in files}) > 1
    same_as_pil(dev, files)
    odd = checked(ridge(2, (9, 33)).astype(np.uint8), compression=1, rows_per_strip=2, shift=1)   # odd strip sizes as well
    same_as_pil(dev, [odd, odd])


def check_big_endian(dev):
    a = ridge(3, (40, 193))
    for kw in (dict(compression=1), dict(compression=5, predictor=2), dict(compression=5), dict(compression=1, rows_per_strip=7, shift=1)):
        f = checked(a, order=">", **kw)
        assert tiff.read_tiff(f).byte_order == "MM"
        same_as_pil(dev, [f])
    b = (a >> 8).astype(np.uint8)
    same_as_pil(dev, [checked(b, order=">", compression=5, predictor=2)])


def check_packbits(dev):
    for a in (ridge(4, (70, 200)), (ridge(4, (70, 200)) >> 8).astype(np.uint8), np.full((70, 200), 9, dtype=np.uint8)):
        f = pil_file(a, "packbits", rows_per_strip=16)
        assert tiff.read_tiff(f).compression == 32773 and len(tiff.read_tiff(f).strips) == 5
        same_as_pil(dev, [f])


def check_rgb(dev):
    rng = np.random.default_rng(5)
    a = np.clip(rng.integers(0, 40, (33, 131, 3)) + np.linspace(0, 215, 131)[None, :, None], 0, 255).astype(np.uint8)
    files = [pil_file(a), pil_file(a, "tiff_lzw", predictor=2, rows_per_strip=8), pil_file(a, "tiff_lzw"), pil_file(a, "packbits"),
             checked(a, order=">", compression=5, predictor=2, rows_per_strip=5)]
    got, _ = same_as_pil(dev, files)
    assert got.dtype == np.int32 and got.max() <= 255
    r, g, b = (a[..., k].astype(np.int64) for k in range(3))
    assert np.array_equal(got[0], (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16)
    assert np.array_equal(load(dev, files[:2], dtype=np.float64)[0], got[:2].astype(np.float64))


def check_mixed_stack(dev):
    a = [ridge(10 + k, (48, 150)) for k in range(5)]
    files = [pil_file(a[0]), pil_file(a[1], "packbits", rows_per_strip=10), pil_file(a[2], "tiff_lzw", predictor=2, rows_per_strip=16),
             checked(a[3], order=">", compression=5, predictor=2, rows_per_strip=48), checked(a[4], order=">", compression=1, shift=3)]
    got, stack = same_as_pil(dev, files)
    assert [x.compression for x in stack.images] == [1, 32773, 5, 5, 1] and [x.byte_order for x in stack.images] == ["II"] * 3 + ["MM"] * 2
    perm = [3, 1, 4, 0, 2]
    assert np.array_equal(load(dev, [files[k] for k in perm])[0], got[perm])
    with pytest.raises(ValueError, match=r"file 1 differs from file 0 in width, height"):
        tiff.load_frames([files[0], pil_file(a[1][:, :-1])], device=dev)
    with pytest.raises(ValueError, match=r"file 1 differs from file 0"):
        tiff.load_frames([files[0], pil_file((a[1] >> 8).astype(np.uint8))], device=dev)


def check_dtype_and_sources(dev, tmp_path):
    a8 = (ridge(6, (31, 77)) >> 8).astype(np.uint8)
    files = [pil_file(a8, "tiff_lzw", predictor=2), pil_file(a8)]
    for dt in (np.uint16, np.float64):
        got, _ = load(dev, files, dtype=dt)
        assert got.dtype == dt and np.array_equal(got, np.stack([a8, a8]).astype(dt))
    a16 = ridge(6, (31, 77))
    got, _ = load(dev, [pil_file(a16, "tiff_lzw")], dtype=np.float64)
    assert got.dtype == np.float64 and np.array_equal(got[0], a16.astype(np.float64))
    with pytest.raises(TypeError, match="np.uint16 or np.float64"):
        tiff.load_frames(files, device=dev, dtype=np.float32)
    with pytest.raises(ValueError, match="no files"):
        tiff.load_frames([], device=dev)
    path = tmp_path / "a.tif"
    path.write_bytes(files[0])
    got, stack = load(dev, [str(path), path, io.BytesIO(files[0]), bytearray(files[0])])
    assert np.array_equal(got, np.stack([a8] * 4)) and stack.images[0].path == str(path) and stack.images[2].path is None
    assert tiff.read_tiff(path).width == 77 and tiff.read_tiff(io.BytesIO(files[0])).height == 31


# ---- 3: resolution --------------------------------------------------------------------------------------------------------
def check_dpi(dev):
    a = ridge(8, (8, 40))
    inch = pil_file(a, dpi=(150, 150))
    info = tiff.read_tiff(inch)
    assert info.dpi == 150.0 and info.dpmm == 150 / 25.4
    cm = checked(a, resolution=(590551, 10000, 3))                                # 59.0551 pixels per centimetre
    want = float(Image.open(io.BytesIO(cm)).info["dpi"][0])
    got = tiff.read_tiff(cm).dpi
    assert got == 59.0551 * 2.54 and abs(got - want) <= 1e-6 * want
    none = checked(a)
    assert tiff.read_tiff(none).dpi is None and tiff.read_tiff(none).dpmm is None
    assert tiff.read_tiff(checked(a, resolution=(72, 1, 1))).dpi is None            # ResolutionUnit 1: no absolute unit
    stack = tiff.load_frames([inch, inch], device=dev)
    assert stack.dpmm == 150 / 25.4
    assert tiff.load_frames([inch, none], device=dev, dpi=200).dpmm == 200 / 25.4   # dpi= overrides the tags
    assert tiff.load_frames([none], device=dev).dpmm is None
    mixed = tiff.load_frames([inch, cm], device=dev)                               # loading is fine ...
    assert np.array_equal(to_np(mixed.frames)[1], a)
    with pytest.raises(ValueError, match="differ in dpmm"):                        # ... asking for ONE dpmm is not
        mixed.dpmm


# ---- 4: status ------------------------------------------------------------------------------------------------------------
def status_files():
    a = [ridge(20 + k, (48, 150)) for k in range(4)]

    def smash(k, s):                                                               # 20 bytes of 0xFF in the middle of strip 1
        return s[:len(s) // 2] + b"\xff" * 20 + s[len(s) // 2 + 20:] if k == 1 else s

    def cut(k, s):                                                                 # an early EOI: the first half of the rows only
        return lzw_encode(strip_bytes(a[2][:8], "<", 1)) if k == 0 else s

    files = [pil_file(a[0], "tiff_lzw", rows_per_strip=16), write_tiff(a[1], compression=5, rows_per_strip=16, mangle=smash),
             write_tiff(a[2], compression=5, rows_per_strip=16, mangle=cut), checked(a[3], compression=5, predictor=2, rows_per_strip=16)]
    for k in (1, 2):                                                               # PIL refuses both
        with pytest.raises(OSError):
            pil_array(files[k])
    return a, files


def check_status(dev, monkeypatch):
    a, files = status_files()
    stack = tiff.load_frames(files, device=dev, check=False)
    assert stack.status.cpu().tolist() == [0, tiff.STATUS_CORRUPT_LZW, tiff.STATUS_SHORT, 0]
    got = to_np(stack.frames)
    assert np.array_equal(got[0], a[0]) and np.array_equal(got[3], a[3])
    assert np.array_equal(got[2][16:], a[2][16:]) and np.array_equal(got[2][:8], a[2][:8])       # the sound strips of a flagged frame
    with pytest.raises(OSError, match=r"file 1: corrupt LZW"):
        tiff.load_frames(files, device=dev)
    with pytest.raises(OSError, match=r"file 1: a strip decodes to fewer bytes"):
        tiff.load_frames([files[0], files[2]], device=dev)
    raw_short = write_tiff(a[0], compression=1, rows_per_strip=16, mangle=lambda k, s: s[:-3] if k == 2 else s)
    assert tiff.load_frames([raw_short], device=dev, check=False).status.cpu().tolist() == [tiff.STATUS_SHORT]
    # check=False transfers nothing back: no tensor of the call is copied to the host
    calls = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *x, **k: (calls.append(self.data_ptr()), real(self, *x, **k))[1])
    stack = tiff.load_frames(files, device=dev, check=False)
    assert not calls
    stack = tiff.load_frames([files[0], files[3]], device=dev, check=True)
    assert set(calls) == {stack.status.data_ptr()}                                 # check=True: the status, and nothing else
    monkeypatch.undo()


def strip_table(files):
    """files -> (buffer, offsets, lengths, descriptors, flags) as load_frames builds them"""
    buf, off, ln, desc, flags = b"", [], [], [], []
    for k, f in enumerate(files):
        buf += b"\0" * (-len(buf) % 4)
        info = tiff.read_tiff(f)
        flags.append((info.predictor == 2) | 2 * (info.byte_order == "MM" and info.bits == 16))
        for o, c, r0, rows in info.strips:
            off.append(len(buf) + o), ln.append(c), desc.append((k, r0, rows, info.compression))
        buf += f
    return (np.frombuffer(buf, dtype=np.uint8), np.array(off, dtype=np.int64), np.array(ln, dtype=np.int64),
            np.array(desc, dtype=np.int32), np.array(flags, dtype=np.int32))


def check_window_outside_the_buffer(dev):
    a = [ridge(30 + k, (24, 100)) for k in range(3)]
    files = [pil_file(a[0], "tiff_lzw", rows_per_strip=8), pil_file(a[1], "packbits", rows_per_strip=8), pil_file(a[2], rows_per_strip=8)]
    buf, off, ln, desc, flags = strip_table(files)
    assert len(off) == 9
    kw = dict(width=100, height=24, bits=16, device=dev, max_strip_bytes=int(ln.max()))
    cases = {(1, "off", -1): 0, (0, "off", len(buf) - 3): 0, (4, "len", 1 << 40): 1, (5, "len", -5): 1, (3, "off", 1 << 50): 1,
             (7, "off", len(buf)): 2, (8, "len", int(ln.max()) + 1): 2, (2, "row", 20): 0, (6, "row", -1): 2, (4, "comp", 8): 1}
    for (s, what, value), frame in cases.items():
        o2, l2, d2 = off.copy(), ln.copy(), desc.copy()
        if what == "off":
            o2[s] = value
        elif what == "len":
            l2[s] = value
        else:
            d2[s, 1 if what == "row" else 3] = value
        out = torch.from_numpy(np.full((3, 24, 100), 0x5A5A, dtype=np.uint16).view(np.int16)).view(torch.uint16).to(dev)
        frames, status = tiff.decode_tiff_strips(buf, o2, l2, d2, flags, out=out, compressions=7, **kw)
        assert status.cpu().tolist() == [int(k == frame) for k in range(3)], (s, what)
        got = to_np(frames)
        for k in range(3):
            assert np.array_equal(got[k], a[k]) if k != frame else (got[k] == 0x5A5A).all(), (s, what, k)
    # a frame index outside the stack: the strip is skipped, nobody else is disturbed
    d2 = desc.copy()
    d2[8, 0] = 3
    frames, status = tiff.decode_tiff_strips(buf, off, ln, d2, flags, compressions=7, **kw)
    assert status.cpu().tolist() == [0, 0, 0] and np.array_equal(to_np(frames)[:2], np.stack(a[:2]))
    assert np.array_equal(to_np(frames)[2][:16], a[2][:16])


# ---- 5: refusals ----------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    a = ridge(40, (16, 40))
    a8 = (a >> 8).astype(np.uint8)
    rgb = np.stack([a8, a8, a8], axis=2)
    rgba = np.concatenate([rgb, rgb[..., :1]], axis=2)
    old_style = write_tiff(a, compression=5, mangle=lambda k, s: b"\x00\x01" + s[2:])
    cases = [
        (write_tiff(a, tags=[(322, 3, [16]), (323, 3, [16])]), "tiled"),
        (write_tiff(a, magic=43), "BigTIFF"),
        (pil_file(a, "tiff_adobe_deflate"), "Compression 8 "),
        (pil_file(a8, "jpeg"), "Compression 7 "),
        (pil_file((a8 > 200), "group4"), "Compression 4 "),
        (write_tiff(a, compression=5, tags=[(317, 3, [3])]), "Predictor 3"),
        (write_tiff(a, predictor=2), "Predictor 2 with Compression 1"),
        (write_tiff(a, compression=32773, predictor=2), "Predictor 2 with Compression 32773"),
        (write_tiff(rgb, tags=[(284, 3, [2]), (273, 4, [8, 8, 8]), (279, 4, [640, 640, 640])]), "PlanarConfiguration 2"),
        (write_tiff(a, tags=[(262, 3, [0])]), "PhotometricInterpretation 0"),
        (write_tiff(a8, tags=[(262, 3, [3])]), "PhotometricInterpretation 3"),
        (pil_file(a8 > 200), "BitsPerSample 1 "),
        (write_tiff(a8, tags=[(258, 3, [4])]), "BitsPerSample 4 "),
        (pil_file(a.astype(np.int32)), "BitsPerSample 32 |SampleFormat 2"),
        (pil_file(a.astype(np.float32)), "SampleFormat 3"),
        (write_tiff(np.stack([a, a, a], axis=2)), r"BitsPerSample \(16, 16, 16\)"),
        (write_tiff(rgba, tags=[(338, 3, [2]), (262, 3, [2])]), "ExtraSamples"),
        (old_style, "old-style"),
    ]
    good = pil_file(a)
    for data, text in cases:
        with pytest.raises(ValueError, match=r"file 1: .*(" + text + ")"):
            tiff.load_frames([good, data], device=dev)
    # the IFD walk: offsets against the file length, in the reader itself
    with pytest.raises(ValueError, match="not a TIFF"):
        tiff.read_tiff(b"PK\x03\x04" + good[4:])
    with pytest.raises(ValueError, match="first IFD .* lies outside the file"):
        tiff.read_tiff(good[:4] + struct.pack("<I", len(good) + 10) + good[8:])
    many = write_tiff(ridge(41, (40, 9)), rows_per_strip=1)                        # 40 strip offsets: an array at an offset
    at = many.index(struct.pack("<HHI", 273, 4, 40)) + 8
    with pytest.raises(ValueError, match="values of tag 273 .* lie outside the file"):
        tiff.read_tiff(many[:at] + struct.pack("<I", len(many) - 20) + many[at + 4:])
    cut = write_tiff(a, tags=[(279, 4, [a.nbytes + 5000])])
    with pytest.raises(ValueError, match="strip 0 .* lies outside the file"):
        tiff.read_tiff(cut)
    with pytest.raises(ValueError, match="7 strip offsets"):
        tiff.read_tiff(write_tiff(a, tags=[(278, 4, [2]), (273, 4, [8] * 7), (279, 4, [80] * 7)]))


def check_c_abi_argument_checks(dev):
    """pl_tiff_decode: unsupported (2) for samples the kernels do not decode, invalid argument (1) for null pointers, n = 0, bad
    masks and kinds -- all before any launch (the pointers below are never dereferenced); pl_tiff_work_bytes: -1 for the same"""
    from pylinac_amd import _lib

    lib = _lib.load()
    buf = torch.zeros(256, dtype=torch.uint8, device=dev)
    idx = torch.zeros(8, dtype=torch.int64, device=dev)
    st = torch.zeros(4, dtype=torch.int32, device=dev)
    p, q, s = buf.data_ptr(), idx.data_ptr(), st.data_ptr()

    def call(n=1, n_strips=1, bits=16, spp=1, mask=1, kind=0, bytes_=p, out=p, work=p, flags=s, w=4, h=4, max_strip=64):
        return lib.pl_tiff_decode(bytes_, 256, q, q, s, n_strips, max_strip, flags, n, w, h, bits, spp, mask, out, kind, s, work, None)

    for bits, spp in ((12, 1), (1, 1), (4, 1), (32, 1), (16, 3), (8, 4), (8, 2)):
        assert call(bits=bits, spp=spp) == 2 and b"unsupported samples" in lib.pl_last_error()
        assert lib.pl_tiff_work_bytes(1, 1, 64, 4, 4, bits, spp, 1) == -1
    assert call(n=0) == 1 and call(n=65536) == 1 and call(n_strips=0) == 1 and call(w=0) == 1 and call(h=0) == 1
    assert call(bytes_=None) == 1 and call(out=None) == 1 and call(work=None) == 1 and call(flags=None) == 1
    assert call(mask=0) == 1 and call(mask=8) == 1 and call(kind=3) == 1 and call(kind=-1) == 1 and call(max_strip=-1) == 1
    assert call(bytes_=p + 1) == 1 and b"4-byte" in lib.pl_last_error()
    assert call(work=p + 4) == 1 and b"16-byte" in lib.pl_last_error()
    assert call(n_strips=65536, mask=2) == 1                                       # PackBits: the stream is a grid axis
    assert lib.pl_tiff_work_bytes(0, 1, 64, 4, 4, 16, 1, 1) == -1 and lib.pl_tiff_work_bytes(1, 1, 64, 4, 4, 16, 1, 0) == -1
    assert lib.pl_tiff_work_bytes(1, 65536, 64, 4, 4, 16, 1, 2) == -1 and lib.pl_tiff_work_bytes(1, 1, 64, 46341, 46341, 8, 1, 1) == -1
    plain, packed = lib.pl_tiff_work_bytes(3, 9, 64, 100, 24, 16, 1, 5), lib.pl_tiff_work_bytes(3, 9, 64, 100, 24, 16, 1, 7)
    assert plain >= 3 * 24 * 100 * 2 and plain % 16 == 0 and packed > plain
    header = (Path(__file__).resolve().parent.parent / "include" / "pylinac_hip.h").read_text()
    assert re.search(r"int pl_tiff_decode\(", header) and re.search(r"int64_t pl_tiff_work_bytes\(", header)
