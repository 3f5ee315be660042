"""Shared checks of ``dicom.load_zip(encapsulated=True)``: RLE Lossless and JPEG Lossless members of ZIP archives decoded on the
device, and of the two kernels it adds (``dicom.index_encapsulated`` / pl_dicom_encap_index, ``dicom.copy_ranges`` /
pl_copy_ranges) -- tests/test_emulated_dicom_zip_encap.py on the CPU emulator, tests/test_gpu_dicom_zip_encap.py on the MI355X.
Every comparison is EQUALITY.

The reference of the loader is ``load_frames(..., jpeg_lossless=True)`` on the bytes ``zipfile`` extracts -- the same tensor,
the same metadata, the same exception with the member's name where ``load_frames`` says ``file K`` -- and the source frames.
The files come from the builders tests/dicom_rle_checks.py, tests/dicom_jpegll_checks.py and tests/zip_checks.py pin.  The
reference of the index kernel is a walk restated here (``walk_items``), that of the copy is numpy slicing.  Without the
feature every loader check fails: ``load_zip`` has no ``encapsulated`` keyword and the library has neither symbol."""
from __future__ import annotations

import contextlib
import io
import re
import struct
import zipfile
from pathlib import Path

import numpy as np
import pytest
import torch

import dicom_jpegll_checks as jl
import dicom_rle_checks as rle
import zip_checks as zc
from pylinac_amd import dicom

H = dicom.ENCAP_HEAD_BYTES
EVEN = zc.EVEN
ODD = (29, 35)
to_np = dicom._to_numpy
ARCHIVE = "ZIP archive"                                      # zipstack's name for an archive given as bytes
TODAY_RLE = "RLE Lossless Pixel Data inside an archive"
TODAY_ENCAP = "encapsulated \\(compressed\\) Pixel Data: decoded by pydicom's codec plug-ins"


# ---- the wrapper: encapsulated=True for load_zip, jpeg_lossless=True for load_frames ---------------------------------------------
def extracted(data: bytes, names=None) -> list:
    with zipfile.ZipFile(io.BytesIO(data)) as zf:
        return [zf.read(n) for n in (names if names is not None else [i.filename for i in zf.infolist() if i.filename.endswith(".dcm")])]


def same(dev, data: bytes, frames, names=None, **kw):
    """load_zip(encapsulated=True) == load_frames(jpeg_lossless=True) on what the stdlib extracts, and == ``frames``"""
    x, metas, got = dicom.load_zip(data, device=dev, encapsulated=True, **kw)
    want, want_metas = dicom.load_frames(extracted(data, got), device=dev, jpeg_lossless=True, **zc.reference_keywords(kw))
    assert x.dtype == want.dtype and x.shape == want.shape and torch.equal(x, want)
    assert [m._values for m in metas] == [m._values for m in want_metas]
    for m in metas:
        if "PixelDataFragments" in m:                                              # (native members carry none)
            assert m.PixelData[1] == -1 and all(isinstance(v, int) for frag in m.PixelDataFragments for v in frag)
    if names is not None:
        assert got == names
    if frames is not None:
        assert np.array_equal(to_np(x), frames)
    return x, metas, got


def same_error(dev, data: bytes, member: str | None, exc=ValueError, **kw):
    """the exception load_frames raises for the extracted bytes, with ``ARCHIVE: member 'NAME'`` where it names ``file K`` (or in
    front, where it names no file); ``member`` None: the very same text"""
    with pytest.raises(exc) as want:
        dicom.load_frames(extracted(data), device=dev, jpeg_lossless=True, **zc.reference_keywords(kw))
    with pytest.raises(exc) as got:
        dicom.load_zip(data, device=dev, encapsulated=True, **kw)
    assert type(got.value) is type(want.value)
    text, who = str(want.value), f"{ARCHIVE}: member {member!r}"
    if member is None:
        expected = text
    elif re.search(r"file \d+", text):
        expected = re.sub(r"file \d+", lambda _: who, text)
    else:
        expected = f"{who}: {text}"
    assert str(got.value) == expected
    return expected


@contextlib.contextmanager
def counted(name: str, keep=lambda a: a):
    """calls of ``dicom.<name>`` made while the block runs: the list receives ``keep`` of each call's positional arguments"""
    real, seen = getattr(dicom, name), []

    def spy(*a, **kw):
        seen.append(keep(a))
        return real(*a, **kw)

    setattr(dicom, name, spy)
    try:
        yield seen
    finally:
        setattr(dicom, name, real)


def one_each(frames, build, prefix="s"):
    return [(f"{prefix}{k}.dcm", build(frames[k:k + 1], k)) for k in range(len(frames))]


def bits_stored(n: int) -> bytes:
    return rle._el(0x0028, 0x0101, "US", struct.pack("<H", n))


# ---- 1: RLE members -------------------------------------------------------------------------------------------------------
def check_rle_members(dev):
    mixed = [zipfile.ZIP_STORED, zipfile.ZIP_DEFLATED, zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED]
    for dtype in (np.uint8, np.int16, np.uint16):
        frames = rle.container_frames(dtype, shape=EVEN)
        files = one_each(frames, lambda f, k: rle.rle_file(f, table="filled" if k % 2 else "empty"))
        x, metas, _ = same(dev, zc.dicom_zip(files, kinds=mixed), frames, names=[f[0] for f in files])
        assert str(x.dtype) == f"torch.{np.dtype(dtype).name}" and metas[0].TransferSyntaxUID == rle.RLE_UID
    frames = rle.container_frames(np.uint16, shape=ODD)                            # frames of 2030 bytes: any alignment of the segments
    files = one_each(frames, lambda f, k: rle.rle_file(f))
    data = zc.dicom_zip(files, kinds=mixed)
    same(dev, data, frames)
    same(dev, data, frames, raw_pixels=True)
    same(dev, data, frames.astype(np.float64), dtype=np.float64)
    same(dev, data, frames.astype(np.int32), raw_pixels=True, dtype=np.int32)
    pick = [files[2][0], files[0][0]]
    same(dev, data, frames[[2, 0]], names=pick, members=pick)
    # a multi-frame member between single-frame ones, its table filled
    multi = [("a.dcm", rle.rle_file(frames[:1])), ("b.dcm", rle.rle_file(frames[1:4], table="filled")), ("c.dcm", rle.rle_file(frames[:1]))]
    x, metas, _ = same(dev, zc.dicom_zip(multi), np.concatenate([frames[:1], frames[1:4], frames[:1]]))
    assert metas[1].NumberOfFrames == 3 and len(metas[1].PixelDataFragments) == 3 and x.shape[0] == 5
    # rescale: shared (the fused float64 form) and per member; raw_pixels leaves it out
    signed = rle.container_frames(np.int16, shape=ODD)
    shared = zc.ds(0x1052, "-1024") + zc.ds(0x1053, "1.5")
    files = one_each(signed, lambda f, k: rle.rle_file(f, extra=shared))
    x, _, _ = same(dev, zc.dicom_zip(files), signed.astype(np.float64) * 1.5 + -1024)
    assert x.dtype == torch.float64
    same(dev, zc.dicom_zip(files), signed, raw_pixels=True)
    own = one_each(signed, lambda f, k: rle.rle_file(f, extra=zc.ds(0x1052, str(-1000 - k)) + zc.ds(0x1053, str(1 + k))))
    same(dev, zc.dicom_zip(own), np.stack([signed[k].astype(np.float64) * (1 + k) + (-1000 - k) for k in range(4)]))
    # BitsStored 12 with dirty upper bits
    dirty = rle.container_frames(np.uint16, shape=EVEN)
    assert (dirty >> 12).any()
    files = one_each(dirty, lambda f, k: rle.rle_file(f, extra=bits_stored(12)))
    same(dev, zc.dicom_zip(files), dirty & 0x0FFF, correct_unused_bits=True)
    same(dev, zc.dicom_zip(files), dirty)


# ---- 2: JPEG Lossless members ---------------------------------------------------------------------------------------------
def check_jpegll_members(dev):
    uids = (jl.UID70, jl.UID57, jl.UID70)
    for precision, dtype in ((8, np.uint8), (12, np.uint16), (16, np.uint16)):
        frames = np.stack([jl.noise(60 + k, EVEN, precision) for k in range(3)]).astype(dtype)
        files = one_each(frames, lambda f, k: jl.jpegll_file(f, uid=uids[k], precision=precision, sel=(1, 4, 7)[k]))
        kinds = [zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED, zipfile.ZIP_DEFLATED]
        with counted("copy_ranges") as copies, counted("_fetch_stream_head") as fetches:
            x, metas, _ = same(dev, zc.dicom_zip(files, kinds=kinds), frames, names=[f[0] for f in files])
        assert not copies and not fetches                                          # one fragment per frame: decoded in place
        assert [m.TransferSyntaxUID for m in metas] == list(uids) and all(m.PixelDataOffsetTable == [] for m in metas)
    for width in (35, 64, 65):                                                     # the wave's seams
        frames = np.stack([jl.noise(70 + k, (3, width), 16) for k in range(2)])
        same(dev, zc.dicom_zip(one_each(frames, lambda f, k: jl.jpegll_file(f, sel=1 + 3 * k))), frames)
    frames = rle.container_frames(np.uint16, shape=ODD)
    # a restart interval, a point transform, members that differ in table and predictor
    same(dev, zc.dicom_zip(one_each(frames, lambda f, k: jl.jpegll_file(f, restart=35 * 10, sel=4))), frames)
    same(dev, zc.dicom_zip(one_each(frames, lambda f, k: jl.jpegll_file(f, pt=2))), (frames >> 2) << 2, raw_pixels=True)
    opts = [dict(sel=1), dict(sel=7, table=jl.FLAT), dict(sel=4, restart=35 * 5), dict(sel=6, table=jl.FLAT, table_id=2)]
    data = zc.dicom_zip(one_each(frames, lambda f, k: jl.jpegll_file(f, **opts[k])))
    same(dev, data, frames)
    same(dev, data, frames.astype(np.float64), dtype=np.float64)
    pick = ["s3.dcm", "s1.dcm"]
    same(dev, data, frames[[3, 1]], names=pick, members=pick)
    # a two-frame member, table empty and filled
    for table in ("empty", "filled"):
        multi = [("a.dcm", jl.jpegll_file(frames[:1])), ("b.dcm", jl.jpegll_file(frames[1:3], table=table)), ("c.dcm", jl.jpegll_file(frames[3:]))]
        _, metas, _ = same(dev, zc.dicom_zip(multi), frames)
        assert len(metas[1].PixelDataOffsetTable) == (2 if table == "filled" else 0)
    # signed CT-like int16 with rescale tags; BitsStored 12
    ct = jl.ct_slices(3, 32)
    shared = zc.ds(0x1052, "-1024") + zc.ds(0x1053, "1")
    files = one_each(ct, lambda f, k: jl.jpegll_file(f, extra=shared, sel=1 + k))
    x, _, _ = same(dev, zc.dicom_zip(files), ct.astype(np.float64) - 1024)
    assert x.dtype == torch.float64 and (ct < 0).any()
    x, _, _ = same(dev, zc.dicom_zip(files), ct, raw_pixels=True)
    assert x.dtype == torch.int16
    dirty = rle.container_frames(np.uint16, shape=EVEN)
    same(dev, zc.dicom_zip(one_each(dirty, lambda f, k: jl.jpegll_file(f, extra=bits_stored(12)))), dirty & 0x0FFF, correct_unused_bits=True)


# ---- 3: frames that span fragments ----------------------------------------------------------------------------------------
def check_spanning_fragments(dev):
    frames = rle.container_frames(np.uint16, shape=ODD)
    plain = jl.encode(jl.unsigned(frames)[0], 16)
    sos = plain.index(b"\xff\xda") + 10                                            # the first byte of the scan
    assert sos == 63 and plain.index(b"\xff\xc4") < 20 < sos
    com = jl.segment(0xFE, b"x")                                                   # five bytes: the scan then starts at an even byte
    cases = {
        "inside the header, and inside the scan at an odd byte of it": jl.split_file(frames[:1], (20, 100)),
        "directly after SOS": jl.split_file(frames[:1], (sos + 5,), head=com),
    }
    assert (100 - sos) % 2 == 1
    for what, file in cases.items():
        assert len(dicom.read_part10(file, jpeg_lossless=True)[0].PixelDataFragments) >= 2
        with counted("copy_ranges") as copies:
            same(dev, zc.dicom_zip([("x.dcm", file)]), frames[:1])
        assert len(copies) == 1, what
    # two frames, a filled table, 3 + 2 fragments: the second frame's stream is shorter than the second cut
    pair = np.stack([frames[0], np.full(ODD, 700, dtype=np.uint16)])
    two = jl.split_file(pair, (50, 600), table="filled", sel=5)
    meta, _ = dicom.read_part10(two, jpeg_lossless=True)
    assert len(meta.PixelDataFragments) == 5 and len(meta.PixelDataOffsetTable) == 2
    with counted("copy_ranges") as copies:
        same(dev, zc.dicom_zip([("two.dcm", two)]), pair)
    assert len(copies) == 1 and len(copies[0][2]) == 5                             # ONE call over the five fragments
    # frames decoded in place and staged frames in one archive: one decode call per buffer, the frames in their order
    files = [("a.dcm", jl.jpegll_file(frames[1:2], sel=7)), ("b.dcm", cases["directly after SOS"]), ("c.dcm", two),
             ("d.dcm", jl.jpegll_file(frames[2:3], sel=4))]
    want = np.concatenate([frames[1:2], frames[:1], pair, frames[2:3]])
    with counted("copy_ranges") as copies:
        same(dev, zc.dicom_zip(files, kinds=[zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED] * 2), want)
        same(dev, zc.dicom_zip(files), want.astype(np.float64), dtype=np.float64)
    assert len(copies) == 2


# ---- 4: the head boundary ---------------------------------------------------------------------------------------------------
def check_head_boundary(dev):
    frames = rle.container_frames(np.uint16, shape=ODD)

    def fetches_of(file, want_frames=frames[:1]):
        with counted("_fetch_stream_head") as fetches:
            same(dev, zc.dicom_zip([("p.dcm", jl.jpegll_file(frames[1:2])), ("h.dcm", file)]), np.concatenate([frames[1:2], want_frames]))
        return [a[2] for a in fetches]

    def length(file):
        return sum(n for _, n in dicom.read_part10(file, jpeg_lossless=True)[0].PixelDataFragments)

    for end, want in ((H - 1, []), (H, []), (H + 1, [4096])):
        com = jl.segment(0xFE, b"c" * (end - 63 - 4))
        file = jl.jpegll_file(frames[:1], head=com)
        stream = jl.encode(jl.unsigned(frames)[0], 16, head=com)
        assert stream.index(b"\xff\xda") + 10 == end
        assert fetches_of(file) == [min(w, length(file)) for w in want], end
    # a 10 KiB APPn: 4 -> 8 -> 16 KiB (the frame ends before 16 KiB)
    file = jl.jpegll_file(frames[:1], head=jl.segment(0xE1, bytes(range(256)) * 40))
    total = length(file)
    assert 10240 + 63 < total < 16384
    assert fetches_of(file) == [4096, 8192, total]
    # a first fragment shorter than 64 bytes: the heads of both fragments hold the header
    assert fetches_of(jl.split_file(frames[:1], (40,))) == []
    # a header that runs past a short first fragment and past the heads: fetched end to end across the fragments
    file = jl.split_file(frames[:1], (40,), head=jl.segment(0xFE, b"c" * 300))
    assert 40 + H < 63 + 304 < length(file) and fetches_of(file) == [min(4096, length(file))]


# ---- 5: capacity ----------------------------------------------------------------------------------------------------------
def check_capacity(dev):
    frames = rle.container_frames(np.uint16, shape=ODD)
    for pieces, calls in ((40, 2), (16, 1)):
        file = jl.split_file(frames[:1], tuple(range(20, 20 * pieces, 20)))
        assert len(dicom.read_part10(file, jpeg_lossless=True)[0].PixelDataFragments) == pieces
        with counted("index_encapsulated") as index:
            same(dev, zc.dicom_zip([("p.dcm", jl.jpegll_file(frames[1:2])), ("m.dcm", file)]), frames[[1, 0]])
        assert len(index) == calls, pieces
        assert index[0][3:5] == (16, 1) and (calls == 1 or index[1][3:5] == (40, 1))


# ---- 6: a long header in front of encapsulated Pixel Data -----------------------------------------------------------------------
def check_long_header(dev):
    """a 150 KiB private element in front of the Pixel Data: the 64 KiB prefix doubles twice, and the walk ends at the element's
    header however much of the member follows"""
    rng = np.random.default_rng(53)
    frames = rle.container_frames(np.uint16, n=2, shape=EVEN)
    private = rle._el(0x0029, 0x1010, "OB", rng.integers(0, 256, 150 * 1024, dtype=np.uint8).tobytes())
    for build in (rle.rle_file, jl.jpegll_file):
        files = [("long.dcm", build(frames[:1], extra=private)), ("plain.dcm", build(frames[1:2]))]
        data = zc.dicom_zip(files)
        with counted("_walk_part10", keep=lambda a: len(a[0])) as walks:          # (a kept view would pin the growing prefix)
            x, metas, _ = dicom.load_zip(data, device=dev, encapsulated=True)
        assert walks[:3] == [65536, 131072, len(files[0][1])] and len(files[0][1]) < 262144
        assert metas[0].PixelData == (metas[1].PixelData[0] + len(private), -1) and np.array_equal(to_np(x), frames)
        if build is rle.rle_file:
            same(dev, data, frames)
        else:
            same(dev, zc.dicom_zip(files, kinds=[zipfile.ZIP_STORED] * 2), frames)


# ---- damage and refusals ----------------------------------------------------------------------------------------------------
def edited(file: bytes, at: int, fmt: str, *values) -> bytes:
    return zc.patched(file, at, fmt, *values)


def check_damaged_items(dev):
    """the item sequence: every message of ``_fragments``, for RLE and for JPEG members; the second member is the damaged one"""
    frames = rle.container_frames(np.uint16, shape=EVEN)
    for build, kind in ((rle.rle_file, "rle"), (jl.jpegll_file, "jpegll")):
        good = build(frames[:1])
        meta, _ = dicom.read_part10(good, jpeg_lossless=True)
        first, (frag, length) = meta.PixelData[0], meta.PixelDataFragments[0]
        filled = build(frames[:2], table="filled")
        table_at = dicom.read_part10(filled, jpeg_lossless=True)[0].PixelData[0] + 8
        cases = {
            "the sequence delimiter is missing": good[:-8],
            "delimiter is missing": good[:-3],
            "an item of defined length inside the file was expected": edited(good, frag - 8, "<HH", 0xFFFE, 0xE001),
            "item of defined length inside the file": edited(good, frag - 4, "<I", length + 1000),
            "an item of defined length": edited(good, frag - 4, "<I", 0xFFFFFFFF),
            "of defined length": edited(good, frag - 4, "<I", 0xFFFFFFFE),
            "the Basic Offset Table is no list of uint32 values": good[:first + 4] + struct.pack("<I", 6) + bytes(6) + good[first + 8:],
            "the Basic Offset Table item is missing": good[:first] + struct.pack("<HHI", 0xFFFE, 0xE0DD, 0),
            "the Basic Offset Table disagrees": edited(filled, table_at + 4, "<I", struct.unpack_from("<I", filled, table_at + 4)[0] + 2),
        }
        for k, (text, bad) in enumerate(cases.items()):
            data = zc.dicom_zip([("ok.dcm", good), ("bad.dcm", bad)], kinds=[zipfile.ZIP_DEFLATED, (zipfile.ZIP_STORED, zipfile.ZIP_DEFLATED)[k % 2]])
            message = same_error(dev, data, "bad.dcm")
            assert text in message and message.startswith(f"{ARCHIVE}: member 'bad.dcm': malformed encapsulated Pixel Data"), (kind, text)
        # fragment counts that fit no rule
        data = zc.dicom_zip([("n.dcm", rle._meta(meta.TransferSyntaxUID) + rle.image_tags(frames[:2]) + good[good.index(struct.pack("<HH", 0x7FE0, 0x0010)):])])
        assert "for NumberOfFrames = 2" in same_error(dev, data, "n.dcm")


def check_damaged_headers(dev):
    """RLE segment headers and JPEG markers: ``_rle_segments``' and ``_jpegll_header``'s own words behind the member's name"""
    frames = rle.container_frames(np.uint16, shape=EVEN)
    good = rle.rle_file(frames[:1])
    frag = dicom.read_part10(good)[0].PixelDataFragments[0][0]
    offs = struct.unpack_from("<16I", good, frag)
    for text, bad in {"states 3 segments": edited(good, frag, "<I", 3), "not strictly increasing": edited(good, frag + 8, "<I", offs[1]),
                      "lies outside the fragment": edited(good, frag + 8, "<I", 1 << 20),
                      "shorter than its 64-byte header": good[:frag - 4] + struct.pack("<I", 40) + good[frag:frag + 40] + struct.pack("<HHI", 0xFFFE, 0xE0DD, 0)}.items():
        assert text in same_error(dev, zc.dicom_zip([("ok.dcm", good), ("bad.dcm", bad)]), "bad.dcm"), text
    f = jl.unsigned(frames)[0]

    def one(stream, stack=frames[:1], uid=jl.UID70):
        return rle._meta(uid) + rle.image_tags(stack) + rle.encapsulate([stream])

    plain = jl.encode(f, 16)
    ok = ("ok.dcm", one(plain))
    for text, stream, exc in (("does not start with SOI", b"\x00" + plain[1:], ValueError),
                              ("SOF0 (baseline DCT), marker FFC0", jl.encode(f, 16, sof=0xC0), NotImplementedError),
                              ("SOF3 with Nf = 3", jl.encode(f, 16, nf=3), NotImplementedError),
                              ("DAC (arithmetic conditioning), marker FFCC", jl.encode(f, 16, head=jl.segment(0xCC, b"\x00\x00")), NotImplementedError),
                              ("DNL (number of lines), marker FFDC", jl.encode(f, 16, head=jl.segment(0xDC, b"\x00\x1d")), NotImplementedError),
                              ("without SOS", plain[:plain.index(b"\xff\xda")], ValueError),
                              ("lies outside the fragment", plain[:plain.index(b"\xff\xc4") + 10], ValueError),
                              ("SOF3 states Y x X = 29 x 36", jl.encode(f, 16, size=(29, 36)), ValueError),
                              # the same certain errors where the header does not fit the head
                              ("SOF0 (baseline DCT), marker FFC0", jl.encode(f, 16, sof=0xC0, head=jl.segment(0xFE, b"c" * 300)), NotImplementedError),
                              ("without SOS", jl.segment(0xFE, b"c" * 5000).join([plain[:2], plain[2:plain.index(b"\xff\xda")]]), ValueError)):
        message = same_error(dev, zc.dicom_zip([ok, ("bad.dcm", one(stream))]), "bad.dcm", exc)
        assert message.startswith(f"{ARCHIVE}: member 'bad.dcm': ") and text in message, text
    # refused before anything is extracted: BitsAllocated 32, more than 8192 columns
    wide = np.zeros((1, 1, dicom.JPEGLL_MAX_COLS + 2), dtype=np.uint16)
    assert f"at most {dicom.JPEGLL_MAX_COLS} samples" in same_error(dev, zc.dicom_zip([("w.dcm", one(plain, stack=wide))]), None)
    deep = rle.image_tags(frames[:1].astype(np.uint32))
    data = zc.dicom_zip([("d.dcm", rle._meta(jl.UID70) + deep + rle.encapsulate([plain]))])
    assert "BitsAllocated 32" in same_error(dev, data, None, NotImplementedError)


def check_scan_status(dev):
    """a scan cut short and a corrupted scan byte: ``check=True`` names member and frame, ``check=False`` leaves the flags"""
    frames = (120 + (jl.noise(41, (3, 12, 40), 8) >> 4)).astype(np.uint8)
    present = sorted(set().union(*(jl.encode_stats(f, 8)["categories"] for f in frames)))
    table = ([0, 0, len(present)] + [0] * 13, present)                             # 3-bit codes; 110 and 111 are in no table
    good = [jl.encode(f, 8, table=table) for f in frames]
    start = good[1].index(b"\xff\xda") + 10
    cut = good[1][:start + (len(good[1]) - start) // 2]
    found = next(t for t in (good[1][:i] + bytes([v]) + good[1][i + 1:] for i in range(start + 4, len(good[1]) - 2) for v in (0xB7, 0xDB, 0x6D)
                             if good[1][i - 1] != 0xFF) if jl.ref_decode(t, 12, 40)[1] == 4)
    for middle, flag in ((cut, 2), (found, 4), (good[1], 0)):
        files = [(f"f{k}.dcm", rle._meta(jl.UID70) + rle.image_tags(frames[k:k + 1]) + rle.encapsulate([s])) for k, s in enumerate((good[0], middle, good[2]))]
        data = zc.dicom_zip(files)
        x, _, _ = dicom.load_zip(data, device=dev, encapsulated=True, check=False, raw_pixels=True)
        assert x._pl_status.cpu().tolist() == [0, flag, 0]
        got = to_np(x)
        assert np.array_equal(got[0], frames[0]) and np.array_equal(got[2], frames[2])
        if flag:
            message = same_error(dev, data, "f1.dcm")
            assert message.startswith(f"{ARCHIVE}: member 'f1.dcm', frame 1 of the stack: JPEG Lossless Pixel Data: ")
            same_error(dev, data, "f1.dcm", dtype=np.int32, raw_pixels=True)
        else:
            same(dev, data, frames)
    # RLE: a segment that decodes to fewer bytes than the plane
    u16 = rle.container_frames(np.uint16, shape=EVEN)
    short = rle.rle_file(u16[1:2])
    frag, length = dicom.read_part10(short)[0].PixelDataFragments[0]
    offs = struct.unpack_from("<16I", short, frag)
    short = short[:frag + offs[2] + 8] + bytes([0x80]) * (length - offs[2] - 8) + short[frag + length:]     # no-ops: nothing decoded
    data = zc.dicom_zip([("f0.dcm", rle.rle_file(u16[:1])), ("f1.dcm", short)])
    x, _, _ = dicom.load_zip(data, device=dev, encapsulated=True, check=False)
    assert x._pl_status.cpu().tolist() == [0, 2]
    assert f"({ARCHIVE}: member 'f1.dcm', frame 1 of the stack)" in same_error(dev, data, "f1.dcm")
    same_error(dev, data, "f1.dcm", dtype=np.int32, raw_pixels=True)


def check_kinds_and_defaults(dev):
    frames = rle.container_frames(np.uint16, shape=EVEN)
    jp, rl, nat = ("j.dcm", jl.jpegll_file(frames[:1])), ("r.dcm", rle.rle_file(frames[1:2])), ("n.dcm", rle.native_file(frames[2:3]))
    for files, text in (([jp, nat], "JPEG Lossless files are mixed"), ([rl, jp], "JPEG Lossless files are mixed"),
                        ([nat, rl], "native and RLE Lossless files are mixed"), ([nat, jp, rl], "JPEG Lossless files are mixed")):
        assert text in same_error(dev, zc.dicom_zip(files), None)
    # native members with the keyword: what they always were
    native = one_each(frames, lambda f, k: rle.native_file(f))
    same(dev, zc.dicom_zip(native), frames)
    # another encapsulated syntax keeps today's refusal, with and without the keyword
    other = ("ls.dcm", rle.rle_file(frames[:1], uid="1.2.840.10008.1.2.4.80"))
    for kw in (dict(encapsulated=True), {}):
        with pytest.raises(NotImplementedError, match="member 'ls.dcm': " + TODAY_ENCAP):
            dicom.load_zip(zc.dicom_zip([nat, other]), device=dev, **kw)
    # the defaults: exactly today's two refusals for the archives that load with the keyword
    for files, text in (([rl], "member 'r.dcm': " + TODAY_RLE), ([jp], "member 'j.dcm': " + TODAY_ENCAP)):
        data = zc.dicom_zip([nat] + files)
        for kw in ({}, dict(encapsulated=False)):
            with pytest.raises(NotImplementedError, match=text):
                dicom.load_zip(data, device=dev, **kw)
        same(dev, zc.dicom_zip(files), None)
    with pytest.raises(ValueError, match="differ in pixel format or frame size"):
        dicom.load_zip(zc.dicom_zip([jp, ("w.dcm", jl.jpegll_file(frames[:1, :, :-1]))]), device=dev, encapsulated=True)
    # verify: a damaged pixel byte inside a stored RLE member
    data = zc.dicom_zip([("r0.dcm", rle.rle_file(frames[:1])), rl], kinds=[zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED])
    m = zc.zipstack.read_zip(data)[1]
    at = m.data_offset + m.size - 20                                              # inside the last segment, before the delimiter
    bad = zc.patched(data, at, "<B", data[at] ^ 1)
    with pytest.raises(zipfile.BadZipFile, match="Bad CRC-32 for file 'r.dcm'"):
        dicom.load_zip(bad, device=dev, encapsulated=True)
    x, _, _ = dicom.load_zip(bad, device=dev, encapsulated=True, verify=False, check=False)
    assert np.array_equal(to_np(x)[0], frames[0])


# ---- 7: index_encapsulated on hand-built buffers -----------------------------------------------------------------------------
def walk_items(buf: bytes, pos: int, end: int):
    """PS3.5 A.4 restated: -> (status, [(payload, length, tag)], table entries) of the items from ``pos`` up to ``end``"""
    frags, table = [], None
    while True:
        if end - pos < 8:
            return dicom.ENCAP_MALFORMED | dicom.ENCAP_NO_DELIMITER, frags, table or []
        tag, ln = struct.unpack_from("<II", buf, pos)
        if tag == 0xE0DDFFFE:
            return (0 if table is not None else dicom.ENCAP_TABLE), frags, table or []
        if tag != 0xE000FFFE or ln == 0xFFFFFFFF or ln > end - pos - 8:
            return dicom.ENCAP_MALFORMED, frags, table or []
        if table is None:
            if ln % 4:
                return dicom.ENCAP_TABLE | dicom.ENCAP_TABLE_LENGTH, frags, []
            table = list(struct.unpack_from(f"<{ln // 4}I", buf, pos + 8))
        else:
            frags.append((pos + 8, ln, pos))
        pos += 8 + ln


def item(payload: bytes) -> bytes:
    return struct.pack("<HHI", 0xFFFE, 0xE000, len(payload)) + payload


DELIMITER = struct.pack("<HHI", 0xFFFE, 0xE0DD, 0)
SENTINEL = 0xA5


def run_index(dev, buf: bytes, first, end, cap, tcap, head=H):
    """the kernel on a sentinel-filled block -> host views (frags, heads, info, table); compared with ``walk_items``"""
    need = dicom._lib.load().pl_dicom_encap_index_bytes(len(first), cap, tcap, head)
    block = torch.full((need,), SENTINEL, dtype=torch.uint8).to(dev)
    index = dicom.index_encapsulated(np.frombuffer(buf, dtype=np.uint8), first, end, cap, tcap, head_bytes=head, device=dev, block=block)
    frags, heads, info, table = index.host()
    assert [tuple(v.shape) for v in index.views()] == [(len(first), cap, 3), (len(first), cap, head), (len(first), 4), (len(first), tcap)]
    untouched64 = int.from_bytes(bytes([SENTINEL]) * 8, "little", signed=True)
    for m, (lo, hi) in enumerate(zip(first, end)):
        if lo < 0 or hi < lo or hi > len(buf):
            assert info[m, 0] == dicom.ENCAP_DESCRIPTOR
            assert (frags[m] == untouched64).all() and (heads[m] == SENTINEL).all() and (table[m].view(np.uint8) == SENTINEL).all()
            assert (info[m, 1:].view(np.uint8) == SENTINEL).all()
            continue
        status, want, entries = walk_items(buf, lo, hi)
        if len(want) > cap or len(entries) > tcap:
            status |= dicom.ENCAP_CAPACITY
        assert info[m].tolist() == [status, len(want), len(entries), 0], (m, info[m].tolist(), status)
        k = min(len(want), cap)
        assert frags[m, :k].tolist() == [list(w) for w in want[:k]] and (frags[m, k:] == untouched64).all()
        assert table[m, :min(len(entries), tcap)].tolist() == entries[:tcap]
        assert (table[m, min(len(entries), tcap):].view(np.uint8) == SENTINEL).all()
        for j, (at, ln, _) in enumerate(want[:k]):
            assert heads[m, j].tobytes() == buf[at:at + min(ln, head)] + bytes(head - min(ln, head)), (m, j)
        assert (heads[m, k:] == SENTINEL).all()
    return frags, heads, info, table


def check_index_kernel(dev):
    rng = np.random.default_rng(77)
    lengths = [0, 1, 63, 64, 65, H - 1, H, H + 1, 4 * H]
    buf, first, end = b"", [], []
    for r in range(16):                                                             # every residue mod 16 of the first item
        buf += bytes(rng.integers(0, 256, (r - len(buf) - 3) % 16 + 3, dtype=np.uint8))
        assert len(buf) % 16 == r
        first.append(len(buf))
        table = struct.pack(f"<{r % 3}I", *range(r % 3))
        some = lengths[r % 9:] + lengths[:r % 9] if r else []                       # member 0: the table and the delimiter only
        buf += item(table) + b"".join(item(bytes(rng.integers(0, 256, n, dtype=np.uint8))) for n in some) + DELIMITER
        end.append(len(buf) + (r % 2) * 5)                                          # bytes behind the delimiter are not looked at
        buf += bytes(5)
    # the last member ends exactly at the buffer's end
    first.append(len(buf))
    buf += item(b"") + item(b"last") + DELIMITER
    end.append(len(buf))
    frags, heads, info, _ = run_index(dev, buf, first, end, 12, 4)
    assert info[0].tolist() == [0, 0, 0, 0] and info[1, 1] == 9 and info[-1].tolist() == [0, 1, 0, 0] and not info[:, 0].any()
    # descriptors outside the buffer: bit 0, the slots untouched; the neighbours unharmed
    run_index(dev, buf, [first[1], -8, first[2], first[3], len(buf) + 1, first[4]], [end[1], 40, len(buf) + 1, first[3] - 1, len(buf) + 9, end[4]], 12, 4)
    # capacity: bit 3, full counts, the slots within cap correct, nothing beyond
    _, _, info, _ = run_index(dev, buf, first[:4], end[:4], 4, 1)
    assert (info[1:, 0] == dicom.ENCAP_CAPACITY).all() and info[1, 1] == 9 and info[2, 2] == 2
    run_index(dev, buf, first[:4], end[:4], 16, 2, head=64)
    # malformed: each stops the walk where it is, with what came before it stored
    base = item(struct.pack("<I", 0)) + item(b"abcdef")
    bad = [base, base + DELIMITER[:7], base + struct.pack("<HHI", 0xFFFE, 0xE00D, 0) + DELIMITER, base + struct.pack("<HHI", 0xFFFE, 0xE000, 0xFFFFFFFF),
           base + struct.pack("<HHI", 0xFFFE, 0xE000, 9) + bytes(8), item(b"123456") + DELIMITER, DELIMITER, item(b"") + item(b"ab"), b""]
    buf, first, end = b"", [], []
    for b in bad:
        first.append(len(buf))
        buf += b
        end.append(len(buf))
    buf += DELIMITER * 4                                                            # what a walk that left its window would find
    _, _, info, _ = run_index(dev, buf, first, end, 4, 2)
    E = dicom
    assert info[:, 0].tolist() == [E.ENCAP_MALFORMED | E.ENCAP_NO_DELIMITER] * 2 + [E.ENCAP_MALFORMED] * 3 + [E.ENCAP_TABLE | E.ENCAP_TABLE_LENGTH, E.ENCAP_TABLE] + \
        [E.ENCAP_MALFORMED | E.ENCAP_NO_DELIMITER] * 2
    # an item length of 0xFFFFFFFE near the end of the buffer: no hop, bit 1
    tail = bytes(rng.integers(0, 256, 1000, dtype=np.uint8)) + item(b"") + struct.pack("<HHI", 0xFFFE, 0xE000, 0xFFFFFFFE) + b"xy"
    _, _, info, _ = run_index(dev, tail, [1000], [len(tail)], 4, 1)
    assert info[0].tolist() == [dicom.ENCAP_MALFORMED, 0, 0, 0]


def check_index_far_offsets(dev):
    """GPU only: offsets beyond 2^31 -- a member whose first item lies past 2 GiB, and a length of 0xFFFFFFFE there"""
    size = (1 << 31) + 4096
    buf = torch.zeros(size, dtype=torch.uint8, device=dev)
    body = item(struct.pack("<I", 0)) + item(b"far away") + DELIMITER
    evil = item(b"") + struct.pack("<HHI", 0xFFFE, 0xE000, 0xFFFFFFFE)
    at = (1 << 31) + 101
    buf[at:at + len(body)] = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(dev)
    buf[at + 1000:at + 1000 + len(evil)] = torch.frombuffer(bytearray(evil), dtype=torch.uint8).to(dev)
    frags, heads, info, table = dicom.index_encapsulated(buf, [at, at + 1000], [at + len(body), size], 2, 1, device=dev).host()
    assert info.tolist() == [[0, 1, 1, 0], [dicom.ENCAP_MALFORMED, 0, 0, 0]]
    assert frags[0, 0].tolist() == [at + 20, 8, at + 12] and heads[0, 0, :9].tobytes() == b"far away\x00"


# ---- 8: copy_ranges against numpy --------------------------------------------------------------------------------------------
def run_copy(dev, src: np.ndarray, dst_size: int, ranges):
    dst = torch.full((dst_size,), SENTINEL, dtype=torch.uint8).to(dev)
    table = np.asarray(ranges, dtype=np.int64).reshape(-1, 3)
    status = dicom.copy_ranges(src, dst, table[:, 0], table[:, 1], table[:, 2], device=dev)
    want, flags = np.full(dst_size, SENTINEL, dtype=np.uint8), []
    for s, n, d in table.tolist():
        ok = s >= 0 and n >= 0 and d >= 0 and s + n <= src.size and d + n <= dst_size
        flags.append(0 if ok else 1)
        if ok:
            want[d:d + n] = src[s:s + n]
    assert status.cpu().tolist() == flags
    got = to_np(dst)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def check_copy_kernel(dev):
    rng = np.random.default_rng(78)
    src = rng.integers(0, 256, 40000, dtype=np.uint8)
    src[src == SENTINEL] = 0
    lengths = list(range(71)) + [255, 256, 257, 4099]
    # every pair of residues mod 16, the lengths dealt round: disjoint destination slots of 4352 bytes
    ranges = [(1552 + 16 * ((16 * a + b) % 37) + a, lengths[(16 * a + b) % len(lengths)], 4352 * (16 * a + b) + 16 + b)
              for a in range(16) for b in range(16)]
    run_copy(dev, src, 4352 * 256, ranges)
    # every length at one odd pair of residues, and at the aligned pair
    for a, b in ((5, 11), (0, 0), (3, 0), (0, 7)):
        run_copy(dev, src, 4352 * len(lengths), [(1600 + a, n, 4352 * k + 32 + b) for k, n in enumerate(lengths)])
    # the source's last bytes, at every misalignment of a source of any size mod 4; a destination used to its last byte
    for size in (4099, 4100, 4101, 4102):
        run_copy(dev, src[:size], 400, [(size - 70 - k, 70, 100 + 81 * k) for k in range(3)] + [(size - 33, 33, 400 - 33)])
    # ranges outside either buffer: flagged, nothing copied; the sound ones between them are
    run_copy(dev, src, 1000, [(-1, 4, 0), (0, 16, 100), (39990, 11, 200), (10, -1, 300), (10, 8, -4), (20, 40, 961), (5, 40, 960), (1 << 40, 1, 0),
                              (0, 1 << 40, 0), (0, 1, 1 << 40), (40000, 0, 1000)])


def check_copy_large(dev):
    """GPU only: one 3 MB range at odd alignment on both sides"""
    rng = np.random.default_rng(79)
    src = rng.integers(0, 256, 3_200_000, dtype=np.uint8)
    src[src == SENTINEL] = 1
    run_copy(dev, src, 3_100_000, [(4097, 3_000_001, 1027)])


# ---- 9: the C ABI -----------------------------------------------------------------------------------------------------------
def check_c_abi_argument_checks(dev):
    """pl_dicom_encap_index / pl_copy_ranges: invalid argument (1) for every null pointer, n = 0, negative sizes, misaligned
    buffers -- all before any launch (the pointers below are never dereferenced); pl_dicom_encap_index_bytes: -1 for the same"""
    lib = dicom._lib.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
    idx = torch.zeros(8, dtype=torch.int64, device=dev)
    st = torch.zeros(4, dtype=torch.int32, device=dev)
    p, q, s = buf.data_ptr(), idx.data_ptr(), st.data_ptr()

    def index(**kw):
        a = dict(bytes_=p, nbytes=64, first=q, end=q, n=1, cap=2, tcap=1, head=H, result=p)
        a.update(kw)
        return lib.pl_dicom_encap_index(a["bytes_"], a["nbytes"], a["first"], a["end"], a["n"], a["cap"], a["tcap"], a["head"], a["result"], None)

    for name in ("bytes_", "first", "end", "result"):
        assert index(**{name: None}) == 1 and b"null pointer" in lib.pl_last_error(), name
    assert index(n=0) == 1 and index(n=-1) == 1 and index(nbytes=-1) == 1 and index(cap=0) == 1 and index(tcap=0) == 1
    assert index(head=0) == 1 and index(head=H + 8) == 1 and index(head=2048) == 1 and index(result=p + 8) == 1 and b"16-byte" in lib.pl_last_error()
    size = lib.pl_dicom_encap_index_bytes
    assert size(0, 2, 1, H) == -1 and size(1, 0, 1, H) == -1 and size(1, 1, 0, H) == -1 and size(1, 1, 1, 8) == -1 and size(1, 1, 1, 1040) == -1
    # cap x (24 + head) + 16 + 4 x tcap bytes a member, rounded up to 16
    assert size(1, 1, 1, H) == 304 and size(3, 16, 2, H) == 13520 and size(2, 1, 1, 1024) == 2144

    def copy(**kw):
        a = dict(src=p, src_bytes=64, dst=p + 2048, dst_bytes=64, so=q, ln=q, do=q, n=1, max_len=64, status=s)
        a.update(kw)
        return lib.pl_copy_ranges(a["src"], a["src_bytes"], a["dst"], a["dst_bytes"], a["so"], a["ln"], a["do"], a["n"], a["max_len"], a["status"], None)

    for name in ("src", "dst", "so", "ln", "do", "status"):
        assert copy(**{name: None}) == 1 and b"null pointer" in lib.pl_last_error(), name
    assert copy(n=0) == 1 and copy(n=-2) == 1 and copy(src_bytes=-1) == 1 and copy(dst_bytes=-1) == 1 and copy(max_len=-1) == 1
    assert copy(src=p + 1) == 1 and b"4-byte" in lib.pl_last_error() and copy(dst=p + 2050) == 1
    header = (Path(__file__).resolve().parent.parent / "include" / "pylinac_hip.h").read_text()
    for entry in (r"int pl_dicom_encap_index\(", r"int64_t pl_dicom_encap_index_bytes\(", r"int pl_copy_ranges\(", r"#define PL_DICOM_ENCAP_HEAD 256"):
        assert re.search(entry, header), entry
    assert lib.pl_abi_version() == 3 and H == 256 and H % 16 == 0


# ---- GPU only: many waves side by side ---------------------------------------------------------------------------------------
def check_volume(dev, build):
    """64 deflated members of 128 x 128 int16"""
    frames = jl.ct_slices(64, 128)
    data = zc.dicom_zip([(f"CT{k:03d}.dcm", build(frames[k:k + 1])) for k in range(64)])
    x, metas, names = dicom.load_zip(data, device=dev, encapsulated=True)
    assert x.dtype == torch.int16 and len(names) == 64 and np.array_equal(to_np(x), frames)
    want, _ = dicom.load_frames(extracted(data, names), device=dev, jpeg_lossless=True)
    assert torch.equal(x, want)
