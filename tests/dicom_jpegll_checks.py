"""Shared checks of JPEG Lossless Pixel Data (1.2.840.10008.1.2.4.57 / .70, T.81 process 14) in pylinac_amd.dicom:
read_part10 / load_frames / DicomImage with ``jpeg_lossless=True``, decode_jpeg_lossless_frames and pl_dicom_jpegll_decode
(tests/test_emulated_dicom_jpegll.py on the CPU emulator, tests/test_gpu_dicom_jpegll.py on the MI355X).  Every comparison is
EQUALITY.

A lossless codec has its source as the reference.  The test files come from an ENCODER written here (T.81 Annex H, C.2:
prediction and differences with numpy, canonical codes, stuffing, restart markers); ``ref_decode`` is a decoder restated
separately from Annex H and F.2.2 -- it walks bits with the MINCODE / MAXCODE / VALPTR procedure and shares no table code with
the encoder; ``assert_reference`` pins it to the encoder's input on every case before the device is asked.  For 8-bit streams
PIL (libjpeg-turbo with lossless support) is a third, independent decoder.  For damaged streams ``ref_decode`` also states the
status the device must report (bit values 1 / 2 / 4 as in include/pylinac_hip.h).

The DICOM wrapping (``_meta``, ``image_tags``, ``encapsulate``, ``native_file``) is the one tests/dicom_rle_checks.py pins.
Shapes are the smallest at which the kernel can go wrong: a wave reconstructs 64 columns at a time, the input is staged in
windows of 1024 raw bytes of which every lane classifies 16."""
from __future__ import annotations

import io
import struct

import numpy as np
import pytest
import torch

import dicom_rle_checks as rle
from oracle import pylinac_oracle as o
from pylinac_amd import dicom

UID70, UID57 = "1.2.840.10008.1.2.4.70", "1.2.840.10008.1.2.4.57"
TODAY = "encapsulated \\(compressed\\) Pixel Data: decoded by pydicom's codec plug-ins"
to_np = dicom._to_numpy

# BITS[16], HUFFVAL: seven 3-bit codes, then one code each of 4 .. 13 bits (no all-ones code; category 16 is 13 bits long)
DEFAULT = ([0, 0, 7] + [1] * 10 + [0] * 3, [2, 3, 4, 5, 1, 6, 0, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16])
FLAT = ([0, 0, 0, 15, 2] + [0] * 11, list(range(17)))                          # 15 codes of 4 bits, 2 of 5
SKEWED = ([1] * 16, list(range(16)))                                       # lengths 1 .. 16 for categories 0 .. 15


# ---- the encoder (test files only) ----------------------------------------------------------------------------------------
def code_table(table) -> dict:
    """C.2: category -> (code, length)"""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def dht(tables: dict) -> bytes:
    return segment(0xC4, b"".join(bytes([tid]) + bytes(t[0]) + bytes(t[1]) for tid, t in tables.items()))


def differences(x: np.ndarray, precision: int, sel: int, pt: int, interval_rows: int) -> np.ndarray:
    """H.1.2: the differences modulo 2^16 of the samples ``x`` (already shifted right by Pt), as values -32768 .. 32767"""
    x = x.astype(np.int64)
    ra, rb, rc = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    ra[:, 1:], rb[1:], rc[1:, 1:] = x[:, :-1], x[:-1], x[:-1, :-1]
    px = {1: ra, 2: rb, 3: rc, 4: ra + rb - rc, 5: ra + ((rb - rc) >> 1), 6: rb + ((ra - rc) >> 1), 7: (ra + rb) >> 1}[sel]
    px = px.copy()
    px[:, 0] = rb[:, 0]
    firsts = np.arange(x.shape[0]) % (interval_rows or x.shape[0]) == 0
    px[firsts] = ra[firsts]
    px[firsts, 0] = 1 << (precision - pt - 1)
    return ((x - px + 32768) % 65536) - 32768


def pack_tokens(d: np.ndarray, codes: dict, stats: dict) -> bytes:
    """the tokens of one restart interval -> entropy-coded bytes, padded with 1-bits, FF bytes stuffed"""
    d = d.ravel()
    ssss = np.where(d == -32768, 16, np.ceil(np.log2(np.abs(d) + 1)).astype(np.int64))
    stats.setdefault("categories", set()).update(int(v) for v in np.unique(ssss))
    code = np.array([codes.get(s, (0, 0))[0] for s in range(17)], dtype=np.uint64)[ssss]
    clen = np.array([codes.get(s, (0, 0))[1] for s in range(17)], dtype=np.int64)[ssss]
    assert (clen > 0).all(), "the table lacks a category that occurs"
    stats["longest"] = max(stats.get("longest", 0), int(clen.max()))
    extra = np.where(ssss == 16, 0, ssss)
    v = np.where(d < 0, d + (1 << extra) - 1, d).astype(np.uint64) & ((np.uint64(1) << extra.astype(np.uint64)) - np.uint64(1))
    word, length = (code << extra.astype(np.uint64)) | v, clen + extra
    parts = []
    for a in range(0, d.size, 1 << 15):
        w, n = word[a:a + (1 << 15), None], length[a:a + (1 << 15), None]
        shift = n - 1 - np.arange(32)[None, :]
        parts.append(((w >> np.maximum(shift, 0).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)[shift >= 0])
    bits = np.concatenate(parts)
    stats["pad_bits"] = stats.get("pad_bits", []) + [int(-bits.size % 8)]
    data = np.packbits(np.concatenate([bits, np.ones(-bits.size % 8, dtype=np.uint8)]))
    return bytes(np.insert(data, np.flatnonzero(data == 0xFF) + 1, 0))


def encode(frame: np.ndarray, precision: int, sel: int = 1, pt: int = 0, restart: int = 0, table=DEFAULT, table_id: int = 0,
           tables: dict | None = None, head: bytes = b"", dri_first: bool = False, late_dht: bytes = b"", eoi: bool = True,
           sof: int = 0xC3, nf: int = 1, size=None, stats: dict | None = None) -> bytes:
    """one frame [rows, cols] of unsigned samples below 2^precision -> a T.81 lossless stream.  ``restart``: the interval in
    samples (rows * cols of them at most matter); ``tables``: {id: table} for the DHT segment (default {table_id: table});
    ``head``: segments between SOI and SOF; ``dri_first``: DRI before DHT instead of after it; ``late_dht``: a further DHT
    segment after the first; ``size``: (Y, X) for SOF instead of the frame's; ``stats`` receives the categories that occur,
    the longest code used and the pad bits of every interval"""
    stats = {} if stats is None else stats
    rows, cols = frame.shape
    x = frame.astype(np.int64) >> pt
    assert frame.min() >= 0 and frame.max() < 1 << precision and restart % cols == 0
    q = restart // cols
    d = differences(x, precision, sel, pt, q)
    codes = code_table(table)
    body = b""
    for k, a in enumerate(range(0, rows, q or rows)):
        body += (bytes([0xFF, 0xD0 + (k - 1) % 8]) if k else b"") + pack_tokens(d[a:a + (q or rows)], codes, stats)
    y, xx = size or (rows, cols)
    sof3 = segment(sof, bytes([precision]) + struct.pack(">HH", y, xx) + bytes([nf]) + b"".join(bytes([c + 1, 0x11, 0]) for c in range(nf)))
    dri = segment(0xDD, struct.pack(">H", restart)) if restart else b""
    tabs = dht(tables or {table_id: table}) + late_dht
    sos = segment(0xDA, bytes([1, 1, table_id << 4, sel, 0, pt]))
    return b"\xff\xd8" + head + sof3 + (dri + tabs if dri_first else tabs + dri) + sos + body + (b"\xff\xd9" if eoi else b"")


def unsigned(frames: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(frames).view({1: np.uint8, 2: np.uint16}[frames.dtype.itemsize])


def jpegll_file(frames: np.ndarray, uid: str = UID70, table: str = "empty", extra: bytes = b"", precision=None, **opts) -> bytes:
    """[F, rows, cols] frames of an 8- or 16-bit integer dtype -> a Part-10 file with JPEG Lossless Pixel Data"""
    p = precision or 8 * frames.dtype.itemsize
    return rle._meta(uid) + rle.image_tags(frames, extra) + rle.encapsulate([encode(f, p, **opts) for f in unsigned(frames)], table)


def fixture_as_jpegll(blob: np.ndarray, table: str = "empty", **opts):
    """an explicit-VR-little-endian native fixture of tests/golden/dicom.npz -> (the same data set with JPEG Lossless Pixel
    Data, the frames it encodes): every element between the File Meta group and Pixel Data is kept as it is"""
    raw = blob.tobytes()
    arr, _, start = o.dicom_pixel_array(blob)
    frames = arr.reshape((-1,) + arr.shape[-2:])
    pos = 132
    while struct.unpack_from("<H", raw, pos)[0] == 0x0002:
        vr = raw[pos + 4:pos + 6]
        pos += 12 + struct.unpack_from("<I", raw, pos + 8)[0] if vr in (b"OB", b"UN") else 8 + struct.unpack_from("<H", raw, pos + 6)[0]
    assert raw[start - 12:start - 8] == struct.pack("<HH", 0x7FE0, 0x0010)
    streams = [encode(f, 8 * frames.dtype.itemsize, **opts) for f in unsigned(frames)]
    return rle._meta(UID70) + raw[pos:start - 12] + rle.encapsulate(streams, table), frames


# ---- the reference decoder: T.81 Annex H and F.2.2, restated --------------------------------------------------------------
def ref_decode(jpeg: bytes, rows: int, cols: int):
    """a whole stream (SOI ... ) -> (uint16 [rows, cols] as the device stores them, status).  Status: 0, 2 the data ends
    before rows * cols samples, 4 a code that is not in the table / a wrong restart index / data where RSTn belongs"""
    pos, tables, interval, precision = 2, {}, 0, None
    while True:
        assert jpeg[pos] == 0xFF
        marker = jpeg[pos + 1]
        if marker == 0xFF:
            pos += 1
            continue
        length = int.from_bytes(jpeg[pos + 2:pos + 4], "big")
        seg = jpeg[pos + 4:pos + 2 + length]
        pos += 2 + length
        if marker == 0xC3:
            precision = seg[0]
        elif marker == 0xC4:
            while seg:
                n = sum(seg[1:17])
                tables[seg[0] & 15] = (list(seg[1:17]), list(seg[17:17 + n]))
                seg = seg[17 + n:]
        elif marker == 0xDD:
            interval = int.from_bytes(seg, "big")
        elif marker == 0xDA:
            return ref_decode_scan(jpeg[pos:], precision, seg[3], seg[5] & 15, interval, tables[seg[2] >> 4], rows, cols)


def ref_decode_scan(scan: bytes, precision: int, sel: int, pt: int, interval: int, table, rows: int, cols: int):
    bits, huffval = table
    # Figure C.1 / C.2: HUFFSIZE, HUFFCODE; Figure F.15: MINCODE, MAXCODE, VALPTR
    huffsize = [i for i in range(1, 17) for _ in range(bits[i - 1])]
    huffcode, code, k = [], 0, 0
    si = huffsize[0] if huffsize else 0
    while k < len(huffsize):
        while k < len(huffsize) and huffsize[k] == si:
            huffcode.append(code)
            code, k = code + 1, k + 1
        code, si = code << 1, si + 1
    mincode, maxcode, valptr, j = [0] * 17, [-1] * 17, [0] * 17, 0
    for i in range(1, 17):
        if bits[i - 1]:
            valptr[i], mincode[i] = j, huffcode[j]
            j += bits[i - 1]
            maxcode[i] = huffcode[j - 1]
    # the entropy-coded segments between markers, stuffing removed (F.1.2.3, B.1.1.5): [(data bytes, the marker that ended them)]
    pieces, cur, i = [], bytearray(), 0
    while cur is not None and i < len(scan):
        b = scan[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
        elif i + 1 >= len(scan):
            break
        elif scan[i + 1] == 0:
            cur.append(0xFF)
            i += 2
        elif scan[i + 1] == 0xFF:
            i += 1
        else:
            pieces.append((cur, scan[i + 1]))
            cur = bytearray() if 0xD0 <= scan[i + 1] <= 0xD7 else None
            i += 2
    if cur is not None:
        pieces.append((cur, 0))
    out = np.zeros((rows, cols), dtype=np.uint16)

    class Ended(Exception):
        pass

    piece, at = 0, 0                                                              # the piece in use, the next bit of it

    def nextbit():
        nonlocal at
        data = pieces[piece][0]
        if at >= 8 * len(data):
            raise Ended
        bit = (data[at >> 3] >> (7 - (at & 7))) & 1
        at += 1
        return bit

    per = interval // cols if interval else 0
    prev = cur_row = None
    try:
        for r in range(rows):
            restarted = r == 0
            if per and r and r % per == 0:
                at = (at + 7) & ~7
                if at < 8 * len(pieces[piece][0]):
                    return out, 4
                marker = pieces[piece][1]
                if not 0xD0 <= marker <= 0xD7:
                    return out, 2
                if marker != 0xD0 + (r // per - 1) % 8:
                    return out, 4
                piece, at, restarted = piece + 1, 0, True
                if piece >= len(pieces):
                    pieces.append((bytearray(), 0))
            prev, cur_row = cur_row, [0] * cols
            for c in range(cols):
                # F.2.2.3 DECODE
                code, i = nextbit(), 1
                while code > maxcode[i]:
                    i += 1
                    if i > 16:
                        return out, 4
                    code = (code << 1) + nextbit()
                ssss = huffval[valptr[i] + code - mincode[i]]
                # F.2.2.1 / H.1.2.2: RECEIVE and EXTEND; category 16 stands for 32768 alone
                if ssss == 16:
                    diff = 32768
                else:
                    v = 0
                    for _ in range(ssss):
                        v = (v << 1) + nextbit()
                    diff = v if ssss == 0 or v >= 1 << (ssss - 1) else v - (1 << ssss) + 1
                if restarted:
                    px = 1 << (precision - pt - 1) if c == 0 else cur_row[c - 1]
                elif c == 0:
                    px = prev[0]
                else:
                    a, b, cc = cur_row[c - 1], prev[c], prev[c - 1]
                    px = (a, b, cc, a + b - cc, a + ((b - cc) >> 1), b + ((a - cc) >> 1), (a + b) >> 1)[sel - 1]
                cur_row[c] = (px + diff) & 0xFFFF
                out[r, c] = (cur_row[c] << pt) & 0xFFFF
    except Ended:
        return out, 2
    return out, 0


def assert_reference(jpeg: bytes, frame: np.ndarray, pt: int = 0):
    """the restated decoder against the ENCODER'S INPUT (before anything is asked of the device)"""
    got, status = ref_decode(jpeg, *frame.shape)
    assert status == 0 and np.array_equal(got, (frame.astype(np.uint16) >> pt) << pt)


# ---- helpers --------------------------------------------------------------------------------------------------------------
def load(dev, files, **kw):
    x, metas = dicom.load_frames(files, device=dev, jpeg_lossless=True, **kw)
    return to_np(x), metas


def scan_tables(buf: bytes, where: list, rows: int, cols: int, bits: int):
    """streams at (offset, length) inside ``buf`` -> the arrays decode_jpeg_lossless_frames takes (the host's own parser)"""
    so, sl, par, huff = [], [], [], []
    for off, ln in where:
        start, length, p, t = dicom._jpegll_header(buf[off:off + ln], rows, cols, bits, "stream")
        so.append(off + start), sl.append(length), par.append(p), huff.append(list(t))
    return np.array(so, dtype=np.int64), np.array(sl, dtype=np.int64), np.array(par, dtype=np.int32), np.array(huff, dtype=np.uint8)


def decode_streams(dev, streams: list, rows: int, cols: int, bits: int = 16, lead: bytes = b"", **kw):
    buf, where = lead, []
    for s in streams:
        where.append((len(buf), len(s)))
        buf += s
    x = dicom.decode_jpeg_lossless_frames(np.frombuffer(buf, dtype=np.uint8), *scan_tables(buf, where, rows, cols, bits), rows, cols,
                                          bits, device=dev, **kw)
    return to_np(x), x._pl_status.cpu().tolist()


def assert_stream(dev, frame: np.ndarray, precision: int, **opts):
    """one frame through the encoder, the restated decoder and the kernel entry"""
    jpeg = encode(frame, precision, **opts)
    pt = opts.get("pt", 0)
    assert_reference(jpeg, frame, pt)
    bits = 8 if precision <= 8 else 16
    got, status = decode_streams(dev, [jpeg], *frame.shape, bits=bits)
    assert status == [0] and np.array_equal(got[0], ((frame >> pt) << pt).astype(got.dtype)), (precision, opts)
    return jpeg


def noise(seed: int, shape, precision: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    smooth = rng.integers(0, 1 << precision, 1) + np.cumsum(rng.integers(-9, 10, shape), axis=1) + np.cumsum(rng.integers(-5, 6, shape), axis=0)
    jumps = rng.integers(0, 1 << precision, shape) * (rng.random(shape) < 0.1)
    return ((smooth + jumps) % (1 << precision)).astype(np.uint16)


def ct_slices(n: int, size: int, seed: int = 7) -> np.ndarray:
    """CT-like int16 slices: air, a water disc, inserts, noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    r = np.hypot(yy - size / 2, xx - size / 2)
    out = []
    for k in range(n):
        base = np.where(r < 0.42 * size, 0.0, -1000.0)
        for ang, hu in ((0.3 + 0.1 * k, 900.0), (2.1, -200.0), (4.0, 340.0)):
            base = np.where(np.hypot(yy - size / 2 - 0.25 * size * np.sin(ang), xx - size / 2 - 0.25 * size * np.cos(ang)) < 0.05 * size, hu, base)
        out.append(np.clip(np.round(base + rng.normal(0, 12.0, base.shape)), -1024, 3071).astype(np.int16))
    return np.stack(out)


# ---- 1: every predictor x precision ---------------------------------------------------------------------------------------
PRECISIONS = [8, 10, 12, 16]
SELECTIONS = [1, 2, 3, 4, 5, 6, 7]


def check_predictor_precision(dev, sel: int, precision: int):
    for shape in ((5, 7), (1, 1), (1, 9), (9, 1)):
        assert_stream(dev, noise(sel * 100 + precision, shape, precision), precision, sel=sel)


# ---- 2: wave seams --------------------------------------------------------------------------------------------------------
SEAM_SHAPES = [(3, 63), (3, 64), (3, 65), (2, 129), (2, 257)]


def check_wave_seam(dev, sel: int, shape):
    assert_stream(dev, noise(sel * 1000 + shape[1], shape, 16), 16, sel=sel)
    assert_stream(dev, noise(sel * 1000 + shape[1] + 1, shape, 12), 12, sel=sel)


# ---- 3: category extremes -------------------------------------------------------------------------------------------------
def check_category_extremes(dev):
    cols = np.arange(70)[None, :] + np.zeros((3, 1), dtype=np.int64)
    for high in (32768, 65535):
        stats = {}
        frame = np.where(cols % 2 == 0, 0, high).astype(np.uint16)
        frame[1] = frame[1, ::-1] if frame.shape[1] % 2 else high - frame[1]      # the row above differs: Rb and Rc matter
        for sel in (1, 4, 7):
            assert_stream(dev, frame, 16, sel=sel, stats=stats)
        if high == 32768:
            assert 16 in stats["categories"]                                        # the token without extra bits
    stats = {}
    assert_stream(dev, np.full((4, 130), 1 << 15, dtype=np.uint16), 16, stats=stats)
    assert stats["categories"] == {0}
    stats = {}
    assert_stream(dev, np.full((4, 130), 40000, dtype=np.uint16), 16, sel=4, stats=stats)
    assert stats["categories"] <= {0, 13}


# ---- 4: Huffman tables ----------------------------------------------------------------------------------------------------
TABLES = ["flat", "skewed", "occurring only", "ids 0-3, SOS selects 2, id 2 redefined"]


def check_table(dev, kind: str):
    frame = noise(11, (6, 70), 16)
    stats = {}
    if kind == "flat":
        assert_stream(dev, frame, 16, table=FLAT, stats=stats)
        assert stats["longest"] == 5
    elif kind == "skewed":
        frame = (frame >> 1).astype(np.uint16)                                      # 15 bits: the categories 0 .. 15 of SKEWED
        frame[2, 5], frame[2, 6] = 0, 32767                                         # a difference of category 15: the 16-bit code
        assert_stream(dev, frame, 15, table=SKEWED, stats=stats)
        assert stats["longest"] == 16
    elif kind == "occurring only":
        present = sorted(encode_stats(frame, 16)["categories"])
        bits = [0] * 16
        bits[4] = len(present)                                                      # 5-bit codes for what occurs, the rest undefined
        table = (bits, present)
        assert len(present) < 17
        assert_stream(dev, frame, 16, table=table, stats=stats)
        assert stats["longest"] == 5
    else:
        other = ([0, 0, 0, 0, 17] + [0] * 11, list(range(16, -1, -1)))
        tables = {0: other, 1: FLAT, 2: other, 3: SKEWED}
        frame[3, 10], frame[3, 11] = 0, 32768                                       # category 16: the 13-bit code of DEFAULT
        jpeg = assert_stream(dev, frame, 16, table=DEFAULT, table_id=2, tables=tables, late_dht=dht({2: DEFAULT, 1: other}), stats=stats)
        assert jpeg.count(b"\xff\xc4") == 2 and stats["longest"] == 13              # category 16 occurs: the longest code of DEFAULT


def encode_stats(frame, precision, **opts) -> dict:
    stats = {}
    encode(frame, precision, table=FLAT, stats=stats, **opts)
    return stats


# ---- 5: byte stuffing -----------------------------------------------------------------------------------------------------
def check_byte_stuffing(dev):
    # category 8 with the code 1111 (FLAT's 15th is 1110; give 8 the code 1111 through a table of 16 4-bit codes) and extra
    # bits 1111 1111: a difference of +255 is the byte FF when it is byte-aligned
    table = ([0, 0, 0, 16] + [0] * 12, [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 8])
    rng = np.random.default_rng(5)
    d = np.where(rng.random((6, 300)) < 0.5, 255, -255)
    d[-1, -1] = 255                                                                # the last token of the scan: FF 00 before EOI
    first = (1 << 15) + np.cumsum(d[:, 0])                                         # first columns are predicted by Rb
    frame = ((first[:, None] + np.concatenate([np.zeros((6, 1), dtype=np.int64), np.cumsum(d[:, 1:], axis=1)], axis=1)) % 65536).astype(np.uint16)
    jpeg = assert_stream(dev, frame, 16, table=table)
    start = jpeg.index(b"\xff\xda") + 10
    scan = jpeg[start:-2]
    at = [i for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] == 0]
    assert len(at) >= 10 and {i % 4 for i in at} == {0, 1, 2, 3} and len(scan) > 1024
    assert scan.endswith(b"\xff\x00") and jpeg.endswith(b"\xff\x00\xff\xd9")
    # the scan at every alignment of the buffer; without EOI the stuffed byte ends the window itself
    for lead in range(4):
        for stream in (jpeg, jpeg[:-2]):
            got, status = decode_streams(dev, [stream], 6, 300, lead=b"\x5a" * lead)
            assert status == [0] and np.array_equal(got[0], frame), lead


# ---- 6: restart intervals -------------------------------------------------------------------------------------------------
def check_restart_intervals(dev):
    frame = noise(21, (20, 6), 12)
    for sel in (1, 7):
        for rows_per in (1, 3, 20):
            stats = {}
            jpeg = assert_stream(dev, frame, 12, sel=sel, restart=6 * rows_per, stats=stats)
            markers = [jpeg[i + 1] for i in range(jpeg.index(b"\xff\xda"), len(jpeg) - 2) if jpeg[i] == 0xFF and 0xD0 <= jpeg[i + 1] <= 0xD7]
            assert markers == [0xD0 + k % 8 for k in range((20 - 1) // rows_per)]
            if rows_per == 1:
                assert 0xD7 in markers and markers[8] == 0xD0 and any(stats["pad_bits"][:-1])   # wraps past D7; padding before RSTn
    # an interval larger than the frame, and the same rows in a frame wide enough for several wave passes
    assert_stream(dev, frame, 12, restart=6 * 40)
    wide = noise(22, (7, 130), 16)
    for sel in (1, 4, 6):
        assert_stream(dev, wide, 16, sel=sel, restart=130 * 2)


# ---- 7: point transform ---------------------------------------------------------------------------------------------------
def check_point_transform(dev):
    for precision in (8, 16):
        for pt in (1, 3):
            for sel in (1, 5, 7):
                frame = noise(pt * 10 + sel, (5, 67), precision)
                assert (frame & ((1 << pt) - 1)).any()
                assert_stream(dev, frame, precision, sel=sel, pt=pt)


# ---- 8: header variety ----------------------------------------------------------------------------------------------------
def check_header_variety(dev):
    frame = noise(31, (9, 11), 16).astype(np.uint16)
    head = segment(0xE0, b"JFIF\x00\x01\x02\x00\x00\x01\x00\x01\x00\x00") + segment(0xFE, b"a comment \xff\xc0 with marker bytes inside")
    streams = {"APP0 + COM": encode(frame, 16, head=head), "DRI before DHT": encode(frame, 16, restart=22, dri_first=True),
               "DRI after DHT": encode(frame, 16, restart=22), "no EOI": encode(frame, 16, eoi=False)}
    odd = next(s for s in (encode(frame, 16, sel=k) for k in range(1, 8)) if len(s) % 2)
    streams["odd length, pad byte"] = odd
    for name, jpeg in streams.items():
        assert_reference(jpeg, frame)
        got, status = decode_streams(dev, [jpeg], 9, 11)
        assert status == [0] and np.array_equal(got[0], frame), name
        file = rle._meta(UID70) + rle.image_tags(frame[None]) + rle.encapsulate([jpeg])
        assert np.array_equal(load(dev, [file], raw_pixels=True)[0][0], frame), name


# ---- 9: the kernel entry --------------------------------------------------------------------------------------------------
CONTAINERS = [np.uint8, np.int8, np.uint16, np.int16]


def check_container_kernel_entry(dev, dtype):
    frames = rle.container_frames(dtype)
    ib, (n, rows, cols) = frames.dtype.itemsize, frames.shape
    rng = np.random.default_rng(5)
    buf, where = b"", []
    for k, f in enumerate(unsigned(frames)):
        jpeg = encode(f, 8 * ib, sel=(1, 4, 6, 7)[k], table=(DEFAULT, FLAT)[k % 2])
        assert_reference(jpeg, f)
        scan_at = jpeg.index(b"\xff\xda") + 10
        buf += rng.integers(0, 256, (k - len(buf) - scan_at) % 4 + 4, dtype=np.uint8).tobytes()
        where.append((len(buf), len(jpeg)))
        buf += jpeg
    raw = np.frombuffer(buf, dtype=np.uint8)
    so, sl, par, huff = scan_tables(buf, where, rows, cols, 8 * ib)
    assert {int(v) % 4 for v in so} == {0, 1, 2, 3}
    kw = dict(rows=rows, cols=cols, bits_allocated=8 * ib, pixel_representation=int(frames.dtype.kind == "i"), device=dev)
    fb = rows * cols * ib
    guard = torch.full(((n + 2) * fb,), 0x5A, dtype=torch.uint8).to(dev)
    native = guard[fb:(n + 1) * fb].view(n, fb)
    x = dicom.decode_jpeg_lossless_frames(raw, so, sl, par, huff, native=native, **kw)
    assert x._pl_status.cpu().tolist() == [0] * n
    got = to_np(x)
    assert got.dtype == frames.dtype and np.array_equal(got, frames)
    edge = guard.cpu().numpy()
    assert (edge[:fb] == 0x5A).all() and (edge[(n + 1) * fb:] == 0x5A).all()      # nothing outside the frames' slots
    # device tensors are used in place; float64 with the fused rescale and float32 go through pl_dicom_decode
    on = [torch.from_numpy(a.copy()).to(dev) for a in (raw, so, sl, par, huff)]
    x = dicom.decode_jpeg_lossless_frames(*on, out="float64", rescale=(1.25, -1000.5), **kw)
    want = frames.astype(np.float64) * 1.25
    want += -1000.5
    assert np.array_equal(x.cpu().numpy(), want)
    assert np.array_equal(dicom.decode_jpeg_lossless_frames(raw, so, sl, par, huff, out="float32", **kw).cpu().numpy(), frames.astype(np.float32))


# ---- 10: the loader equals the native load --------------------------------------------------------------------------------
FIXTURES = ["u16_explicit", "u16_explicit_shifted", "u16_sequence", "i16_ct", "u16_stored12_dirty", "i16_stored12_dirty",
            "u8_multiframe", "u8_odd", "i8", "u16_inverted_sign", "u16_epid_tags"]


def same_answer(dev, native_files, jpeg_files, **kw):
    try:
        want, _ = rle.load(dev, native_files, **kw)
    except NotImplementedError as e:
        with pytest.raises(NotImplementedError, match=str(e)[:30]):
            load(dev, jpeg_files, **kw)
        return None
    got, _ = load(dev, jpeg_files, **kw)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), kw
    return got


def check_loader_fixture(golden, dev, name):
    blob = rle.explicit_fixtures(golden)[name]
    file, frames = fixture_as_jpegll(blob, sel=1 + len(name) % 7)
    meta, data = dicom.read_part10(file, jpeg_lossless=True)
    for f, frag in zip(unsigned(frames), meta.PixelDataFragments):
        assert_reference(bytes(data[frag[0]:frag[0] + frag[1]]), f)
    raw, _ = load(dev, [file], raw_pixels=True)
    assert raw.dtype == frames.dtype and np.array_equal(raw, frames)               # pixel_array itself
    for kw in rle.loader_keywords(name):
        same_answer(dev, [blob.tobytes()], [file], **kw)


def check_loader_rescale_per_file(golden, dev):
    """a series (one slope and intercept: the fused float64 form) and files that differ (decoded once, rescaled file by file)"""
    blob = rle.explicit_fixtures(golden)["i16_ct"].tobytes()
    at = blob.index(struct.pack("<HH2s", 0x0028, 0x1053, b"DS")) + 8
    assert blob[at:at + 3] == b"1.5"
    natives = [blob, blob[:at] + b"2.5" + blob[at + 3:], blob]
    files = [fixture_as_jpegll(np.frombuffer(b, dtype=np.uint8), sel=k + 1)[0] for k, b in enumerate(natives)]
    for kw in (dict(), dict(dtype=np.float32), dict(raw_pixels=True), dict(invert_pixels=True)):
        got = same_answer(dev, natives, files, **kw)
        same_answer(dev, [blob, blob], [files[0], files[2]], **kw)
    assert got.dtype == np.float64 and not np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


# ---- 11: fragments and stacks ---------------------------------------------------------------------------------------------
def split_file(frames, cuts, table="empty", uid=UID70, **opts):
    """every frame's stream cut into fragments at ``cuts`` (byte positions; the pieces but the last must be even for PS3.5's
    even-length items, so the cuts are even); a filled table names the first fragment of every frame"""
    items, firsts = [], []
    for f in unsigned(frames):
        jpeg = encode(f, 8 * frames.dtype.itemsize, **opts)
        firsts.append(len(items))
        edges = [0] + [c for c in cuts if c < len(jpeg)] + [len(jpeg)]
        items += [jpeg[a:b] for a, b in zip(edges, edges[1:])]
    body = rle.encapsulate(items)
    if table == "filled":
        sizes = [8 + len(i) + len(i) % 2 for i in items]
        offs = [sum(sizes[:k]) for k in firsts]
        bot = struct.pack(f"<{len(offs)}I", *offs)
        body = body[:12] + struct.pack("<HHI", 0xFFFE, 0xE000, len(bot)) + bot + body[20:]
    return rle._meta(uid) + rle.image_tags(frames) + body


def check_fragments_and_stacks(golden, dev, tmp_path):
    frames = rle.container_frames(np.uint16, n=2)
    for table in ("empty", "filled"):
        file = jpegll_file(frames, table=table, sel=4)
        meta, _ = dicom.read_part10(file, jpeg_lossless=True)
        assert len(meta.PixelDataFragments) == 2 and len(meta.PixelDataOffsetTable) == (2 if table == "filled" else 0)
        assert np.array_equal(load(dev, [file], raw_pixels=True)[0], frames), table
    # one frame in three fragments at odd places of its stream (header, table and scan are all cut); two frames, a filled table
    one = split_file(frames[:1], (6, 70, 300))
    assert len(dicom.read_part10(one, jpeg_lossless=True)[0].PixelDataFragments) == 4
    assert np.array_equal(load(dev, [one], raw_pixels=True)[0], frames[:1])
    two = split_file(frames, (50, 400), table="filled", sel=5)
    meta, _ = dicom.read_part10(two, jpeg_lossless=True)
    assert len(meta.PixelDataFragments) == 6 and len(meta.PixelDataOffsetTable) == 2
    assert np.array_equal(load(dev, [two], raw_pixels=True)[0], frames)
    # a stack of files that differ in predictor, table, point transform and restart interval == each file alone, permuted
    fx = rle.explicit_fixtures(golden)
    names = ["u16_explicit", "u16_explicit_shifted", "u16_sequence", "u16_epid_tags"]
    opts = [dict(sel=1), dict(sel=7, table=FLAT), dict(sel=4, restart=64 * 5), dict(sel=6, table=FLAT, restart=64)]
    files = [fixture_as_jpegll(fx[n], **opt)[0] for n, opt in zip(names, opts)]
    whole, metas = load(dev, files)
    assert np.array_equal(whole, rle.load(dev, [fx[n].tobytes() for n in names])[0])
    assert [m.TransferSyntaxUID for m in metas] == [UID70] * 4
    perm = [2, 0, 3, 1]
    assert np.array_equal(load(dev, [files[k] for k in perm])[0], whole[perm])
    mixed = jpegll_file(frames[:1], uid=UID57, sel=6), jpegll_file(frames[1:], uid=UID70, pt=2)
    got = load(dev, mixed, raw_pixels=True)[0]
    assert np.array_equal(got[0], frames[0]) and np.array_equal(got[1], (frames[1] >> 2) << 2)
    # paths, bytes and file objects
    path = tmp_path / "a.dcm"
    path.write_bytes(files[0])
    assert np.array_equal(load(dev, [str(path), path, io.BytesIO(files[0]), bytearray(files[0])])[0], whole[[0, 0, 0, 0]])


def check_dicom_image(golden, dev):
    fx = rle.explicit_fixtures(golden)
    for name in ("u16_epid_tags", "i16_ct", "u16_inverted_sign", "u8_multiframe"):
        file, _ = fixture_as_jpegll(fx[name])
        a, b = dicom.DicomImage(file, jpeg_lossless=True), dicom.DicomImage(fx[name].tobytes())
        assert a.array.dtype == b.array.dtype and a.array.shape == b.array.shape and np.array_equal(a.array, b.array), name
        assert np.array_equal(a.array, o.dicom_image_array(fx[name])), name
        assert a._original_dtype == b._original_dtype and a.metadata.TransferSyntaxUID == UID70
    with pytest.raises(NotImplementedError, match=TODAY):
        dicom.DicomImage(file)


# ---- 12: status is per frame ----------------------------------------------------------------------------------------------
def check_status(dev):
    frames = (120 + (noise(41, (3, 12, 40), 8) >> 4)).astype(np.uint8)            # small differences: few categories
    present = set(encode_stats(frames[1], 8, restart=80)["categories"])
    for f in frames:
        present |= encode_stats(f, 8)["categories"]
    present = sorted(present)
    assert len(present) <= 6
    table = ([0, 0, len(present)] + [0] * 13, present)                             # 3-bit codes; 110 and 111 are in no table
    good = [encode(f, 8, table=table) for f in frames]
    start = good[1].index(b"\xff\xda") + 10
    cut = good[1][:start + (len(good[1]) - start) // 2]
    # a byte of the scan whose change makes the restated decoder meet a code that is not in the table
    found = None
    for i in range(start + 4, len(good[1]) - 2):
        for value in (0xB7, 0xDB, 0x6D):
            trial = good[1][:i] + bytes([value]) + good[1][i + 1:]
            if good[1][i - 1] != 0xFF and ref_decode(trial, 12, 40)[1] == 4:
                found = trial
                break
        if found:
            break
    assert found is not None
    restarts = encode(frames[1], 8, table=table, restart=80)
    at = restarts.index(b"\xff\xd1", start)
    wrong = restarts[:at + 1] + b"\xd3" + restarts[at + 2:]
    for middle, flag in ((cut, 2), (found, 4), (wrong, 4), (good[1], 0), (restarts, 0)):
        assert ref_decode(middle, 12, 40)[1] == flag
        files = [rle._meta(UID70) + rle.image_tags(frames[k:k + 1]) + rle.encapsulate([s]) for k, s in enumerate((good[0], middle, good[2]))]
        x, _ = dicom.load_frames(files, device=dev, check=False, raw_pixels=True, jpeg_lossless=True)
        assert x._pl_status.cpu().tolist() == [0, flag, 0]
        got = to_np(x)
        assert np.array_equal(got[0], frames[0]) and np.array_equal(got[2], frames[2])
        if flag:
            with pytest.raises(ValueError, match=r"file 1, frame 1 of the stack: JPEG Lossless"):
                dicom.load_frames(files, device=dev, jpeg_lossless=True)
            with pytest.raises(ValueError, match=r"file 1"):
                dicom.load_frames(files, device=dev, dtype=np.int32, raw_pixels=True, jpeg_lossless=True)
        else:
            assert np.array_equal(got[1], frames[1])
    # a window outside the buffer, an unsound parameter or table: bit 0 and the frame untouched
    buf, where = b"", []
    for s in good:
        where.append((len(buf), len(s)))
        buf += s
    raw = np.frombuffer(buf, dtype=np.uint8)
    so, sl, par, huff = scan_tables(buf, where, 12, 40, 8)
    oversubscribed = huff.copy()
    oversubscribed[1, :3] = (0, 0, 9)
    cases = [(so, -1), (so, len(buf) - 3), (sl, 1 << 40), (sl, -5), (so, 1 << 50), (par, (9, 1, 0, 0)), (par, (8, 0, 0, 0)),
             (par, (8, 8, 0, 0)), (par, (8, 1, 8, 0)), (par, (8, 1, 0, 41)), (huff, oversubscribed[1]), (huff, [18] + [0] * 15 + [0] * 17),
             (huff, [0, 1] + [0] * 14 + [17] + [0] * 16)]
    for which, value in cases:
        arrays = [a.copy() for a in (so, sl, par, huff)]
        next(a for a, b in zip(arrays, (so, sl, par, huff)) if b is which)[1] = value
        native = torch.full((3, 12 * 40), 0x5A, dtype=torch.uint8).to(dev)
        x = dicom.decode_jpeg_lossless_frames(raw, *arrays, 12, 40, 8, device=dev, native=native)
        assert x._pl_status.cpu().tolist() == [0, 1, 0], value
        got = to_np(x)
        assert np.array_equal(got[0], frames[0]) and np.array_equal(got[2], frames[2]) and (got[1] == 0x5A).all(), value


# ---- 13: refusals ---------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    frames = rle.container_frames(np.uint16, n=2)
    f = unsigned(frames)[0]

    def one(streams, stack=frames[:1], uid=UID70, table="empty"):
        return rle._meta(uid) + rle.image_tags(stack) + rle.encapsulate(streams, table)

    good = encode(f, 16)
    # without the keyword: today's refusal, in read_part10, load_frames and DicomImage
    for uid in (UID57, UID70):
        for call in (lambda b: dicom.load_frames([b], device=dev), dicom.read_part10, lambda b: dicom.read_part10(b, jpeg_lossless=False)):
            with pytest.raises(NotImplementedError, match=TODAY):
                call(one([good], uid=uid))
    # with it: the other encapsulated syntaxes keep today's message
    for uid in ("1.2.840.10008.1.2.4.50", "1.2.840.10008.1.2.4.80", "1.2.840.10008.1.2.4.90"):
        with pytest.raises(NotImplementedError, match=TODAY):
            load(dev, [one([good], uid=uid)])
    with pytest.raises(NotImplementedError, match="Deflated Explicit VR Little Endian"):
        load(dev, [one([good], uid="1.2.840.10008.1.2.1.99")])
    # processes other than Huffman-coded lossless, named by their marker
    for sof, word in ((0xC0, "SOF0"), (0xC1, "SOF1"), (0xC2, "SOF2"), (0xC9, "SOF9"), (0xCA, "SOF10"), (0xCB, "SOF11")):
        with pytest.raises(NotImplementedError, match=rf"file 0: {word} .*marker FF{sof:02X}"):
            load(dev, [one([encode(f, 16, sof=sof)])])
    for extra, word in ((segment(0xCC, b"\x00\x00"), "DAC"), (segment(0xDC, b"\x00\x1d"), "DNL")):
        with pytest.raises(NotImplementedError, match=rf"file 0: {word} .*marker"):
            load(dev, [one([encode(f, 16, head=extra)])])
    with pytest.raises(NotImplementedError, match="file 0: SOF3 with Nf = 3"):
        load(dev, [one([encode(f, 16, nf=3)])])
    spp3 = rle.image_tags(frames[:1]).replace(struct.pack("<HH2sHH", 0x0028, 0x0002, b"US", 2, 1), struct.pack("<HH2sHH", 0x0028, 0x0002, b"US", 2, 3))
    with pytest.raises(NotImplementedError, match="SamplesPerPixel = 1 only"):
        load(dev, [rle._meta(UID70) + spp3 + rle.encapsulate([good])])
    # malformed streams
    too_many = ([0, 0, 0, 14, 4] + [0] * 11, list(range(17)) + [3])
    oversubscribed = ([0, 0, 9] + [0] * 13, list(range(9)))
    bad_symbol = ([0, 0, 0, 2] + [0] * 12, [1, 17])
    cases = {
        "SOF3 states Y x X = 29 x 36": encode(f, 16, size=(29, 36)),
        "SOF3 states Y x X = 28 x 35": encode(f, 16, size=(28, 35)),
        "restart interval 36 is not a whole number of rows": good.replace(b"\xff\xc4", segment(0xDD, b"\x00\x24") + b"\xff\xc4", 1),
        "a DHT table of 18 symbols": good.replace(dht({0: DEFAULT}), dht({0: too_many})),
        "over-subscribed": good.replace(dht({0: DEFAULT}), dht({0: oversubscribed})),
        "holds the symbol 17": good.replace(dht({0: DEFAULT}), dht({0: bad_symbol})),
        "without SOS": good[:good.index(b"\xff\xda")],
        "EOI without SOS": good[:good.index(b"\xff\xda")] + b"\xff\xd9",
        "does not start with SOI": good[2:],
        "selects the Huffman table 1": encode(f, 16, table_id=1, tables={0: DEFAULT}),
        "lies outside the fragment": good[:good.index(b"\xff\xc4") + 10],
        "selection value 0": good.replace(segment(0xDA, bytes([1, 1, 0, 1, 0, 0])), segment(0xDA, bytes([1, 1, 0, 0, 0, 0]))),
    }
    for text, stream in cases.items():
        with pytest.raises(ValueError, match="file 0: .*" + text):
            load(dev, [one([stream])])
    with pytest.raises(ValueError, match="file 0: SOF3 precision 16 exceeds BitsAllocated = 8"):
        load(dev, [rle._meta(UID70) + rle.image_tags(frames[:1].astype(np.uint8)) + rle.encapsulate([good])])
    with pytest.raises(ValueError, match="point transform 2 at precision 2"):
        load(dev, [one([encode(f & 3, 2).replace(segment(0xDA, bytes([1, 1, 0, 1, 0, 0])), segment(0xDA, bytes([1, 1, 0, 1, 0, 2])))])])
    # fragment counts that fit no rule; tables that disagree
    with pytest.raises(ValueError, match="file 0: 3 JPEG fragments for NumberOfFrames = 2"):
        load(dev, [one([good, good, good], stack=frames)])
    with pytest.raises(ValueError, match="file 0: 1 JPEG fragments for NumberOfFrames = 2"):
        load(dev, [one([good], stack=frames)])
    with pytest.raises(ValueError, match="a Basic Offset Table of 2 entries for NumberOfFrames = 1"):
        load(dev, [one([good, good], table="filled")])
    ok = one([good, good], stack=frames, table="filled")
    at = ok.index(struct.pack("<HHI", 0xFFFE, 0xE000, 8)) + 12
    with pytest.raises(ValueError, match="Basic Offset Table disagrees"):
        load(dev, [ok[:at] + struct.pack("<I", 6 + len(good)) + ok[at + 4:]])
    # mixtures
    jp, rl, nat = jpegll_file(frames[:1]), rle.rle_file(frames[:1]), rle.native_file(frames[1:2])
    for files in ([jp, nat], [rl, jp], [nat, jp, rl]):
        with pytest.raises(ValueError, match="JPEG Lossless files are mixed with native or RLE Lossless files"):
            load(dev, files)
    with pytest.raises(ValueError, match="native and RLE Lossless files are mixed"):
        load(dev, [rl, nat])
    with pytest.raises(ValueError, match="differ in pixel format or frame size"):
        load(dev, [jp, jpegll_file(frames[:1, :, :-1])])
    # a frame wider than the kernel buffers: refused before anything is copied
    with pytest.raises(ValueError, match=f"at most {dicom.JPEGLL_MAX_COLS} samples"):
        dicom.decode_jpeg_lossless_frames(np.zeros(8, dtype=np.uint8), [0], [8], [[16, 1, 0, 0]], np.zeros((1, 33), dtype=np.uint8), 1,
                                          dicom.JPEGLL_MAX_COLS + 1, 16, device=dev)


# ---- 14: C-ABI argument checks --------------------------------------------------------------------------------------------
def check_c_abi_argument_checks(dev):
    """pl_dicom_jpegll_decode: unsupported (2) for bytes_per_sample other than 1 / 2 and cols over the limit, invalid argument
    (1) for n_frames outside 1 .. 65535, rows or cols < 1 and null pointers -- all before any launch (the pointers below are
    never dereferenced)"""
    import re
    from pathlib import Path

    from pylinac_amd import _lib

    lib = _lib.load()
    buf = torch.zeros(256, dtype=torch.uint8, device=dev)
    idx = torch.zeros(8, dtype=torch.int64, device=dev)
    st = torch.zeros(4, dtype=torch.int32, device=dev)
    p, q, s = buf.data_ptr(), idx.data_ptr(), st.data_ptr()
    limit = dicom.JPEGLL_MAX_COLS

    def call(n, rows, cols, bps=2, bytes_=p, native=p, params=q, huff=p, status=s, nbytes=256):
        return lib.pl_dicom_jpegll_decode(bytes_, nbytes, q, q, params, huff, n, rows, cols, bps, native, status, None, None)

    for bps in (0, 3, 4, -1):
        assert call(1, 4, 4, bps=bps) == 2 and b"unsupported bytes_per_sample" in lib.pl_last_error()
    assert call(1, 4, limit + 1) == 2 and b"unsupported cols" in lib.pl_last_error()
    assert call(0, 4, 4) == 1 and call(-1, 4, 4) == 1 and call(65536, 4, 4) == 1 and call(1, 0, 4) == 1 and call(1, 4, 0) == 1
    assert call(1, -4, 4) == 1 and call(1, 4, -4) == 1 and call(1, 4, 4, nbytes=-1) == 1
    for null in ("bytes_", "native", "params", "huff", "status"):
        assert call(1, 4, 4, **{null: None}) == 1 and b"null pointer" in lib.pl_last_error()
    work = lib.pl_dicom_jpegll_work_bytes
    assert work(0, 4, 4) == -1 and work(-1, 4, 4) == -1 and work(65536, 4, 4) == -1 and work(1, 0, 4) == -1 and work(1, 4, 0) == -1
    assert work(1, 4, limit + 1) == -1 and work(1, 4, limit) >= 0 and work(65535, 1, 1) >= 0
    header = (Path(__file__).resolve().parent.parent / "include" / "pylinac_hip.h").read_text()
    assert int(re.search(r"#define PL_DICOM_JPEGLL_MAX_COLS (\d+)", header).group(1)) == limit >= 4096


# ---- PIL as a third decoder of the 8-bit streams --------------------------------------------------------------------------
def check_pil_agrees(dev):
    from PIL import Image

    frame = (noise(51, (20, 70), 8)).astype(np.uint8)
    streams = [encode(frame, 8, sel=sel) for sel in SELECTIONS] + [encode(frame, 8, sel=1, restart=70), encode(frame, 8, sel=7, restart=210),
                                                                    encode(frame, 8, sel=4, table=([0, 0, 0, 14, 3] + [0] * 11, list(range(17))))]
    # (libjpeg-turbo refuses a table that uses the all-ones code, as FLAT does: 14 + 3 codes leave it free)
    try:
        probe = np.asarray(Image.open(io.BytesIO(streams[0])))
    except Exception as e:                                                         # a PIL whose libjpeg has no lossless support
        pytest.skip(f"the installed PIL does not open SOF3 streams ({e})")
    assert np.array_equal(probe, frame)
    for jpeg in streams:
        third = np.asarray(Image.open(io.BytesIO(jpeg)))
        got, status = decode_streams(dev, [jpeg], 20, 70, bits=8)
        assert status == [0] and np.array_equal(got[0], third) and np.array_equal(third, frame)
        assert np.array_equal(ref_decode(jpeg, 20, 70)[0], third)


# ---- 15: frames of clinical size (GPU only) -------------------------------------------------------------------------------
def check_ct_stack(dev):
    a, b = ct_slices(2, 512)
    files = [jpegll_file(s[None]) for s in (a, b)]
    x, metas = load(dev, [files[0], files[1], files[0]], raw_pixels=True)
    assert x.dtype == np.int16 and np.array_equal(x, np.stack([a, b, a]))


def check_large_frame(dev):
    frame = noise(61, (1024, 1024), 16)
    x, _ = load(dev, [jpegll_file(frame[None], sel=4)], raw_pixels=True)
    assert x.dtype == np.uint16 and np.array_equal(x[0], frame)
