"""Shared checks of RLE Lossless Pixel Data (1.2.840.10008.1.2.5) in pylinac_amd.dicom: read_part10's item walk,
load_frames / DicomImage, decode_rle_frames and pl_dicom_rle_decode (tests/test_emulated_dicom_rle.py on the CPU emulator,
tests/test_gpu_dicom_rle.py on the MI355X).  Every comparison is EQUALITY.

pydicom is in no environment of this build, so the reference is restated here byte for byte: ``rle_decode_segment`` is
pydicom 2.x ``pixel_data_handlers/rle_handler.py::_rle_decode_segment`` (the ten-line loop with its IndexError exit),
``rle_decode_frame`` its ``_rle_decode_frame`` for SamplesPerPixel 1 and little-endian output (PS3.5 Annex G).  The test
files come from a PackBits ENCODER written independently of it (planes most significant byte first, one row at a time, with
options for 0x80 no-ops, runs that cross rows and the pad byte); ``assert_reference`` pins the restated decoder to the
encoder's input on every case before the device is asked, so that no check is green because both sides err alike.

Shapes are the smallest at which the kernels can go wrong: a chunk is ``dicom.RLE_CHUNK`` input bytes, its entry offset one of
0 .. 128, pass 2 stages 64 table rows at a time (the 129-chunk stream of check_every_entry_offset takes three batches)."""
from __future__ import annotations

import struct
import warnings

import numpy as np
import pytest
import torch

from oracle import pylinac_oracle as o
from pylinac_amd import dicom

K = dicom.RLE_CHUNK
RLE_UID = "1.2.840.10008.1.2.5"
SHORT = "The amount of decoded RLE segment data doesn't match the expected amount"
PADDING = "non-conformant padding"


# ---- the reference: pydicom 2.x rle_handler, restated ---------------------------------------------------------------------
def rle_decode_segment(data: bytes) -> bytearray:
    """pydicom.pixel_data_handlers.rle_handler._rle_decode_segment"""
    data = bytearray(data)
    result = bytearray()
    pos = 0
    result_extend = result.extend
    try:
        while True:
            # header_byte is N + 1
            header_byte = data[pos] + 1
            pos += 1
            if header_byte > 129:
                # Extend by copying the next byte (-N + 1) times; however since using uint8 instead of int8 this is
                # (256 - N + 1) times
                result_extend(data[pos:pos + 1] * (258 - header_byte))
                pos += 1
            elif header_byte < 129:
                # Extend by literally copying the next (N + 1) bytes
                result_extend(data[pos:pos + header_byte])
                pos += header_byte
    except IndexError:
        pass
    return result


def rle_decode_frame(fragment: bytes, rows: int, cols: int, bits: int) -> bytes:
    """rle_handler._rle_decode_frame(data, rows, columns, nr_samples=1, nr_bits, segment_order='<'): the frame's
    little-endian bytes; ValueError for a wrong segment count or a short segment, a warning for a long one"""
    fragment = bytes(fragment)
    head = struct.unpack_from("<16L", fragment, 0)
    nr_segments = head[0]
    offsets = list(head[1:nr_segments + 1])
    bytes_per_sample = bits // 8
    if nr_segments != bytes_per_sample:
        raise ValueError(f"The number of RLE segments in the pixel data doesn't match the expected amount "
                         f"({nr_segments} vs. {bytes_per_sample} segments)")
    offsets.append(len(fragment))
    frame = bytearray(rows * cols * bytes_per_sample)
    for byte_offset in range(bytes_per_sample):
        segment = rle_decode_segment(fragment[offsets[byte_offset]:offsets[byte_offset + 1]])
        if len(segment) < rows * cols:
            raise ValueError(f"{SHORT} ({len(segment)} vs. {rows * cols} bytes)")
        if len(segment) != rows * cols:
            warnings.warn(f"The decoded RLE segment contains {PADDING} - {len(segment)} vs. {rows * cols} bytes expected")
        frame[bytes_per_sample - 1 - byte_offset::bytes_per_sample] = segment[:rows * cols]      # segment 0: the MSB
    return bytes(frame)


def walk_entries(segment: bytes) -> list:
    """the reference walk's control-byte positions -> the entry offset of every chunk of K input bytes the walk enters"""
    pos, n, first = 0, len(segment), {}
    while pos < n:
        first.setdefault(pos // K, pos % K)
        c = segment[pos]
        pos += 2 + c if c < 128 else (2 if c > 128 else 1)
    return [first[j] for j in sorted(first)]


# ---- the encoder (test files only) ----------------------------------------------------------------------------------------
def packbits_runs(a: np.ndarray) -> list:
    """one run of bytes -> PackBits runs: replicate runs (2 .. 128 equal bytes) and literal runs (1 .. 128 bytes)"""
    a = np.ascontiguousarray(a, dtype=np.uint8).ravel()
    n = a.size
    if n == 0:
        return []
    starts = np.concatenate([[0], np.flatnonzero(a[1:] != a[:-1]) + 1])
    lens = np.diff(np.concatenate([starts, [n]]))
    plural = np.flatnonzero(lens > 1)
    runs, i, m = [], 0, len(starts)
    while i < m:
        if lens[i] > 1:
            s, left = int(starts[i]), int(lens[i])
            while left:
                k = min(left, 128)
                runs.append(bytes([257 - k, a[s]]) if k > 1 else bytes([0, a[s]]))
                s, left = s + k, left - k
            i += 1
            continue
        q = int(np.searchsorted(plural, i))
        j = int(plural[q]) if q < len(plural) else m
        s, e = int(starts[i]), int(starts[j]) if j < m else n
        for t in range(s, e, 128):
            piece = a[t:min(t + 128, e)]
            runs.append(bytes([piece.size - 1]) + piece.tobytes())
        i = j
    return runs


def encode_segment(plane: np.ndarray, cross_rows: bool = False, noop_every: int = 0, pad: int | None = 0) -> bytes:
    """one byte plane [rows, cols] -> a segment: one row at a time (``cross_rows``: the whole plane as one run of bytes, which
    the standard forbids to encoders and decoders accept), a 0x80 no-op before every ``noop_every``-th run, padded to an even
    length with ``pad`` (None: no pad)"""
    rows = [plane.ravel()] if cross_rows else list(plane)
    runs = [r for row in rows for r in packbits_runs(row)]
    if noop_every:
        runs = [(b"\x80" if k % noop_every == 0 else b"") + r for k, r in enumerate(runs)]
    seg = b"".join(runs)
    if pad is not None and len(seg) % 2:
        seg += bytes([pad])
    return seg


def fragment_of(segments: list) -> bytes:
    offs, pos = [], 64
    for s in segments:
        offs.append(pos)
        pos += len(s)
    return struct.pack("<16L", len(segments), *(offs + [0] * (15 - len(offs)))) + b"".join(segments)


def encode_frame(frame: np.ndarray, **opts) -> bytes:
    """one frame [rows, cols] of a 1-, 2- or 4-byte integer dtype -> its RLE fragment (64-byte header + segments, MSB first)"""
    ib = frame.dtype.itemsize
    planes = np.ascontiguousarray(frame).view(np.uint8).reshape(frame.shape[0], frame.shape[1], ib)
    order = range(ib - 1, -1, -1) if frame.dtype.byteorder != ">" else range(ib)
    return fragment_of([encode_segment(planes[:, :, b], **opts) for b in order])


# ---- Part-10 files (explicit VR little endian) ----------------------------------------------------------------------------
def _el(group: int, element: int, vr: str, value: bytes) -> bytes:
    if len(value) % 2:
        value += b" " if vr not in ("UI", "OB", "OW") else b"\x00"
    if vr in ("OB", "OW", "SQ", "UN"):
        return struct.pack("<HH2sHI", group, element, vr.encode(), 0, len(value)) + value
    return struct.pack("<HH2sH", group, element, vr.encode(), len(value)) + value


def _meta(uid: str) -> bytes:
    body = _el(0x0002, 0x0010, "UI", uid.encode())
    return b"\x00" * 128 + b"DICM" + _el(0x0002, 0x0000, "UL", struct.pack("<I", len(body))) + body


def image_tags(frames: np.ndarray, extra: bytes = b"") -> bytes:
    """the group-0028 elements of a [F, rows, cols] stack (``extra``: encoded elements of group 0028 beyond 0103)"""
    f, rows, cols = frames.shape
    bits = 8 * frames.dtype.itemsize
    us = lambda v: struct.pack("<H", v)
    out = _el(0x0028, 0x0002, "US", us(1)) + _el(0x0028, 0x0004, "CS", b"MONOCHROME2")
    if f > 1:
        out += _el(0x0028, 0x0008, "IS", str(f).encode())
    out += _el(0x0028, 0x0010, "US", us(rows)) + _el(0x0028, 0x0011, "US", us(cols)) + _el(0x0028, 0x0100, "US", us(bits))
    out += _el(0x0028, 0x0101, "US", us(bits)) + _el(0x0028, 0x0102, "US", us(bits - 1))
    return out + _el(0x0028, 0x0103, "US", us(int(frames.dtype.kind == "i"))) + extra


def encapsulate(fragments: list, table: str = "empty") -> bytes:
    """(7FE0,0010) OB of undefined length: the Basic Offset Table (``table``: "empty" | "filled"), one item per fragment, the
    sequence delimiter (PS3.5 section A.4)"""
    items, offs, pos = [], [], 0
    for frag in fragments:
        frag = bytes(frag) + (b"\x00" if len(frag) % 2 else b"")
        offs.append(pos)
        items.append(struct.pack("<HHI", 0xFFFE, 0xE000, len(frag)) + frag)
        pos += 8 + len(frag)
    bot = struct.pack(f"<{len(offs)}I", *offs) if table == "filled" else b""
    return (struct.pack("<HH2sHI", 0x7FE0, 0x0010, b"OB", 0, 0xFFFFFFFF) + struct.pack("<HHI", 0xFFFE, 0xE000, len(bot)) + bot
            + b"".join(items) + struct.pack("<HHI", 0xFFFE, 0xE0DD, 0))


def native_file(frames: np.ndarray, extra: bytes = b"") -> bytes:
    return _meta("1.2.840.10008.1.2.1") + image_tags(frames, extra) + _el(0x7FE0, 0x0010, "OW", frames.astype(frames.dtype.newbyteorder("<")).tobytes())


def rle_file(frames: np.ndarray, extra: bytes = b"", table: str = "empty", uid: str = RLE_UID, **opts) -> bytes:
    return _meta(uid) + image_tags(frames, extra) + encapsulate([encode_frame(f, **opts) for f in frames], table)


def fixture_as_rle(blob: np.ndarray, table: str = "empty", **opts):
    """an explicit-VR-little-endian native fixture of tests/golden/dicom.npz -> (the same data set with RLE Lossless Pixel
    Data, the frames [F, rows, cols] it encodes): every element between the File Meta group and Pixel Data is kept as it is"""
    raw = blob.tobytes()
    arr, _, start = o.dicom_pixel_array(blob)
    frames = arr.reshape((-1,) + arr.shape[-2:])
    pos = 132
    while struct.unpack_from("<H", raw, pos)[0] == 0x0002:
        vr = raw[pos + 4:pos + 6]
        pos += 12 + struct.unpack_from("<I", raw, pos + 8)[0] if vr in (b"OB", b"UN") else 8 + struct.unpack_from("<H", raw, pos + 6)[0]
    assert raw[start - 12:start - 8] == struct.pack("<HH", 0x7FE0, 0x0010) and 0 <= len(raw) - start - frames.nbytes <= 1
    return _meta(RLE_UID) + raw[pos:start - 12] + encapsulate([encode_frame(f, **opts) for f in frames], table), frames


def explicit_fixtures(golden) -> dict:
    g = golden("dicom")
    names = [k[len("file__"):] for k in g.files if k.startswith("file__")]
    keep = {n: g["file__" + n] for n in names if not any(t in n for t in ("implicit", "big_endian"))}
    assert len(keep) >= 12
    return keep


# ---- helpers --------------------------------------------------------------------------------------------------------------
to_np = dicom._to_numpy


def assert_reference(fragment: bytes, frame: np.ndarray):
    """the restated decoder against the ENCODER'S INPUT (before anything is asked of the device)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = rle_decode_frame(fragment, frame.shape[0], frame.shape[1], 8 * frame.dtype.itemsize)
    assert got == frame.astype(frame.dtype.newbyteorder("<")).tobytes()


def segment_table(buf: bytes, fragments: list, segments: int):
    """[(offset, length)] of fragments inside ``buf`` -> int64 [N, segments] offsets and lengths of their segments"""
    so, sl = [], []
    for off, ln in fragments:
        head = struct.unpack_from("<16L", buf, off)
        assert head[0] == segments
        offs = list(head[1:segments + 1]) + [ln]
        so.append([off + a for a in offs[:-1]])
        sl.append([b - a for a, b in zip(offs, offs[1:])])
    return np.array(so, dtype=np.int64), np.array(sl, dtype=np.int64)


def decode_streams(dev, streams: list, cols: int, fill: int = 0xA5):
    """raw one-segment streams as an 8-bit stack of 1 x ``cols`` frames through the kernel entry, into a pre-filled buffer
    -> (bytes [N, cols], status list)"""
    buf, so, sl = b"\x11\x22\x33", [], []
    for s in streams:
        so.append([len(buf)])
        sl.append([len(s)])
        buf += bytes(s) + b"\x77"                                                  # (streams start at every alignment in turn)
    native = torch.full((len(streams), cols), fill, dtype=torch.uint8).to(dev)
    x = dicom.decode_rle_frames(np.frombuffer(buf, dtype=np.uint8), np.array(so), np.array(sl), 1, cols, 8, device=dev, native=native)
    assert x.dtype == torch.uint8 and x.shape == (len(streams), 1, cols)
    return to_np(x).reshape(len(streams), cols), x._pl_status.cpu().tolist()


def assert_stream(dev, stream: bytes):
    """one raw stream == the reference walk, with the frame exactly as long as what it decodes to (status 0), one byte longer
    (short: bit 1, the byte beyond untouched) and one byte shorter (extra: bit 2)"""
    want = bytes(rle_decode_segment(stream))
    n = len(want)
    got, status = decode_streams(dev, [stream], max(n, 1) + 1)
    assert bytes(got[0, :n]) == want and status == [2] and (got[0, n:] == 0xA5).all()
    if n >= 1:
        got, status = decode_streams(dev, [stream], n)
        assert bytes(got[0]) == want and status == [0]
    if n >= 2:
        got, status = decode_streams(dev, [stream], n - 1)
        assert bytes(got[0]) == want[:n - 1] and status == [4]


def filler(rng, nbytes: int) -> bytes:
    """exactly ``nbytes`` stream bytes of whole literal and replicate runs"""
    out = bytearray()
    while len(out) < nbytes:
        left = nbytes - len(out)
        if left == 1:
            out += b"\x80"
        elif left == 3 or rng.random() < 0.4:
            out += bytes([int(rng.integers(129, 256)), int(rng.integers(0, 256))])
        else:
            n = int(rng.integers(1, min(128, left - 1) + 1))
            out += bytes([n - 1]) + rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    assert len(out) == nbytes
    return bytes(out)


def noise(rng, shape, dtype=np.uint8) -> np.ndarray:
    """no two horizontally adjacent bytes equal in any byte plane: every run is a literal run"""
    ib = np.dtype(dtype).itemsize
    step = rng.integers(1, 256, shape + (ib,), dtype=np.int64)
    planes = (np.cumsum(step.reshape(-1, ib), axis=0) % 256).astype(np.uint8)
    return planes.reshape(shape + (ib,)).copy().view(dtype).reshape(shape)


def load(dev, files, **kw):
    x, metas = dicom.load_frames(files, device=dev, **kw)
    return to_np(x), metas


# ---- 1: every entry offset ------------------------------------------------------------------------------------------------
def check_every_entry_offset(dev):
    rng = np.random.default_rng(1)
    frame = noise(rng, (1032, 128))                                               # rows of 128 literals: runs of 129 stream bytes
    frag = encode_frame(frame)
    assert_reference(frag, frame)
    seg = frag[64:]
    entries = walk_entries(seg)
    assert len(seg) == 1032 * 129 and len(entries) >= 129 and set(entries) == set(range(129))
    got, status = decode_streams(dev, [seg], frame.size)
    assert status == [0] and bytes(got[0]) == frame.tobytes()
    # ... and through the loader
    x, _ = load(dev, [rle_file(frame[None])], raw_pixels=True)
    assert x.dtype == np.uint8 and np.array_equal(x[0], frame)


# ---- 2: chunk seams -------------------------------------------------------------------------------------------------------
def seam_streams():
    rng = np.random.default_rng(2)
    tail = filler(rng, K + 37)
    lit = rng.integers(0, 256, 40, dtype=np.uint8).tobytes()
    out = {
        "a replicate control, its value byte first in the next chunk": filler(rng, K - 1) + bytes([200, 9]) + tail,
        "a literal control": filler(rng, K - 1) + bytes([39]) + lit + tail,
        "a literal's last data byte": filler(rng, K - 41) + bytes([39]) + lit + tail,
        "a 0x80": filler(rng, K - 1) + b"\x80" + tail,
        "a literal of 128 bytes begun at the last byte (entry offset 128)": filler(rng, K - 1) + bytes([127]) + bytes(range(128)) + tail,
        "K + 5 no-ops in a row": filler(rng, 300) + b"\x80" * (K + 5) + tail,
        "a literal cut by the end of the segment": filler(rng, K + 3) + bytes([99]) + lit,
        "a replicate control as the last byte": filler(rng, 2 * K - 1) + bytes([130]),
    }
    for n in (K - 1, K, K + 1, 1, 2, 100):
        out[f"a segment of {n} bytes"] = filler(rng, n)
    out["one control byte and nothing else"] = bytes([5])
    out["a pad byte alone"] = b"\x00"
    return out


SEAMS = list(seam_streams())


def check_chunk_seam(dev, name):
    s = seam_streams()[name]
    if name.endswith("last byte (entry offset 128)"):
        assert walk_entries(s)[1] == 128
    assert_stream(dev, s)


# ---- 3: extreme ratios and shapes -----------------------------------------------------------------------------------------
def check_constant_plane(dev):
    frame = np.full((256, 512), 77, dtype=np.uint8)
    frag = encode_frame(frame)
    assert_reference(frag, frame)
    assert len(frag) - 64 == 2 * K and set(frag[64::2]) == {129}                   # replicate runs only: a chunk gives 64 * K bytes
    x, _ = load(dev, [rle_file(frame[None])], raw_pixels=True)
    assert np.array_equal(x[0], frame)


def check_noise_plane(dev):
    frame = noise(np.random.default_rng(3), (37, 301), np.uint16)
    frag = encode_frame(frame)
    assert_reference(frag, frame)
    assert all(c < 128 for c in (frag[64], frag[64 + 129]))
    x, _ = load(dev, [rle_file(frame[None])], raw_pixels=True)
    assert x.dtype == np.uint16 and np.array_equal(x[0], frame)


SHAPES = [(1, 1), (1, 300), (300, 1), (3, 5), (7, 11)]


def check_small_shape(dev, rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    for dtype in (np.uint8, np.uint16):
        smooth = (rng.integers(0, 3, (rows, cols)).cumsum(axis=1) * 97).astype(dtype)
        for frame in (smooth, noise(rng, (rows, cols), dtype)):
            frag = encode_frame(frame)
            assert_reference(frag, frame)
            x, _ = load(dev, [rle_file(frame[None])], raw_pixels=True)
            assert x.dtype == frame.dtype and np.array_equal(x[0], frame), (rows, cols, dtype)


def check_encoder_options(dev):
    """no-ops, runs that cross rows and the pad byte 0x80: the same frames"""
    for seed in range(4, 40):                                                      # the first frame with a segment of odd length
        frame = (np.random.default_rng(seed).integers(0, 2, (33, 47)).cumsum(axis=1) * 1237 + 3).astype(np.uint16)
        planes = frame.view(np.uint8).reshape(33, 47, 2)
        if any(len(encode_segment(planes[:, :, b], pad=None)) % 2 for b in (0, 1)):
            break
    else:
        raise AssertionError("no frame needs the pad byte")
    for opts in (dict(noop_every=1), dict(noop_every=3, cross_rows=True), dict(cross_rows=True), dict(pad=0x80)):
        frag = encode_frame(frame, **opts)
        assert_reference(frag, frame)
        x, _ = load(dev, [rle_file(frame[None], **opts)], raw_pixels=True)
        assert np.array_equal(x[0], frame), opts
    assert len(encode_frame(frame, cross_rows=True)) < len(encode_frame(frame))


# ---- 4: containers --------------------------------------------------------------------------------------------------------
CONTAINERS = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32]


def container_frames(dtype, n=4, shape=(29, 35)):
    rng = np.random.default_rng(np.dtype(dtype).itemsize * 10 + (np.dtype(dtype).kind == "i"))
    info = np.iinfo(dtype)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    out = []
    for k in range(n):
        base = info.min / 2 + (info.max / 2 - info.min / 2) * np.exp(-(((yy - 14) / 9.0) ** 2 + ((xx - 17 - k) / 11.0) ** 2))
        noisy = base + rng.normal(0, (2.0, 40.0, 3000.0, 0.5)[k % 4], shape)       # unequal segment lengths from frame to frame
        out.append(np.clip(np.round(noisy), info.min, info.max).astype(dtype))
    return np.stack(out)


def check_container_kernel_entry(dev, dtype):
    """fragments at every alignment mod 4 inside one buffer, through decode_rle_frames"""
    frames = container_frames(dtype)
    ib = frames.dtype.itemsize
    if frames.dtype.kind == "i":
        assert (frames < 0).any() and (frames > 0).any()
    rng = np.random.default_rng(5)
    buf, where = b"", []
    for k, f in enumerate(frames):
        frag = encode_frame(f)
        assert_reference(frag, f)
        buf += rng.integers(0, 256, (k - len(buf)) % 4 + 4, dtype=np.uint8).tobytes()
        where.append((len(buf), len(frag)))
        buf += frag
    assert {w[0] % 4 for w in where} == {0, 1, 2, 3}
    so, sl = segment_table(buf, where, ib)
    assert len({int(v) for v in sl.ravel()}) > ib                                  # segments of unequal lengths
    raw = np.frombuffer(buf, dtype=np.uint8)
    kw = dict(rows=frames.shape[1], cols=frames.shape[2], bits_allocated=8 * ib, pixel_representation=int(frames.dtype.kind == "i"),
              device=dev)
    x = dicom.decode_rle_frames(raw, so, sl, **kw)
    assert x._pl_status.cpu().tolist() == [0] * 4
    got = to_np(x)
    assert got.dtype == frames.dtype and np.array_equal(got, frames)
    # device tensors are used in place; float64 with the fused rescale goes through pl_dicom_decode
    x = dicom.decode_rle_frames(torch.from_numpy(raw.copy()).to(dev), torch.from_numpy(so).to(dev), torch.from_numpy(sl).to(dev),
                                out="float64", rescale=(1.25, -1000.5), max_segment_bytes=int(sl.max()), **kw)
    want = frames.astype(np.float64) * 1.25
    want += -1000.5
    assert np.array_equal(x.cpu().numpy(), want)
    assert np.array_equal(dicom.decode_rle_frames(raw, so, sl, out="float32", **kw).cpu().numpy(), frames.astype(np.float32))


def check_container_loader(dev, dtype):
    frames = container_frames(dtype)
    files = [rle_file(f[None]) for f in frames]
    x, metas = load(dev, files, raw_pixels=True)
    assert x.dtype == frames.dtype and np.array_equal(x, frames)
    assert all(m.TransferSyntaxUID == RLE_UID and len(m.PixelDataFragments) == 1 and m.PixelData[1] == -1 for m in metas)
    # (the native container form of a BATCH needs frame bytes % 4 == 0, which 29 x 35 is not: one file at a time)
    y = np.concatenate([load(dev, [native_file(f[None])], raw_pixels=True)[0] for f in frames])
    assert y.dtype == x.dtype and np.array_equal(x, y)


# ---- 5: the loader --------------------------------------------------------------------------------------------------------
def loader_keywords(name):
    kws = [dict(), dict(raw_pixels=True), dict(invert_pixels=True), dict(invert_pixels=False)]
    kws += [dict(raw_pixels=True, dtype=dt) for dt in (np.float32, np.float64, np.int32, np.uint8)]
    kws += [dict(dtype=np.float64), dict(dtype=np.float32)]
    if "stored12" in name:
        kws += [dict(raw_pixels=True, correct_unused_bits=True), dict(raw_pixels=True, correct_unused_bits=True, dtype=np.float64)]
    return kws


def same_answer(dev, native_files, rle_files, **kw):
    """load_frames on the RLE files == load_frames on the same frames stored native: values, dtype, or the same refusal"""
    try:
        want, _ = load(dev, native_files, **kw)
    except NotImplementedError as e:
        with pytest.raises(NotImplementedError, match=str(e)[:30]):
            load(dev, rle_files, **kw)
        return None
    got, _ = load(dev, rle_files, **kw)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), kw
    return got


def check_loader_fixture(golden, dev, name):
    blob = explicit_fixtures(golden)[name]
    rle, frames = fixture_as_rle(blob)
    for f, frag in zip(frames, dicom.read_part10(rle)[0].PixelDataFragments):
        assert_reference(rle[frag[0]:frag[0] + frag[1]], f)
    raw, _ = load(dev, [rle], raw_pixels=True)
    assert raw.dtype == frames.dtype and np.array_equal(raw, frames)               # pixel_array itself
    for kw in loader_keywords(name):
        same_answer(dev, [blob.tobytes()], [rle], **kw)


def check_loader_rescale_per_file(golden, dev):
    """a series (one slope and intercept: the fused float64 form) and files that differ (decoded once, rescaled file by file)"""
    blob = explicit_fixtures(golden)["i16_ct"].tobytes()
    at = blob.index(struct.pack("<HH2s", 0x0028, 0x1053, b"DS")) + 8
    assert blob[at:at + 3] == b"1.5"
    other = blob[:at] + b"2.5" + blob[at + 3:]
    natives = [blob, other, blob]
    rles = [fixture_as_rle(np.frombuffer(b, dtype=np.uint8))[0] for b in natives]
    for kw in (dict(), dict(dtype=np.float32), dict(raw_pixels=True), dict(invert_pixels=True)):
        got = same_answer(dev, natives, rles, **kw)
        same_answer(dev, [blob, blob], [rles[0], rles[2]], **kw)
    assert got.dtype == np.float64 and not np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


def check_loader_multiframe_and_stacks(golden, dev, tmp_path):
    fx = explicit_fixtures(golden)
    blob = fx["u8_multiframe"]
    for table in ("filled", "empty"):
        rle, frames = fixture_as_rle(blob, table=table)
        assert frames.shape[0] == 3
        meta, _ = dicom.read_part10(rle)
        assert len(meta.PixelDataFragments) == 3 and int(meta.NumberOfFrames) == 3
        for kw in (dict(raw_pixels=True), dict(), dict(invert_pixels=True), dict(dtype=np.float64)):
            same_answer(dev, [blob.tobytes()], [rle], **kw)
        same_answer(dev, [blob.tobytes()] * 2, [rle, rle], invert_pixels=True)
    # a stack == each file alone == a permuted stack (files of one format: the 48 x 64 uint16 fixtures)
    names = ["u16_explicit", "u16_explicit_shifted", "u16_sequence", "u16_epid_tags"]
    rles = [fixture_as_rle(fx[n], noop_every=(0, 2, 0, 5)[k])[0] for k, n in enumerate(names)]
    whole, metas = load(dev, rles)
    assert np.array_equal(whole, load(dev, [fx[n].tobytes() for n in names])[0])
    for k, f in enumerate(rles):
        assert np.array_equal(load(dev, [f])[0][0], whole[k]), k
    perm = [2, 0, 3, 1]
    assert np.array_equal(load(dev, [rles[k] for k in perm])[0], whole[perm])
    # paths, bytes and file objects
    path = tmp_path / "a.dcm"
    path.write_bytes(rles[0])
    import io

    assert np.array_equal(load(dev, [str(path), path, io.BytesIO(rles[0]), bytearray(rles[0])])[0], whole[[0, 0, 0, 0]])


def check_dicom_image(golden, dev):
    fx = explicit_fixtures(golden)
    for name in ("u16_epid_tags", "i16_ct", "u16_inverted_sign", "u8_multiframe"):
        rle, _ = fixture_as_rle(fx[name])
        a, b = dicom.DicomImage(rle), dicom.DicomImage(fx[name].tobytes())
        assert a.array.dtype == b.array.dtype and a.array.shape == b.array.shape and np.array_equal(a.array, b.array), name
        assert np.array_equal(a.array, o.dicom_image_array(fx[name])), name
        assert a._original_dtype == b._original_dtype and a.metadata.TransferSyntaxUID == RLE_UID
    img = dicom.DicomImage(fixture_as_rle(fx["u16_epid_tags"])[0])
    assert img.sid == 1500.0 and img.sad == 1000.0 and abs(img.dpmm - (1 / 0.336) * 1.5) < 1e-12
    a = dicom.DicomImage(fixture_as_rle(fx["u16_explicit"])[0], dtype=np.float32, raw_pixels=True).array
    assert a.dtype == np.float32 and np.array_equal(a, o.dicom_image_array(fx["u16_explicit"], dtype=np.float32, raw_pixels=True))


# ---- 6: status and refusals -----------------------------------------------------------------------------------------------
def status_files():
    frames = container_frames(np.uint16)
    files = [rle_file(f[None]) for f in frames]
    # file 1: the low-byte segment loses its last run (the fragment's item says so)
    lo = encode_segment(np.ascontiguousarray(frames[1]).view(np.uint8).reshape(29, 35, 2)[:, :, 0])
    hi = encode_segment(np.ascontiguousarray(frames[1]).view(np.uint8).reshape(29, 35, 2)[:, :, 1])
    cut = fragment_of([hi, lo[:-40]])
    files[1] = _meta(RLE_UID) + image_tags(frames[1:2]) + encapsulate([cut])
    # file 2: two trailing zero bytes after the last segment (a literal of one byte: one byte too many)
    files[2] = _meta(RLE_UID) + image_tags(frames[2:3]) + encapsulate([encode_frame(frames[2]) + b"\x00\x00"])
    return frames, files, cut


def check_status(dev):
    frames, files, cut = status_files()
    with pytest.raises(ValueError, match="decoded RLE segment data"):
        rle_decode_frame(cut, 29, 35, 16)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        x, _ = dicom.load_frames(files, device=dev, check=False)
    assert not seen and x._pl_status.cpu().tolist() == [0, 2, 4, 0]
    got = to_np(x)
    for k in (0, 2, 3):
        assert np.array_equal(got[k], frames[k]), k
    with pytest.raises(ValueError, match=r"decoded RLE segment data doesn't match the expected amount \(file 1"):
        dicom.load_frames(files, device=dev)
    with pytest.raises(ValueError, match=r"expected amount \(file 1"):
        dicom.load_frames(files, device=dev, dtype=np.int32, raw_pixels=True)
    with pytest.warns(UserWarning, match=PADDING + r" \(file 1"):
        x, _ = dicom.load_frames([files[0], files[2], files[3]], device=dev)
    assert np.array_equal(to_np(x), frames[[0, 2, 3]])
    with pytest.raises(ValueError, match="expected amount"):
        dicom.DicomImage(files[1])


def check_window_outside_the_buffer(dev):
    frames = container_frames(np.int16, n=3)
    frags = [encode_frame(f) for f in frames]
    buf, where = b"", []
    for frag in frags:
        where.append((len(buf), len(frag)))
        buf += frag
    raw = np.frombuffer(buf, dtype=np.uint8)
    so, sl = segment_table(buf, where, 2)
    for (row, col), (arr, value) in {(1, 0): ("off", -1), (1, 1): ("off", len(buf) - 3), (0, 1): ("len", 1 << 40), (2, 0): ("len", -5),
                                     (2, 1): ("off", 1 << 50)}.items():
        o2, l2 = so.copy(), sl.copy()
        (o2 if arr == "off" else l2)[row, col] = value
        native = torch.full((3, 29 * 35 * 2), 0x5A, dtype=torch.uint8).to(dev)
        x = dicom.decode_rle_frames(raw, o2, l2, 29, 35, 16, pixel_representation=1, device=dev, native=native,
                                    max_segment_bytes=int(sl.max()))
        assert x._pl_status.cpu().tolist() == [int(k == row) for k in range(3)], (row, col)
        got = to_np(x)
        for k in range(3):
            assert np.array_equal(got[k], frames[k]) if k != row else (got[k].view(np.uint8) == 0x5A).all(), (row, col, k)
    # a segment longer than max_segment_bytes is outside what the tables hold: flagged, never read
    bound = int(np.sort(sl.max(axis=1))[1])
    want = [int(v > bound) for v in sl.max(axis=1)]
    assert sorted(want) == [0, 0, 1]
    x = dicom.decode_rle_frames(raw, so, sl, 29, 35, 16, pixel_representation=1, device=dev, max_segment_bytes=bound)
    assert x._pl_status.cpu().tolist() == want
    assert all(np.array_equal(to_np(x)[k], frames[k]) for k in range(3) if not want[k])


def check_malformed_and_refused(golden, dev):
    frames = container_frames(np.uint16)
    good = encode_frame(frames[0])

    def one(fragments, stack=frames[:1], uid=RLE_UID):
        return _meta(uid) + image_tags(stack) + encapsulate(fragments)

    head = list(struct.unpack_from("<16L", good))
    bad_count = struct.pack("<16L", 3, *head[1:]) + good[64:]
    not_increasing = struct.pack("<16L", 2, head[2], head[1], *head[3:]) + good[64:]
    same_twice = struct.pack("<16L", 2, head[1], head[1], *head[3:]) + good[64:]
    beyond = struct.pack("<16L", 2, head[1], len(good) + 2, *head[3:]) + good[64:]
    for frag, text in ((bad_count, "3 segments"), (not_increasing, "strictly increasing"), (same_twice, "strictly increasing"),
                       (beyond, "outside the fragment"), (good[:40], "64-byte header")):
        with pytest.raises(ValueError, match=text):
            dicom.load_frames([one([frag])], device=dev)
    with pytest.raises(ValueError, match="2 RLE fragments for NumberOfFrames = 1"):
        dicom.load_frames([one([good, good])], device=dev)
    with pytest.raises(ValueError, match="1 RLE fragments for NumberOfFrames = 2"):
        dicom.load_frames([one([good], frames[:2])], device=dev)
    # a filled Basic Offset Table that disagrees with the items
    ok = rle_file(frames[:2], table="filled")
    at = ok.index(struct.pack("<HHI", 0xFFFE, 0xE000, 8)) + 12
    assert struct.unpack_from("<I", ok, at)[0] == 8 + len(good)
    with pytest.raises(ValueError, match="Basic Offset Table disagrees"):
        dicom.load_frames([ok[:at] + struct.pack("<I", 6 + len(good)) + ok[at + 4:]], device=dev)
    assert np.array_equal(load(dev, [ok], raw_pixels=True)[0], frames[:2])
    with pytest.raises(ValueError, match="delimiter is missing"):
        dicom.load_frames([ok[:-8]], device=dev)
    # the other encapsulated syntaxes and deflate are refused as before, with the same messages
    for uid in ("1.2.840.10008.1.2.4.50", "1.2.840.10008.1.2.4.70", "1.2.840.10008.1.2.4.80", "1.2.840.10008.1.2.4.90"):
        with pytest.raises(NotImplementedError, match="encapsulated \\(compressed\\) Pixel Data: decoded by pydicom's codec plug-ins"):
            dicom.load_frames([one([good], uid=uid)], device=dev)
    with pytest.raises(NotImplementedError, match="Deflated Explicit VR Little Endian is inflated by pydicom's reader"):
        dicom.load_frames([one([good], uid="1.2.840.10008.1.2.1.99")], device=dev)
    # native and RLE files do not mix
    with pytest.raises(ValueError, match="native and RLE Lossless files are mixed"):
        dicom.load_frames([rle_file(frames[:1]), native_file(frames[1:2])], device=dev)
    with pytest.raises(ValueError, match="differ in pixel format or frame size"):
        dicom.load_frames([rle_file(frames[:1]), rle_file(frames[:1, :, :-1])], device=dev)


def check_c_abi_argument_checks(dev):
    """pl_dicom_rle_decode: unsupported (2) for a segment count other than 1 / 2 / 4, invalid argument (1) for n_frames outside
    1 .. 65535, rows or cols < 1 and null pointers -- all before any launch (the pointers below are never dereferenced)"""
    import re
    from pathlib import Path

    from pylinac_amd import _lib

    lib = _lib.load()
    buf = torch.zeros(256, dtype=torch.uint8, device=dev)
    idx = torch.zeros(8, dtype=torch.int64, device=dev)
    st = torch.zeros(4, dtype=torch.int32, device=dev)
    p, q, s = buf.data_ptr(), idx.data_ptr(), st.data_ptr()

    def call(n, segments, rows, cols, bytes_=p, native=p, work=p, max_seg=64):
        return lib.pl_dicom_rle_decode(bytes_, 256, q, q, n, segments, max_seg, rows, cols, native, s, work, None)

    for segments in (0, 3, 5, 8, -1):
        assert call(1, segments, 4, 4) == 2 and b"unsupported segment count" in lib.pl_last_error()
        assert lib.pl_dicom_rle_work_bytes(1, segments, 64) == -1
    assert call(0, 2, 4, 4) == 1 and call(65536, 2, 4, 4) == 1 and call(1, 2, 0, 4) == 1 and call(1, 2, 4, 0) == 1
    assert call(1, 2, 4, 4, bytes_=None) == 1 and call(1, 2, 4, 4, native=None) == 1 and call(1, 2, 4, 4, work=None) == 1
    assert call(1, 2, 4, 4, max_seg=-1) == 1
    assert lib.pl_dicom_rle_work_bytes(0, 2, 64) == -1 and lib.pl_dicom_rle_work_bytes(65536, 2, 64) == -1
    one, many = lib.pl_dicom_rle_work_bytes(1, 1, K), lib.pl_dicom_rle_work_bytes(3, 4, 5 * K + 1)
    assert 0 < one and one % 16 == 0 and many >= 3 * 4 * 6 * (129 * 4 + 8 + 1)
    # the chunk size is one constant in the header and in Python
    header = (Path(__file__).resolve().parent.parent / "include" / "pylinac_hip.h").read_text()
    assert int(re.search(r"#define PL_DICOM_RLE_CHUNK (\d+)", header).group(1)) == K >= 129
