"""Shared checks of JPEG 2000 lossless Pixel Data (1.2.840.10008.1.2.4.90 / .91) in pylinac_amd.dicom: read_part10's item walk,
load_frames / DicomImage with ``jpeg2000=True``, the host's header and packet-header parse (``_j2k_codestream``),
decode_jpeg2000_frames and pl_dicom_j2k_decode (tests/test_emulated_dicom_j2k.py on the CPU emulator,
tests/test_gpu_dicom_j2k.py on the MI355X).  Every comparison is EQUALITY.

The streams come from Pillow's OpenJPEG (``irreversible=False, no_jp2=True``: the raw codestream DICOM encapsulates), an
encoder and decoder independent of this project: the first expectation is the SOURCE array, the second is what
``PIL.Image.open`` decodes from the same stream, both bit for bit.  Refusals are made with Pillow's keywords where it has one
(layers, precincts, the 9/7 transform, the JP2 wrapper, tiles, RGB) and by patching bytes or inserting a segment otherwise.

Shapes are the smallest at which each part can go wrong: heights that are no multiple of the stripe's four rows, blocks cut by
a subband's edge, odd band lengths at every level, single rows and columns (Pillow writes them without levels, so a band of
size 0 is in none of its streams), several blocks per band with a tag tree of more than one level (129 x 67 with 4 x 4 and
32 x 32 blocks), oblong blocks, all five progression orders, Psot = 0 and every skipped segment; no stack has more than 8
frames of 129 x 67."""
from __future__ import annotations

import io
import struct
import zipfile

import numpy as np
import pytest
import torch
from PIL import Image

import dicom_rle_checks as rl
from pylinac_amd import dicom

UIDS = dicom.JPEG_2000
TODAY = "encapsulated \\(compressed\\) Pixel Data: decoded by pydicom's codec plug-ins, not by this path"
SHAPES = [(1, 1), (1, 9), (9, 1), (5, 7), (33, 65), (64, 64), (129, 67)]
LEVELS = [0, 2, 5]
BLOCKS = [(4, 4), (32, 32), (64, 64)]
CONTENTS = ["constant", "constant, off the middle", "spike", "ramp", "checkerboard"]
PRECISIONS = [9, 12, 16]


def to_np(x: torch.Tensor) -> np.ndarray:
    return x.cpu().numpy()


# ---- streams and files ----------------------------------------------------------------------------------------------------
def stream(frame: np.ndarray, **kw) -> bytes:
    """one frame [rows, cols] uint8 / uint16 -> its lossless JPEG 2000 codestream (Pillow: mode L / I;16)"""
    out = io.BytesIO()
    kw.setdefault("irreversible", False)
    kw.setdefault("no_jp2", True)
    Image.fromarray(frame).save(out, "JPEG2000", **kw)
    return out.getvalue()


def pil_decode(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)))


def segments(data: bytes) -> dict:
    """marker -> offset of the marker inside the main header of a codestream (up to SOT)"""
    assert data[:2] == b"\xff\x4f"
    pos, found = 2, {}
    while True:
        marker, ln = struct.unpack_from(">HH", data, pos)
        found.setdefault(marker, pos)
        if marker == 0xFF90:
            return found
        pos += 2 + ln


def cod_levels(data: bytes) -> int:
    return data[segments(data)[0xFF52] + 4 + 5]


def patched(data: bytes, at: int, value: int) -> bytes:
    return data[:at] + bytes([value]) + data[at + 1:]


def with_ssiz(data: bytes, precision: int, signed: bool) -> bytes:
    """the Ssiz byte (offset 40 from the SIZ marker) of a Pillow stream set to ``precision`` bits, signed or not"""
    at = segments(data)[0xFF51] + 40
    assert at == 42 and data[at] in (7, 15)
    return patched(data, at, (precision - 1) | (0x80 if signed else 0))


def inserted(data: bytes, marker: int, payload: bytes, before: int = 0xFF5C) -> bytes:
    """a marker segment put in front of the main header's ``before`` segment (QCD)"""
    at = segments(data)[before]
    return data[:at] + struct.pack(">HH", marker, len(payload) + 2) + payload + data[at:]


def with_psot(data: bytes, psot: int) -> bytes:
    at = segments(data)[0xFF90]
    return data[:at + 6] + struct.pack(">I", psot) + data[at + 10:]


def signed_stream(frame: np.ndarray, **kw) -> bytes:
    """an int16 / int8 frame as a SIGNED stream of full precision: the encoder sees the values shifted up by half the range,
    bit 7 of Ssiz takes the shift back"""
    bits = 8 * frame.dtype.itemsize
    unsigned = (frame.astype(np.int32) + (1 << (bits - 1))).astype(np.uint16 if bits == 16 else np.uint8)
    return with_ssiz(stream(unsigned, **kw), bits, True)


def frame_stream(frame: np.ndarray, **kw) -> bytes:
    return signed_stream(frame, **kw) if frame.dtype.kind == "i" else stream(frame, **kw)


def pieces(data: bytes, n: int) -> list:
    """a stream as n fragments of even length"""
    cut = [((len(data) * k // n) + 1) & ~1 for k in range(n)] + [len(data)]
    return [data[a:b] for a, b in zip(cut, cut[1:])]


def j2k_file(frames: np.ndarray, uid: str = UIDS[0], table: str = "empty", extra: bytes = b"", streams: list | None = None,
             split: int = 1, **kw) -> bytes:
    """a Part-10 file of [F, rows, cols] frames with JPEG 2000 Pixel Data (``streams``: the codestreams, else Pillow's for the
    frames; ``split``: fragments per frame, which needs a filled table or a single frame)"""
    streams = [frame_stream(f, **kw) for f in frames] if streams is None else streams
    if split == 1:
        return rl._meta(uid) + rl.image_tags(frames, extra) + rl.encapsulate(streams, table)
    frags = [p for s in streams for p in pieces(s, split)]
    body = rl.encapsulate(frags, "empty")
    if table == "filled":                                    # (one entry per FRAME: the offset of its first fragment's item)
        offs, pos = [], 0
        for k, frag in enumerate(frags):
            if k % split == 0:
                offs.append(pos)
            pos += 8 + len(frag) + len(frag) % 2
        bot = struct.pack(f"<{len(offs)}I", *offs)
        head = struct.pack("<HH2sHI", 0x7FE0, 0x0010, b"OB", 0, 0xFFFFFFFF)
        assert body.startswith(head + struct.pack("<HHI", 0xFFFE, 0xE000, 0))
        body = head + struct.pack("<HHI", 0xFFFE, 0xE000, len(bot)) + bot + body[len(head) + 8:]
    return rl._meta(uid) + rl.image_tags(frames, extra) + body


def ds(element: int, text: str) -> bytes:
    return rl._el(0x0028, element, "DS", text.encode())


def bits_stored(n: int) -> bytes:
    return rl._el(0x0028, 0x0101, "US", struct.pack("<H", n))


def load(dev, files, **kw):
    x, metas = dicom.load_frames(files, device=dev, jpeg2000=True, **kw)
    return to_np(x), metas


def noise(rng, shape, dtype) -> np.ndarray:
    """uniform over the full range: every bit plane and every pass is coded"""
    info = np.iinfo(dtype)
    return rng.integers(info.min, int(info.max) + 1, shape, dtype=np.int64).astype(dtype)


def assert_decodes(dev, frames: np.ndarray, streams: list, **file_kw):
    """the device's frames == the source == Pillow's decode of the same streams"""
    for f, s in zip(frames, streams):
        assert np.array_equal(pil_decode(s), f)                                   # the oracle agrees with the encoder's input
    got, _ = load(dev, [j2k_file(frames, streams=streams, **file_kw)])
    assert got.dtype == frames.dtype and np.array_equal(got, frames)


# ---- 1: geometry ------------------------------------------------------------------------------------------------------------
def allowed_levels(shape) -> list:
    """what Pillow encodes: 1 x 1 only with num_resolutions = 1, 1 x 9 and 9 x 1 only without the keyword, 5 x 7 up to 3"""
    if shape == (1, 1):
        return [0]
    if shape in ((1, 9), (9, 1)):
        return [None]
    return [0, 2] if shape == (5, 7) else LEVELS


def check_geometry(dev, shape, dtype, block, only=None):
    """``only``: the levels to run out of ``allowed_levels(shape)`` (None: all of them)"""
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + block[0])
    seen, wanted = set(), [v for v in allowed_levels(shape) if only is None or v in only]
    assert wanted
    for levels in wanted:
        frames = noise(rng, (1,) + shape, dtype)
        kw = {} if levels is None else {"num_resolutions": levels + 1}
        data = stream(frames[0], codeblock_size=block, **kw)
        assert levels is None or cod_levels(data) == levels
        seen.add(cod_levels(data))
        assert_decodes(dev, frames, [data])
    assert seen == {0} if 1 in shape else len(seen) == len(wanted)                 # (Pillow: no levels for a length of 1)


PROGRESSIONS = ["LRCP", "RLCP", "RPCL", "PCRL", "CPRL"]
OBLONG_BLOCKS = [(64, 16), (8, 64), (16, 4)]                 # area <= 4096, the two sides differ: the block's own row pitch


def check_progression_orders(dev):
    """one layer, one component and one precinct per resolution: all five orders put the packets in resolution order"""
    frames = noise(np.random.default_rng(11), (1, 33, 65), np.uint8)
    orders = set()
    for k, name in enumerate(PROGRESSIONS):
        data = stream(frames[0], progression=name, num_resolutions=4)
        assert data[segments(data)[0xFF52] + 4 + 1] == k                          # SGcod: the progression order
        orders.add(data[segments(data)[0xFF52] + 4 + 1])
        assert_decodes(dev, frames, [data])
    assert orders == {0, 1, 2, 3, 4}


def check_oblong_blocks(dev):
    rng = np.random.default_rng(12)
    for k, block in enumerate(OBLONG_BLOCKS):
        for dtype, shape in ((np.uint16, (33, 65)), (np.uint8, (129, 67)))[:2 if k == 0 else 1]:
            frames = noise(rng, (1,) + shape, dtype)
            data = stream(frames[0], codeblock_size=block, num_resolutions=3)
            cod = segments(data)[0xFF52] + 4
            assert {1 << (data[cod + 6] + 2), 1 << (data[cod + 7] + 2)} == set(block)    # the stream states an oblong block
            assert_decodes(dev, frames, [data])


def check_psot_zero_and_skipped_segments(dev):
    """Psot = 0 (the tile-part runs to EOC) on good streams, with and without the item's pad byte behind EOC; PLT in the
    tile-part header (Pillow's ``plt=True``); PLM, CRG, TLM and COM in the main header: all skipped"""
    frames = noise(np.random.default_rng(13), (1, 33, 65), np.uint16)
    good = stream(frames[0])
    assert struct.unpack_from(">I", good, segments(good)[0xFF90] + 6)[0] != 0 and good[-2:] == b"\xff\xd9"
    open_ended = with_psot(good, 0)
    other = inserted(open_ended, 0xFF64, b"\x00\x01x")                            # seven bytes more: the other parity
    assert {len(open_ended) % 2, len(other) % 2} == {0, 1}                        # one of the two items carries a pad byte
    for data in (open_ended, other):
        assert struct.unpack_from(">I", data, segments(data)[0xFF90] + 6)[0] == 0
        assert_decodes(dev, frames, [data])
    with_plt = stream(frames[0], plt=True)
    sot = segments(with_plt)[0xFF90]
    assert with_plt[sot + 12:sot + 14] == b"\xff\x58" and good[sot + 12:sot + 14] == b"\xff\x93"   # PLT opens the tile-part header
    assert_decodes(dev, frames, [with_plt])
    assert_decodes(dev, frames, [with_psot(with_plt, 0)])
    assert 0xFF64 in segments(good)                                               # (COM: Pillow writes one into every stream)
    for marker, payload in ((0xFF57, bytes([0, 2, 0x10, 0x11])), (0xFF63, bytes(4)), (0xFF55, bytes(8))):       # PLM, CRG, TLM
        data = inserted(good, marker, payload)
        assert marker in segments(data) and marker not in segments(good)
        assert_decodes(dev, frames, [data])


# ---- 2: content -------------------------------------------------------------------------------------------------------------
def content(kind: str, shape, dtype=np.uint16) -> np.ndarray:
    top = np.iinfo(dtype).max
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    if kind == "constant":                                                       # the middle of the range: every coefficient is 0
        return np.full(shape, top // 2 + 1, dtype)
    if kind == "constant, off the middle":
        return np.full(shape, 1000 % (top + 1), dtype)
    if kind == "spike":
        a = np.zeros(shape, dtype)
        a[shape[0] // 2 + 1, shape[1] // 3] = top
        return a
    if kind == "ramp":
        rng = np.random.default_rng(5)
        return ((yy * 37 + xx * 91) * (top // 8192 or 1) // 4 + rng.integers(0, 4, shape)).astype(dtype)
    return (((yy + xx) & 1) * top).astype(dtype)


def check_content(dev, kind):
    for shape in ((40, 40), (33, 65)):
        for dtype in (np.uint16, np.uint8):
            frame = content(kind, shape, dtype)
            data = stream(frame)
            if kind == "constant":                                                # every packet empty or every block excluded
                assert dicom._j2k_codestream(np.frombuffer(data, np.uint8), *shape, 16, "constant")[3] == []
            assert_decodes(dev, frame[None], [data])


# ---- 3: precision and sign --------------------------------------------------------------------------------------------------
def check_precision_sign(dev, precision: int, signed: bool):
    rng = np.random.default_rng(precision * 2 + signed)
    half = 1 << (precision - 1)
    inside = (32768 + rng.integers(-half, half, (2, 33, 65))).astype(np.uint16)      # decodes to values inside the P-bit range
    full = noise(rng, (2, 33, 65), np.uint16)                                        # the clamp
    for u in (inside, full):
        streams = [with_ssiz(stream(f), precision, signed) for f in u]
        wide = u.astype(np.int64)
        want = np.clip(wide - 32768, -half, half - 1) if signed else np.clip(wide - 32768 + half, 0, 2 * half - 1)
        if u is inside:
            assert np.array_equal(want, wide - 32768 + (0 if signed else half))      # nothing is clamped in this stack
        else:
            assert precision == 16 or not np.array_equal(want, wide - 32768 + (0 if signed else half))
        for f, s in zip(want, streams):                                              # Pillow: unsigned, shifted up to 16 bits
            assert np.array_equal(pil_decode(s).astype(np.int64), (f + (half if signed else 0)) << (16 - precision))
        frames = want.astype(np.int16 if signed else np.uint16)
        got, metas = load(dev, [j2k_file(frames, streams=streams, extra=bits_stored(precision))])
        assert got.dtype == frames.dtype and np.array_equal(got, frames)
        assert metas[0].BitsStored == precision and metas[0].PixelRepresentation == int(signed)


def check_eight_bit_sign(dev):
    rng = np.random.default_rng(8)
    frames = noise(rng, (2, 33, 65), np.int8)
    streams = [signed_stream(f) for f in frames]
    assert streams[0][42] == 0x87
    got, _ = load(dev, [j2k_file(frames, streams=streams)])
    assert got.dtype == np.int8 and np.array_equal(got, frames)


# ---- 4: DICOM plumbing ------------------------------------------------------------------------------------------------------
SMALL = (18, 13)                                            # rows no multiple of four, an odd width, frame bytes a multiple of four


def stack(dtype=np.uint16, n=4, shape=SMALL) -> np.ndarray:
    return rl.container_frames(dtype, n=n, shape=shape)


def check_plumbing(dev, tmp_path):
    frames = stack()
    native, _ = dicom.load_frames([rl.native_file(frames)], device=dev)
    for uid in UIDS:
        for table in ("empty", "filled"):
            got, metas = load(dev, [j2k_file(frames, uid=uid, table=table)])
            assert np.array_equal(got, frames) and np.array_equal(got, to_np(native))
            assert metas[0].TransferSyntaxUID == uid and metas[0].PixelData[1] == -1 and len(metas[0].PixelDataFragments) == 4
            assert len(metas[0].PixelDataOffsetTable) == (0 if table == "empty" else 4)
    # a frame split over three fragments: alone with an empty table, in a multi-frame file with a filled one
    got, metas = load(dev, [j2k_file(frames[:1], split=3)])
    assert np.array_equal(got, frames[:1]) and len(metas[0].PixelDataFragments) == 3
    got, metas = load(dev, [j2k_file(frames, split=3, table="filled")])
    assert np.array_equal(got, frames) and len(metas[0].PixelDataFragments) == 12 and len(metas[0].PixelDataOffsetTable) == 4
    with pytest.raises(ValueError, match="12 JPEG 2000 fragments for NumberOfFrames = 4"):
        load(dev, [j2k_file(frames, split=3)])
    # several files in one call (their streams differ in levels and block size), paths and bytes, signed frames
    files = [j2k_file(frames[:1], num_resolutions=1), j2k_file(frames[1:3], codeblock_size=(16, 16)), j2k_file(frames[3:], num_resolutions=4)]
    path = tmp_path / "a.dcm"
    path.write_bytes(files[0])
    got, metas = load(dev, [path, files[1], io.BytesIO(files[2])])
    assert np.array_equal(got, frames) and len(metas) == 3
    signed = stack(np.int16)
    got, _ = load(dev, [j2k_file(signed[:2]), j2k_file(signed[2:])])
    assert got.dtype == np.int16 and np.array_equal(got, signed) and (signed < 0).any()
    # both keywords
    x, _ = dicom.load_frames([j2k_file(frames)], device=dev, jpeg2000=True, jpeg_lossless=True)
    assert np.array_equal(to_np(x), frames)
    meta, _ = dicom.read_part10(j2k_file(frames), jpeg2000=True)
    assert len(meta.PixelDataFragments) == 4


def check_rescale_and_dtypes(dev):
    signed = stack(np.int16)
    shared = ds(0x1052, "-1024") + ds(0x1053, "1.5")
    files = [j2k_file(signed[:2], extra=shared), j2k_file(signed[2:], extra=shared)]
    natives = [rl.native_file(signed[:2], extra=shared), rl.native_file(signed[2:], extra=shared)]
    x, _ = dicom.load_frames(files, device=dev, jpeg2000=True)
    want, _ = dicom.load_frames(natives, device=dev)
    assert x.dtype == torch.float64 and np.array_equal(to_np(x), signed.astype(np.float64) * 1.5 + -1024)      # the fused path
    assert np.array_equal(to_np(x), to_np(want))
    for kw in (dict(raw_pixels=True), dict(dtype=np.float64), dict(dtype=np.uint16, raw_pixels=True), dict(dtype=np.float64, raw_pixels=True),
               dict(dtype=np.float32), dict(invert_pixels=True)):
        got, _ = load(dev, files, **kw)
        ref, _ = dicom.load_frames(natives, device=dev, **kw)
        assert got.dtype == to_np(ref).dtype and np.array_equal(got, to_np(ref)), kw
    own = [j2k_file(signed[k:k + 1], extra=ds(0x1052, str(-1000 - k)) + ds(0x1053, str(1 + k))) for k in range(4)]
    got, _ = load(dev, own)
    assert np.array_equal(got, np.stack([signed[k].astype(np.float64) * (1 + k) + (-1000 - k) for k in range(4)]))
    dirty = stack(np.uint16)
    assert (dirty >> 12).any()
    got, _ = load(dev, [j2k_file(dirty, extra=bits_stored(12))], correct_unused_bits=True)
    assert np.array_equal(got, dirty & 0x0FFF)


def check_dicom_image(dev):
    frames = stack(np.uint16, n=1, shape=(33, 65))
    img = dicom.DicomImage(io.BytesIO(j2k_file(frames)), jpeg2000=True)
    ref = dicom.DicomImage(io.BytesIO(rl.native_file(frames)))
    assert img.array.dtype == ref.array.dtype and np.array_equal(img.array, ref.array) and img.array.shape == (33, 65)
    with pytest.raises(NotImplementedError, match=TODAY):
        dicom.DicomImage(io.BytesIO(j2k_file(frames)))


# ---- 5: refusals ------------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    frames = stack(np.uint16, n=1, shape=(33, 65))
    frame = frames[0]
    good = stream(frame)
    seg = segments(good)

    def refused(data, error, match, of=frames):
        with pytest.raises(error, match=match):
            load(dev, [j2k_file(of, streams=[data])])

    for uid in UIDS:                                                              # without the keyword: today's message
        with pytest.raises(NotImplementedError, match=TODAY):
            dicom.load_frames([j2k_file(frames, uid=uid)], device=dev)
        with pytest.raises(NotImplementedError, match=TODAY):
            dicom.read_part10(j2k_file(frames, uid=uid), jpeg_lossless=True)
    for uid in ("1.2.840.10008.1.2.4.50", "1.2.840.10008.1.2.4.80"):              # lossy JPEG and JPEG-LS stay refused
        with pytest.raises(NotImplementedError, match=TODAY):
            load(dev, [j2k_file(frames, uid=uid)])
    for other in (rl.native_file(frames), rl.rle_file(frames)):
        with pytest.raises(ValueError, match="JPEG 2000 files are mixed with native, RLE Lossless or JPEG Lossless files"):
            load(dev, [j2k_file(frames), other])
    refused(stream(frame, quality_layers=[4, 2, 1], quality_mode="rates"), NotImplementedError, "file 0: .*COD with 3 quality layers")
    refused(stream(frame, precinct_size=(32, 32)), NotImplementedError, "file 0: .*more than one precinct in a resolution")
    small = stack(np.uint16, n=1, shape=(16, 16))
    one_precinct = stream(small[0], precinct_size=(32, 32))
    assert one_precinct[segments(one_precinct)[0xFF52] + 4] & 1                     # Scod bit 0: the precincts are stated
    assert_decodes(dev, small, [one_precinct])
    refused(stream(frame, irreversible=True), NotImplementedError, "file 0: .*irreversible 9/7 transform")
    refused(stream(frame, no_jp2=False), NotImplementedError, "file 0: .*JP2 file \\(box wrapper\\)")
    refused(stream(np.dstack([frame.astype(np.uint8)] * 3)), NotImplementedError, "file 0: .*Csiz = 3")
    big = stack(np.uint16, n=1, shape=(64, 64))
    refused(stream(big[0], tile_size=(32, 32)), NotImplementedError, "file 0: .*more than one tile", of=big)
    cod = seg[0xFF52] + 4
    refused(patched(good, cod + 8, 1), NotImplementedError, "file 0: .*code-block style 0x01")
    refused(patched(good, cod, 2), NotImplementedError, "file 0: .*SOP or EPH")
    refused(patched(good, cod, 4), NotImplementedError, "file 0: .*SOP or EPH")
    refused(patched(good, cod + 5, 17), NotImplementedError, "file 0: .*17 decomposition levels: at most J2K_MAX_LEVELS = 16")
    refused(patched(patched(good, cod + 6, 5), cod + 7, 3), NotImplementedError, "file 0: .*code blocks of 128 x 32")
    refused(patched(good, seg[0xFF5C] + 4, good[seg[0xFF5C] + 4] | 2), NotImplementedError, "file 0: .*quantisation style 2")
    siz = seg[0xFF51] + 4
    refused(patched(good, siz + 37, 2), NotImplementedError, "file 0: .*subsampling XRsiz x YRsiz = 2 x 1")
    refused(patched(good, siz + 13, 1), NotImplementedError, "file 0: .*non-zero image or tile origin")
    refused(patched(good, 42, 16), ValueError, "file 0: .*SIZ precision 17")
    refused(inserted(good, 0xFF53, bytes(7)), NotImplementedError, "file 0: .*marker FF53, COC")
    refused(inserted(good, 0xFF5F, bytes(7)), NotImplementedError, "file 0: .*marker FF5F, POC")
    refused(inserted(good, 0xFF5D, bytes(4)), NotImplementedError, "file 0: .*marker FF5D, QCC")
    refused(inserted(good, 0xFF5E, bytes(3)), NotImplementedError, "file 0: .*marker FF5E, RGN")
    refused(inserted(good, 0xFF60, bytes(3)), NotImplementedError, "file 0: .*marker FF60, PPM")
    assert_decodes(dev, frames, [inserted(inserted(good, 0xFF64, b"\x00\x01a comment"), 0xFF55, bytes(8))])   # COM and TLM: skipped
    refused(good, ValueError, "file 0: .*SIZ states Ysiz x Xsiz = 33 x 65 where Rows x Columns = 33 x 64", of=frames[:, :, :-1])
    refused(good[:seg[0xFF5C] + 6], ValueError, "file 0: .*cut off|file 0: .*ends without SOT")
    refused(b"\xff\xd8" + good[2:], ValueError, "file 0: .*does not start with SOC")
    refused(with_psot(good, 13), ValueError, "file 0: .*SOT states a tile-part of 13 bytes")
    # a stream cut inside a packet header, and one whose last 40 % are gone with Psot corrected: host errors, nothing is launched
    noisy = noise(np.random.default_rng(3), (1, 33, 65), np.uint16)
    data = stream(noisy[0])
    sot = segments(data)[0xFF90]
    sod = data.index(b"\xff\x93", sot) + 2
    for keep in (sod, sod + 1):
        refused(with_psot(data[:keep], keep - sot), ValueError, "file 0: .*the packet header of resolution 0 runs out of bytes", of=noisy)
    keep = len(data) * 6 // 10
    refused(with_psot(data[:keep], keep - sot), ValueError, "file 0: .*(truncated code block|runs out of bytes)", of=noisy)
    refused(with_psot(data[:keep], 0), ValueError, "file 0: .*(truncated code block|runs out of bytes)", of=noisy)
    # a truncated (lossy) stream: fewer coding passes than 3 x planes - 2
    refused(stream(noisy[0], quality_layers=[8], quality_mode="rates"), ValueError,
            "file 0: .*not a lossless JPEG 2000 stream: truncated code block", of=noisy)
    # archives keep refusing the members
    archive = io.BytesIO()
    with zipfile.ZipFile(archive, "w", zipfile.ZIP_DEFLATED) as z:
        z.writestr("a.dcm", j2k_file(frames))
    for kw in (dict(), dict(encapsulated=True)):
        with pytest.raises(NotImplementedError, match=TODAY):
            dicom.load_zip(archive.getvalue(), device=dev, **kw)


# ---- 6: status --------------------------------------------------------------------------------------------------------------
def staged(files):
    read = [dicom.read_part10(f, jpeg2000=True) for f in files]
    metas, blobs = [m for m, _ in read], [b for _, b in read]
    lay = [dicom._layout(m) for m in metas]
    return dicom._j2k_stage(metas, blobs, lay, [f"file {k}" for k in range(len(files))]), lay[0]


def check_status(dev):
    frames = stack(np.uint16, n=3)
    (host, (blocks, params), owner), lay = staged([j2k_file(frames[:2]), j2k_file(frames[2:])])
    assert owner == [0, 0, 1] and blocks.shape[1] == 10 and params.shape == (3, 4) and set(blocks[:, 0]) == {0, 1, 2}
    x = dicom.decode_jpeg2000_frames(host, blocks, params, *SMALL, 16, device=dev)
    assert to_np(x._pl_status).tolist() == [0, 0, 0] and np.array_equal(to_np(x), frames)
    bad = blocks.copy()
    row = int(np.flatnonzero(bad[:, 0] == 1)[0])
    bad[row, 1] = len(host) + 1                                                   # one block of frame 1 begins beyond the buffer
    x = dicom.decode_jpeg2000_frames(host, bad, params, *SMALL, 16, device=dev)
    assert to_np(x._pl_status).tolist() == [0, 1, 0]
    assert np.array_equal(to_np(x)[[0, 2]], frames[[0, 2]])
    for column, value in ((2, len(host)), (6, SMALL[1]), (7, -1), (8, 65), (9, 0), (5, 4), (4, 31), (3, 2)):     # every other check
        bad = blocks.copy()
        bad[row, column] = value
        x = dicom.decode_jpeg2000_frames(host, bad, params, *SMALL, 16, device=dev)
        assert to_np(x._pl_status).tolist() == [0, 1, 0], column
        assert np.array_equal(to_np(x)[[0, 2]], frames[[0, 2]]), column
    wrong = params.copy()
    wrong[2, 1] = 17                                                              # a precision the container cannot hold
    x = dicom.decode_jpeg2000_frames(host, blocks, wrong, *SMALL, 16, device=dev)
    assert to_np(x._pl_status).tolist() == [0, 0, 1] and np.array_equal(to_np(x)[:2], frames[:2])
    # a buffer that does not begin on a dword, a native buffer of the caller's, device tensors
    shifted = np.concatenate([np.zeros(1, np.uint8), host])
    moved = blocks.copy()
    moved[:, 1] += 1
    dbuf = torch.from_numpy(shifted).to(dev)[1:]
    native = torch.full((3, SMALL[0] * SMALL[1] * 2), 0xA5, dtype=torch.uint8, device=dev)
    x = dicom.decode_jpeg2000_frames(dbuf, blocks, torch.from_numpy(params).to(dev), *SMALL, 16, device=dev, native=native)
    assert np.array_equal(to_np(x), frames) and x.data_ptr() == native.data_ptr()
    x = dicom.decode_jpeg2000_frames(shifted, moved, params, *SMALL, 16, device=dev)
    assert np.array_equal(to_np(x), frames)


def check_status_through_the_loader(dev, monkeypatch):
    """check=True reads the status once and names file and frame"""
    frames = stack(np.uint16, n=2)
    real = dicom._j2k_stage

    def broken(*a):
        host, (blocks, params), owner = real(*a)
        blocks[np.flatnonzero(blocks[:, 0] == 1)[0], 1] = len(host) + 5
        return host, (blocks, params), owner

    monkeypatch.setattr(dicom, "_j2k_stage", broken)
    with pytest.raises(ValueError, match="file 1, frame 1 of the stack: JPEG 2000 Pixel Data: a code-block descriptor"):
        load(dev, [j2k_file(frames[:1]), j2k_file(frames[1:])])
    got, _ = load(dev, [j2k_file(frames[:1]), j2k_file(frames[1:])], check=False)
    assert np.array_equal(got[0], frames[0])


def check_c_abi_argument_checks(dev):
    """pl_dicom_j2k_decode: invalid argument (1) / unsupported (2) before any launch (the pointers are never dereferenced)"""
    lib = dicom._lib.load()
    p = 1 << 20
    good = dict(bytes_=p, nbytes=64, blocks=p, n_blocks=1, params=p, n=1, levels=5, rows=8, cols=8, bps=2, native=p, status=p, work=p)

    def call(**kw):
        a = {**good, **kw}
        return lib.pl_dicom_j2k_decode(a["bytes_"], a["nbytes"], a["blocks"], a["n_blocks"], a["params"], a["n"], a["levels"], a["rows"],
                                       a["cols"], a["bps"], a["native"], a["status"], a["work"], None)

    for kw in (dict(bytes_=None), dict(blocks=None), dict(params=None), dict(native=None), dict(status=None), dict(work=None), dict(n=0),
               dict(n=65536), dict(n_blocks=-1), dict(rows=0), dict(cols=65536), dict(nbytes=-1), dict(levels=-1), dict(bytes_=p + 2),
               dict(work=p + 8)):
        assert call(**kw) == 1, kw
        assert b"pl_dicom_j2k_decode" in lib.pl_last_error()
    assert call(bps=4) == 2 and call(levels=17) == 2
    size = lib.pl_dicom_j2k_work_bytes
    assert size(3, 33, 65) == 3 * 2 * 33 * 65 * 4 and size(0, 8, 8) == -1 and size(65536, 8, 8) == -1 and size(1, 0, 8) == -1
    header = open(dicom._lib.__file__.replace("pylinac_amd/_lib.py", "include/pylinac_hip.h")).read()
    assert "#define PL_J2K_MAX_LEVELS %d" % dicom.J2K_MAX_LEVELS in header and "#define PL_J2K_BLOCK_FIELDS 10" in header
