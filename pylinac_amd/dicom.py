"""DICOM native Pixel Data on the device (the DICOM half): the step before the hot path.

``DicomImage`` mirrors the array-producing part of ``pylinac.core.image.DicomImage`` (pylinac/core/image.py:1383-1444, the
properties :1491-1578); ``load_frames`` is the batched form the reference does not have: every file's bytes go to the GPU as
they are, ONE ``pl_dicom_decode`` launch turns the (arbitrarily aligned) Pixel Data values into ``[N, H, W]`` frames -- the
container dtype, ``astype(dtype)`` or the rescaled float64 of ``_rescale_dicom_values`` (image.py:363-389) -- and nothing
comes back to the host.

The reference gets ``pixel_array`` from pydicom (``pydicom>=2.0,<3``, pyproject.toml:40; absent from every environment this
build reaches).  What is restated here is pydicom's documented native path -- ``numpy_handler.get_pixeldata``:
``np.frombuffer(PixelData[:expected_len], pixel_dtype(ds))`` reshaped to (NumberOfFrames, Rows, Columns) -- and the reading
of a Part-10 stream as far as that path needs it (PS3.10 section 7.1 preamble + ``DICM``, PS3.5 section 7.1 data elements,
explicit / implicit VR little endian and explicit VR big endian; sequences are skipped, never entered).

One encapsulated transfer syntax is decoded here as well: RLE Lossless (1.2.840.10008.1.2.5; PS3.5 Annex G, section A.4.2),
which pydicom decodes without a plug-in in a pure-Python byte loop (``rle_handler._rle_decode_segment``).  The item walk
(Basic Offset Table, one fragment per frame, delimiter) and the 64-byte fragment headers are read on the host from the bytes
it already holds; the files go to the device compressed, ``pl_dicom_rle_decode`` (``decode_rle_frames``: three passes over
chunks of ``RLE_CHUNK`` input bytes, launches independent of N, nothing read back) expands the PackBits segments into the
native little-endian frame buffer, and ``pl_dicom_decode`` takes that buffer wherever a conversion, a rescale or the
unused-bit correction is asked for.  ``metadata.PixelDataFragments`` (our name, not pydicom's) lists the fragments as
(offset, length).  The other compressed (encapsulated) transfer syntaxes and deflate belong to pydicom's codec plug-ins and
reader, not to this path: ``NotImplementedError``.

With ``jpeg_lossless=True`` (``read_part10``, ``load_frames``, ``DicomImage``) the two JPEG Lossless syntaxes
(1.2.840.10008.1.2.4.57 and .70: T.81 process 14, Huffman coding, one component) are decoded too: the host reads every frame's
markers (``_jpegll_header``), the frames' payloads go to the device compressed and ``pl_dicom_jpegll_decode``
(``decode_jpeg_lossless_frames``: one wave per frame, one launch, nothing read back) writes the same native buffer.  Without
the keyword they are refused as before.

With ``jpeg2000=True`` the same three take lossless JPEG 2000 files (1.2.840.10008.1.2.4.90 and, with a reversible stream,
.91: T.800, one component, one tile, one layer, the 5/3 transform, code-block style 0): the host reads every frame's main
header and packet headers (``_j2k_codestream``: tier 2), the payloads go to the device compressed and ``pl_dicom_j2k_decode``
(``decode_jpeg2000_frames``: one wave per code block, then the inverse transform) writes the same native buffer.  Without
the keyword they are refused as before.

``load_zip(encapsulated=True)`` reads RLE Lossless and JPEG Lossless files out of ZIP archives: the members are inflated on the
device, where
``pl_dicom_encap_index`` (``index_encapsulated``) walks their items and hands the host every fragment's place and first bytes, and
``pl_copy_ranges`` (``copy_ranges``) lays the fragments of a JPEG frame that spans several end to end.  With ``jpeg2000=True``
as well it reads JPEG 2000 members: the host reads the main header from the fragment's head, ``pl_dicom_j2k_plan``
(``plan_jpeg2000_blocks``: tier 2 on the device, one wave per frame) reads the packet headers where the member lies.
"""
from __future__ import annotations

import struct
import warnings
import zipfile
from dataclasses import dataclass
from functools import partial
from pathlib import Path
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import PL_F32, PL_F64, PL_I16, PL_I32, PL_U8, PL_U16, check
from ._stack_io import bytes_tensor, index_tensor, on_device, source_bytes
from .geometry import Point

MM_PER_INCH = 25.4

IMPLICIT_LE, EXPLICIT_LE, EXPLICIT_BE = "1.2.840.10008.1.2", "1.2.840.10008.1.2.1", "1.2.840.10008.1.2.2"
RLE_LOSSLESS = "1.2.840.10008.1.2.5"
RLE_CHUNK = 1024                                             # PL_DICOM_RLE_CHUNK: input bytes per chunk of the three passes
_RLE_SHORT = "The amount of decoded RLE segment data doesn't match the expected amount"
_RLE_PADDING = "The decoded RLE segment contains non-conformant padding"
JPEG_LOSSLESS = ("1.2.840.10008.1.2.4.57", "1.2.840.10008.1.2.4.70")   # T.81 process 14: any predictor / first-order prediction
JPEG_2000 = ("1.2.840.10008.1.2.4.90", "1.2.840.10008.1.2.4.91")       # T.800: lossless only / either; a reversible stream is decoded
J2K_MAX_LEVELS = 16                                          # PL_J2K_MAX_LEVELS: decomposition levels the device decode walks
JPEGLL_MAX_COLS = 8192                                       # PL_DICOM_JPEGLL_MAX_COLS: the rows the kernel buffers in LDS
_LONG_VRS = {b"OB", b"OD", b"OF", b"OL", b"OV", b"OW", b"SQ", b"UC", b"UN", b"UR", b"UT", b"SV", b"UV"}

# (group, element) -> (keyword, VR): the elements the image classes read (the VR column serves implicit-VR streams)
_TAGS = {
    (0x0002, 0x0010): ("TransferSyntaxUID", "UI"), (0x0008, 0x0016): ("SOPClassUID", "UI"), (0x0008, 0x0018): ("SOPInstanceUID", "UI"),
    (0x0008, 0x0060): ("Modality", "CS"), (0x0008, 0x0070): ("Manufacturer", "LO"), (0x0008, 0x0022): ("AcquisitionDate", "DA"),
    (0x0008, 0x0020): ("StudyDate", "DA"), (0x0008, 0x0023): ("ContentDate", "DA"), (0x0008, 0x0008): ("ImageType", "CS"),
    (0x0018, 0x0050): ("SliceThickness", "DS"), (0x0018, 0x0088): ("SpacingBetweenSlices", "DS"),
    (0x0018, 0x1110): ("DistanceSourceToDetector", "DS"),
    (0x0020, 0x000E): ("SeriesInstanceUID", "UI"), (0x0020, 0x0013): ("InstanceNumber", "IS"),
    (0x0020, 0x0032): ("ImagePositionPatient", "DS"), (0x0020, 0x1041): ("SliceLocation", "DS"),
    (0x0028, 0x0002): ("SamplesPerPixel", "US"), (0x0028, 0x0004): ("PhotometricInterpretation", "CS"),
    (0x0028, 0x0008): ("NumberOfFrames", "IS"), (0x0028, 0x0010): ("Rows", "US"), (0x0028, 0x0011): ("Columns", "US"),
    (0x0028, 0x0030): ("PixelSpacing", "DS"), (0x0028, 0x0100): ("BitsAllocated", "US"), (0x0028, 0x0101): ("BitsStored", "US"),
    (0x0028, 0x0102): ("HighBit", "US"), (0x0028, 0x0103): ("PixelRepresentation", "US"),
    (0x0028, 0x1040): ("PixelIntensityRelationship", "CS"), (0x0028, 0x1041): ("PixelIntensityRelationshipSign", "SS"),
    (0x0028, 0x1052): ("RescaleIntercept", "DS"), (0x0028, 0x1053): ("RescaleSlope", "DS"),
    (0x3002, 0x0011): ("ImagePlanePixelSpacing", "DS"), (0x3002, 0x000D): ("XRayImageReceptorTranslation", "DS"),
    (0x3002, 0x0022): ("RadiationMachineSAD", "DS"), (0x3002, 0x0026): ("RTImageSID", "DS"),
    (0x300A, 0x011E): ("GantryAngle", "DS"), (0x300A, 0x0120): ("BeamLimitingDeviceAngle", "DS"),
    (0x300A, 0x0122): ("PatientSupportAngle", "DS"),
    (0x7FE0, 0x0008): ("FloatPixelData", "OF"), (0x7FE0, 0x0009): ("DoubleFloatPixelData", "OD"), (0x7FE0, 0x0010): ("PixelData", "OW"),
}
_BULK = {"PixelData", "FloatPixelData", "DoubleFloatPixelData"}


class Metadata:
    """The parsed elements by pydicom keyword: attribute access raises ``AttributeError`` for an absent tag and ``get`` returns
    a default, like ``pydicom.Dataset`` -- which is all the reference's image code asks of ``self.metadata``."""

    def __init__(self, values: dict):
        self.__dict__["_values"] = values

    def __getattr__(self, name):
        try:
            return self._values[name]
        except KeyError:
            raise AttributeError(name) from None

    def __contains__(self, name) -> bool:
        return name in self._values

    def get(self, name, default=None):
        return self._values.get(name, default)

    def keys(self):
        return self._values.keys()


def _value(vr: str, raw: bytes, big: bool):
    e = ">" if big else "<"
    if vr in ("US", "SS", "UL", "SL", "FL", "FD"):
        code = {"US": "H", "SS": "h", "UL": "I", "SL": "i", "FL": "f", "FD": "d"}[vr]
        n = len(raw) // struct.calcsize(code)
        vals = struct.unpack(e + code * n, raw[:n * struct.calcsize(code)])
        return vals[0] if n == 1 else list(vals)
    text = raw.decode("latin-1").rstrip(" \x00")
    if vr in ("DS", "IS"):
        parts = [p.strip() for p in text.split("\\")] if text else []
        conv = float if vr == "DS" else (lambda s: int(float(s)))
        vals = [conv(p) for p in parts if p != ""]
        return None if not vals else (vals[0] if len(vals) == 1 else vals)
    if "\\" in text and vr in ("CS", "LO", "SH", "UI"):
        return text.split("\\")
    return text


def _skip_undefined(buf: memoryview, pos: int, explicit: bool, big: bool) -> int:
    """-> the position after the Sequence Delimitation Item that closes an undefined-length value starting at ``pos``
    (PS3.5 section 7.5: items (FFFE,E000) of defined or undefined length, closed by (FFFE,E0DD))."""
    e = ">" if big else "<"
    while True:
        g, el, ln = struct.unpack_from(e + "HHI", buf, pos)
        pos += 8
        if (g, el) == (0xFFFE, 0xE0DD):
            return pos
        if (g, el) != (0xFFFE, 0xE000):
            raise ValueError("malformed sequence: an item tag was expected")
        if ln != 0xFFFFFFFF:
            pos += ln
            continue
        while True:                                        # an item of undefined length: data elements until (FFFE,E00D)
            g, el = struct.unpack_from(e + "HH", buf, pos)
            if (g, el) == (0xFFFE, 0xE00D):
                pos += 8
                break
            pos, _, _, _, _ = _element(buf, pos, explicit, big)


def _fragments(buf: memoryview, pos: int, out: list, frame_table: list | None = None) -> int:
    """The items of an encapsulated Pixel Data value starting at ``pos`` (PS3.5 section A.4): the Basic Offset Table, then one
    item per fragment, closed by (FFFE,E0DD) -> the position after the delimiter; ``out`` receives (offset, length) of every
    fragment.  A filled Basic Offset Table must agree with the walk (RLE: one fragment per frame, section A.4.2).
    ``frame_table`` (JPEG Lossless: a frame may span fragments): a list that receives the table, whose entries must then
    start at 0, increase and each name the item tag of a fragment."""
    n, table, tags = len(buf), None, []
    while True:
        if pos + 8 > n:
            raise ValueError(_ITEMS_NO_DELIMITER)
        g, el, ln = struct.unpack_from("<HHI", buf, pos)
        if (g, el) == (0xFFFE, 0xE0DD):
            break
        if (g, el) != (0xFFFE, 0xE000) or ln == 0xFFFFFFFF or pos + 8 + ln > n:
            raise ValueError(_ITEMS_NO_ITEM)
        if table is None:
            if ln % 4:
                raise ValueError(_ITEMS_TABLE_LENGTH)
            table = list(struct.unpack_from(f"<{ln // 4}I", buf, pos + 8))
        else:
            tags.append(pos)
            out.append((pos + 8, ln))
        pos += 8 + ln
    if table is None:
        raise ValueError(_ITEMS_NO_TABLE)
    _check_offset_table(table, tags, frame_table is not None)
    if frame_table is not None:
        frame_table.extend(table)
    return pos + 8


_ITEMS = "malformed encapsulated Pixel Data: "
_ITEMS_NO_DELIMITER = _ITEMS + "the sequence delimiter is missing"
_ITEMS_NO_ITEM = _ITEMS + "an item of defined length inside the file was expected"
_ITEMS_TABLE_LENGTH = _ITEMS + "the Basic Offset Table is no list of uint32 values"
_ITEMS_NO_TABLE = _ITEMS + "the Basic Offset Table item is missing"
_HEADER_ONLY = object()         # ``_element(fragments=...)``: stop at the header of an encapsulated (7FE0,0010), walk no item


def _check_offset_table(table: list, tags: list, frames_span: bool) -> None:
    """A filled Basic Offset Table against the item tags found (``_fragments``): RLE, one fragment per frame -- the table IS
    the tags' offsets from the first; ``frames_span`` (JPEG Lossless) -- it starts at 0, increases and names item tags."""
    starts = [t - tags[0] for t in tags]
    if not frames_span:
        agrees = not table or table == starts
    else:
        agrees = not table or (table[0] == 0 and all(b > a for a, b in zip(table, table[1:])) and set(table) <= set(starts))
    if not agrees:
        raise ValueError(_ITEMS + "the Basic Offset Table disagrees with the fragments that follow it")


def _element(buf: memoryview, pos: int, explicit: bool, big: bool, fragments: list | None = None, frame_table: list | None = None):
    """One data element at ``pos`` -> (position after it, (group, element), VR or None, value offset, value length).
    ``fragments``: a list that receives the fragments of an encapsulated (7FE0,0010) -- RLE Lossless, JPEG Lossless with
    ``frame_table`` (``_fragments``); None refuses them; ``_HEADER_ONLY`` returns at the value's first item."""
    e = ">" if big else "<"
    g, el = struct.unpack_from(e + "HH", buf, pos)
    pos += 4
    vr = None
    if explicit and g != 0xFFFE:
        vrb = bytes(buf[pos:pos + 2])
        vr = vrb.decode("latin-1")
        if vrb in _LONG_VRS:
            (ln,) = struct.unpack_from(e + "I", buf, pos + 4)
            pos += 8
        else:
            (ln,) = struct.unpack_from(e + "H", buf, pos + 2)
            pos += 4
    else:
        (ln,) = struct.unpack_from(e + "I", buf, pos)
        pos += 4
    start = pos
    if ln == 0xFFFFFFFF:
        if (g, el) == (0x7FE0, 0x0010):
            if fragments is _HEADER_ONLY:
                return pos, (g, el), vr, start, -1
            if fragments is not None:
                return _fragments(buf, pos, fragments, frame_table), (g, el), vr, start, -1
            raise NotImplementedError("encapsulated (compressed) Pixel Data: decoded by pydicom's codec plug-ins, not by this path")
        return _skip_undefined(buf, pos, explicit, big), (g, el), vr, start, -1
    return pos + ln, (g, el), vr, start, ln


def read_part10(source, jpeg_lossless: bool = False, jpeg2000: bool = False) -> tuple[Metadata, np.ndarray]:
    """``pydicom.dcmread(source, force=True)`` as far as the image classes need it -> (metadata, the file's bytes as a uint8
    array).  ``metadata.PixelData`` (``FloatPixelData`` / ``DoubleFloatPixelData``) is the pair (offset, length) of the value
    inside those bytes -- the samples are never copied on the host.  RLE Lossless: ``PixelData`` is (offset, -1) and
    ``metadata.PixelDataFragments`` the list of (offset, length) of the fragments.  ``jpeg_lossless=True`` walks the items of
    the two JPEG Lossless syntaxes (``JPEG_LOSSLESS``) the same way; ``metadata.PixelDataOffsetTable`` is then the Basic
    Offset Table (a list, empty or one entry per frame).  Without it they are refused like every other encapsulated syntax.
    ``jpeg2000=True`` does the same for the two JPEG 2000 syntaxes (``JPEG_2000``)."""
    data = np.frombuffer(source_bytes(source), dtype=np.uint8)
    return _walk_part10(memoryview(data).cast("B"), jpeg_lossless=jpeg_lossless, jpeg2000=jpeg2000), data


class _PrefixTooShort(Exception):
    """the prefix of a member ends before its (7FE0,0010) element header"""


def _walk_part10(buf: memoryview, size: int | None = None, jpeg_lossless: bool = False, encapsulated: bool = False,
                 jpeg2000: bool = False) -> Metadata:
    """The element walk of ``read_part10`` over ``buf``.  ``size`` None: ``buf`` is the whole file.  Otherwise the PREFIX form
    ``load_zip`` uses: ``buf`` holds the first bytes of a file of ``size`` bytes, the walk stops at the Pixel Data element
    header -- (offset, length) of its value are validated against ``size``, not against the prefix -- and raises
    ``_PrefixTooShort`` when the prefix ends before it (an element that is cut off is never read).  ``encapsulated`` (the
    prefix form only): a Pixel Data element of undefined length in an RLE Lossless or a JPEG Lossless file (with ``jpeg2000``
    a JPEG 2000 file) ends the walk too, ``PixelData`` = (offset of its first item, -1); the items are walked on the device."""
    n = len(buf)
    whole = size is None or n >= size
    try:
        return _walk_elements(buf, n, size, whole, jpeg_lossless, encapsulated and size is not None, jpeg2000)
    except struct.error:
        if whole:
            raise
        raise _PrefixTooShort from None


def _walk_elements(buf: memoryview, n: int, size, whole: bool, jpeg_lossless: bool = False, items_later: bool = False,
                   jpeg2000: bool = False) -> Metadata:
    pos = 132 if n >= 132 and bytes(buf[128:132]) == b"DICM" else 0
    values: dict = {}
    ts = IMPLICIT_LE if pos == 0 else EXPLICIT_LE          # (no preamble, force=True: pydicom assumes implicit VR little endian)
    # the File Meta group is always explicit VR little endian (PS3.10 section 7.1)
    while pos + 8 <= n and struct.unpack_from("<H", buf, pos)[0] == 0x0002:
        pos, tag, vr, start, ln = _element(buf, pos, True, False)
        if pos > n and not whole:
            raise _PrefixTooShort
        if tag in _TAGS and ln >= 0:
            values[_TAGS[tag][0]] = _value(vr or _TAGS[tag][1], bytes(buf[start:start + ln]), False)
    ts = values.get("TransferSyntaxUID", ts)
    if ts not in (IMPLICIT_LE, EXPLICIT_LE, EXPLICIT_BE):
        if ts == "1.2.840.10008.1.2.1.99":
            raise NotImplementedError("Deflated Explicit VR Little Endian is inflated by pydicom's reader, not by this path")
        explicit, big = True, False                         # every encapsulated syntax is explicit VR little endian
    else:
        explicit, big = ts != IMPLICIT_LE, ts == EXPLICIT_BE
    if size is not None and ts == RLE_LOSSLESS and not items_later:
        raise NotImplementedError("RLE Lossless Pixel Data inside an archive: the segment headers lie inside the compressed part; "
                                  "extract the member and use load_frames")
    # the syntaxes whose frames may span fragments, each behind its keyword: JPEG Lossless and JPEG 2000 are walked alike
    spanning = size is None and ((jpeg_lossless and ts in JPEG_LOSSLESS) or (jpeg2000 and ts in JPEG_2000))
    fragments = [] if ts == RLE_LOSSLESS or spanning else None
    if items_later and (ts == RLE_LOSSLESS or ts in JPEG_LOSSLESS or (jpeg2000 and ts in JPEG_2000)):
        fragments = _HEADER_ONLY
    frame_table = [] if spanning else None
    while pos + 8 <= n:
        pos, tag, vr, start, ln = _element(buf, pos, explicit, big, fragments, frame_table)
        if size is not None and tag == (0x7FE0, 0x0010):    # the prefix form ends here: the value is judged against the file
            if ln < 0 and start > size:
                raise ValueError(f"the encapsulated Pixel Data value (at offset {start}) lies outside the file ({size} bytes)")
            if ln >= 0 and (start > size or ln > size - start):
                raise ValueError(f"the Pixel Data value ({ln} bytes at offset {start}) lies outside the file ({size} bytes)")
            values["PixelData"] = (start, ln)
            break
        if pos > n and not whole:
            raise _PrefixTooShort
        if tag == (0x7FE0, 0x0010) and ln < 0:
            values["PixelData"], values["PixelDataFragments"] = (start, -1), fragments
            if spanning:
                values["PixelDataOffsetTable"] = frame_table
        if tag not in _TAGS or ln < 0:
            continue
        key, table_vr = _TAGS[tag]
        if key in _BULK:
            values[key] = (start, ln)
        else:
            values[key] = _value(vr if vr and vr != "UN" else table_vr, bytes(buf[start:start + ln]), big)
    else:
        if not whole:
            raise _PrefixTooShort
    values.setdefault("TransferSyntaxUID", ts)
    return Metadata(values)


_CONTAINERS = {(8, 0): torch.uint8, (8, 1): torch.int8, (16, 0): torch.uint16, (16, 1): torch.int16, (32, 0): torch.uint32,
               (32, 1): torch.int32}


class _Layout(NamedTuple):
    container: torch.dtype
    sample_bytes: int
    frames: int
    rows: int
    cols: int
    big_endian: bool
    value: tuple                                             # (offset, length) of the Pixel Data value; length -1: encapsulated

    @property
    def format(self):                                        # what the files of one stack must agree in
        return self.container, self.rows, self.cols, self.big_endian


def _layout(meta: Metadata) -> _Layout:
    """pydicom.pixel_data_handlers.util.pixel_dtype + get_expected_length for native data."""
    for need in ("BitsAllocated", "Rows", "Columns", "PixelRepresentation", "SamplesPerPixel"):
        if need not in meta:
            raise AttributeError(f"Unable to convert the pixel data as the following required elements are missing from the dataset: {need}")
    if "PixelData" not in meta:
        raise AttributeError("Unable to convert the pixel data: one of Pixel Data, Float Pixel Data or Double Float Pixel Data "
                             "must be present in the dataset" if "FloatPixelData" not in meta and "DoubleFloatPixelData" not in meta
                             else "Float Pixel Data / Double Float Pixel Data are float32 / float64 arrays as stored: read them with numpy")
    if int(meta.SamplesPerPixel) != 1:
        raise NotImplementedError("SamplesPerPixel = 1 only (the image classes of the hot path are single-channel)")
    bits, rep = int(meta.BitsAllocated), int(meta.PixelRepresentation)
    if bits not in (8, 16, 32):
        raise NotImplementedError(f"BitsAllocated {bits}: 8, 16 and 32 are decoded on the device")
    if rep not in (0, 1):
        raise ValueError(f"Unable to determine the data type to use to contain the Pixel Data as a value of '{rep}' for "
                         "'(0028,0103) Pixel Representation' is invalid")
    return _Layout(_CONTAINERS[(bits, rep)], bits // 8, int(meta.get("NumberOfFrames") or 1), int(meta.Rows), int(meta.Columns),
                   meta.get("TransferSyntaxUID") == EXPLICIT_BE, meta.PixelData)


_NP_TO_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}


def decode_frames(file_bytes, offsets, rows: int, cols: int, bits_allocated: int, bits_stored: int, pixel_representation: int,
                  big_endian: bool = False, correct_unused_bits: bool = False, out: str = "container", rescale=None,
                  device=None) -> torch.Tensor:
    """``pl_dicom_decode``: frames of one format anywhere inside ``file_bytes`` (uint8 array / tensor; device tensors are used
    in place) -> device tensor [N, rows, cols].  ``out``: "container" | "float32" | "float64"; ``rescale`` = (slope, intercept)
    with "float64".  Raises ``ValueError`` when a frame does not lie inside the buffer (pydicom: "The length of the pixel
    data in the dataset doesn't match the expected length")."""
    dev = on_device(device)
    buf = file_bytes if isinstance(file_bytes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(file_bytes, dtype=np.uint8))
    buf = buf.to(device=dev, dtype=torch.uint8).contiguous()
    offs = index_tensor(offsets, torch.int64, dev)
    n = int(offs.numel())
    bits, rep = int(bits_allocated), int(pixel_representation)
    code = {8: PL_U8, 16: PL_I16 if rep else PL_U16, 32: PL_I32}[bits]
    odt, ocode = {"container": (_CONTAINERS[(bits, rep)], code), "float32": (torch.float32, PL_F32),
                  "float64": (torch.float64, PL_F64)}[out]
    res = torch.empty((n, rows, cols), dtype=odt, device=dev)
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    slope, intercept = (float(rescale[0]), float(rescale[1])) if rescale is not None else (1.0, 0.0)
    check(_lib.load().pl_dicom_decode(buf.data_ptr(), buf.numel(), offs.data_ptr(), n, rows, cols, bits,
                                      int(bits_stored), rep, int(bool(big_endian)), int(bool(correct_unused_bits)), res.data_ptr(),
                                      ocode, int(rescale is not None), slope, intercept, status.data_ptr(),
                                      torch.cuda.current_stream(dev).cuda_stream), "pl_dicom_decode")
    res._pl_status = status                                  # checked by the caller that wants the error (one sync)
    return res


def decode_rle_frames(file_bytes, seg_off, seg_len, rows: int, cols: int, bits_allocated: int, bits_stored: int | None = None,
                      pixel_representation: int = 0, correct_unused_bits: bool = False, out: str = "container", rescale=None,
                      device=None, max_segment_bytes: int | None = None, native: torch.Tensor | None = None) -> torch.Tensor:
    """``pl_dicom_rle_decode``, the RLE Lossless counterpart of ``decode_frames``: N frames whose PackBits segments lie
    anywhere inside ``file_bytes`` (uint8 array / tensor; device tensors are used in place); ``seg_off`` / ``seg_len`` are
    int64 [N, BitsAllocated / 8]: segment s of a frame (the most significant byte plane first) is ``seg_len[f, s]`` bytes at
    byte ``seg_off[f, s]``.  -> device tensor [N, rows, cols] exactly as ``decode_frames`` gives it for the same frames
    stored native (``out``, ``rescale``, ``correct_unused_bits``: the decoded little-endian buffer goes through
    ``pl_dicom_decode``; the plain container dtype IS that buffer, returned as a view).  ``_pl_status`` int32 [N]: bit 0 a
    segment window outside the buffer (the frame is left untouched), bit 1 a segment decoded to fewer than rows * cols
    bytes, bit 2 to more (the frame is complete).  ``max_segment_bytes``: an upper bound of ``seg_len`` (taken from a host
    array when absent; a device tensor is reduced and read back once).  ``native``: a uint8 device tensor
    [N, rows * cols * BitsAllocated / 8] to decode into."""
    dev = on_device(device)
    bits, rep = int(bits_allocated), int(pixel_representation)
    segments = bits // 8
    if max_segment_bytes is None:
        max_segment_bytes = int(seg_len.max()) if isinstance(seg_len, torch.Tensor) else int(np.max(seg_len, initial=0))
    buf = bytes_tensor(file_bytes, dev)
    so = index_tensor(seg_off, torch.int64, dev).reshape(-1, segments)
    sl = index_tensor(seg_len, torch.int64, dev).reshape(-1, segments)
    n = int(so.shape[0])
    if so.shape != sl.shape:
        raise ValueError("decode_rle_frames: seg_off and seg_len must both be [N, BitsAllocated / 8]")
    native = _native_buffer(native, n, rows * cols * segments, dev, "decode_rle_frames")
    lib = _lib.load()
    nwork = int(lib.pl_dicom_rle_work_bytes(n, segments, int(max_segment_bytes)))
    work = torch.empty(max(nwork, 16), dtype=torch.uint8, device=dev)
    status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    check(lib.pl_dicom_rle_decode(buf.data_ptr(), buf.numel(), so.data_ptr(), sl.data_ptr(), n, segments, int(max_segment_bytes),
                                  rows, cols, native.data_ptr(), status.data_ptr(), work.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream), "pl_dicom_rle_decode")
    return _from_native(native, status[:n], rows, cols, bits, bits_stored, rep, correct_unused_bits, out, rescale, dev)


def _native_buffer(native, n: int, frame_bytes: int, dev, who: str) -> torch.Tensor:
    """the ``native=`` argument of the two encapsulated decodes, validated under ``who``'s name; None: allocated"""
    if native is None:
        return torch.empty((n, frame_bytes), dtype=torch.uint8, device=dev)
    if native.dtype != torch.uint8 or tuple(native.shape) != (n, frame_bytes) or not native.is_contiguous() or not native.is_cuda:
        raise ValueError(f"{who}: native must be a contiguous uint8 device tensor [N, rows * cols * BitsAllocated / 8]")
    return native


def _from_native(native: torch.Tensor, status: torch.Tensor, rows: int, cols: int, bits: int, bits_stored, rep: int,
                 correct_unused_bits: bool, out: str, rescale, dev) -> torch.Tensor:
    """The tail the RLE and the JPEG Lossless decodes share: the decoded little-endian buffer [N, frame bytes] -> [N, rows,
    cols] -- a view for the plain container dtype, through ``pl_dicom_decode`` otherwise -- carrying ``status``."""
    n, frame_bytes = int(native.shape[0]), int(native.shape[1])
    stored = bits if bits_stored is None else int(bits_stored)
    if out == "container" and not (correct_unused_bits and stored < bits):
        res = native.view(_CONTAINERS[(bits, rep)]).reshape(n, rows, cols)
    else:
        res = decode_frames(native.reshape(-1), torch.arange(n, dtype=torch.int64, device=dev) * frame_bytes, rows, cols, bits,
                            stored, rep, big_endian=False, correct_unused_bits=correct_unused_bits, out=out, rescale=rescale,
                            device=dev)
    res._pl_status = status
    return res


def _rle_segments(header, fragment: tuple, segments: int, name: str):
    """The 64-byte header of one RLE fragment (PS3.5 section G.5: the number of segments, then 15 offsets from the start of the
    header) -> [(offset, length)] of its segments, in the frame of reference of ``fragment`` = (offset, length); ``header``:
    the fragment's first bytes (64 of them are read when the fragment is that long).  ``ValueError`` for a header that is
    malformed."""
    off, ln = fragment
    if ln < 64:
        raise ValueError(f"{name}: the RLE fragment is shorter than its 64-byte header")
    head = struct.unpack_from("<16I", header, 0)
    if head[0] != segments:
        raise ValueError(f"{name}: the RLE header states {head[0]} segments where BitsAllocated / 8 = {segments} are expected")
    offs = list(head[1:1 + segments])
    if any(b <= a for a, b in zip(offs, offs[1:])):
        raise ValueError(f"{name}: the segment offsets of the RLE header are not strictly increasing")
    if offs[-1] > ln:
        raise ValueError(f"{name}: a segment offset of the RLE header lies outside the fragment")
    return [(off + a, b - a) for a, b in zip(offs, offs[1:] + [ln])]


def _check_rle_status(status: torch.Tensor, owner, names) -> None:
    """pydicom's answers to the status of ``decode_rle_frames`` (one transfer): ``ValueError`` for the first frame with a
    short segment (or a window outside the buffer), one warning for segments that decoded to more than the plane."""
    flags = status.cpu().numpy()
    bad = np.flatnonzero(flags & 3)
    if bad.size:
        raise ValueError(f"{_RLE_SHORT} ({names[owner[int(bad[0])]]}, frame {int(bad[0])} of the stack)")
    if (flags & 4).any():
        warnings.warn(f"{_RLE_PADDING} ({names[owner[int(np.flatnonzero(flags & 4)[0])]]})")


def _jpegll_cols(cols: int) -> None:
    if cols > JPEGLL_MAX_COLS:
        raise ValueError(f"JPEG Lossless frames of {cols} columns: the device decode buffers rows of at most {JPEGLL_MAX_COLS} samples")


def _jpegll_refusals(ib: int, cols: int) -> None:
    """what a JPEG Lossless stack is refused for before any of its streams is read (``load_frames`` and ``load_zip``)"""
    if ib not in (1, 2):
        raise NotImplementedError(f"JPEG Lossless Pixel Data with BitsAllocated {ib * 8}: 8 and 16 are decoded on the device")
    _jpegll_cols(cols)


def decode_jpeg_lossless_frames(file_bytes, scan_off, scan_len, params, huff, rows: int, cols: int, bits_allocated: int,
                                bits_stored: int | None = None, pixel_representation: int = 0, correct_unused_bits: bool = False,
                                out: str = "container", rescale=None, device=None,
                                native: torch.Tensor | None = None) -> torch.Tensor:
    """``pl_dicom_jpegll_decode``, the JPEG Lossless counterpart of ``decode_rle_frames`` (T.81 process 14, Annex H): N frames
    whose entropy-coded segments lie anywhere inside ``file_bytes`` (uint8 array / tensor; device tensors are used in place).
    ``scan_off`` / ``scan_len`` int64 [N]: the bytes after each frame's SOS header, up to EOI or the fragment's end;
    ``params`` int32 [N, 4]: precision, selection value, point transform, restart interval in samples (0: none); ``huff``
    uint8 [N, 33]: BITS[16] then HUFFVAL[17] of the table SOS selects.  One wave decodes one frame.  -> device tensor
    [N, rows, cols] exactly as ``decode_frames`` gives it for the same samples stored native, zero-extended into the
    container (``out``, ``rescale``, ``correct_unused_bits``: the decoded little-endian buffer goes through
    ``pl_dicom_decode``; the plain container dtype IS that buffer, returned as a view).  ``_pl_status`` int32 [N]: bit 0 a
    window outside the buffer or an unsound parameter (the frame is left untouched), bit 1 the data ends before rows * cols
    samples, bit 2 corrupt data (a code outside the table, a wrong restart marker).  ``native``: a uint8 device tensor
    [N, rows * cols * BitsAllocated / 8] to decode into.  ``ValueError`` for more than ``JPEGLL_MAX_COLS`` columns."""
    _jpegll_cols(cols)
    dev = on_device(device)
    bits, rep = int(bits_allocated), int(pixel_representation)
    if bits not in (8, 16):
        raise ValueError("decode_jpeg_lossless_frames: BitsAllocated 8 or 16")
    buf = bytes_tensor(file_bytes, dev)
    so, sl = index_tensor(scan_off, torch.int64, dev).reshape(-1), index_tensor(scan_len, torch.int64, dev).reshape(-1)
    n = int(so.numel())
    par = index_tensor(params, torch.int32, dev).reshape(-1, 4)
    tab = bytes_tensor(huff, dev).reshape(-1, 33)
    if not (sl.numel() == par.shape[0] == tab.shape[0] == n):
        raise ValueError("decode_jpeg_lossless_frames: scan_off and scan_len [N], params [N, 4] and huff [N, 33] must agree in N")
    native = _native_buffer(native, n, rows * cols * (bits // 8), dev, "decode_jpeg_lossless_frames")
    lib = _lib.load()
    nwork = int(lib.pl_dicom_jpegll_work_bytes(n, rows, cols))
    work = torch.empty(max(nwork, 16), dtype=torch.uint8, device=dev)
    status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    check(lib.pl_dicom_jpegll_decode(buf.data_ptr(), buf.numel(), so.data_ptr(), sl.data_ptr(), par.data_ptr(), tab.data_ptr(), n,
                                     rows, cols, bits // 8, native.data_ptr(), status.data_ptr(), work.data_ptr(),
                                     torch.cuda.current_stream(dev).cuda_stream), "pl_dicom_jpegll_decode")
    return _from_native(native, status[:n], rows, cols, bits, bits_stored, rep, correct_unused_bits, out, rescale, dev)


_SOF_REFUSED = {0xC0: "SOF0 (baseline DCT)", 0xC1: "SOF1 (extended sequential DCT)", 0xC2: "SOF2 (progressive DCT)",
                0xC5: "SOF5 (differential sequential DCT)", 0xC6: "SOF6 (differential progressive DCT)",
                0xC7: "SOF7 (differential lossless)", 0xC8: "JPG (reserved)", 0xC9: "SOF9 (arithmetic coding)",
                0xCA: "SOF10 (arithmetic coding)", 0xCB: "SOF11 (lossless, arithmetic coding)",
                0xCD: "SOF13 (arithmetic coding)", 0xCE: "SOF14 (arithmetic coding)", 0xCF: "SOF15 (arithmetic coding)",
                0xCC: "DAC (arithmetic conditioning)", 0xDC: "DNL (number of lines)", 0xDE: "DHP (hierarchical)",
                0xDF: "EXP (hierarchical)"}


def _jpegll_header(data, rows: int, cols: int, bits: int, name: str, total: int | None = None):
    """The markers of one frame's JPEG stream up to its scan (T.81 Annex B) -> (offset of the entropy-coded segment inside
    ``data``, its length up to the end of the stream, [P, selection value, Pt, restart interval], the 33 bytes BITS + HUFFVAL
    of the table SOS selects).  Every offset is checked against the stream.  ``NotImplementedError`` for a process other than
    Huffman-coded lossless (any SOFn but SOF3, DAC, DNL, hierarchical markers) and for more than one component;
    ``ValueError`` for a malformed stream.  ``total``: ``data`` holds only the first bytes of a stream of ``total`` bytes
    (``load_zip``: the stream lies on the device); a check that fails only because ``data`` ends raises ``_PrefixTooShort``,
    a malformed stream is reported when it is certain."""
    data = bytes(data)
    n = len(data)
    size = n if total is None else total                    # the stream's length

    def ends(text):                                         # the bytes given end here: the stream's end, or only the prefix's
        if n < size:
            raise _PrefixTooShort
        raise ValueError(f"{name}: {text}")

    if n < 2 and n < size:
        raise _PrefixTooShort
    if n < 2 or data[:2] != b"\xff\xd8":
        raise ValueError(f"{name}: the JPEG stream does not start with SOI")
    pos, tables, interval, frame = 2, {}, 0, None
    while True:
        while pos + 1 < n and data[pos] == 0xFF and data[pos + 1] == 0xFF:         # fill bytes before a marker (B.1.1.2)
            pos += 1
        if pos + 2 > n:
            ends("the JPEG stream ends without SOS (no scan)")
        if data[pos] != 0xFF:
            raise ValueError(f"{name}: a JPEG marker was expected at byte {pos} of the frame")
        m = data[pos + 1]
        if m == 0xD9:
            raise ValueError(f"{name}: EOI without SOS (no scan)")
        if m == 0x01 or 0xD0 <= m <= 0xD8:                                          # stand-alone markers
            pos += 2
            continue
        if pos + 4 > n:
            ends("the JPEG stream ends without SOS (no scan)")
        ln = struct.unpack_from(">H", data, pos + 2)[0]
        if ln < 2 or pos + 2 + ln > size:
            raise ValueError(f"{name}: the segment of marker FF{m:02X} lies outside the fragment")
        if pos + 2 + ln > n:
            raise _PrefixTooShort
        seg = data[pos + 4:pos + 2 + ln]
        if m in _SOF_REFUSED:
            raise NotImplementedError(f"{name}: {_SOF_REFUSED[m]}, marker FF{m:02X}: only Huffman-coded lossless JPEG (SOF3) "
                                      "is decoded by this path")
        if m == 0xC3:
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                raise ValueError(f"{name}: malformed SOF3 segment")
            p, y, x, nf = seg[0], struct.unpack_from(">H", seg, 1)[0], struct.unpack_from(">H", seg, 3)[0], seg[5]
            if nf != 1:
                raise NotImplementedError(f"{name}: SOF3 with Nf = {nf} components: single-component frames only")
            if y == 0:
                raise NotImplementedError(f"{name}: SOF3 with Y = 0 leaves the number of lines to a DNL marker")
            if not 2 <= p <= 16:
                raise ValueError(f"{name}: SOF3 precision {p} (2 .. 16)")
            if p > bits:
                raise ValueError(f"{name}: SOF3 precision {p} exceeds BitsAllocated = {bits}")
            if (y, x) != (rows, cols):
                raise ValueError(f"{name}: SOF3 states Y x X = {y} x {x} where Rows x Columns = {rows} x {cols}")
            frame = (p, seg[6])
        elif m == 0xC4:
            at = 0
            while at < len(seg):
                if at + 17 > len(seg):
                    raise ValueError(f"{name}: a DHT table definition is cut off")
                tc, th = seg[at] >> 4, seg[at] & 15
                counts = seg[at + 1:at + 17]
                symbols = sum(counts)
                if tc != 0 or th > 3:
                    raise ValueError(f"{name}: DHT table class {tc}, id {th}: lossless scans use class 0, ids 0 .. 3")
                if symbols > 17:
                    raise ValueError(f"{name}: a DHT table of {symbols} symbols (at most 17 categories, 0 .. 16)")
                if at + 17 + symbols > len(seg):
                    raise ValueError(f"{name}: a DHT table definition is cut off")
                values = seg[at + 17:at + 17 + symbols]
                if any(v > 16 for v in values):
                    raise ValueError(f"{name}: a DHT table holds the symbol {max(values)} (categories 0 .. 16)")
                if sum(c << (15 - k) for k, c in enumerate(counts)) > 1 << 16:
                    raise ValueError(f"{name}: a DHT table is over-subscribed (Kraft sum above 1)")
                tables[th] = bytes(counts) + values + b"\xff" * (17 - symbols)   # (a later definition replaces the earlier)
                at += 17 + symbols
        elif m == 0xDD:
            if ln != 4:
                raise ValueError(f"{name}: malformed DRI segment")
            interval = struct.unpack_from(">H", seg, 0)[0]
        elif m == 0xDA:
            if frame is None:
                raise ValueError(f"{name}: SOS before SOF3")
            if len(seg) < 1 or seg[0] != 1 or len(seg) != 6:
                raise ValueError(f"{name}: SOS with Ns = {seg[0] if seg else '?'}: one component per scan")
            cs, td, ss, ah, al = seg[1], seg[2] >> 4, seg[3], seg[5] >> 4, seg[5] & 15
            if cs != frame[1]:
                raise ValueError(f"{name}: SOS selects component {cs}, SOF3 defines {frame[1]}")
            if not 1 <= ss <= 7:
                raise ValueError(f"{name}: SOS selection value {ss} (lossless predictors 1 .. 7)")
            if ah != 0 or al >= frame[0]:
                raise ValueError(f"{name}: SOS with Ah = {ah}, point transform {al} at precision {frame[0]}")
            if td not in tables:
                raise ValueError(f"{name}: SOS selects the Huffman table {td}, which no DHT defines")
            if interval % cols:
                raise ValueError(f"{name}: the restart interval {interval} is not a whole number of rows of {cols} samples "
                                 "(T.81 H.1.1)")
            start = pos + 2 + ln
            return start, size - start, [frame[0], ss, al, interval], tables[td]
        pos += 2 + ln                                                               # APPn, COM, DQT, ...: skipped


def _jpegll_frames(meta: Metadata, frames: int, name: str, codec: str = "JPEG") -> list:
    """The fragments of each frame of a JPEG Lossless (or, ``codec``, JPEG 2000) file (PS3.5 section A.4, a frame may span
    fragments): one frame with an empty Basic Offset Table owns them all, a filled table says where frames begin, and as many
    fragments as frames are one each -> [[(offset, length), ...] per frame]; ``ValueError`` otherwise."""
    found, table = meta.PixelDataFragments, meta.PixelDataOffsetTable
    if table:
        if len(table) != frames or not found:
            raise ValueError(f"{name}: a Basic Offset Table of {len(table)} entries for NumberOfFrames = {frames}")
        first = found[0][0]
        begins = [k for k, (o, _) in enumerate(found) if o - first in set(table)] + [len(found)]
        return [found[a:b] for a, b in zip(begins, begins[1:])]
    if frames == 1 and found:
        return [list(found)]
    if len(found) == frames:
        return [[f] for f in found]
    raise ValueError(f"{name}: {len(found)} {codec} fragments for NumberOfFrames = {frames} with an empty Basic Offset Table "
                     "(one fragment per frame, or a filled table)")


_JPEGLL_FLAGS = ((1, "the scan window or a parameter is unsound"), (2, "the data ends before Rows x Columns samples"),
                 (4, "corrupt data (a code outside the Huffman table or a wrong restart marker)"))


def _check_jpegll_status(status: torch.Tensor, owner, names) -> None:
    """``ValueError`` naming the file and the frame for the first flagged frame of ``decode_jpeg_lossless_frames`` (one
    transfer)."""
    flags = status.cpu().numpy()
    bad = np.flatnonzero(flags)
    if bad.size:
        k = int(bad[0])
        why = "; ".join(text for bit, text in _JPEGLL_FLAGS if flags[k] & bit)
        raise ValueError(f"{names[owner[k]]}, frame {k} of the stack: JPEG Lossless Pixel Data: {why}")


def decode_jpeg2000_frames(file_bytes, blocks, params, rows: int, cols: int, bits_allocated: int, bits_stored: int | None = None,
                           pixel_representation: int = 0, correct_unused_bits: bool = False, out: str = "container", rescale=None,
                           device=None, native: torch.Tensor | None = None, max_levels: int | None = None) -> torch.Tensor:
    """``pl_dicom_j2k_decode``, the JPEG 2000 counterpart of ``decode_jpeg_lossless_frames`` (T.800: one component, one tile,
    one layer, the reversible 5/3 transform, code-block style 0): N frames whose code-block segments lie anywhere inside
    ``file_bytes`` (uint8 array / tensor; device tensors are used in place).  ``blocks`` int64 [B, 10], one row per included
    code block of the stack: frame, segment offset, segment length, coding passes, magnitude bit planes, subband orientation
    (0 LL, 1 HL, 2 LH, 3 HH), then x0, y0, width, height of its rectangle in the frame's coefficient plane; ``params`` int32
    [N, 4]: decomposition levels, precision, signed (0 / 1), 0.  One wave decodes one block (tier 1), the inverse transform
    takes two launches per level, one launch shifts, clamps and stores.  -> device tensor [N, rows, cols] exactly as
    ``decode_frames`` gives it for the same samples stored native (``out``, ``rescale``, ``correct_unused_bits``: the decoded
    little-endian buffer goes through ``pl_dicom_decode``; the plain container dtype IS that buffer, returned as a view).
    ``_pl_status`` int32 [N]: bit 0 a descriptor of the frame is unsound (a segment window outside the buffer, a rectangle
    outside the plane, passes that are not 3 x planes - 2, parameters out of range); nothing of that block is read or stored
    and the other frames are not disturbed.  ``max_levels``: an upper bound of the levels in ``params`` (taken from a host
    array when absent, ``J2K_MAX_LEVELS`` for a device tensor).  ``native``: a uint8 device tensor
    [N, rows * cols * BitsAllocated / 8] to decode into."""
    dev = on_device(device)
    bits, rep = int(bits_allocated), int(pixel_representation)
    if bits not in (8, 16):
        raise ValueError("decode_jpeg2000_frames: BitsAllocated 8 or 16")
    if max_levels is None:
        max_levels = J2K_MAX_LEVELS if isinstance(params, torch.Tensor) else int(np.max(np.asarray(params).reshape(-1, 4)[:, 0], initial=0))
    if not 0 <= int(max_levels) <= J2K_MAX_LEVELS:
        raise ValueError(f"decode_jpeg2000_frames: {max_levels} decomposition levels (0 .. {J2K_MAX_LEVELS})")
    buf = bytes_tensor(file_bytes, dev)
    if buf.data_ptr() % 4:                                  # (the segments are read by the aligned dword)
        buf = buf.clone()
    blk = index_tensor(blocks, torch.int64, dev).reshape(-1, 10)
    par = index_tensor(params, torch.int32, dev).reshape(-1, 4)
    n, nblk = int(par.shape[0]), int(blk.shape[0])
    native = _native_buffer(native, n, rows * cols * (bits // 8), dev, "decode_jpeg2000_frames")
    lib = _lib.load()
    nwork = int(lib.pl_dicom_j2k_work_bytes(n, rows, cols))
    if nwork < 0:
        raise ValueError(f"decode_jpeg2000_frames: {n} frames of {rows} x {cols} (1 .. 65535 each)")
    work = torch.empty(max(nwork, 16), dtype=torch.uint8, device=dev)
    status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    check(lib.pl_dicom_j2k_decode(buf.data_ptr(), buf.numel(), blk.data_ptr() if nblk else None, nblk, par.data_ptr(), n,
                                  int(max_levels), rows, cols, bits // 8, native.data_ptr(), status.data_ptr(), work.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream), "pl_dicom_j2k_decode")
    return _from_native(native, status[:n], rows, cols, bits, bits_stored, rep, correct_unused_bits, out, rescale, dev)


_J2K = "JPEG 2000 Pixel Data: "
_J2K_TRUNCATED = "not a lossless JPEG 2000 stream: truncated code block"
# (one text each for what the host's packet parse and the device's, ``plan_jpeg2000_blocks``, both find)
_J2K_HEADER_SHORT = "the packet header of resolution {} runs out of bytes"
_J2K_PASSES = "({} coding passes for {} magnitude bit planes)"
_J2K_PLANES = "a code block of {} magnitude bit planes: at most {}"
_J2K_BEYOND = "(its segment reaches beyond the tile-part)"
_J2K_SECOND_SOT = "a second SOT: more than one tile-part"
_J2K_REFUSED = {0xFF53: "COC (coding style of a component)", 0xFF5D: "QCC (quantisation of a component)",
                0xFF5E: "RGN (region of interest)", 0xFF5F: "POC (progression order change)", 0xFF60: "PPM (packed packet headers)",
                0xFF61: "PPT (packed packet headers)", 0xFF50: "CAP (extended capabilities)", 0xFF59: "CPF (corresponding profile)"}
_J2K_SKIPPED = {0xFF64, 0xFF55, 0xFF57, 0xFF58, 0xFF63}    # COM, TLM, PLM, PLT, CRG
_J2K_MAX_PLANES = 30                                        # the device keeps a magnitude in 31 bits


class _J2kShort(Exception):
    """a packet header asks for a bit beyond the tile-part"""


class _J2kBits:
    """The bits of a packet header (T.800 B.10.1), most significant first: after a byte FF the next byte carries 7 bits."""

    __slots__ = ("data", "pos", "end", "buf", "ct")

    def __init__(self, data, pos: int, end: int):
        self.data, self.pos, self.end, self.buf, self.ct = data, pos, end, 0, 0

    def bit(self) -> int:
        if self.ct == 0:
            if self.pos >= self.end:
                raise _J2kShort
            self.ct = 7 if self.buf == 0xFF else 8
            self.buf = self.data[self.pos]
            self.pos += 1
        self.ct -= 1
        return (self.buf >> self.ct) & 1

    def bits(self, n: int) -> int:
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def align(self) -> int:
        """the header's end: the rest of its last byte is dropped, and a last byte FF is followed by one stuffed byte"""
        if self.buf == 0xFF:
            if self.pos >= self.end:
                raise _J2kShort
            self.pos += 1
        self.buf = self.ct = 0
        return self.pos


class _J2kTagTree:
    """A tag tree over ``w`` x ``h`` leaves (T.800 B.10.2): every node keeps its value (once known) and the lower bound the
    bits read so far have set."""

    def __init__(self, w: int, h: int):
        self.dims = [(w, h)]
        while (w, h) != (1, 1):
            w, h = (w + 1) // 2, (h + 1) // 2
            self.dims.append((w, h))
        self.value = [[1 << 30] * (a * b) for a, b in self.dims]
        self.low = [[0] * (a * b) for a, b in self.dims]

    def decode(self, bio: _J2kBits, x: int, y: int, threshold: int) -> bool:
        """-> whether the value of leaf (x, y) is below ``threshold``, reading only the bits that settles"""
        low = 0
        for l in range(len(self.dims) - 1, -1, -1):
            at = (y >> l) * self.dims[l][0] + (x >> l)
            value = self.value[l][at]
            low = max(low, self.low[l][at])
            while low < threshold and low < value:
                if bio.bit():
                    value = self.value[l][at] = low
                else:
                    low += 1
            self.low[l][at] = low
        return value < threshold


def _j2k_passes(bio: _J2kBits) -> int:
    """the number of coding passes of a code block (Table B.4): codewords for 1, 2, 3 .. 5, 6 .. 36, 37 .. 164"""
    if not bio.bit():
        return 1
    if not bio.bit():
        return 2
    v = bio.bits(2)
    if v < 3:
        return 3 + v
    v = bio.bits(5)
    return 6 + v if v < 31 else 37 + bio.bits(7)


def _j2k_main_header(mv, n: int, rows: int, cols: int, bits: int, name: str, total: int | None = None):
    """SOC, then the marker segments up to SOT (T.800 Annex A) -> (position of SOT, levels, precision, signed, guard bits,
    exponents per subband, (xcb, ycb), precinct exponents per resolution or None); what the main header shows of a stream this
    path does not decode is refused here, naming the marker or the field.  ``total`` (``load_zip``): ``mv`` holds the first
    ``n`` bytes of a stream of ``total`` bytes; ``_PrefixTooShort`` when they end inside the header where the stream does
    not."""
    def u16(at):
        return (mv[at] << 8) | mv[at + 1]

    def u32(at):
        return (u16(at) << 16) | u16(at + 2)

    if total is None:
        total = n

    def need(upto):                                         # bytes [0, upto) are looked at next
        if n < upto <= total:
            raise _PrefixTooShort

    need(12)
    if n >= 12 and bytes(mv[4:8]) == b"jP  ":
        raise NotImplementedError(f"{name}: {_J2K}a JP2 file (box wrapper) where DICOM encapsulates the raw codestream")
    need(2)
    if n < 2 or u16(0) != 0xFF4F:
        raise ValueError(f"{name}: {_J2K}the codestream does not start with SOC (FF4F)")
    pos, siz, cod, qcd = 2, None, None, None
    while True:
        need(pos + 4)
        if pos + 4 > n:
            raise ValueError(f"{name}: {_J2K}the main header ends without SOT")
        marker, ln = u16(pos), u16(pos + 2)
        if marker >> 8 != 0xFF:
            raise ValueError(f"{name}: {_J2K}a marker was expected at byte {pos} of the frame")
        if ln >= 2:
            need(pos + 2 + ln)
        if ln < 2 or pos + 2 + ln > n:
            raise ValueError(f"{name}: {_J2K}the segment of marker {marker:04X} lies outside the frame (cut off)")
        if marker == 0xFF90:
            break
        at, size = pos + 4, ln - 2
        if marker in _J2K_REFUSED:
            raise NotImplementedError(f"{name}: {_J2K}marker {marker:04X}, {_J2K_REFUSED[marker]}, is not decoded by this path")
        if marker == 0xFF51:
            if size < 36 or size != 36 + 3 * u16(at + 34):
                raise ValueError(f"{name}: {_J2K}malformed SIZ segment")
            csiz = u16(at + 34)
            if csiz != 1:
                raise NotImplementedError(f"{name}: {_J2K}SIZ with Csiz = {csiz} components: single-component frames only")
            xs, ys, xo, yo, xt, yt, xto, yto = (u32(at + 2 + 4 * k) for k in range(8))
            if xo or yo or xto or yto:
                raise NotImplementedError(f"{name}: {_J2K}SIZ with a non-zero image or tile origin (XOsiz, YOsiz, XTOsiz, YTOsiz)")
            if mv[at + 37] != 1 or mv[at + 38] != 1:
                raise NotImplementedError(f"{name}: {_J2K}SIZ with subsampling XRsiz x YRsiz = {mv[at + 37]} x {mv[at + 38]}")
            if xt < xs or yt < ys:
                raise NotImplementedError(f"{name}: {_J2K}SIZ with more than one tile (XTsiz x YTsiz = {xt} x {yt})")
            if (ys, xs) != (rows, cols):
                raise ValueError(f"{name}: {_J2K}SIZ states Ysiz x Xsiz = {ys} x {xs} where Rows x Columns = {rows} x {cols}")
            prec, signed = (mv[at + 36] & 127) + 1, mv[at + 36] >> 7
            if not 2 <= prec <= bits:
                raise ValueError(f"{name}: {_J2K}SIZ precision {prec} (2 .. BitsAllocated = {bits})")
            siz = (prec, signed)
        elif marker == 0xFF52:
            if size < 10:
                raise ValueError(f"{name}: {_J2K}malformed COD segment")
            scod, prog, layers, mct, levels, xcb, ycb, style, wavelet = (mv[at], mv[at + 1], u16(at + 2), mv[at + 4], mv[at + 5],
                                                                         mv[at + 6] + 2, mv[at + 7] + 2, mv[at + 8], mv[at + 9])
            if levels > 32 or size != 10 + (levels + 1 if scod & 1 else 0) or prog > 4 or scod > 7 or xcb > 10 or ycb > 10 or xcb + ycb > 12:
                raise ValueError(f"{name}: {_J2K}malformed COD segment")
            if scod & 6:
                raise NotImplementedError(f"{name}: {_J2K}COD with SOP or EPH markers in the packets (Scod = {scod:#04x})")
            if layers != 1:
                raise NotImplementedError(f"{name}: {_J2K}COD with {layers} quality layers: one layer only")
            if mct:
                raise NotImplementedError(f"{name}: {_J2K}COD with a multiple-component transform")
            if wavelet != 1:
                raise NotImplementedError(f"{name}: {_J2K}COD selects the irreversible 9/7 transform: only the reversible 5/3 "
                                          "transform (lossless) is decoded by this path")
            if style:
                raise NotImplementedError(f"{name}: {_J2K}COD with code-block style {style:#04x}: style 0 only")
            if levels > J2K_MAX_LEVELS:
                raise NotImplementedError(f"{name}: {_J2K}COD with {levels} decomposition levels: at most J2K_MAX_LEVELS = "
                                          f"{J2K_MAX_LEVELS}")
            if xcb > 6 or ycb > 6:
                raise NotImplementedError(f"{name}: {_J2K}COD with code blocks of {1 << xcb} x {1 << ycb}: at most 64 on a side")
            cod = (levels, xcb, ycb, [(mv[at + 10 + r] & 15, mv[at + 10 + r] >> 4) for r in range(levels + 1)] if scod & 1 else None)
        elif marker == 0xFF5C:
            if size < 2:
                raise ValueError(f"{name}: {_J2K}malformed QCD segment")
            if mv[at] & 31:
                raise NotImplementedError(f"{name}: {_J2K}QCD with quantisation style {mv[at] & 31}: style 0 (none, reversible) only")
            qcd = (mv[at] >> 5, [mv[at + 1 + k] >> 3 for k in range(size - 1)])
        elif marker not in _J2K_SKIPPED:
            raise NotImplementedError(f"{name}: {_J2K}marker {marker:04X} in the main header is not decoded by this path")
        pos += 2 + ln
    if siz is None or cod is None or qcd is None:
        raise ValueError(f"{name}: {_J2K}SOT before " + ("SIZ" if siz is None else "COD" if cod is None else "QCD"))
    if len(qcd[1]) < 3 * cod[0] + 1:
        raise ValueError(f"{name}: {_J2K}QCD holds {len(qcd[1])} exponents where {cod[0]} levels need {3 * cod[0] + 1}")
    return pos, cod[0], siz[0], siz[1], qcd[0], qcd[1], (cod[1], cod[2]), cod[3]


def _j2k_tile_header(mv, n: int, sot: int, name: str, total: int | None = None):
    """SOT at ``sot`` and the tile-part header through SOD -> (the first packet's position, the tile-part's end, Psot).
    ``total``: ``_j2k_main_header``'s.  With a prefix the marker behind the tile-part (a second SOT is refused) is the
    caller's to look at, and so are the last three bytes that place the end of a tile-part with Psot = 0: the end returned is
    then ``total``."""
    def u16(at):
        return (mv[at] << 8) | mv[at + 1]

    whole = total is None or n >= total
    if total is None:
        total = n

    def need(upto):
        if n < upto <= total:
            raise _PrefixTooShort

    if u16(sot + 2) != 10:
        raise ValueError(f"{name}: {_J2K}malformed SOT segment")
    isot, psot, tpsot, tnsot = u16(sot + 4), (u16(sot + 6) << 16) | u16(sot + 8), mv[sot + 10], mv[sot + 11]
    if isot:
        raise NotImplementedError(f"{name}: {_J2K}SOT of tile {isot}: one tile only")
    if tpsot or tnsot > 1:
        raise NotImplementedError(f"{name}: {_J2K}SOT with TPsot = {tpsot}, TNsot = {tnsot}: more than one tile-part")
    if psot:
        end = sot + psot
        if psot < 14 or end > total:
            raise ValueError(f"{name}: {_J2K}SOT states a tile-part of {psot} bytes where {total - sot} are left (cut off)")
        if end + 2 <= n and u16(end) == 0xFF90:
            raise NotImplementedError(f"{name}: {_J2K}{_J2K_SECOND_SOT}")
    elif whole:                                             # up to EOC (an item's pad byte may follow it)
        end = n - 2 if n >= 2 and u16(n - 2) == 0xFFD9 else n - 3 if n >= 3 and u16(n - 3) == 0xFFD9 else n
    else:
        end = total
    pos = sot + 12
    while True:                                             # the tile-part header
        if pos + 2 > end:
            raise ValueError(f"{name}: {_J2K}the tile-part header ends without SOD")
        need(pos + 2)
        marker = u16(pos)
        if marker == 0xFF93:
            pos += 2
            break
        if marker in _J2K_REFUSED or marker in (0xFF52, 0xFF5C):
            what = _J2K_REFUSED.get(marker, "COD / QCD in a tile-part header")
            raise NotImplementedError(f"{name}: {_J2K}marker {marker:04X}, {what}, is not decoded by this path")
        if marker not in _J2K_SKIPPED:
            raise ValueError(f"{name}: {_J2K}marker {marker:04X} where the tile-part header or SOD was expected")
        if pos + 4 <= end:
            need(pos + 4)
        if pos + 4 > end or u16(pos + 2) < 2 or pos + 2 + u16(pos + 2) > end:
            raise ValueError(f"{name}: {_J2K}the segment of marker {marker:04X} lies outside the tile-part (cut off)")
        pos += 2 + u16(pos + 2)
    return pos, end, psot


def _j2k_geometry(rows: int, cols: int, levels: int, xcb: int, ycb: int, precincts, exps, name: str):
    """The geometry the main header fixes, resolution by resolution (a generator: what it refuses of resolution r is raised
    when r is reached) -> (r, code-block width, height, [(orientation, x0, y0, width, height, exponent)] per subband, the low
    band first along either axis; empty bands are listed).  The host's packet parse and the plan of the device's walk it."""
    res = [((cols + (1 << d) - 1) >> d, (rows + (1 << d) - 1) >> d) for d in range(levels, -1, -1)]
    for r, (rw, rh) in enumerate(res):
        ppx, ppy = precincts[r] if precincts else (15, 15)
        if ((rw + (1 << ppx) - 1) >> ppx) > 1 or ((rh + (1 << ppy) - 1) >> ppy) > 1:
            raise NotImplementedError(f"{name}: {_J2K}COD states precincts of {1 << ppx} x {1 << ppy} at resolution {r} of "
                                      f"{rw} x {rh}: more than one precinct in a resolution")
        if r and (ppx == 0 or ppy == 0):
            raise ValueError(f"{name}: {_J2K}COD states a precinct exponent 0 above resolution 0")
        cbw, cbh = 1 << min(xcb, ppx - (r > 0)), 1 << min(ycb, ppy - (r > 0))
        if r == 0:
            bands = [(0, 0, 0, rw, rh, exps[0])]
        else:
            lw, lh = res[r - 1]
            bands = [(1, lw, 0, rw - lw, lh, exps[3 * r - 2]), (2, 0, lh, lw, rh - lh, exps[3 * r - 1]), (3, lw, lh, rw - lw, rh - lh, exps[3 * r])]
        yield r, cbw, cbh, bands


def _j2k_tree_nodes(w: int, h: int) -> int:
    """the nodes of a tag tree over ``w`` x ``h`` leaves"""
    n = w * h
    while (w, h) != (1, 1):
        w, h = (w + 1) // 2, (h + 1) // 2
        n += w * h
    return n


def _j2k_block_counts(geometry) -> tuple[int, int]:
    """-> (the code blocks of a frame, included or not: the rows ``plan_jpeg2000_blocks`` fills; the nodes of its largest tag
    tree)"""
    blocks, nodes = 0, 1
    for _, cbw, cbh, bands in geometry:
        for _, _, _, bw, bh, _ in bands:
            if bw and bh:
                ncx, ncy = (bw + cbw - 1) // cbw, (bh + cbh - 1) // cbh
                blocks += ncx * ncy
                nodes = max(nodes, _j2k_tree_nodes(ncx, ncy))
    return blocks, nodes


def _j2k_codestream(data, rows: int, cols: int, bits: int, name: str):
    """One frame's JPEG 2000 codestream (``data``: its bytes, a uint8 array) -> (levels, precision, signed, [(segment offset
    inside ``data``, length, passes, magnitude bit planes, orientation, x0, y0, w, h)] per included code block).  The main
    header (``_j2k_main_header``), SOT and SOD (``_j2k_tile_header``), then tier 2 (T.800 Annex B): one packet per resolution
    of the one tile -- the zero-length bit, per subband the inclusion and zero-bit-plane tag trees, the passes, ``Lblock`` and
    the segment length of every included block, the header byte-aligned -- and the packet's body, the segments in the same
    order.  ``NotImplementedError`` for what this path does not decode, ``ValueError`` for a malformed or truncated stream."""
    mv = memoryview(np.ascontiguousarray(data, dtype=np.uint8))
    n = len(mv)
    sot, levels, prec, signed, guard, exps, (xcb, ycb), precincts = _j2k_main_header(mv, n, rows, cols, bits, name)
    pos, end, _ = _j2k_tile_header(mv, n, sot, name)
    blocks = []
    for r, cbw, cbh, bands in _j2k_geometry(rows, cols, levels, xcb, ycb, precincts, exps, name):
        bio, found = _J2kBits(mv, pos, end), []
        try:
            if bio.bit():
                for orient, bx, by, bw, bh, exponent in bands:
                    if bw == 0 or bh == 0:
                        continue
                    ncx, ncy = (bw + cbw - 1) // cbw, (bh + cbh - 1) // cbh
                    inclusion, zero_planes = _J2kTagTree(ncx, ncy), _J2kTagTree(ncx, ncy)
                    for cy in range(ncy):
                        for cx in range(ncx):
                            if not inclusion.decode(bio, cx, cy, 1):
                                continue
                            z = 1
                            while not zero_planes.decode(bio, cx, cy, z):
                                z += 1
                            passes, lblock = _j2k_passes(bio), 3
                            while bio.bit():
                                lblock += 1
                            length = bio.bits(lblock + passes.bit_length() - 1)
                            found.append((length, passes, guard + exponent - 1 - (z - 1), orient, bx + cx * cbw, by + cy * cbh,
                                          min(cbw, bw - cx * cbw), min(cbh, bh - cy * cbh)))
            pos = bio.align()
        except _J2kShort:
            raise ValueError(f"{name}: {_J2K}{_J2K_HEADER_SHORT.format(r)}") from None
        for length, passes, planes, *rest in found:
            if passes != 3 * planes - 2 or planes < 1:
                raise ValueError(f"{name}: {_J2K_TRUNCATED} {_J2K_PASSES.format(passes, planes)}")
            if planes > _J2K_MAX_PLANES:
                raise NotImplementedError(f"{name}: {_J2K}{_J2K_PLANES.format(planes, _J2K_MAX_PLANES)}")
            if length > end - pos:
                raise ValueError(f"{name}: {_J2K_TRUNCATED} {_J2K_BEYOND}")
            blocks.append((pos, length, passes, planes, *rest))
            pos += length
    return levels, prec, signed, blocks


def _j2k_refusals(ib: int) -> None:
    """what a JPEG 2000 stack is refused for before any of its streams is read"""
    if ib not in (1, 2):
        raise NotImplementedError(f"JPEG 2000 Pixel Data with BitsAllocated {ib * 8}: 8 and 16 are decoded on the device")


def _j2k_stage(metas, blobs, lay, names):
    """The host side of a JPEG 2000 stack, as ``_jpegll_stage``: every frame's fragment payloads end to end at a 4-byte
    boundary of one host buffer, its headers and packet headers parsed where they lie (``_j2k_codestream``) -> (the staging
    buffer, (blocks, params) as ``decode_jpeg2000_frames`` takes them, the file of every frame); every refusal of a file
    happens here, before anything is copied to the device."""
    rows, cols, ib = lay[0].rows, lay[0].cols, lay[0].sample_bytes
    _j2k_refusals(ib)
    pieces, table, params, owner, pos = [], [], [], [], 0
    for k, (m, b, l) in enumerate(zip(metas, blobs, lay)):
        for frags in _jpegll_frames(m, l.frames, names[k], "JPEG 2000"):
            data = b[frags[0][0]:frags[0][0] + frags[0][1]] if len(frags) == 1 else np.concatenate([b[o:o + n] for o, n in frags])
            levels, prec, signed, blocks = _j2k_codestream(data, rows, cols, ib * 8, names[k])
            table += [(len(owner), pos + at, *rest) for at, *rest in blocks]
            params.append((levels, prec, signed, 0))
            owner.append(k)
            pieces.append((pos, data))
            pos += (len(data) + 3) & ~3
    host = np.zeros(pos, dtype=np.uint8)
    for at, data in pieces:
        host[at:at + len(data)] = data
    return host, (np.asarray(table, dtype=np.int64).reshape(-1, 10), np.asarray(params, dtype=np.int32).reshape(-1, 4)), owner


def _check_j2k_status(status: torch.Tensor, owner, names) -> None:
    """``ValueError`` naming the file and the frame for the first flagged frame of ``decode_jpeg2000_frames`` (one
    transfer)."""
    bad = np.flatnonzero(status.cpu().numpy())
    if bad.size:
        k = int(bad[0])
        raise ValueError(f"{names[owner[k]]}, frame {k} of the stack: {_J2K}a code-block descriptor or a parameter is unsound")


def _check_native_status(status: torch.Tensor, owner=None, names=None) -> None:
    if bool(status.any()):
        raise ValueError("The length of the pixel data in the dataset doesn't match the expected length; the dataset may be "
                         "corrupted")


def _check_status(frames: torch.Tensor) -> torch.Tensor:
    st = getattr(frames, "_pl_status", None)
    if st is not None:
        _check_native_status(st)
    return frames


_MIXED_JPEGLL = "load_frames: JPEG Lossless files are mixed with native or RLE Lossless files; load the kinds separately"
_MIXED_RLE = "load_frames: native and RLE Lossless files are mixed; load the two kinds separately"
_MIXED_J2K = "load_frames: JPEG 2000 files are mixed with native, RLE Lossless or JPEG Lossless files; load the kinds separately"
_DECODERS = {"native": (decode_frames, _check_native_status), "rle": (decode_rle_frames, _check_rle_status),
             "jpegll": (decode_jpeg_lossless_frames, _check_jpegll_status), "j2k": (decode_jpeg2000_frames, _check_j2k_status)}


def _frame_plan(metas, who: str, noun: str):
    """What ``load_frames`` (``noun``: files) and ``load_zip`` (members) settle as soon as the headers are parsed, before a
    fragment is looked at: one pixel format and frame size, one kind -> (kind "native" | "rle" | "jpegll" | "j2k", the layouts, and
    for native data the file of every frame and the frame's offset inside that file)."""
    lay = [_layout(m) for m in metas]
    first = lay[0]
    for l in lay[1:]:
        if l.format != first.format:
            raise ValueError(f"{who}: the {noun} differ in pixel format or frame size (the reference's stacks refuse that too)")
    kinds = {"native" if m.PixelData[1] >= 0 else "rle" if m.TransferSyntaxUID == RLE_LOSSLESS else
             "j2k" if m.TransferSyntaxUID in JPEG_2000 else "jpegll" for m in metas}
    if len(kinds) > 1:
        raise ValueError(_MIXED_J2K if "j2k" in kinds else _MIXED_JPEGLL if "jpegll" in kinds else _MIXED_RLE)
    owner, inside = [], []
    if kinds == {"native"}:
        frame_bytes = first.rows * first.cols * first.sample_bytes
        for k, l in enumerate(lay):
            off, ln = l.value
            if ln < l.frames * frame_bytes:
                raise ValueError(f"The length of the pixel data in the dataset ({ln} bytes) "
                                 f"doesn't match the expected length ({l.frames * frame_bytes} bytes). "
                                 "The dataset may be corrupted or there may be an issue with the pixel data handler.")
            owner += [k] * l.frames
            inside += [off + f * frame_bytes for f in range(l.frames)]
    return kinds.pop(), lay, owner, np.asarray(inside, dtype=np.int64)


def _rle_windows(metas, lay, names, base, head):
    """The segments of every RLE frame (one fragment per frame, PS3.5 section A.4.2) -> (seg_off, seg_len as
    ``decode_rle_frames`` takes them, the file of every frame).  ``base[k]``: where file k begins in the buffer that is
    decoded; ``head(k, j)``: the first 64 bytes of its fragment j."""
    windows, owner = [], []
    for k, (meta, l) in enumerate(zip(metas, lay)):
        found = meta.PixelDataFragments
        if len(found) != l.frames:
            raise ValueError(f"{names[k]}: {len(found)} RLE fragments for NumberOfFrames = {l.frames} (one fragment per frame)")
        for j, frag in enumerate(found):
            windows.append([(int(base[k]) + o, n) for o, n in _rle_segments(head(k, j), frag, l.sample_bytes, names[k])])
            owner.append(k)
    windows = np.asarray(windows, dtype=np.int64).reshape(-1, lay[0].sample_bytes, 2)
    return np.ascontiguousarray(windows[:, :, 0]), np.ascontiguousarray(windows[:, :, 1]), owner


def _jpegll_tables(scans: list):
    """[(file, where the frame's stream begins in the buffer that is decoded, ``_jpegll_header``'s answer for it)] per frame
    -> ((scan_off, scan_len, params, huff) as ``decode_jpeg_lossless_frames`` takes them, the file of every frame)"""
    tables = (np.asarray([at + h[0] for _, at, h in scans], dtype=np.int64),
              np.asarray([h[1] for _, _, h in scans], dtype=np.int64),
              np.asarray([h[2] for _, _, h in scans], dtype=np.int32).reshape(-1, 4),
              np.stack([np.frombuffer(h[3], dtype=np.uint8) for _, _, h in scans]))
    return tables, [k for k, _, _ in scans]


def _decode_keywords(l: _Layout, meta: Metadata, correct_unused_bits: bool, device) -> dict:
    """the keywords the three decodes share, for a stack of layout ``l`` whose first file's metadata are ``meta``"""
    bits = l.sample_bytes * 8
    return dict(rows=l.rows, cols=l.cols, bits_allocated=bits, bits_stored=int(meta.get("BitsStored") or bits),
                pixel_representation=int(meta.PixelRepresentation), correct_unused_bits=correct_unused_bits, device=device)


def _decode_step(kind: str, buffer, where: tuple, l: _Layout, meta: Metadata, correct_unused_bits: bool, device):
    """-> decode(out=..., rescale=...) = (frames, status) for ``_finish_frames``: the decode of ``kind`` over ``buffer``,
    ``where`` being the arrays that place the frames in it (frame offsets | seg_off, seg_len | scan_off, scan_len, params,
    huff | blocks, params)."""
    common = _decode_keywords(l, meta, correct_unused_bits, device)
    if kind == "native":
        common["big_endian"] = l.big_endian
    elif kind == "rle":
        common["max_segment_bytes"] = int(where[1].max(initial=0))

    def decode(**kw):
        x = _DECODERS[kind][0](buffer, *where, **common, **kw)
        return x, x._pl_status

    return decode


def load_frames(sources, dtype=None, raw_pixels: bool = False, invert_pixels: bool | None = None,
                correct_unused_bits: bool = False, device=None, check: bool = True, jpeg_lossless: bool = False,
                jpeg2000: bool = False):
    """The batched loader: Part-10 files (paths, bytes or file objects; every file may hold several frames) of ONE pixel
    format, frame size and kind (all native or all RLE Lossless; with the keywords below all JPEG Lossless or all JPEG 2000) ->
    (device tensor [N, H, W], list of per-file metadata).  Per
    file exactly what ``DicomImage.__init__`` does (image.py:1431-1444): ``pixel_array`` [``.astype(dtype)``] then
    ``_rescale_dicom_values``;
    files with both rescale tags take the fused float64 form of the kernel when every file carries the SAME slope and
    intercept (a series), otherwise the frames are decoded once and rescaled file by file.

    ``jpeg_lossless=True`` accepts a third kind: files of the JPEG Lossless syntaxes (``JPEG_LOSSLESS``: T.81 process 14,
    SamplesPerPixel 1, BitsAllocated 8 or 16), decoded by ``decode_jpeg_lossless_frames`` with a wave per frame.  Their files
    may differ in predictor, point transform, restart interval and Huffman table; a frame may span fragments (its payloads
    are laid end to end on the host).  ``check=True`` reads the decode's status once and raises ``ValueError`` naming the
    file and the frame.

    ``jpeg2000=True`` accepts a fourth kind: files of the JPEG 2000 syntaxes (``JPEG_2000``) whose streams are lossless --
    SamplesPerPixel 1, BitsAllocated 8 or 16, a raw codestream of one component, one tile and tile-part, one quality layer,
    the reversible 5/3 transform with up to ``J2K_MAX_LEVELS`` levels, code blocks of at most 64 x 64 in style 0, one
    precinct per resolution.  The host reads the headers and the packet headers (``_j2k_codestream``), the device decodes
    the code blocks with a wave each and runs the inverse transform (``decode_jpeg2000_frames``).  Everything else of
    JPEG 2000 is refused naming the file and the marker or field (``NotImplementedError``), a malformed or truncated stream
    is a ``ValueError``, both before anything is copied to the device.  Both keywords may be given; the kinds do not mix
    in one call."""
    sources = list(sources)
    metas, blobs = [], []
    for s in sources:
        m, b = read_part10(s, jpeg_lossless=jpeg_lossless, jpeg2000=jpeg2000)
        metas.append(m)
        blobs.append(b)
    names = [f"file {k}" + (f" ({s})" if isinstance(s, (str, Path)) else "") for k, s in enumerate(sources)]
    kind, lay, owner, inside = _frame_plan(metas, "load_frames", "files")
    if kind == "jpegll":
        host, where, owner = _jpegll_stage(metas, blobs, lay, names)
    elif kind == "j2k":
        host, where, owner = _j2k_stage(metas, blobs, lay, names)
    else:                                                   # one host buffer, every file at a 4-byte boundary
        starts = np.cumsum([0] + [(len(b) + 3) & ~3 for b in blobs])
        if kind == "rle":
            *where, owner = _rle_windows(metas, lay, names, starts,
                                         lambda k, j: blobs[k][metas[k].PixelDataFragments[j][0]:][:64])
        else:
            where = (starts[owner] + inside,)
        host = np.zeros(starts[-1], dtype=np.uint8)
        for st, b in zip(starts, blobs):
            host[st:st + len(b)] = b
    decode = _decode_step(kind, host, where, lay[0], metas[0], correct_unused_bits, device)
    verify = partial(_DECODERS[kind][1], owner=owner, names=names)
    return _finish_frames(decode, verify, metas, owner, lay[0].rows, lay[0].cols, dtype, raw_pixels, invert_pixels, check), metas


def _jpegll_stage(metas, blobs, lay, names):
    """The host side of a JPEG Lossless stack: every frame's fragment payloads end to end at a 4-byte boundary of one host
    buffer (the kernel sees one window per frame), its markers parsed where they lie -> (the staging buffer, (scan_off,
    scan_len, params, huff) as ``decode_jpeg_lossless_frames`` takes them, the file of every frame); every refusal of a file
    happens here."""
    rows, cols, ib = lay[0].rows, lay[0].cols, lay[0].sample_bytes
    _jpegll_refusals(ib, cols)
    pieces, scans, pos = [], [], 0
    for k, (m, b, l) in enumerate(zip(metas, blobs, lay)):
        for frags in _jpegll_frames(m, l.frames, names[k]):
            data = b[frags[0][0]:frags[0][0] + frags[0][1]] if len(frags) == 1 else np.concatenate([b[o:o + n] for o, n in frags])
            scans.append((k, pos, _jpegll_header(data, rows, cols, ib * 8, names[k])))
            pieces.append((pos, data))
            pos += (len(data) + 3) & ~3
    host = np.zeros(pos, dtype=np.uint8)
    for at, data in pieces:
        host[at:at + len(data)] = data
    return (host,) + _jpegll_tables(scans)


def _finish_frames(decode, verify, metas, owner, rows: int, cols: int, dtype, raw_pixels: bool, invert_pixels, check: bool):
    """The tail ``load_frames`` and ``load_zip`` share: ``decode(out=..., rescale=...)`` is the device decode of every frame
    -> (frames, per-frame status), ``verify(status)`` raises for a flagged one; the dtype rules, the rescale (fused when every
    file carries the same tags, file by file otherwise) and the inversion of ``DicomImage.__init__``.  The frames returned
    carry the status as ``_pl_status``."""
    from .image import rescale_dicom_values

    has_rescale = [("RescaleSlope" in m and "RescaleIntercept" in m) for m in metas]
    same = all(has_rescale) and len({(m.RescaleSlope, m.RescaleIntercept) for m in metas}) == 1
    inverts = [bool(invert_pixels or (invert_pixels is None and m.get("PixelIntensityRelationshipSign") == -1)) for m in metas]
    np_dt = None if dtype is None else np.dtype(dtype)
    if raw_pixels or not any(has_rescale):
        if np_dt in _NP_TO_TORCH:
            x, status = decode(out={4: "float32", 8: "float64"}[np_dt.itemsize])
        else:
            x, status = decode(out="container")
            if np_dt is not None:
                x = _astype(x, np_dt)
        if check:
            verify(status)
    elif same and np_dt in (None, np.dtype(np.float64)):
        x, status = decode(out="float64", rescale=(metas[0].RescaleSlope, metas[0].RescaleIntercept))
        if check:
            verify(status)
    else:
        if not all(has_rescale):
            raise ValueError("load_frames: some files carry rescale tags and some do not; load them separately")
        base, status = decode(out="container")
        if check:
            verify(status)
        if np_dt is not None:
            base = _astype(base, np_dt)
        own = np.asarray(owner)
        parts = []
        for k, m in enumerate(metas):
            sel = base[torch.from_numpy(np.flatnonzero(own == k)).to(base.device)].contiguous()
            parts.append(rescale_dicom_values(sel, m.RescaleSlope, m.RescaleIntercept, invert_pixels=False))
        x = torch.cat(parts)
    if not raw_pixels and any(inverts):
        from . import ops

        if x.dtype in (torch.int8, torch.uint32):
            raise NotImplementedError(f"inverting {x.dtype} pixel data is not available on the device (no EPID / CT panel stores "
                                      "it); pass dtype= to widen it first")

        own = np.asarray(owner)
        if all(inverts) and len(own) == len(metas):
            x = ops.invert(x)                                 # max - a + min per file (image.py:383-388), one frame per file
        else:                                                 # a multi-frame file inverts about the extrema of ALL its frames
            x = x.clone()
            for k in np.flatnonzero(inverts):
                idx = np.flatnonzero(own == k)
                a, b = int(idx[0]), int(idx[-1]) + 1
                x[a:b] = ops.invert(x[a:b].reshape(1, (b - a) * rows, cols)).reshape(b - a, rows, cols)
    x._pl_status = status
    return x


def _member_header(raw, member, what: str, encapsulated: bool = False, jpeg2000: bool = False):
    """The Part-10 header of one archive member without inflating it whole -> its metadata, or None for a member without
    ``DICM`` at byte 128.  ``raw``: the member's bytes as they lie in the archive (a uint8 array view).  A stored member is
    walked where it lies; of a deflated one the first 64 KiB are inflated on the host, and twice as many again until the walk
    reaches the (7FE0,0010) element header or the member ends.  ``encapsulated``, ``jpeg2000``: ``_walk_part10``'s."""
    import zlib

    def walk(view, size):                                   # (the keywords only when set: the default call stays (view, size))
        kw = dict(encapsulated=True, **(dict(jpeg2000=True) if jpeg2000 else {})) if encapsulated else {}
        return _walk_part10(view, size, **kw)

    if member.size < 132:
        return None
    if member.method == 0:
        view = memoryview(raw).cast("B")
        return walk(view, member.size) if bytes(view[128:132]) == b"DICM" else None
    inflater, have, want, data = zlib.decompressobj(-15), bytearray(), 65536, memoryview(raw).cast("B")
    while True:
        try:
            have += inflater.decompress(data, want - len(have))
        except zlib.error as e:
            raise zipfile.BadZipFile(f"{what}: corrupt Deflate data in its header ({e})") from None
        data = inflater.unconsumed_tail
        if len(have) >= 132 and bytes(have[128:132]) != b"DICM":
            return None
        ended = inflater.eof or (len(have) < want and not data)
        try:
            return walk(memoryview(have), len(have) if ended else max(member.size, len(have) + 1))
        except _PrefixTooShort:
            if ended:
                raise zipfile.BadZipFile(f"{what}: the Deflate stream ends inside the data set's header") from None
            want *= 2


def load_zip(source, members=None, verify: bool = True, dtype=None, raw_pixels: bool = False, invert_pixels: bool | None = None,
             correct_unused_bits: bool = False, device=None, check: bool = True, encapsulated: bool = False,
             jpeg2000: bool = False):
    """``load_frames([zf.read(n) for n in names], ...)`` for a ZIP archive of native Part-10 files (what
    ``DicomImageStack.from_zip`` / ``CatPhan504.from_zip`` are handed) without a member ever being inflated whole on the host
    -> (device tensor [N, H, W], list of per-member metadata, names).  The archive goes to the device compressed; ONE
    ``pl_zip_extract`` (``zipstack.extract``) inflates every member with a wave of its own and, with ``verify``, checks its
    CRC-32 as ``zipfile`` does; ``pl_dicom_decode`` then reads the frames where the members lie.  The host inflates only each
    member's first kilobytes, for the Part-10 header walk.  ``members``: names in the order wanted; None takes every member
    with ``DICM`` at byte 128, in central-directory order (``names`` lists them).  By default RLE Lossless members raise
    ``NotImplementedError`` naming the member (``encapsulated=True``, below, decodes them); the other refusals, the
    dtype rules, rescale and inversion are ``load_frames``'s own.  ``check=True`` reads the archive's status once
    (``zipfile.BadZipFile``: ``Bad CRC-32 for file 'NAME'``) and the decode's.

    ``encapsulated=True`` extends the same contract to the members a CT series usually leaves a PACS with:
    ``load_frames([zf.read(n) for n in names], jpeg_lossless=True, ...)`` for archives whose members are all RLE Lossless or
    all JPEG Lossless (``JPEG_LOSSLESS``) -- the same tensor, metadata (``PixelData`` = (offset, -1), ``PixelDataFragments``,
    ``PixelDataOffsetTable``), kind-mixing rules and refusals, the member named ``ARCHIVE: member 'NAME'``.  The host's header
    walk stops at the Pixel Data element; after the extraction ONE ``pl_dicom_encap_index`` (``index_encapsulated``) walks
    every member's items on the device and ONE transfer brings back, per fragment, its place and its first
    ``ENCAP_HEAD_BYTES`` bytes, from which the host reads RLE segment headers and JPEG markers.  The fragments are decoded
    where the members lie; only a JPEG frame that spans fragments is first laid end to end (``copy_ranges``), and only a frame
    whose markers run past the head has its leading bytes fetched (4 KiB, doubling).  No Pixel Data comes back to the host.
    Without the keyword such members raise ``NotImplementedError`` as they always did.

    ``jpeg2000=True`` (with ``encapsulated=True``; ``ValueError`` without it) takes archives whose members are all JPEG 2000
    (``JPEG_2000``): ``load_frames([zf.read(n) for n in names], jpeg2000=True, ...)``, the same contract again.  The host reads
    each frame's main header, SOT and tile-part header from the heads (a main header that runs past them has the stream's
    leading bytes fetched); the packet headers, which lie all through the stream, are read by the device
    (``plan_jpeg2000_blocks``) where the member was inflated, and what only that walk can find -- a packet header out of
    bytes, a truncated code block, more than 30 bit planes, a segment beyond the tile-part -- is raised from ONE transfer of
    its result before the code blocks are decoded, whatever ``check`` says, as ``load_frames`` raises it unconditionally.
    Two bytes per frame, the marker behind the tile-part, come back with one more transfer (a second tile-part is refused).
    The ORDER of refusals differs from ``load_frames`` where several faults meet: what the host reads of ANY member's headers
    and geometry is raised before what the device finds in any member (its result is read once, for all of them), so an
    archive whose member 0 has a truncated block and whose member 1 has a COC marker names member 1 where ``load_frames``
    names file 0; each message is the one ``load_frames`` has for that member.
    Without the keyword JPEG 2000 members are refused as before.

    The device form is for archives of MANY members of moderate size -- a CT volume: 80 - 300 slices of 0.5 MB, every Deflate
    stream a wave of its own.  One Deflate stream is one serial chain (about 150 ns per output byte), so an archive of a few
    large deflated members (a Winston-Lutz session of 1280 x 1280 frames) is read faster by ``zipfile`` on the host followed by
    ``load_frames``; stored members cost a copy either way."""
    from . import zipstack

    if jpeg2000 and not encapsulated:
        raise ValueError("load_zip: jpeg2000=True extends encapsulated=True; pass both")
    archive, what, host, dbuf = zipstack.stage(source, device)
    hv = host.numpy()
    taken, metas, labels = [], [], []
    for m in zipstack._select(archive, members, what):
        name = f"{what}: member {m.name!r}"
        try:
            meta = _member_header(hv[m.data_offset:m.data_offset + m.compressed_size], m, name, encapsulated, jpeg2000)
        except NotImplementedError as e:
            raise NotImplementedError(f"{name}: {e}") from None
        if meta is None:
            if members is None:
                continue
            raise ValueError(f"{name}: not a DICOM Part-10 file (no DICM at byte 128)")
        taken.append(m)
        metas.append(meta)
        labels.append(name)
    if not taken:
        raise ValueError(f"{what}: no DICOM members")
    kind, lay, owner, inside = _frame_plan(metas, "load_zip", "members")
    if kind == "jpegll":
        _jpegll_refusals(lay[0].sample_bytes, lay[0].cols)
    elif kind == "j2k":
        _j2k_refusals(lay[0].sample_bytes)
    stack = zipstack.run(taken, what, host, dbuf, verify=verify, check=check)
    copied = None
    if kind == "jpegll":
        decode, owner, copied = _zip_jpegll_decode(stack, metas, lay, labels, correct_unused_bits)
    elif kind == "j2k":
        decode, owner, copied = _zip_j2k_decode(stack, metas, lay, labels, correct_unused_bits, what)
    else:
        if kind == "rle":
            heads = _index_members(stack, metas, lay, labels, False)
            *where, owner = _rle_windows(metas, lay, labels, stack.offsets, lambda k, j: heads[k][j])
        else:
            where = (stack.offsets[owner] + inside,)
        decode = _decode_step(kind, stack.buffer, where, lay[0], metas[0], correct_unused_bits, stack.buffer.device)

    def verify_frames(status):
        if copied is not None and bool(copied.any()):
            raise ValueError(f"{what}: a fragment of a frame that spans fragments lies outside the extracted members")
        _DECODERS[kind][1](status, owner, labels)

    x = _finish_frames(decode, verify_frames, metas, owner, lay[0].rows, lay[0].cols, dtype, raw_pixels, invert_pixels, check)
    return x, metas, [m.name for m in taken]


ENCAP_HEAD_BYTES = 256                                       # PL_DICOM_ENCAP_HEAD: the bytes of every fragment the index brings back
ENCAP_DESCRIPTOR, ENCAP_MALFORMED, ENCAP_TABLE, ENCAP_CAPACITY, ENCAP_NO_DELIMITER, ENCAP_TABLE_LENGTH = 1, 2, 4, 8, 16, 32


@dataclass
class EncapIndex:
    """What ``index_encapsulated`` returns: ``block``, the result block of ``pl_dicom_encap_index`` (uint8, on the device),
    and views of its parts -- ``frags`` int64 [M, cap, 3] (payload offset, length, offset of the item tag, all inside the
    buffer), ``heads`` uint8 [M, cap, head_bytes], ``info`` int32 [M, 4] (status, fragments found, table entries found, 0),
    ``table`` uint32 [M, tcap].  ``host()``: the same views as numpy arrays after ONE transfer of the block."""
    block: torch.Tensor
    members: int
    cap: int
    tcap: int
    head_bytes: int

    def _parts(self):
        m, cap, tcap, h = self.members, self.cap, self.tcap, self.head_bytes
        heads = m * cap * 24
        info = heads + m * cap * h
        table = info + m * 16
        return ((0, heads, "int64", (m, cap, 3)), (heads, info, "uint8", (m, cap, h)), (info, table, "int32", (m, 4)),
                (table, table + m * tcap * 4, "uint32", (m, tcap)))

    def views(self):
        """-> (frags, heads, info, table): views of the block where it lies"""
        return [self.block[a:b].view(getattr(torch, dt)).reshape(shape) for a, b, dt, shape in self._parts()]

    frags = property(lambda self: self.views()[0])
    heads = property(lambda self: self.views()[1])
    info = property(lambda self: self.views()[2])
    table = property(lambda self: self.views()[3])

    def host(self):
        """-> (frags, heads, info, table) as numpy arrays: one transfer"""
        block = self.block.cpu().numpy()
        return [block[a:b].view(dt).reshape(shape) for a, b, dt, shape in self._parts()]


def _addressable(buf: torch.Tensor) -> torch.Tensor:
    """``buf``, or a few bytes in its place when it is empty (an empty tensor has no address to hand to a kernel)"""
    return buf if buf.numel() else torch.zeros(4, dtype=torch.uint8, device=buf.device)


def index_encapsulated(buffer, first, end, cap: int, tcap: int, head_bytes: int = ENCAP_HEAD_BYTES, device=None,
                       block: torch.Tensor | None = None) -> EncapIndex:
    """``pl_dicom_encap_index``: the items of M encapsulated Pixel Data values lying anywhere inside ``buffer`` (uint8 array /
    tensor; a device tensor is used in place), one wave per value, nothing read back -> ``EncapIndex``.  Value m: its first
    item (the Basic Offset Table's) starts at byte ``first[m]``, and nothing at or beyond byte ``end[m]`` belongs to it.  Up
    to ``cap`` fragments and ``tcap`` table entries per value are stored, all are counted.  Status bits (``info[:, 0]``):
    ``ENCAP_DESCRIPTOR`` the window lies outside the buffer (nothing but the status is stored), ``ENCAP_MALFORMED`` an item
    that is none (with ``ENCAP_NO_DELIMITER``: the value ends without its delimiter), ``ENCAP_TABLE`` no table item (with
    ``ENCAP_TABLE_LENGTH``: its length is no multiple of 4), ``ENCAP_CAPACITY`` more fragments than ``cap`` or entries than
    ``tcap``.  ``block``: a uint8 device tensor of the block's size to write into."""
    dev = on_device(device)
    buf = bytes_tensor(buffer, dev)
    nbytes, buf = int(buf.numel()), _addressable(buf)
    lo, hi = index_tensor(first, torch.int64, dev).reshape(-1), index_tensor(end, torch.int64, dev).reshape(-1)
    m = int(lo.numel())
    if int(hi.numel()) != m:
        raise ValueError("index_encapsulated: first / end [M]")
    lib = _lib.load()
    need = int(lib.pl_dicom_encap_index_bytes(m, int(cap), int(tcap), int(head_bytes)))
    if need < 0:
        raise ValueError(f"index_encapsulated: M = {m}, cap = {cap}, tcap = {tcap}, head_bytes = {head_bytes} are out of range")
    if block is None:
        block = torch.empty(need, dtype=torch.uint8, device=dev)
    elif block.dtype != torch.uint8 or block.dim() != 1 or int(block.numel()) != need or not block.is_contiguous() or not block.is_cuda:
        raise ValueError(f"index_encapsulated: block must be a contiguous uint8 device tensor of {need} bytes")
    check(lib.pl_dicom_encap_index(buf.data_ptr(), nbytes, lo.data_ptr(), hi.data_ptr(), m, int(cap), int(tcap), int(head_bytes),
                                   block.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "pl_dicom_encap_index")
    return EncapIndex(block, m, int(cap), int(tcap), int(head_bytes))


def copy_ranges(src, dst: torch.Tensor, src_off, length, dst_off, device=None) -> torch.Tensor:
    """``pl_copy_ranges``: R byte ranges of ``src`` (uint8 array / tensor; a device tensor is used in place) into ``dst`` (a
    contiguous uint8 device tensor), any alignment on either side: range r is the ``length[r]`` bytes at ``src_off[r]``, they
    go to ``dst_off[r]``; no other byte of ``dst`` is written.  -> status int32 [R] on the device: 1 for a range that does not
    lie inside both buffers (nothing of it is copied).  An upper bound of the lengths is taken from a host array; a device
    tensor is reduced and read back once."""
    dev = on_device(device)
    buf = bytes_tensor(src, dev)
    if dst.dtype != torch.uint8 or dst.dim() != 1 or not dst.is_contiguous() or not dst.is_cuda:
        raise ValueError("copy_ranges: dst must be a contiguous uint8 device tensor")
    so, ln, do = (index_tensor(a, torch.int64, dev).reshape(-1) for a in (src_off, length, dst_off))
    r = int(so.numel())
    if int(ln.numel()) != r or int(do.numel()) != r:
        raise ValueError("copy_ranges: src_off / length / dst_off [R]")
    status = torch.empty(max(r, 1), dtype=torch.int32, device=dev)
    if r == 0:
        return status[:0]
    longest = int(length.max()) if isinstance(length, torch.Tensor) else int(np.max(length, initial=0))
    src_bytes, dst_bytes = int(buf.numel()), int(dst.numel())
    buf, dst = _addressable(buf), _addressable(dst)
    check(_lib.load().pl_copy_ranges(buf.data_ptr(), src_bytes, dst.data_ptr(), dst_bytes, so.data_ptr(), ln.data_ptr(),
                                     do.data_ptr(), r, max(longest, 0), status.data_ptr(),
                                     torch.cuda.current_stream(dev).cuda_stream), "pl_copy_ranges")
    return status


def _index_members(stack, metas, lay, names, frames_span: bool) -> list:
    """The item walk of every member's Pixel Data on the device (``index_encapsulated``, a second call with the exact counts
    when the first guess of the capacities overflows) and ``_fragments``' checks on what ONE transfer brings back: the
    members' metadata receive ``PixelDataFragments`` (and ``PixelDataOffsetTable`` with ``frames_span``, JPEG Lossless) as
    ``read_part10`` states them -> the heads of every member's fragments, uint8 [fragments, ENCAP_HEAD_BYTES] each."""
    base, dev = stack.offsets, stack.buffer.device
    first = base + np.asarray([m.PixelData[0] for m in metas], dtype=np.int64)
    most = max(l.frames for l in lay)
    cap, tcap = max(16, 2 * most), max(most, 1)
    while True:
        frags, heads, info, table = index_encapsulated(stack.buffer, first, base + stack.sizes, cap, tcap, device=dev).host()
        if not (info[:, 0] & ENCAP_CAPACITY).any():
            break
        walked = info[(info[:, 0] & ENCAP_DESCRIPTOR) == 0]                         # (an unsound descriptor leaves no counts)
        cap, tcap = max(int(walked[:, 1].max()), 1), max(int(walked[:, 2].max()), 1)  # the exact counts: it cannot overflow again
    out = []
    for k, (meta, name) in enumerate(zip(metas, names)):
        status, n_frag, n_table = (int(v) for v in info[k, :3])
        for bit, text in ((ENCAP_DESCRIPTOR, "the encapsulated Pixel Data value lies outside the member"),
                          (ENCAP_NO_DELIMITER, _ITEMS_NO_DELIMITER), (ENCAP_MALFORMED, _ITEMS_NO_ITEM),
                          (ENCAP_TABLE_LENGTH, _ITEMS_TABLE_LENGTH), (ENCAP_TABLE, _ITEMS_NO_TABLE)):
            if status & bit:
                raise ValueError(f"{name}: {text}")
        inside = frags[k, :n_frag] - np.asarray([base[k], 0, base[k]], dtype=np.int64)
        entries = [int(v) for v in table[k, :n_table]]
        try:
            _check_offset_table(entries, [int(t) for t in inside[:, 2]], frames_span)
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None
        meta._values["PixelDataFragments"] = [(int(o), int(n)) for o, n, _ in inside]
        if frames_span:
            meta._values["PixelDataOffsetTable"] = entries
        out.append(heads[k, :n_frag])
    return out


def _fetch_stream_head(buffer: torch.Tensor, pieces: list, nbytes: int) -> bytes:
    """The first ``nbytes`` bytes of a stream whose pieces (offset, length) lie in a device buffer, laid end to end: plain
    slice copies, one transfer (``load_zip``: a JPEG frame whose markers run past the head the index brought back)."""
    parts = []
    for off, ln in pieces:
        take = min(ln, nbytes)
        if take:
            parts.append(buffer[off:off + take])
        nbytes -= take
        if nbytes <= 0:
            break
    return (parts[0] if len(parts) == 1 else torch.cat(parts)).cpu().numpy().tobytes() if parts else b""


def _zip_frame_headers(stack, metas, lay, names, heads, codec: str, parse):
    """Every frame of the members of an archive whose frames may span fragments (JPEG Lossless, JPEG 2000) -> (member, the
    frame's pieces (offset in ``stack.buffer``, length), its length, ``parse(data, name, total)``'s answer) per frame.
    ``parse`` is given the heads of the frame's fragments as far as they are the stream's leading bytes; when it raises
    ``_PrefixTooShort`` the leading bytes are fetched from the device (4 KiB, or twice what the heads gave, and doubling)."""
    base = stack.offsets
    for k, (meta, l) in enumerate(zip(metas, lay)):
        index_of = {o: j for j, (o, _) in enumerate(meta.PixelDataFragments)}
        for frags in _jpegll_frames(meta, l.frames, names[k], codec):
            total = sum(n for _, n in frags)
            pieces = [(int(base[k]) + o, n) for o, n in frags]
            data = b""
            for o, n in frags:                              # the heads, as far as they are the stream's leading bytes
                data += heads[k][index_of[o]][:min(n, ENCAP_HEAD_BYTES)].tobytes()
                if n > ENCAP_HEAD_BYTES:
                    break
            want = max(4096, 2 * len(data))                 # (the heads of many short fragments may hold more than 4 KiB)
            while True:
                try:
                    parsed = parse(data, names[k], total)
                    break
                except _PrefixTooShort:
                    data = _fetch_stream_head(stack.buffer, pieces, min(want, total))
                    want *= 2
            yield k, pieces, total, parsed


def _zip_jpegll_decode(stack, metas, lay, names, correct_unused_bits: bool):
    """The JPEG Lossless half of ``load_zip(encapsulated=True)``: every frame's markers parsed from the heads of its fragments
    (``_jpegll_header``; leading bytes fetched from the device only when they run past the heads), a frame of one fragment
    decoded where it lies, the frames that span fragments laid end to end at 4-byte boundaries of a staging buffer by ONE
    ``copy_ranges`` -> (decode(out=, rescale=) for ``_finish_frames``, the member of every frame, the copy's status or
    None).  ``decode_jpeg_lossless_frames`` takes one buffer: with both kinds of frames it is called once per buffer, into
    the two parts of one native tensor."""
    rows, cols, ib = lay[0].rows, lay[0].cols, lay[0].sample_bytes
    dev = stack.buffer.device
    heads = _index_members(stack, metas, lay, names, True)
    scans, staged, ranges, pos = [], [], [], 0
    for k, pieces, total, header in _zip_frame_headers(stack, metas, lay, names, heads, "JPEG",
                                                       lambda data, name, total: _jpegll_header(data, rows, cols, ib * 8, name, total=total)):
        staged.append(len(pieces) > 1)
        if len(pieces) == 1:
            scans.append((k, pieces[0][0], header))
        else:
            scans.append((k, pos, header))
            at = pos
            for o, n in pieces:
                ranges.append((o, n, at))
                at += n
            pos += (total + 3) & ~3
    tables, owner = _jpegll_tables(scans)
    staged = np.asarray(staged, dtype=bool)
    staging = copied = None
    if ranges:
        moves = np.asarray(ranges, dtype=np.int64)
        staging = torch.empty(max(pos, 16), dtype=torch.uint8, device=dev)
        copied = copy_ranges(stack.buffer, staging, moves[:, 0], moves[:, 1], moves[:, 2], device=dev)
    groups = [(buf, np.flatnonzero(sel)) for buf, sel in ((stack.buffer, ~staged), (staging, staged)) if sel.any()]
    if len(groups) == 1:
        return _decode_step("jpegll", groups[0][0], tables, lay[0], metas[0], correct_unused_bits, dev), owner, copied
    common = _decode_keywords(lay[0], metas[0], correct_unused_bits, dev)
    bits, rep = common["bits_allocated"], common["pixel_representation"]
    back = torch.from_numpy(np.argsort(np.concatenate([idx for _, idx in groups]))).to(dev)

    def decode(out="container", rescale=None):              # one call per buffer, then the frames back into their order
        native = torch.empty((len(owner), rows * cols * ib), dtype=torch.uint8, device=dev)
        status, done = [], 0
        for buf, idx in groups:
            part = decode_jpeg_lossless_frames(buf, *(t[idx] for t in tables), rows, cols, bits, device=dev,
                                               native=native[done:done + idx.size])
            status.append(part._pl_status)
            done += idx.size
        x = _from_native(native[back], torch.cat(status)[back], rows, cols, bits, common["bits_stored"], rep, correct_unused_bits,
                         out, rescale, dev)
        return x, x._pl_status

    return decode, owner, copied


J2K_PLAN_FIELDS, J2K_PLAN_TABLE = 8, 72                     # PL_J2K_PLAN_FIELDS, PL_J2K_PLAN_TABLE
J2K_PLAN_UNSOUND, J2K_PLAN_HEADER_SHORT, J2K_PLAN_PASSES, J2K_PLAN_PLANES, J2K_PLAN_BEYOND = 1, 2, 4, 8, 16


def plan_jpeg2000_blocks(file_bytes, plan, tables, rows: int, cols: int, max_nodes: int, n_blocks: int | None = None, device=None,
                         blocks: torch.Tensor | None = None):
    """``pl_dicom_j2k_plan``, tier 2 of JPEG 2000 on the device: the packet headers of N codestreams lying anywhere inside
    ``file_bytes`` (uint8 array / tensor; a device tensor is used in place), one wave per frame, nothing read back ->
    (blocks int64 [n_blocks, 10] as ``decode_jpeg2000_frames`` takes them, info int32 [N, 4]), both on the device.  ``plan``
    int64 [N, ``J2K_PLAN_FIELDS``] and ``tables`` uint8 [N, ``J2K_PLAN_TABLE``] state what the host read of each stream's
    headers (``_j2k_plan_row`` builds a frame's pair; include/pylinac_hip.h has the layout): where the stream and its first
    packet lie, the tile-part's end, the coding parameters, and the rows of ``blocks`` the frame owns -- one for every code
    block of its geometry.  The rows of the included blocks are filled from the front of that range, the rest carry frame
    -1, which the decode skips.  ``info``: status (``J2K_PLAN_UNSOUND`` the plan row is unsound, nothing else is written;
    ``J2K_PLAN_HEADER_SHORT`` a packet header runs out of bytes; ``J2K_PLAN_PASSES`` passes that are not 3 x planes - 2;
    ``J2K_PLAN_PLANES`` more than 30 bit planes; ``J2K_PLAN_BEYOND`` a segment beyond the tile-part), the number of included
    blocks, two details.  A flagged frame has no rows.  ``max_nodes``: the nodes of the largest tag tree
    (``_j2k_block_counts``); ``n_blocks``: the rows of ``blocks`` (taken from a host ``plan`` when absent); ``blocks``: an
    int64 device tensor [n_blocks, 10] to write into."""
    dev = on_device(device)
    buf = bytes_tensor(file_bytes, dev)
    nbytes, buf = int(buf.numel()), _addressable(buf)
    if n_blocks is None:
        if isinstance(plan, torch.Tensor):
            raise ValueError("plan_jpeg2000_blocks: n_blocks is needed with a device plan")
        n_blocks = int(np.max(np.asarray(plan, dtype=np.int64).reshape(-1, J2K_PLAN_FIELDS)[:, 5:7].sum(axis=1), initial=0))
    plan_t = index_tensor(plan, torch.int64, dev).reshape(-1, J2K_PLAN_FIELDS)
    tab = bytes_tensor(tables, dev).reshape(-1, J2K_PLAN_TABLE)
    n = int(plan_t.shape[0])
    if int(tab.shape[0]) != n:
        raise ValueError("plan_jpeg2000_blocks: plan [N, 8] and tables [N, 72]")
    lib = _lib.load()
    nwork = int(lib.pl_dicom_j2k_plan_work_bytes(n, int(max_nodes)))
    if nwork < 0 or not 0 <= int(n_blocks) < 2 ** 31:
        raise ValueError(f"plan_jpeg2000_blocks: {n} frames (1 .. 65535), max_nodes = {max_nodes} (1 .. 2^24), n_blocks = {n_blocks}")
    if blocks is None:
        blocks = torch.empty((int(n_blocks), 10), dtype=torch.int64, device=dev)
    elif blocks.dtype != torch.int64 or tuple(blocks.shape) != (int(n_blocks), 10) or not blocks.is_contiguous() or not blocks.is_cuda:
        raise ValueError(f"plan_jpeg2000_blocks: blocks must be a contiguous int64 device tensor [{n_blocks}, 10]")
    info = torch.empty((n, 4), dtype=torch.int32, device=dev)
    work = torch.empty(nwork, dtype=torch.uint8, device=dev)
    check(lib.pl_dicom_j2k_plan(buf.data_ptr(), nbytes, plan_t.data_ptr(), tab.data_ptr(), n, int(rows), int(cols),
                                blocks.data_ptr() if n_blocks else None, int(n_blocks), info.data_ptr(), work.data_ptr(),
                                int(max_nodes), torch.cuda.current_stream(dev).cuda_stream), "pl_dicom_j2k_plan")
    return blocks, info


def _j2k_plan_row(start: int, length: int, first: int, end: int, levels: int, xcb: int, ycb: int, guard: int, exps, precincts,
                  row0: int, nrows: int):
    """one frame's row of ``plan`` and of ``tables`` for ``plan_jpeg2000_blocks``; ``end`` 0: Psot = 0"""
    coding = levels | xcb << 8 | ycb << 16 | guard << 24 | (1 << 32 if precincts else 0)
    table = np.zeros(J2K_PLAN_TABLE, dtype=np.uint8)
    table[:3 * levels + 1] = exps[:3 * levels + 1]
    if precincts:
        table[49:49 + levels + 1] = [px | py << 4 for px, py in precincts]
    return (start, length, first, end, coding, row0, nrows, 0), table


def _stream_places(pieces: list, at: int, count: int) -> list:
    """where bytes [at, at + count) of a stream lie in the buffer that holds its pieces (offset, length)"""
    out = []
    for off, ln in pieces:
        if at >= ln:
            at -= ln
            continue
        take = min(ln - at, count)
        out += range(off + at, off + at + take)
        count, at = count - take, 0
        if not count:
            break
    return out


def _check_j2k_plan(info: np.ndarray, owner, names) -> None:
    """what only the device's walk of the packet headers finds, in ``_j2k_codestream``'s words, for the first flagged frame"""
    for k in np.flatnonzero(info[:, 0]):
        status, _, d0, d1 = (int(v) for v in info[k])
        name = names[owner[k]]
        if status & J2K_PLAN_HEADER_SHORT:
            raise ValueError(f"{name}: {_J2K}{_J2K_HEADER_SHORT.format(d0)}")
        if status & J2K_PLAN_PASSES:
            raise ValueError(f"{name}: {_J2K_TRUNCATED} {_J2K_PASSES.format(d0, d1)}")
        if status & J2K_PLAN_PLANES:
            raise NotImplementedError(f"{name}: {_J2K}{_J2K_PLANES.format(d0, _J2K_MAX_PLANES)}")
        if status & J2K_PLAN_BEYOND:
            raise ValueError(f"{name}: {_J2K_TRUNCATED} {_J2K_BEYOND}")
        raise ValueError(f"{name}, frame {k} of the stack: {_J2K}the plan of its packet headers is unsound")


class _J2kFrame(NamedTuple):
    """what ``_zip_j2k_decode`` keeps of a frame between its headers and its plan row"""
    staged: bool            # it spans fragments: laid end to end in the staging buffer
    start: int              # where its stream begins in the buffer it is planned and decoded in
    length: int
    first: int              # the first packet's offset inside the stream
    end: int                # the tile-part's end inside the stream, 0 for Psot = 0
    coding: tuple           # levels, xcb, ycb, guard bits, exponents, precincts
    nrows: int              # the code blocks of its geometry
    nodes: int              # the nodes of its largest tag tree
    params: tuple           # its row of ``decode_jpeg2000_frames``' params


def _zip_j2k_decode(stack, metas, lay, names, correct_unused_bits: bool, what: str):
    """The JPEG 2000 half of ``load_zip(encapsulated=True, jpeg2000=True)``, as ``_zip_jpegll_decode``: every frame's main
    header, SOT and tile-part header parsed from the heads of its fragments (leading bytes fetched from the device only when
    the headers run past them), a frame of one fragment planned and decoded where it lies, the frames that span fragments
    laid end to end at 4-byte boundaries of a staging buffer by ONE ``copy_ranges``; per buffer one ``plan_jpeg2000_blocks``
    and one ``decode_jpeg2000_frames`` -> (decode(out=, rescale=) for ``_finish_frames``, the member of every frame, the
    copy's status or None).  The plan's result is read once, here, and what it flags is raised before any block is
    decoded.  An archive with frames that span fragments pays one transfer more: the copy's status is read before the plan
    call, which reads what was copied."""
    rows, cols, ib = lay[0].rows, lay[0].cols, lay[0].sample_bytes
    dev = stack.buffer.device
    heads = _index_members(stack, metas, lay, names, True)
    frames, owner, ranges, peeks, pos = [], [], [], [], 0

    def parse(data, name, total):
        mv = memoryview(data)
        main = _j2k_main_header(mv, len(mv), rows, cols, ib * 8, name, total=total)
        return main, _j2k_tile_header(mv, len(mv), main[0], name, total=total), len(mv)

    for k, pieces, total, (main, (first, end, psot), seen) in _zip_frame_headers(stack, metas, lay, names, heads, "JPEG 2000", parse):
        _, levels, prec, signed, guard, exps, (xcb, ycb), precincts = main
        nrows, nodes = _j2k_block_counts(_j2k_geometry(rows, cols, levels, xcb, ycb, precincts, exps, names[k]))
        if psot and seen < end + 2 <= total:                # the marker behind the tile-part is not in hand
            peeks.append((k, _stream_places(pieces, end, 2)))
        staged = len(pieces) > 1
        frames.append(_J2kFrame(staged, pos if staged else pieces[0][0], total, first, end if psot else 0,
                                (levels, xcb, ycb, guard, exps, precincts), nrows, nodes, (levels, prec, signed, 0)))
        owner.append(k)
        if staged:
            at = pos
            for o, n in pieces:
                ranges.append((o, n, at))
                at += n
            pos += (total + 3) & ~3
    if peeks:                                               # one transfer: two bytes per frame
        places = torch.from_numpy(np.asarray([p for _, where in peeks for p in where], dtype=np.int64)).to(dev)
        behind = stack.buffer[places].cpu().numpy().reshape(-1, 2)
        for (k, _), pair in zip(peeks, behind):
            if tuple(pair) == (0xFF, 0x90):
                raise NotImplementedError(f"{names[k]}: {_J2K}{_J2K_SECOND_SOT}")
    staging = copied = None
    if ranges:
        moves = np.asarray(ranges, dtype=np.int64)
        staging = torch.empty(max(pos, 16), dtype=torch.uint8, device=dev)
        copied = copy_ranges(stack.buffer, staging, moves[:, 0], moves[:, 1], moves[:, 2], device=dev)
        if bool(copied.any()):                              # (the plan below reads what was copied)
            raise ValueError(f"{what}: a fragment of a frame that spans fragments lies outside the extracted members")
    is_staged = np.asarray([f.staged for f in frames], dtype=bool)
    groups = []
    for buf, sel in ((stack.buffer, ~is_staged), (staging, is_staged)):
        idx = np.flatnonzero(sel)
        if not idx.size:
            continue
        plan, tables, row0 = [], [], 0
        for f in (frames[j] for j in idx):
            row, table = _j2k_plan_row(f.start, f.length, f.first, f.end, *f.coding, row0, f.nrows)
            plan.append(row)
            tables.append(table)
            row0 += f.nrows
        blocks, info = plan_jpeg2000_blocks(buf, np.asarray(plan, dtype=np.int64), np.stack(tables), rows, cols,
                                            max(frames[j].nodes for j in idx), n_blocks=row0, device=dev)
        params = np.asarray([frames[j].params for j in idx], dtype=np.int32)
        groups.append((buf, idx, blocks, info, params))
    order = np.concatenate([g[1] for g in groups])
    info = (groups[0][3] if len(groups) == 1 else torch.cat([g[3] for g in groups])).cpu().numpy()
    _check_j2k_plan(info[np.argsort(order)], owner, names)
    common = _decode_keywords(lay[0], metas[0], correct_unused_bits, dev)
    bits, rep = common["bits_allocated"], common["pixel_representation"]
    back = torch.from_numpy(np.argsort(order)).to(dev)

    def decode(out="container", rescale=None):              # one call per buffer, then the frames back into their order
        native = torch.empty((len(owner), rows * cols * ib), dtype=torch.uint8, device=dev)
        status, done = [], 0
        for buf, idx, blocks, _, params in groups:
            part = decode_jpeg2000_frames(buf, blocks, params, rows, cols, bits, device=dev, native=native[done:done + idx.size])
            status.append(part._pl_status)
            done += idx.size
        if len(groups) > 1:
            native, status = native[back], [torch.cat(status)[back]]
        x = _from_native(native, status[0], rows, cols, bits, common["bits_stored"], rep, correct_unused_bits, out, rescale, dev)
        return x, x._pl_status

    return decode, owner, copied


def _astype(x: torch.Tensor, np_dt: np.dtype) -> torch.Tensor:
    """``ndarray.astype`` for the integer targets the kernel does not write itself: same-size targets are a re-view (numpy's
    wrap-around), anything else goes through int64 (every container value is exact there) and wraps like a C cast."""
    name = {"uint8": torch.uint8, "int8": torch.int8, "uint16": torch.uint16, "int16": torch.int16, "uint32": torch.uint32,
            "int32": torch.int32, "int64": torch.int64, "float32": torch.float32, "float64": torch.float64}.get(np_dt.name)
    if name is None:
        raise NotImplementedError(f"dtype {np_dt} is not available on the device")
    if x.dtype == name:
        return x
    if x.element_size() == np_dt.itemsize and not name.is_floating_point:
        return x.view(name)
    if name.is_floating_point:
        return x.to(torch.int64).to(name) if not x.dtype.is_floating_point else x.to(name)
    wide = x.to(torch.int64)
    bits = np_dt.itemsize * 8
    if bits < 64:
        wide = wide & ((1 << bits) - 1)
        if np_dt.kind == "i":
            wide = torch.where(wide >= (1 << (bits - 1)), wide - (1 << bits), wide)
    signed = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[np_dt.itemsize]
    return wide.to(signed).view(name) if signed != name else wide.to(signed)


def _image_base():
    from .image import BaseImage

    return BaseImage


class DicomImage(_image_base()):
    """``pylinac.core.image.DicomImage`` (image.py:1356-1578) over the device decode: ``array`` is a numpy array like every
    class-API image; ``metadata`` answers the tags the reference's properties read."""

    def __init__(self, path, *, dtype=None, dpi: float = None, sid: float = None, sad: float = 1000, raw_pixels: bool = False,
                 invert_pixels: bool | None = None, jpeg_lossless: bool = False, jpeg2000: bool = False):
        self.path = path
        self._sid, self._dpi, self._sad = sid, dpi, sad
        self._raw_pixels, self._invert_pixels = raw_pixels, invert_pixels
        frames, metas = load_frames([path], dtype=dtype, raw_pixels=raw_pixels, invert_pixels=invert_pixels,
                                    jpeg_lossless=jpeg_lossless, jpeg2000=jpeg2000)
        self.metadata = metas[0]
        self._original_dtype = np.dtype(str(_layout(self.metadata).container).replace("torch.", ""))
        arr = _to_numpy(frames)
        self.array = arr[0] if arr.shape[0] == 1 else arr      # pydicom: (rows, cols) for one frame, (frames, rows, cols) else
        self.metrics = []
        self.metric_values = {}

    @property
    def z_position(self) -> float:
        """utilities.z_position: ImagePositionPatient[-1], else SliceLocation"""
        ipp = self.metadata.get("ImagePositionPatient")
        if ipp is not None:
            return ipp[-1]
        return self.metadata.SliceLocation

    @property
    def slice_spacing(self) -> float:
        try:
            return abs(self.metadata.SpacingBetweenSlices)
        except AttributeError:
            return self.metadata.SliceThickness

    @property
    def sid(self) -> float:
        try:
            return float(self.metadata.RTImageSID)
        except (AttributeError, ValueError, TypeError):
            return self._sid

    @property
    def sad(self) -> float:
        try:
            return float(self.metadata.RadiationMachineSAD)
        except (AttributeError, ValueError, TypeError):
            return self._sad

    @property
    def dpi(self) -> float:
        try:
            return self.dpmm * MM_PER_INCH
        except Exception:
            return self._dpi

    @property
    def dpmm(self) -> float:
        dpmm = None
        for tag in ("PixelSpacing", "ImagePlanePixelSpacing"):
            mmpd = self.metadata.get(tag)
            if mmpd is not None:
                dpmm = 1 / mmpd[0]
                break
        if dpmm is not None and self.sid is not None:
            dpmm *= self.sid / self.sad
        elif dpmm is None and self._dpi is not None:
            dpmm = self._dpi / MM_PER_INCH
        return dpmm

    @property
    def cax(self) -> Point:
        try:
            mag_factor = self.sid / self.sad
            x = self.center.x - self.metadata.XRayImageReceptorTranslation[0] * self.dpmm / mag_factor
            y = self.center.y + self.metadata.XRayImageReceptorTranslation[1] * self.dpmm / mag_factor
        except (AttributeError, ValueError, TypeError):
            return self.center
        return Point(x, y)


def _to_numpy(x: torch.Tensor) -> np.ndarray:
    t = x.cpu()
    if t.dtype in (torch.uint16, torch.uint32):            # torch -> numpy has no unsigned 16 / 32 bridge on every version
        signed = t.view(torch.int16 if t.dtype == torch.uint16 else torch.int32).numpy()
        return signed.view(np.uint16 if t.dtype == torch.uint16 else np.uint32)
    return t.numpy()
