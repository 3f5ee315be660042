"""Strip TIFFs of scanned film (the third container ``pylinac.image.load`` accepts, after DICOM and XIM): the IFD walk on the
host, the pixels on the device.

``read_tiff`` walks the first IFD of a classic TIFF (TIFF 6.0 section 2) -> ``TiffInfo``; ``decode_tiff_strips`` is the
kernel-level entry (``pl_tiff_decode``); ``load_frames`` is the batched loader in the shape of ``xim.load_frames``: the
files, still compressed, laid at 4-byte boundaries of one pinned buffer -> one copy -> ONE ``pl_tiff_decode`` call over a
per-strip descriptor table -> ``TiffStack`` with ``[N, H, W]`` frames and a per-file status, nothing read back unless
``check``.  The values are ``np.asarray(PIL.Image.open(f))`` -- what the reference's ``FileImage`` hands its analyzers --
for grey files, and PIL's ``convert("I")`` of an RGB file.

Deflate strips (Compression 8, "Adobe Deflate", and 32946: what GIMP, Python writers and scanners' "compressed TIFF" make)
are opt-in: ``load_frames(..., deflate=True)`` and a ``compressions`` mask with bit 8 go through ``pl_tiff_decode_ex``, where
every strip -- one zlib stream -- is inflated by one wave of the device and its Adler-32 is checked, as libtiff does (status
bits ``STATUS_CORRUPT_DEFLATE`` and ``STATUS_ADLER``).  Without the keyword such files are refused as before.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np
import torch

from . import _lib
from ._lib import check as _check
from ._stack_io import (FileStack, bytes_tensor, file_name, frames_out, index_tensor, on_device, out_kind, pack_files,
                        source_bytes, trim_frames)

COMPRESSION_NONE, COMPRESSION_LZW, COMPRESSION_PACKBITS = 1, 5, 32773
COMPRESSION_DEFLATE, COMPRESSION_DEFLATE_OLD = 8, 32946
_COMPRESSION_BIT = {COMPRESSION_NONE: 1, COMPRESSION_PACKBITS: 2, COMPRESSION_LZW: 4}
_DEFLATE_BIT = {COMPRESSION_DEFLATE: 8, COMPRESSION_DEFLATE_OLD: 8}      # (pl_tiff_decode_ex only)
STATUS_WINDOW, STATUS_SHORT, STATUS_CORRUPT_LZW = 1, 2, 4
STATUS_CORRUPT_DEFLATE, STATUS_ADLER = 8, 16
# TIFF 6.0 field types -> (struct code, bytes); SHORT, LONG and RATIONAL are what the tags read here may have
_TYPES = {1: ("B", 1), 3: ("H", 2), 4: ("I", 4), 5: ("II", 8)}
_TAGS = (256, 257, 258, 259, 262, 273, 277, 278, 279, 282, 283, 284, 296, 317, 338, 339, 322)


@dataclass
class TiffInfo:
    """The first IFD of a classic TIFF as ``load_frames`` needs it.  ``strips``: (offset, byte count, first row, rows) per
    strip; ``dpi``: XResolution in pixels per inch (ResolutionUnit 2, or 3 = per centimetre x 2.54), None without them."""
    width: int
    height: int
    bits: int
    samples: int
    compression: int
    predictor: int
    byte_order: str
    strips: list
    dpi: float | None
    photometric: int = 1
    planar: int = 1
    sample_format: int = 1
    extra_samples: int = 0
    tiled: bool = False
    bits_per_sample: tuple = ()
    path: object = None
    tags: dict = field(default_factory=dict, repr=False)

    @property
    def dpmm(self) -> float | None:
        return None if self.dpi is None else self.dpi / 25.4


def _walk_ifd(data, what: str) -> tuple:
    """-> (byte order, {tag: tuple of values}) of the first IFD; every offset is checked against the file length"""
    buf = memoryview(data).cast("B")
    n = len(buf)
    if n < 8 or bytes(buf[:2]) not in (b"II", b"MM"):
        raise ValueError(f"{what}: not a TIFF file (no II / MM byte-order mark)")
    order = bytes(buf[:2]).decode()
    e = "<" if order == "II" else ">"
    magic, ifd = struct.unpack_from(e + "HI", buf, 2)
    if magic == 43:
        raise ValueError(f"{what}: BigTIFF (magic 43) is not supported")
    if magic != 42:
        raise ValueError(f"{what}: not a TIFF file (magic {magic})")
    if ifd < 8 or ifd + 2 > n:
        raise ValueError(f"{what}: the first IFD (offset {ifd}) lies outside the file ({n} bytes)")
    count, = struct.unpack_from(e + "H", buf, ifd)
    if ifd + 2 + 12 * count > n:
        raise ValueError(f"{what}: the first IFD ({count} entries at offset {ifd}) lies outside the file ({n} bytes)")
    tags = {}
    for k in range(count):
        tag, typ, cnt = struct.unpack_from(e + "HHI", buf, ifd + 2 + 12 * k)
        if tag not in _TAGS:
            continue
        if typ not in _TYPES:
            raise ValueError(f"{what}: tag {tag} has field type {typ}; BYTE, SHORT, LONG or RATIONAL expected")
        code, size = _TYPES[typ]
        at = ifd + 2 + 12 * k + 8
        if size * cnt > 4:
            at, = struct.unpack_from(e + "I", buf, at)
            if at + size * cnt > n:
                raise ValueError(f"{what}: the values of tag {tag} ({cnt} x {size} bytes at offset {at}) lie outside the "
                                 f"file ({n} bytes)")
        vals = struct.unpack_from(e + code * cnt, buf, at)
        if typ == 5:
            vals = tuple((vals[2 * j], vals[2 * j + 1]) for j in range(cnt))
        tags[tag] = vals
    return order, tags


def read_tiff(source, _what: str | None = None) -> TiffInfo:
    """The first IFD of a classic TIFF (``source``: a path, bytes or a binary file object): byte order II / MM, magic 42
    (BigTIFF is refused), the tags 256-259, 262, 273, 277-279, 282-284, 296, 317, 338, 339 (and 322 for detection), inline or
    at an offset, every offset validated against the file length.  Nothing about the pixel format is judged here
    (``load_frames`` refuses what the kernels do not decode)."""
    what = _what or (str(source) if isinstance(source, (str, Path)) else "TIFF")
    data = source if isinstance(source, (np.ndarray, memoryview)) else source_bytes(source)
    order, tags = _walk_ifd(data, what)
    n = len(memoryview(data).cast("B"))

    def one(tag, default=None):
        v = tags.get(tag)
        if v is None:
            if default is None:
                raise ValueError(f"{what}: tag {tag} is missing")
            return default
        return v[0]

    width, height = int(one(256)), int(one(257))
    if width < 1 or height < 1:
        raise ValueError(f"{what}: ImageWidth {width} x ImageLength {height}")
    samples = int(one(277, 1))
    bps = tuple(int(b) for b in tags.get(258, (1,)))
    if len(bps) == 1 and samples > 1:
        bps = bps * samples
    tiled = 322 in tags
    strips = []
    if not tiled:
        offs = tags.get(273)
        counts = tags.get(279)
        if offs is None:
            raise ValueError(f"{what}: tag 273 (StripOffsets) is missing")
        rps = min(int(one(278, height)), height)
        if rps < 1:
            raise ValueError(f"{what}: RowsPerStrip 0")
        n_strips = -(-height // rps)
        planes = samples if int(one(284, 1)) == 2 else 1
        if len(offs) != n_strips * planes or (counts is not None and len(counts) != len(offs)):
            raise ValueError(f"{what}: {len(offs)} strip offsets / {0 if counts is None else len(counts)} byte counts for "
                             f"{n_strips * planes} strips")
        if counts is None:                                # (TIFF 6.0 requires the tag; old writers of one strip leave it out)
            if n_strips != 1:
                raise ValueError(f"{what}: tag 279 (StripByteCounts) is missing")
            counts = (n - offs[0],)
        for k, (o, c) in enumerate(zip(offs, counts)):
            if o + c > n:
                raise ValueError(f"{what}: strip {k} ({c} bytes at offset {o}) lies outside the file ({n} bytes)")
            row0 = (k % n_strips) * rps
            strips.append((int(o), int(c), row0, min(rps, height - row0)))
    unit, xres = int(one(296, 2)), tags.get(282)
    dpi = None
    if xres is not None and xres[0][1] != 0 and unit in (2, 3):
        dpi = xres[0][0] / xres[0][1] * (2.54 if unit == 3 else 1.0)
    return TiffInfo(width=width, height=height, bits=bps[0], samples=samples, compression=int(one(259, 1)),
                    predictor=int(one(317, 1)), byte_order=order, strips=strips, dpi=dpi, photometric=int(one(262, 1)),
                    planar=int(one(284, 1)), sample_format=int(one(339, 1)), extra_samples=len(tags.get(338, ())), tiled=tiled,
                    bits_per_sample=bps, path=source if isinstance(source, (str, Path)) else None, tags=tags)


def _refuse(info: TiffInfo, data, what: str, deflate: bool = False):
    """ValueError for what the kernels do not decode, naming the file (before anything is copied).  ``deflate``: Compression
    8 / 32946 passes, with Predictor 1 or 2; every other message is what it is without it."""
    def no(text):
        raise ValueError(f"load_frames: {what}: {text}")

    deflated = deflate and info.compression in _DEFLATE_BIT
    if info.tiled:
        no("tiled TIFFs (tag 322 TileWidth) are not supported, strips only")
    if info.compression not in _COMPRESSION_BIT and not deflated:
        no(f"Compression {info.compression} is not supported: 1 (none), 32773 (PackBits) or 5 (LZW)"
           + ("; 8 or 32946 (Deflate)" if deflate else ""))
    if info.predictor not in (1, 2):
        no(f"Predictor {info.predictor} is not supported: 1, or 2 (horizontal differencing) with LZW"
           + (" or Deflate" if deflate else ""))
    if info.predictor == 2 and info.compression != COMPRESSION_LZW and not deflated:
        no(f"Predictor 2 with Compression {info.compression} is not supported (LZW only"
           + (", or Deflate)" if deflate else ")"))
    if info.planar != 1:
        no(f"PlanarConfiguration {info.planar} is not supported (1, chunky)")
    if info.sample_format != 1:
        no(f"SampleFormat {info.sample_format} is not supported (1, unsigned integers)")
    if info.extra_samples:
        no("ExtraSamples (an alpha channel) are not supported")
    if info.samples == 1:
        if info.photometric != 1:
            no(f"PhotometricInterpretation {info.photometric} of a one-sample image is not supported (1, BlackIsZero)")
        if info.bits not in (8, 16):
            no(f"BitsPerSample {info.bits} is not supported: 8 or 16 (grey), 8/8/8 (RGB)")
    elif info.samples == 3:
        if info.photometric != 2:
            no(f"PhotometricInterpretation {info.photometric} of a three-sample image is not supported (2, RGB)")
        if info.bits_per_sample != (8, 8, 8):
            no(f"BitsPerSample {info.bits_per_sample} is not supported for RGB: 8/8/8")
    else:
        no(f"SamplesPerPixel {info.samples} is not supported: 1 (grey) or 3 (RGB)")
    if info.compression == COMPRESSION_LZW:
        buf = memoryview(data).cast("B")
        for k, (o, c, _, _) in enumerate(info.strips):
            if c >= 2 and buf[o] == 0 and (buf[o + 1] & 1):
                no(f"strip {k} is an old-style (bit-reversed) LZW stream, which is not supported")


def decode_tiff_strips(buffer, strip_off, strip_len, strip_desc, frame_flags, width: int, height: int, bits: int,
                       samples: int = 1, dtype=None, device=None, compressions: int | None = None,
                       max_strip_bytes: int | None = None, out=None):
    """``pl_tiff_decode``: strips anywhere inside ``buffer`` (uint8 array / tensor; a device tensor is used in place) ->
    (frames [N, height, width], status int32 [N]), both on the device, nothing read back.  ``strip_off`` / ``strip_len``
    int64 [S]; ``strip_desc`` int32 [S, 4] = frame, first row, rows, Compression; ``frame_flags`` int32 [N]: bit 0 Predictor
    2, bit 1 big-endian samples.  ``compressions`` (mask 1 none | 2 PackBits | 4 LZW | 8 Deflate: descriptors 8 and 32946) and
    ``max_strip_bytes`` are derived from host arrays when not given; a mask with bit 8 goes through ``pl_tiff_decode_ex``.
    ``out``: a device tensor to decode into.  status bits: 1 a strip outside the buffer or an unsound descriptor (nothing of
    the frame is stored), 2 a short strip, 4 corrupt LZW, 8 corrupt Deflate, 16 a Deflate strip's Adler-32 differs."""
    kind = out_kind(dtype)
    dev = on_device(device)
    if compressions is None:
        compressions = 0
        for c in np.unique(np.asarray(strip_desc.cpu() if isinstance(strip_desc, torch.Tensor) else strip_desc)[:, 3]):
            compressions |= _COMPRESSION_BIT.get(int(c), 0) | _DEFLATE_BIT.get(int(c), 0)
        compressions = compressions or 1
    if max_strip_bytes is None:
        max_strip_bytes = int(np.asarray(strip_len.cpu() if isinstance(strip_len, torch.Tensor) else strip_len).max(initial=0))
        max_strip_bytes = max(0, min(max_strip_bytes, 1 << 36))
    buf = bytes_tensor(buffer, dev)
    off, ln = index_tensor(strip_off, torch.int64, dev), index_tensor(strip_len, torch.int64, dev)
    desc, flags = index_tensor(strip_desc, torch.int32, dev), index_tensor(frame_flags, torch.int32, dev)
    n_strips, n = int(off.numel()), int(flags.numel())
    if off.dim() != 1 or int(ln.numel()) != n_strips or tuple(desc.shape) != (n_strips, 4) or flags.dim() != 1:
        raise ValueError("decode_tiff_strips: strip_off / strip_len [S], strip_desc [S, 4], frame_flags [N]")
    lib = _lib.load()
    ex = bool(compressions & 8)                           # (the older entries go on refusing masks above 7)
    work_bytes, decode, who = ((lib.pl_tiff_work_bytes_ex, lib.pl_tiff_decode_ex, "pl_tiff_decode_ex") if ex else
                               (lib.pl_tiff_work_bytes, lib.pl_tiff_decode, "pl_tiff_decode"))
    nwork = int(work_bytes(n, n_strips, max_strip_bytes, width, height, bits, samples, compressions))
    work = torch.empty(max(nwork, 16), dtype=torch.uint8, device=dev)
    out = frames_out(out, "decode_tiff_strips", n, height, width, bits, samples, kind, dev)
    status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    _check(decode(buf.data_ptr(), buf.numel(), off.data_ptr(), ln.data_ptr(), desc.data_ptr(), n_strips, max_strip_bytes,
                  flags.data_ptr(), n, width, height, bits, samples, compressions, out.data_ptr(), kind, status.data_ptr(),
                  work.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), who)
    return trim_frames(out, n, height, width), status[:n]


class TiffStack(FileStack):
    """What ``load_frames`` returns: ``frames`` [N, H, W] and ``status`` int32 [N] on the device, ``images`` the N files'
    ``TiffInfo``; ``dpi`` the ``dpi=`` argument of the call (it overrides the files' resolution tags)."""
    FORMAT = "TIFF"


def _stage(sources, device=None, deflate: bool = False):
    """The host half of ``load_frames``: every file's IFD walked and judged, then the files laid at 4-byte boundaries of one
    pinned buffer and ONE copy of it queued -> (images, device buffer, strip offsets, lengths, descriptors, frame flags,
    compression mask, longest strip)."""
    def parse(data, k, what):
        info = read_tiff(data, _what=what)
        _refuse(info, data, what, deflate)
        return info

    images, starts, host, dbuf = pack_files(sources, device, parse)
    dev = dbuf.device
    first = images[0]
    for k, x in enumerate(images):
        shape = (x.width, x.height, x.bits, x.samples)
        if shape != (first.width, first.height, first.bits, first.samples):
            raise ValueError(f"load_frames: {file_name(images, k)} differs from file 0 in width, height, bits per sample or "
                             f"samples per pixel: {shape} against {(first.width, first.height, first.bits, first.samples)}")
    off, ln, desc, flags, mask = [], [], [], [], 0
    for k, (st, x) in enumerate(zip(starts, images)):
        flags.append((1 if x.predictor == 2 else 0) | (2 if x.byte_order == "MM" and x.bits == 16 else 0))
        mask |= _COMPRESSION_BIT.get(x.compression) or _DEFLATE_BIT[x.compression]
        for o, c, row0, rows in x.strips:
            off.append(st + o)
            ln.append(c)
            desc.append((k, row0, rows, x.compression))
    if (mask & 2) and len(off) > 65535:
        raise ValueError(f"load_frames: {len(off)} strips in a stack with PackBits files; at most 65535")
    dbuf.copy_(host, non_blocking=True)
    table = np.concatenate([np.asarray(off, dtype=np.int64), np.asarray(ln, dtype=np.int64)])
    table = torch.from_numpy(table).to(dev)
    small = np.concatenate([np.asarray(desc, dtype=np.int32).ravel(), np.asarray(flags, dtype=np.int32)])
    small = torch.from_numpy(small).to(dev)
    s = len(off)
    return (images, dbuf, table[:s], table[s:], small[:4 * s].reshape(s, 4), small[4 * s:], mask, max(ln, default=0))


def load_frames(sources, dtype=None, dpi=None, device=None, check: bool = True, deflate: bool = False) -> TiffStack:
    """The batched loader the reference does not have: strip TIFFs (paths, bytes or binary file objects) of ONE width,
    height, BitsPerSample and SamplesPerPixel -> ``TiffStack``.  Files may differ in compression (none, PackBits, LZW),
    predictor, byte order and strip layout.  Grey files of 8 or 16 bits give uint8 / uint16 frames (``dtype=np.uint16`` or
    ``np.float64``: ``array.astype(dtype)``), 8-bit RGB files int32 frames, PIL's ``convert("I")``.  What is not decoded
    (tiles, BigTIFF, other compressions, Predictor 3 or Predictor 2 without LZW, PlanarConfiguration 2, WhiteIsZero and
    palette images, 1-, 4- and 32-bit and float samples, 16-bit RGB, ExtraSamples, old-style LZW) raises ``ValueError`` naming
    the file before anything is copied.  ``dpi`` overrides the files' resolution tags, as ``FileImage(path, dpi=...)`` does.
    ``check=True`` reads the status once and raises ``OSError`` naming the first flagged file (PIL raises ``OSError`` for a
    truncated or corrupt strip); ``check=False`` transfers nothing back.

    ``deflate=True`` also accepts Compression 8 and 32946 (Deflate), with Predictor 1 or 2, in the same sample formats and
    mixed with the others in one stack.  Every strip is inflated on the device and checked as libtiff checks it: corrupt
    Deflate data (a bad zlib header included) and an Adler-32 that differs from the stream's field flag the file; bytes
    behind the stream, a field that is cut off and a stream longer than the strip's rows do not."""
    out_kind(dtype)                        # TypeError before any file is read
    images, dbuf, off, ln, desc, flags, mask, longest = _stage(sources, device, deflate)
    first = images[0]
    frames, status = decode_tiff_strips(dbuf, off, ln, desc, flags, first.width, first.height, first.bits, first.samples,
                                        dtype=dtype, device=dbuf.device, compressions=mask, max_strip_bytes=longest)
    stack = TiffStack(frames=frames, status=status, images=images, dpi=None if dpi is None else float(dpi))
    if check:
        got = status.cpu().numpy()
        for k in np.flatnonzero(got):
            what = ("a strip lies outside the file" if got[k] & STATUS_WINDOW else
                    "corrupt LZW data (a code names a table entry that does not exist)" if got[k] & STATUS_CORRUPT_LZW else
                    "corrupt Deflate data in a strip" if got[k] & STATUS_CORRUPT_DEFLATE else
                    "the Adler-32 of a strip differs from the checksum its stream ends with" if got[k] & STATUS_ADLER else
                    "a strip decodes to fewer bytes than its rows hold")
            raise OSError(f"load_frames: {file_name(images, int(k))}: {what}")
    return stack
