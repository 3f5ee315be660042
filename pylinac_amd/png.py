"""PNG files (the lossless format film scanners, portal-dose exports and ``FileImage`` users produce besides TIFF): the chunk
walk on the host, Deflate and the filters on the device.

``read_png`` walks the chunks of a PNG -> ``PngInfo``; ``inflate`` is ``zlib.decompress`` for a batch of streams
(``pl_inflate``); ``decode_png_streams`` is the kernel-level entry (``pl_png_decode``); ``load_frames`` is the batched loader
in the shape of ``tiff.load_frames``: the files, still compressed, laid at 4-byte boundaries of one pinned buffer -> one
copy -> ONE ``pl_png_decode`` call over a per-IDAT descriptor table -> ``PngStack`` with ``[N, H, W]`` frames and a
per-file status, nothing read back unless ``check``.  The values are ``np.asarray(PIL.Image.open(f))`` -- what the
reference's ``FileImage`` hands its analyzers -- for grey files, and PIL's ``convert("I")`` of an RGB file.
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

SIGNATURE = b"\x89PNG\r\n\x1a\n"
STATUS_WINDOW, STATUS_SHORT, STATUS_CORRUPT_DEFLATE, STATUS_FILTER = 1, 2, 4, 8
COLOUR_GREY, COLOUR_RGB, COLOUR_PALETTE, COLOUR_GREY_ALPHA, COLOUR_RGBA = 0, 2, 3, 4, 6
_COLOUR_NAMES = {COLOUR_PALETTE: "palette", COLOUR_GREY_ALPHA: "grey + alpha", COLOUR_RGBA: "RGBA"}


@dataclass
class PngInfo:
    """A PNG's IHDR and chunk layout as ``load_frames`` needs them.  ``idat``: (offset, length) of every IDAT payload in file
    order; ``consecutive``: no other chunk lies between them; ``dpi``: pHYs with unit 1 (pixels per metre x 0.0254, PIL's
    ``info["dpi"][0]``), None otherwise; ``chunks``: (type, offset of the payload, length) of every chunk."""
    width: int
    height: int
    bits: int
    colour_type: int
    compression: int
    filter_method: int
    interlace: int
    idat: list
    consecutive: bool
    dpi: float | None
    path: object = None
    chunks: list = field(default_factory=list, repr=False)

    @property
    def samples(self) -> int:
        return {COLOUR_GREY: 1, COLOUR_RGB: 3, COLOUR_PALETTE: 1, COLOUR_GREY_ALPHA: 2, COLOUR_RGBA: 4}.get(self.colour_type, 0)

    @property
    def dpmm(self) -> float | None:
        return None if self.dpi is None else self.dpi / 25.4


def read_png(source, _what: str | None = None) -> PngInfo:
    """The chunks of a PNG (``source``: a path, bytes or a binary file object): the 8-byte signature, then every chunk's
    length checked against the file length up to IEND; IHDR (which must come first), the IDAT payloads, pHYs; ancillary
    chunks are skipped.  Chunk CRCs are NOT verified (a CRC pass over a session's files on the host would cost more than
    their decode on the device), nor is the zlib stream's Adler-32.  Nothing about the pixel format is judged here
    (``load_frames`` refuses what the kernels do not decode)."""
    what = _what or (str(source) if isinstance(source, (str, Path)) else "PNG")
    data = source if isinstance(source, (np.ndarray, memoryview)) else source_bytes(source)
    buf = memoryview(data).cast("B")
    n = len(buf)
    if n < 8 or bytes(buf[:8]) != SIGNATURE:
        raise ValueError(f"{what}: not a PNG file (no PNG signature)")
    pos, chunks, idat, ihdr, phys, ended = 8, [], [], None, None, False
    while pos < n and not ended:
        if pos + 8 > n:
            raise ValueError(f"{what}: a chunk header at offset {pos} runs past the end of the file ({n} bytes)")
        length, kind = struct.unpack_from(">I4s", buf, pos)
        if pos + 12 + length > n:
            raise ValueError(f"{what}: chunk {kind!r} ({length} bytes at offset {pos}) runs past the end of the file ({n} bytes)")
        if not chunks and kind != b"IHDR":
            raise ValueError(f"{what}: the first chunk is {kind!r}, not IHDR")
        chunks.append((kind, pos + 8, length))
        if kind == b"IHDR":
            if length != 13:
                raise ValueError(f"{what}: IHDR of {length} bytes")
            ihdr = struct.unpack_from(">IIBBBBB", buf, pos + 8)
        elif kind == b"IDAT":
            idat.append((pos + 8, length))
        elif kind == b"pHYs" and length == 9:
            phys = struct.unpack_from(">IIB", buf, pos + 8)
        elif kind == b"IEND":
            ended = True
        pos += 12 + length
    if ihdr is None:
        raise ValueError(f"{what}: no IHDR chunk")
    width, height, bits, colour, compression, filter_method, interlace = ihdr
    if width < 1 or height < 1:
        raise ValueError(f"{what}: width {width} x height {height}")
    kinds = [c[0] for c in chunks]
    first = kinds.index(b"IDAT") if idat else 0
    consecutive = all(k == b"IDAT" for k in kinds[first:first + len(idat)])
    dpi = phys[0] * 0.0254 if phys is not None and phys[2] == 1 else None
    return PngInfo(width=width, height=height, bits=bits, colour_type=colour, compression=compression,
                   filter_method=filter_method, interlace=interlace, idat=idat, consecutive=consecutive, dpi=dpi,
                   path=source if isinstance(source, (str, Path)) else None, chunks=chunks)


def _refuse(info: PngInfo, what: str):
    """ValueError for what the kernels do not decode, naming the file (before anything is copied)"""
    def no(text):
        raise ValueError(f"load_frames: {what}: {text}")

    if info.compression != 0:
        no(f"compression method {info.compression} is not supported (0, Deflate)")
    if info.filter_method != 0:
        no(f"filter method {info.filter_method} is not supported (0, adaptive filtering with five types)")
    if info.interlace != 0:
        no("Adam7 interlace is not supported")
    if info.colour_type in _COLOUR_NAMES:
        no(f"colour type {info.colour_type} ({_COLOUR_NAMES[info.colour_type]}) is not supported: 0 (grey) or 2 (RGB)")
    if info.colour_type not in (COLOUR_GREY, COLOUR_RGB):
        no(f"colour type {info.colour_type} is not supported: 0 (grey) or 2 (RGB)")
    if info.colour_type == COLOUR_GREY and info.bits not in (8, 16):
        no(f"bit depth {info.bits} is not supported: 8 or 16 (grey), 8 (RGB)")
    if info.colour_type == COLOUR_RGB and info.bits != 8:
        no(f"bit depth {info.bits} of an RGB image is not supported: 8")
    if not info.idat:
        no("no IDAT chunk")
    if not info.consecutive:
        no("the IDAT chunks are not consecutive")


def _input(buffer, dev):
    """-> (``buffer`` on the device, the size the kernel is told).  PNG's own, where the other loaders hand over the device
    tensor and its ``numel()``: an empty buffer becomes 4 zero bytes, so that the kernel holds a pointer, while the size stays
    that of the ARGUMENT, 0."""
    buf = bytes_tensor(buffer, dev)
    return (buf if buf.numel() else torch.zeros(4, dtype=torch.uint8, device=dev)), int(buf.numel())


def inflate(buffer, in_off, in_len, out_cap, wrapper: bool = True, out_off=None, device=None, out=None):
    """``pl_inflate``: ``zlib.decompress`` (``wrapper=True``; ``False``: raw Deflate, ``zlib.decompress(data, -15)``) of S
    streams lying anywhere inside ``buffer`` (uint8 array / tensor; a device tensor is used in place) -> (out uint8 tensor,
    out_off int64 [S], out_len int64 [S], status int32 [S]), all on the device, nothing read back.  Stream i is the
    ``in_len[i]`` bytes at ``in_off[i]``; at most ``out_cap[i]`` bytes of its output are stored, from ``out_off[i]`` of ``out``
    on (default: one after the other on 16-byte boundaries; given offsets must keep every window inside ``out``).  status
    bits: 1 an unsound descriptor, 2 the input ended first or the stream ended below ``out_cap[i]``, 4 corrupt Deflate.  The
    Adler-32 is not verified."""
    dev = on_device(device)
    buf, nbytes = _input(buffer, dev)
    caps = np.asarray(out_cap.cpu() if isinstance(out_cap, torch.Tensor) else out_cap, dtype=np.int64).reshape(-1)
    n = int(caps.size)
    if out_off is None:
        room = (np.clip(caps, 0, None) + 15) & ~15
        out_off = np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.int64)
    offs = np.asarray(out_off.cpu() if isinstance(out_off, torch.Tensor) else out_off, dtype=np.int64).reshape(-1)
    need = int((offs + np.clip(caps, 0, None)).max(initial=0)) if offs.size == n else 0
    if out is None:
        out = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < need or (n and offs.min() < 0):
        raise ValueError("inflate: out must be a contiguous uint8 tensor that holds every [out_off, out_off + out_cap)")
    off, ln = index_tensor(in_off, torch.int64, dev), index_tensor(in_len, torch.int64, dev)
    if off.dim() != 1 or int(off.numel()) != n or int(ln.numel()) != n or offs.size != n:
        raise ValueError("inflate: in_off / in_len / out_cap / out_off [S]")
    table = torch.from_numpy(np.concatenate([offs, caps])).to(dev)
    out_len = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    _check(_lib.load().pl_inflate(buf.data_ptr(), nbytes, off.data_ptr(), ln.data_ptr(), n, 1 if wrapper else 0, out.data_ptr(),
                                  table[:n].data_ptr(), table[n:].data_ptr(), out_len.data_ptr(), status.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream), "pl_inflate")
    return out, table[:n], out_len[:n], status[:n]


def decode_png_streams(buffer, seg_off, seg_len, seg_frame, n: int, width: int, height: int, bits: int, samples: int = 1,
                       dtype=None, device=None, idat_bytes: int | None = None, out=None):
    """``pl_png_decode``: IDAT payloads anywhere inside ``buffer`` (uint8 array / tensor; a device tensor is used in place)
    -> (frames [N, height, width], status int32 [N]), both on the device, nothing read back.  ``seg_off`` / ``seg_len`` int64
    [S], ``seg_frame`` int32 [S]: a frame's zlib stream is its segments in table order (consecutive in the table).
    ``idat_bytes`` (the sum of the lengths that lie inside the buffer) is derived from host arrays when not given.  ``out``:
    a device tensor to decode into.  status bits: 1 a segment outside the buffer or an unsound descriptor (nothing of the frame
    is stored), 2 the stream ends early, 4 corrupt Deflate, 8 a filter-type byte above 4."""
    kind = out_kind(dtype)
    dev = on_device(device)
    buf, nbytes = _input(buffer, dev)
    if idat_bytes is None:
        lens = np.asarray(seg_len.cpu() if isinstance(seg_len, torch.Tensor) else seg_len, dtype=np.int64)
        idat_bytes = int(np.clip(lens, 0, nbytes).sum())
    off, ln = index_tensor(seg_off, torch.int64, dev), index_tensor(seg_len, torch.int64, dev)
    frame = index_tensor(seg_frame, torch.int32, dev)
    n_seg = int(off.numel())
    if off.dim() != 1 or int(ln.numel()) != n_seg or int(frame.numel()) != n_seg or frame.dim() != 1:
        raise ValueError("decode_png_streams: seg_off / seg_len / seg_frame [S]")
    lib = _lib.load()
    nwork = int(lib.pl_png_work_bytes(n, n_seg, idat_bytes, width, height, bits, samples))
    work = torch.empty(max(nwork, 16), dtype=torch.uint8, device=dev)
    out = frames_out(out, "decode_png_streams", n, height, width, bits, samples, kind, dev)
    status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    _check(lib.pl_png_decode(buf.data_ptr(), nbytes, off.data_ptr(), ln.data_ptr(), frame.data_ptr(), n_seg, n, width, height,
                             bits, samples, out.data_ptr(), kind, status.data_ptr(), work.data_ptr(),
                             torch.cuda.current_stream(dev).cuda_stream), "pl_png_decode")
    return trim_frames(out, n, height, width), status[:n]


class PngStack(FileStack):
    """What ``load_frames`` returns: ``frames`` [N, H, W] and ``status`` int32 [N] on the device, ``images`` the N files'
    ``PngInfo``; ``dpi`` the ``dpi=`` argument of the call (it overrides the files' pHYs chunks)."""
    FORMAT = "PNG"


def _stage(sources, device=None):
    """The host half of ``load_frames``: every file's chunks walked and judged, then the files laid at 4-byte boundaries of
    one pinned buffer and ONE copy of it queued -> (images, device buffer, segment offsets, lengths, frames, IDAT bytes)."""
    def parse(data, k, what):
        info = read_png(data, _what=f"load_frames: {what}")
        _refuse(info, what)
        return info

    images, starts, host, dbuf = pack_files(sources, device, parse)
    dev = dbuf.device
    first = images[0]
    for k, x in enumerate(images):
        shape = (x.width, x.height, x.bits, x.colour_type)
        if shape != (first.width, first.height, first.bits, first.colour_type):
            raise ValueError(f"load_frames: {file_name(images, k)} differs from file 0 in width, height, bit depth or colour "
                             f"type: {shape} against {(first.width, first.height, first.bits, first.colour_type)}")
    off, ln, frame = [], [], []
    for k, (st, x) in enumerate(zip(starts, images)):
        for o, c in x.idat:
            off.append(st + o)
            ln.append(c)
            frame.append(k)
    dbuf.copy_(host, non_blocking=True)
    table = torch.from_numpy(np.concatenate([np.asarray(off, dtype=np.int64), np.asarray(ln, dtype=np.int64)])).to(dev)
    frames = torch.from_numpy(np.asarray(frame, dtype=np.int32)).to(dev)
    s = len(off)
    return images, dbuf, table[:s], table[s:], frames, sum(ln)


def load_frames(sources, dtype=None, dpi=None, device=None, check: bool = True, out=None) -> PngStack:
    """The batched loader the reference does not have: PNG files (paths, bytes or binary file objects) of ONE width, height,
    bit depth and colour type -> ``PngStack``.  Files may differ in filter choice, compression level and IDAT layout.  Grey
    files of 8 or 16 bits give uint8 / uint16 frames (``dtype=np.uint16`` or ``np.float64``: ``array.astype(dtype)``), 8-bit
    RGB files int32 frames, PIL's ``convert("I")``.  What is not decoded (palette, grey + alpha and RGBA images, bit depths 1,
    2 and 4, 16-bit RGB, Adam7 interlace, a compression or filter method other than 0, a file without IDAT or whose IDAT chunks
    are not consecutive) raises ``ValueError`` naming the file before anything is copied.  Chunk CRCs and the Adler-32 are not
    verified.  ``dpi`` overrides the files' pHYs chunks, as ``FileImage(path, dpi=...)`` does; ``out``: a device tensor to
    decode into.  ``check=True`` reads the status once and raises ``OSError`` naming the first flagged file (PIL raises
    ``OSError`` for truncated or corrupt image data); ``check=False`` transfers nothing back."""
    out_kind(dtype)                        # TypeError before any file is read
    images, dbuf, off, ln, frame, idat_bytes = _stage(sources, device)
    first = images[0]
    frames, status = decode_png_streams(dbuf, off, ln, frame, len(images), first.width, first.height, first.bits, first.samples,
                                        dtype=dtype, device=dbuf.device, idat_bytes=idat_bytes, out=out)
    stack = PngStack(frames=frames, status=status, images=images, dpi=None if dpi is None else float(dpi))
    if check:
        got = status.cpu().numpy()
        for k in np.flatnonzero(got):
            what = ("an IDAT chunk lies outside the file" if got[k] & STATUS_WINDOW else
                    "corrupt Deflate data" if got[k] & STATUS_CORRUPT_DEFLATE else
                    "the image data ends before the last row" if got[k] & STATUS_SHORT else
                    "a filter-type byte above 4")
            raise OSError(f"load_frames: {file_name(images, int(k))}: {what}")
    return stack
