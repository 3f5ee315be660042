"""PNG files (the lossless format film scanners, portal-dose exports and ``FileImage`` users produce besides TIFF): the chunk
walk on the host, Deflate and the filters on the device.

``read_png`` walks the chunks of a PNG -> ``PngInfo``; ``inflate`` is ``zlib.decompress`` for a batch of streams
(``pl_inflate``; ``verify=True``: with its data check, ``pl_inflate_checked``); ``decode_png_streams`` is the kernel-level entry
(``pl_png_decode``; ``verify=True``: ``pl_png_decode_checked``); ``load_frames`` is the batched loader
in the shape of ``tiff.load_frames``: the files, still compressed, laid at 4-byte boundaries of one pinned buffer -> one
copy -> ONE ``pl_png_decode`` call over a per-IDAT descriptor table -> ``PngStack`` with ``[N, H, W]`` frames and a
per-file status, nothing read back unless ``check``; ``verify=True`` also computes every chunk's CRC-32 and the stream's
Adler-32 on the device and flags the files whose stored ones differ.  The values are ``np.asarray(PIL.Image.open(f))`` -- what the
reference's ``FileImage`` hands its analyzers -- for grey files, and PIL's ``convert("I")`` of an RGB file.
"""
from __future__ import annotations

import struct
import zlib
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
STATUS_CHUNK_CRC, STATUS_ADLER = 16, 32                     # load_frames / decode_png_streams with verify=True
INFLATE_ADLER, INFLATE_OVERFLOW = 8, 16                     # inflate with verify=True
COLOUR_GREY, COLOUR_RGB, COLOUR_PALETTE, COLOUR_GREY_ALPHA, COLOUR_RGBA = 0, 2, 3, 4, 6
_COLOUR_NAMES = {COLOUR_PALETTE: "palette", COLOUR_GREY_ALPHA: "grey + alpha", COLOUR_RGBA: "RGBA"}


@dataclass
class PngInfo:
    """A PNG's IHDR and chunk layout as ``load_frames`` needs them.  ``idat``: (offset, length) of every IDAT payload in file
    order; ``consecutive``: no other chunk lies between them; ``dpi``: pHYs with unit 1 (pixels per metre x 0.0254, PIL's
    ``info["dpi"][0]``), None otherwise; ``chunks``: (type, offset of the payload, length) of every chunk; ``crcs``: the CRC-32
    each of them stores (it covers type + payload: ``length + 4`` bytes from ``offset - 4``)."""
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
    crcs: list = field(default_factory=list, repr=False)

    @property
    def samples(self) -> int:
        return {COLOUR_GREY: 1, COLOUR_RGB: 3, COLOUR_PALETTE: 1, COLOUR_GREY_ALPHA: 2, COLOUR_RGBA: 4}.get(self.colour_type, 0)

    @property
    def dpmm(self) -> float | None:
        return None if self.dpi is None else self.dpi / 25.4


def read_png(source, _what: str | None = None) -> PngInfo:
    """The chunks of a PNG (``source``: a path, bytes or a binary file object): the 8-byte signature, then every chunk's
    length checked against the file length up to IEND; IHDR (which must come first), the IDAT payloads, pHYs; ancillary
    chunks are skipped.  Every chunk's stored CRC is recorded but not verified here, nor is the zlib stream's Adler-32:
    ``load_frames`` with ``verify=True`` checks both on the device, where the files lie anyway.  Nothing about the pixel format is judged here
    (``load_frames`` refuses what the kernels do not decode)."""
    what = _what or (str(source) if isinstance(source, (str, Path)) else "PNG")
    data = source if isinstance(source, (np.ndarray, memoryview)) else source_bytes(source)
    buf = memoryview(data).cast("B")
    n = len(buf)
    if n < 8 or bytes(buf[:8]) != SIGNATURE:
        raise ValueError(f"{what}: not a PNG file (no PNG signature)")
    pos, chunks, crcs, idat, ihdr, phys, ended = 8, [], [], [], None, None, False
    while pos < n and not ended:
        if pos + 8 > n:
            raise ValueError(f"{what}: a chunk header at offset {pos} runs past the end of the file ({n} bytes)")
        length, kind = struct.unpack_from(">I4s", buf, pos)
        if pos + 12 + length > n:
            raise ValueError(f"{what}: chunk {kind!r} ({length} bytes at offset {pos}) runs past the end of the file ({n} bytes)")
        if not chunks and kind != b"IHDR":
            raise ValueError(f"{what}: the first chunk is {kind!r}, not IHDR")
        chunks.append((kind, pos + 8, length))
        crcs.append(struct.unpack_from(">I", buf, pos + 8 + length)[0])
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
                   path=source if isinstance(source, (str, Path)) else None, chunks=chunks, crcs=crcs)


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


def inflate(buffer, in_off, in_len, out_cap, wrapper: bool = True, out_off=None, device=None, out=None, verify: bool = False):
    """``pl_inflate``: ``zlib.decompress`` (``wrapper=True``; ``False``: raw Deflate, ``zlib.decompress(data, -15)``) of S
    streams lying anywhere inside ``buffer`` (uint8 array / tensor; a device tensor is used in place) -> (out uint8 tensor,
    out_off int64 [S], out_len int64 [S], status int32 [S]), all on the device, nothing read back.  Stream i is the
    ``in_len[i]`` bytes at ``in_off[i]``; at most ``out_cap[i]`` bytes of its output are stored, from ``out_off[i]`` of ``out``
    on (default: one after the other on 16-byte boundaries; given offsets must keep every window inside ``out``).  status
    bits: 1 an unsound descriptor, 2 the input ended first or the stream ended below ``out_cap[i]``, 4 corrupt Deflate.  The
    Adler-32 is not verified.

    ``verify=True`` (``pl_inflate_checked``; zlib-wrapped streams only) is what ``zlib.decompress`` really does -> (out,
    out_len, status, in_used): every stream is decoded to its end, its trailer read and compared with the Adler-32 of the
    output.  status bits besides: 2 also a missing or cut trailer and an input that ends before the final block does (zlib's
    Error -5), 8 the Adler-32 differs (Error -3, incorrect data check), 16 the stream produces more than ``out_cap[i]`` bytes
    (the first ``out_cap[i]`` are stored, the checksum is not judged).  ``in_used`` int64 [S]: the bytes consumed with the
    trailer -- what follows them is ignored, as ``zlib.decompress`` ignores it (``decompressobj().unused_data``).  (The output
    offsets are the caller's ``out_off``, or 16-byte-rounded capacities one after the other.)"""
    if verify and not wrapper:
        raise ValueError("inflate: verify=True needs wrapper=True (a raw Deflate stream has no Adler-32)")
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
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    if verify:
        max_out = int(np.clip(caps, 0, None).max(initial=0))
        work = torch.empty(max(int(lib.pl_inflate_checked_work_bytes(n, max_out)), 16), dtype=torch.uint8, device=dev)
        in_used = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        _check(lib.pl_inflate_checked(buf.data_ptr(), nbytes, off.data_ptr(), ln.data_ptr(), n, out.data_ptr(), table[:n].data_ptr(),
                                      table[n:].data_ptr(), max_out, out_len.data_ptr(), in_used.data_ptr(), status.data_ptr(),
                                      work.data_ptr(), stream), "pl_inflate_checked")
        return out, out_len[:n], status[:n], in_used[:n]
    _check(lib.pl_inflate(buf.data_ptr(), nbytes, off.data_ptr(), ln.data_ptr(), n, 1 if wrapper else 0, out.data_ptr(),
                          table[:n].data_ptr(), table[n:].data_ptr(), out_len.data_ptr(), status.data_ptr(), stream), "pl_inflate")
    return out, table[:n], out_len[:n], status[:n]


def decode_png_streams(buffer, seg_off, seg_len, seg_frame, n: int, width: int, height: int, bits: int, samples: int = 1,
                       dtype=None, device=None, idat_bytes: int | None = None, out=None, verify: bool = False, chunks=None):
    """``pl_png_decode``: IDAT payloads anywhere inside ``buffer`` (uint8 array / tensor; a device tensor is used in place)
    -> (frames [N, height, width], status int32 [N]), both on the device, nothing read back.  ``seg_off`` / ``seg_len`` int64
    [S], ``seg_frame`` int32 [S]: a frame's zlib stream is its segments in table order (consecutive in the table).
    ``idat_bytes`` (the sum of the lengths that lie inside the buffer) is derived from host arrays when not given.  ``out``:
    a device tensor to decode into.  status bits: 1 a segment outside the buffer or an unsound descriptor (nothing of the frame
    is stored), 2 the stream ends early, 4 corrupt Deflate, 8 a filter-type byte above 4.

    ``verify=True`` (``pl_png_decode_checked``) needs ``chunks``: host arrays (offset int64 [C], length int64 [C], stored
    CRC-32 uint32 [C], frame int32 [C]) of EVERY chunk's type + data range.  status bits besides: 16 a chunk's CRC-32 differs
    from the stored one, 32 the Adler-32 of the frame's inflated bytes differs from the stream's trailer (not judged for a
    stream that goes on beyond the frame; a cut trailer is bit 2).  A flagged frame's pixels are stored all the same."""
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
    stream = torch.cuda.current_stream(dev).cuda_stream
    status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    if verify:
        if chunks is None:
            raise ValueError("decode_png_streams: verify=True needs the chunk table")
        c_off, c_len = (np.asarray(x, dtype=np.int64).reshape(-1) for x in chunks[:2])
        c_crc, c_frame = np.asarray(chunks[2], dtype=np.uint32).reshape(-1), np.asarray(chunks[3], dtype=np.int32).reshape(-1)
        n_chunks = int(c_off.size)
        if n_chunks < 1 or c_len.size != n_chunks or c_crc.size != n_chunks or c_frame.size != n_chunks:
            raise ValueError("decode_png_streams: chunks = (offset, length, crc, frame) [C], C >= 1")
        max_chunk = min(max(int(c_len.max()), 0), nbytes)      # (a longer chunk is flagged by its window)
        t64 = torch.from_numpy(np.concatenate([c_off, c_len])).to(dev)
        t32 = torch.from_numpy(np.concatenate([c_crc.view(np.int32), c_frame])).to(dev)
        nwork = int(lib.pl_png_checked_work_bytes(n, n_seg, idat_bytes, width, height, bits, samples, n_chunks, max_chunk))
        work = torch.empty(max(nwork, 16), dtype=torch.uint8, device=dev)
        out = frames_out(out, "decode_png_streams", n, height, width, bits, samples, kind, dev)
        _check(lib.pl_png_decode_checked(buf.data_ptr(), nbytes, off.data_ptr(), ln.data_ptr(), frame.data_ptr(), n_seg, n, width,
                                         height, bits, samples, out.data_ptr(), kind, status.data_ptr(), work.data_ptr(),
                                         t64[:n_chunks].data_ptr(), t64[n_chunks:].data_ptr(), t32[:n_chunks].data_ptr(),
                                         t32[n_chunks:].data_ptr(), n_chunks, max_chunk, stream), "pl_png_decode_checked")
        return trim_frames(out, n, height, width), status[:n]
    nwork = int(lib.pl_png_work_bytes(n, n_seg, idat_bytes, width, height, bits, samples))
    work = torch.empty(max(nwork, 16), dtype=torch.uint8, device=dev)
    out = frames_out(out, "decode_png_streams", n, height, width, bits, samples, kind, dev)
    _check(lib.pl_png_decode(buf.data_ptr(), nbytes, off.data_ptr(), ln.data_ptr(), frame.data_ptr(), n_seg, n, width, height,
                             bits, samples, out.data_ptr(), kind, status.data_ptr(), work.data_ptr(), stream), "pl_png_decode")
    return trim_frames(out, n, height, width), status[:n]


class PngStack(FileStack):
    """What ``load_frames`` returns: ``frames`` [N, H, W] and ``status`` int32 [N] on the device, ``images`` the N files'
    ``PngInfo``; ``dpi`` the ``dpi=`` argument of the call (it overrides the files' pHYs chunks)."""
    FORMAT = "PNG"


def _stage(sources, device=None, verify: dict | None = None):
    """The host half of ``load_frames``: every file's chunks walked and judged, then the files laid at 4-byte boundaries of
    one pinned buffer and ONE copy of it queued -> (images, device buffer, segment offsets, lengths, frames, IDAT bytes).
    ``verify``: a dict that receives ``chunks`` (the chunk table of ``decode_png_streams``), ``host`` (the pinned buffer) and
    ``starts`` (the files' first bytes in it)."""
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
    if verify is not None:                                  # every chunk's type + data, the CRC it stores, its file
        verify["host"], verify["starts"] = host, starts
        verify["chunks"] = (np.asarray([st + o - 4 for st, x in zip(starts, images) for _, o, _ in x.chunks], dtype=np.int64),
                            np.asarray([c + 4 for x in images for _, _, c in x.chunks], dtype=np.int64),
                            np.asarray([v for x in images for v in x.crcs], dtype=np.uint32),
                            np.asarray([k for k, x in enumerate(images) for _ in x.chunks], dtype=np.int32))
    dbuf.copy_(host, non_blocking=True)
    table = torch.from_numpy(np.concatenate([np.asarray(off, dtype=np.int64), np.asarray(ln, dtype=np.int64)])).to(dev)
    frames = torch.from_numpy(np.asarray(frame, dtype=np.int32)).to(dev)
    s = len(off)
    return images, dbuf, table[:s], table[s:], frames, sum(ln)


def _bad_chunk(info: PngInfo, data) -> str:
    """the first chunk of a file whose CRC-32 differs from the stored one, in words (``check=True`` after a flagged status:
    the host looks once, at that file alone)"""
    for (kind, o, c), stored in zip(info.chunks, info.crcs):
        got = zlib.crc32(bytes(data[o - 4:o + c]))
        if got != stored:
            return (f"chunk {kind.decode('latin-1')!r} at byte {o - 8}: CRC-32 {got:#010x} computed, {stored:#010x} stored")
    return "a chunk's CRC-32 differs from the stored one"


def load_frames(sources, dtype=None, dpi=None, device=None, check: bool = True, out=None, verify: bool = False) -> PngStack:
    """The batched loader the reference does not have: PNG files (paths, bytes or binary file objects) of ONE width, height,
    bit depth and colour type -> ``PngStack``.  Files may differ in filter choice, compression level and IDAT layout.  Grey
    files of 8 or 16 bits give uint8 / uint16 frames (``dtype=np.uint16`` or ``np.float64``: ``array.astype(dtype)``), 8-bit
    RGB files int32 frames, PIL's ``convert("I")``.  What is not decoded (palette, grey + alpha and RGBA images, bit depths 1,
    2 and 4, 16-bit RGB, Adam7 interlace, a compression or filter method other than 0, a file without IDAT or whose IDAT chunks
    are not consecutive) raises ``ValueError`` naming the file before anything is copied.  ``dpi`` overrides the files' pHYs
    chunks, as ``FileImage(path, dpi=...)`` does; ``out``: a device tensor to decode into.

    ``verify=True``: the CRC-32 of EVERY chunk (IHDR, ancillary chunks, each IDAT, IEND) and the Adler-32 of the inflated
    pixel data are computed on the device and compared with the stored ones: status bit 16 a chunk's CRC differs, 32 the
    Adler-32 differs.  For the chunks in front of the pixel data and for the Adler-32 this is what PIL refuses
    (``UnidentifiedImageError`` / ``OSError: broken data stream``); for IDAT chunks it is STRICTER than PIL, which does not
    verify their CRCs -- it is libpng's rule.  A flagged frame disturbs no other and its pixels are stored all the same.
    ``verify=False`` (the default) verifies neither, as before.

    ``check=True`` reads the status once and raises ``OSError`` naming the first flagged file (PIL raises ``OSError`` for
    truncated or corrupt image data); ``check=False`` transfers nothing back."""
    out_kind(dtype)                        # TypeError before any file is read
    extra = {} if verify else None
    images, dbuf, off, ln, frame, idat_bytes = _stage(sources, device, extra)
    first = images[0]
    frames, status = decode_png_streams(dbuf, off, ln, frame, len(images), first.width, first.height, first.bits, first.samples,
                                        dtype=dtype, device=dbuf.device, idat_bytes=idat_bytes, out=out, verify=bool(verify),
                                        chunks=extra["chunks"] if verify else None)
    stack = PngStack(frames=frames, status=status, images=images, dpi=None if dpi is None else float(dpi))
    if check:
        got = status.cpu().numpy()
        for k in np.flatnonzero(got):
            k = int(k)
            what = ("an IDAT chunk lies outside the file" if got[k] & STATUS_WINDOW else
                    "corrupt Deflate data" if got[k] & STATUS_CORRUPT_DEFLATE else
                    "the image data ends before the last row" if got[k] & STATUS_SHORT else
                    "a filter-type byte above 4" if got[k] & STATUS_FILTER else
                    _bad_chunk(images[k], extra["host"].numpy()[extra["starts"][k]:]) if got[k] & STATUS_CHUNK_CRC else
                    "Adler-32 of the pixel data differs from the one the zlib stream ends with")
            raise OSError(f"load_frames: {file_name(images, k)}: {what}")
    return stack
