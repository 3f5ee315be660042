"""Varian XIM images (SURVEY.md section 8 "next" row f1): device decoding of the compressed pixel stream.

``decode_xim_pixels`` is the kernel-level entry (``pl_xim_decode``); ``XIM`` mirrors ``pylinac.core.image.XIM``'s
reader (pylinac/core/image.py:1105-1296): same attributes (``img_width_px``, ``img_height_px``, ``bytes_per_pixel``,
``compression``, ``lookup_table``, ``histogram``, ``properties``, ``dpmm``) and the pixel ``array`` as a device
tensor.  The header / property parsing is host I/O like the reference's ``decode_binary`` calls (``parse_xim``, shared
by ``XIM``, ``XIM.from_bytes`` and the loader).

``load_frames`` is the batched form the reference does not have: a session's compressed files -> one pinned buffer -> one
copy -> ONE ``pl_xim_decode_batch`` call (``decode_xim_batch``, the kernel-level entry of the stack) -> ``XIMStack`` with
``[N, H, W]`` frames in the container dtype, uint16 or float64 and a per-file status, nothing read back unless ``check``.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check
from ._stack_io import bytes_tensor, file_name, index_tensor, on_device, out_kind, pack_files

_DTYPES = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
XIM_PROP_INT, XIM_PROP_DOUBLE, XIM_PROP_STRING, XIM_PROP_DOUBLE_ARRAY, XIM_PROP_INT_ARRAY = 0, 1, 2, 4, 5


def decode_xim_pixels(lookup_table_bytes, stream, width: int, height: int, bytes_per_pixel: int,
                      device=None) -> torch.Tensor:
    """XIM._parse_lookup_table + _get_diffs + _parse_compressed_bytes (image.py:1180-1296) on the GPU.
    ``lookup_table_bytes`` / ``stream``: uint8 arrays or tensors (the file's lookup table and the compressed pixel
    buffer that follows its 4-byte length).  -> int8/16/32/64 [height, width] device tensor."""
    if bytes_per_pixel not in _DTYPES:
        raise ValueError("The XIM image has an unsupported bytes per pixel value. "
                         "Raise a ticket on the pylinac Github with this file.")
    dev = on_device(device)

    def up(a):     # bytes_tensor without its copy of a read-only array: XIM(path) hands over views of the file's bytes
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8))
        return t.to(device=dev, dtype=torch.uint8).contiguous()

    lut, buf = up(lookup_table_bytes), up(stream)
    lib = _lib.load()
    work = torch.empty(int(lib.pl_xim_work_bytes(width, height)), dtype=torch.uint8, device=dev)
    out = torch.empty((height, width), dtype=_DTYPES[bytes_per_pixel], device=dev)
    check(lib.pl_xim_decode(lut.data_ptr(), lut.numel(), buf.data_ptr(), buf.numel(), width, height, bytes_per_pixel,
                            out.data_ptr(), work.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
          "pl_xim_decode")
    status = int(work[:4].view(torch.int32)[0])
    if status & 1:
        raise KeyError(3)          # the reference's LOOKUP_CONVERSION has no entry for size code 3
    if status & 2:
        raise ValueError(_SHORT)
    return out


class _Cursor:
    """``read`` / ``skip`` / ``tell`` over a bytes-like object without copying it (``read`` returns a memoryview)."""

    def __init__(self, data):
        self.buf = memoryview(data).cast("B")
        self.pos = 0

    def read(self, n: int):
        out = self.buf[self.pos:self.pos + n]
        self.pos += n
        return out

    def skip(self, n: int):
        self.pos += n

    def tell(self) -> int:
        return self.pos


def _read(f, fmt: str, n: int = 1):
    vals = struct.unpack("<" + fmt * n, f.read(struct.calcsize("<" + fmt) * n))
    return vals[0] if n == 1 else np.array(vals)


def _read_str(f, n: int) -> str:
    return "".join(chr(b) for b in f.read(n) if b != 0)


def parse_xim(data, target, on_pixels=None):
    """The reader of pylinac/core/image.py:1123-1178 over a bytes-like object: header fields, ``lookup_table``, ``histogram``
    and ``properties`` are set on ``target`` -> ((lookup-table offset, length) or None for an uncompressed file, (pixel-buffer
    offset, length)), byte positions inside ``data``.  ``on_pixels(lut_span, buf_span)`` is called where the reference reads
    the pixels, before the histogram and the properties."""
    xim = _Cursor(data)
    target.format_id = _read_str(xim, 8)
    target.format_version = _read(xim, "i")
    target.img_width_px = _read(xim, "i")
    target.img_height_px = _read(xim, "i")
    target.bits_per_pixel = _read(xim, "i")
    target.bytes_per_pixel = _read(xim, "i")
    target.compression = _read(xim, "i")
    if not target.compression:
        pixel_buffer_size = _read(xim, "i")
        lut_span, buf_span = None, (xim.tell(), pixel_buffer_size)
        xim.skip(pixel_buffer_size)
        if on_pixels is not None:
            on_pixels(lut_span, buf_span)
    else:
        lookup_table_size = _read(xim, "i")
        lut_span = (xim.tell(), lookup_table_size)
        target.lookup_table = np.frombuffer(xim.read(lookup_table_size), dtype=np.uint8)
        comp_pixel_buffer_size = _read(xim, "i")
        buf_span = (xim.tell(), comp_pixel_buffer_size)
        xim.skip(comp_pixel_buffer_size)
        if on_pixels is not None:
            on_pixels(lut_span, buf_span)
        _read(xim, "i")                                           # uncompressed size (unused by the reference)
    target.num_hist_bins = _read(xim, "i")
    target.histogram = _read(xim, "i", target.num_hist_bins) if target.num_hist_bins else np.array([], dtype=int)
    target.num_properties = _read(xim, "i")
    target.properties = {}
    for _ in range(target.num_properties):
        name = _read_str(xim, _read(xim, "i"))
        tipe = _read(xim, "i")
        if tipe == XIM_PROP_INT:
            value = _read(xim, "i")
        elif tipe == XIM_PROP_DOUBLE:
            value = _read(xim, "d")
        elif tipe == XIM_PROP_STRING:
            value = _read_str(xim, _read(xim, "i"))
        elif tipe == XIM_PROP_DOUBLE_ARRAY:
            value = _read(xim, "d", int(_read(xim, "i") // 8))
        elif tipe == XIM_PROP_INT_ARRAY:
            value = _read(xim, "i", int(_read(xim, "i") // 4))
        else:
            raise ValueError(f"unknown XIM property type {tipe}")
        target.properties[name] = value
    return lut_span, buf_span


class XIM:
    """pylinac/core/image.py:1105-1178 (reader) with the pixel decoding on the GPU."""

    def __init__(self, file_path, read_pixels: bool = True, device=None):
        self.path = file_path
        with open(file_path, "rb") as xim:
            data = xim.read()
        self._load(data, read_pixels, device)

    @classmethod
    def from_bytes(cls, data, read_pixels: bool = True, device=None) -> "XIM":
        """The same reader over the bytes of a file (``path`` is None)."""
        self = cls.__new__(cls)
        self.path = None
        self._load(bytes(data), read_pixels, device)
        return self

    def _load(self, data: bytes, read_pixels: bool, device):
        def pixels(lut_span, buf_span):
            raw = np.frombuffer(data, dtype=np.uint8, count=max(0, min(buf_span[1], len(data) - buf_span[0])),
                                offset=buf_span[0])
            if lut_span is None:
                dt = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[self.bytes_per_pixel]
                dev = on_device(device)
                self.array = torch.from_numpy(raw.view(dt).reshape(self.img_height_px, self.img_width_px).copy()).to(dev)
            else:
                self.array = decode_xim_pixels(self.lookup_table, raw, self.img_width_px, self.img_height_px,
                                               self.bytes_per_pixel, device=device)

        self._spans = parse_xim(data, self, pixels if read_pixels else None)

    @property
    def dpmm(self) -> float:
        """image.py:1298-1305."""
        if self.properties["PixelWidth"] != self.properties["PixelHeight"]:
            raise ValueError("The XIM image does not have the same pixel height and width")
        return 1 / (10 * self.properties["PixelHeight"])


_SHORT = "XIM pixel buffer is shorter than its lookup table implies"


def decode_xim_batch(buffer, lut_off, lut_len, buf_off, buf_len, width: int, height: int, bytes_per_pixel: int, dtype=None,
                     device=None):
    """``pl_xim_decode_batch``, the stack counterpart of ``decode_xim_pixels``: N compressed images of one (width, height,
    bytes_per_pixel) anywhere inside ``buffer`` (uint8 array / tensor; a device tensor is used in place); image i has its
    lookup table at byte ``lut_off[i]`` (``lut_len[i]`` bytes) and its pixel buffer at ``buf_off[i]`` (``buf_len[i]``
    bytes).  -> (frames [N, height, width] in the container dtype, ``np.uint16`` or ``np.float64``; status int32 [N]), both
    on the device, nothing read back.  status bits: 1 a size code 3 (the reference's ``KeyError(3)``), 2 a lookup table or
    pixel buffer shorter than the shape implies or outside the buffer, 4 (uint16) a pixel outside 0 .. 65535."""
    kind = out_kind(dtype)
    if bytes_per_pixel not in _DTYPES:
        raise ValueError("The XIM image has an unsupported bytes per pixel value. "
                         "Raise a ticket on the pylinac Github with this file.")
    dev = on_device(device)
    buf = bytes_tensor(buffer, dev)
    spans = [index_tensor(a, torch.int64, dev) for a in (lut_off, lut_len, buf_off, buf_len)]
    n = int(spans[0].numel())
    if any(int(s.numel()) != n or s.dim() != 1 for s in spans):
        raise ValueError("decode_xim_batch: the four offset / length arrays must be 1-D and of one size")
    lib = _lib.load()
    nwork = int(lib.pl_xim_batch_work_bytes(n, width, height, bytes_per_pixel, kind))
    work = torch.empty(max(nwork, 16), dtype=torch.uint8, device=dev)
    odt = (_DTYPES[bytes_per_pixel], torch.uint16, torch.float64)[kind]
    frames = torch.empty((n, height, width), dtype=odt, device=dev)
    status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    check(lib.pl_xim_decode_batch(buf.data_ptr(), buf.numel(), *(s.data_ptr() for s in spans), n, width, height,
                                  bytes_per_pixel, kind, frames.data_ptr(), status.data_ptr(), work.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream), "pl_xim_decode_batch")
    return frames, status[:n]


@dataclass
class XIMStack:
    """What ``load_frames`` returns: ``frames`` [N, H, W] and ``status`` int32 [N] on the device, ``images`` the N files as
    ``XIM(path, read_pixels=False)`` has them (header fields, ``lookup_table``, ``histogram``, ``properties``, ``dpmm``)."""
    frames: torch.Tensor
    status: torch.Tensor
    images: list

    @property
    def dpmm(self) -> float:
        """The files' common ``dpmm``; ``ValueError`` when they disagree."""
        values = [x.dpmm for x in self.images]
        if any(v != values[0] for v in values[1:]):
            raise ValueError("the XIM files of the stack differ in dpmm")
        return values[0]


def _stage(sources, device=None):
    """The host half of ``load_frames``: every file parsed, laid at a 4-byte boundary of one pinned buffer, ONE copy of that
    buffer queued -> (images, device buffer, int64 [4, N] device array of lookup offset / length and pixel-buffer offset /
    length inside it)."""
    def parse(data, k, what):
        x = XIM.__new__(XIM)
        x._spans = parse_xim(data, x)
        if x.compression:
            x.lookup_table = x.lookup_table.copy()           # (not a view of the pinned buffer, which is handed back)
        return x

    images, starts, host, dbuf = pack_files(sources, device, parse)
    first = images[0]
    for k, x in enumerate(images):
        if not x.compression:
            raise ValueError(f"load_frames: {file_name(images, k)} is not compressed; read it with XIM(path)")
        if x.bytes_per_pixel not in _DTYPES:
            raise ValueError("The XIM image has an unsupported bytes per pixel value. "
                             "Raise a ticket on the pylinac Github with this file.")
        shape = (x.img_width_px, x.img_height_px, x.bytes_per_pixel)
        if shape != (first.img_width_px, first.img_height_px, first.bytes_per_pixel):
            raise ValueError(f"load_frames: {file_name(images, k)} differs from file 0 in width, height or bytes per pixel: "
                             f"{shape} against {(first.img_width_px, first.img_height_px, first.bytes_per_pixel)}")
    dbuf.copy_(host, non_blocking=True)
    spans = np.array([[st + x._spans[0][0], x._spans[0][1], st + x._spans[1][0], x._spans[1][1]]
                      for st, x in zip(starts, images)], dtype=np.int64).T
    return images, dbuf, torch.from_numpy(np.ascontiguousarray(spans)).to(dbuf.device)


def load_frames(sources, dtype=None, device=None, check: bool = True) -> XIMStack:
    """The batched loader the reference does not have: compressed .xim files (paths, bytes or binary file objects) of ONE
    width, height and bytes per pixel -> ``XIMStack``.  Every file is parsed on the host and laid at a 4-byte boundary of one
    pinned buffer; one copy takes that buffer to the device, ONE ``pl_xim_decode_batch`` call decodes every image where it
    lies and stores ``dtype`` (None: the container dtype, ``np.uint16`` or ``np.float64`` = ``array.astype(dtype)``).
    ``check=True`` reads the status once and raises for the first flagged file what ``XIM(path)`` raises (``KeyError(3)``,
    ``ValueError``), or a ``ValueError`` for a file that does not fit uint16; ``check=False`` transfers nothing back."""
    out_kind(dtype)                        # TypeError before any file is read
    images, dbuf, spans = _stage(sources, device)
    first = images[0]
    frames, status = decode_xim_batch(dbuf, spans[0], spans[1], spans[2], spans[3], first.img_width_px, first.img_height_px,
                                      first.bytes_per_pixel, dtype=dtype, device=dbuf.device)
    stack = XIMStack(frames=frames, status=status, images=images)
    if check:
        flags = status.cpu().numpy()
        for k in np.flatnonzero(flags):
            if flags[k] & 1:
                raise KeyError(3)      # the reference's LOOKUP_CONVERSION has no entry for size code 3
            if flags[k] & 2:
                raise ValueError(_SHORT)
            raise ValueError(f"load_frames: {file_name(images, int(k))} holds pixels outside 0 .. 65535 and does not fit uint16")
    return stack
