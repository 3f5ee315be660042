"""What the batched loaders (``xim``, ``tiff``, ``png`` and ``dicom`` ``.load_frames``) share on the host: sources to bytes,
arrays to device tensors, the files of a session laid into one pinned buffer, the output tensor and the stack they return.
Private: each loader keeps its parser, its refusals, its descriptor table, its kernel call and its status messages.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch

_OUT_KINDS = {None: 0, np.dtype(np.uint16): 1, np.dtype(np.float64): 2}
_NUMPY = {torch.int32: np.int32, torch.int64: np.int64}


def source_bytes(source) -> bytes:
    """A path, a bytes-like object or a binary file object -> the file's bytes (what ``dicom.load_frames`` accepts)."""
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    if isinstance(source, np.ndarray):
        return source.tobytes()
    if isinstance(source, (str, Path)):
        with open(source, "rb") as f:
            return f.read()
    if hasattr(source, "seek"):
        source.seek(0)
    return source.read()


def out_kind(dtype) -> int:
    try:
        return _OUT_KINDS[None if dtype is None else np.dtype(dtype)]
    except (KeyError, TypeError):
        raise TypeError(f"dtype {dtype!r}: None (the container dtype), np.uint16 or np.float64") from None


def on_device(device) -> torch.device:
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def bytes_tensor(buffer, dev) -> torch.Tensor:
    """uint8 array / tensor -> contiguous uint8 tensor on ``dev`` (a device tensor is used in place; a read-only array is
    copied first, torch has no read-only tensors)"""
    if not isinstance(buffer, torch.Tensor):
        host = np.ascontiguousarray(buffer, dtype=np.uint8)
        buffer = torch.from_numpy(host if host.flags.writeable else host.copy())
    return buffer.to(device=dev, dtype=torch.uint8).contiguous()


def index_tensor(a, torch_dtype, dev) -> torch.Tensor:
    """array / tensor of offsets, lengths or descriptors -> contiguous ``torch.int32`` / ``torch.int64`` tensor on ``dev``"""
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=torch_dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=_NUMPY[torch_dtype])).to(dev)


def pack_files(sources, device, parse):
    """The files of a ``load_frames`` call (paths, bytes or binary file objects) laid at 4-byte boundaries of one host buffer,
    pinned when ``device`` is a GPU, the padding zeroed -> (images, starts, host, dbuf).  ``parse(view, k, what)`` is called
    for file k with its bytes where they lie (a uint8 array) and ``what`` = ``file k`` or ``file k (path)``; it returns the
    file's record (or raises), and the record's ``path`` is set to the path, None for bytes.  ``dbuf`` is the device buffer of
    the same size; NOTHING is copied into it here: the caller finishes its refusals and then queues
    ``dbuf.copy_(host, non_blocking=True)`` itself."""
    sources = list(sources)
    if not sources:
        raise ValueError("load_frames: no files")
    # sizes first, so that the files are read straight into the pinned buffer and parsed where they lie
    held = [s if isinstance(s, (str, Path)) else source_bytes(s) for s in sources]
    sizes = [os.path.getsize(s) if isinstance(s, (str, Path)) else len(s) for s in held]
    starts, pos = [], 0
    for size in sizes:
        starts.append(pos)
        pos += (size + 3) & ~3
    dbuf = torch.empty(pos, dtype=torch.uint8, device=on_device(device))
    host = torch.empty(pos, dtype=torch.uint8, pin_memory=dbuf.device.type == "cuda")
    hv = host.numpy()
    images = []
    for k, (s, st, size) in enumerate(zip(held, starts, sizes)):
        path = s if isinstance(s, (str, Path)) else None
        if path is not None:
            with open(s, "rb", buffering=0) as f:
                got = f.readinto(memoryview(hv[st:st + size]))
            if got != size:
                raise OSError(f"{s}: read {got} of {size} bytes")
        else:
            hv[st:st + size] = np.frombuffer(s, dtype=np.uint8)
        hv[st + size:st + ((size + 3) & ~3)] = 0
        image = parse(hv[st:st + size], k, f"file {k}" + (f" ({s})" if path is not None else ""))
        image.path = path
        images.append(image)
    return images, starts, host, dbuf


def file_name(images, k: int) -> str:
    return f"file {k}" + (f" ({images[k].path})" if images[k].path is not None else "")


def frames_out(out, who: str, n: int, height: int, width: int, bits: int, samples: int, kind: int, dev) -> torch.Tensor:
    """The tensor a TIFF / PNG decode stores into: the container dtype of (bits, samples) -- int32 for RGB, PIL's
    ``convert("I")`` -- uint16 or float64 by ``kind``; allocated, or the caller's ``out`` validated under ``who``'s name."""
    container = torch.int32 if samples == 3 else (torch.uint8 if bits == 8 else torch.uint16)
    odt = (container, torch.uint16, torch.float64)[kind]
    if out is None:
        return torch.empty((max(n, 1), height, width), dtype=odt, device=dev)
    if out.dtype != odt or out.numel() < n * height * width or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous {odt} tensor of N x height x width elements")
    return out


def trim_frames(out: torch.Tensor, n: int, height: int, width: int) -> torch.Tensor:
    return out.reshape(-1)[:n * height * width].reshape(n, height, width)


@dataclass
class FileStack:
    """What ``tiff.load_frames`` / ``png.load_frames`` return: ``frames`` [N, H, W] and ``status`` int32 [N] on the device,
    ``images`` the N files' records; ``dpi`` the ``dpi=`` argument of the call (it overrides the files' own resolution)."""
    frames: torch.Tensor
    status: torch.Tensor
    images: list
    dpi: float | None = None

    FORMAT = "image"                                         # the subclass's word in the message below

    @property
    def dpmm(self) -> float | None:
        """The files' common ``dpmm`` (``dpi / 25.4``; None when no file states a resolution); ``ValueError`` when they
        disagree."""
        if self.dpi is not None:
            return self.dpi / 25.4
        values = [x.dpmm for x in self.images]
        if any(v != values[0] for v in values[1:]):
            raise ValueError(f"the {self.FORMAT} files of the stack differ in dpmm")
        return values[0]
