"""ZIP archives (what ``CatPhan504.from_zip``, ``WinstonLutz.from_zip`` and ``DicomImageStack.from_zip`` are handed: a CBCT
export or a Winston-Lutz session as one ``.zip``): the directory walk on the host, Deflate and the CRC-32 on the device.

``read_zip`` walks the End Of Central Directory record, the central directory and the local headers -> ``ZipMember`` records;
``crc32`` / ``adler32`` are ``zlib.crc32`` / ``zlib.adler32`` for a batch of byte ranges (``pl_crc32``, ``pl_adler32``); ``extract`` is ``[zf.read(n) for n in names]``: the
archive, still compressed, into one pinned buffer -> one copy -> ONE ``pl_zip_extract`` call (raw Deflate streams inflated
one wave each, stored members copied, the CRC-32 of every member's OUTPUT compared with the directory's) -> ``ZipStack`` with
the members' bytes in one device buffer and a per-member status, nothing read back unless ``check``.
``dicom.load_zip`` builds on it.  Not read: ZIP64, archives of several disks, encrypted members, methods other than stored
and Deflate; nothing is written.
"""
from __future__ import annotations

import struct
import zipfile
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch

from . import _lib
from ._lib import check as _check
from ._stack_io import bytes_tensor, index_tensor, on_device, pack_files, source_bytes

STATUS_DESCRIPTOR, STATUS_SHORT, STATUS_CORRUPT_DEFLATE, STATUS_CRC = 1, 2, 4, 8
STORED, DEFLATED = 0, 8
_EOCD, _CENTRAL, _LOCAL, _LOCATOR64 = b"PK\x05\x06", b"PK\x01\x02", b"PK\x03\x04", b"PK\x06\x07"
_METHODS = {1: "shrink", 6: "implode", 9: "Deflate64", 12: "bzip2", 14: "LZMA", 93: "Zstandard", 95: "XZ", 98: "PPMd"}


@dataclass
class ZipMember:
    """One file of an archive as the central directory states it (``crc32``, ``compressed_size`` and ``size`` come from
    there, so members written with a data descriptor work); ``header_offset``: its local header, ``data_offset``: the first
    byte of its data (after the LOCAL header's name and extra field)."""
    name: str
    method: int
    flags: int
    crc32: int
    compressed_size: int
    size: int
    header_offset: int
    data_offset: int


def _name_of(source) -> str:
    return str(source) if isinstance(source, (str, Path)) else "ZIP archive"


def read_zip(source, _what: str | None = None) -> list:
    """The members of a ZIP archive (``source``: a path, bytes or a binary file object) in central-directory order,
    directory entries left out.  The End Of Central Directory record is searched from the back (an archive comment is
    allowed); every offset and length is checked against the file length.  ``ValueError`` naming the archive (and the
    member) for what is not read: ZIP64, more than one disk, an encrypted member, a method other than 0 (stored) or 8
    (Deflate), a missing End Of Central Directory record, a central directory or a local header outside the file, a local
    header whose signature is wrong."""
    what = _what or _name_of(source)
    data = source if isinstance(source, (np.ndarray, memoryview)) else source_bytes(source)
    buf = memoryview(data).cast("B")
    n = len(buf)

    def no(text, member=None):
        raise ValueError(f"{what}: " + (f"member {member!r}: " if member is not None else "") + text)

    at = -1
    for pos in range(n - 22, max(n - 22 - 65535, 0) - 1, -1):
        if buf[pos] == 0x50 and bytes(buf[pos:pos + 4]) == _EOCD and pos + 22 + struct.unpack_from("<H", buf, pos + 20)[0] <= n:
            at = pos
            break
    if at < 0:
        no("not a ZIP archive (no End Of Central Directory record)")
    disk, cd_disk, here, total, cd_size, cd_off, _ = struct.unpack_from("<HHHHIIH", buf, at + 4)
    if (at >= 20 and bytes(buf[at - 20:at - 16]) == _LOCATOR64) or 0xFFFF in (disk, cd_disk, here, total) or \
            0xFFFFFFFF in (cd_size, cd_off):
        no("ZIP64 archives are not supported")
    if disk != 0 or cd_disk != 0 or here != total:
        no(f"archives of more than one disk are not supported (disk {disk}, {here} of {total} entries)")
    if cd_off > at or cd_size > at - cd_off:
        no(f"the central directory ({cd_size} bytes at offset {cd_off}) lies outside the file ({n} bytes)")
    members, pos = [], cd_off
    for k in range(total):
        if pos + 46 > cd_off + cd_size or bytes(buf[pos:pos + 4]) != _CENTRAL:
            no(f"entry {k} of the central directory lies outside it or has a wrong signature")
        (_, _, flags, method, _, _, crc, csize, size, nlen, elen, clen, disk0, _, _, off) = struct.unpack_from("<HHHHHHIIIHHHHHII", buf, pos + 4)
        if pos + 46 + nlen + elen + clen > cd_off + cd_size:
            no(f"entry {k} of the central directory runs past its end")
        name = bytes(buf[pos + 46:pos + 46 + nlen]).decode("utf-8" if flags & 0x800 else "cp437")
        pos += 46 + nlen + elen + clen
        if 0xFFFFFFFF in (csize, size, off) or disk0 == 0xFFFF:
            no("ZIP64 sizes or offsets are not supported", name)
        if disk0 != 0:
            no(f"it starts on disk {disk0}: archives of more than one disk are not supported", name)
        if name.endswith("/"):
            continue
        if flags & 1:
            no("encrypted members are not supported", name)
        if method not in (STORED, DEFLATED):
            no(f"compression method {method}" + (f" ({_METHODS[method]})" if method in _METHODS else "") +
               " is not supported: 0 (stored) or 8 (Deflate)", name)
        if off + 30 > n:
            no(f"its local header (offset {off}) lies outside the file ({n} bytes)", name)
        if bytes(buf[off:off + 4]) != _LOCAL:
            no(f"its local header (offset {off}) has a wrong signature", name)
        lnlen, lelen = struct.unpack_from("<HH", buf, off + 26)             # the LOCAL lengths: they may differ from the central ones
        start = off + 30 + lnlen + lelen
        if start > n or csize > n - start:
            no(f"its data ({csize} bytes at offset {start}) lie outside the file ({n} bytes)", name)
        members.append(ZipMember(name=name, method=method, flags=flags, crc32=crc, compressed_size=csize, size=size,
                                 header_offset=off, data_offset=start))
    return members


def _checksum(which: str, buffer, offsets, lengths, device, out):
    """``pl_crc32`` / ``pl_adler32``: the two share their contract line for line"""
    dev = on_device(device)
    buf = bytes_tensor(buffer, dev)
    nbytes = int(buf.numel())
    if nbytes == 0:
        buf = torch.zeros(4, dtype=torch.uint8, device=dev)
    max_len = int(lengths.max()) if isinstance(lengths, torch.Tensor) else int(np.max(lengths, initial=0))
    max_len = min(max(max_len, 0), nbytes)                   # (a longer range is flagged by its window)
    off, ln = index_tensor(offsets, torch.int64, dev), index_tensor(lengths, torch.int64, dev)
    n = int(off.numel())
    if off.dim() != 1 or ln.dim() != 1 or int(ln.numel()) != n:
        raise ValueError(f"{which}: offsets / lengths [R]")
    lib = _lib.load()
    nwork = int(getattr(lib, f"pl_{which}_work_bytes")(n, max_len))
    work = torch.empty(max(nwork, 16), dtype=torch.uint8, device=dev)
    if out is None:
        value = torch.zeros(max(n, 1), dtype=torch.uint32, device=dev)
    elif out.dtype != torch.uint32 or not out.is_contiguous() or out.numel() < n:
        raise ValueError(f"{which}: out must be a contiguous uint32 tensor [R]")
    else:
        value = out
    status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    _check(getattr(lib, f"pl_{which}")(buf.data_ptr(), nbytes, off.data_ptr(), ln.data_ptr(), n, max_len, value.data_ptr(),
                                       status.data_ptr(), work.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), f"pl_{which}")
    return value[:n], status[:n]


def crc32(buffer, offsets, lengths, device=None, out=None):
    """``pl_crc32``: ``zlib.crc32`` of R byte ranges lying anywhere inside ``buffer`` (uint8 array / tensor; a device tensor
    is used in place) -> (crc uint32 [R], status int32 [R]), both on the device, nothing read back.  Range i is the
    ``lengths[i]`` bytes at byte ``offsets[i]``.  status bit 1: the window does not lie inside the buffer -- that range's crc
    word is not written (``out``: a uint32 device tensor [R] to write into; default: zeros).  An upper bound of the lengths is
    taken from a host array; a device tensor is reduced and read back once."""
    return _checksum("crc32", buffer, offsets, lengths, device, out)


def adler32(buffer, offsets, lengths, device=None, out=None):
    """``pl_adler32``: ``zlib.adler32`` of R byte ranges lying anywhere inside ``buffer`` -> (adler uint32 [R], status int32
    [R]), both on the device, nothing read back: the arguments, the status and ``out`` of ``crc32``.  An empty range gives 1."""
    return _checksum("adler32", buffer, offsets, lengths, device, out)


def extract_members(buffer, in_off, in_len, method, crc_expected, out_off, out_size, verify: bool = True, device=None, out=None):
    """``pl_zip_extract``, the kernel-level entry: M members lying anywhere inside ``buffer`` (uint8 array / tensor; a device
    tensor is used in place) -> (out uint8 tensor, out_len int64 [M], status int32 [M]), all on the device, nothing read
    back.  Member m: ``in_len[m]`` bytes at ``in_off[m]``, ``method[m]`` 0 or 8, ``out_size[m]`` bytes to
    ``out[out_off[m]:]``.  status bits: 1 unsound descriptor (nothing of the member is stored), 2 / 4 short / corrupt
    Deflate, 8 CRC-32 mismatch (``verify``).  ``out``: a uint8 device tensor to extract into (its size bounds every output
    window)."""
    dev = on_device(device)
    buf = bytes_tensor(buffer, dev)
    nbytes = int(buf.numel())
    if nbytes == 0:
        buf = torch.zeros(4, dtype=torch.uint8, device=dev)
    offs = np.asarray(out_off, dtype=np.int64).reshape(-1)
    sizes = np.asarray(out_size, dtype=np.int64).reshape(-1)
    n = int(sizes.size)
    table = np.concatenate([np.asarray(in_off, dtype=np.int64).reshape(-1), np.asarray(in_len, dtype=np.int64).reshape(-1), offs, sizes])
    small = np.concatenate([np.asarray(method, dtype=np.int32).reshape(-1),
                            np.asarray(crc_expected, dtype=np.uint32).reshape(-1).view(np.int32)])
    if table.size != 4 * n or small.size != 2 * n:
        raise ValueError("extract_members: in_off / in_len / method / crc_expected / out_off / out_size [M]")
    if out is None:
        need = int((np.clip(offs, 0, None) + np.clip(sizes, 0, None)).max(initial=0))
        out = torch.empty(max((need + 15) & ~15, 16), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.dim() != 1:
        raise ValueError("extract_members: out must be a contiguous uint8 tensor")
    max_size = min(int(np.clip(sizes, 0, None).max(initial=0)), int(out.numel()))
    t64 = torch.from_numpy(table).to(dev)
    t32 = torch.from_numpy(small).to(dev)
    lib = _lib.load()
    nwork = int(lib.pl_zip_work_bytes(n, max_size))
    work = torch.empty(max(nwork, 16), dtype=torch.uint8, device=dev)
    out_len = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    _check(lib.pl_zip_extract(buf.data_ptr(), nbytes, t64[:n].data_ptr(), t64[n:2 * n].data_ptr(), t32[:n].data_ptr(),
                              t32[n:].data_ptr(), n, max_size, out.data_ptr(), int(out.numel()), t64[2 * n:3 * n].data_ptr(),
                              t64[3 * n:].data_ptr(), int(bool(verify)), out_len.data_ptr(), status.data_ptr(), work.data_ptr(),
                              torch.cuda.current_stream(dev).cuda_stream), "pl_zip_extract")
    return out, out_len[:n], status[:n]


@dataclass
class ZipStack:
    """What ``extract`` returns: ``buffer`` uint8 on the device, member k's bytes at ``offsets[k]`` (host int64, on 16-byte
    boundaries), ``sizes[k]`` of them; ``members`` the ``ZipMember`` records, ``status`` int32 [M] and ``lengths`` int64 [M]
    (bytes stored) on the device; ``name`` the archive's."""
    buffer: torch.Tensor
    offsets: np.ndarray
    sizes: np.ndarray
    members: list
    status: torch.Tensor
    lengths: torch.Tensor
    name: str = "ZIP archive"

    def member(self, k: int) -> torch.Tensor:
        """member k's bytes: a device view"""
        return self.buffer[int(self.offsets[k]):int(self.offsets[k]) + int(self.sizes[k])]

    def check(self) -> None:
        """The status, read once: ``zipfile.BadZipFile`` for the first flagged member (a CRC mismatch in the stdlib's words)."""
        got = self.status.cpu().numpy()
        for k in np.flatnonzero(got):
            name = self.members[int(k)].name
            if got[k] == STATUS_CRC:
                raise zipfile.BadZipFile(f"Bad CRC-32 for file {name!r}")
            why = ("its descriptor is unsound (a window outside the archive, or a stored member whose sizes differ)"
                   if got[k] & STATUS_DESCRIPTOR else "corrupt Deflate data" if got[k] & STATUS_CORRUPT_DEFLATE else
                   "the Deflate stream ends before the member's size")
            raise zipfile.BadZipFile(f"{self.name}: member {name!r}: {why}")


class _Archive:
    def __init__(self, members):
        self.members, self.path = members, None


def _select(archive: list, members, what: str) -> list:
    if members is None:
        return list(archive)
    by_name = {m.name: m for m in archive}
    taken = []
    for m in members:
        if isinstance(m, ZipMember):
            taken.append(m)
        elif m in by_name:
            taken.append(by_name[m])
        else:
            raise KeyError(f"There is no item named {m!r} in the archive ({what})")
    return taken


def stage(source, device=None):
    """The host half of ``extract``: the archive read into one pinned buffer and its directory walked where it lies ->
    (every member, the archive's name, host tensor, device buffer).  NOTHING is copied to the device here."""
    what = _name_of(source)
    records, _, host, dbuf = pack_files([source], device, lambda view, k, w: _Archive(read_zip(view, _what=what)))
    return records[0].members, what, host, dbuf


def run(taken: list, what: str, host: torch.Tensor, dbuf: torch.Tensor, verify: bool = True, check: bool = True) -> ZipStack:
    """The device half: one copy of the archive, ONE ``pl_zip_extract`` over ``taken``."""
    if not taken:
        raise ValueError(f"{what}: no members to extract")
    sizes = np.asarray([m.size for m in taken], dtype=np.int64)
    room = (sizes + 15) & ~15
    offsets = np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.int64)
    dbuf.copy_(host, non_blocking=True)
    out = torch.empty(max(int(room.sum()), 16), dtype=torch.uint8, device=dbuf.device)
    out, lengths, status = extract_members(dbuf, [m.data_offset for m in taken], [m.compressed_size for m in taken],
                                           [m.method for m in taken], [m.crc32 for m in taken], offsets, sizes, verify=verify,
                                           device=dbuf.device, out=out)
    stack = ZipStack(buffer=out, offsets=offsets, sizes=sizes, members=taken, status=status, lengths=lengths, name=what)
    if check:
        stack.check()
    return stack


def extract(source, members=None, verify: bool = True, check: bool = True, device=None) -> ZipStack:
    """``[zf.read(n) for n in names]`` on the device: a ZIP archive (a path, bytes or a binary file object) -> ``ZipStack``.
    ``members``: names or ``ZipMember`` records, in the order wanted (default: every file of the archive in
    central-directory order).  ``verify``: the CRC-32 of every member's bytes is computed on the device and compared with
    the central directory's, as ``zipfile`` does on every read.  ``check=True`` reads the status once and raises
    ``zipfile.BadZipFile`` -- ``Bad CRC-32 for file 'NAME'``, the stdlib's text, or the member and the reason for an unsound
    descriptor, a short or a corrupt Deflate stream; ``check=False`` transfers nothing back.  What ``read_zip`` refuses raises
    ``ValueError`` before anything is copied."""
    archive, what, host, dbuf = stage(source, device)
    return run(_select(archive, members, what), what, host, dbuf, verify=verify, check=check)
