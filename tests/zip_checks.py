"""Shared checks of pylinac_amd.zipstack and dicom.load_zip: pl_crc32, pl_zip_extract, read_zip's directory walk, extract and
load_zip (tests/test_emulated_zip.py on the CPU emulator, tests/test_gpu_zip.py on the MI355X).  Every comparison is EQUALITY:
``crc32`` against ``zlib.crc32``, archives against ``zipfile.ZipFile.read``, ``load_zip`` against ``load_frames`` on the
stdlib-extracted bytes AND against the arrays the files were written from.  The archives are written by ``zipfile``; what it
cannot write (a longer local extra field, ZIP64 sentinels, several disks, encryption flags, damage) is made by patching bytes,
and ``zipfile`` must still read every sound fixture back.  A member's output stays below about 100 KiB here (the emulator
runs a fiber per work-item)."""
from __future__ import annotations

import io
import re
import struct
import zipfile
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

import dicom_rle_checks as rle
from pylinac_amd import dicom, zipstack

to_np = dicom._to_numpy
TILE = 16384
CRC_LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 17, 3 * TILE]


def u32(t: torch.Tensor) -> list:
    return [int(v) & 0xFFFFFFFF for v in t.cpu().view(torch.int32).tolist()]


# ---- 1: pl_crc32 against zlib.crc32 ---------------------------------------------------------------------------------------
def crc_layout(fill):
    """every length of CRC_LENGTHS at source offsets 0, 1, 2 and 3 mod 4, other bytes on both sides -> (buffer, offsets, lengths)"""
    total = sum(CRC_LENGTHS) * 4 + 16 * len(CRC_LENGTHS) * 4 + 64
    buf = fill(total)
    off, ln, pos = [], [], 5
    for n in CRC_LENGTHS:
        for a in range(4):
            pos += (a - pos) % 4 + 4                                               # a gap, then the alignment wanted
            off.append(pos), ln.append(n)
            pos += n
    assert pos < total and {o % 4 for o in off} == {0, 1, 2, 3}
    return buf, off, ln


def check_crc_random(dev):
    rng = np.random.default_rng(41)
    buf, off, ln = crc_layout(lambda n: rng.integers(0, 256, n, dtype=np.uint8))
    crc, status = zipstack.crc32(buf, off, ln, device=dev)
    want = [zlib.crc32(buf[o:o + n].tobytes()) for o, n in zip(off, ln)]
    assert status.cpu().tolist() == [0] * len(off)
    got = u32(crc)
    assert got == want, [(o, n) for o, n, g, w in zip(off, ln, got, want) if g != w]
    # device tensors are used in place
    crc2, _ = zipstack.crc32(torch.from_numpy(buf).to(dev), torch.tensor(off[:9]).to(dev), torch.tensor(ln[:9]).to(dev), device=dev)
    assert u32(crc2) == want[:9]


def check_crc_constant(dev, value):
    """all-zero and all-0xFF contents: raw() of zeros is 0, so only the init term tells their lengths apart"""
    buf, off, ln = crc_layout(lambda n: np.full(n, value, dtype=np.uint8))
    crc, status = zipstack.crc32(buf, off, ln, device=dev)
    want = [zlib.crc32(bytes([value]) * n) for n in ln]
    assert status.cpu().tolist() == [0] * len(off) and u32(crc) == want
    assert len({w for w, n in zip(want, ln)}) == len(set(ln))


def check_crc_edges(dev):
    rng = np.random.default_rng(42)
    buf = rng.integers(0, 256, TILE + 39, dtype=np.uint8)                          # (the buffer's size: odd, no multiple of 4)
    n = len(buf)
    # ranges ending at the buffer's last byte at odd lengths, the whole buffer, an empty range at its end
    off = [n - 1, n - 7, n - 33, 3, 0, n]
    ln = [1, 7, 33, n - 3, n, 0]
    crc, status = zipstack.crc32(buf, off, ln, device=dev)
    assert status.cpu().tolist() == [0] * 6
    assert u32(crc) == [zlib.crc32(buf[o:o + m].tobytes()) for o, m in zip(off, ln)]
    # windows outside the buffer: status 1, the crc word keeps its sentinel; the neighbours are computed
    off = [0, n - 4, -1, 5, n + 1, 7]
    ln = [10, 5, 4, -2, 0, 1 << 40]
    out = torch.from_numpy(np.full(6, 0x5A5A5A5A, dtype=np.int32)).view(torch.uint32).to(dev)
    crc, status = zipstack.crc32(buf, off, ln, device=dev, out=out)
    assert status.cpu().tolist() == [0, 1, 1, 1, 1, 1]
    assert u32(crc) == [zlib.crc32(buf[:10].tobytes())] + [0x5A5A5A5A] * 5


# ---- archives (test files only) -------------------------------------------------------------------------------------------
class Pipe:
    """a stream without seek / tell: zipfile then writes data descriptors (flag bit 3)"""

    def __init__(self):
        self.data = bytearray()

    def write(self, b):
        self.data += b
        return len(b)

    def flush(self):
        pass


def make_zip(entries, comment: bytes = b"", pipe: bool = False) -> bytes:
    """entries: (name, data, compress_type, level); a name ending in "/" is a directory entry"""
    sink = Pipe() if pipe else io.BytesIO()
    with zipfile.ZipFile(sink, "w") as zf:
        for name, data, kind, level in entries:
            if name.endswith("/"):
                zf.writestr(zipfile.ZipInfo(name), b"")
            else:
                zf.writestr(zipfile.ZipInfo(name), data, compress_type=kind, compresslevel=level)
        zf.comment = comment
    return bytes(sink.data) if pipe else sink.getvalue()


def stdlib_read(data) -> dict:
    with zipfile.ZipFile(io.BytesIO(data) if isinstance(data, bytes) else data) as zf:
        return {i.filename: zf.read(i.filename) for i in zf.infolist() if not i.is_dir()}


def eocd_at(data: bytes) -> int:
    return data.rindex(b"PK\x05\x06")


def central_entries(data: bytes) -> list:
    """the positions of the central directory's entries"""
    at = eocd_at(data)
    total, _, cd_off = struct.unpack_from("<HII", data, at + 10)
    out, pos = [], cd_off
    for _ in range(total):
        out.append(pos)
        nlen, elen, clen = struct.unpack_from("<HHH", data, pos + 28)
        pos += 46 + nlen + elen + clen
    return out


def patched(data: bytes, pos: int, fmt: str, *values) -> bytes:
    b = bytearray(data)
    struct.pack_into(fmt, b, pos, *values)
    return bytes(b)


def longer_local_extra(data: bytes, extra: bytes = b"\xfe\xca\x06\x00pylinc") -> bytes:
    """the LAST member's local header gets an extra field the central directory does not state"""
    cd = central_entries(data)[-1]
    off = struct.unpack_from("<I", data, cd + 42)[0]
    nlen, elen = struct.unpack_from("<HH", data, off + 26)
    cut = off + 30 + nlen + elen
    out = bytearray(data[:cut] + extra + data[cut:])
    struct.pack_into("<H", out, off + 28, elen + len(extra))
    at = eocd_at(bytes(out))
    struct.pack_into("<I", out, at + 16, struct.unpack_from("<I", out, at + 16)[0] + len(extra))
    return bytes(out)


def payloads():
    rng = np.random.default_rng(50)
    text = b"".join(b"slice %d position %.2f mm; " % (k, k * 1.25) for k in range(2500))
    ramp = (np.arange(12000, dtype=np.uint32) * 7 // 5 % 251).astype(np.uint8).tobytes()
    noisy = (rng.integers(0, 16, 10000) + np.linspace(0, 200, 10000)).astype(np.uint8).tobytes()
    return text, ramp, noisy, rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()


def same_as_stdlib(dev, data: bytes, **kw):
    want = stdlib_read(data)
    stack = zipstack.extract(data, device=dev, check=False, **kw)
    assert stack.status.cpu().tolist() == [0] * len(stack.members)
    assert stack.lengths.cpu().tolist() == [m.size for m in stack.members]
    assert all(o % 16 == 0 for o in stack.offsets)
    for k, m in enumerate(stack.members):
        assert to_np(stack.member(k)).tobytes() == want[m.name], m.name
    return stack, want


def check_archive_kinds(dev):
    text, ramp, noisy, rnd = payloads()
    D, S = zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED
    entries = [("level1.txt", text, D, 1), ("series/", b"", S, None), ("series/level6.bin", ramp, D, 6), ("level9.bin", noisy, D, 9),
               ("stored.bin", rnd, S, None), ("empty.bin", b"", S, None), ("noise_deflated.bin", rnd, D, 6),
               ("empty_deflated.bin", b"", D, 6)]
    data = make_zip(entries, comment=b"exported by the console, 2026-10-19; 64 slices")
    stack, want = same_as_stdlib(dev, data)
    assert [m.name for m in stack.members] == [e[0] for e in entries if not e[0].endswith("/")]
    assert {m.method for m in stack.members} == {0, 8} and 0 in [m.size for m in stack.members]
    # a path, a file object
    members = zipstack.read_zip(io.BytesIO(data))
    assert [(m.name, m.size, m.crc32) for m in members] == [(n, len(b), zlib.crc32(b)) for n, b in want.items()]
    # members= selects a subset, in the order given; verify=False
    stack, _ = same_as_stdlib(dev, data, members=["stored.bin", "level1.txt", members[1]], verify=False)
    assert [m.name for m in stack.members] == ["stored.bin", "level1.txt", "series/level6.bin"]
    with pytest.raises(KeyError, match="no item named 'absent'"):
        zipstack.extract(data, members=["absent"], device=dev)
    # written to a stream that cannot seek: data descriptors, sizes and CRC from the central directory
    piped = make_zip(entries[:5], pipe=True)
    stack, _ = same_as_stdlib(dev, piped)
    assert all(m.flags & 8 for m in stack.members)
    # a local header whose extra field is longer than the central one (by hand, and as force_zip64 writes it)
    longer = longer_local_extra(make_zip(entries[:4]))
    stack, _ = same_as_stdlib(dev, longer)
    last = stack.members[-1]
    assert last.data_offset - last.header_offset == 30 + len(last.name) + 10
    sink = io.BytesIO()
    with zipfile.ZipFile(sink, "w", zipfile.ZIP_DEFLATED) as zf:
        with zf.open("forced.bin", "w", force_zip64=True) as f:                    # a ZIP64 extra field in the LOCAL header only:
            f.write(ramp)                                                          # the central directory holds the true sizes
    stack, _ = same_as_stdlib(dev, sink.getvalue())
    assert stack.members[0].data_offset - stack.members[0].header_offset > 30 + len("forced.bin")


NINE_SIZES = [6, 15, 34, 61, 68, 69, 92, 97, 126]


def check_nine_members_every_residue(dev, tmp_path):
    """nine members laid side by side at the kernel entry: output offsets and sizes of every residue mod 16"""
    rng = np.random.default_rng(51)
    text = payloads()[0]
    entries = []
    for k, n in enumerate(NINE_SIZES):
        body = text[k * 50:k * 50 + n] if k % 3 else rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        entries.append((f"m{k}", body, zipfile.ZIP_STORED if k % 3 == 0 else zipfile.ZIP_DEFLATED, 9))
    data = make_zip(entries)
    want = stdlib_read(data)
    members = zipstack.read_zip(data)
    assert {m.method for m in members} == {0, 8}
    sizes = np.array(NINE_SIZES, dtype=np.int64)
    offs = np.concatenate([[3], 3 + np.cumsum(sizes)[:-1]])
    assert {int(v) % 16 for v in offs} | {int(v) % 16 for v in sizes} == set(range(16))
    out = torch.full((int(offs[-1] + sizes[-1]) + 5,), 0x5A, dtype=torch.uint8, device=dev)
    buf = np.frombuffer(data, dtype=np.uint8)
    out, out_len, status = zipstack.extract_members(buf, [m.data_offset for m in members], [m.compressed_size for m in members],
                                                    [m.method for m in members], [m.crc32 for m in members], offs, sizes,
                                                    device=dev, out=out)
    flat = to_np(out)
    assert status.cpu().tolist() == [0] * 9 and out_len.cpu().tolist() == NINE_SIZES
    assert flat[3:-5].tobytes() == b"".join(want[f"m{k}"] for k in range(9)) and (flat[:3] == 0x5A).all() and (flat[-5:] == 0x5A).all()
    # ... and from a path, through extract
    path = tmp_path / "nine.zip"
    path.write_bytes(data)
    stack, _ = same_as_stdlib(dev, path)
    assert stack.name == str(path)


# ---- damage ---------------------------------------------------------------------------------------------------------------
def check_damage(dev, monkeypatch):
    text, ramp, noisy, rnd = payloads()
    D, S = zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED
    entries = [("a.txt", text[:6000], D, 6), ("stored.bin", rnd, S, None), ("b.bin", ramp[:5000], D, 6), ("c.bin", noisy[:4000], D, 9)]
    good = make_zip(entries)
    want = stdlib_read(good)
    members = zipstack.read_zip(good)
    by = {m.name: m for m in members}

    def statuses(data, damaged=None, **kw):
        stack = zipstack.extract(data, device=dev, check=False, **kw)
        st = stack.status.cpu().tolist()
        for k, m in enumerate(stack.members):
            if not st[k] and m.name != damaged:
                assert to_np(stack.member(k)).tobytes() == want[m.name], m.name     # the others stay equal
        return st

    # one flipped byte in a stored member's data
    flipped = patched(good, by["stored.bin"].data_offset + 77, "<B", good[by["stored.bin"].data_offset + 77] ^ 0x10)
    assert statuses(flipped) == [0, 8, 0, 0] and statuses(flipped, damaged="stored.bin", verify=False) == [0, 0, 0, 0]
    with pytest.raises(zipfile.BadZipFile, match="Bad CRC-32 for file 'stored.bin'"):
        zipstack.extract(flipped, device=dev)
    with pytest.raises(zipfile.BadZipFile, match="Bad CRC-32 for file 'stored.bin'"):
        zipfile.ZipFile(io.BytesIO(flipped)).read("stored.bin")                    # the stdlib's words
    # a flipped bit in a deflated member's central CRC field
    cd = central_entries(good)
    crc_bit = patched(good, cd[2] + 16, "<I", by["b.bin"].crc32 ^ 0x00400000)
    assert statuses(crc_bit) == [0, 0, 8, 0] and statuses(crc_bit, verify=False) == [0, 0, 0, 0]
    with pytest.raises(zipfile.BadZipFile, match="Bad CRC-32 for file 'b.bin'"):
        zipstack.extract(crc_bit, device=dev)
    # a corrupted Deflate block type (3), a compressed_size cut short
    at = by["c.bin"].data_offset
    assert (good[at] >> 1) & 3 == 2
    assert statuses(patched(good, at, "<B", good[at] | 6)) == [0, 0, 0, 4]
    short = patched(good, cd[0] + 20, "<I", by["a.txt"].compressed_size // 2)
    assert statuses(short) == [2, 0, 0, 0]
    for data, text_ in ((patched(good, at, "<B", good[at] | 6), "member 'c.bin': corrupt Deflate"), (short, "member 'a.txt': the Deflate stream ends")):
        with pytest.raises(zipfile.BadZipFile, match=text_):
            zipstack.extract(data, device=dev)
    # descriptors at the kernel entry: windows outside the buffers, a method, a stored member of two sizes
    buf = np.frombuffer(good, dtype=np.uint8)
    base = dict(in_off=[m.data_offset for m in members], in_len=[m.compressed_size for m in members], method=[m.method for m in members],
                crc_expected=[m.crc32 for m in members], out_size=[m.size for m in members])
    room = [(m.size + 15) & ~15 for m in members]
    base["out_off"] = [sum(room[:k]) for k in range(4)]
    for key, k, value in (("in_off", 0, len(buf) - 10), ("in_off", 2, -1), ("in_len", 3, 1 << 40), ("out_off", 1, sum(room)),
                          ("out_off", 0, -16), ("out_size", 2, sum(room) + 1), ("method", 3, 12), ("in_len", 1, len(rnd) - 1)):
        args = {a: list(b) for a, b in base.items()}
        args[key][k] = value
        out = torch.full((sum(room),), 0x5A, dtype=torch.uint8, device=dev)
        out, out_len, status = zipstack.extract_members(buf, device=dev, out=out, **args)
        st, flat = status.cpu().tolist(), to_np(out)
        assert st == [int(j == k) for j in range(4)], (key, k, st)
        assert out_len.cpu().tolist()[k] == 0
        for j, m in enumerate(members):
            got = flat[base["out_off"][j]:base["out_off"][j] + room[j]]
            if j == k:
                assert (got == 0x5A).all(), (key, k)                                # that member's output keeps its sentinel
            else:
                assert got[:m.size].tobytes() == want[m.name] and (got[m.size:] == 0x5A).all(), (key, k, j)
    # check=False transfers nothing back; check=True the status, and nothing else
    calls = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *x, **k: (calls.append(self.data_ptr()), real(self, *x, **k))[1])
    zipstack.extract(flipped, device=dev, check=False)
    assert not calls
    stack = zipstack.extract(good, device=dev)
    assert set(calls) == {stack.status.data_ptr()}
    monkeypatch.undo()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    text = payloads()[0][:3000]
    D = zipfile.ZIP_DEFLATED
    good = make_zip([("a.txt", text, D, 6), ("b.txt", text[::-1], D, 6)])
    cd = central_entries(good)
    at = eocd_at(good)
    off_b = struct.unpack_from("<I", good, cd[1] + 42)[0]
    locator = good[:at] + b"PK\x06\x07" + bytes(16) + good[at:]
    cases = [
        (make_zip([("a.txt", text, D, 6), ("b.bz2", text, zipfile.ZIP_BZIP2, None)]), r"member 'b.bz2': compression method 12 \(bzip2\)"),
        (make_zip([("b.xz", text, zipfile.ZIP_LZMA, None)]), r"member 'b.xz': compression method 14 \(LZMA\)"),
        (patched(good, cd[1] + 24, "<I", 0xFFFFFFFF), "member 'b.txt': ZIP64"),
        (patched(good, cd[1] + 20, "<I", 0xFFFFFFFF), "member 'b.txt': ZIP64"),
        (patched(good, cd[0] + 42, "<I", 0xFFFFFFFF), "member 'a.txt': ZIP64"),
        (patched(good, at + 10, "<H", 0xFFFF), "ZIP64 archives"),
        (patched(good, at + 16, "<I", 0xFFFFFFFF), "ZIP64 archives"),
        (locator, "ZIP64 archives"),
        (patched(good, at + 4, "<H", 1), "more than one disk"),
        (patched(good, at + 8, "<H", 1), "more than one disk"),
        (patched(good, cd[1] + 34, "<H", 2), "member 'b.txt': it starts on disk 2"),
        (patched(good, cd[1] + 8, "<H", struct.unpack_from("<H", good, cd[1] + 8)[0] | 1), "member 'b.txt': encrypted"),
        (patched(good, cd[0] + 10, "<H", 9), r"member 'a.txt': compression method 9 \(Deflate64\)"),
        (good[:at] + good[at + 1:], "no End Of Central Directory"),
        (good[:at + 10], "no End Of Central Directory"),
        (b"", "no End Of Central Directory"),
        (patched(good, at + 16, "<I", at + 1), "central directory .* lies outside the file"),
        (patched(good, at + 12, "<I", at + 1), "central directory .* lies outside the file"),
        (patched(good, cd[1], "<I", 0x04034B50), "entry 1 of the central directory"),
        (patched(good, cd[1] + 42, "<I", len(good) - 10), "member 'b.txt': its local header .* lies outside the file"),
        (patched(good, off_b, "<I", 0x02014B50), "member 'b.txt': its local header .* wrong signature"),
        (patched(good, cd[1] + 20, "<I", len(good)), "member 'b.txt': its data .* lie outside the file"),
    ]
    for data, text_ in cases:
        with pytest.raises(ValueError, match="ZIP archive: .*" + text_):
            zipstack.read_zip(data)
        with pytest.raises(ValueError, match=text_):
            zipstack.extract(data, device=dev)
    assert [m.name for m in zipstack.read_zip(good)] == ["a.txt", "b.txt"]
    m = zipstack.read_zip(good)[1]
    assert (m.method, m.flags & 1, m.size, m.header_offset, m.data_offset) == (8, 0, 3000, off_b, off_b + 30 + 5)


# ---- dicom.load_zip -------------------------------------------------------------------------------------------------------
def ds(tag: int, value: str) -> bytes:
    return rle._el(0x0028, tag, "DS", value.encode())


def dicom_zip(files, kinds=None, extra_members=()) -> bytes:
    """files: [(name, bytes)]; kinds: per file ZIP_STORED / ZIP_DEFLATED (default: deflated, level 6)"""
    entries = list(extra_members[:1])
    for k, (name, data) in enumerate(files):
        entries.append((name, data, (kinds or [zipfile.ZIP_DEFLATED] * len(files))[k], 6))
    return make_zip(entries + list(extra_members[1:]))


def reference_keywords(kw: dict) -> dict:
    return {k: v for k, v in kw.items() if k not in ("members", "verify")}


def same_refusal(dev, data: bytes, **kw):
    """what load_frames refuses for the stdlib-extracted bytes, load_zip refuses in the same words"""
    from pylinac_amd._lib import PylinacHipError

    with zipfile.ZipFile(io.BytesIO(data)) as zf:
        blobs = [zf.read(i.filename) for i in zf.infolist() if i.filename.endswith(".dcm")]
    with pytest.raises(PylinacHipError) as want:
        dicom.load_frames(blobs, device=dev, **reference_keywords(kw))
    with pytest.raises(PylinacHipError, match=re.escape(str(want.value))):
        dicom.load_zip(data, device=dev, **kw)


def same_as_load_frames(dev, data: bytes, frames: np.ndarray | None, names=None, **kw):
    """load_zip == load_frames on what the stdlib extracts (torch.equal), and == `frames` where given"""
    x, metas, got_names = dicom.load_zip(data, device=dev, **kw)
    with zipfile.ZipFile(io.BytesIO(data)) as zf:
        want, want_metas = dicom.load_frames([zf.read(n) for n in got_names], device=dev, **reference_keywords(kw))
    assert x.dtype == want.dtype and x.shape == want.shape and torch.equal(x, want)
    assert [m._values for m in metas] == [m._values for m in want_metas]
    if names is not None:
        assert got_names == names
    if frames is not None:
        assert np.array_equal(to_np(x), frames)
    return x, metas, got_names


EVEN = (30, 35)     # frames of 2100 bytes: pl_dicom_decode stores the container form of a BATCH only when frame bytes % 4 == 0


def check_load_zip_native(dev):
    """four uint16 native files of 29 x 35.  load_frames -- the reference here -- decodes such a batch as float64 and refuses
    its container form (frames of 2030 bytes, see dicom_rle_checks.check_container_loader): load_zip must answer alike in both,
    and the container form is compared on frames of 30 x 35"""
    frames = rle.container_frames(np.uint16)
    assert frames.shape == (4, 29, 35)
    files = [(f"CT/slice{k}.dcm", rle.native_file(frames[k:k + 1])) for k in range(4)]
    readme = ("README.txt", b"exported " * 40, zipfile.ZIP_DEFLATED, 6)
    folder = ("CT/", b"", zipfile.ZIP_STORED, None)
    data = dicom_zip(files, extra_members=(readme, folder))
    assert "README.txt" in stdlib_read(data)
    x, metas, names = same_as_load_frames(dev, data, frames.astype(np.float64), names=[f[0] for f in files], dtype=np.float64)
    assert x.dtype == torch.float64 and metas[0].Rows == 29 and "README.txt" not in names
    same_as_load_frames(dev, data, frames.astype(np.float32), raw_pixels=True, dtype=np.float32)
    same_refusal(dev, data)
    same_refusal(dev, data, raw_pixels=True)
    for k in range(4):                                                             # one member at a time: the container form
        same_as_load_frames(dev, data, frames[k:k + 1], members=[files[k][0]])
    # the container form of a batch; stored and deflated members mixed; members= in the order wanted
    even = rle.container_frames(np.uint16, shape=EVEN)
    files = [(f"CT/slice{k}.dcm", rle.native_file(even[k:k + 1])) for k in range(4)]
    x, _, names = same_as_load_frames(dev, dicom_zip(files, extra_members=(readme, folder)), even, names=[f[0] for f in files])
    assert x.dtype == torch.uint16
    mixed = dicom_zip(files, kinds=[zipfile.ZIP_STORED, zipfile.ZIP_DEFLATED, zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED])
    assert sorted({m.method for m in zipstack.read_zip(mixed)}) == [0, 8]
    same_as_load_frames(dev, mixed, even)
    pick = [files[2][0], files[0][0]]
    same_as_load_frames(dev, mixed, even[[2, 0]], names=pick, members=pick)
    # dtype and raw_pixels
    same_as_load_frames(dev, mixed, even.astype(np.float64), dtype=np.float64)
    same_as_load_frames(dev, mixed, even, raw_pixels=True)
    same_as_load_frames(dev, mixed, even.astype(np.int32), raw_pixels=True, dtype=np.int32)
    with pytest.raises(ValueError, match="member 'README.txt': not a DICOM Part-10 file"):
        dicom.load_zip(data, members=["README.txt"], device=dev)
    with pytest.raises(ValueError, match="no DICOM members"):
        dicom.load_zip(make_zip([readme]), device=dev)


def check_load_zip_rescale(dev):
    frames = rle.container_frames(np.int16)                                         # 29 x 35: the float64 forms
    assert (frames < 0).any()
    shared = ds(0x1052, "-1024") + ds(0x1053, "1.5")
    files = [(f"s{k}.dcm", rle.native_file(frames[k:k + 1], extra=shared)) for k in range(4)]
    x, _, _ = same_as_load_frames(dev, dicom_zip(files), frames.astype(np.float64) * 1.5 + -1024)     # the fused float64 form
    assert x.dtype == torch.float64
    same_as_load_frames(dev, dicom_zip(files), frames.astype(np.float64) * 1.5 + -1024, dtype=np.float64)
    even = rle.container_frames(np.int16, shape=EVEN)
    files = [(f"s{k}.dcm", rle.native_file(even[k:k + 1], extra=shared)) for k in range(4)]
    same_as_load_frames(dev, dicom_zip(files), even, raw_pixels=True)
    own = [(f"s{k}.dcm", rle.native_file(even[k:k + 1], extra=ds(0x1052, str(-1000 - k)) + ds(0x1053, str(1 + k)))) for k in range(4)]
    want = np.stack([even[k].astype(np.float64) * (1 + k) + (-1000 - k) for k in range(4)])
    same_as_load_frames(dev, dicom_zip(own, kinds=[zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED] * 2), want)   # per-file rescale
    # a multi-frame member between single-frame ones
    multi = [("a.dcm", rle.native_file(even[:1])), ("b.dcm", rle.native_file(even[1:4])), ("c.dcm", rle.native_file(even[:1]))]
    x, metas, _ = same_as_load_frames(dev, dicom_zip(multi), np.concatenate([even[:1], even[1:4], even[:1]]))
    assert metas[1].NumberOfFrames == 3 and x.shape[0] == 5


def check_load_zip_long_header(dev):
    """a 150 KiB private element in front of Pixel Data: the 64 KiB prefix doubles twice"""
    rng = np.random.default_rng(52)
    frames = rle.container_frames(np.uint16, n=2, shape=EVEN)
    private = rle._el(0x0029, 0x1010, "OB", rng.integers(0, 256, 150 * 1024, dtype=np.uint8).tobytes())
    files = [("long.dcm", rle.native_file(frames[:1], extra=private)), ("plain.dcm", rle.native_file(frames[1:2]))]
    data = dicom_zip(files)
    seen = []
    real = dicom._walk_part10
    try:
        dicom._walk_part10 = lambda buf, size=None: (seen.append(len(buf)), real(buf, size))[1]
        x, metas, names = dicom.load_zip(data, device=dev)
    finally:
        dicom._walk_part10 = real
    assert seen[:3] == [65536, 131072, len(files[0][1])] and len(files[0][1]) < 262144, seen
    assert metas[0].PixelData[0] > 150 * 1024 and np.array_equal(to_np(x), frames)
    same_as_load_frames(dev, data, frames)
    same_as_load_frames(dev, dicom_zip(files, kinds=[zipfile.ZIP_STORED] * 2), frames)


def check_load_zip_refusals(dev):
    frames = rle.container_frames(np.uint16, shape=EVEN)
    native = [(f"s{k}.dcm", rle.native_file(frames[k:k + 1])) for k in range(2)]
    with pytest.raises(NotImplementedError, match="member 'r.dcm': RLE Lossless"):
        dicom.load_zip(dicom_zip(native + [("r.dcm", rle.rle_file(frames[2:3]))]), device=dev)
    with pytest.raises(NotImplementedError, match="member 'j.dcm': encapsulated"):
        dicom.load_zip(dicom_zip(native + [("j.dcm", rle.rle_file(frames[2:3], uid="1.2.840.10008.1.2.4.70"))]), device=dev)
    with pytest.raises(ValueError, match="differ in pixel format or frame size"):
        dicom.load_zip(dicom_zip(native + [("w.dcm", rle.native_file(frames[2:3, :, :-1]))]), device=dev)
    cut = rle.native_file(frames[2:3])[:-70]
    with pytest.raises(ValueError, match="Pixel Data value .* lies outside the file"):
        dicom.load_zip(dicom_zip(native + [("cut.dcm", cut)]), device=dev)
    # a Pixel Data element that ends inside the frame it states: load_frames's refusal in its words, an integer dtype included
    short = rle._meta("1.2.840.10008.1.2.1") + rle.image_tags(frames[2:3]) + rle._el(0x7FE0, 0x0010, "OW", frames[2].tobytes()[:-70])
    for kw in ({}, dict(dtype=np.int32, raw_pixels=True)):
        with pytest.raises(ValueError, match=r"\(2030 bytes\) doesn't match the expected length \(2100 bytes\)") as want:
            dicom.load_frames([f for _, f in native] + [short], device=dev, **kw)
        with pytest.raises(ValueError) as got:
            dicom.load_zip(dicom_zip(native + [("short.dcm", short)]), device=dev, **kw)
        assert str(got.value) == str(want.value)
    # verify: a damaged pixel byte in a stored member
    data = dicom_zip(native, kinds=[zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED])
    m = zipstack.read_zip(data)[1]
    bad = patched(data, m.data_offset + m.size - 9, "<B", data[m.data_offset + m.size - 9] ^ 1)
    with pytest.raises(zipfile.BadZipFile, match="Bad CRC-32 for file 's1.dcm'"):
        dicom.load_zip(bad, device=dev)
    x, _, _ = dicom.load_zip(bad, device=dev, verify=False)
    got = to_np(x)
    assert np.array_equal(got[0], frames[0]) and (got[1] != frames[1]).sum() == 1
    # read_part10 for whole files is what it was
    meta, blob = dicom.read_part10(native[0][1])
    assert meta.PixelData == (len(native[0][1]) - frames[0].nbytes, frames[0].nbytes) and len(blob) == len(native[0][1])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def check_c_abi_argument_checks(dev):
    """pl_crc32 / pl_zip_extract: invalid argument (1) for every null pointer, n = 0, a misaligned d_bytes -- all before any
    launch (the pointers below are never dereferenced); the work sizes: -1 for the same"""
    from pylinac_amd import _lib

    lib = _lib.load()
    buf = torch.zeros(256, dtype=torch.uint8, device=dev)
    idx = torch.zeros(8, dtype=torch.int64, device=dev)
    st = torch.zeros(4, dtype=torch.int32, device=dev)
    p, q, s = buf.data_ptr(), idx.data_ptr(), st.data_ptr()

    def crc(**kw):
        a = dict(bytes_=p, nbytes=256, off=q, len_=q, n=1, max_len=64, crc=s, status=s, work=p)
        a.update(kw)
        return lib.pl_crc32(a["bytes_"], a["nbytes"], a["off"], a["len_"], a["n"], a["max_len"], a["crc"], a["status"], a["work"], None)

    for name in ("bytes_", "off", "len_", "crc", "status", "work"):
        assert crc(**{name: None}) == 1 and b"null pointer" in lib.pl_last_error(), name
    assert crc(n=0) == 1 and crc(n=-1) == 1 and crc(max_len=-1) == 1 and crc(nbytes=-1) == 1 and crc(max_len=65535 * TILE + 1) == 1
    assert crc(bytes_=p + 1) == 1 and b"4-byte" in lib.pl_last_error()
    assert lib.pl_crc32_work_bytes(0, 64) == -1 and lib.pl_crc32_work_bytes(1, -1) == -1
    assert lib.pl_crc32_work_bytes(3, 0) == 16 and lib.pl_crc32_work_bytes(3, 2 * TILE + 1) == 48 and lib.pl_crc32_work_bytes(1, TILE) == 16

    names = ("bytes_", "in_off", "in_len", "method", "expected", "out", "out_off", "out_size", "out_len", "status", "work")

    def ext(**kw):
        a = dict(bytes_=p, nbytes=256, in_off=q, in_len=q, method=s, expected=s, n=1, max_size=64, out=p, out_bytes=256, out_off=q,
                 out_size=q, verify=1, out_len=q, status=s, work=p)
        a.update(kw)
        return lib.pl_zip_extract(a["bytes_"], a["nbytes"], a["in_off"], a["in_len"], a["method"], a["expected"], a["n"], a["max_size"],
                                  a["out"], a["out_bytes"], a["out_off"], a["out_size"], a["verify"], a["out_len"], a["status"],
                                  a["work"], None)

    for name in names:
        assert ext(**{name: None}) == 1 and b"null pointer" in lib.pl_last_error(), name
    assert ext(n=0) == 1 and ext(n=-3) == 1 and ext(max_size=-1) == 1 and ext(verify=2) == 1 and ext(nbytes=-1) == 1 and ext(out_bytes=-1) == 1
    assert ext(bytes_=p + 2) == 1 and b"4-byte" in lib.pl_last_error()
    assert ext(out=p + 1) == 1 and ext(work=p + 4) == 1 and b"16-byte" in lib.pl_last_error()
    assert lib.pl_zip_work_bytes(0, 64) == -1 and lib.pl_zip_work_bytes(1, -1) == -1 and lib.pl_zip_work_bytes(1, 1 << 31) == -1
    assert lib.pl_zip_work_bytes(3, 2 * TILE + 1) == 3 * 32 + 48
    header = (Path(__file__).resolve().parent.parent / "include" / "pylinac_hip.h").read_text()
    for entry in (r"int pl_crc32\(", r"int64_t pl_crc32_work_bytes\(", r"int pl_zip_extract\(", r"int64_t pl_zip_work_bytes\("):
        assert re.search(entry, header), entry
    assert lib.pl_abi_version() == 3
