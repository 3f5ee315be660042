"""Shared checks of the device's tier 2 of JPEG 2000 (``dicom.plan_jpeg2000_blocks`` / pl_dicom_j2k_plan) and of
``dicom.load_zip(encapsulated=True, jpeg2000=True)`` on top of it -- tests/test_emulated_dicom_zip_j2k.py on the CPU emulator,
tests/test_gpu_dicom_zip_j2k.py on the MI355X.  Every comparison is EQUALITY.

The reference of the plan kernel is the host's packet-header parse, ``dicom._j2k_codestream``, which ``load_frames`` keeps: the
rows the kernel writes at the front of a frame's range are the host's list, row for row, shifted by the stream's place in the
buffer.  The reference of the loader is ``load_frames(..., jpeg2000=True)`` on the bytes ``zipfile`` extracts -- the same
tensor, metadata and exception, the member named where ``load_frames`` says ``file K`` -- and the source frames.  The streams
are Pillow's (tests/dicom_j2k_checks.py), the archives tests/zip_checks.py's.  What Pillow's encoder never writes -- status 8
(more than 30 bit planes), a header that ends in FF, empty bands, blocks excluded between included ones -- comes from the
test-side writer in tests/dicom_j2k_conformance_checks.py.  Without the feature the loader checks fail
(``load_zip`` has no ``jpeg2000`` keyword) and so do the plan checks (the library has no such symbol)."""
from __future__ import annotations

import re
import struct
import zipfile

import numpy as np
import pytest
import torch

import dicom_j2k_checks as jk
import dicom_rle_checks as rle
import dicom_zip_encap_checks as ze
import zip_checks as zc
from pylinac_amd import dicom

to_np = dicom._to_numpy
ARCHIVE = ze.ARCHIVE
SENTINEL = -0x5A5A5A5A5A5A5A5B


# ---- A: the plan kernel against the host parser ---------------------------------------------------------------------------
def headers(data: bytes, shape, bits: int):
    """what the host reads of a stream's headers -> (first packet, tile-part end, Psot, the coding parameters, the geometry)"""
    mv = memoryview(data)
    sot, levels, _, _, guard, exps, (xcb, ycb), precincts = dicom._j2k_main_header(mv, len(mv), *shape, bits, "stream")
    first, end, psot = dicom._j2k_tile_header(mv, len(mv), sot, "stream")
    geometry = list(dicom._j2k_geometry(*shape, levels, xcb, ycb, precincts, exps, "stream"))
    return first, end, psot, (levels, xcb, ycb, guard, exps, precincts), geometry


def laid_out(streams, gap: int = 3):
    """the streams in one buffer, `gap` bytes of 0xEE in front of each (odd places) -> (the buffer, where each starts)"""
    buf, starts = bytearray(), []
    for s in streams:
        buf += b"\xee" * gap
        starts.append(len(buf))
        buf += s
    return np.frombuffer(bytes(buf) + b"\xee" * gap, dtype=np.uint8), starts


def plan_rows(streams, starts, shape, bits: int, edit=None):
    """-> (plan, tables, the rows each frame owns, max_nodes); ``edit(k, fields)`` may change frame k's fields before packing"""
    plan, tables, owned, row0, most = [], [], [], 0, 1
    for k, (s, at) in enumerate(zip(streams, starts)):
        first, end, psot, coding, geometry = headers(s, shape, bits)
        nrows, nodes = dicom._j2k_block_counts(geometry)
        fields = dict(start=at, length=len(s), first=first, end=end if psot else 0, row0=row0, nrows=nrows)
        if edit is not None:
            edit(k, fields)
        row, table = dicom._j2k_plan_row(fields["start"], fields["length"], fields["first"], fields["end"], *coding, fields["row0"],
                                         fields["nrows"])
        plan.append(row)
        tables.append(table)
        owned.append((row0, nrows))
        row0, most = row0 + nrows, max(most, nodes)
    return np.asarray(plan, dtype=np.int64), np.stack(tables), owned, most


def host_rows(data: bytes, shape, bits: int, frame: int, at: int) -> np.ndarray:
    blocks = dicom._j2k_codestream(np.frombuffer(data, np.uint8), *shape, bits, "stream")[3]
    return np.asarray([(frame, at + off, *rest) for off, *rest in blocks], dtype=np.int64).reshape(-1, 10)


def header_ff_bytes(data: bytes, shape, bits: int) -> int:
    """the FF bytes inside the packet headers: the tile-part's bytes from the first packet on that belong to no segment"""
    first, end, _, _, _ = headers(data, shape, bits)
    body = np.zeros(len(data), dtype=bool)
    for off, ln, *_ in dicom._j2k_codestream(np.frombuffer(data, np.uint8), *shape, bits, "stream")[3]:
        body[off:off + ln] = True
    inside = np.frombuffer(data, np.uint8)[first:end]
    return int(((inside == 0xFF) & ~body[first:end]).sum())


def assert_plan_equals_host(dev, streams, shape, bits: int = 16) -> set:
    """ONE plan call over all the streams == the host's rows per stream -> the pass counts met"""
    buf, starts = laid_out(streams)
    plan, tables, owned, nodes = plan_rows(streams, starts, shape, bits)
    blocks, info = dicom.plan_jpeg2000_blocks(buf, plan, tables, *shape, nodes, device=dev)
    assert blocks.is_cuda and info.is_cuda and blocks.dtype == torch.int64 and info.dtype == torch.int32
    blocks, info, passes = to_np(blocks), to_np(info), set()
    assert blocks.shape == (sum(n for _, n in owned), 10) and info.shape == (len(streams), 4)
    for k, (s, at) in enumerate(zip(streams, starts)):
        want = host_rows(s, shape, bits, k, at)
        row0, nrows = owned[k]
        assert len(want) <= nrows
        assert info[k].tolist() == [0, len(want), 0, 0], (k, info[k])
        assert np.array_equal(blocks[row0:row0 + len(want)], want), k
        assert (blocks[row0 + len(want):row0 + nrows, 0] == -1).all(), k
        passes |= set(want[:, 3].tolist())
    return passes


def noise_stream(seed, shape, dtype, **kw):
    return jk.stream(jk.noise(np.random.default_rng(seed), shape, dtype), **kw)


def check_plan_geometry(dev, block):
    """129 x 67 full-range uint16 noise x levels {0, 2, 5} with ``block``; without levels 4 x 4 blocks give 17 x 33 leaves (a
    tag tree seven levels deep; 17 x 9 and six at the two-level stream's top resolution); every such stream has FF bytes
    inside its packet headers"""
    shape, passes = (129, 67), set()
    streams = [noise_stream(100 + levels + block[0], shape, np.uint16, codeblock_size=block, num_resolutions=levels + 1) for levels in jk.LEVELS]
    for s, levels in zip(streams, jk.LEVELS):
        assert jk.cod_levels(s) == levels
        assert header_ff_bytes(s, shape, 16) >= 1
    if block == (4, 4):
        geometry = headers(streams[0], shape, 16)[4]
        assert dicom._j2k_block_counts(geometry) == (33 * 17, dicom._j2k_tree_nodes(17, 33)) and dicom._j2k_tree_nodes(17, 33) > 33 * 17 + 9 * 17
    passes |= assert_plan_equals_host(dev, streams, shape)
    assert any(p >= 37 for p in passes)                                            # the longest codeword of Table B.4
    return passes


def check_plan_shapes(dev):
    for shape in [(1, 1), (1, 9), (9, 1), (5, 7), (33, 65)]:
        for dtype in (np.uint8, np.uint16):
            streams = []
            for levels in jk.allowed_levels(shape):
                kw = {} if levels is None else {"num_resolutions": levels + 1}
                streams.append(noise_stream(shape[0] * 7 + shape[1], shape, dtype, **kw))
            assert_plan_equals_host(dev, streams, shape, 8 * np.dtype(dtype).itemsize)


def check_plan_oblong_and_orders(dev):
    for block in jk.OBLONG_BLOCKS:
        assert_plan_equals_host(dev, [noise_stream(12, (33, 65), np.uint16, codeblock_size=block, num_resolutions=3)], (33, 65))
    streams = [noise_stream(11, (33, 65), np.uint8, progression=name, num_resolutions=4) for name in jk.PROGRESSIONS]
    assert {s[jk.segments(s)[0xFF52] + 4 + 1] for s in streams} == {0, 1, 2, 3, 4}
    assert_plan_equals_host(dev, streams, (33, 65), 8)


def check_plan_contents(dev) -> set:
    """a constant frame (every block above LL excluded or every packet empty), low-amplitude uint8 (short codewords of Table
    B.4), signed streams, stated precincts that leave one precinct per resolution, Psot = 0 with and without the pad byte"""
    passes = set()
    for dtype in (np.uint8, np.uint16):
        constant = jk.stream(jk.content("constant", (33, 65), dtype))
        assert dicom._j2k_codestream(np.frombuffer(constant, np.uint8), 33, 65, 16, "constant")[3] == []
        off_middle = jk.stream(jk.content("constant, off the middle", (33, 65), dtype))
        passes |= assert_plan_equals_host(dev, [constant, off_middle], (33, 65), 16)
    # zero-length packets (first bit 0): the one-byte packets 80 of the constant stream's upper resolutions patched to 00;
    # Pillow decodes the patched stream to the source
    frame = jk.content("constant", (33, 65), np.uint16)
    constant = jk.stream(frame)
    first = headers(constant, (33, 65), 16)[0]
    assert constant[first:] == b"\x80" * 6 + b"\xff\xd9"
    empty = constant
    for at in range(first + 1, first + 6):
        empty = jk.patched(empty, at, 0)
    assert np.array_equal(jk.pil_decode(empty), frame)
    passes |= assert_plan_equals_host(dev, [empty], (33, 65))
    rng = np.random.default_rng(21)
    low = [jk.stream(rng.integers(0, 3, (129, 67)).astype(np.uint8), codeblock_size=(4, 4), num_resolutions=n) for n in (1, 3, 6)]
    passes |= assert_plan_equals_host(dev, low, (129, 67), 8)
    signed = [jk.signed_stream(f) for f in jk.stack(np.int16, n=2, shape=(33, 65))]
    assert signed[0][42] == 0x8F
    passes |= assert_plan_equals_host(dev, signed, (33, 65))
    small = jk.stack(np.uint16, n=1, shape=(16, 16))
    one_precinct = jk.stream(small[0], precinct_size=(32, 32))
    assert one_precinct[jk.segments(one_precinct)[0xFF52] + 4] & 1                  # Scod bit 0: the precincts are stated
    assert headers(one_precinct, (16, 16), 16)[3][5] is not None
    passes |= assert_plan_equals_host(dev, [one_precinct], (16, 16))
    good = noise_stream(13, (33, 65), np.uint16)
    open_ended = jk.with_psot(good, 0)
    padded = open_ended + b"\x00"                                                   # an item's pad byte behind EOC
    for data in (open_ended, padded):
        assert headers(data, (33, 65), 16)[2] == 0 and headers(data, (33, 65), 16)[1] == len(open_ended) - 2
    passes |= assert_plan_equals_host(dev, [good, open_ended, padded, open_ended[:-2]], (33, 65))
    plt = noise_stream(13, (33, 65), np.uint16, plt=True)
    passes |= assert_plan_equals_host(dev, [plt, jk.with_psot(plt, 0)], (33, 65))
    return passes


def check_pass_classes(passes: set):
    """the union over the streams above falls into all four codeword classes a lossless one-layer stream can use"""
    assert 1 in passes and 4 in passes and any(7 <= p <= 34 for p in passes) and any(p >= 37 for p in passes), sorted(passes)
    assert 2 not in passes and all(p % 3 == 1 for p in passes)


# ---- B: the archive path ----------------------------------------------------------------------------------------------------
def same(dev, data: bytes, frames, names=None, **kw):
    """load_zip(encapsulated=True, jpeg2000=True) == load_frames(jpeg2000=True) on what the stdlib extracts, and == ``frames``"""
    x, metas, got = dicom.load_zip(data, device=dev, encapsulated=True, jpeg2000=True, **kw)
    want, want_metas = dicom.load_frames(ze.extracted(data, got), device=dev, jpeg2000=True, **zc.reference_keywords(kw))
    assert x.dtype == want.dtype and x.shape == want.shape and torch.equal(x, want)
    assert [m._values for m in metas] == [m._values for m in want_metas]
    for m in metas:
        assert m.PixelData[1] == -1 and all(isinstance(v, int) for frag in m.PixelDataFragments for v in frag)
        assert isinstance(m.PixelDataOffsetTable, list)
    if names is not None:
        assert got == names
    if frames is not None:
        assert np.array_equal(to_np(x), frames)
    return x, metas, got


def same_error(dev, data: bytes, member: str, **kw):
    """the exception load_frames raises for the extracted bytes, its type and text, behind ``ARCHIVE: member 'NAME'``"""
    with pytest.raises((ValueError, NotImplementedError)) as want:
        dicom.load_frames(ze.extracted(data), device=dev, jpeg2000=True, **zc.reference_keywords(kw))
    with pytest.raises((ValueError, NotImplementedError)) as got:
        dicom.load_zip(data, device=dev, encapsulated=True, jpeg2000=True, **kw)
    assert type(got.value) is type(want.value)
    text, who = str(want.value), f"{ARCHIVE}: member {member!r}"
    assert re.search(r"file \d+", text), text
    assert str(got.value) == re.sub(r"file \d+", lambda _: who, text)
    return str(got.value)


ODD = (29, 35)


def check_members(dev, full: bool = True):
    """deflated and stored members, several members, ``members=`` in another order, both UIDs, multi-frame members with an
    empty and a filled table (``full`` False: the first archive only, for the emulator)"""
    frames = jk.stack(np.uint16, n=4, shape=ODD)
    files = ze.one_each(frames, lambda f, k: jk.j2k_file(f, uid=jk.UIDS[k % 2], num_resolutions=1 + k))
    kinds = [zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED, zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED]
    with ze.counted("copy_ranges") as copies, ze.counted("_fetch_stream_head") as fetches, ze.counted("plan_jpeg2000_blocks") as plans:
        x, metas, _ = same(dev, zc.dicom_zip(files[:2] if not full else files, kinds=kinds), frames[:2] if not full else frames,
                           names=[f[0] for f in (files if full else files[:2])])
    assert not copies and not fetches and len(plans) == 1                          # one fragment per frame: planned in place
    assert [m.TransferSyntaxUID for m in metas] == [jk.UIDS[k % 2] for k in range(len(metas))] and x.dtype == torch.uint16
    if not full:
        return
    data = zc.dicom_zip(files, kinds=kinds)
    pick = [files[2][0], files[0][0]]
    same(dev, data, frames[[2, 0]], names=pick, members=pick)
    for table in ("empty", "filled"):
        multi = [("a.dcm", jk.j2k_file(frames[:1])), ("b.dcm", jk.j2k_file(frames[1:3], table=table)), ("c.dcm", jk.j2k_file(frames[3:]))]
        _, metas, _ = same(dev, zc.dicom_zip(multi), frames)
        assert len(metas[1].PixelDataOffsetTable) == (2 if table == "filled" else 0) and len(metas[1].PixelDataFragments) == 2


def check_spanning(dev):
    """three fragments a frame (the staging copy, ONE call), and an archive of both kinds of frame (one plan and one decode per
    buffer, the frames in their order)"""
    frames = jk.stack(np.uint16, n=4, shape=ODD)
    alone = jk.j2k_file(frames[:1], split=3)
    assert len(dicom.read_part10(alone, jpeg2000=True)[0].PixelDataFragments) == 3
    with ze.counted("copy_ranges") as copies, ze.counted("plan_jpeg2000_blocks") as plans:
        same(dev, zc.dicom_zip([("x.dcm", alone)]), frames[:1])
    assert len(copies) == 1 and len(copies[0][2]) == 3 and len(plans) == 1
    multi = jk.j2k_file(frames[1:3], split=3, table="filled")
    files = [("a.dcm", jk.j2k_file(frames[3:])), ("b.dcm", multi), ("c.dcm", jk.j2k_file(frames[:1], codeblock_size=(4, 4))), ("d.dcm", alone)]
    want = np.concatenate([frames[3:], frames[1:3], frames[:1], frames[:1]])
    with ze.counted("copy_ranges") as copies, ze.counted("plan_jpeg2000_blocks") as plans, ze.counted("decode_jpeg2000_frames") as decodes:
        same(dev, zc.dicom_zip(files, kinds=[zipfile.ZIP_DEFLATED, zipfile.ZIP_STORED] * 2), want)
    assert len(copies) == 1 and len(copies[0][2]) == 9 and len(plans) == 2
    assert len(decodes) == 2                                                       # (one per buffer; load_frames' own goes through its table)
    same(dev, zc.dicom_zip(files), want.astype(np.float64), dtype=np.float64)


def check_rescale_and_dtypes(dev):
    signed = jk.stack(np.int16, n=4, shape=ODD)
    shared = jk.ds(0x1052, "-1024") + jk.ds(0x1053, "1.5")
    files = ze.one_each(signed, lambda f, k: jk.j2k_file(f, extra=shared))
    data = zc.dicom_zip(files)
    x, _, _ = same(dev, data, signed.astype(np.float64) * 1.5 + -1024)
    assert x.dtype == torch.float64 and (signed < 0).any()
    x, _, _ = same(dev, data, signed, raw_pixels=True)
    assert x.dtype == torch.int16
    same(dev, data, signed.astype(np.float32), raw_pixels=True, dtype=np.float32)
    same(dev, data, None, dtype=np.float64)
    same(dev, data, None, invert_pixels=True)
    own = ze.one_each(signed, lambda f, k: jk.j2k_file(f, extra=jk.ds(0x1052, str(-1000 - k)) + jk.ds(0x1053, str(1 + k))))
    same(dev, zc.dicom_zip(own), np.stack([signed[k].astype(np.float64) * (1 + k) + (-1000 - k) for k in range(4)]))
    dirty = jk.stack(np.uint16, n=2)                                               # (jk.SMALL: frame bytes a multiple of four)
    assert (dirty >> 12).any()
    files = ze.one_each(dirty, lambda f, k: jk.j2k_file(f, extra=jk.bits_stored(12)))
    same(dev, zc.dicom_zip(files), dirty & 0x0FFF, correct_unused_bits=True)
    same(dev, zc.dicom_zip(files), dirty)


def check_long_headers(dev):
    """a COM segment of 300 bytes and one of 5 000 bytes in front of QCD: the main header runs past the head, and past the
    first 4 KiB fetch; PLT in the tile-part header"""
    frames = jk.stack(np.uint16, n=2, shape=ODD)
    plain = jk.frame_stream(frames[0])
    assert 100 < jk.segments(plain)[0xFF90] < dicom.ENCAP_HEAD_BYTES - 14
    for size, want in ((300, [4096]), (5000, [4096, 8192])):
        long = jk.inserted(plain, 0xFF64, b"\x00\x01" + b"c" * (size - 2))
        total = len(long) + len(long) % 2
        files = [("p.dcm", jk.j2k_file(frames[1:2])), ("h.dcm", jk.j2k_file(frames[:1], streams=[long]))]
        with ze.counted("_fetch_stream_head") as fetches:
            same(dev, zc.dicom_zip(files), frames[[1, 0]])
        assert [a[2] for a in fetches] == [min(w, total) for w in want], size
    with_plt = jk.stream(frames[0], plt=True)
    sot = jk.segments(with_plt)[0xFF90]
    assert with_plt[sot + 12:sot + 14] == b"\xff\x58"
    same(dev, zc.dicom_zip([("plt.dcm", jk.j2k_file(frames[:1], streams=[with_plt])),
                            ("open.dcm", jk.j2k_file(frames[:1], streams=[jk.with_psot(with_plt, 0)]))]), frames[[0, 0]])


def check_keyword_and_crc(dev):
    frames = jk.stack(np.uint16, n=2, shape=ODD)
    files = ze.one_each(frames, lambda f, k: jk.j2k_file(f))
    data = zc.dicom_zip(files)
    with pytest.raises(ValueError, match="jpeg2000=True extends encapsulated=True"):
        dicom.load_zip(data, device=dev, jpeg2000=True)
    for kw in (dict(), dict(encapsulated=True)):                                   # without the keyword: the refusal as it was
        with pytest.raises(NotImplementedError, match=jk.TODAY):
            dicom.load_zip(data, device=dev, **kw)
    member = zc.zipstack.read_zip(data)[1]
    assert member.name == files[1][0]
    broken = zc.patched(data, zc.central_entries(data)[1] + 16, "<I", member.crc32 ^ 0x00400000)   # the central directory's CRC field
    with pytest.raises(zipfile.BadZipFile, match=f"Bad CRC-32 for file {files[1][0]!r}"):
        dicom.load_zip(broken, device=dev, encapsulated=True, jpeg2000=True, verify=True)
    x, _, _ = dicom.load_zip(broken, device=dev, encapsulated=True, jpeg2000=True, verify=False)
    assert np.array_equal(to_np(x), frames)
    # the kinds do not mix, in load_frames' words
    mixed = zc.dicom_zip([files[0], ("n.dcm", rle.native_file(frames[1:]))])
    with pytest.raises(ValueError) as want:
        dicom.load_frames(ze.extracted(mixed), device=dev, jpeg2000=True)
    with pytest.raises(ValueError) as got:
        dicom.load_zip(mixed, device=dev, encapsulated=True, jpeg2000=True)
    assert str(got.value) == str(want.value) == dicom._MIXED_J2K


# ---- C: refusals and status -------------------------------------------------------------------------------------------------
def check_refusals_through_the_loader(dev):
    """every refusal of ``dicom_j2k_checks.check_refusals`` that concerns the stream, inside an archive member"""
    frames = jk.stack(np.uint16, n=1, shape=(33, 65))
    frame = frames[0]
    good = jk.stream(frame)
    seg = jk.segments(good)
    seen = []

    def refused(stream, fragment, of=frames):
        files = [("ok.dcm", jk.j2k_file(frames))] * (of.shape == frames.shape) + [("bad.dcm", jk.j2k_file(of, streams=[stream]))]
        text = same_error(dev, zc.dicom_zip(files), "bad.dcm")
        assert re.search(fragment, text), (fragment, text)
        seen.append(text)

    patched, inserted = jk.patched, jk.inserted
    refused(jk.stream(frame, quality_layers=[4, 2, 1], quality_mode="rates"), "COD with 3 quality layers")
    refused(jk.stream(frame, precinct_size=(32, 32)), "more than one precinct in a resolution")
    refused(jk.stream(frame, irreversible=True), "irreversible 9/7 transform")
    refused(jk.stream(frame, no_jp2=False), "JP2 file \\(box wrapper\\)")
    refused(jk.stream(np.dstack([frame.astype(np.uint8)] * 3)), "Csiz = 3")
    big = jk.stack(np.uint16, n=1, shape=(64, 64))
    files = [("bad.dcm", jk.j2k_file(big, streams=[jk.stream(big[0], tile_size=(32, 32))]))]
    assert "more than one tile" in same_error(dev, zc.dicom_zip(files), "bad.dcm")
    cod, siz = seg[0xFF52] + 4, seg[0xFF51] + 4
    refused(patched(good, cod + 8, 1), "code-block style 0x01")
    refused(patched(good, cod, 2), "SOP or EPH")
    refused(patched(good, cod, 4), "SOP or EPH")
    refused(patched(good, cod + 5, 17), "17 decomposition levels: at most J2K_MAX_LEVELS = 16")
    refused(patched(patched(good, cod + 6, 5), cod + 7, 3), "code blocks of 128 x 32")
    refused(patched(good, seg[0xFF5C] + 4, good[seg[0xFF5C] + 4] | 2), "quantisation style 2")
    refused(patched(good, siz + 37, 2), "subsampling XRsiz x YRsiz = 2 x 1")
    refused(patched(good, siz + 13, 1), "non-zero image or tile origin")
    refused(patched(good, 42, 16), "SIZ precision 17")
    for marker, size, what in ((0xFF53, 7, "COC"), (0xFF5F, 7, "POC"), (0xFF5D, 4, "QCC"), (0xFF5E, 3, "RGN"), (0xFF60, 3, "PPM")):
        refused(inserted(good, marker, bytes(size)), f"marker {marker:04X}, {what}")
    refused(good, "SIZ states Ysiz x Xsiz = 33 x 65 where Rows x Columns = 33 x 64", of=frames[:, :, :-1])
    refused(good[:seg[0xFF5C] + 6], "cut off|ends without SOT")
    refused(b"\xff\xd8" + good[2:], "does not start with SOC")
    refused(jk.with_psot(good, 13), "SOT states a tile-part of 13 bytes")
    # what only the device's walk of the packet headers finds
    noisy = jk.noise(np.random.default_rng(3), (1, 33, 65), np.uint16)
    data = jk.stream(noisy[0])
    sot = jk.segments(data)[0xFF90]
    sod = data.index(b"\xff\x93", sot) + 2
    for keep in (sod, sod + 1):
        refused(jk.with_psot(data[:keep], keep - sot), "the packet header of resolution 0 runs out of bytes", of=noisy)
    keep = len(data) * 6 // 10
    refused(jk.with_psot(data[:keep], keep - sot), "truncated code block|runs out of bytes", of=noisy)
    refused(jk.with_psot(data[:keep], 0), "truncated code block|runs out of bytes", of=noisy)
    refused(jk.stream(noisy[0], quality_layers=[8], quality_mode="rates"), "not a lossless JPEG 2000 stream: truncated code block", of=noisy)
    # a second tile-part behind the first: the marker lies beyond the head
    two = data[:-2] + b"\xff\x90" + bytes(10) + b"\xff\xd9"
    assert sot + struct.unpack_from(">I", data, sot + 6)[0] == len(data) - 2 > dicom.ENCAP_HEAD_BYTES
    refused(two, "a second SOT: more than one tile-part", of=noisy)
    assert len(set(seen)) >= 25, len(set(seen))                                    # (distinct refusals; two cuts share a text)
    # check=False raises the device's findings all the same, as load_frames does
    files = [("bad.dcm", jk.j2k_file(noisy, streams=[jk.with_psot(data[:keep], keep - sot)]))]
    with pytest.raises(ValueError, match="truncated code block|runs out of bytes"):
        dicom.load_zip(zc.dicom_zip(files), device=dev, encapsulated=True, jpeg2000=True, check=False)


def check_plan_status(dev):
    """status 2, 4, 16 and 1 through the kernel entry; a flagged frame between two good ones disturbs neither"""
    shape = (33, 65)
    frames = jk.noise(np.random.default_rng(31), (3,) + shape, np.uint16)
    streams = [jk.stream(f, num_resolutions=3, codeblock_size=(16, 16)) for f in frames]   # (several blocks a band: trees of 3 levels)
    buf, starts = laid_out(streams)
    first, end, psot, _, _ = headers(streams[1], shape, 16)
    rows1 = host_rows(streams[1], shape, 16, 1, 0)
    last = rows1[-1]

    def run(edit=None, data=None, fill=None):
        plan, tables, owned, nodes = plan_rows(streams, starts, shape, 16, edit)
        blocks = None if fill is None else torch.full((sum(n for _, n in owned), 10), fill, dtype=torch.int64, device=dev)
        blocks, info = dicom.plan_jpeg2000_blocks(buf if data is None else data, plan, tables, *shape, nodes, device=dev, blocks=blocks,
                                                  n_blocks=sum(n for _, n in owned))
        return blocks, to_np(info), owned

    def others_stand(blocks, info, owned):
        got = to_np(blocks)
        for k in (0, 2):
            want = host_rows(streams[k], shape, 16, k, starts[k])
            assert info[k].tolist() == [0, len(want), 0, 0] and np.array_equal(got[owned[k][0]:owned[k][0] + len(want)], want)
        assert (got[owned[1][0]:owned[1][0] + owned[1][1], 0] == -1).all()         # every row of the flagged frame

    # 2: the tile-part ends inside the packet header of a resolution (the header of resolution 0 begins at `first`)
    def cut(k, f):
        if k == 1:
            f["end"] = first + 1
    blocks, info, owned = run(cut)
    assert info[1].tolist() == [2, 0, 0, 0]
    others_stand(blocks, info, owned)
    res1 = int(rows1[np.flatnonzero(rows1[:, 5] != 0)[0] - 1][1] + rows1[np.flatnonzero(rows1[:, 5] != 0)[0] - 1][2])   # resolution 1's header

    def cut1(k, f):
        if k == 1:
            f["end"] = res1 + 1
    with pytest.raises(ValueError, match="the packet header of resolution 1 runs out of bytes"):     # (the host on the same cut)
        cut_at = res1 + 1
        sot = jk.segments(streams[1])[0xFF90]
        dicom._j2k_codestream(np.frombuffer(jk.with_psot(streams[1][:cut_at], cut_at - sot), np.uint8), *shape, 16, "s")
    blocks, info, owned = run(cut1)
    assert info[1].tolist() == [2, 0, 1, 0]
    others_stand(blocks, info, owned)
    # 16: the tile-part's end moved in front of the last segment's end
    def short(k, f):
        if k == 1:
            f["end"] = int(last[1] + last[2]) - 1
    blocks, info, owned = run(short)
    assert info[1].tolist() == [16, 0, 0, 0]
    others_stand(blocks, info, owned)
    # the frames of that call decode: the flagged one is left out, the others equal the source
    plan, tables, _, _ = plan_rows(streams, starts, shape, 16, short)
    params = np.asarray([(2, 16, 0, 0)] * 3, dtype=np.int32)
    x = dicom.decode_jpeg2000_frames(buf, blocks, params, *shape, 16, device=dev)
    assert to_np(x._pl_status).tolist() == [0, 0, 0] and np.array_equal(to_np(x)[[0, 2]], frames[[0, 2]])
    # 4: one bit of the first header bytes flipped so that the host names a truncated block: the first such flip (whatever its
    # pass count), and the one that turns the first block's passes into Table B.4's codeword "2" (bits 10), which no valid
    # lossless stream holds
    flips = []
    for at in range(first, first + 4):
        for bit in range(8):
            trial = bytearray(streams[1])
            trial[at] ^= 1 << bit
            try:
                dicom._j2k_codestream(np.frombuffer(bytes(trial), np.uint8), *shape, 16, "s")
            except ValueError as e:
                m = re.search(r"truncated code block \((\d+) coding passes for (-?\d+) magnitude bit planes\)", str(e))
                if m:
                    flips.append((bytes(trial), int(m.group(1)), int(m.group(2))))
    two = [f for f in flips if f[1] == 2]
    assert flips and two and flips[0][1] != 2
    for found in (flips[0], two[0]):
        damaged, _ = laid_out([streams[0], found[0], streams[2]])
        blocks, info, owned = run(data=damaged)
        assert info[1].tolist() == [4, 0, found[1], found[2]]
        others_stand(blocks, info, owned)
    assert info[1, 2] == 2                                  # the codeword "2"
    # 1: an unsound plan row; nothing but the status is written (a sentinel-filled blocks tensor)
    edits = [lambda f: f.update(start=len(buf) - 10), lambda f: f.update(length=-1), lambda f: f.update(first=f["length"] + 1),
             lambda f: f.update(end=f["length"] + 1),
             lambda f: f.update(row0=1 << 40), lambda f: f.update(row0=-1), lambda f: f.update(start=-1)]
    for n, change in enumerate(edits):
        def unsound(k, f, change=change):
            if k == 1:
                change(f)
        blocks, info, owned = run(unsound, fill=SENTINEL)
        assert info[1].tolist() == [1, 0, 0, 0], n
        got = to_np(blocks)
        assert (got[owned[1][0]:owned[1][0] + owned[1][1]] == SENTINEL).all(), n
        for k in (0, 2):
            want = host_rows(streams[k], shape, 16, k, starts[k])
            assert info[k].tolist() == [0, len(want), 0, 0] and np.array_equal(got[owned[k][0]:owned[k][0] + len(want)], want)
    # a row count that is not the geometry's, a parameter out of range, a tree larger than max_nodes
    plan, tables, owned, nodes = plan_rows(streams, starts, shape, 16)
    for change in (lambda p, t: p.__setitem__((1, 6), p[1, 6] - 1), lambda p, t: p.__setitem__((1, 4), p[1, 4] | 17),
                   lambda p, t: p.__setitem__((1, 4), (p[1, 4] & ~0xFF00) | (7 << 8)), lambda p, t: t.__setitem__((1, 0), 32),
                   lambda p, t: p.__setitem__((1, 7), 1)):
        p, t = plan.copy(), tables.copy()
        change(p, t)
        blocks = torch.full((sum(n for _, n in owned), 10), SENTINEL, dtype=torch.int64, device=dev)
        _, info = dicom.plan_jpeg2000_blocks(buf, p, t, *shape, nodes, device=dev, blocks=blocks, n_blocks=len(blocks))
        assert to_np(info)[:, 0].tolist() == [0, 1, 0]
        assert (to_np(blocks)[owned[1][0]:owned[1][0] + owned[1][1]] == SENTINEL).all()
    blocks = torch.full((sum(n for _, n in owned), 10), SENTINEL, dtype=torch.int64, device=dev)
    _, info = dicom.plan_jpeg2000_blocks(buf, plan, tables, *shape, nodes - 1, device=dev, blocks=blocks, n_blocks=len(blocks))
    assert to_np(info)[:, 0].tolist() == [1, 1, 1] and (to_np(blocks) == SENTINEL).all()


def check_c_abi_argument_checks(dev):
    """pl_dicom_j2k_plan: invalid argument (1) before any launch (the pointers are never dereferenced)"""
    lib = dicom._lib.load()
    p = 1 << 20
    good = dict(bytes_=p, nbytes=64, plan=p, tables=p, n=1, rows=8, cols=8, blocks=p, n_blocks=1, info=p, work=p, nodes=4)

    def call(**kw):
        a = {**good, **kw}
        return lib.pl_dicom_j2k_plan(a["bytes_"], a["nbytes"], a["plan"], a["tables"], a["n"], a["rows"], a["cols"], a["blocks"],
                                     a["n_blocks"], a["info"], a["work"], a["nodes"], None)

    for kw in (dict(bytes_=None), dict(plan=None), dict(tables=None), dict(blocks=None), dict(info=None), dict(work=None), dict(n=0),
               dict(n=65536), dict(n_blocks=-1), dict(n_blocks=1 << 31), dict(rows=0), dict(cols=65536), dict(nbytes=-1), dict(nodes=0),
               dict(nodes=(1 << 24) + 1), dict(work=p + 8)):
        assert call(**kw) == 1, kw
        assert b"pl_dicom_j2k_plan" in lib.pl_last_error()
    size = lib.pl_dicom_j2k_plan_work_bytes
    assert size(3, 100) == 3 * 100 * 16 and size(0, 8) == -1 and size(65536, 8) == -1 and size(1, 0) == -1 and size(1, (1 << 24) + 1) == -1
    header = open(dicom._lib.__file__.replace("pylinac_amd/_lib.py", "include/pylinac_hip.h")).read()
    assert "#define PL_J2K_PLAN_FIELDS %d" % dicom.J2K_PLAN_FIELDS in header and "#define PL_J2K_PLAN_TABLE %d" % dicom.J2K_PLAN_TABLE in header
