"""JPEG 2000 conformance: legal streams that OpenJPEG's encoder never writes, through the host parser
(``dicom._j2k_codestream``), the decode kernels (``load_frames(jpeg2000=True)``), the plan kernel (``plan_jpeg2000_blocks``) and
``load_zip(encapsulated=True, jpeg2000=True)`` -- tests/test_emulated_dicom_j2k_conformance.py on the CPU emulator,
tests/test_gpu_dicom_j2k_conformance.py on the MI355X.  Every comparison is EQUALITY.

The streams come from tests/j2k_writer.py, a plain-Python T.800 writer in which every choice an encoder is free to make is a
parameter.  Three oracles, none of them this project's:
  1  the SOURCE array the writer was given;
  2  Pillow's OpenJPEG: ``verified(name)`` has ``PIL.Image.open`` decode every sound fixture to the source BEFORE a device is
     asked anything (for P below the container's bits the value shifted up, as ``dicom_j2k_checks.check_precision_sign`` states
     it).  What Pillow refuses although T.800 permits it is listed in ``PILLOW_LESS`` with Pillow's message, differs from a
     sibling that Pillow accepts in one writer parameter, and has the sibling's coefficients and segments (asserted from the
     two records); the list is asserted to be exactly what Pillow refuses;
  3  the writer's record of what it wrote, which ``_j2k_codestream``'s rows must equal (a device-free test of the host parser).
Every structural claim a fixture is named for -- a band of size 0, a header that ends in FF, a segment that ends in FF, blocks
excluded between included ones, the depth of a tag tree, the width of a length field -- is asserted on the CPU from the bytes
or from the record, in ``verified`` or in the group's ``claims_*``, before the device runs.

Fixtures are built once per process from fixed seeds; the seeds of groups b and g were found by a seeded search on the CPU
(a segment length with L mod 256 = 255; a segment that ends in FF and is sensitive to what the decoder feeds behind it; a 64 x 64 block whose last 1 KiB window holds
1 .. 3 bytes).  No frame is larger than 33 x 65, but for the one-block frames of 64 x 64 in group g."""
from __future__ import annotations

import functools
import io
import re

import numpy as np
import pytest
from PIL import Image

import dicom_j2k_checks as jk
import dicom_zip_j2k_checks as zj
import j2k_writer as jw
import zip_checks as zc
from pylinac_amd import dicom

to_np = dicom._to_numpy
MID8 = 128

# fixture name -> Pillow's message.  T.800 permits each (B.10.7.1 bounds neither Lblock nor the width of a length); OpenJPEG
# reads a length in at most 32 bits.  Every other fixture has Pillow's verdict.
PILLOW_LESS = {"c/16x16/k=30": "broken data stream when reading image file", "c/16x16/k=33": "broken data stream when reading image file"}
SIBLING = {"c/16x16/k=30": "c/16x16/k=20", "c/16x16/k=33": "c/16x16/k=20"}     # same frame, same writer parameters but ``lblock_extra``


class Fixture:
    def __init__(self, name: str, frame: np.ndarray, **kw):
        self.name, self.frame, self.kw = name, frame, kw
        self.data, self.rec = jw.encode(frame, **kw)
        self.bits = 8 * frame.dtype.itemsize
        self.precision = kw.get("precision", self.bits)
        self.signed = kw.get("signed", frame.dtype.kind == "i")

    def pillow_wants(self) -> np.ndarray:
        half = 1 << (self.precision - 1)
        return (self.frame.astype(np.int64) + (half if self.signed else 0)) << (self.bits - self.precision)

    def host_rows(self) -> list:
        return [tuple(r) for r in dicom._j2k_codestream(np.frombuffer(self.data, np.uint8), *self.frame.shape, self.bits, self.name)[3]]

    def header(self, packet) -> bytes:
        return self.data[packet.start:packet.header_end]


def noise(seed, shape, dtype=np.uint8, lo=None, hi=None) -> np.ndarray:
    info = np.iinfo(dtype)
    return np.random.default_rng(seed).integers(info.min if lo is None else lo, int(info.max) + 1 if hi is None else hi, shape).astype(dtype)


def sparse(shape=(33, 65)) -> np.ndarray:
    """mid-grey with seven spikes of different heights at odd places (every band of a level sees each): every band of the 4 x 4
    fixture (one level) and the one band of the 16 x 16 fixture (no level) has blocks with nothing in them before, between and
    behind blocks with something, and sibling leaves of unequal bit-plane counts"""
    a = np.full(shape, MID8, np.uint8)
    for (y, x), v in {(5, 21): 100, (5, 27): 3, (5, 53): 3, (7, 23): 9, (9, 41): 30, (21, 37): 17, (23, 13): 60}.items():
        a[y, x] = MID8 + v
    return a


def partly_noise(n: int, seed: int = 77) -> np.ndarray:
    """64 x 64 uint8: noise in the first ``n`` samples, mid-grey behind them (the segment's length follows n byte by byte)"""
    a = np.full(4096, MID8, np.uint8)
    a[:n] = np.random.default_rng(seed).integers(0, 256, n)
    return a.reshape(64, 64)


def _range_ends(seed, shape, precision, signed, dtype) -> np.ndarray:
    half = 1 << (precision - 1)
    lo, hi = (-half, half) if signed else (0, 2 * half)
    a = noise(seed, shape, dtype, lo, hi)
    a[0, 0], a[-1, -1], a[0, -1] = lo, hi - 1, hi - 1
    return a


# ---- the fixtures: name -> a function that builds it ------------------------------------------------------------------------
BUILDERS: dict = {}
GUARD_MB = [(0, 8), (1, 10), (2, 10), (7, 10), (2, 30), (7, 30), (2, 32), (7, 33), (7, 34), (6, 35), (7, 36), (7, 37)]   # (guard, Mb)
D_CONTENTS = {"noise": lambda: noise(41, (16, 16)), "constant, off the middle": lambda: np.full((16, 16), 1000 % 256, np.uint8),
              "spike": lambda: jk.content("spike", (16, 16), np.uint8)}
G_SIZES = [(1, 1), (1, 64), (64, 1), (3, 5), (4, 4), (64, 64)]
PRECISIONS = [(2, np.uint8), (7, np.uint8), (8, np.uint8), (9, np.uint16), (15, np.uint16)]
# what the seeded searches found (claims_b and claims_g assert each from the bytes):
B1 = dict(seed=19, top=180, termination="flush", guard=2, k=0)       # 16 x 16 noise below 180: a segment of 255 bytes, header CF B6 FF 00
B2 = dict(seed=174, top=1 << 12, termination="flush", guard=3, k=1)  # 33 x 65 noise below 2^12, 2 levels: LL's segment has 255 bytes
G_ENDS_FF = dict(shape=(4, 4), seed=619)                             # FLUSH .. 68 03 FF 7F, the shortest prefix ends in front of the FF
G_WINDOW = dict(n=953, termination="flush")                          # 1026 bytes: the second window holds 2


def _register():
    def add(name, make, **kw):
        assert name not in BUILDERS
        BUILDERS[name] = lambda: Fixture(name, make(), **kw)

    # a: bands of size 0, resolutions of 1 x 1, packets of resolutions without a band
    for shape in ((1, 9), (9, 1)):
        for levels in (1, 2, 4):
            add(f"a/{shape[0]}x{shape[1]}/L{levels}", lambda s=shape, l=levels: noise(10 + l, s), levels=levels)
    add("a/1x9/L0", lambda: noise(10, (1, 9)))
    add("a/9x1/L4/u16", lambda: noise(15, (9, 1), np.uint16), levels=4)
    for levels in (0, 3, 16):
        for empty in ("00", "80"):
            add(f"a/1x1/L{levels}/{empty}", lambda l=levels: np.array([[200 - l]], np.uint8), levels=levels, empty_packet=empty)
    add("a/5x7/L5", lambda: noise(16, (5, 7)), levels=5)
    add("a/5x7/L5/u16", lambda: noise(17, (5, 7), np.uint16), levels=5)
    add("a/2x3/L2", lambda: noise(18, (2, 3)), levels=2)
    # b: a packet header whose last byte is FF, in the last packet and in the first of three
    add("b/16x16", lambda: noise(B1["seed"], (16, 16), np.uint8, 0, B1["top"]), guard=B1["guard"], lblock_extra=B1["k"], termination=B1["termination"])
    add("b/33x65/L2", lambda: noise(B2["seed"], (33, 65), np.uint16, 0, B2["top"]), levels=2, guard=B2["guard"], termination=B2["termination"],
        lblock_extra=lambda i: B2["k"] if i == 0 else 0)
    # c: Lblock grows by more than it must
    for k in (1, 5, 20):
        add(f"c/33x65/k={k}", lambda: noise(31, (33, 65)), levels=2, block=(4, 4), lblock_extra=k)
    for k in (0, 5, 20, 30, 33):
        add(f"c/16x16/k={k}", lambda: noise(32, (16, 16)), levels=1, block=(4, 4), lblock_extra=k)
    # d: guard bits and exponents; the zero bit planes make up the difference
    for kind, make in D_CONTENTS.items():
        for guard, mb in GUARD_MB:
            add(f"d/{kind}/G{guard}/Mb{mb}", make, levels=1, block=(4, 4), guard=guard, exponents=[mb + 1 - guard] * 4)
    add("d/33x65/G7/Mb37", lambda: noise(42, (33, 65)), levels=2, block=(4, 4), guard=7, exponents=[31] * 7)
    # f: blocks not included between included ones
    for block in ((4, 4), (16, 16)):
        for kind, make in (("sparse", sparse), ("noise", lambda: noise(51, (33, 65))), ("constant", lambda: np.full((33, 65), MID8, np.uint8))):
            add(f"f/{kind}/cb{block[0]}", make, levels=1 if block[0] == 4 else 0, block=block, empty_packet="80" if block[0] == 4 else "00")
    # g: segment termination
    for shape in G_SIZES:
        for dtype in (np.uint8, np.uint16):
            for termination in ("shortest", "flush"):
                add(f"g/{shape[0]}x{shape[1]}/{np.dtype(dtype).name}/{termination}", lambda s=shape, d=dtype: noise(61 + s[0] + s[1], s, d),
                    termination=termination)
    add("g/16x16/cb4/shortest", lambda: noise(62, (16, 16)), block=(4, 4), termination="shortest")
    add("g/ends in FF", lambda: noise(G_ENDS_FF["seed"], G_ENDS_FF["shape"]), termination="shortest+ff")
    add("g/shorter than FLUSH", lambda: noise(G_ENDS_FF["seed"], G_ENDS_FF["shape"]), termination="shortest")
    add("g/16x16/cb4/shortest+ff", lambda: noise(62, (16, 16)), block=(4, 4), termination="shortest+ff")
    add("g/window tail", lambda: partly_noise(G_WINDOW["n"]), termination=G_WINDOW["termination"])
    for v in (1, -1, 2):                                     # all-MPS content: one small coefficient
        add(f"g/1x1/one coefficient {v}", lambda v=v: np.array([[MID8 + v]], np.uint8), termination="shortest")
        add(f"g/4x4/one coefficient {v}", lambda v=v: np.array([[MID8] * 4] * 3 + [[MID8, MID8 + v, MID8, MID8]], np.uint8), termination="shortest")
    # h: precision and sign written by the writer
    for precision, dtype in PRECISIONS:
        for signed in (False, True):
            container = np.dtype(dtype.__name__[1:]) if signed else np.dtype(dtype)
            add(f"h/P{precision}/{'signed' if signed else 'unsigned'}",
                lambda p=precision, s=signed, c=container: _range_ends(70 + p, (16, 16), p, s, c), precision=precision, signed=signed, levels=1)


_register()


@functools.lru_cache(maxsize=None)
def fixture(name: str) -> Fixture:
    return BUILDERS[name]()


def names(prefix: str) -> list:
    return [n for n in BUILDERS if n.startswith(prefix)]


def pillow_verdict(fx: Fixture):
    """None where Pillow decodes the fixture to the source, else its message"""
    try:
        got = np.asarray(Image.open(io.BytesIO(fx.data)))
    except OSError as e:
        return str(e)
    assert np.array_equal(got.astype(np.int64), fx.pillow_wants()), fx.name      # if the writer and Pillow disagree, the writer is wrong
    return None


@functools.lru_cache(maxsize=None)
def verified(name: str) -> Fixture:
    """oracles 2 and 3 and the Pillow-less conditions for one fixture, once per process, before any device sees it"""
    fx = fixture(name)
    message = pillow_verdict(fx)
    assert (message is not None) == (name in PILLOW_LESS), (name, message)
    if message is not None:
        assert message == PILLOW_LESS[name]
        sib = verified(SIBLING[name])
        differing = {k for k in set(fx.kw) | set(sib.kw) if fx.kw.get(k) != sib.kw.get(k)}
        assert differing == {"lblock_extra"} and np.array_equal(fx.frame, sib.frame) and pillow_verdict(sib) is None
        assert np.array_equal(fx.rec.coefficients, sib.rec.coefficients)
        assert [s.data for s in fx.rec.segments] == [s.data for s in sib.rec.segments]
        assert [r[1:] for r in fx.rec.blocks] == [r[1:] for r in sib.rec.blocks]
    assert fx.host_rows() == fx.rec.blocks, name
    return fx


# ---- structural claims, from the bytes and the record -----------------------------------------------------------------------
def empty_bands(fx: Fixture) -> int:
    return sum(1 for p in fx.rec.packets for b in p.bands if b.w == 0 or b.h == 0)


def claims_a():
    for name in names("a/1x9/L") + names("a/9x1/L"):
        fx, levels = verified(name), fixture(name).kw.get("levels", 0)
        assert empty_bands(fx) == 2 * levels                                       # HL or LH, and HH, of every level
        geometry = list(dicom._j2k_geometry(*fx.frame.shape, levels, 6, 6, None, [8] * (3 * levels + 1), name))
        assert sum(1 for _, _, _, bands in geometry for b in bands if b[3] == 0 or b[4] == 0) == 2 * levels   # the host lists them
    for levels in (0, 3, 16):
        for empty, byte in (("00", 0x00), ("80", 0x80)):
            fx = verified(f"a/1x1/L{levels}/{empty}")
            assert len(fx.rec.packets) == levels + 1 and empty_bands(fx) == 3 * levels and len(fx.rec.blocks) == 1
            assert all(fx.header(p) == bytes([byte]) and p.end == p.header_end for p in fx.rec.packets[1:])
    assert empty_bands(verified("a/5x7/L5")) == 6 and len(verified("a/5x7/L5").rec.packets) == 6    # resolutions 0 .. 2 are 1 x 1
    assert empty_bands(verified("a/5x7/L5/u16")) == 6
    assert empty_bands(verified("a/2x3/L2")) == 2


def claims_b():
    one = verified("b/16x16")
    assert len(one.rec.blocks) == 1 and one.rec.blocks[0][1] % 256 == 255 and len(one.rec.packets) == 1
    p = one.rec.packets[0]
    assert p.stuffed and one.header(p)[-2:] == b"\xff\x00" and one.header(p)[-2] == one.rec.blocks[0][1] & 255
    assert one.rec.blocks[0][0] == p.header_end                                    # the body begins behind the stuffed byte
    two = verified("b/33x65/L2")
    p = two.rec.packets[0]
    assert len(two.rec.packets) == 3 and p.stuffed and two.header(p)[-2:] == b"\xff\x00" and two.rec.blocks[0][1] % 256 == 255
    assert two.rec.packets[1].start == p.end == p.header_end + two.rec.blocks[0][1]    # the next packet's place depends on it
    assert len(two.rec.blocks) == 7


def header_ff_places(fx: Fixture) -> set:
    return {at - fx.rec.first_packet for p in fx.rec.packets for at in range(p.start, p.header_end) if fx.data[at] == 0xFF}


def claims_c():
    places = {}
    for k in (1, 5, 20):
        fx = verified(f"c/33x65/k={k}")
        least = [max(0, ln.bit_length() - 3 - (passes.bit_length() - 1)) for _, ln, passes, *_ in fx.rec.blocks]
        assert [s.lblock for s in fx.rec.segments] == [3 + m + k for m in least] and len(least) > 100
        places[k] = header_ff_places(fx)
        assert places[k]                                                           # FF bytes, and 7-bit bytes behind them
    assert places[1] != places[5] != places[20] != places[1]                       # in new places
    for k, bits in ((30, 37), (33, 40)):                                           # (the kernel follows a length exactly up to 2^40)
        assert {s.length_bits for s in verified(f"c/16x16/k={k}").rec.segments} == {bits}
    assert {s.length_bits for s in verified("c/16x16/k=20").rec.segments} == {27}


def claims_d():
    for kind in D_CONTENTS:
        first = verified(f"d/{kind}/G{GUARD_MB[0][0]}/Mb{GUARD_MB[0][1]}")
        deepest = 0
        for guard, mb in GUARD_MB:
            fx = verified(f"d/{kind}/G{guard}/Mb{mb}")
            assert np.array_equal(fx.rec.coefficients, first.rec.coefficients)
            assert [s.data for s in fx.rec.segments] == [s.data for s in first.rec.segments]     # the same coefficients and segments
            assert max(r[3] for r in fx.rec.blocks) <= 30
            zeros = [z for p in fx.rec.packets for b in p.bands for row in b.zero_planes for z in row if z is not None]
            assert zeros and all(z == mb - r[3] for z, r in zip(zeros, fx.rec.blocks))
            deepest = max(deepest, max(zeros))
            assert fx.data[jk.segments(fx.data)[0xFF5C] + 4] >> 5 == guard
        assert deepest >= 27 and first.rec.blocks                                  # thresholds far above what OpenJPEG's streams ask for
    assert max(r[3] for r in verified("d/noise/G0/Mb8").rec.blocks) == 8         # guard 0: Mb is exactly what the content needs


def inclusion_runs(band) -> str:
    return "".join("1" if inc else "0" for row in band.included for inc in row)


def claims_f():
    for cb in (4, 16):
        fx = verified(f"f/sparse/cb{cb}")
        bands = [b for p in fx.rec.packets for b in p.bands if b.w and b.h]
        assert len(bands) == (4 if cb == 4 else 1)
        for b in bands:
            runs = inclusion_runs(b)
            assert re.fullmatch("0+1.*10+1.*0+", runs), (cb, b.orient, runs)       # excluded before, between and behind included ones
            assert b.tree_depth >= 3
            unequal = [(cx, cy) for cy in range(b.ncy) for cx in range(0, b.ncx - 1, 2)
                       if b.included[cy][cx] and b.included[cy][cx + 1] and b.zero_planes[cy][cx] != b.zero_planes[cy][cx + 1]]
            unequal += [(cx, cy) for cy in range(0, b.ncy - 1, 2) for cx in range(b.ncx)
                        if b.included[cy][cx] and b.included[cy + 1][cx] and b.zero_planes[cy][cx] != b.zero_planes[cy + 1][cx]]
            assert unequal, (cb, b.orient)                             # sibling leaves of unequal value
        everything, nothing = verified(f"f/noise/cb{cb}"), verified(f"f/constant/cb{cb}")
        assert all("0" not in inclusion_runs(b) for p in everything.rec.packets for b in p.bands)
        assert nothing.rec.blocks == [] and len(nothing.data) - nothing.rec.first_packet == len(nothing.rec.packets) + 2    # one-byte packets and EOC


def claims_g() -> dict:
    segs = [(n, s) for n in names("g/") for s in verified(n).rec.segments]
    found = {
        "ends in FF": [n for n, s in segs if s.data.endswith(b"\xff")],
        "cut behind FF in front of a byte <= 8F": [n for n, s in segs if s.data.endswith(b"\xff") and len(s.full) > len(s.data)
                                                   and s.full[len(s.data)] <= 0x8F],
        "length 0": [n for n, s in segs if len(s.data) == 0],
        "window tail": [n for n, s in segs if len(s.data) > 1024 and len(s.data) % 1024 in (1, 2, 3)],
        "shorter than FLUSH": [n for n, s in segs if len(s.data) < len(s.full)],
    }
    for n, s in segs:
        assert s.full.startswith(s.data) and not s.full.endswith(b"\xff")
        if n.endswith("/flush"):
            assert s.data == s.full
    assert "g/shorter than FLUSH" in found["shorter than FLUSH"] and "g/ends in FF" in found["ends in FF"]
    # what follows that final FF matters: a decoder that reads seven 0-bits behind it (FF 00) decodes other decisions
    fx = verified("g/ends in FF")
    _, cxs, ds = jw.block_decisions(fx.rec.coefficients, 0)
    cut = fx.rec.segments[0].data
    assert jw.mq_replay(cut, len(cut), cxs, ds) and not jw.mq_replay(cut + b"\x00", len(cut) + 1, cxs, ds)
    assert found["ends in FF"] and found["cut behind FF in front of a byte <= 8F"] and found["window tail"] and found["shorter than FLUSH"]
    # No included block has a segment of length 0, and none can: its first decision 1 is coded under context 0 or the run-length
    # context, whose MPS is still 0 and whose Qe (0x0521, 0x0AC1 and below along NMPS) is under half the interval, so it is an
    # LPS in the interval's lower part -- and a decoder fed nothing but 1-bits stays in the upper part.  The one-coefficient
    # fixtures are the all-MPS-but-one content that comes closest: one or two bytes.
    assert found["length 0"] == []
    assert all(len(s.data) <= 2 for n in names("g/1x1/one") + names("g/4x4/one") for s in verified(n).rec.segments)
    return found


def claims_h():
    for precision, dtype in PRECISIONS:
        for signed in (False, True):
            fx = verified(f"h/P{precision}/{'signed' if signed else 'unsigned'}")
            half = 1 << (precision - 1)
            assert fx.data[42] == (precision - 1) | (0x80 if signed else 0)
            assert (int(fx.frame.min()), int(fx.frame.max())) == ((-half, half - 1) if signed else (0, 2 * half - 1))


# ---- the three ways ---------------------------------------------------------------------------------------------------------
def stacks(fixture_names) -> list:
    """the fixtures grouped into stacks one call can load: same shape, container, precision and sign"""
    groups: dict = {}
    for n in fixture_names:
        fx = verified(n)
        groups.setdefault((fx.frame.shape, fx.frame.dtype, fx.precision), []).append(fx)
    return list(groups.values())


def file_of(fxs) -> bytes:
    extra = jk.bits_stored(fxs[0].precision) if fxs[0].precision != fxs[0].bits else b""
    return jk.j2k_file(np.stack([f.frame for f in fxs]), streams=[f.data for f in fxs], extra=extra)


def assert_loads(dev, fixture_names, one_file_each: bool = False):
    """way 1, ``load_frames``: the host's tier 2 and the decode kernels == the source (``one_file_each``: a file per fixture in
    one call, so that frames with fewer levels sit out launches)"""
    for fxs in stacks(fixture_names):
        frames = np.stack([f.frame for f in fxs])
        if fxs[0].precision == fxs[0].bits and not fxs[0].signed and not any(f.name in PILLOW_LESS for f in fxs) and not one_file_each:
            jk.assert_decodes(dev, frames, [f.data for f in fxs])                  # (Pillow once more, and the load)
            continue
        got, metas = jk.load(dev, [file_of([f]) for f in fxs] if one_file_each else [file_of(fxs)])
        assert got.dtype == frames.dtype and np.array_equal(got, frames), [f.name for f in fxs]
        assert metas[0].BitsStored == fxs[0].precision and metas[0].PixelRepresentation == int(fxs[0].signed)


def assert_plans(dev, fixture_names):
    """way 2, ``plan_jpeg2000_blocks`` against ``_j2k_codestream`` row for row (the -1 rows, the count, status 0), a stack per
    call"""
    for fxs in stacks(fixture_names):
        zj.assert_plan_equals_host(dev, [f.data for f in fxs], fxs[0].frame.shape, fxs[0].bits)


def assert_archive(dev, fixture_names):
    """way 3, ``load_zip``: one archive, a member per fixture == ``load_frames`` on the extracted members == the source"""
    (fxs,) = stacks(fixture_names)
    files = [(f"m{k}.dcm", file_of([f])) for k, f in enumerate(fxs)]
    zj.same(dev, zc.dicom_zip(files), np.stack([f.frame for f in fxs]), names=[n for n, _ in files])


def check_group(dev, prefix: str, claims=None, skip=()):
    """the group's claims on the CPU, then ways 1 and 2 for every fixture of it"""
    if claims is not None:
        claims()
    wanted = [n for n in names(prefix) if n not in skip]
    assert wanted
    for n in wanted:
        verified(n)
    assert_loads(dev, wanted)
    assert_plans(dev, wanted)


def check_stack_of_level_counts(dev):
    """1 x 9 files of 0, 1, 2 and 4 levels in ONE call: the frames with fewer levels sit out the launches of the upper ones"""
    wanted = ["a/1x9/L4", "a/1x9/L0", "a/1x9/L2", "a/1x9/L1"]
    assert [fixture(n).kw.get("levels", 0) for n in wanted] == [4, 0, 2, 1]
    assert_loads(dev, wanted, one_file_each=True)
    assert_archive(dev, wanted)


def check_mixed_inclusion_stack(dev):
    """the sparse frame between an all-included and an all-excluded one, in one file and in one archive"""
    claims_f()
    for cb in (4, 16):
        wanted = [f"f/noise/cb{cb}", f"f/sparse/cb{cb}", f"f/constant/cb{cb}"]
        assert_loads(dev, wanted)
        assert_plans(dev, wanted)
    assert_archive(dev, ["f/noise/cb4", "f/sparse/cb4", "f/constant/cb4", "f/sparse/cb16", "c/33x65/k=20", "d/33x65/G7/Mb37"])


ARCHIVE_16 = ["b/16x16", "c/16x16/k=30", "d/noise/G7/Mb37", "d/spike/G0/Mb8", "g/16x16/cb4/shortest", "h/P8/unsigned"]


def check_archive_of_every_group(dev):
    """way 3: archives that between them hold a fixture of every group -- b, c, d, g and h in one of 16 x 16 (a of 1 x 9 in
    ``check_stack_of_level_counts``; c, d and f of 33 x 65 in ``check_mixed_inclusion_stack``; e in ``check_status_8``)"""
    assert {n[0] for n in ARCHIVE_16} == set("bcdgh")
    assert_archive(dev, ARCHIVE_16)
    assert_archive(dev, ["h/P7/unsigned"])                                         # BitsStored below the container's


# ---- e: more than 30 magnitude bit planes -------------------------------------------------------------------------------------
def check_status_8(dev):
    """one block of 31 bit planes and 91 passes behind a real header: ``load_frames`` refuses it in ``_J2K_PLANES``'s words,
    the plan kernel flags that frame alone (status 8, detail 31) between two good frames that still plan and decode, and
    ``load_zip`` refuses the member in the same words"""
    shape = (16, 16)
    good = [verified("d/noise/G2/Mb30"), verified("d/spike/G7/Mb37")]
    frame = noise(41, shape)
    bad, rec = jw.encode(frame, guard=2, exponents=[30], forged=(31, 91, bytes(range(1, 9))))
    assert rec.blocks == [(rec.packets[0].header_end, 8, 91, 31, 0, 0, 0, 16, 16)]
    text = "JPEG 2000 Pixel Data: a code block of 31 magnitude bit planes: at most 30"
    with pytest.raises(NotImplementedError, match=re.escape(text)):
        dicom._j2k_codestream(np.frombuffer(bad, np.uint8), *shape, 8, "s")
    with pytest.raises(NotImplementedError, match="file 1: " + re.escape(text)):
        jk.load(dev, [file_of(good[:1]), jk.j2k_file(frame[None], streams=[bad]), file_of(good[1:])])
    streams = [good[0].data, bad, good[1].data]
    buf, starts = zj.laid_out(streams)
    plan, tables, owned, nodes = zj.plan_rows(streams, starts, shape, 8)
    blocks, info = dicom.plan_jpeg2000_blocks(buf, plan, tables, *shape, nodes, device=dev)
    info, rows = to_np(info), to_np(blocks)
    assert info[1].tolist() == [dicom.J2K_PLAN_PLANES, 0, 31, 0] and dicom.J2K_PLAN_PLANES == 8
    assert (rows[owned[1][0]:owned[1][0] + owned[1][1], 0] == -1).all()
    for k in (0, 2):
        want = zj.host_rows(streams[k], shape, 8, k, starts[k])
        assert info[k].tolist() == [0, len(want), 0, 0] and np.array_equal(rows[owned[k][0]:owned[k][0] + len(want)], want)
    params = np.asarray([(1, 8, 0, 0), (0, 8, 0, 0), (1, 8, 0, 0)], dtype=np.int32)
    x = dicom.decode_jpeg2000_frames(buf, blocks, params, *shape, 8, device=dev)
    assert to_np(x._pl_status).tolist() == [0, 0, 0]
    assert np.array_equal(to_np(x)[0], good[0].frame) and np.array_equal(to_np(x)[2], good[1].frame)
    files = [("ok.dcm", file_of(good[:1])), ("bad.dcm", jk.j2k_file(frame[None], streams=[bad])), ("fine.dcm", file_of(good[1:]))]
    assert text in zj.same_error(dev, zc.dicom_zip(files), "bad.dcm")


# ---- device-free ------------------------------------------------------------------------------------------------------------
def check_writer_and_host_parser(skip=()):
    """every fixture: Pillow's verdict, the Pillow-less list exactly, the record == the host's rows; every group's claims"""
    refused = set()
    for n in BUILDERS:
        if n in skip:
            continue
        fx = verified(n)
        if pillow_verdict(fx) is not None:
            refused.add(n)
    assert refused == set(PILLOW_LESS) - set(skip)
    claims_a(), claims_b(), claims_c(), claims_d(), claims_f(), claims_h()
    return claims_g()
