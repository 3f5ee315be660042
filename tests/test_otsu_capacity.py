"""The capacity-limited machinery of the median + Otsu stage (pylinac_amd/csrc/hist_otsu.hip) at its limits:

  A. otsu16_full_kernel's wave-uniform bulk adds (``tally_bulk``): the 64-entry side list, the list-full branch into the 16-bit
     fields, a key whose count is field + note, the checked-total retry and the guarded pass taking bulk adds, partial waves.
     Row-constant frames: one value per row -> the 3x3 median is row-constant too, EVERY wave row is flat, every row one key.
     (What the outputs can and cannot show: a bulk count that is DROPPED or doubled makes the decoded total differ from the
     pixel count, the kernel repeats the frame with the guard bit and the answer is right again, only later.  These cases pin
     what the total cannot: a count that reaches the wrong key -- in the list, in the field behind a full list, in the scan's
     look-ups -- and the guarded pass itself, which has no second net.)
  B. the 38 912-bin LDS window of otsu16_window_kernel at range == kWinBins - 1 / kWinBins / kWinBins + 1, pinned to 0, pinned
     to 65535 and centred (straddling the int16 sign), a narrow range at either end (the centred window is shifted, not cut),
     a value the 1/16 sample did not see, and the caller's bounds (exact, one too wide, not enclosing).

Reference: scipy.ndimage.median_filter(f, size=3) per frame (the raw frame for ops.otsu16), then the oracle's threshold_otsu,
min and max.  Integers: every comparison is np.array_equal.  Every case as uint16 and as int16 (values - 32768).  The
``-m gpu`` tests run on the device; the rest run the same check functions on the CPU-emulated kernels (tests/hipemu)."""
from __future__ import annotations

import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

K_WIN = 38912          # kWinBins
K_BULK = 64            # kFullBulk
DTYPES = (np.uint16, np.int16)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


# ---- reference and calls ------------------------------------------------------------------------------------------------------
def _typed(keys, dt):
    """frames given as keys 0 .. 65535 (int64) -> the dtype under test (int16: values - 32768)"""
    return (keys - (32768 if dt == np.int16 else 0)).astype(dt)


def _reference(frames, median):
    """(threshold, min, max) int64 [N] of the frames, or of their 3x3 medians"""
    from scipy import ndimage

    from oracle import pylinac_oracle as o

    planes = np.stack([ndimage.median_filter(f, size=3) for f in frames]) if median else frames
    flat = planes.reshape(len(planes), -1).astype(np.int64)
    return np.array([int(o.threshold_otsu(f)) for f in planes], dtype=np.int64), flat.min(1), flat.max(1), planes


def _native(x, median, lo=None, hi=None):
    """pl_otsu16 / pl_median3_otsu16 through the C entry point (caller's bounds; the flag of the plain form)
    -> (thr, min, max, flag) numpy"""
    from pylinac_amd import _lib, ops

    n, h, w = x.shape
    dev = x.device
    thr, mn, mx, flag = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    hist = torch.empty((n, 65536), dtype=torch.int32, device=dev)
    plo = None if lo is None else lo.data_ptr()
    phi = None if hi is None else hi.data_ptr()
    lib = _lib.load()
    if median:
        scratch = torch.empty_like(x)
        _lib.check(lib.pl_median3_otsu16(x.data_ptr(), scratch.data_ptr(), ops._dt(x), n, h, w, plo, phi, thr.data_ptr(),
                                         mn.data_ptr(), mx.data_ptr(), flag.data_ptr(), hist.data_ptr(), ops._stream()),
                   "pl_median3_otsu16")
    else:
        _lib.check(lib.pl_otsu16(x.data_ptr(), ops._dt(x), n, h * w, plo, phi, thr.data_ptr(), mn.data_ptr(), mx.data_ptr(),
                                 flag.data_ptr(), hist.data_ptr(), ops._stream()), "pl_otsu16")
    return tuple(t.cpu().numpy() for t in (thr, mn, mx, flag))


def _assert_both_forms(frames, refs, dev, tag, median_flag, plain_flag=None):
    """ops.median3_otsu16 and ops.otsu16 of one batch against the references (median, raw); median_flag / plain_flag: the
    flags the window kernel must leave (plain_flag through the C entry point: ops.otsu16 does not return it)"""
    from pylinac_amd import ops

    x = torch.from_numpy(np.array(frames)).to(dev)
    thr, mn, mx, flag = (t.cpu().numpy() for t in ops.median3_otsu16(x))
    print(tag, "median3_otsu16", thr.tolist(), mn.tolist(), mx.tolist(), flag.tolist(), "want", refs[True][0].tolist())
    assert np.array_equal(flag, median_flag), (tag, flag.tolist())
    for got, want, what in zip((thr, mn, mx), refs[True], ("threshold", "min", "max")):
        assert np.array_equal(got, want), (tag, "median", what, got.tolist(), want.tolist())
    thr, mn, mx = (t.cpu().numpy() for t in ops.otsu16(x))
    print(tag, "otsu16", thr.tolist(), mn.tolist(), mx.tolist(), "want", refs[False][0].tolist())
    for got, want, what in zip((thr, mn, mx), refs[False], ("threshold", "min", "max")):
        assert np.array_equal(got, want), (tag, "plain", what, got.tolist(), want.tolist())
    if plain_flag is not None:
        thr, mn, mx, flag = _native(x, False)
        assert np.array_equal(flag, plain_flag), (tag, "plain", flag.tolist())
        for got, want, what in zip((thr, mn, mx), refs[False], ("threshold", "min", "max")):
            assert np.array_equal(got, want), (tag, "plain, C entry", what, got.tolist(), want.tolist())


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _refs(frames):
    return {True: _frozen(*_reference(frames, True)[:3]), False: _frozen(*_reference(frames, False)[:3])}


def _flat_rows(plane):
    """rows of a [H, W] plane that hold one value"""
    return (plane == plane[:, :1]).all(1)


# ---- A. flat waves in the full-range kernel -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wedge_case(w, dt):
    """A1: 160 rows, value(row) = 300 * row: 160 flat keys (> the 64 list entries: the rest go to the fields, n = 8 x lanes
    per add), range 47 700 > the window"""
    keys = np.broadcast_to(300 * np.arange(160, dtype=np.int64)[:, None], (160, w))
    frames = _typed(keys, dt)[None]
    med = _reference(frames, True)[3][0]
    assert _flat_rows(med).all() and len(np.unique(med)) == 160 > K_BULK      # what the case is built for
    assert int(med.max()) - int(med.min()) + 1 > K_WIN
    return _frozen(frames)[0], _refs(frames)


def check_wedge(dev, dt, widths=(512, 520, 64)):
    """w = 512: one column wave, all 64 lanes on (n = 512).  w = 520: a second column wave with ONE lane on (n = 8; the lane
    that adds is `first_on`).  w = 64: eight lanes on (n = 64).  The plain form on the same frames (A4) has no bulk branch."""
    for w in widths:
        frames, refs = _wedge_case(w, dt)
        _assert_both_forms(frames, refs, dev, ("wedge", w, dt.__name__), median_flag=[1])


@functools.lru_cache(maxsize=None)
def _bands_case(w, dt):
    """A2: 40 flat bands of 8 rows (40 keys: the list does not fill), values over the whole range in no order; 300 scattered
    single pixels (the median removes them; the plain form sees them); and 3x3 patches that carry ONE band's value inside
    ANOTHER band: the median keeps their centre cross, those rows are not flat and tally pixel by pixel -- the count of
    such a key is its 16-bit field PLUS its list entry."""
    rng = np.random.default_rng(404)
    nb, rows = 40, 8
    values = np.round(np.linspace(0, 65535, nb)).astype(np.int64)
    values = values[rng.permutation(nb)]
    keys = np.repeat(values, rows)[:, None] * np.ones((1, w), dtype=np.int64)
    ys, xs = rng.integers(0, nb * rows, 300), rng.integers(0, w, 300)
    keys[ys, xs] = rng.integers(0, 65536, 300)
    donors = rng.permutation(nb)[:12]
    for k, a in enumerate(donors):
        b = int(donors[(k + 1) % len(donors)])                   # band b receives band a's value
        c = int(rng.integers(1, w - 4))
        keys[b * rows + 3:b * rows + 6, c:c + 3] = values[a]
    frames = _typed(keys, dt)[None]
    med = _reference(frames, True)[3][0]
    flat = _flat_rows(med)
    off = 32768 if dt == np.int16 else 0
    both = [int(v) for v in values[donors] if (med[flat] == v - off).any() and (med[~flat] == v - off).any()]
    assert len(both) >= 6, both                                   # keys counted in a field AND in a note
    assert len(np.unique(med[flat][:, 0])) <= K_BULK
    return _frozen(frames)[0], _refs(frames)


def check_bands(dev, dt, w=512):
    frames, refs = _bands_case(w, dt)
    _assert_both_forms(frames, refs, dev, ("bands", w, dt.__name__), median_flag=[1])


@functools.lru_cache(maxsize=None)
def _block_case(w, block_rows, dt):
    """A3: three frames of 1024 wedge rows (value = 60 * row, 1024 flat keys) and `block_rows` rows of ONE value V, more than
    65 535 pixels of it.

    Why V finds the side list full in frames 0 and 1: full_tally_pass gives wave wv the items wv, wv + 16, wv + 32, ... in that
    order, and with w <= 512 (one column wave) item i is the row group [32 i, 32 i + 32).  Items 0 .. 31 are the 1024 wedge
    rows, so the first TWO items of each of the 16 waves are 64 wedge rows of its own: 64 different keys, none of them met
    before (no list hit), each taking one ticket of n_bulk.  A wave therefore reaches its third item -- the first that can
    touch the block -- only after n_bulk >= 64 by its own tickets alone: the list is full, V goes to its 16-bit field 8 x lanes
    at a time, the field overflows, the decoded total comes out short and the guarded pass runs with bulk adds (one fold per
    32 768: two folds at 512 x 160).

      frame 0: wedge, then the block.  Every add to V is a multiple of 8 x lanes: the guard is crossed at exactly 0x8000.
      frame 1: the same with five 3x3 patches of another value near the top of the block: the median keeps their centre
               cross, those rows tally V pixel by pixel, and the bulk add that crosses the guard finds a field that is NOT
               a multiple of its own size.
      frame 2: the block on top, the wedge below: V takes list entries first (one per wave that starts in the block: duplicate
               entries of one key), a 32-bit count, no retry.
    """
    wedge_rows = 1024
    assert w <= 512 and w % 8 == 0 and wedge_rows == 16 * 2 * 32 and block_rows * w > 65535   # the argument above
    V, other = 65000, 7
    wedge = 60 * np.arange(wedge_rows, dtype=np.int64)
    col = np.concatenate([wedge, np.full(block_rows, V, dtype=np.int64)])
    keys = np.stack([np.broadcast_to(col[:, None], (len(col), w)).copy() for _ in range(3)])
    for j in range(5):
        r0, c0 = wedge_rows + 32 * j + 2, 5 + 9 * j
        keys[1, r0:r0 + 3, c0:c0 + 3] = other
    keys[2] = keys[0][::-1]                                       # the block first; the wedge falls from 61 380 to 0
    frames = _typed(keys, dt)
    med = _reference(frames, True)[3]
    off = 32768 if dt == np.int16 else 0
    for f in range(3):
        assert ((med[f] == V - off) & _flat_rows(med[f])[:, None]).sum() > 65535
        assert (~_flat_rows(med[f])).sum() == (15 if f == 1 else 0)
        assert len(np.unique(med[f][:wedge_rows] if f < 2 else med[f][block_rows:])) == wedge_rows
    singles = int(((med[1] == V - off) & ~_flat_rows(med[1])[:, None]).sum())
    assert singles > 0 and singles % (8 * min(w // 8, 64)) != 0, singles
    return _frozen(frames)[0], _refs(frames)


def check_block(dev, dt, w, block_rows):
    frames, refs = _block_case(w, block_rows, dt)
    _assert_both_forms(frames, refs, dev, ("block", w, block_rows, dt.__name__), median_flag=[1, 1, 1])


# ---- B. the window's edges ----------------------------------------------------------------------------------------------------
def _edge_frame(rng, shape, lo, hi, stray=None):
    """noise inside [lo, hi] (a third of it ON the four end values), both extrema as 3x3 patches in rows 0 .. 2: inside the
    first 1024 pixels, which the window kernel's 1/16 sample always reads -- the window is placed from the true range -- and
    the median keeps the centre of a patch (on row 0 as well: 'reflect' repeats it).  stray = (value, size): a size x size
    patch of a value outside [lo, hi] in rows the sample does not read."""
    h, w = shape
    assert 3 * w <= 1024 and h * w <= 16384                      # one sampled block: pixels 0 .. 1023
    keys = rng.integers(lo, hi + 1, shape)
    ends = rng.choice(np.array([lo, lo + 1, hi - 1, hi]), shape)
    keys = np.where(rng.random(shape) < 0.33, ends, keys).astype(np.int64)
    keys[0:3, 2:5] = lo
    keys[0:3, 10:13] = hi
    if stray is not None:
        value, size = stray
        r0 = 1024 // w + 5
        keys[r0:r0 + size, 20:20 + size] = value
    return keys


@functools.lru_cache(maxsize=None)
def _edges_case(shape, dt):
    """-> frames [13, H, W], references, the (lo, hi) keys the frames were built from, the flags of the median and plain form"""
    rng = np.random.default_rng(38912 + shape[1])
    spans = []
    for r in (K_WIN - 1, K_WIN, K_WIN + 1):
        for lo in (0, 65536 - r, (65536 - r) // 2):             # pinned to 0, pinned to 65535, centred (int16: straddles 0)
            spans.append((lo, lo + r - 1))
    spans += [(65536 - 20000, 65535), (0, 19999)]                # narrow at an end: the centred window is shifted, not cut
    frames = [_edge_frame(rng, shape, lo, hi) for lo, hi in spans]
    # sampled range 10000 .. 39999 -> window 5544 .. 44455; 47000 is outside it although 10000 .. 47000 would fit a window
    spans += [(10000, 39999)] * 2
    frames.append(_edge_frame(rng, shape, 10000, 39999, stray=(47000, 1)))   # one pixel: the median removes it
    frames.append(_edge_frame(rng, shape, 10000, 39999, stray=(47000, 3)))   # 3x3: the median keeps its centre cross
    frames = _typed(np.stack(frames), dt)
    spills = [int(hi - lo + 1 > K_WIN) for lo, hi in spans[:11]]
    refs = _refs(frames)
    off = 32768 if dt == np.int16 else 0
    for median in (True, False):                                 # the frames are what they were built to be
        assert np.array_equal(refs[median][1][:11] + off, [lo for lo, _ in spans[:11]])
        assert np.array_equal(refs[median][2][:11] + off, [hi for _, hi in spans[:11]])
    assert refs[True][2][11] + off == 39999 and refs[False][2][11] + off == 47000 and refs[True][2][12] + off == 47000
    return _frozen(frames)[0], refs, tuple(spans), spills + [0, 1], spills + [1, 1]


def check_window_edges(dev, dt, shape):
    frames, refs, spans, median_flag, plain_flag = _edges_case(shape, dt)
    _assert_both_forms(frames, refs, dev, ("edges", shape, dt.__name__), median_flag=median_flag, plain_flag=plain_flag)


def check_window_hints(dev, dt, shape):
    """The caller's bounds: exact at range 38 912 (served by the window), exact at 38 913 (fall back), one short at either end
    on a narrow frame (a value outside the bounds: fall back) -- the reference's numbers every time, both forms."""
    frames, refs, spans, _, _ = _edges_case(shape, dt)
    off = 32768 if dt == np.int16 else 0
    pick = [3, 4, 5, 6, 7, 8, 9, 10]
    lo = np.array([spans[k][0] for k in pick]) - off
    hi = np.array([spans[k][1] for k in pick]) - off
    lo[6] += 1                                                    # frame 9 holds its lo, frame 10 its hi (3x3 patches)
    hi[7] -= 1
    want_flag = [0, 0, 0, 1, 1, 1, 1, 1]
    x = torch.from_numpy(np.array(frames[pick])).to(dev)
    tlo = torch.from_numpy(lo.astype(np.int32)).to(dev)
    thi = torch.from_numpy(hi.astype(np.int32)).to(dev)
    for median in (True, False):
        thr, mn, mx, flag = _native(x, median, tlo, thi)
        tag = ("hints", shape, dt.__name__, "median" if median else "plain")
        print(tag, thr.tolist(), mn.tolist(), mx.tolist(), flag.tolist())
        assert np.array_equal(flag, want_flag), (tag, flag.tolist())
        for got, want, what in zip((thr, mn, mx), refs[median], ("threshold", "min", "max")):
            assert np.array_equal(got, want[pick]), (tag, what, got.tolist(), want[pick].tolist())


EDGE_SHAPES = ((64, 256), (37, 264))
each_dtype = pytest.mark.parametrize("dt", DTYPES, ids=lambda d: d.__name__)
each_shape = pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "%dx%d" % s)


# ---- the emulated kernels (the emulator's forms are smaller where the emulator's speed asks for it) ------------------------------
@each_dtype
def test_emulated_wedge_list_overflow(emulated, dt):
    check_wedge(emulated, dt)


@each_dtype
def test_emulated_bands_field_plus_note(emulated, dt):
    check_bands(emulated, dt, w=64)


@each_dtype
def test_emulated_block_overflow_guarded_bulk(emulated, dt):
    check_block(emulated, dt, w=64, block_rows=1040)              # 66 560 pixels of V


@each_shape
@each_dtype
def test_emulated_window_edges(emulated, dt, shape):
    check_window_edges(emulated, dt, shape)


@each_shape
@each_dtype
def test_emulated_window_hints(emulated, dt, shape):
    check_window_hints(emulated, dt, shape)


# ---- the device ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@each_dtype
def test_wedge_list_overflow(gpu, dt):
    check_wedge(gpu, dt)


@pytest.mark.gpu
@each_dtype
def test_bands_field_plus_note(gpu, dt):
    check_bands(gpu, dt, w=512)
    check_bands(gpu, dt, w=64)


@pytest.mark.gpu
@each_dtype
def test_block_overflow_guarded_bulk(gpu, dt):
    check_block(gpu, dt, w=512, block_rows=160)                   # 81 920 pixels of V: two folds
    check_block(gpu, dt, w=64, block_rows=1040)


@pytest.mark.gpu
@each_shape
@each_dtype
def test_window_edges(gpu, dt, shape):
    check_window_edges(gpu, dt, shape)


@pytest.mark.gpu
@each_shape
@each_dtype
def test_window_hints(gpu, dt, shape):
    check_window_hints(gpu, dt, shape)
