"""Checks of the row walk of pl_median3_threshold_profile_fwxm_cells_u16 / ..._cells_keep_u16, whose loads and stores are
predicated by OFFSET (a lane that must not load or store aims beyond a bounded buffer resource) -- shared by
tests/test_gpu_threshold_walk.py (MI355X) and tests/test_emulated_threshold_walk.py (the CPU emulator, the smaller shapes).

The reference in every case is the sequence of SEPARATE launches of tests/step_tail_checks.py (pl_median3_threshold_colsum_u16 ->
pl_colsum_to_mean -> pl_find_peaks -> pl_fwxm_record: kernels without a cell table, whose loads are not predicated at all), on
the same inputs, compared bit for bit: thresholded frames, profile, peaks, FWXM, record.  The kept-zero table must equal
`cellmax < threshold`, entry for entry.  The cell table handed to the launch is the true cell maxima of scipy's 3x3 median.

One needed cell beside the wave seam: 2 x 96 x 584 (73 lanes: a full column wave and a ragged one of nine lanes; three row
groups, so the band's fourth wave has no rows).  Exactly ONE 32 x 64 cell per frame reaches the threshold.  That cell is
filled with random values far above it; the column on either side of it holds such a value in every third row, and so does
the row above and below it in every third column -- too few to lift a median OUTSIDE the cell to the threshold (at most 4 of a
window's 9), but the medians along the cell's border depend on those values, so a neighbour column or row that was read as
zeros, or not read, changes pixels of `out`.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import keep_zeros_checks as kz
import step_tail_checks as checks

SEAM_SHAPE = (2, 96, 584)
SEAM_THR = 15000
# (row group, cell) of frame 0's needed cell; frame 1 takes the row group mirrored (2 - rg):
# the last cell of column wave 0 (columns 448-511: lane 63 fetches column 512 itself while wave 1 loads nothing), the first
# cell of column wave 1 (lane 0 fetches column 511), the ragged last cell (columns 576-583), and the first / last row group
SEAM_PLACES = ((1, 7), (1, 8), (1, 9), (0, 7), (2, 8), (0, 9))
CANARY = 0xBEEF

RAGGED_HEIGHTS = (2, 3, 9, 40)                     # rings deeper than the frame, a row group that is not full, two row groups
RAGGED_WIDTHS = (8, 520)                           # one lane; a full column wave and one lane of the next


def seam_frames(place, seed=3):
    """uint16 [2, 96, 584] as the module's docstring describes, frame 0's needed cell at `place`"""
    n, h, w = SEAM_SHAPE
    rng = np.random.default_rng(seed + 16 * place[0] + place[1])
    x = rng.integers(50, 150, SEAM_SHAPE).astype(np.uint16)
    high = lambda *s: rng.integers(20000, 30000, s).astype(np.uint16)
    for i in range(n):
        rg, cc = (place[0] if i == 0 else 2 - place[0]), place[1]
        ra, rb, ca, cb = 32 * rg, min(32 * rg + 32, h), 64 * cc, min(64 * cc + 64, w)
        x[i, ra:rb, ca:cb] = high(rb - ra, cb - ca)
        rows = np.arange(ra + 1, rb - 1, 3)
        cols = np.arange(ca + 1, cb - 1, 3)
        for c in (ca - 1, cb):
            if 0 <= c < w:
                x[i, rows, c] = high(rows.size)
        for r in (ra - 1, rb):
            if 0 <= r < h:
                x[i, r, cols] = high(cols.size)
    return x


def _expected_table(table_np, thr):
    return (table_np.astype(np.int64) < thr.cpu().numpy().astype(np.int64)[:, None, None]).astype(np.uint8)


def run_cells_launch(x, thr, table, out_fill=-1):
    """pl_median3_threshold_profile_fwxm_cells_u16 (CELLS without KEEP) on sentinel outputs"""
    import torch

    from pylinac_amd import _lib, ops
    from pylinac_amd._lib import check

    lib = _lib.load()
    n, h, w = x.shape
    o = checks.new_outputs(x)
    kz._fill(o["out"], out_fill)
    ws = torch.zeros((n, w + 1), dtype=torch.int64, device=x.device)
    prm = ops.make_peak_params(w, fwxm_height=0.5, max_number=1)
    check(lib.pl_median3_threshold_profile_fwxm_cells_u16(
        x.data_ptr(), o["out"].data_ptr(), n, h, w, thr.data_ptr(), table.data_ptr(),
        *kz._tail_args(prm, o, ws, 0, torch.cuda.current_stream().cuda_stream)), "cells tail")
    assert int(ws.cpu().abs().sum()) == 0, "workspace not returned to zero"
    return o


def run_keep_launch(x, thr, table, out, zeroed, reset):
    """pl_median3_threshold_profile_fwxm_cells_keep_u16 on the given `out` and table, every other output a sentinel buffer"""
    import torch

    from pylinac_amd import _lib, ops
    from pylinac_amd._lib import check

    lib = _lib.load()
    n, h, w = x.shape
    o = checks.new_outputs(x)
    o["out"] = out
    ws = torch.zeros((n, w + 1), dtype=torch.int64, device=x.device)
    prm = ops.make_peak_params(w, fwxm_height=0.5, max_number=1)
    check(lib.pl_median3_threshold_profile_fwxm_cells_keep_u16(
        x.data_ptr(), out.data_ptr(), n, h, w, thr.data_ptr(), table.data_ptr(), zeroed.data_ptr(), reset,
        *kz._tail_args(prm, o, ws, 0, torch.cuda.current_stream().cuda_stream)), "keep tail")
    assert int(ws.cpu().abs().sum()) == 0, "workspace not returned to zero"
    return o


def _new_out_and_table(x, out_pattern, table_pattern):
    import torch

    n, h, w = x.shape
    out = kz._fill(torch.empty((n, h, w), dtype=torch.uint16, device=x.device), out_pattern)
    zeroed = kz._fill(torch.empty((n, -(-h // 32), -(-w // 64)), dtype=torch.uint8, device=x.device), table_pattern)
    return out, zeroed


_SEAM = {}


def seam_case(dev, place):
    """(frames, thresholds, cell table, its numpy form, the separate launches' outputs), computed once per device and place"""
    import torch

    key = (str(dev), place)
    if key not in _SEAM:
        x_np = seam_frames(place)
        t_np = kz.cell_max(x_np)
        # the layout the case is about: one needed cell per frame, where it was placed
        want = np.zeros(t_np.shape, dtype=bool)
        want[0, place[0], place[1]] = want[1, 2 - place[0], place[1]] = True
        assert ((t_np >= SEAM_THR) == want).all(), np.argwhere((t_np >= SEAM_THR) != want).tolist()
        x = torch.from_numpy(x_np).to(dev)
        thr = torch.full((x.shape[0],), SEAM_THR, dtype=torch.int32, device=dev)
        _SEAM[key] = (x, thr, torch.from_numpy(t_np).to(dev), t_np, checks.run_reference(x, thr, checks.new_outputs(x)))
    return _SEAM[key]


def check_seam_keep(dev, place):
    """reset = 1 on an `out` of 0xFFFF and a table of 0x5A == the reference; then reset = 0 over a canary-filled `out` whose
    table says "kept" everywhere: the canary survives in every cell that is not needed and nowhere else, everything else and
    the table as before"""
    import torch

    x, thr, table, t_np, ref = seam_case(dev, place)
    out, zeroed = _new_out_and_table(x, -1, 0x5A)
    got = run_keep_launch(x, thr, table, out, zeroed, reset=1)
    checks.assert_same(ref, got, ("reset", place))
    assert np.array_equal(zeroed.cpu().numpy(), _expected_table(t_np, thr)), ("reset: table", place)
    kz._fill(out, CANARY - 0x10000)
    kz._fill(zeroed, 1)
    got = run_keep_launch(x, thr, table, out, zeroed, reset=0)
    n, h, w = x.shape
    needed = np.repeat(np.repeat(t_np >= SEAM_THR, 32, axis=1), 64, axis=2)[:, :h, :w]
    want = np.where(needed, ref["out"].cpu().numpy(), np.uint16(CANARY))
    assert np.array_equal(out.cpu().numpy(), want), ("kept: out", place, np.argwhere(out.cpu().numpy() != want)[:8].tolist())
    got["out"] = ref["out"]
    checks.assert_same(ref, got, ("kept: everything but the frames", place))
    assert np.array_equal(zeroed.cpu().numpy(), _expected_table(t_np, thr)), ("kept: table", place)


def check_seam_cells(dev, place):
    """keep_zeros=False's launch (CELLS without KEEP: the same predication) == the reference, every pixel stored"""
    x, thr, table, _, ref = seam_case(dev, place)
    checks.assert_same(ref, run_cells_launch(x, thr, table), ("cells", place))


_RAGGED = {}


def ragged_case(dev, h, w):
    """(frames, cell table, its numpy form, the three threshold vectors): below every median, a median that occurs, above"""
    import torch
    from scipy.ndimage import median_filter

    key = (str(dev), h, w)
    if key not in _RAGGED:
        x_np = np.random.default_rng(100 * h + w).integers(1000, 40000, (2, h, w)).astype(np.uint16)
        med = np.stack([median_filter(f, size=3, mode="reflect") for f in x_np])
        occurs = [int(np.sort(m.ravel())[(2 * m.size) // 3]) for m in med]        # most cells needed, some pixels below
        assert all((m == t).any() and (m < t).any() for m, t in zip(med, occurs))
        thrs = ([int(med.min())] * 2, occurs, [int(med.max()) + 1] * 2)
        t_np = kz.cell_max(x_np)
        _RAGGED[key] = (torch.from_numpy(x_np).to(dev), torch.from_numpy(t_np).to(dev), t_np,
                        [torch.tensor(t, dtype=torch.int32, device=dev) for t in thrs])
    return _RAGGED[key]


def check_ragged(dev, h, w):
    """frames shorter than the ring is deep, row groups that are not full, one-lane and ragged column waves, at the three
    thresholds: both launches == the reference; the keep launch a second time on what the first left (reset = 0)"""
    x, table, t_np, thrs = ragged_case(dev, h, w)
    for which, thr in enumerate(thrs):
        ref = checks.run_reference(x, thr, checks.new_outputs(x))
        checks.assert_same(ref, run_cells_launch(x, thr, table), ("cells", h, w, which))
        out, zeroed = _new_out_and_table(x, -1, 0x5A)
        for reset in (1, 0):
            got = run_keep_launch(x, thr, table, out, zeroed, reset=reset)
            checks.assert_same(ref, got, ("keep", h, w, which, reset))
            assert np.array_equal(zeroed.cpu().numpy(), _expected_table(t_np, thr)), ("table", h, w, which, reset)


def check_size_guard(lib):
    """the bounded resource holds frames of fewer than 2^31 bytes: larger ones are "not covered" (a host call, nothing allocated)"""
    from pylinac_amd import ops

    # (32768 columns are also more than the in-launch peak search takes; the tall frames of 1024 columns are not: the first of
    # them is exactly 2^31 bytes, the second sixteen rows short of it)
    for (h, w), want in (((32768, 32768), 0), ((1024, 1024), 1), ((1 << 20, 1024), 0), (((1 << 20) - 16, 1024), 1)):
        prm = ops.make_peak_params(w, fwxm_height=0.5, max_number=1)
        assert lib.pl_median3_threshold_profile_fwxm_covers(h, w, C.byref(prm)) == want, (h, w)
