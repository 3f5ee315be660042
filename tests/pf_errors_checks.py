"""Checks of picketfence.evaluate_batch / pl_pf_errors -- the picket fits, the leaf errors in mm and the pass / fail summary
computed on the device from the position table of picketfence.analyze_batch -- shared by tests/test_gpu_pf_errors.py
(MI355X) and tests/test_emulated_pf_errors.py (the CPU emulator of tests/hipemu).  tests/test_pf_errors_restatement.py
ties `restate` below to the reference's own ``PicketFence.analyze()`` through the ``max_error`` the goldens store.

The rule (pinned on the goldens, bit for bit): a picket's line is ``np.polyfit`` of degree 1 through (upper marker coordinate
of the leaf, measured position) over the leaves it measured, with ``up = leaf_center_px - leaf_width_px / 2 *
leaf_analysis_width_ratio``; a window's error is its position minus the line evaluated at ``leaf_center_px``, over dpmm.

Bounds of the device comparison: 1e-9 mm on errors / max_error / abs_median_error and 1e-9 px on the line's values at the
first and last leaf centre -- the project's bar for picket positions.  The kernel fits in the centred form (means, Sxx, Sxy)
where numpy solves a scaled least-squares system; positions are below 2^10 pixels, so one rounding is 1.1e-13 px and the two
forms differ by a few tens of roundings, two orders inside the bound.  Every other field is compared exactly; each case first
shows on the restatement that no |error| lies within 1e-8 of a tolerance and that the two largest |errors| differ by more
than 1e-8, so that the exact fields cannot hinge on the last bits of an error.
"""
from __future__ import annotations

import numpy as np

from oracle import pylinac_oracle as o

FIELDS = ("n_measured", "max_error", "max_error_leaf", "max_error_picket", "abs_median_error", "percent_passing", "passed",
          "percent_under_action")
BOUND_MM = 1e-9
BOUND_PX = 1e-9
GAP = 1e-8


# ----------------------------------------------------------------------------------------------------------- restatement
def geometry(shape, dpmm, mlc="MILLENNIUM", orientation="UP_DOWN", ratio=0.4):
    """-> (leaf numbers in view, leaf_center_px, leaf_up_px): _leaves_in_view / _get_mlc_window arithmetic and the upper
    marker coordinate of MLCValue"""
    leaves, centers, widths = o.mlc_arrangement(o.MLC_ARRANGEMENTS[mlc] if isinstance(mlc, str) else mlc)
    across = shape[0] if orientation == "UP_DOWN" else shape[1]
    pixel_range = across / 2
    pixel_range -= max(widths[0] * ratio, widths[-1] * ratio) * dpmm
    view = [(n, c, w) for n, c, w in zip(leaves, centers, widths) if abs(c) < pixel_range / dpmm]
    nums = [n for n, _, _ in view]
    center_px = np.array([c * dpmm + across / 2 for _, c, _ in view])
    up_px = np.array([(c * dpmm + across / 2) - (w * dpmm) / 2 * ratio for _, c, w in view])
    return nums, center_px, up_px


def restate(position, status, picket_count, leaf_nums, center_px, up_px, dpmm, tolerance=0.5, action_tolerance=None):
    """one frame: position [L, cap] float64 (NaN = none), status [L, cap] -> dict(fit [cap, 2], picket_status [cap],
    error [L, cap], passed_window [L, cap], summary [8]) with numpy: np.polyfit / np.poly1d per picket, np.median"""
    position = np.asarray(position, np.float64)
    nl, cap = position.shape
    meas = (np.asarray(status) == 0) & ~np.isnan(position)
    fit = np.full((cap, 2), np.nan)
    pst = np.zeros(cap, np.int32)
    err = np.full((nl, cap), np.nan)
    for p in range(cap):
        if p >= picket_count:
            pst[p] = 1
            continue
        kept = meas[:, p]
        if kept.sum() < 2 or np.ptp(up_px[kept]) == 0:
            pst[p] = 2
            continue
        coef = np.polyfit(up_px[kept], position[kept, p], 1)
        fit[p] = coef
        err[kept, p] = (position[kept, p] - np.poly1d(coef)(center_px[kept])) / dpmm
    a = np.abs(err)
    flat = a.ravel()                                           # leaf-major, then picket: the order of the reference's mlc_meas
    vals = flat[~np.isnan(flat)]
    n = len(vals)
    passed_window = (a < tolerance).astype(np.uint8)           # (NaN compares False)
    summary = np.full(8, np.nan)
    summary[0], summary[6] = n, 0.0
    if n:
        first = int(np.nanargmax(flat))
        summary[1] = vals.max()
        summary[2] = leaf_nums[first // cap]
        summary[3] = first % cap
        summary[4] = np.median(vals)
        under = int((vals < tolerance).sum())
        summary[5] = 100 * under / n
        summary[6] = float(under == n)
        if action_tolerance is not None:
            summary[7] = 100 * int((vals < action_tolerance).sum()) / n
    return dict(fit=fit, picket_status=pst, error=err, passed_window=passed_window, summary=summary)


# ---------------------------------------------------------------------------------------------------------- golden cases
def golden_frames(golden):
    """the seven goldens that carry their frame: (tag, cropped frame, dpmm, mlc, orientation, the reference's max_error)"""
    g = golden("picketfence")
    for k in (0, 1):
        yield f"millennium{k}", g[f"{k}.cropped"], float(g[f"{k}.dpmm"]), "MILLENNIUM", "UP_DOWN", float(g[f"{k}.max_error"])
    g = golden("picketfence_mlc")
    for name, mlc, tr in zip(g["names"], g["mlcs"], g["transposed"]):
        name = str(name)
        yield (name, g[f"{name}.cropped"], float(g[f"{name}.dpmm"]), str(mlc), "LEFT_RIGHT" if bool(tr) else "UP_DOWN",
               float(g[f"{name}.max_error"]))


_ORACLE = {}


def oracle_table(tag, raw, dpmm, mlc, orient):
    """(position [L, P], status, leaf numbers) of the oracle's measurement, computed once per golden frame"""
    if tag not in _ORACLE:
        r = o.pf_measure(o.normalize(o.ground(raw)), dpmm, mlc=mlc, orientation=orient)
        pos = r["position"]
        _ORACLE[tag] = (pos, np.where(np.isnan(pos), 2, 0).astype(np.int32), [n for n, _, _ in r["leaves"]])
    return _ORACLE[tag]


def restate_golden(tag, raw, dpmm, mlc, orient):
    pos, st, nums = oracle_table(tag, raw, dpmm, mlc, orient)
    gn, c_px, u_px = geometry(raw.shape, dpmm, mlc, orient)
    assert gn == nums
    return restate(pos, st, pos.shape[1], nums, c_px, u_px, dpmm)


def bench_size_tables(golden):
    """config #3's four 768 x 1024 frames: the position tables rebuilt from what the reference measured and kept
    (pf.k.meas: leaf, picket, position, approximate index) -> (k, position [L, 10], status, nums, centres, ups, dpmm, max_error)"""
    g = golden("bench_size")
    dpmm = 1 / float(g["pf.pixel_mm"])
    nums, c_px, u_px = geometry((768, 1024), dpmm)
    idx = {n: i for i, n in enumerate(nums)}
    for k in range(4):
        meas = g[f"pf.{k}.meas"]
        pos = np.full((len(nums), 10), np.nan)
        for leaf, picket, p, _ in meas:
            pos[idx[int(leaf)], int(picket)] = p
        yield k, pos, np.where(np.isnan(pos), 2, 0).astype(np.int32), nums, c_px, u_px, dpmm, float(g[f"pf.{k}.max_error"])


# ------------------------------------------------------------------------------------------------------- synthetic tables
def plain_bank(nl):
    """`nl` leaves of 5 mm, all in view of a 1024-row frame at 2.56 pixels per mm (a custom leaf arrangement, as the
    reference's ``MLCArrangement``): the table sizes of the sweep do not depend on what a named bank shows.  Two and three
    leaves are one of 10 mm followed by 5 mm ones.  A line through two leaves of ONE width leaves no errors but rounding noise,
    and three equally spaced leaves of one width leave the outer two the same error: nothing a maximum's place could be
    read from.  With two widths the upper markers sit 5.12 and 2.56 pixels from the centres, so a picket tilted by t has the
    errors 5.12 t and 2.56 t pixels on two leaves, and three leaves are not equally spaced"""
    mlc = [(1, 10.0), (nl - 1, 5.0)] if nl <= 3 else [(nl, 5.0)]
    return dict(mlc=mlc, orientation="UP_DOWN", shape=(1024, 1280), dpmm=2.56)


HD = dict(mlc="HD_MILLENNIUM", orientation="UP_DOWN", shape=(404, 524), dpmm=2.564102564102564)      # two leaf widths in view
AGILITY_LR = dict(mlc="AGILITY", orientation="LEFT_RIGHT", shape=(508, 388), dpmm=2.0)


def synthetic_table(n, cap, c_px, seed, holes=True):
    """position [n, len(c_px), cap] = a tilted line per picket + noise of a few hundredths of a pixel, status 0; with `holes`
    about a tenth of the windows are taken out (NaN, status 2)"""
    rng = np.random.default_rng(seed)
    nl = len(c_px)
    base = 60.0 + 37.5 * np.arange(cap)
    tilt = rng.uniform(-2e-3, 2e-3, (n, 1, cap))
    pos = base[None, None, :] + tilt * (c_px[:, None] - c_px.mean())[None] + rng.normal(0.0, 0.03, (n, nl, cap))
    st = np.zeros((n, nl, cap), np.int32)
    if holes and nl > 3:
        out = rng.random((n, nl, cap)) < 0.1
        pos[out] = np.nan
        st[out] = 2
    return pos, st


class Case:
    """a bank, a table on its leaves in view and the tolerances; `want` = the restatement per frame, computed once"""

    def __init__(self, tag, bank, n, cap, seed, tolerance=0.012, action_tolerance=None, holes=True, count=None):
        self.tag, self.bank = tag, bank
        self.nums, self.c_px, self.u_px = geometry(bank["shape"], bank["dpmm"], bank["mlc"], bank["orientation"])
        self.dpmm = bank["dpmm"]
        self.pos, self.st = synthetic_table(n, cap, self.c_px, seed, holes)
        self.count = np.asarray([cap] * n if count is None else count, np.int32)
        self.tolerance, self.action_tolerance = tolerance, action_tolerance
        self.kw = dict(bank, tolerance=tolerance, action_tolerance=action_tolerance)
        self._want = None

    @property
    def want(self):
        if self._want is None:
            self._want = [restate(self.pos[i], self.st[i], int(self.count[i]), self.nums, self.c_px, self.u_px, self.dpmm,
                                  self.tolerance, self.action_tolerance) for i in range(len(self.pos))]
        return self._want


SIZES = [(nl, cap, n) for nl in (2, 3, 63, 64, 65, 80) for cap in (1, 10, 16) for n in (1, 3)]
_CASES = {}


def _once(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def size_case(nl, cap, n):
    """the size sweep; the tolerance (0.012 mm) sits inside the noise (0.03 px = 0.0117 mm) so that windows fall on both sides
    of it, the action tolerance below it"""
    def make():
        case = Case(("size", nl, cap, n), plain_bank(nl), n, cap, seed=1000 * nl + 10 * cap + n, action_tolerance=0.006)
        assert len(case.nums) == nl
        return case

    return _once(("size", nl, cap, n), make)


def bank_case(which):
    """the HD Millennium (leaves of two widths in view) and the Agility with LEFT_RIGHT pickets, 2 frames x 10 slots"""
    return _once(("bank", which), lambda: Case(("bank", which), {"hd": HD, "agility_lr": AGILITY_LR}[which], 2, 10,
                                               seed={"hd": 31, "agility_lr": 32}[which], action_tolerance=0.006))


def special_case():
    """3 frames x the HD Millennium's leaves in view x 10 slots: frame 0 has a picket with exactly ONE measured leaf (status
    2), two with exactly TWO (slot 5 upright: errors 0; slot 6 tilted: the line goes through both upper markers and is read at the
    centres, 1.28 pixels further, so both errors are -slope * 1.28 px) and 8 of 10 slots in use; frame 1 has picket_count = 0;
    frame 2 is all NaN"""
    def make():
        case = Case("special", HD, 3, 10, seed=77, count=[8, 0, 10])
        pos, st = case.pos, case.st
        assert len(case.nums) > 20 and case.c_px[4] - case.c_px[3] != case.c_px[18] - case.c_px[17]
        pos[0, 1:, 2] = np.nan                                 # slot 2: leaf 0 only
        st[0, 1:, 2] = 2
        pos[0, :, 5] = np.nan                                  # slot 5: leaves 12 and 17
        st[0, :, 5] = 2
        pos[0, 12, 5], pos[0, 17, 5] = 247.25, 247.25
        st[0, 12, 5] = st[0, 17, 5] = 0
        pos[0, :, 6] = np.nan                                  # slot 6: the same two leaves, tilted
        st[0, :, 6] = 2
        pos[0, [12, 17], 6] = 284.75, 285.0
        st[0, [12, 17], 6] = 0
        assert case.c_px[12] - case.u_px[12] == case.c_px[17] - case.u_px[17]
        pos[0, :, 8:] = np.nan
        st[0, :, 8:] = 1
        pos[1], st[1] = np.nan, 1
        pos[2], st[2] = np.nan, 2
        return case

    return _once("special", make)


def parity_case():
    """even and odd n_measured on one geometry (13 leaves x 3 pickets, no holes: 39; one window out: 38)"""
    def make():
        case = Case("parity", plain_bank(13), 2, 3, seed=5, holes=False, action_tolerance=0.006)
        case.pos[1, 4, 1], case.st[1, 4, 1] = np.nan, 2
        return case

    return _once("parity", make)


TIE_D = np.array([0.0, 0.125, -0.25, 0.125, -0.125, 0.25, -0.125, 0.0])
TIE_SCALE = (0.5, 1.0, 0.5)


def tie_case():
    """a table mirrored about its lines, in numbers every step of the fit represents exactly: 8 leaves of 5 mm at 2 pixels
    per mm (centres and upper markers are integers, 10 apart), positions = an upright line plus scale_p * TIE_D[k].  TIE_D is
    antisymmetric about the middle of the table with sum(d) = sum(d * x) = 0, so the fitted line IS that line (Sxy = 0) and
    the error of window (k, p) is scale_p * TIE_D[k] / 2 exactly: leaves 2 and 5 of slot 1 tie for the maximum, and the first
    in leaf-major order is leaf index 2"""
    def make():
        case = Case("tie", dict(mlc=[(8, 5.0)], orientation="UP_DOWN", shape=(128, 512), dpmm=2.0), 1, 3, seed=0,
                    tolerance=0.5, holes=False)
        assert np.array_equal(case.c_px, 64.0 + 10.0 * np.arange(8) - 35.0) and np.array_equal(case.u_px, case.c_px - 2.0)
        for p, scale in enumerate(TIE_SCALE):
            case.pos[0, :, p] = 128.0 + 64.0 * p + scale * TIE_D
        return case

    return _once("tie", make)


# --------------------------------------------------------------------------------------------------------- device checks
def run(case, dev, frames=None):
    """evaluate_batch on the case's table (or on `frames` of it) through a hand-made PFBatchResult"""
    import torch

    from pylinac_amd import picketfence as ppf

    sel = slice(None) if frames is None else frames
    pos, st, cnt = case.pos[sel], case.st[sel], case.count[sel]
    n, nl, cap = pos.shape
    res = ppf.PFBatchResult(list(case.nums), torch.zeros((n, cap), dtype=torch.int32, device=dev),
                            torch.from_numpy(cnt).to(dev), torch.zeros(n, dtype=torch.float64, device=dev),
                            torch.from_numpy(np.ascontiguousarray(pos)).to(dev), torch.from_numpy(np.ascontiguousarray(st)).to(dev))
    return ppf.evaluate_batch(res, **case.kw)


def snapshot(got):
    return {k: getattr(got, k).cpu().numpy().copy() for k in ("fit", "picket_status", "error", "passed_window", "summary")}


def assert_margins(case):
    """on the restatement: no |error| within 1e-8 of a tolerance, the two largest |errors| more than 1e-8 apart"""
    for i, w in enumerate(case.want):
        a = np.abs(w["error"]).ravel()
        a = np.sort(a[~np.isnan(a)])
        for t in (case.tolerance, case.action_tolerance):
            if t is not None and len(a):
                assert np.abs(a - t).min() > GAP, (case.tag, i, "an |error| sits on the tolerance", t)
        if len(a) >= 2:
            assert a[-1] - a[-2] > GAP, (case.tag, i, "the two largest |errors| are too close")


def assert_matches(case, snap, frames=None, tag=""):
    from pylinac_amd import picketfence as ppf

    assert tuple(ppf.PF_SUMMARY_FIELDS) == FIELDS
    idx = range(len(case.pos)) if frames is None else range(len(case.pos))[frames]
    for k, i in enumerate(idx):
        w, t = case.want[i], (case.tag, tag, "frame", i)
        assert np.array_equal(snap["picket_status"][k], w["picket_status"]), (t, snap["picket_status"][k], w["picket_status"])
        e, we = snap["error"][k], w["error"]
        assert np.array_equal(np.isnan(e), np.isnan(we)), (t, "NaN pattern of the errors")
        ok = ~np.isnan(we)
        if ok.any():
            worst = float(np.abs(e[ok] - we[ok]).max())
            assert worst <= BOUND_MM, (t, "error", worst)
        assert np.array_equal(snap["passed_window"][k], w["passed_window"]), (t, "passed_window")
        f, wf = snap["fit"][k], w["fit"]
        assert np.array_equal(np.isnan(f), np.isnan(wf)), (t, "NaN pattern of the fits")
        for p in np.flatnonzero(w["picket_status"] == 0):
            for c in (case.c_px[0], case.c_px[-1]):
                dv = abs((f[p, 0] * c + f[p, 1]) - (wf[p, 0] * c + wf[p, 1]))
                assert dv <= BOUND_PX, (t, "fit", p, dv)
        s, ws = snap["summary"][k], w["summary"]
        assert np.array_equal(np.isnan(s), np.isnan(ws)), (t, "NaN pattern of the summary", s, ws)
        for name in ("n_measured", "max_error_leaf", "max_error_picket", "percent_passing", "passed", "percent_under_action"):
            j = FIELDS.index(name)
            assert s[j] == ws[j] or (np.isnan(s[j]) and np.isnan(ws[j])), (t, name, s[j], ws[j])
        for name in ("max_error", "abs_median_error"):
            j = FIELDS.index(name)
            if not np.isnan(ws[j]):
                assert abs(s[j] - ws[j]) <= BOUND_MM, (t, name, s[j], ws[j])


def check_size(dev, nl, cap, n):
    case = size_case(nl, cap, n)
    assert_margins(case)
    assert_matches(case, snapshot(run(case, dev)))
    below = np.concatenate([w["passed_window"][~np.isnan(w["error"])] for w in case.want])
    if nl > 2 and below.size >= 20:
        assert 0 < below.sum() < below.size                    # the tolerance splits the windows


def check_special(dev):
    case = special_case()
    assert_margins(case)
    w = case.want
    assert list(w[0]["picket_status"]) == [0, 0, 2, 0, 0, 0, 0, 0, 1, 1]
    assert np.isnan(w[0]["error"][:, 2]).all() and np.isnan(w[0]["fit"][2]).all()
    two = w[0]["error"][[12, 17], 5]
    assert np.abs(two).max() <= BOUND_MM and np.isnan(np.delete(w[0]["error"][:, 5], [12, 17])).all()
    slope = (case.pos[0, 17, 6] - case.pos[0, 12, 6]) / (case.u_px[17] - case.u_px[12])
    tilted = -slope * (case.c_px[12] - case.u_px[12]) / case.dpmm
    assert abs(tilted) > 1e-6 and np.abs(w[0]["error"][[12, 17], 6] - tilted).max() <= BOUND_MM
    assert (w[1]["picket_status"] == 1).all() and (w[2]["picket_status"] == 2).all()
    for i in (1, 2):
        assert w[i]["summary"][0] == 0 and w[i]["summary"][6] == 0 and np.isnan(np.delete(w[i]["summary"], [0, 6])).all()
    snap = snapshot(run(case, dev))
    assert_matches(case, snap)
    assert np.abs(snap["error"][0][[12, 17], 5]).max() <= BOUND_MM


def check_parity(dev):
    case = parity_case()
    assert_margins(case)
    assert [int(w["summary"][0]) for w in case.want] == [39, 38]
    assert_matches(case, snapshot(run(case, dev)))


def check_bank(dev, which):
    case = bank_case(which)
    assert_margins(case)
    if which == "hd":
        assert len(set(np.round(np.diff(case.c_px), 6))) > 2       # 5 mm leaves, 2.5 mm leaves and the step between them
        assert len(set(np.round(case.c_px - case.u_px, 9))) == 2   # the upper marker is no affine function of the centre
    assert_matches(case, snapshot(run(case, dev)))


def check_tie(dev):
    case = tie_case()
    exact = TIE_D[:, None] * np.asarray(TIE_SCALE)[None, :] / 2.0
    w = case.want[0]
    assert np.abs(w["error"] - exact).max() <= BOUND_MM and w["summary"][0] == 24
    snap = snapshot(run(case, dev))
    e = snap["error"][0]
    assert np.array_equal(e, exact), "the mirrored table's errors are not the exact ones"
    assert abs(e[2, 1]) == abs(e[5, 1]) == np.abs(e).max() and (np.abs(e) == np.abs(e).max()).sum() == 2
    s = snap["summary"][0]
    assert s[FIELDS.index("max_error")] == 0.125
    assert s[FIELDS.index("max_error_leaf")] == case.nums[2] and s[FIELDS.index("max_error_picket")] == 1, s
    assert s[FIELDS.index("abs_median_error")] == np.median(np.abs(exact))
    assert np.array_equal(snap["fit"][0], [[0.0, 128.0], [0.0, 192.0], [0.0, 256.0]])


def _bits_equal(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)


def check_independence(dev):
    """frame i alone == frame i inside the batch, and two runs of the batch, bit for bit"""
    for case in (size_case(65, 10, 3), special_case()):
        whole = snapshot(run(case, dev))
        assert _bits_equal(whole, snapshot(run(case, dev))), (case.tag, "two runs differ")
        for i in range(len(case.pos)):
            alone = snapshot(run(case, dev, frames=slice(i, i + 1)))
            assert _bits_equal(alone, {k: v[i:i + 1] for k, v in whole.items()}), (case.tag, "frame", i, "alone differs")


def check_limits_and_validation(dev):
    import pytest
    import torch

    from pylinac_amd import picketfence as ppf
    from pylinac_amd._lib import PylinacHipError

    case = size_case(3, 10, 1)
    good = dict(case.kw)

    def result(nl, cap, nums, **extra):
        return ppf.PFBatchResult(list(nums), torch.zeros((1, cap), dtype=torch.int32, device=dev),
                                 torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float64, device=dev),
                                 torch.full((1, nl, cap), float("nan"), dtype=torch.float64, device=dev),
                                 torch.ones((1, nl, cap), dtype=torch.int32, device=dev), **extra)

    nums = size_case(80, 1, 1).nums
    big = dict(good, **plain_bank(80))
    ppf.evaluate_batch(result(80, 51, nums), **big)                                # 4080 windows: the largest table
    with pytest.raises(PylinacHipError, match="4096"):
        ppf.evaluate_batch(result(80, 52, nums), **big)                            # 4160
    with pytest.raises(ValueError, match="leaf_nums"):
        ppf.evaluate_batch(result(3, 10, [n + 1 for n in case.nums]), **good)
    z = torch.zeros((1, 3, 10), dtype=torch.float64, device=dev)
    with pytest.raises(NotImplementedError):
        ppf.evaluate_batch(result(3, 10, case.nums, left=z, right=z), **good)
    for bad in (0.012, 0.5):
        with pytest.raises(ValueError, match="action_tolerance"):
            ppf.evaluate_batch(result(3, 10, case.nums), **dict(good, action_tolerance=bad))
    with pytest.raises(ValueError, match="tolerance"):
        ppf.evaluate_batch(result(3, 10, case.nums), **dict(good, tolerance=0.0, action_tolerance=None))
    # the entry point itself: a null pointer and a table beyond 4096 windows return 1 and leave a text
    from pylinac_amd import _lib

    lib = _lib.load()
    assert lib.pl_pf_errors(None, None, None, 1, 3, 10, None, None, None, 1.0, 0.5, float("nan"), None, None, None, None, None,
                            None) == 1 and b"pl_pf_errors" in lib.pl_last_error()
    t = torch.zeros(8, dtype=torch.float64, device=dev)
    p = t.data_ptr()
    assert lib.pl_pf_errors(p, p, p, 1, 65, 64, p, p, p, 1.0, 0.5, float("nan"), p, p, p, p, p, None) == 1
    assert b"4096" in lib.pl_last_error()


def check_end_to_end(golden, dev, tags=None):
    """evaluate_batch(analyze_batch(frame)) on the golden frames: the reference's max_error within 1e-9 mm, the restatement's
    leaf and picket"""
    import torch

    from pylinac_amd import picketfence as ppf

    seen = 0
    for tag, raw, dpmm, mlc, orient, max_error in golden_frames(golden):
        if tags is not None and tag not in tags:
            continue
        seen += 1
        res = ppf.analyze_batch(torch.from_numpy(np.ascontiguousarray(raw)[None]).to(dev), dpmm, mlc=mlc, orientation=orient)
        got = ppf.evaluate_batch(res, raw.shape, dpmm, mlc=mlc, orientation=orient)
        s = got.summary[0].cpu().numpy()
        want = restate_golden(tag, raw, dpmm, mlc, orient)["summary"]
        assert want[1] == max_error, (tag, "the restatement left the golden")
        assert abs(s[1] - max_error) <= BOUND_MM, (tag, s[1], max_error)
        assert s[0] == want[0] and s[2] == want[2] and s[3] == want[3], (tag, s, want)
        assert s[5] == 100.0 and s[6] == 1.0 and np.isnan(s[7]), (tag, s)
        assert abs(s[4] - want[4]) <= BOUND_MM
    assert seen == (7 if tags is None else len(tags))
