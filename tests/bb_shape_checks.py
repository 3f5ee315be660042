"""The BB finder on a zoo of shapes (tests/golden/bb_shapes.npz, tests/golden/make_bb_shapes_golden.py): the checks shared by
tests/test_gpu_bb_shapes.py (MI355X), tests/test_emulated_bb_shapes.py (the CPU emulator, a subset) and the oracle pin in
tests/test_oracle_golden.py.

Every window goes through ``find_features_batch`` three ways -- the default call, ``level_by_level=True`` and
``defer=True`` (the sweep kernel alone) -- and is held to ``oracle.find_features_restated`` on the same sample: count,
first level, the points in the oracle's ORDER to rtol 1e-12, and the status word as include/pylinac_hip.h documents it:

    0  everywhere except
    3  the sweep alone on ``tall67`` (a candidate taller than its 64-pixel crop); the default call redoes that window on
       the level path and reports the oracle's answer with 0
    4  more than 8 features (``many.discs10``, and ``dedup`` with min_separation 0): count 8, the oracle's first eight
    2  ``many.blobs40``: more than 32 candidates at a level.  The kernels then analyse the FIRST 32 in label (raster) order
       and nothing else of that level, so the answer is ``truncated_reference`` below, not the oracle's: a feature behind
       the 32nd candidate is lost at that level and found at a later one only if the sweep goes on."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
from scipy import ndimage

from oracle import pylinac_oracle as o

XY_RTOL = 1e-12
MAX_OUT = 8                     # features the kernels report per window
MAX_CAND = 32                   # candidates they analyse per level
EMULATED = ("rows31_32_33", "holes", "edges.solid", "edges.area_lo")        # the emulator takes 10-20 s per window


def names(g):
    return [str(n) for n in g["names"]]


def sweep_cutoffs():
    out, cutoff = [], 0.0 + 1.0 / 50
    while cutoff <= 1.0:
        out.append(cutoff)
        cutoff += 1.0 / 50
    return out


# ------------------------------------------------------------------------------------------------ references
def _passes_cheap_test(p, h, w, dpmm, radius, tol):
    """the kernels' candidate test: the conditions on (area, bbox) alone that every accepted region satisfies"""
    r0, c0, r1, c1 = p["bbox"]
    if r0 == 0 or c0 == 0 or r1 == h or c1 == w:
        return False
    y, x = r1 - r0, c1 - c0
    return bool(p["area"] / dpmm**2 < np.pi * (radius + tol) ** 2
                and p["bbox_area"] / dpmm**2 > max(np.pi * (radius - tol) ** 2, 2)
                and not (x > max(y * 1.05, y + 3) or x < min(y * 0.95, y - 3))
                and p["area"] / p["bbox_area"] < np.pi / 4 * 1.2)


def truncated_reference(sample, dpmm, radius, tol, max_number, min_separation_mm, limit=MAX_CAND):
    """oracle.find_features_restated with the documented table limit: per level only the first ``limit`` candidates in
    label order are analysed.  -> (points, first level, truncated anywhere)"""
    s = o.stretch(sample, min=0, max=1)
    total, found, cut_short = [], -1, False
    for level, cutoff in enumerate(sweep_cutoffs()):
        if len(total) >= max_number:
            break
        lab, n = ndimage.label(s > cutoff)
        cand = []
        for k in range(1, n + 1):
            rr, cc = np.nonzero(lab == k)
            box = dict(area=len(rr), bbox=(rr.min(), cc.min(), rr.max() + 1, cc.max() + 1))
            box["bbox_area"] = (box["bbox"][2] - box["bbox"][0]) * (box["bbox"][3] - box["bbox"][1])
            if _passes_cheap_test(box, *s.shape, dpmm, radius, tol):
                cand.append(k)
        cut_short |= len(cand) > limit
        for k in cand[:limit]:
            p = o.region_props_like_skimage(lab, k, s)
            if not o.bb_predicates(p, dpmm, radius, tol):
                continue
            pt = (p["weighted_centroid"][1], p["weighted_centroid"][0])
            if all(math.hypot(pt[0] - q[0], pt[1] - q[1]) >= min_separation_mm * dpmm for q in total):
                total.append(pt)
                found = level if found < 0 else found
    return total, found, cut_short


@functools.lru_cache(maxsize=None)
def _reference_cached(key, maxn, minsep, truncated):
    sample, prm = _reference_cached.samples[key]
    if truncated:
        pts, level, cut = truncated_reference(sample, *prm, maxn, minsep)
        assert cut, "the window is there for the candidate table's limit"
        full = o.find_features_restated(sample, *prm, max_number=maxn, min_separation_mm=minsep)[0]
        # max_number 1: the level that completes the sweep loses the disc behind the 32nd candidate.  max_number 2: the sweep goes
        # on and finds it once the diamonds have left the mask -- the oracle's points, reached later
        assert len(pts) < len(full) if maxn == 1 else len(pts) == len(full) == 2, "the truncation must lose the last disc"
        return np.array(pts, dtype=float).reshape(-1, 2), level
    try:
        pts, level = o.find_features_restated(sample, *prm, max_number=maxn, min_separation_mm=minsep)
    except ValueError:                       # "Couldn't find the minimum number of disks": the batch reports count 0
        pts, level = [], -1
    return np.array(pts, dtype=float).reshape(-1, 2), level


_reference_cached.samples = {}


def reference(key, sample, prm, maxn, minsep, truncated=False):
    """the oracle's (points [k, 2], first level) for one window and run; computed once per session"""
    _reference_cached.samples[key] = (sample, tuple(prm))
    return _reference_cached(key, int(maxn), float(minsep), bool(truncated))


def expected_status(name, ref_count, path):
    """``path``: "default", "levels" or "sweep" (defer=True: the sweep kernel's own word)"""
    if name == "many.blobs40":
        return 2
    if name == "tall67" and path == "sweep":
        return 3
    return 4 if ref_count > MAX_OUT else 0


def _assert_result(res, i, ref_pts, ref_level, status, what, zero_tail=True):
    count = min(len(ref_pts), MAX_OUT)
    got = (int(res["status"][i]), int(res["count"][i]), int(res["level"][i]))
    assert got == (status, count, ref_level), (what, "status, count, level", got, "expected", (status, count, ref_level))
    xy = res["xy"][i].cpu().numpy()
    assert np.allclose(xy[:count], ref_pts[:count], rtol=XY_RTOL, atol=0), (what, xy[:count], ref_pts[:count])
    if zero_tail:
        assert not xy[count:].any(), (what, "slots past count are zero")


# ------------------------------------------------------------------------------------------------ float64 windows
def check_window(dev, g, name):
    """one window of the golden, every run of it, the three ways"""
    from pylinac_amd import features as pf

    window, prm = g[f"{name}.window"], tuple(float(v) for v in g[f"{name}.params"])
    x = torch.from_numpy(window[None].copy()).to(dev)
    for maxn, minsep in g[f"{name}.runs"]:
        maxn, minsep = int(maxn), float(minsep)
        ref_pts, ref_level = reference(name, window, prm, maxn, minsep, truncated=name == "many.blobs40")
        kw = dict(max_number=maxn, min_separation_mm=minsep)
        what = (name, maxn, minsep)
        default = pf.find_features_batch(x, *prm, **kw)
        levels = pf.find_features_batch(x, *prm, level_by_level=True, **kw)
        sweep = pf.find_features_batch(x, *prm, defer=True, **kw)
        _assert_result(default, 0, ref_pts, ref_level, expected_status(name, len(ref_pts), "default"), what + ("default",))
        _assert_result(levels, 0, ref_pts, ref_level, expected_status(name, len(ref_pts), "levels"), what + ("levels",))
        if expected_status(name, len(ref_pts), "sweep") == 3:
            assert int(sweep["status"][0]) == 3, what + ("sweep",)        # handed back: its points are the caller's to redo
            assert len(ref_pts) == 1                                       # ... and the level path accepted the tall disc
        else:
            _assert_result(sweep, 0, ref_pts, ref_level, expected_status(name, len(ref_pts), "sweep"), what + ("sweep",))
        if int(default["status"][0]) == 0 and int(levels["status"][0]) == 0:
            for key in ("xy", "count", "level"):
                assert torch.equal(default[key], levels[key]), what + (key, "default vs level by level")


# ------------------------------------------------------------------------------------------------ uint16 frames
def u16_sample(frame, dpmm, diameter, low_density):
    """the float64 sample WLBaseImage.find_bb_centroids hands to find_features (oracle.wl_analyze_frame's window) and the
    window's (top, bottom, left, right) in the frame"""
    arr = o.normalize(o.ground(frame.astype(np.float64)))
    win = (40 + diameter) * dpmm
    ex, ey = frame.shape[1] / 2, frame.shape[0] / 2
    left, right = max(math.floor(ex - win / 2), 0), min(math.ceil(ex + win / 2), frame.shape[1])
    top, bottom = max(math.floor(ey - win / 2), 0), min(math.ceil(ey + win / 2), frame.shape[0])
    sample = arr[top:bottom, left:right]
    return (sample if low_density else o.invert(sample)), (top, bottom, left, right)


def check_u16(dev, g, ks):
    """frames ``ks`` (one shape) in one batch through bb_centroids_batch -- pl_features_sweep_u16 -- with low_density False
    and True, and through the separate kernels (_bb_sample + find_features_batch, both paths)"""
    from pylinac_amd import features as pf
    from pylinac_amd import ops

    dpmm, diameter = (float(v) for v in g["u16.params"])
    tol = float(np.interp(diameter, (1.5, 30), (2, 4)))
    frames = np.stack([g[f"u16.{k}.frame"] for k in ks])
    x = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    found = 0
    for low in (False, True):
        refs = []
        for k, frame in zip(ks, frames):
            sample, win = u16_sample(frame, dpmm, diameter, low)
            pts, level = reference(f"u16.{k}.{low}", sample, (dpmm, diameter / 2, tol), 1, 5.0)
            refs.append((pts, level))
            found += len(pts)
        top, bottom, left, right = win
        off = np.array([left, top], dtype=float)
        for defer in (False, True):
            res = pf.bb_centroids_batch(x, dpmm, diameter, low_density=low, defer=defer)
            assert res["window"] == win
            for i, (pts, level) in enumerate(refs):
                # (after the shift to frame coordinates the slots past count hold the offsets: they are not looked at)
                _assert_result(res, i, pts + off if len(pts) else pts, level, 0, ("u16", ks[i], low, defer), zero_tail=False)
        unshifted = pf.bb_centroids_batch(x, dpmm, diameter, low_density=low, shift=False)
        vmin, vmax = ops.minmax(x)
        sample = pf._bb_sample(x, top, bottom, left, right, vmin.to(torch.float64).contiguous(),
                               vmax.to(torch.float64).contiguous(), low)
        for i, frame in enumerate(frames):                    # the separate kernels build the oracle's sample, bit for bit
            assert np.array_equal(sample[i].cpu().numpy(), u16_sample(frame, dpmm, diameter, low)[0]), ("sample", ks[i], low)
        for lbl in (False, True):
            res = pf.find_features_batch(sample, dpmm, diameter / 2, tol, level_by_level=lbl)
            for i, (pts, level) in enumerate(refs):
                _assert_result(res, i, pts, level, 0, ("u16 sample", ks[i], low, lbl))
            for key in ("xy", "count", "level", "status"):     # ... and the fused uint16 sweep is bit-identical to them
                assert torch.equal(res[key], unshifted[key]), ("u16 fused vs separate", ks, low, lbl, key)
    assert found == 2 * len(ks)                                # a BB for either polarity in every frame


# ------------------------------------------------------------------------------------------------ the oracle, pinned
def check_oracle_pinned(g):
    """oracle.region_props_like_skimage == scikit-image 0.18.3's regionprops on every stored region (integers exact; perimeter,
    solidity, centroid to 1e-12 relative), and ndimage.label + border removal yields exactly the stored region set"""
    dpmm, diameter = (float(v) for v in g["u16.params"])
    samples = {name: g[f"{name}.window"] for name in names(g)}
    for k in range(3):
        for tag, low in (("inv", False), ("low", True)):
            samples[f"u16.{k}.{tag}"] = u16_sample(g[f"u16.{k}.frame"], dpmm, diameter, low)[0]
    checked = 0
    for name, sample in samples.items():
        table = g[f"{name}.levels"]
        s = o.stretch(sample, 0, 1)
        prev, seen = None, set()
        for lvl, cutoff in enumerate(sweep_cutoffs()):
            bw = s > cutoff
            if prev is not None and np.array_equal(bw, prev):
                continue
            prev = bw
            lab, n = ndimage.label(bw)
            border = set(np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]])).tolist())
            areas = np.bincount(lab.ravel(), minlength=n + 1)
            seen |= {(lvl, k) for k in range(1, n + 1) if k not in border and areas[k] >= 4}
            for row in table[table[:, 0] == lvl]:
                p = o.region_props_like_skimage(lab, int(row[1]), s)
                assert (p["area"], p["filled_area"], p["convex_area"]) == (row[2], row[3], row[9]), (name, lvl, row[1])
                assert tuple(p["bbox"]) == tuple(row[4:8]), (name, lvl, row[1])
                assert abs(p["perimeter"] - row[8]) <= 1e-12 * row[8], (name, lvl, row[1], p["perimeter"], row[8])
                assert abs(p["solidity"] - row[10]) <= 1e-12 * row[10], (name, lvl, row[1])
                assert np.allclose(p["weighted_centroid"], row[11:13], rtol=1e-12, atol=0), (name, lvl, row[1])
                checked += 1
        assert seen == {(int(r[0]), int(r[1])) for r in table}, (name, "region set")
    assert checked == sum(len(g[f"{n}.levels"]) for n in samples) and checked > 400
    assert any("scikit-image 0.18.3" in str(v) for v in g["versions"])
