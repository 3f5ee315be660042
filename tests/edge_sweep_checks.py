"""Edge sweeps through the host layer, shared by tests/test_gpu_edge_sweeps.py (MI355X) and tests/test_emulated_kernels.py (the
CPU emulator of tests/hipemu).  Every function takes `dev` and calls pylinac_amd.ops / profile / winston_lutz / xim / gamma /
picketfence, so the same inputs reach the library that hipcc built for the device and the one the emulator built for the host.

The emulator alone is not evidence for these inputs: it runs the work-items of a launch one after another (no race can happen
in the union-find of ccl.hip or in an LDS flood fill), tests/hipemu/build.py rewrites every line of inline assembly before it
compiles (the instructions themselves never run there), and it is host clang at -O1 with one emulated CU.

References: scipy.ndimage / numpy / the oracle, compared with array_equal unless a function says otherwise.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import pylinac_oracle as orc

STENCIL_SHAPES = ((1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (5, 64), (64, 5), (9, 33), (17, 66), (33, 130), (40, 2))
STENCIL_DTYPES = (np.uint16, np.int16, np.uint8, np.int32, np.float32, np.float64)


def _t(a, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _report(failures, what):
    assert not failures, f"{what}: {len(failures)} mismatches, first: " + "; ".join(failures[:12])


# ---- Gaussian / median / Sobel on frames smaller than the stencil ------------------------------------------------

def check_stencils_awkward(dev, dtypes=STENCIL_DTYPES):
    """ops.gaussian_filter (sigma 1, 2, 3, 5, 6), ops.median_filter (size 1, 2, 3, 4, 5, 7) and, for float64, ops.sobel on both
    axes, on two frames of every shape of STENCIL_SHAPES: one-pixel, one-row and one-column frames, frames smaller than the
    stencil (halos that reflect more than once), widths either side of the packed kernels' vectors.  Integers are drawn over
    the whole range of the type, floats are normal * 50.  Equal to scipy for every case."""
    from scipy import ndimage

    from pylinac_amd import ops

    failures = []
    for dt in dtypes:
        dt = np.dtype(dt)
        rng = np.random.default_rng([12, STENCIL_DTYPES.index(dt.type)])
        for h, w in STENCIL_SHAPES:
            if dt.kind == "f":
                f = (rng.normal(size=(2, h, w)) * 50).astype(dt)
            else:
                info = np.iinfo(dt)
                f = rng.integers(info.min, info.max, (2, h, w), endpoint=True).astype(dt)
            t = _t(f, dev)
            for sigma in (1, 2, 3, 5, 6):
                want = np.stack([orc.filter(a, sigma, "gaussian") for a in f])
                if not np.array_equal(ops.gaussian_filter(t, sigma).cpu().numpy(), want):
                    failures.append(f"gaussian {dt.name} {h}x{w} sigma {sigma}")
            for size in (1, 2, 3, 4, 5, 7):
                want = np.stack([orc.filter(a, size, "median") for a in f])
                if not np.array_equal(ops.median_filter(t, size).cpu().numpy(), want):
                    failures.append(f"median {dt.name} {h}x{w} size {size}")
            if dt == np.float64:
                for axis in (0, 1):
                    want = np.stack([ndimage.sobel(a, axis=axis) for a in f])
                    if not np.array_equal(ops.sobel(t, axis).cpu().numpy(), want):
                        failures.append(f"sobel {h}x{w} axis {axis}")
            if not np.array_equal(t.cpu().numpy(), f):
                failures.append(f"input written {dt.name} {h}x{w}")
    _report(failures, "stencils")


# ---- labelling, hole filling, clear_border, centroid -----------------------------------------------------------------

def label_masks():
    """random masks of several densities and shapes (frame sizes that are / are not multiples of the 64-lane chunk),
    plus structured ones: solid, a frame with one hole, stripes, a checkerboard, staircases, a spiral"""
    rng = np.random.default_rng(6)
    out = []
    for shape in ((2, 45, 61), (3, 16, 64), (2, 33, 130), (1, 70, 7), (2, 1, 200), (2, 9, 1)):
        for dens in (0.15, 0.45, 0.6, 0.9):
            out.append((rng.random(shape) < dens).astype(np.uint8))
    h, w = 40, 150
    solid = np.ones((1, h, w), np.uint8)
    ring = solid.copy(); ring[0, 10:30, 20:120] = 0; ring[0, 15:25, 40:100] = 1
    stripes_v = np.zeros((1, h, w), np.uint8); stripes_v[0, :, ::3] = 1
    stripes_h = np.zeros((1, h, w), np.uint8); stripes_h[0, ::2, :] = 1
    checker = (np.indices((h, w)).sum(0) % 2).astype(np.uint8)[None]
    stairs = np.zeros((1, h, w), np.uint8)
    for k in range(h):
        stairs[0, k, max(0, 3 * k - 4):3 * k + 2] = 1
    anti = stairs[:, :, ::-1].copy()
    spiral = np.zeros((1, 41, 41), np.uint8)
    r, c, dr, dc, n = 0, 0, 0, 1, 41
    seg = [41, 40, 40, 38, 38, 36, 36, 34, 34, 32, 32, 30, 30, 28, 28, 26, 26, 24, 24, 22, 22]
    for k, length in enumerate(seg):
        for _ in range(length - (0 if k == 0 else 1)):
            spiral[0, r, c] = 1
            r, c = r + dr, c + dc
        r, c = r - dr, c - dc
        dr, dc = dc, -dr
        r, c = r + dr, c + dc
    out += [solid, ring, stripes_v, stripes_h, checker, stairs, anti, spiral, 1 - spiral, 1 - ring]
    return out


def _serpentine(h, w):
    """even rows full, odd rows one pixel at alternating ends: ONE component rooted at pixel 0 whose last pixel is h*w/2 links
    away, every row joined to the next through a single pixel"""
    m = np.zeros((h, w), np.uint8)
    m[::2] = 1
    m[1::4, w - 1] = 1
    m[3::4, 0] = 1
    return m


def _comb(h, w):
    """teeth on the even columns, the bar in the LAST row: every tooth is its own tree until the last row joins them all"""
    m = np.zeros((h, w), np.uint8)
    m[:, ::2] = 1
    m[h - 1] = 1
    return m


def _rings(h, w):
    """concentric square rings, two pixels on and two off: holes inside holes"""
    r, c = np.indices((h, w))
    d = np.minimum(np.minimum(r, h - 1 - r), np.minimum(c, w - 1 - c))
    return (d % 4 < 2).astype(np.uint8)


def _band(h, w):
    """three pixels per row starting at column 3 * row mod w: consecutive rows touch through the upper-LEFT diagonal only (one
    component per row at connectivity 4, long chains at 8); mirrored, through the upper-right one"""
    m = np.zeros((h, w), np.uint8)
    r = np.arange(h)
    for k in range(3):
        m[r, (3 * r + k) % w] = 1
    return m


# base masks of the contention zoo; each goes in as the batch [m, 1 - m, m rotated by 180 degrees]
CONTENTION = {
    "serpentine": _serpentine,
    "serpentine_t": lambda h, w: np.ascontiguousarray(_serpentine(w, h).T),
    "comb": _comb,
    "comb_flip": lambda h, w: np.ascontiguousarray(_comb(h, w)[::-1]),
    "checker": lambda h, w: (np.indices((h, w)).sum(0) % 2).astype(np.uint8),   # every pixel a root at connectivity 4
    "rings": _rings,
    "band": _band,
    "band_mirror": lambda h, w: np.ascontiguousarray(_band(h, w)[:, ::-1]),
}
# neither pixel count is a multiple of 64: with three frames in a call the 64-lane run chunks of ccl_init_kernel cut rows
# and frames at different lanes in every frame
CONTENTION_SIZES = ((97, 200), (130, 67))
BIG_SIZE = (513, 520)       # 800 thousand pixels, > 3 000 workgroups per launch: the whole device merges into one forest


def contention_batch(name, h, w):
    m = CONTENTION[name](h, w)
    assert m.shape == (h, w) and m.dtype == np.uint8
    return np.ascontiguousarray(np.stack([m, 1 - m, m[::-1, ::-1]]))


def _check_mask_batch(dev, mask, tag, failures):
    from scipy import ndimage

    from pylinac_amd import ops

    n = mask.shape[0]
    t = _t(mask, dev)
    for conn in (4, 8):
        lab, cnt = ops.label(t, conn)
        lab, cnt = lab.cpu().numpy(), cnt.cpu().numpy()
        for f in range(n):
            want, num = orc.label_like_skimage(mask[f], conn)
            if int(cnt[f]) != num:
                failures.append(f"label count {tag} conn {conn} frame {f}: {int(cnt[f])} for {num}")
            if not np.array_equal(lab[f], want):
                failures.append(f"label {tag} conn {conn} frame {f}: {int((lab[f] != want).sum())} pixels")
    for conn, structure in ((4, None), (8, np.ones((3, 3)))):
        got = ops.fill_holes(t, conn).cpu().numpy()
        for f in range(n):
            # scipy's `structure` is the connectivity of the hole-growing step, i.e. of the BACKGROUND
            want = ndimage.binary_fill_holes(mask[f], structure=structure)
            if not np.array_equal(got[f], want.astype(np.uint8)):
                failures.append(f"fill_holes {tag} conn {conn} frame {f}: {int((got[f] != want).sum())} pixels")
    for buf in (0, 1, 3):
        got = ops.clear_border(t, buf).cpu().numpy()
        for f in range(n):
            want = orc.clear_border_like_skimage(mask[f].astype(bool), buf)
            if not np.array_equal(got[f], want.astype(np.uint8)):
                failures.append(f"clear_border {tag} buffer {buf} frame {f}: {int((got[f] != want).sum())} pixels")
    cen = ops.binary_centroid(t).cpu().numpy()
    for f in range(n):
        rr, cc = np.nonzero(mask[f])
        k = len(rr)
        want = [rr.sum() / k, cc.sum() / k, k] if k else [np.nan, np.nan, 0.0]     # an empty mask: 0 / 0, like scipy
        if not np.array_equal(cen[f], want, equal_nan=True):
            failures.append(f"centroid {tag} frame {f}: {cen[f].tolist()} for {want}")
    if not np.array_equal(t.cpu().numpy(), mask):
        failures.append(f"input written {tag}")


def check_label_zoo(dev, big=False, only=None):
    """ops.label (4 / 8, plane and count) against the oracle's skimage numbering, ops.fill_holes (4 / 8) against
    scipy.ndimage.binary_fill_holes, ops.clear_border (buffer 0, 1, 3) against the oracle and ops.binary_centroid against exact
    integer sums.  big=False: every mask of label_masks() and the contention zoo (CONTENTION) at CONTENTION_SIZES.  big=True:
    the contention zoo at BIG_SIZE only.  `only` names the contention shapes to run (default: all)."""
    failures = []
    names = list(CONTENTION) if only is None else list(only)
    with np.errstate(invalid="ignore"):
        if big:
            for name in names:
                _check_mask_batch(dev, contention_batch(name, *BIG_SIZE), f"{name} {BIG_SIZE[0]}x{BIG_SIZE[1]}", failures)
        else:
            for k, mask in enumerate(label_masks()):
                _check_mask_batch(dev, mask, f"zoo[{k}] {mask.shape}", failures)
            for h, w in CONTENTION_SIZES:
                for name in names:
                    _check_mask_batch(dev, contention_batch(name, h, w), f"{name} {h}x{w}", failures)
    _report(failures, "label zoo")


# ---- find_peaks ------------------------------------------------------------------------------------------------------

def check_find_peaks_sweep(dev):
    """pl_find_peaks through the host layer on short, flat, plateau-rich and noisy profiles with the argument
    combinations the analyzers use: indices exact, properties to 1e-12 of scipy.signal.find_peaks (the oracle calls it
    as the reference does).  Profiles whose peaks tie exactly on the sort key are skipped (np.argsort's tie order)."""
    from pylinac_amd import profile

    rng = np.random.default_rng(21)
    profs = [np.array([0.0, 1, 0]), np.array([0.0, 1, 1, 0]), np.array([1.0, 1, 1, 1]), np.array([0.0, 2, 1, 2, 0, 3, 0]),
             np.arange(9.0), np.array([0.0, 1, 2, 3, 4, 3, 2, 1, 0])]
    for L in (5, 12, 63, 64, 65, 200, 1030):
        for _ in range(3):
            profs.append(np.round(rng.random(L) * 20) / 4)                       # plateaus and ties
            x = np.linspace(0, 1, L)
            profs.append(sum(np.exp(-0.5 * ((x - c) / 0.03) ** 2) * a for c, a in ((0.2, 1.0), (0.5, 0.7), (0.8, 1.3)))
                         + rng.normal(0, 0.01, L))
    rng2 = np.random.default_rng(22)          # either side of the one-wave-per-profile limit (128 samples), no exact ties
    for L in (127, 128, 129):
        x = np.linspace(0, 1, L)
        profs.append(rng2.random(L))
        profs.append(sum(np.exp(-0.5 * ((x - c) / 0.03) ** 2) * a for c, a in ((0.2, 1.0), (0.5, 0.7), (0.8, 1.3)))
                     + rng2.normal(0, 0.01, L))
    combos = [dict(), dict(threshold=0.3, peak_separation=0.05), dict(threshold=0.5, peak_separation=3, max_number=2),
              dict(fwxm_height=0.8, max_number=1), dict(threshold=0.1, required_prominence=0.2, peak_sort="peak_heights"),
              dict(search_region=(0.2, 0.9), threshold=0.2), dict(min_width=2, peak_separation=0.02)]
    checked = 0
    for v in profs:
        for kw in combos:
            try:
                widx, wprops = orc.find_peaks(v, **kw)
            except (IndexError, ValueError) as exc:
                with pytest.raises(type(exc)):
                    profile.find_peaks(v, **kw)
                continue
            key = wprops[kw.get("peak_sort", "prominences")]
            if len(np.unique(key)) != len(key) or len(np.unique(wprops["peak_heights"])) != len(key):
                continue
            idx, props = profile.find_peaks(v, **kw)
            np.testing.assert_array_equal(idx, widx, err_msg=f"{len(v)} {kw}")
            for k in ("peak_heights", "prominences", "left_ips", "right_ips", "widths", "width_heights"):
                np.testing.assert_allclose(props[k], wprops[k], rtol=1e-12, atol=1e-12, err_msg=f"{k} {len(v)} {kw}")
            for k in ("left_bases", "right_bases"):
                np.testing.assert_array_equal(props[k], wprops[k], err_msg=f"{k} {len(v)} {kw}")
            checked += 1
    assert checked > 150
    # the FWXM search (max_number = 1 by prominence, no filter) takes a short cut through the search; with a prominence bound of
    # zero -- which no peak fails -- the same call takes the general path: same peak, exact ties on the prominence included
    same = 0
    for v in [p for p in profs if len(p) <= 200] + [profs[-1]]:
        for kw in (dict(max_number=1), dict(max_number=1, fwxm_height=0.3, peak_separation=2)):
            a_idx, a = profile.find_peaks(v, **kw)
            b_idx, b = profile.find_peaks(v, required_prominence=0.0, **kw)
            np.testing.assert_array_equal(a_idx, b_idx, err_msg=f"{len(v)} {kw}")
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{k} {len(v)} {kw}")
            same += len(a_idx)
    assert same > 50


# ---- reductions, Otsu, percentiles, circle profiles ------------------------------------------------------------------

def check_reductions_sweep(dev):
    """Axis reductions, min/max, Otsu, percentiles and circle profiles on small odd shapes and several dtypes against
    numpy / the oracle."""
    import torch

    from pylinac_amd import ops

    rng = np.random.default_rng(33)
    for h, w in ((1, 1), (1, 9), (9, 1), (3, 65), (65, 3), (17, 31), (40, 128)):
        for dt in (np.uint16, np.int16, np.float32, np.float64, np.uint8):
            if np.issubdtype(dt, np.integer):
                info = np.iinfo(dt)
                f = rng.integers(info.min, info.max, (2, h, w)).astype(dt)
            else:
                f = (rng.normal(size=(2, h, w)) * 50).astype(dt)
            t = torch.from_numpy(f).to(dev)
            mn, mx = ops.minmax(t)
            assert np.array_equal(mn.cpu().numpy(), f.reshape(2, -1).min(1)) and np.array_equal(mx.cpu().numpy(), f.reshape(2, -1).max(1))
            for axis in (0, 1):
                for op, fn in (("sum", np.sum), ("mean", np.mean), ("max", np.max), ("min", np.min)):
                    got = ops.reduce_axis(t, axis, op).cpu().numpy()
                    want = fn(f if dt == np.float32 else f.astype(np.float64), axis=axis + 1)
                    if np.issubdtype(dt, np.integer) or op in ("max", "min"):
                        assert np.array_equal(got, want), (dt, h, w, axis, op)
                    elif dt == np.float32:      # numpy accumulates float32 sums in float32 (pairwise): a few ulps
                        assert np.allclose(got, want, rtol=2e-6, atol=1e-4), (dt, h, w, axis, op)
                    else:
                        assert np.allclose(got, want, rtol=1e-12, atol=1e-12), (dt, h, w, axis, op)
            if dt in (np.uint16, np.int16) and h * w >= 9:
                thr = ops.threshold_otsu(t).cpu().numpy()
                want = np.array([orc.threshold_otsu(a) for a in f])
                assert np.array_equal(thr, want), (dt, h, w, thr, want)
                qs = [0, 5, 37.5, 50, 99.9, 100]
                got = ops.percentile(t, qs).cpu().numpy()
                assert np.array_equal(got, np.stack([np.percentile(a, qs) for a in f])), (dt, h, w)
    # circle profiles: centres near / outside the border, radii that leave the frame (out-of-bounds samples read 0)
    img = rng.integers(0, 60000, (1, 37, 53)).astype(np.uint16)
    t = torch.from_numpy(img).to(dev)
    for cx, cy, r in ((26.2, 18.7, 9.5), (3.0, 4.0, 7.0), (50.5, 35.5, 11.0), (-4.0, 10.0, 8.0), (26.0, 18.0, 40.0)):
        size = np.pi * r * 2
        got = ops.circle_profile(t, cx, cy, [r], size)[0].cpu().numpy()
        want = orc.circle_profile(img[0], (cx, cy), r).astype(np.float64)
        assert np.array_equal(got, want), (cx, cy, r)
        radii = np.linspace(r * 0.9, r * 1.1, 5)
        got = ops.circle_profile(t, cx, cy, radii, np.pi * radii.max() * 2, 0, True, 5.0)[0].cpu().numpy()
        want = orc.collapsed_circle_profile(img[0], (cx, cy), r, width_ratio=0.1, num_profiles=5)
        assert np.allclose(got, want, rtol=1e-13, atol=1e-9), (cx, cy, r)


# ---- random picket-fence frames --------------------------------------------------------------------------------------

def check_pf_random_frames(dev):
    """analyze_batch (scaled column mean, picket peaks, leaf x picket windows, FWXM positions) on random picket-fence
    frames -- picket count, spacing, gap, pixel size, frame size, hidden rows -- against the oracle's per-image loop
    (pinned to the reference's own PicketFence.analyze): same NaN pattern, identical positions."""
    import torch

    from pylinac_amd import picketfence as ppf
    from tests.golden.make_golden import pf_frame

    rng = np.random.default_rng(88)
    for k in range(6):
        pixel = float(rng.choice([0.78125, 0.6, 1.0]))
        h, w = int(rng.integers(120, 200)), int(rng.integers(260, 420))
        n_pickets = int(rng.integers(3, 8))
        spacing = float(rng.uniform(18, 30))
        frame = pf_frame(h + 8, w + 8, pixel, 4000 + k, n_pickets=n_pickets, spacing_mm=spacing,
                         gap_mm=float(rng.uniform(1.5, 3.5)))[4:-4, 4:-4]
        frame = np.ascontiguousarray(frame)
        res = ppf.analyze_batch(torch.from_numpy(frame[None]).to(dev), 1 / pixel)
        ref = orc.pf_measure(orc.normalize(orc.ground(frame)), 1 / pixel)
        P = len(ref["peak_idxs"])
        assert int(res.picket_count[0]) == P, (k, P)
        pos = res.position[0, :, :P].cpu().numpy()
        assert np.array_equal(np.isnan(pos), np.isnan(ref["position"])), k
        assert np.array_equal(pos[~np.isnan(pos)], ref["position"][~np.isnan(pos)]), k
    # leaf heights either side of the column-median networks: MLCi leaves (10 mm) at 0.4 mm -> 25 rows (32-value network),
    # at 0.26 mm -> 38 rows (beyond the networks: rank counting), Millennium at 0.8 mm -> 6 / 12 rows (16-value network)
    for k, (pixel, mlc, h, w) in enumerate([(0.4, "MLCI", 150, 300), (0.26, "MLCI", 160, 360), (0.8, "MILLENNIUM", 130, 280)]):
        frame = pf_frame(h + 8, w + 8, pixel, 4100 + k, n_pickets=4, spacing_mm=w * pixel / 6, gap_mm=3.0)[4:-4, 4:-4]
        frame = np.ascontiguousarray(frame)
        res = ppf.analyze_batch(torch.from_numpy(frame[None]).to(dev), 1 / pixel, mlc=mlc)
        ref = orc.pf_measure(orc.normalize(orc.ground(frame)), 1 / pixel, mlc=mlc)
        P = len(ref["peak_idxs"])
        assert int(res.picket_count[0]) == P and P >= 3, (k, P)
        pos = res.position[0, :, :P].cpu().numpy()
        assert np.isfinite(pos).sum() >= P, k
        assert np.array_equal(np.isnan(pos), np.isnan(ref["position"])), k
        assert np.array_equal(pos[~np.isnan(pos)], ref["position"][~np.isnan(pos)]), k


# ---- random Winston-Lutz fields, XIM images, gamma_2d pairs ----------------------------------------------------------

def check_wl_xim_gamma_random(dev):
    """Three more randomised audits: the WL field CAX (percentile threshold -> fill holes -> centre of mass) on random
    field / BB geometries, XIM decoding of random images whose differences need 1-, 2- and 4-byte codes, and gamma_2d on
    random dose pairs -- all against the pinned restatements, exact."""
    import torch

    from pylinac_amd import gamma as pg
    from pylinac_amd import winston_lutz, xim

    rng = np.random.default_rng(99)
    # ---- WL field CAX
    frames = []
    for k in range(5):
        h, w = int(rng.integers(90, 160)), int(rng.integers(90, 160))
        yy, xx = np.mgrid[0:h, 0:w]
        cy, cx, half = rng.integers(35, h - 35), rng.integers(35, w - 35), int(rng.integers(10, 25))
        img = np.where((abs(yy - cy) < half) & (abs(xx - cx) < half), 42000, 1500).astype(np.int64)
        bb = ((yy - cy - rng.integers(-4, 5)) ** 2 + (xx - cx - rng.integers(-4, 5)) ** 2) < rng.integers(9, 40)
        img[bb] = 11000
        img = img + rng.integers(0, 300, img.shape)
        frames.append(img.astype(np.uint16))
    for f in frames:
        got = winston_lutz.field_centroids_batch(torch.from_numpy(f[None]).to(dev))[0].cpu().numpy()
        want = orc.wl_field_centroid(f)
        assert np.allclose(got, want, rtol=0, atol=1e-9), (got, want)
    # ---- XIM
    for k, (h, w, step) in enumerate(((23, 31, 90), (40, 17, 20000), (9, 64, 3000000))):
        img = np.cumsum(rng.integers(-step, step, (h, w)), axis=1)
        img = (img + rng.integers(-step, step, (h, 1))).astype(np.int32)
        lut, stream = orc.xim_encode(img)
        out = xim.decode_xim_pixels(lut, stream, w, h, 4, device=dev).cpu().numpy()
        assert np.array_equal(out, img), k
    # ---- gamma_2d
    for k in range(3):
        ref = rng.uniform(0, 100, (20 + k, 24)) * (rng.random((20 + k, 24)) > 0.05)
        ev = ref * rng.uniform(0.95, 1.05, ref.shape)
        kw = dict(dose_to_agreement=float(rng.choice([1, 2, 3])), distance_to_agreement=int(rng.integers(1, 4)),
                  gamma_cap_value=2, global_dose=bool(k % 2), dose_threshold=float(rng.choice([0, 5, 10])))
        got = pg.gamma_2d(ref, ev, device=dev, **kw).cpu().numpy()
        want = orc.gamma_2d(ref, ev, **kw)
        assert np.array_equal(got, want, equal_nan=True), kw
