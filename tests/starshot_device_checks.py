"""Checks of starshot.wobble_batch / pl_starshot_wobble -- LineManager's lines and focus test, the wobble circle by a replay of
scipy's Nelder-Mead, the accept test -- shared by tests/test_emulated_starshot_device.py (CPU emulator) and
tests/test_gpu_starshot_device.py (MI355X).

The reference of every check is the class path of this package on the host: ``Line.distance_to`` under
``scipy.optimize.minimize(method="Nelder-Mead", options={"fatol": 0.001})``, ``LineManager`` and ``Starshot._accept``.  The fit
is compared with EQUALITY: the replay either takes scipy's comparisons or it does not, and a one-ulp difference that flips one
of them moves the stopping point by about 1e-3 px."""
from __future__ import annotations

import functools

import numpy as np
import torch
from scipy import optimize

from pylinac_amd import starshot as ss
from pylinac_amd.image import ArrayImage
from pylinac_amd.profile import Point

N_RANDOM = 300
CHUNKS = 6                            # the random table is checked in six parts of 50 sets: scipy's side takes ~2 s per part


# ------------------------------------------------------------------------------------------------------------ host reference
class _Profile:
    def __init__(self, peaks, center):
        self.peaks, self.center = peaks, center


class _Meta:
    def __init__(self, dpmm):
        self.dpmm = dpmm


def host_accept(points, focus, dpmm, max_wobble_diameter=2.0, tolerance=1.0, recursive=True):
    """``Starshot._accept`` on the host for one dataset -> (fit_status, analyzer): the status ``pl_starshot_wobble`` must
    report (4 has no host counterpart) and the ``Starshot`` that holds lines / wobble."""
    a = object.__new__(ss.Starshot)
    a.image, a.wobble, a.tolerance = _Meta(dpmm), ss.Wobble(), tolerance
    fp = Point(x=focus[0], y=focus[1])
    a.circle_profile = _Profile([Point(x=p[0], y=p[1]) for p in points], fp)
    try:
        ok = a._accept(fp, recursive, max_wobble_diameter)
    except ValueError:
        return 2, a
    except RuntimeError:                      # recursive=False and the lines were not detected
        return 1, a
    n = len(points)
    if n < 6 or n % 2:
        return 1, a
    return (0 if ok else 3), a


def scipy_fit(points, focus):
    """The reference's optimiser over this package's ``Line.distance_to`` -> x, y, fun, nit, nfev."""
    nl = len(points) // 2
    lines = [ss.Line(points[k], points[k + nl]) for k in range(nl)]

    def distance(p, lines):
        return max(line.distance_to(Point(x=p[0], y=p[1])) for line in lines)

    res = optimize.minimize(distance, np.array([focus[0], focus[1], 0.0]), args=(lines,), method="Nelder-Mead",
                            options={"fatol": 0.001})
    return float(res.x[0]), float(res.x[1]), float(res.fun), int(res.nit), int(res.nfev)


def spokes(rng, n_lines):
    """``n_lines`` spokes through a centre in 200-900 px, each shifted sideways by 1-2 px, as a peak list (first ends, then far
    ends: ``peaks[k]`` pairs with ``peaks[k + n / 2]``) and an integer start point near the centre."""
    cx, cy = rng.uniform(200, 900, 2)
    ang = (np.arange(n_lines) + rng.uniform(-0.3, 0.3, n_lines)) * np.pi / n_lines + rng.uniform(0, np.pi)
    off = rng.uniform(1, 2, n_lines) * rng.choice([-1.0, 1.0], n_lines)
    reach = rng.uniform(100, 180, (2, n_lines))
    px, py = cx - np.sin(ang) * off, cy + np.cos(ang) * off
    first = np.stack([px + np.cos(ang) * reach[0], py + np.sin(ang) * reach[0]], 1)
    far = np.stack([px - np.cos(ang) * reach[1], py - np.sin(ang) * reach[1]], 1)
    focus = np.array([round(cx) + rng.integers(-3, 4), round(cy) + rng.integers(-3, 4)], dtype=float)
    return np.concatenate([first, far]), focus


@functools.lru_cache(maxsize=None)
def random_sets():
    """The seeded table: every line count from 3 to 32 once, the other 270 sets with the 3-8 lines a star shot has."""
    rng = np.random.default_rng(20261018)
    counts = np.concatenate([np.arange(3, 33), rng.integers(3, 9, N_RANDOM - 30)])
    rng.shuffle(counts)
    return [spokes(rng, int(c)) for c in counts]


@functools.lru_cache(maxsize=None)
def scipy_answers(chunk):
    """scipy's answers for one part of the table, computed once per process."""
    return [scipy_fit(p, f) for p, f in random_sets()[chunk::CHUNKS]]


def pack(sets, cap=ss.WOBBLE_CAP):
    pts = np.full((len(sets), cap, 2), np.nan)
    cnt = np.zeros(len(sets), np.int32)
    foc = np.zeros((len(sets), 2))
    for i, (p, f) in enumerate(sets):
        p = np.asarray(p, dtype=float).reshape(-1, 2)
        cnt[i] = len(p)
        pts[i, :min(len(p), cap)] = p[:cap]
        foc[i] = f
    return pts, cnt, foc


def run(dev, sets, dpmm, cap=ss.WOBBLE_CAP, **kw):
    pts, cnt, foc = pack(sets, cap)
    res = ss.wobble_batch(torch.from_numpy(pts).to(dev), torch.from_numpy(cnt).to(dev), torch.from_numpy(foc).to(dev), dpmm, **kw)
    return res.record.cpu().numpy(), res.lines.cpu().numpy(), res.fit_status.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------- checks
def check_fit_against_scipy(dev, chunk):
    """x, y, fun, nit and nfev of scipy on one part of the 300 seeded sets of 3-32 lines: equal, bit for bit."""
    sets, ref = random_sets()[chunk::CHUNKS], scipy_answers(chunk)
    rec, lines, st = run(dev, sets, dpmm=3.0, recursive=False)
    assert (st == 0).all()
    bad = [i for i, r in enumerate(ref)
           if not (rec[i, 0] == r[0] and rec[i, 1] == r[1] and rec[i, 2] == r[2] and rec[i, 5] == r[3] and rec[i, 6] == r[4])]
    assert not bad, (len(bad), bad[:5], [(rec[i, [0, 1, 2, 5, 6]].tolist(), ref[i]) for i in bad[:3]])
    for i, (p, _) in enumerate(sets):                                   # the lines are LineManager's
        nl = len(p) // 2
        assert rec[i, 7] == nl
        assert np.array_equal(lines[i, :nl], np.concatenate([p[:nl], p[nl:]], 1))
        assert np.isnan(lines[i, nl:]).all()
    assert {len(p) // 2 for p, _ in random_sets()} == set(range(3, 33)) and len(random_sets()) == N_RANDOM


def constructed_cases():
    """name -> (points, focus, dpmm).  Spokes through about (300, 300) unless the case says otherwise."""
    rng = np.random.default_rng(7)
    base, focus = spokes(rng, 4)
    cases = {}
    # a start coordinate of exactly 0.0: scipy displaces it to 0.00025, not by 5 %
    shift = np.array([focus[0], 0.0])
    cases["zero_start_x"] = (base - shift, focus - shift, 3.0)
    shift = focus.copy()
    cases["zero_start_xy"] = (base - shift, focus - shift, 3.0)
    # all lines parallel (the objective has a valley, not a point)
    par = np.array([[100.0, 299.0], [100.0, 301.5], [100.0, 302.25], [500.0, 299.5], [500.0, 301.0], [500.0, 302.0]])
    cases["parallel"] = (par, np.array([300.0, 300.0]), 3.0)
    # a vertical line among the spokes (Line.m divides by zero; the distance does not)
    vert = np.array([[301.0, 100.0], [100.0, 250.0], [120.0, 420.0], [301.0, 500.0], [500.0, 352.0], [480.0, 190.0]])
    cases["vertical"] = (vert, np.array([300.0, 300.0]), 3.0)
    # a line exactly 10 * dpmm from the focus (kept: the test is a strict >) and one a rounding beyond it (ValueError)
    at = np.array([[100.0, 320.0], [100.0, 250.0], [120.0, 420.0], [500.0, 320.0], [500.0, 352.0], [480.0, 190.0]])
    cases["line_at_limit"] = (at, np.array([300.0, 300.0]), 2.0)
    beyond = at.copy()
    beyond[[0, 3], 1] = np.nextafter(320.0, np.inf)
    cases["line_beyond_limit"] = (beyond, np.array([300.0, 300.0]), 2.0)
    # 4 peaks, 7 peaks: no analysis; 66 peaks: more than the table holds
    cases["four_peaks"] = (base[[0, 1, 4, 5]], focus, 3.0)
    cases["seven_peaks"] = (np.concatenate([base, base[:1] + 40.0])[:7], focus, 3.0)
    big, bfocus = spokes(rng, 33)
    cases["sixty_six_peaks"] = (big, bfocus, 3.0)
    # a diameter EQUAL to max_wobble_diameter: dpmm = the fitted radius in px makes radius_mm exactly 1.0
    fun = scipy_fit(base, focus)[2]
    assert fun / fun * 2 == 2.0
    cases["diameter_at_limit"] = (base, focus, fun)
    cases["diameter_under_limit"] = (base, focus, float(np.nextafter(fun, np.inf)))
    return cases


def check_constructed(dev, recursive):
    """Every constructed case against LineManager and Starshot._accept on the host: status, lines, wobble, passed."""
    cases = constructed_cases()
    names = list(cases)
    # what each case is FOR (the host decides the rest): the line at the limit is kept, the one beyond it is not, ...
    expect = {"line_at_limit": (0, 3), "line_beyond_limit": (2,), "four_peaks": (1,), "seven_peaks": (1,),
              "diameter_at_limit": (3,) if recursive else (0,), "diameter_under_limit": (0,)}
    by_dpmm = {}
    for name in names:
        by_dpmm.setdefault(cases[name][2], []).append(name)
    for dpmm, group in by_dpmm.items():
        rec, lines, st = run(dev, [cases[k][:2] for k in group], dpmm, max_wobble_diameter=2.0, tolerance=1.0, recursive=recursive)
        for j, name in enumerate(group):
            pts, focus, _ = cases[name]
            if len(pts) > ss.WOBBLE_CAP:
                assert st[j] == 4 and np.isnan(rec[j, :7]).all() and np.isnan(lines[j]).all(), name
                continue
            want, a = host_accept(pts, focus, dpmm, 2.0, 1.0, recursive)
            assert st[j] == want, (name, st[j], want)
            if name in expect:
                assert st[j] in expect[name], (name, st[j])
            if want in (1, 2):
                assert np.isnan(rec[j, :7]).all(), name
                if want == 1:
                    assert np.isnan(lines[j]).all(), name
                continue
            w = a.wobble
            got = rec[j]
            assert (got[0], got[1], got[2], got[3], got[4]) == (w.center.x, w.center.y, w.radius, w.radius_mm, w.diameter_mm), name
            assert got[7] == len(a.lines) and bool(got[8]) == a.passed, name
            host_lines = np.array([[ln.point1.x, ln.point1.y, ln.point2.x, ln.point2.y] for ln in a.lines.lines])
            assert np.array_equal(lines[j, :len(host_lines)], host_lines) and np.isnan(lines[j, len(host_lines):]).all(), name


def check_goldens(golden, dev):
    """The peaks and start points of tests/golden/starshot.npz (the reference's own run) give the golden wobble within 1e-6,
    the tolerance the drop-in test allows Nelder-Mead across scipy builds; the lines are the golden lines exactly."""
    g = golden("starshot")
    for name in (str(s) for s in g["names"]):
        peaks, circle, wobble = g[f"{name}.peaks"], g[f"{name}.circle"], g[f"{name}.wobble"]
        dpmm = ArrayImage(np.zeros((2, 2), np.uint16), dpi=float(g[f"{name}.dpi"]), sid=1000).dpmm
        rec, lines, st = run(dev, [(peaks[:, 2:4], circle[:2])], dpmm)
        assert st[0] == 0, name
        assert np.allclose(rec[0, :5], wobble, rtol=0, atol=1e-6), (name, rec[0, :5], wobble)
        assert np.array_equal(lines[0, :len(g[f"{name}.lines"])], g[f"{name}.lines"]), name
        assert bool(rec[0, 8]) == bool(g[f"{name}.passed"]) or name == "float", name      # "float" ran with tolerance=0.4


def check_validation(dev):
    import pytest

    pts, cnt, foc = pack([spokes(np.random.default_rng(0), 3)])
    with pytest.raises(ValueError):
        ss.wobble_batch(pts[:, :63], cnt, foc, 3.0)                     # odd cap
    with pytest.raises(ValueError):
        ss.wobble_batch(np.full((1, 66, 2), np.nan), cnt, foc, 3.0)     # cap above 64
    with pytest.raises(ValueError):
        ss.wobble_batch(pts, cnt, foc[:, :1], 3.0)
    with pytest.raises(ValueError):
        ss.wobble_batch(pts, cnt, foc, 0.0)
    empty = ss.wobble_batch(pts[:0], cnt[:0], foc[:0], 3.0)
    assert len(empty) == 0 and tuple(empty.lines.shape) == (0, 32, 4)
    # a table of 65 datasets spans two waves; a row's result does not depend on its neighbours
    sets = random_sets()
    rec_all, _, st_all = run(dev, sets[:65], 3.0)
    rec_one, _, st_one = run(dev, sets[64:65], 3.0)
    assert np.array_equal(rec_all[64], rec_one[0]) and st_all[64] == st_one[0]
    rec_small, lines_small, _ = run(dev, sets[64:65], 3.0, cap=2 * (len(sets[64][0]) // 2))      # a table cut to the dataset
    assert np.array_equal(rec_small[0], rec_one[0]) and not np.isnan(lines_small).any()


# ------------------------------------------------------------------------------------------- the profile tail and end to end
def golden_cases(g):
    """name, frame, dpi, analyze keywords of every golden case that carries a frame of its own."""
    for name in (str(s) for s in g["names"]):
        if f"{name}.frame" in g.files:
            yield name, g[f"{name}.frame"], float(g[f"{name}.dpi"]), eval(str(g[f"{name}.kw"]), {"__builtins__": {}}, {})


def check_tail(golden, dev, names=None):
    """star_tail against StarProfile on the golden frames, fwhm True and False: the number of peaks, their profile indices and
    their image coordinates, bit for bit; so are the processed ring and the roll."""
    from pylinac_amd import ops
    from pylinac_amd.array_utils import _Staged

    g = golden("starshot")
    done = 0
    for name, frame, dpi, kw in golden_cases(g):
        if names and name not in names:
            continue
        s = ss.Starshot(frame.copy(), dpi=dpi, sid=1000)
        s.image.check_inversion_by_histogram(percentiles=[4, 50, 96])
        s.image.ground()
        sx, sy, local_max = g[f"{name}.start"]
        radius, mph = kw.get("radius", 0.85), kw.get("min_peak_height", 0.25)
        ring = ss.StarProfile._ring(s.image.shape[:2], Point(x=sx, y=sy), radius)
        staged = _Staged(s.image.array).t
        vals = ops.circle_profile(staged, ring.center.x, ring.center.y, ring._radii, ring.size, 0, True, 20.0)
        geom = np.array([[ring.radius, ring.center.x, ring.center.y]])
        for fwhm in (True, False):
            # the reference's height for this frame, and a ratio (a value in [0, 1]) on the same ring
            for height in (mph * local_max, 0.3):
                want = ss.StarProfile(s.image, Point(x=sx, y=sy), radius, height, fwhm)
                count, pidx, points, values, roll = ss.star_tail(vals, [height], geom, ring.size, fwhm)
                c = int(count[0])
                assert c == len(want.peaks) and c >= 6, (name, fwhm, c, len(want.peaks))
                assert pidx[0, :c].cpu().tolist() == [int(p.idx) for p in want.peaks], (name, fwhm, "idx")
                assert np.array_equal(points[0, :c].cpu().numpy(), np.array([[p.x, p.y] for p in want.peaks])), (name, fwhm, "points")
                assert np.isnan(points[0, c:].cpu().numpy()).all() and (pidx[0, c:] == -1).all()
                assert np.array_equal(values[0].cpu().numpy(), np.asarray(want.values, dtype=float)), (name, fwhm, "values")
        done += 1
    assert done == (len(names) if names else 5)


def _spoke_frame(shape, centre, amps, width=3.0, base=200.0, noise=10.0, seed=0, first_angle=0.3):
    """len(amps) radiation lines through ``centre``, line k with peak amplitude amps[k], on a noisy background (uint16)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(float)
    img = np.zeros(shape)
    for k, amp in enumerate(amps):
        a = np.pi * k / len(amps) + first_angle
        d = (xx - centre[0]) * np.sin(a) - (yy - centre[1]) * np.cos(a)
        img += amp * np.exp(-0.5 * (d / width) ** 2)
    return np.clip(img + base + rng.normal(0, noise, shape), 0, 65535).astype(np.uint16)


def _blob_frame(shape, seed=5):
    """a bright disc and no spokes: the start point exists, no (radius, peak height) pair finds radiation lines"""
    rng = np.random.default_rng(seed)
    cy, cx = shape[0] // 2, shape[1] // 2
    blob = 1000 + 20000 * np.exp(-(((np.arange(shape[0])[:, None] - cy) ** 2 + (np.arange(shape[1])[None, :] - cx) ** 2) / (2 * 60.0 ** 2)))
    return (blob + rng.integers(0, 3, shape)).astype(np.uint16)


EXACT_FIELDS = ("status", "wobble_center", "wobble_radius", "wobble_radius_mm", "wobble_diameter_mm", "passed", "n_lines",
                "start_point", "local_max", "inverted", "radius", "min_peak_height")


def compare_paths(dev, stack, dpi, expect_status=None, **kw):
    """analyze_batch(analyzers=False) against the default path on one stack, field for field -> (device result, default)."""
    t = torch.from_numpy(np.ascontiguousarray(stack)).to(dev)
    ref = ss.analyze_batch(t, dpi=dpi, sid=1000, **kw)
    got = ss.analyze_batch(t, dpi=dpi, sid=1000, analyzers=False, **kw)
    if expect_status is not None:
        assert ref.status.tolist() == expect_status, ref.status
    for f in EXACT_FIELDS:
        a, b = getattr(got, f), getattr(ref, f)
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (f, a, b)
    assert got.analyzers == [] and ref.lines is None and ref.angles is None and ref.nit is None
    assert got.lines.shape == (len(stack), 32, 4) and got.angles.shape == (len(stack), 32)
    fallback = [i for i in range(len(stack)) if got.status[i] == 0 and got.nit[i] < 0]
    assert not fallback, f"frames {fallback} were finished on the per-frame path: only a ring of more than 64 peaks may be"
    for i, a in enumerate(ref.analyzers):
        if a is None:
            assert np.isnan(got.lines[i]).all() and np.isnan(got.angles[i]).all() and got.nit[i] == -1 and got.nfev[i] == -1
            continue
        nl = len(a.lines)
        lines = np.array([[ln.point1.x, ln.point1.y, ln.point2.x, ln.point2.y] for ln in a.lines.lines])
        assert np.array_equal(got.lines[i, :nl], lines) and np.isnan(got.lines[i, nl:]).all(), (i, "lines")
        assert np.allclose(got.angles[i, :nl], a.angles, rtol=0, atol=1e-9) and np.isnan(got.angles[i, nl:]).all(), (i, "angles")
        assert got.nit[i] > 1 and got.nfev[i] > got.nit[i]
    return got, ref


E2E_STACKS = ("four", "six_off", "inverted", "nofwhm", "shifted8", "retry", "blank", "exhausted")


def check_end_to_end(golden, dev, which):
    g = golden("starshot")
    cases = {name: (frame, dpi, kw) for name, frame, dpi, kw in golden_cases(g) if frame.dtype == np.uint16}
    if which in cases:                                            # a golden frame as a one-frame stack, with its own keywords
        frame, dpi, kw = cases[which]
        got, _ = compare_paths(dev, frame[None], dpi, expect_status=[0], **kw)
        assert np.allclose([*got.wobble_center[0], got.wobble_radius[0]], g[f"{which}.wobble"][:3], rtol=0, atol=1e-6)
    elif which == "shifted8":                                     # one frame shifted by a few pixels: several ring sizes per pass
        frame, dpi, kw = cases["four"]
        shifts = [(0, 0), (3, -2), (-4, 5), (7, 1), (-1, -6), (2, 8), (-9, 3), (5, -7)]
        got, _ = compare_paths(dev, np.stack([np.roll(frame, s, axis=(0, 1)) for s in shifts]), dpi, expect_status=[0] * 8, **kw)
        rings = {ss.StarProfile._ring(frame.shape, Point(x=p[0], y=p[1]), 0.85).size for p in got.start_point}
        assert len(rings) > 1, "the shifts must give more than one ring size"
    elif which == "retry":                                        # a faint third line: 4 peaks at 0.25, 6 at the sweep's 0.05
        frame = _spoke_frame((420, 440), (221.3, 208.6), (3000.0, 3000.0, 400.0))
        got, _ = compare_paths(dev, frame[None], 100, expect_status=[0])
        assert (got.radius[0], got.min_peak_height[0]) != (0.85, 0.25), "the frame must need the retry sweep"
    elif which == "blank":                                        # no FW80M peak in the central third: status 3
        frame = g["inverted.frame"]
        compare_paths(dev, np.stack([np.full_like(frame, 1000), frame]), float(g["inverted.dpi"]), expect_status=[3, 0])
    elif which == "exhausted":                                    # the sweep runs out: status 1; recursive=False: status 2
        blob = _blob_frame((300, 320))
        compare_paths(dev, blob[None], 100, expect_status=[1])
        compare_paths(dev, blob[None], 100, expect_status=[2], recursive=False)
    else:
        raise KeyError(which)


def check_fallback(golden, dev):
    """A ring with more peaks than the table holds (fit_status 4) is finished by the class path for that pass.  The peak
    search keeps peaks 2 % of the ring apart, so no frame reaches 64 peaks: the table is shrunk to 4 peaks here, which sends the
    golden frame's 8 peaks down that path.  Same numbers as the default path; ``nit`` = -1 says which path measured the frame."""
    g = golden("starshot")
    frame, dpi = g["four.frame"], float(g["four.dpi"])
    t = torch.from_numpy(np.stack([frame, np.roll(frame, (2, -3), axis=(0, 1))])).to(dev)
    ref = ss.analyze_batch(t, dpi=dpi, sid=1000)
    cap = ss.WOBBLE_CAP
    ss.WOBBLE_CAP = 4
    try:
        got = ss.analyze_batch(t, dpi=dpi, sid=1000, analyzers=False)
    finally:
        ss.WOBBLE_CAP = cap
    assert ref.status.tolist() == [0, 0] and (ref.n_lines == 4).all()
    for f in EXACT_FIELDS:
        a, b = getattr(got, f), getattr(ref, f)
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (f, a, b)
    assert got.nit.tolist() == [-1, -1] and got.nfev.tolist() == [-1, -1] and got.lines.shape == (2, 2, 4)
    for i, a in enumerate(ref.analyzers):
        lines = np.array([[ln.point1.x, ln.point1.y, ln.point2.x, ln.point2.y] for ln in a.lines.lines])
        assert np.array_equal(got.lines[i], lines[:2]) and np.allclose(got.angles[i], a.angles[:2], rtol=0, atol=1e-9)
