"""Golden of shapes for the BB finder (pl_features_sweep / pl_features_sweep_u16 / pl_features_level): windows that put a
region on each switch, bound and table limit of the kernels, with scikit-image 0.18.3's own region properties of every
region the sweep sees on them (tests/golden/skimage_bb_shapes_py39.py).  Build container only:

    python tests/golden/make_bb_shapes_golden.py        # -> tests/golden/bb_shapes.npz

Every window is float64 in [0, 1]: a 0.2 background, each region a plateau of its own value (so each region leaves the
sweep at a level of its own), noise and blur only where a window says so, seeded.  Each window asserts HERE, with the
oracle, the property it is there for -- 31 / 32 / 33 / 64 / 65+ rows, "rejected by exactly this predicate", accept and
reject on the two sides of a bound, more than 32 candidates, more than 8 features -- so the golden cannot silently stop
covering it.

Keys: ``names``; per window NAME: ``NAME.window``, ``NAME.params`` (dpmm, radius_mm, tolerance_mm), ``NAME.runs``
[(max_number, min_separation_mm)], ``NAME.levels`` (the helper's table); ``u16.K.frame``, ``u16.params`` (dpmm, BB diameter) and, for the
samples the uint16 frames turn into, ``u16.K.inv.levels`` / ``u16.K.low.levels``; ``versions``."""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import pylinac_oracle as o  # noqa: E402

PY39 = "/opt/conda/bin/python3.9"
BG = 0.2
PRED = ("size", "round", "circumference", "symmetric", "solid")


# ---------------------------------------------------------------------------------------------- predicates, one by one
def predicates(p, dpmm, radius, tol):
    """the five conditions of pylinac/metrics/features.py:7-68, separately (oracle.bb_predicates ANDs them)"""
    bb_area = p["filled_area"] / dpmm**2
    size = max((np.pi * (radius - tol) ** 2, 2)) < bb_area < np.pi * (radius + tol) ** 2
    ratio = p["filled_area"] / p["bbox_area"]
    rnd = np.pi / 4 * 1.2 > ratio > np.pi / 4 * 0.8
    per = p["perimeter"] / dpmm
    circ = 2 * np.pi * (radius + tol) > per > 2 * np.pi * (radius - tol)
    y, x = p["bbox"][2] - p["bbox"][0], p["bbox"][3] - p["bbox"][1]
    sym = not (x > max(y * 1.05, y + 3) or x < min(y * 0.95, y - 3))
    return dict(zip(PRED, (bool(size), bool(rnd), bool(circ), bool(sym), bool(p["solidity"] > 0.9))))


def failed(mask, prm):
    """-> (names of the predicates the one-region mask fails, its props)"""
    lab, n = ndimage.label(mask)
    assert n == 1, "a shape is one 4-connected region"
    m = np.pad(mask, 1)
    p = o.region_props_like_skimage(m.astype(int), 1, m.astype(float))
    ok = predicates(p, *prm)
    assert all(ok.values()) == o.bb_predicates(p, *prm)
    return tuple(k for k in PRED if not ok[k]), p


# ---------------------------------------------------------------------------------------------- shapes (cropped masks)
def crop(m):
    rr, cc = np.nonzero(m)
    return m[rr.min():rr.max() + 1, cc.min():cc.max() + 1]


def ellipse(ry, rx, half_y=False, half_x=False):
    n = 2 * int(math.ceil(max(ry, rx))) + 5
    cy, cx = n // 2 + (0.5 if half_y else 0.0), n // 2 + (0.5 if half_x else 0.0)
    yy, xx = np.mgrid[0:n, 0:n]
    return crop(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0)


def disc(r, half=False):
    return ellipse(r, r, half, half)


def rows_disc(rows):
    """a disc whose bbox is exactly ``rows`` rows"""
    m = disc(rows / 2 + 0.47, half=rows % 2 == 0)
    assert m.shape[0] == rows
    return m


def diamond(k):
    yy, xx = np.mgrid[-k:k + 1, -k:k + 1]
    return np.abs(yy) + np.abs(xx) <= k


def ring(r, r_in):
    n = 2 * int(math.ceil(r)) + 5
    yy, xx = np.mgrid[0:n, 0:n] - n // 2
    d2 = yy**2 + xx**2
    return crop((d2 <= r * r) & (d2 > r_in * r_in))


def crescent(r, rho):
    """a disc with a round bite of radius rho centred on its rim at 45 degrees (the bbox stays the disc's)"""
    n = 2 * int(math.ceil(r)) + 5
    yy, xx = np.mgrid[0:n, 0:n] - n // 2
    by = bx = r / math.sqrt(2)
    return crop((yy**2 + xx**2 <= r * r) & ((yy - by) ** 2 + (xx - bx) ** 2 > rho * rho))


def lobed(r, a, n_lobes):
    n = 2 * int(math.ceil(r * (1 + a))) + 5
    yy, xx = np.mgrid[0:n, 0:n] - n // 2
    th = np.arctan2(yy, xx)
    return crop(np.hypot(yy, xx) <= r * (1 + a * np.cos(n_lobes * th)))


def notched(r, removed):
    """a disc of radius r with a 6-pixel slot cut down from its top; ``removed`` pixels of it are taken, in raster order"""
    m = disc(r).copy()
    c = m.shape[1] // 2
    cells = [(y, x) for y in range(m.shape[0]) for x in range(c - 3, c + 3) if m[y, x]][:removed]
    for y, x in cells:
        m[y, x] = False
    return crop(m)


def search(make, grid, want, prm):
    """first parameter tuple of ``grid`` whose shape fails exactly the predicates ``want``"""
    for g in grid:
        m = make(*g)
        if ndimage.label(m)[1] == 1 and failed(m, prm)[0] == want:
            return m, g
    raise AssertionError(f"no {make.__name__} fails exactly {want}")


# ---------------------------------------------------------------------------------------------- windows
class Win:
    def __init__(self, h, w):
        self.a = np.full((h, w), BG)
        self.used = np.zeros((h, w), bool)
        self.at = {}

    def put(self, name, mask, top, left, value):
        h, w = mask.shape
        assert top >= 0 and left >= 0 and top + h <= self.a.shape[0] and left + w <= self.a.shape[1], name
        full = np.zeros_like(self.used)
        full[top:top + h, left:left + w] = mask
        assert not (ndimage.binary_dilation(full, np.ones((3, 3))) & self.used).any(), f"{name} touches another shape"
        self.used |= full
        self.a[full] = value
        r, c = np.argwhere(full)[0]
        self.at[name] = (int(r), int(c))
        return self

    def level0(self, prm):
        """name -> (failed predicates, touches the border, props) at the sweep's first level"""
        s = o.stretch(self.a, 0, 1)
        lab, n = ndimage.label(s > 0.0 + 1 / 50)
        border = set(np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]])).tolist())
        out = {}
        for name, (r, c) in self.at.items():
            k = int(lab[r, c])
            assert k > 0
            p = o.region_props_like_skimage(lab, k, s)
            ok = predicates(p, *prm)
            out[name] = (tuple(q for q in PRED if not ok[q]), k in border, p)
        return out


def passes_cheap_test(p, h, w, dpmm, radius, tol):
    """stage G of the kernels: the necessary conditions on (area, bbox) that make a region a CANDIDATE"""
    r0, c0, r1, c1 = p["bbox"]
    if r0 == 0 or c0 == 0 or r1 == h or c1 == w:
        return False
    y, x = r1 - r0, c1 - c0
    return bool(p["area"] / dpmm**2 < np.pi * (radius + tol) ** 2
                and p["bbox_area"] / dpmm**2 > max(np.pi * (radius - tol) ** 2, 2)
                and not (x > max(y * 1.05, y + 3) or x < min(y * 0.95, y - 3))
                and p["area"] / p["bbox_area"] < np.pi / 4 * 1.2)


def points(win, prm, maxn=8, minsep=5.0):
    try:
        return o.find_features_restated(win, *prm, max_number=maxn, min_separation_mm=minsep)
    except ValueError:
        return [], -1


WINDOWS = {}          # name -> (window, (dpmm, radius_mm, tol_mm), [(max_number, min_separation_mm)])


def add(name, win, prm, runs=((8, 1.0),)):
    a = win.a if isinstance(win, Win) else win
    assert a.dtype == np.float64 and a.min() >= 0 and a.max() <= 1 and max(a.shape) <= 161
    WINDOWS[name] = (a, tuple(float(x) for x in prm), [(int(m), float(s)) for m, s in runs])


def rows_content(h, w):
    """the three discs of 31, 32 and 33 rows in an h x w window: side by side if they fit, else stacked"""
    win = Win(h, w)
    ms = [rows_disc(31), rows_disc(32), rows_disc(33)]
    if w >= 117:
        x = (w - 111) // 2
        for k, m in enumerate(ms):
            win.put(f"rows{m.shape[0]}", m, (h - 33) // 2, x, 1.0 - 0.1 * k)
            x += m.shape[1] + 7
    else:
        y = (h - 111) // 2
        for k, m in enumerate(ms):
            win.put(f"rows{m.shape[0]}", m, y, (w - 33) // 2, 1.0 - 0.1 * k)
            y += m.shape[0] + 7
    return win


def build():
    # ---- rows31_32_33: the switch between the one-wave hull pruning (ch <= 31) and the sequential chains
    prm = (3, 5.2, 1)
    win = rows_content(41, 117)
    v = win.level0(prm)
    for rows in (31, 32, 33):
        fl, brd, p = v[f"rows{rows}"]
        assert fl == () and not brd and p["bbox"][2] - p["bbox"][0] == rows, (rows, fl)
    assert len(points(win.a, prm)[0]) == 3
    add("rows31_32_33", win, prm)

    # ---- tall35_64: accepted regions far taller than a clinical BB, up to the sweep's 64-pixel crop, and one beyond it
    for name, rows, prm in (("tall35", 35, (3, 6, 1)), ("tall64", 64, (3, 32 / 3, 1)), ("tall67", 67, (3, 11, 1.5))):
        m = rows_disc(rows)
        win = Win(rows + 12, rows + 13).put("disc", m, 6, 7, 1.0)
        fl, brd, p = win.level0(prm)["disc"]
        assert fl == () and not brd and p["bbox"][2] - p["bbox"][0] == rows and p["bbox"][3] - p["bbox"][1] == rows
        assert passes_cheap_test(p, *win.a.shape, *prm)
        if rows == 35:
            assert (p["area"], p["convex_area"]) == (1005, 1021), (p["area"], p["convex_area"])
        add(name, win, prm)

    # ---- one_predicate_each: one accepted disc and six shapes, each rejected by exactly ONE predicate
    prm = (3, 6, 1)
    shapes = {"disc": (disc(17.6), ()), "square": (np.ones((30, 30), bool), ("round",)), "diamond": (diamond(20), ("round",)),
              "ellipse": (ellipse(15.4, 15.4 * 1.25), ("symmetric",))}
    shapes["ring"] = (search(ring, [(r, q) for r in np.arange(15.1, 16.6, 0.1) for q in np.arange(4.0, 7.5, 0.1)],
                             ("solid",), prm)[0], ("solid",))
    shapes["crescent"] = (search(crescent, [(r, q) for r in np.arange(16.0, 19.5, 0.25) for q in np.arange(5.0, 10.0, 0.25)],
                                 ("solid",), prm)[0], ("solid",))
    shapes["lobed"] = (search(lobed, [(r, a, n) for n in (12, 10, 8) for r in np.arange(18.0, 20.6, 0.25)
                                      for a in np.arange(0.03, 0.09, 0.005)], ("circumference",), prm)[0], ("circumference",))
    win = Win(150, 150)
    for k, (name, (m, want)) in enumerate(shapes.items()):
        assert max(m.shape) <= 46, (name, m.shape)
        win.put(name, m, 3 + 49 * (k // 3), 3 + 49 * (k % 3), 1.0 - 0.08 * k)
    for name, (fl, brd, p) in win.level0(prm).items():
        assert fl == shapes[name][1] and not brd, (name, fl)
    pts, lvl = points(win.a, prm)
    assert len(pts) == 1 and lvl == 0
    add("one_predicate_each", win, prm)

    # ---- edges_of_predicates: near-identical pairs on the two sides of a bound (accept / reject)
    prm = (3, 5.2, 1)
    for name, centre in (("edges.area_hi", 18.6), ("edges.area_lo", 12.6)):
        cand = {}
        for r in np.arange(centre - 0.8, centre + 0.8, 0.02):
            for half in (False, True):
                m = disc(r, half)
                cand.setdefault(int(m.sum()), m)
        verdict = {a: failed(m, prm)[0] for a, m in cand.items()}
        acc = [a for a in sorted(cand) if verdict[a] == ()]
        hi = name.endswith("hi")
        bound = np.pi * ((5.2 + 1) if hi else (5.2 - 1)) ** 2 * 9
        # (a digital disc's scikit-image perimeter is 1-2 % above 2 pi r and the upper bounds of size and circumference are the
        # same circle, so by the isoperimetric inequality no hole-free shape fails the UPPER size bound alone: there the
        # rejected twin fails both; below, it fails size alone)
        a_in = max(a for a in acc if a < bound) if hi else min(a for a in acc if a > bound)
        a_out = min(a for a in cand if a > bound) if hi else max(a for a in cand if a < bound)
        assert verdict[a_out] == (("size", "circumference") if hi else ("size",)), (name, verdict[a_out])
        assert abs(a_in - a_out) < 0.06 * bound, (name, a_in, a_out)
        win = Win(46, 92).put("in", cand[a_in], 3, 3, 1.0).put("out", cand[a_out], 3, 49, 0.9)
        v = win.level0(prm)
        assert v["in"][0] == () and v["out"][0] == verdict[a_out]
        add(name, win, prm)
    e33, e34 = ellipse(15.2, 16.4, True, False), ellipse(15.2, 17.2, True, True)
    assert e33.shape == (30, 33) and e34.shape == (30, 34)
    win = Win(40, 83).put("in", e33, 5, 4, 1.0).put("out", e34, 5, 44, 0.9)
    v = win.level0(prm)
    assert v["in"][0] == () and v["out"][0] == ("symmetric",)
    add("edges.symmetric", win, prm)
    prm = (3, 5.5, 2)
    k = next(k for k in range(40, 200) if failed(notched(16.4, k), prm)[1]["solidity"] <= 0.9)
    m_in, m_out = notched(16.4, k - 1), notched(16.4, k)
    assert failed(m_in, prm)[0] == () and failed(m_out, prm)[0] == ("solid",) and m_in.sum() - m_out.sum() == 1
    assert 0.9 < failed(m_in, prm)[1]["solidity"] < 0.902
    win = Win(40, 83).put("in", m_in, 4, 4, 1.0).put("out", m_out, 4, 44, 0.9)
    v = win.level0(prm)
    assert v["in"][0] == () and v["out"][0] == ("solid",)
    add("edges.solid", win, prm)

    # ---- holes: filled_area decides.  The disc's own area is below the size bound, its filled area above it: accepted
    # while the hole is enclosed, rejected (by size alone) once background reaches it through a one-pixel slit or through a
    # diagonal, 8-connected-only gap
    prm = (3, 5.35, 1)
    base = disc(13.3)
    c = base.shape[0] // 2
    yy, xx = np.mgrid[0:base.shape[0], 0:base.shape[1]]
    hole = (yy - (c - 7)) ** 2 + (xx - c) ** 2 <= 3.0**2
    closed = base & ~hole
    top_of_hole = int(np.nonzero(hole[:, c])[0].min())
    slit = closed.copy()
    slit[:top_of_hole, c] = False                              # straight up, 4-connected to the outside
    diag = closed.copy()
    y, x = top_of_hole - 1, c + 1                              # up and to the right, touching the hole by a corner only
    while y >= 0 and x < base.shape[1] and base[y, x]:
        diag[y, x] = False
        y, x = y - 1, x + 1
    two = base & ~((yy - c) ** 2 + (xx - (c - 5)) ** 2 <= 2.2**2) & ~((yy - c) ** 2 + (xx - (c + 5)) ** 2 <= 2.2**2)
    win = Win(35, 125)
    for k, (name, m) in enumerate((("closed", closed), ("slit", slit), ("diag", diag), ("two", two))):
        win.put(name, crop(m), 4, 4 + 30 * k, 1.0 - 0.1 * k)
    v = win.level0(prm)
    assert v["closed"][0] == () and v["closed"][2]["filled_area"] > v["closed"][2]["area"]
    assert v["two"][0] == () and v["two"][2]["filled_area"] - v["two"][2]["area"] > 20
    for name in ("slit", "diag"):
        assert v[name][0] == ("size",) and v[name][2]["filled_area"] == v[name][2]["area"], (name, v[name][0])
    # the diagonal gap is closed for a 4-connected background: a hole fill of the wrong connectivity accepts it
    assert ndimage.binary_fill_holes(crop(diag)).sum() > crop(diag).sum()
    add("holes", win, prm)

    # ---- border: clear_border.  Touching a border: rejected, however bright; one pixel away: accepted
    prm = (3, 2.5, 0.5)
    d15 = rows_disc(15)
    assert failed(d15, prm)[0] == ()
    touch = Win(75, 76).put("top", d15, 0, 30, 1.0).put("bottom", d15, 60, 30, 0.95).put("left", d15, 30, 0, 0.9) \
        .put("right", d15, 30, 61, 0.85).put("inner", d15, 30, 30, 0.6)
    v = touch.level0(prm)
    assert all(v[k][1] and v[k][0] == () for k in ("top", "bottom", "left", "right")) and not v["inner"][1]
    assert len(points(touch.a, prm)[0]) == 1
    add("border.touch", touch, prm)
    near = Win(75, 76).put("top", d15, 1, 30, 1.0).put("bottom", d15, 59, 30, 0.95).put("left", d15, 30, 1, 0.9) \
        .put("right", d15, 30, 60, 0.85)
    v = near.level0(prm)
    assert all(not v[k][1] and v[k][0] == () for k in v)
    assert len(points(near.a, prm)[0]) == 4
    add("border.near", near, prm)

    # ---- levels_and_dedup
    runs = ((1, 5), (2, 5), (4, 5), (8, 5), (8, 0), (3, 0))
    # four blurred discs, too large for the size bound at the first level; each shrinks below it at a level of its own
    prm = (3, 5.2, 1)
    win = Win(50, 160)
    for k, val in enumerate((1.0, 0.8, 0.6, 0.4)):
        win.put(f"d{k}", disc(18.4), 6, 3 + 39 * k, val)
    a = np.clip(ndimage.gaussian_filter(win.a, 1.2), 0, 1)
    s = o.stretch(a, 0, 1)
    first = {}
    cutoff = 0.0 + 1 / 50
    for lvl in range(50):
        lab, n = ndimage.label(s > cutoff)
        for k in range(4):
            r, c = win.at[f"d{k}"]
            lbl = int(lab[r + 18, c])                                          # the disc's centre
            if lbl and f"d{k}" not in first and o.bb_predicates(o.region_props_like_skimage(lab, lbl, s), *prm):
                first[f"d{k}"] = lvl
        cutoff += 1 / 50
    assert len(first) == 4 and len(set(first.values())) == 4 and min(first.values()) > 0, first
    assert [len(points(a, prm, m, sep)[0]) for m, sep in runs[:4]] == [1, 2, 4, 4]
    add("levels", a, prm, runs)
    # three small discs, two of them 3 mm apart: the second is a same-level duplicate under min_separation 5, and with
    # min_separation 0 every level appends all three again
    prm = (3, 1.3, 0.5)
    d4 = disc(3.5)
    win = Win(24, 50).put("a", d4, 7, 5, 1.0).put("b", d4, 7, 14, 0.9).put("c", d4, 7, 36, 0.8)
    v = win.level0(prm)
    assert all(v[k][0] == () for k in v)
    pa, pb = v["a"][2]["weighted_centroid"], v["b"][2]["weighted_centroid"]
    assert math.hypot(pa[0] - pb[0], pa[1] - pb[1]) == 9.0                     # 3 mm
    assert [len(points(win.a, prm, m, sep)[0]) for m, sep in runs] == [2, 2, 2, 2, 9, 3]
    add("dedup", win, prm, runs)

    # ---- many_candidates: the tables' limits
    prm = (3, 2.5, 0.5)
    # 40 diamonds that pass the cheap candidate test (and fail the size predicate), between an accepted disc that is FIRST
    # in label order and a brighter one that is LAST: more than 32 candidates at every level the diamonds are part of
    win = Win(100, 150).put("first", d15, 3, 60, 0.9)
    for k in range(40):
        win.put(f"blob{k}", diamond(5), 22 + 14 * (k // 10), 6 + 14 * (k % 10), 0.5)
    win.put("last", d15, 81, 60, 1.0)
    v = win.level0(prm)
    assert sum(passes_cheap_test(p, 100, 150, *prm) for _, _, p in v.values()) == 42
    assert all("size" in v[f"blob{k}"][0] for k in range(40)) and v["first"][0] == () and v["last"][0] == ()
    add("many.blobs40", win, prm, ((1, 5), (2, 5)))
    win = Win(40, 160)
    for k in range(10):
        win.put(f"d{k}", d15, 3 + 19 * (k // 5), 5 + 31 * (k % 5) + 3 * (k // 5), 1.0 - 0.05 * k)
    assert len(points(win.a, prm, 8, 5)[0]) == 10                              # more than the 8 the kernels report
    add("many.discs10", win, prm, ((8, 5),))

    # ---- geometry: h != w, padded level-map rows (w % 4 != 0), the 160 limit and the general path beyond it, and accepted
    # regions across the 64-bit words of the row masks
    prm = (3, 5.2, 1)
    for h, w in ((97, 150), (150, 97), (160, 160), (161, 130)):
        win = rows_content(h, w)
        assert all(fl == () and not brd for fl, brd, _ in win.level0(prm).values())
        add(f"geometry.{h}x{w}", win, prm)
    d32 = rows_disc(32)
    win = Win(40, 160).put("c63", d32, 4, 48, 1.0).put("c127", d32, 4, 112, 0.9)
    v = win.level0(prm)
    assert [v[k][2]["weighted_centroid"][1] for k in ("c63", "c127")] == [63.5, 127.5] and all(x[0] == () for x in v.values())
    add("geometry.words", win, prm)

    # ---- u16: uint16 frames through bb_centroids_batch: a BB inside a field, darker than it (the usual BB: the window is
    # inverted) and brighter than it (low_density=True: no inversion).  dpmm 3.5: the (40 + 5) mm window is 158 px, and the
    # 150-row frame clips it top and bottom
    rng = np.random.default_rng(20261)
    frames = []
    for k, (h, w, dy, dx) in enumerate(((400, 400, 4.3, -6.6), (400, 400, -9.2, 3.1), (150, 400, 5.7, 8.4))):
        yy, xx = np.mgrid[0:h, 0:w]
        f = np.full((h, w), 5000.0)
        f[(abs(yy - h / 2) <= 50) & (abs(xx - w / 2) <= 50)] = 40000.0
        f[(yy - h / 2 - dy) ** 2 + (xx - w / 2 - dx) ** 2 <= 8.75**2] = 28000.0           # the BB low_density=False finds
        f[(yy - h / 2 + dy * 3) ** 2 + (xx - w / 2 + dx * 3) ** 2 <= 8.75**2] = 52000.0   # ... and low_density=True
        g = ndimage.gaussian_filter(f, 1.5) + rng.integers(-4, 5, size=(h, w))
        frames.append(np.clip(np.rint(g), 0, 65535).astype(np.uint16))
    return frames


def u16_sample(frame, dpmm, low_density):
    """the float64 sample find_bb_centroids hands to find_features (oracle.wl_analyze_frame's window), and its offsets"""
    arr = o.normalize(o.ground(frame.astype(np.float64)))
    win = (40 + 5.0) * dpmm
    ex, ey = frame.shape[1] / 2, frame.shape[0] / 2
    left, right = max(math.floor(ex - win / 2), 0), math.ceil(ex + win / 2)
    top, bottom = max(math.floor(ey - win / 2), 0), math.ceil(ey + win / 2)
    sample = arr[top:bottom, left:right]
    return (sample if low_density else o.invert(sample)), top, left


def main():
    frames = build()
    u16_dpmm, tol = 3.5, float(np.interp(5.0, (1.5, 30), (2, 4)))
    out = {"names": np.array(list(WINDOWS))}
    helper_in = []
    for name, (a, prm, runs) in WINDOWS.items():
        out[f"{name}.window"], out[f"{name}.params"], out[f"{name}.runs"] = a, np.array(prm), np.array(runs, dtype=float)
        helper_in.append((f"{name}.levels", a))
    for k, frame in enumerate(frames):
        out[f"u16.{k}.frame"] = frame
        for tag, low in (("inv", False), ("low", True)):
            sample, top, left = u16_sample(frame, u16_dpmm, low)
            assert sample.shape[1] <= 160 and sample.shape[0] <= 160
            if k == 2:
                assert top == 0 and sample.shape[0] == frame.shape[0]          # clipped by the frame, top and bottom
            pts, _ = points(sample, (u16_dpmm, 2.5, tol), 1, 5)
            assert len(pts) == 1, (k, tag)
            helper_in.append((f"u16.{k}.{tag}.levels", sample))
    out["u16.params"] = np.array([u16_dpmm, 5.0])                              # dpmm, bb_diameter_mm
    with tempfile.TemporaryDirectory() as td:
        inp, outp = os.path.join(td, "w.npz"), os.path.join(td, "f.npz")
        np.savez(inp, count=len(helper_in), **{f"w{i}": a for i, (_, a) in enumerate(helper_in)})
        subprocess.run([PY39, os.path.join(HERE, "skimage_bb_shapes_py39.py"), inp, outp], check=True)
        res = np.load(outp)
        for i, (key, _) in enumerate(helper_in):
            out[key] = res[f"{i}.levels"]
        out["versions"] = res["versions"]
    path = os.path.join(HERE, "bb_shapes.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(WINDOWS), "windows;",
          sum(len(out[k]) for k in out if k.endswith(".levels")), "regions")


if __name__ == "__main__":
    main()
