"""Helper run under /opt/conda/bin/python3.9 (scikit-image 0.18.3) by make_bb_shapes_golden.py: scikit-image's OWN
region properties of every region the BB finder's threshold sweep sees on the shape-zoo windows.  The reference tree is
not needed (and not imported): the sweep's masks are ``stretch(window, 0, 1) > cutoff`` with the cutoffs accumulated as
pylinac/metrics/utils.py:121-128, 180 does, labelled and cleared as utils.py:130-134 does.  Build container only.

    python3.9 skimage_bb_shapes_py39.py IN.npz OUT.npz

IN holds ``count`` and the float64 windows ``w0 .. w{count-1}``.  OUT holds, per window k, ``k.levels``: one row per
region of at least four pixels (smaller ones are speckle no predicate can accept: max(pi (r - t)^2, 2) mm^2 is 18 px at
3 px/mm) at every level whose mask differs from the level before,
    level, label, area, filled_area, bbox (4), perimeter, convex_area, solidity, weighted_centroid (2)
and ``versions``."""
import sys
import warnings

warnings.filterwarnings("ignore")
import numpy as np
import scipy
import skimage
from skimage import measure, segmentation

d = np.load(sys.argv[1])
out = {"versions": np.array([f"numpy {np.__version__}", f"scipy {scipy.__version__}", f"scikit-image {skimage.__version__}"])}
for k in range(int(d["count"])):
    a = d[f"w{k}"].astype(float)
    g = a - a.min() + 0                               # stretch(a, 0, 1) = ground(normalize(ground(a)) * 1, value=0)
    n = (g / g.max()) * 1.0
    s = n - n.min() + 0
    rows, prev = [], None
    cutoff = 0.0 + 1.0 / 50
    for lvl in range(50):
        if cutoff > 1.0:
            break
        bw = s > cutoff
        if prev is None or not np.array_equal(bw, prev):
            lab = segmentation.clear_border(measure.label(bw, connectivity=1))
            for r in measure.regionprops(lab, intensity_image=s):
                if r.area < 4:
                    continue
                rows.append([lvl, r.label, r.area, r.filled_area, *r.bbox, r.perimeter, r.convex_area, r.solidity,
                             *r.weighted_centroid])
        prev = bw
        cutoff += 1.0 / 50
    out[f"{k}.levels"] = np.array(rows, dtype=float).reshape(-1, 13)
np.savez_compressed(sys.argv[2], **out)
