"""starshot.analyze_batch with per-frame analyzers (the default: profile tail and scipy's Nelder-Mead on the host, frame by frame)
against analyzers=False (profile tail and wobble fit on the device: pl_starshot_roll / pl_starshot_peaks / pl_starshot_wobble)
on the SAME resident stack, in one process.

    python scripts/time_starshot_batch.py [--frames 64 512] [--steps 5] [--warmup 1] [--device-only]

The stack is the golden frame "four" of tests/golden/starshot.npz (600 x 640 uint16) shifted by up to +-8 pixels per frame, so a
pass of the sweep holds several ring sizes.  Prints one JSON line: per stack size the median and minimum wall time of each path
(host clock around a synchronised call: both paths are host-driven), the number of sweep passes and ring-size groups of the
first pass, and whether the two results agree field for field.  --device-only runs analyzers=False alone (for a
`rocprofv3 --kernel-trace --stats` run of its kernels)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXACT = ("status", "wobble_center", "wobble_radius", "wobble_radius_mm", "wobble_diameter_mm", "passed", "n_lines", "radius",
         "min_peak_height")


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    from pylinac_amd import starshot as ss

    dev = torch.device("cuda:0")
    g = np.load(os.path.join(ROOT, "tests", "golden", "starshot.npz"), allow_pickle=False)
    frame, dpi = g["four.frame"], float(g["four.dpi"])
    rng = np.random.default_rng(0)
    out = {"what": "starshot.analyze_batch: analyzers=True vs analyzers=False", "shape": list(frame.shape), "steps": args.steps,
           "stacks": []}
    ok = True
    for n in args.frames:
        shifts = rng.integers(-8, 9, (n, 2))
        x = torch.from_numpy(np.stack([np.roll(frame, tuple(s), axis=(0, 1)) for s in shifts])).to(dev)
        row = {"frames": n}
        dev_res = ss.analyze_batch(x, dpi=dpi, sid=1000, analyzers=False)
        sizes = {ss.StarProfile._ring(frame.shape, ss.Point(x=p[0], y=p[1]), 0.85).size for p in dev_res.start_point}
        row["ring_sizes_first_pass"] = len(sizes)
        row["measured"] = int((dev_res.status == 0).sum())
        row["retried"] = int(((dev_res.radius != 0.85) | (dev_res.min_peak_height != 0.25))[dev_res.status == 0].sum())
        row["nfev_mean"] = round(float(dev_res.nfev[dev_res.status == 0].mean()), 1)
        row["analyzers_false"] = timed(lambda: ss.analyze_batch(x, dpi=dpi, sid=1000, analyzers=False), args.steps, args.warmup)
        if not args.device_only:
            ref = ss.analyze_batch(x, dpi=dpi, sid=1000)
            same = all(np.array_equal(getattr(dev_res, f), getattr(ref, f), equal_nan=True) for f in EXACT)
            row["equal_to_default"] = bool(same)
            ok = ok and same
            row["analyzers_true"] = timed(lambda: ss.analyze_batch(x, dpi=dpi, sid=1000), max(1, args.steps // 2), args.warmup)
            row["ratio"] = round(row["analyzers_true"]["ms_median"] / row["analyzers_false"]["ms_median"], 1)
        out["stacks"].append(row)
    print(json.dumps(out))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
