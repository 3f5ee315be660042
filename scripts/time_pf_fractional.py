"""Throughput of picketfence.analyze_batch(measure_fractional=True) on float64 frames: 512 x 768 x 1024 config #3 frames
(synthetic.pf_frames) rescaled as a DICOM series with RescaleSlope 0.0173 / RescaleIntercept -7.25 would be (3.2 GB resident).

    python scripts/time_pf_fractional.py [--frames 512] [--steps 10] [--warmup 3]

Prints one JSON line (frames/s over `steps` timed passes after `warmup`, device events around each pass) and checks frame 0
against the oracle.  Under `rocprofv3 --kernel-trace --stats` it gives the per-kernel table of the float64 path."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from oracle import pylinac_oracle as o
    from pylinac_amd import picketfence
    from pylinac_amd.synthetic import pf_frames

    dev = torch.device("cuda:0")
    dpmm = 1 / 0.390625
    raw = pf_frames(args.frames, device=dev)
    x = raw.to(torch.float64) * 0.0173
    x += -7.25
    del raw
    run = lambda: picketfence.analyze_batch(x, dpmm, num_pickets=10, measure_fractional=True)  # noqa: E731
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = run()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    ms = float(np.median(times))
    f0 = x[0].cpu().numpy()
    ref = o.pf_measure(o.normalize(o.ground(f0)), dpmm, num_pickets=10)
    P = len(ref["peak_idxs"])
    got = res.position[0, :, :P].cpu().numpy()
    ok = (int(res.picket_count[0]) == P and np.array_equal(np.isnan(got), np.isnan(ref["position"]))
          and np.array_equal(got[~np.isnan(got)], ref["position"][~np.isnan(ref["position"])]))
    print(json.dumps({"what": "picketfence.analyze_batch(measure_fractional=True)", "frames": args.frames, "shape": list(x.shape[1:]),
                      "dtype": "float64", "ms_per_pass_median": round(ms, 4), "ms_min": round(min(times), 4),
                      "frames_per_s": round(args.frames / ms * 1e3, 1), "steps": args.steps, "windows_measured":
                      int((res.status == 0).sum()), "frame0_vs_oracle": bool(ok)}))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
