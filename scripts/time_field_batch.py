"""field_analysis.analyze_batch on 256 x 1024^2 uint16 synthetic.epid_open_field_frames (VARIAN / Beam center / Inflection
Derivative): the device pass (inversion check, centre sums, centre search, strips, profiles, field_data windows: device events
after warm-up), the whole call including the host "top" fits (host clock ending in a synchronise), and the per-image class
sequence (test_field_batch.per_image) on 16 of the same frames for the per-frame speed-up.  Prints one JSON line.

    python scripts/time_field_batch.py [--frames 256] [--reps 3] [--out PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--class-frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from pylinac_amd import field_analysis as pfa
    from pylinac_amd import ops, synthetic
    from test_field_batch import per_image

    dev = torch.device("cuda:0")
    frames = synthetic.epid_open_field_frames(a.frames, device=dev)
    pixel_mm = 0.336
    dpmm = 1 / pixel_mm
    kw = dict(protocol="VARIAN", centering="Beam center", edge_detection_method="Inflection Derivative")

    # the device pass: everything before the one device-to-host copy, timed with device events
    captured = {}
    real_copy = ops.HostCopy

    class Marked(real_copy):
        def __init__(self, t):
            captured["end"] = torch.cuda.Event(enable_timing=True)
            captured["end"].record()
            super().__init__(t)

    pfa.analyze_batch(frames, dpmm, **kw)                      # warm-up (library load, caches)
    torch.cuda.synchronize()
    device_ms, whole_ms = [], []
    ops.HostCopy = Marked
    try:
        for _ in range(a.reps):
            start = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            start.record()
            res = pfa.analyze_batch(frames, dpmm, **kw)
            torch.cuda.synchronize()
            whole_ms.append((time.perf_counter() - t0) * 1e3)
            device_ms.append(start.elapsed_time(captured["end"]))
    finally:
        ops.HostCopy = real_copy
    assert (res.status == 0).all()

    host = frames[: a.class_frames].cpu().numpy()
    dpi = dpmm * 25.4
    per_image(host[0], dpi, kw, dev)                           # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(a.class_frames):
        per_image(host[k], dpi, kw, dev)
    torch.cuda.synchronize()
    class_ms = (time.perf_counter() - t0) * 1e3 / a.class_frames

    line = {"frames": a.frames, "shape": list(frames.shape), "dtype": "uint16", "config": kw,
            "device_pass_ms": min(device_ms), "device_pass_ms_all": device_ms,
            "whole_call_ms": min(whole_ms), "whole_call_ms_all": whole_ms,
            "per_frame_batch_ms": min(whole_ms) / a.frames, "per_frame_class_ms": class_ms,
            "per_frame_speedup": class_ms / (min(whole_ms) / a.frames), "class_frames": a.class_frames,
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
