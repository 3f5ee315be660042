"""JPEG Lossless Part-10 files as a stack: ``dicom.load_frames(jpeg_lossless=True)`` (a) against ``dicom.load_frames`` on the
SAME frames stored native (b) and RLE Lossless (c), in one process.

    python scripts/time_dicom_jpeg_lossless.py [--reps 3] [--quick] [--out FILE.json]

Two workloads: 128 slices of 512 x 512 int16 (a CT-like phantom plus noise) and 64 frames of 1024 x 1024 uint16 (seeded
Winston-Lutz frames with dark-current noise, ``synthetic.wl_frames``).  A few distinct frames are encoded once by the test
suite's encoders (tests/dicom_jpegll_checks.py, selection value 1; tests/dicom_rle_checks.py -- the product writes neither) and
used as many times as the stack is long.  Each path runs --reps times, alternating a, b, c, a, ...; a repetition is the host
clock from the first file's bytes to a device synchronise.  The device part of (a) is split by stream events into the copy of
the compressed bytes, ``pl_dicom_jpegll_decode`` (one wave per frame: one serial chain each) and ``pl_dicom_decode`` (the
conversion of the decoded buffer, here to float64).  Also: the restated pure-Python decoder of the tests on ONE frame on the
host, and the compression ratio.  Prints one JSON line (and writes it to --out).  --quick: 8 slices and 4 frames."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def workload(name, frames, n, reps, dev):
    import dicom_jpegll_checks as jl
    import dicom_rle_checks as rl
    from pylinac_amd import dicom

    distinct, size = frames.shape[0], frames.shape[1]
    pick = [k % distinct for k in range(n)]
    blobs = {"jpegll": [jl.jpegll_file(f[None]) for f in frames], "native": [rl.native_file(f[None]) for f in frames],
             "rle": [rl.rle_file(f[None]) for f in frames]}
    files = {kind: [b[k] for k in pick] for kind, b in blobs.items()}
    want = torch.from_numpy(np.ascontiguousarray(frames[pick]).view(np.int16)).to(dev)

    def clocked(kind, count=None):
        t0 = time.perf_counter()
        x, _ = dicom.load_frames(files[kind][:count], device=dev, raw_pixels=True, jpeg_lossless=kind == "jpegll")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    # the device part of (a), staged by hand: one pinned buffer, the scan windows and tables from the JPEG headers
    read = [dicom.read_part10(b, jpeg_lossless=True) for b in files["jpegll"]]
    metas, raw = [m for m, _ in read], [b for _, b in read]
    staged, tables, _ = dicom._jpegll_stage(metas, raw, [dicom._layout(m) for m in metas], [f"file {k}" for k in range(n)])
    host = torch.from_numpy(staged).pin_memory()
    dbuf = torch.empty(host.numel(), dtype=torch.uint8, device=dev)
    on = [torch.from_numpy(t).to(dev) for t in tables]
    rep = int(frames.dtype.kind == "i")

    def device_part():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        dbuf.copy_(host, non_blocking=True)
        ev[1].record()
        x = dicom.decode_jpeg_lossless_frames(dbuf, *on, size, size, 16, pixel_representation=rep, device=dev)
        ev[2].record()
        y = dicom.decode_frames(x.view(torch.uint8).reshape(-1), torch.arange(n, dtype=torch.int64, device=dev) * (size * size * 2),
                                size, size, 16, 16, rep, out="float64", device=dev)
        ev[3].record()
        torch.cuda.synchronize()
        return [ev[k].elapsed_time(ev[k + 1]) for k in range(3)], x, y

    device_part()                                            # warm-up: code objects and the allocator's pools
    for kind in files:
        clocked(kind, 2)
    ms, same = {kind: [] for kind in files}, True
    for _ in range(reps):
        for kind in files:
            t, x = clocked(kind)
            ms[kind].append(t)
            same = same and torch.equal(x.view(torch.int16), want)
            del x
    parts = []
    for _ in range(reps):
        p, x, y = device_part()
        parts.append(p)
        same = same and torch.equal(x.view(torch.int16), want) and bool((x._pl_status == 0).all())
        same = same and torch.equal(y, (want.to(torch.float64) if rep else want.to(torch.int32).bitwise_and(0xFFFF).to(torch.float64)))
        del x, y
    # the restated pure-Python decoder on one frame (a host-only reader decodes file by file)
    (frag,) = metas[0].PixelDataFragments
    stream = bytes(raw[0][frag[0]:frag[0] + frag[1]])
    t0 = time.perf_counter()
    one, status = jl.ref_decode(stream, size, size)
    python_ms = (time.perf_counter() - t0) * 1e3
    same = same and status == 0 and np.array_equal(one, jl.unsigned(frames[0]))
    best = min(range(reps), key=lambda k: sum(parts[k]))
    scan_bytes = int(tables[1].sum())
    return {"workload": name, "files": n, "shape": [size, size], "dtype": str(frames.dtype), "distinct_frames": distinct,
            "selection_value": 1, "jpegll_file_bytes": [len(b) for b in blobs["jpegll"]], "rle_file_bytes": [len(b) for b in blobs["rle"]],
            "native_file_bytes": len(blobs["native"][0]),
            "compression_ratio_native_over_jpegll": round(sum(len(b) for b in blobs["native"]) / sum(len(b) for b in blobs["jpegll"]), 2),
            "compression_ratio_native_over_rle": round(sum(len(b) for b in blobs["native"]) / sum(len(b) for b in blobs["rle"]), 2),
            "a_jpegll_ms": [round(t, 2) for t in ms["jpegll"]], "b_native_ms": [round(t, 2) for t in ms["native"]],
            "c_rle_ms": [round(t, 2) for t in ms["rle"]],
            "ratio_a_fastest_over_b_fastest": round(min(ms["jpegll"]) / min(ms["native"]), 2),
            "ratio_a_fastest_over_c_fastest": round(min(ms["jpegll"]) / min(ms["rle"]), 2),
            "device_copy_ms": [round(p[0], 3) for p in parts], "device_jpegll_decode_ms": [round(p[1], 3) for p in parts],
            "device_dicom_decode_float64_ms": [round(p[2], 3) for p in parts],
            "jpegll_decode_ns_per_sample_of_a_chain": round(parts[best][1] * 1e6 / (size * size), 1),   # (the chains run side by side)
            "jpegll_decode_input_mb_per_s": round(scan_bytes / (parts[best][1] * 1e-3) / 1e6, 1),
            "jpegll_decode_output_mb_per_s": round(n * size * size * 2 / (parts[best][1] * 1e-3) / 1e6, 1),
            "python_decoder_one_frame_ms": round(python_ms, 1), "python_decoder_all_files_ms_extrapolated": round(python_ms * n, 0),
            "same_pixels": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import dicom_jpegll_checks as jl
    from pylinac_amd.synthetic import wl_frames

    dev = torch.device("cuda:0")
    ct = workload("CT slices", jl.ct_slices(4, 512), 8 if args.quick else 128, args.reps, dev)
    wl = workload("Winston-Lutz frames", wl_frames(4, 1024, 1024, seed0=3300, noise_sigma=0.002), 4 if args.quick else 64, args.reps, dev)
    out = {"what": "dicom.load_frames on JPEG Lossless files (a) vs on the same frames stored native (b) and RLE Lossless (c), one "
                   "process, alternating; one wave and one serial chain per frame", "workloads": [ct, wl],
           "same_pixels": ct["same_pixels"] and wl["same_pixels"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not out["same_pixels"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
