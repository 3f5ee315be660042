"""JPEG 2000 lossless Part-10 files as a stack: ``dicom.load_frames(jpeg2000=True)`` (a) against ``dicom.load_frames`` on the
SAME frames stored native (b), RLE Lossless (c) and JPEG Lossless (d), in one process, and against Pillow (OpenJPEG) decoding
the same streams one by one on one host thread plus one upload (e).

    python scripts/time_dicom_j2k.py [--reps 3] [--quick] [--out FILE.json]

The two workloads of scripts/time_dicom_jpeg_lossless.py: 128 slices of 512 x 512 int16 (a CT-like phantom plus noise) and 64
frames of 1024 x 1024 uint16 (seeded Winston-Lutz frames with dark-current noise).  A few distinct frames are encoded once
(JPEG 2000 by Pillow with its defaults, 64 x 64 code blocks and 6 resolutions: tests/dicom_j2k_checks.py; the others by the
test suite's encoders -- the product writes none of them) and used as many times as the stack is long.  Each path runs --reps
times, alternating a, b, c, d, a, ...; a repetition is the host clock from the first file's bytes to a device synchronise.
(a) is split: the host's item walk, header and packet-header parse and staging (``_j2k_stage``) on the host clock; on the
device, by stream events, the copy of the compressed bytes, ``pl_dicom_j2k_decode`` whole, the same call WITHOUT code blocks
(the clearing of the planes, the inverse transform and the store: tier 1 is the difference) and ``pl_dicom_decode`` (the
conversion of the decoded buffer, here to float64).  Prints one JSON line (and writes it to --out).  --quick: 8 slices and 4
frames."""
from __future__ import annotations

import argparse
import io
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
    import dicom_j2k_checks as jk
    import dicom_jpegll_checks as jl
    import dicom_rle_checks as rl
    from PIL import Image
    from pylinac_amd import dicom

    distinct, size = frames.shape[0], frames.shape[1]
    pick = [k % distinct for k in range(n)]
    blobs = {"j2k": [jk.j2k_file(f[None]) for f in frames], "native": [rl.native_file(f[None]) for f in frames],
             "rle": [rl.rle_file(f[None]) for f in frames], "jpegll": [jl.jpegll_file(f[None]) for f in frames]}
    files = {kind: [b[k] for k in pick] for kind, b in blobs.items()}
    want = torch.from_numpy(np.ascontiguousarray(frames[pick]).view(np.int16)).to(dev)

    def clocked(kind, count=None):
        t0 = time.perf_counter()
        x, _ = dicom.load_frames(files[kind][:count], device=dev, raw_pixels=True, jpeg_lossless=kind == "jpegll", jpeg2000=kind == "j2k")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    # (a) by hand: the host part on the host clock, the device part between stream events
    names = [f"file {k}" for k in range(n)]
    host_ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        read = [dicom.read_part10(b, jpeg2000=True) for b in files["j2k"]]
        metas, raw = [m for m, _ in read], [b for _, b in read]
        t1 = time.perf_counter()
        staged, (blocks, params), _ = dicom._j2k_stage(metas, raw, [dicom._layout(m) for m in metas], names)
        host_ms.append([(t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3])
    host = torch.from_numpy(staged).pin_memory()
    dbuf = torch.empty(host.numel(), dtype=torch.uint8, device=dev)
    dblocks, dparams = torch.from_numpy(blocks).to(dev), torch.from_numpy(params).to(dev)
    levels, rep = int(params[:, 0].max()), int(frames.dtype.kind == "i")

    def device_part():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        dbuf.copy_(host, non_blocking=True)
        ev[1].record()
        x = dicom.decode_jpeg2000_frames(dbuf, dblocks, dparams, size, size, 16, pixel_representation=rep, device=dev, max_levels=levels)
        ev[2].record()
        z = dicom.decode_jpeg2000_frames(dbuf, dblocks[:0], dparams, size, size, 16, pixel_representation=rep, device=dev, max_levels=levels)
        ev[3].record()
        y = dicom.decode_frames(x.view(torch.uint8).reshape(-1), torch.arange(n, dtype=torch.int64, device=dev) * (size * size * 2),
                                size, size, 16, 16, rep, out="float64", device=dev)
        ev[4].record()
        torch.cuda.synchronize()
        del z
        return [ev[k].elapsed_time(ev[k + 1]) for k in range(4)], x, y

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
    # (e) Pillow on one host thread, stream by stream, then one upload (a signed stream comes back shifted up by half the range)
    streams = [bytes(raw[k][o:o + ln]) for k in range(n) for o, ln in metas[k].PixelDataFragments]
    pil_ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        stack = np.stack([np.asarray(Image.open(io.BytesIO(s))) for s in streams])
        x = torch.from_numpy(stack.view(np.int16)).to(dev)
        if rep:
            x = torch.bitwise_xor(x, -32768)
        torch.cuda.synchronize()
        pil_ms.append((time.perf_counter() - t0) * 1e3)
        same = same and torch.equal(x, want)
    best = min(range(reps), key=lambda k: parts[k][1])
    tier1 = max(parts[best][1] - parts[best][2], 1e-6)
    seg_bytes, passes = int(blocks[:, 2].sum()), int(blocks[:, 3].sum())
    fastest = {k: min(v) for k, v in ms.items()}
    return {"workload": name, "files": n, "shape": [size, size], "dtype": str(frames.dtype), "distinct_frames": distinct,
            "levels": levels, "code_blocks": int(blocks.shape[0]), "coding_passes": passes, "segment_bytes": seg_bytes,
            "j2k_file_bytes": [len(b) for b in blobs["j2k"]], "native_file_bytes": len(blobs["native"][0]),
            "compression_ratio_native_over_j2k": round(sum(len(b) for b in blobs["native"]) / sum(len(b) for b in blobs["j2k"]), 2),
            "compression_ratio_native_over_jpegll": round(sum(len(b) for b in blobs["native"]) / sum(len(b) for b in blobs["jpegll"]), 2),
            "a_j2k_ms": [round(t, 2) for t in ms["j2k"]], "b_native_ms": [round(t, 2) for t in ms["native"]],
            "c_rle_ms": [round(t, 2) for t in ms["rle"]], "d_jpegll_ms": [round(t, 2) for t in ms["jpegll"]],
            "e_pillow_one_thread_plus_upload_ms": [round(t, 2) for t in pil_ms],
            "ratio_a_fastest_over_b_fastest": round(fastest["j2k"] / fastest["native"], 2),
            "ratio_a_fastest_over_c_fastest": round(fastest["j2k"] / fastest["rle"], 2),
            "ratio_a_fastest_over_d_fastest": round(fastest["j2k"] / fastest["jpegll"], 2),
            "ratio_a_fastest_over_e_fastest": round(fastest["j2k"] / min(pil_ms), 2),
            "host_read_part10_ms": [round(h[0], 2) for h in host_ms], "host_headers_tier2_staging_ms": [round(h[1], 2) for h in host_ms],
            "device_copy_ms": [round(p[0], 3) for p in parts], "device_j2k_decode_ms": [round(p[1], 3) for p in parts],
            "device_j2k_decode_without_blocks_ms": [round(p[2], 3) for p in parts],
            "device_dicom_decode_float64_ms": [round(p[3], 3) for p in parts],
            "tier1_ms_by_difference": round(tier1, 3),
            "tier1_output_mb_per_s": round(n * size * size * 2 / (tier1 * 1e-3) / 1e6, 1),
            "tier1_input_mb_per_s": round(seg_bytes / (tier1 * 1e-3) / 1e6, 1),
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
    out = {"what": "dicom.load_frames on JPEG 2000 lossless files (a) vs on the same frames stored native (b), RLE Lossless (c) and "
                   "JPEG Lossless (d), one process, alternating, and vs Pillow on one host thread plus one upload (e); one wave per "
                   "code block, the packet headers parsed on the host", "workloads": [ct, wl],
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
