"""Deflate TIFFs as a stack: ``tiff.load_frames(deflate=True)`` on Deflate + predictor-2 files in 64 KiB strips (a), on the
SAME frames as LZW + predictor 2 (b) and uncompressed (c) -- the copy's floor --, on the same Deflate data as ONE strip per
file (d: the latency chain of one stream a file), and the reference path (e): ``np.asarray(PIL.Image.open(f))`` per file on one
host thread plus one upload of the stack.  One process.

    python scripts/time_tiff_deflate.py [--files 64] [--size 1024] [--reps 3] [--only-device] [--out FILE.json]

A few distinct seeded picket-fence frames with noise (``synthetic.pf_frames``, uint16: film-like ridges) are written once by
PIL (the product does not write TIFF) and used --files times.  Each path runs --reps times, alternating a, b, c, d, e, a, ...;
a repetition is the host clock from the files' bytes to a device synchronise.  The device part of (a) is split by stream
events into the copy of the compressed bytes and ``pl_tiff_decode_ex`` (all its launches).  Prints one JSON line (and writes
it to --out).  --only-device runs the device part of (a) alone, five times (for a `rocprofv3 --kernel-trace --stats` run of
its kernels)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only-device", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from PIL import Image

    from pylinac_amd import dicom, tiff
    from pylinac_amd.synthetic import pf_frames

    dev = torch.device("cuda:0")
    n, size = args.files, args.size
    frames = dicom._to_numpy(pf_frames(args.distinct, size, size, seed0=2800))

    def written(a, **kw):
        out = io.BytesIO()
        Image.fromarray(a).save(out, format="TIFF", **kw)
        return out.getvalue()

    pick = [k % args.distinct for k in range(n)]
    deflate = [written(f, compression="tiff_adobe_deflate", tiffinfo={317: 2}) for f in frames]
    lzw = [written(f, compression="tiff_lzw", tiffinfo={317: 2}) for f in frames]
    raw = [written(f) for f in frames]
    one = [written(f, compression="tiff_adobe_deflate", tiffinfo={317: 2, 278: size}) for f in frames]
    sets = {"a_deflate_64k_strips": [deflate[k] for k in pick], "b_lzw_64k_strips": [lzw[k] for k in pick],
            "c_uncompressed": [raw[k] for k in pick], "d_deflate_one_strip": [one[k] for k in pick]}
    want = torch.from_numpy(frames[pick].view(np.int16)).to(dev)

    def clocked(files):
        t0 = time.perf_counter()
        x = tiff.load_frames(files, device=dev, deflate=True).frames
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    def reference(files):
        t0 = time.perf_counter()
        stack = np.stack([np.asarray(Image.open(io.BytesIO(f))) for f in files])
        x = torch.from_numpy(stack.view(np.int16)).to(dev)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x.view(torch.uint16)

    # the device part of (a), staged by hand
    images, dbuf, off, ln, desc, flags, mask, longest = tiff._stage(sets["a_deflate_64k_strips"], dev, deflate=True)
    host = dbuf.cpu().pin_memory()

    def device_part():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        dbuf.copy_(host, non_blocking=True)
        ev[1].record()
        x, status = tiff.decode_tiff_strips(dbuf, off, ln, desc, flags, size, size, 16, device=dev, compressions=mask,
                                            max_strip_bytes=longest)
        ev[2].record()
        torch.cuda.synchronize()
        return [ev[k].elapsed_time(ev[k + 1]) for k in range(2)], x, status

    # warm-up: code objects and the allocator's pools
    device_part()
    for files in sets.values():
        clocked(files[:2])
    reference(sets["a_deflate_64k_strips"][:2])
    if args.only_device:
        for _ in range(5):
            device_part()
        print(json.dumps({"what": "device part of load_frames(deflate=True) on Deflate + predictor-2 files, five times", "files": n}))
        return
    ms = {k: [] for k in list(sets) + ["e_pil_one_thread_plus_upload"]}
    same = True
    for _ in range(args.reps):
        for name, files in sets.items():
            t, x = clocked(files)
            ms[name].append(t)
            same = same and torch.equal(x.view(torch.int16), want)
            del x
        t, x = reference(sets["a_deflate_64k_strips"])
        ms["e_pil_one_thread_plus_upload"].append(t)
        same = same and torch.equal(x.view(torch.int16), want)
        del x
    parts = []
    for _ in range(args.reps):
        p, x, status = device_part()
        parts.append(p)
        same = same and torch.equal(x.view(torch.int16), want) and bool((status == 0).all())
        del x
    best = min(range(args.reps), key=lambda k: parts[k][1])
    a, b, e = ms["a_deflate_64k_strips"], ms["b_lzw_64k_strips"], ms["e_pil_one_thread_plus_upload"]
    out = {"what": "tiff.load_frames(deflate=True) on Deflate + predictor-2 files in 64 KiB strips (a), the same frames as LZW + "
                   "predictor 2 (b) and uncompressed (c), the same Deflate data as one strip per file (d), PIL per file on one host "
                   "thread + one upload (e); one process, alternating",
           "files": n, "shape": [size, size], "dtype": "uint16", "distinct_frames": args.distinct,
           "deflate_file_bytes": [len(f) for f in deflate], "lzw_file_bytes": [len(f) for f in lzw],
           "uncompressed_file_bytes": len(raw[0]), "one_strip_file_bytes": [len(f) for f in one],
           "compression_ratio": round(sum(len(f) for f in raw) / sum(len(f) for f in deflate), 3),
           "strips_per_file": len(images[0].strips), "strips": int(off.numel()), "longest_strip_bytes": int(longest),
           **{k + "_ms": [round(t, 2) for t in v] for k, v in ms.items()},
           "a_over_e_by_repetition": [round(x / y, 4) for x, y in zip(a, e)],
           "a_over_b_by_repetition": [round(x / y, 3) for x, y in zip(a, b)],
           "a_below_e_in_every_repetition": bool(all(x < y for x, y in zip(a, e))),
           "d_over_a_fastest": round(min(ms["d_deflate_one_strip"]) / min(a), 2),
           "device_copy_ms": [round(p[0], 3) for p in parts], "device_tiff_decode_ms": [round(p[1], 3) for p in parts],
           "tiff_decode_output_gb_per_s": round(n * size * size * 2 / (parts[best][1] * 1e-3) / 1e9, 2),
           "same_pixels": bool(same)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
