"""PNG files as a stack: ``png.load_frames`` on PIL's PNG files (a), the SAME frames through ``tiff.load_frames`` uncompressed
(b) -- the copy's floor --, the reference path (c): ``np.asarray(PIL.Image.open(f))`` per file on one host thread plus one
upload of the stack, and the device part of (a) between stream events (d): the copy of the compressed bytes and
``pl_png_decode`` (all its launches).  One process.

    python scripts/time_png_batch.py [--files 64] [--size 1024] [--reps 3] [--only-device] [--out FILE.json]

A few distinct seeded picket-fence frames with noise (``synthetic.pf_frames``, uint16) are written once by PIL (the product
does not write PNG) and used --files times.  Each path runs --reps times, alternating a, b, c, a, ...; a repetition is the host
clock from the files' bytes to a device synchronise.  Prints one JSON line (and writes it to --out).  --only-device runs the
device part of (a) alone, five times (for a `rocprofv3 --kernel-trace --stats` run of its kernels)."""
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

    from pylinac_amd import dicom, png, tiff
    from pylinac_amd.synthetic import pf_frames

    dev = torch.device("cuda:0")
    n, size = args.files, args.size
    frames = dicom._to_numpy(pf_frames(args.distinct, size, size, seed0=2900))

    def written(a, fmt):
        out = io.BytesIO()
        Image.fromarray(a).save(out, format=fmt)
        return out.getvalue()

    pick = [k % args.distinct for k in range(n)]
    pngs = [written(f, "PNG") for f in frames]
    raw = [written(f, "TIFF") for f in frames]
    sets = {"a_png_load_frames": (png, [pngs[k] for k in pick]), "b_tiff_uncompressed": (tiff, [raw[k] for k in pick])}
    want = torch.from_numpy(frames[pick].view(np.int16)).to(dev)

    def clocked(module, files):
        t0 = time.perf_counter()
        x = module.load_frames(files, device=dev).frames
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    def reference(files):
        t0 = time.perf_counter()
        stack = np.stack([np.asarray(Image.open(io.BytesIO(f))) for f in files])
        x = torch.from_numpy(stack.view(np.int16)).to(dev)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x.view(torch.uint16)

    # the device part of (a), staged by hand
    images, dbuf, off, ln, frame, idat_bytes = png._stage(sets["a_png_load_frames"][1], dev)
    host = dbuf.cpu().pin_memory()

    def device_part():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        dbuf.copy_(host, non_blocking=True)
        ev[1].record()
        x, status = png.decode_png_streams(dbuf, off, ln, frame, n, size, size, 16, device=dev, idat_bytes=idat_bytes)
        ev[2].record()
        torch.cuda.synchronize()
        return [ev[k].elapsed_time(ev[k + 1]) for k in range(2)], x, status

    # warm-up: code objects and the allocator's pools
    device_part()
    for module, files in sets.values():
        clocked(module, files[:2])
    reference(sets["a_png_load_frames"][1][:2])
    if args.only_device:
        for _ in range(5):
            device_part()
        print(json.dumps({"what": "device part of png.load_frames, five times", "files": n}))
        return
    ms = {k: [] for k in list(sets) + ["c_pil_one_thread_plus_upload"]}
    same = True
    for _ in range(args.reps):
        for name, (module, files) in sets.items():
            t, x = clocked(module, files)
            ms[name].append(t)
            same = same and torch.equal(x.view(torch.int16), want)
            del x
        t, x = reference(sets["a_png_load_frames"][1])
        ms["c_pil_one_thread_plus_upload"].append(t)
        same = same and torch.equal(x.view(torch.int16), want)
        del x
    parts = []
    for _ in range(args.reps):
        p, x, status = device_part()
        parts.append(p)
        same = same and torch.equal(x.view(torch.int16), want) and bool((status == 0).all())
        del x
    best = min(range(args.reps), key=lambda k: parts[k][1])
    a, b, c = (min(ms[k]) for k in ms)
    out = {"what": "png.load_frames on PIL's PNG files (a), the same frames through tiff.load_frames uncompressed (b), PIL per "
                   "file on one host thread + one upload (c), the copy and pl_png_decode of (a) between stream events (d); one "
                   "process, alternating",
           "files": n, "shape": [size, size], "dtype": "uint16", "distinct_frames": args.distinct,
           "png_file_bytes": [len(f) for f in pngs], "uncompressed_file_bytes": len(raw[0]),
           "compression_ratio": round(sum(len(f) for f in raw) / sum(len(f) for f in pngs), 3),
           "idat_chunks_per_file": len(images[0].idat),
           **{k + "_ms": [round(t, 2) for t in v] for k, v in ms.items()},
           "a_below_c_after_the_first": all(x < y for x, y in zip(ms["a_png_load_frames"][1:], ms["c_pil_one_thread_plus_upload"][1:])),
           "a_over_c_fastest": round(a / c, 4), "a_over_b_fastest": round(a / b, 3),
           "d_device_copy_ms": [round(p[0], 3) for p in parts], "d_device_png_decode_ms": [round(p[1], 3) for p in parts],
           "png_decode_output_gb_per_s": round(n * size * size * 2 / (parts[best][1] * 1e-3) / 1e9, 2),
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
