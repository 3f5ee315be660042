"""A session's .xim files as a stack: the per-file loop ``XIM(path).array`` (a) against ``xim.load_frames(paths)`` (b) on the
SAME files, in one process.

    python scripts/time_xim_batch.py [--files 64] [--size 1280] [--reps 3] [--only-b] [--out FILE.json]

A few distinct seeded int32 images (smooth field + noise + 2^21 outliers: 1-, 2- and 4-byte differences) are encoded once by
a vectorised form of oracle.xim_encode -- checked against it on a small image first -- and written --files times to a
temporary directory.  Each path runs --reps times, alternating a, b, a, b, ...; a repetition is the host clock from the
first file to a device synchronise.  For (b) the host part (read + parse + fill of the pinned buffer + queueing the copy) is
clocked on the host, and the copy and the decode are bracketed by device events.  Prints one JSON line (and writes it to
--out): the times, the bytes moved, whether both paths gave the same pixels, and whether (b)'s slowest repetition beats (a)'s
fastest.  --only-b runs (b) alone (for a `rocprofv3 --kernel-trace --stats` run of its kernels)."""
from __future__ import annotations

import argparse
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def encode_fast(pixels: np.ndarray):
    """oracle.xim_encode without its per-difference Python loop -> (lookup table, pixel buffer)"""
    h, w = pixels.shape
    flat = pixels.astype(np.int64).ravel()
    i = np.arange(w + 1, h * w)
    diffs = flat[i] - flat[i - 1] - flat[i - w] + flat[i - w - 1]
    codes = np.where((diffs >= -128) & (diffs <= 127), 0, np.where((diffs >= -32768) & (diffs <= 32767), 1, 2)).astype(np.uint8)
    pad = (-len(codes)) % 4
    c4 = np.concatenate([codes, np.zeros(pad, np.uint8)]).reshape(-1, 4)
    lut = (c4[:, 0] | (c4[:, 1] << 2) | (c4[:, 2] << 4) | (c4[:, 3] << 6)).astype(np.uint8)
    sizes = np.int64(1) << codes.astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    body = np.zeros(int(sizes.sum()), dtype=np.uint8)
    bits = diffs & 0xFFFFFFFF
    for k in range(4):
        use = sizes > k
        body[offs[use] + k] = (bits[use] >> (8 * k)) & 0xFF
    return lut, np.concatenate([flat[: w + 1].astype("<i4").view(np.uint8), body])


def file_bytes(pixels: np.ndarray, pixel_cm: float = 0.0336) -> bytes:
    """oracle.xim_file_bytes' layout (4 bytes per pixel, no histogram, the two pixel-size properties) around encode_fast"""
    h, w = pixels.shape
    lut, stream = encode_fast(pixels)
    out = [b"VMS.XI\x00\x00", struct.pack("<6i", 1, w, h, 32, 4, 1), struct.pack("<i", len(lut)), lut.tobytes(),
           struct.pack("<i", len(stream)), stream.tobytes(), struct.pack("<i", w * h * 4), struct.pack("<i", 0), struct.pack("<i", 2)]
    for name in ("PixelWidth", "PixelHeight"):
        out.append(struct.pack("<i", len(name)) + name.encode() + struct.pack("<id", 1, pixel_cm))
    return b"".join(out)


def image(seed: int, size: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    img = (30000 + 20000 * np.sin(yy / (90.0 + seed)) * np.cos(xx / (140.0 - seed)) + rng.normal(0, 50, (size, size))).round().astype(np.int64)
    img.ravel()[rng.integers(0, img.size, 50)] = 1 << 21
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--size", type=int, default=1280)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only-b", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from oracle import pylinac_oracle as o
    from pylinac_amd import xim as px

    small = image(1, 48)[:37, :41]
    lut, stream = encode_fast(small)
    lut0, stream0 = o.xim_encode(small)
    assert np.array_equal(lut, lut0) and np.array_equal(stream, stream0), "encode_fast differs from oracle.xim_encode"
    assert file_bytes(small) == o.xim_file_bytes(small, 4, {"PixelWidth": 0.0336, "PixelHeight": 0.0336})

    dev = torch.device("cuda:0")
    imgs = [image(100 + k, args.size) for k in range(args.distinct)]
    blobs = [file_bytes(im) for im in imgs]
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for k in range(args.files):
            paths.append(os.path.join(tmp, f"{k:03d}.xim"))
            with open(paths[-1], "wb") as f:
                f.write(blobs[k % args.distinct])

        def per_file():
            t0 = time.perf_counter()
            arrays = [px.XIM(p, device=dev).array for p in paths]
            torch.cuda.synchronize()
            return {"ms": (time.perf_counter() - t0) * 1e3}, arrays

        def stack():
            e1, e2 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            images, dbuf, spans = px._stage(paths, dev)           # the copy is queued when this returns
            t1 = time.perf_counter()
            e1.record()
            first = images[0]
            frames, status = px.decode_xim_batch(dbuf, spans[0], spans[1], spans[2], spans[3], first.img_width_px,
                                                 first.img_height_px, first.bytes_per_pixel, device=dev)
            e2.record()
            flags = status.cpu()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert not bool(flags.any())
            return {"ms": (t2 - t0) * 1e3, "host_parse_fill_queue_ms": (t1 - t0) * 1e3, "decode_device_ms": e1.elapsed_time(e2),
                    "buffer_bytes": int(dbuf.numel())}, frames

        # warm-up: code objects, the allocator's pools, the page cache of the files
        if not args.only_b:
            per_file()
        stack()
        px.load_frames(paths[:2], device=dev)
        a_runs, b_runs, same = [], [], None
        for _ in range(args.reps):
            if not args.only_b:
                ra, arrays = per_file()
                a_runs.append(ra)
            rb, frames = stack()
            b_runs.append(rb)
            if not args.only_b and same is None:
                same = all(torch.equal(frames[k], arrays[k]) for k in range(args.files))
                same = same and all(np.array_equal(frames[k].cpu().numpy(), imgs[k].astype(np.int32)) for k in range(args.distinct))
            del frames
        # the copy alone: the same pinned buffer size, bracketed by events
        nbytes = b_runs[0]["buffer_bytes"]
        host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        copies = []
        for _ in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(host, non_blocking=True)
            e1.record()
            torch.cuda.synchronize()
            copies.append(e0.elapsed_time(e1))
    out = {"what": "XIM(path).array per file (a) vs xim.load_frames (b), same files, one process, alternating",
           "files": args.files, "shape": [args.size, args.size], "bytes_per_pixel": 4, "distinct_images": args.distinct,
           "file_bytes": len(blobs[0]), "buffer_bytes": nbytes, "frames_bytes": args.files * args.size * args.size * 4,
           "a_ms": [round(r["ms"], 2) for r in a_runs], "b_ms": [round(r["ms"], 2) for r in b_runs],
           "b_host_parse_fill_queue_ms": [round(r["host_parse_fill_queue_ms"], 2) for r in b_runs],
           "b_decode_device_ms": [round(r["decode_device_ms"], 3) for r in b_runs],
           "copy_device_ms": [round(c, 3) for c in copies[1:]],
           "copy_gb_per_s": round(nbytes / (min(copies[1:]) * 1e-3) / 1e9, 1)}
    if not args.only_b:
        out["same_pixels"] = bool(same)
        out["b_slowest_beats_a_fastest"] = bool(max(out["b_ms"]) < min(out["a_ms"]))
        out["ratio_a_fastest_over_b_slowest"] = round(min(out["a_ms"]) / max(out["b_ms"]), 2)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not args.only_b and not (same and out["b_slowest_beats_a_fastest"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
