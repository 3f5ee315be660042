"""RLE Lossless Part-10 files as a stack: ``dicom.load_frames`` on RLE files (a) against ``dicom.load_frames`` on the SAME
frames stored native (b) -- the floor the decoder cannot beat --, in one process.

    python scripts/time_dicom_rle.py [--files 64] [--size 1024] [--reps 3] [--only-rle] [--out FILE.json]

A few distinct seeded Winston-Lutz frames with dark-current noise (``synthetic.wl_frames``, uint16: the low-byte plane barely
compresses, the high-byte plane is almost all replicate runs) are encoded once by the test suite's PackBits encoder
(tests/dicom_rle_checks.py; the product does not write RLE) and used --files times.  Each path runs --reps times, alternating
a, b, a, b, ...; a repetition is the host clock from the first file's bytes to a device synchronise.  The device part of (a)
is split by stream events into the copy of the compressed bytes, ``pl_dicom_rle_decode`` (the three passes) and
``pl_dicom_decode`` (the conversion of the decoded buffer, here to float64).  Also: the restated pure-Python decoder of
pydicom on ONE frame on the host (what the reference's loader does per file), and a best-case stack of constant frames.
Prints one JSON line (and writes it to --out).  --only-rle runs the device part of (a) alone, five times (for a
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only-rle", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import dicom_rle_checks as enc
    from pylinac_amd import dicom
    from pylinac_amd.synthetic import wl_frames

    dev = torch.device("cuda:0")
    n, size = args.files, args.size
    frames = wl_frames(args.distinct, size, size, seed0=3300, noise_sigma=0.002)
    rle_blobs = [enc.rle_file(f[None]) for f in frames]
    native_blobs = [enc.native_file(f[None]) for f in frames]
    rle_files = [rle_blobs[k % args.distinct] for k in range(n)]
    native_files = [native_blobs[k % args.distinct] for k in range(n)]
    want = torch.from_numpy(frames[[k % args.distinct for k in range(n)]].view(np.int16)).to(dev).view(torch.uint16)

    def clocked(files):
        t0 = time.perf_counter()
        x, _ = dicom.load_frames(files, device=dev)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    # the device part of (a), staged by hand: one pinned buffer, the segment table from the 64-byte headers
    metas = [dicom.read_part10(b) for b in rle_files]
    starts, pos, table = [], 0, []
    for m, b in metas:
        starts.append(pos)
        (frag,) = m.PixelDataFragments
        table.append([(pos + o, ln) for o, ln in dicom._rle_segments(b[frag[0]:frag[0] + 64], frag, 2, "file")])
        pos += (len(b) + 3) & ~3
    host = torch.zeros(pos, dtype=torch.uint8).pin_memory()
    for st, (_, b) in zip(starts, metas):
        host.numpy()[st:st + len(b)] = b
    table = np.asarray(table, dtype=np.int64)
    seg_off, seg_len = torch.from_numpy(table[:, :, 0].copy()).to(dev), torch.from_numpy(table[:, :, 1].copy()).to(dev)
    longest = int(table[:, :, 1].max())
    dbuf = torch.empty(pos, dtype=torch.uint8, device=dev)

    def device_part():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        dbuf.copy_(host, non_blocking=True)
        ev[1].record()
        x = dicom.decode_rle_frames(dbuf, seg_off, seg_len, size, size, 16, device=dev, max_segment_bytes=longest)
        ev[2].record()
        y = dicom.decode_frames(x.view(torch.uint8).reshape(-1), torch.arange(n, dtype=torch.int64, device=dev) * (size * size * 2),
                                size, size, 16, 16, 0, out="float64", device=dev)
        ev[3].record()
        torch.cuda.synchronize()
        return [ev[k].elapsed_time(ev[k + 1]) for k in range(3)], x, y

    # warm-up: code objects and the allocator's pools
    device_part()
    clocked(rle_files[:2])
    clocked(native_files[:2])
    if args.only_rle:
        for _ in range(5):
            device_part()
        print(json.dumps({"what": "device part of load_frames on RLE files, five times", "files": n}))
        return
    a_ms, b_ms, same = [], [], True
    for _ in range(args.reps):
        t, x = clocked(rle_files)
        a_ms.append(t)
        same = same and torch.equal(x.view(torch.int16), want.view(torch.int16))
        t, x = clocked(native_files)
        b_ms.append(t)
        same = same and torch.equal(x.view(torch.int16), want.view(torch.int16))
        del x
    parts = []
    for _ in range(args.reps):
        p, x, y = device_part()
        parts.append(p)
        same = same and torch.equal(x.view(torch.int16), want.view(torch.int16)) and bool((x._pl_status == 0).all())
        same = same and torch.equal(y, want.view(torch.int16).to(torch.int32).bitwise_and(0xFFFF).to(torch.float64))
        del x, y
    # the reference's loader, per file: the restated pure-Python decoder on one frame
    (frag,) = metas[0][0].PixelDataFragments
    blob = bytes(metas[0][1][frag[0]:frag[0] + frag[1]])
    t0 = time.perf_counter()
    one = enc.rle_decode_frame(blob, size, size, 16)
    python_ms = (time.perf_counter() - t0) * 1e3
    same = same and one == frames[0].tobytes()
    # the best case: constant frames (replicate runs only: a chunk of input gives 64 chunks of output)
    flat = [enc.rle_file(np.full((1, size, size), 1000 + k, dtype=np.uint16)) for k in range(args.distinct)]
    flat = [flat[k % args.distinct] for k in range(n)]
    clocked(flat[:2])
    flat_ms = []
    for _ in range(args.reps):
        t, x = clocked(flat)
        flat_ms.append(t)
        same = same and bool((x[1].view(torch.int16) == 1001).all())
        del x
    best = min(range(args.reps), key=lambda k: sum(parts[k]))
    out = {"what": "dicom.load_frames on RLE Lossless files (a) vs on the same frames stored native (b), one process, alternating",
           "files": n, "shape": [size, size], "dtype": "uint16", "distinct_frames": args.distinct, "chunk_bytes": dicom.RLE_CHUNK,
           "rle_file_bytes": [len(b) for b in rle_blobs], "native_file_bytes": len(native_blobs[0]),
           "segment_bytes_high_low": table[:args.distinct, :, 1].tolist(), "rle_buffer_bytes": pos,
           "a_rle_ms": [round(t, 2) for t in a_ms], "b_native_ms": [round(t, 2) for t in b_ms],
           "ratio_a_fastest_over_b_fastest": round(min(a_ms) / min(b_ms), 2),
           "device_copy_ms": [round(p[0], 3) for p in parts], "device_rle_decode_ms": [round(p[1], 3) for p in parts],
           "device_dicom_decode_float64_ms": [round(p[2], 3) for p in parts],
           "rle_decode_input_gb_per_s": round(int(table[:, :, 1].sum()) / (parts[best][1] * 1e-3) / 1e9, 1),
           "rle_decode_output_gb_per_s": round(n * size * size * 2 / (parts[best][1] * 1e-3) / 1e9, 1),
           "python_decoder_one_frame_ms": round(python_ms, 1), "python_decoder_all_files_ms_extrapolated": round(python_ms * n, 0),
           "constant_frames_load_ms": [round(t, 2) for t in flat_ms], "constant_file_bytes": len(flat[0]),
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
