"""ZIP archives of native DICOM files: ``dicom.load_zip`` against the path without it -- ``zipfile`` reading every member on one
host thread, then ``dicom.load_frames`` -- in one process.

    python scripts/time_zip_batch.py [--slices 128] [--wl-frames 16] [--reps 3] [--loop 20] [--only-device] [--out FILE.json]

  a   ``dicom.load_zip`` of --slices members of 512 x 512 int16 (``synthetic.catphan_volume``, noise included), Deflate level 6
  b   the same archive through ``zipfile`` + ``dicom.load_frames``
  c   a and b for the same files stored
  d   a and b for --wl-frames members of 1280 x 1280 uint16 (``synthetic.wl_frames`` with its noise layer), Deflate level 6
  e   ``pl_crc32`` over the volume's extracted members and the inflate launch (``pl_inflate``, raw streams) over its
      compressed ones, each alone between stream events around a sustained loop of --loop calls
  f   ``zlib.crc32`` over the same bytes on one host thread

The variants alternate over --reps repetitions after a warm-up call of each; a repetition is the host clock from the archive's
bytes to a device synchronise.  Prints one JSON line (and writes it to --out).  --only-device runs one ``load_zip`` of (a) five
times (for a `rocprofv3 --kernel-trace --stats` run of its kernels)."""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time
import zipfile
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=128)
    ap.add_argument("--wl-frames", type=int, default=16)
    ap.add_argument("--wl-size", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop", type=int, default=20)
    ap.add_argument("--only-device", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import dicom_rle_checks as enc                          # the Part-10 writer of the tests (the product writes no DICOM)
    from pylinac_amd import _lib, dicom, zipstack
    from pylinac_amd.synthetic import catphan_volume, wl_frames

    dev = torch.device("cuda:0")

    def archive(frames, kind):
        out = io.BytesIO()
        with zipfile.ZipFile(out, "w") as zf:
            for k, f in enumerate(frames):
                zf.writestr(zipfile.ZipInfo(f"series/IM{k:04d}.dcm"), enc.native_file(f[None]), compress_type=kind, compresslevel=6)
        return out.getvalue()

    volume = catphan_volume(seed=4100, n_slices=args.slices, size=512)
    wl = wl_frames(args.wl_frames, args.wl_size, args.wl_size, seed0=3100, noise_sigma=0.002)
    wl = dicom._to_numpy(wl) if isinstance(wl, torch.Tensor) else np.asarray(wl)
    sets = {"ct_deflated": (archive(volume, zipfile.ZIP_DEFLATED), volume), "ct_stored": (archive(volume, zipfile.ZIP_STORED), volume),
            "wl_deflated": (archive(wl, zipfile.ZIP_DEFLATED), wl)}

    def on_device(data):
        t0 = time.perf_counter()
        x, _, _ = dicom.load_zip(data, device=dev)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    def on_host(data):
        t0 = time.perf_counter()
        with zipfile.ZipFile(io.BytesIO(data)) as zf:
            blobs = [zf.read(i) for i in zf.infolist()]
        t1 = time.perf_counter()
        x, _ = dicom.load_frames(blobs, device=dev)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x, (t1 - t0) * 1e3

    def same(x, frames):
        return bool(np.array_equal(dicom._to_numpy(x), frames))

    for data, _ in sets.values():                           # warm-up: code objects and the allocator's pools
        on_device(data)
        on_host(data)
    if args.only_device:
        for _ in range(5):
            on_device(sets["ct_deflated"][0])
        print(json.dumps({"what": "dicom.load_zip of the deflated volume, five times", "members": args.slices}))
        return
    ms = {f"{name}_{path}": [] for name in sets for path in ("load_zip", "zipfile_load_frames")}
    read_ms = {name: [] for name in sets}
    equal = True
    for _ in range(args.reps):
        for name, (data, frames) in sets.items():
            t, x = on_device(data)
            ms[f"{name}_load_zip"].append(t)
            equal = equal and same(x, frames)
            del x
            t, x, t_read = on_host(data)
            ms[f"{name}_zipfile_load_frames"].append(t)
            read_ms[name].append(t_read)
            equal = equal and same(x, frames)
            del x

    # e: the CRC pair and the inflate launch alone, over the volume's members
    data = sets["ct_deflated"][0]
    stack = zipstack.extract(data, device=dev)
    members = stack.members
    lib = _lib.load()
    n = len(members)
    total = int(stack.sizes.sum())
    max_len = int(stack.sizes.max())
    table = torch.from_numpy(np.concatenate([stack.offsets, stack.sizes])).to(dev)
    crc = torch.zeros(n, dtype=torch.uint32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    work = torch.empty(int(lib.pl_crc32_work_bytes(n, max_len)), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def crc_call():
        _lib.check(lib.pl_crc32(stack.buffer.data_ptr(), stack.buffer.numel(), table[:n].data_ptr(), table[n:].data_ptr(), n, max_len,
                                crc.data_ptr(), status.data_ptr(), work.data_ptr(), stream), "pl_crc32")

    dbuf = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    in_off = torch.tensor([m.data_offset for m in members], dtype=torch.int64, device=dev)
    in_len = torch.tensor([m.compressed_size for m in members], dtype=torch.int64, device=dev)
    out = torch.empty_like(stack.buffer)
    out_len = torch.empty(n, dtype=torch.int64, device=dev)
    st2 = torch.empty(n, dtype=torch.int32, device=dev)

    def inflate_call():
        _lib.check(lib.pl_inflate(dbuf.data_ptr(), dbuf.numel(), in_off.data_ptr(), in_len.data_ptr(), n, 0, out.data_ptr(),
                                  table[:n].data_ptr(), table[n:].data_ptr(), out_len.data_ptr(), st2.data_ptr(), stream), "pl_inflate")

    def looped(call, loops):
        call()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(loops):
            call()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / loops

    crc_ms = [looped(crc_call, args.loop) for _ in range(args.reps)]
    inflate_ms = [looped(inflate_call, max(args.loop // 5, 2)) for _ in range(args.reps)]
    blobs = [dicom._to_numpy(stack.member(k)).tobytes() for k in range(n)]
    want = [zlib.crc32(b) for b in blobs]
    equal = equal and [int(v) & 0xFFFFFFFF for v in crc.cpu().view(torch.int32).tolist()] == want and want == [m.crc32 for m in members]
    equal = equal and bool((status == 0).all()) and bool((st2 == 0).all())
    equal = equal and all(torch.equal(out[o:o + s], stack.buffer[o:o + s]) for o, s in zip(stack.offsets.tolist(), stack.sizes.tolist()))
    host_crc_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for b in blobs:
            zlib.crc32(b)
        host_crc_ms.append((time.perf_counter() - t0) * 1e3)

    def after_first(a, b):
        return all(x < y for x, y in zip(ms[a][1:], ms[b][1:]))

    res = {"what": "dicom.load_zip (a) against zipfile on one host thread + dicom.load_frames (b) for a CT volume deflated at level 6, "
                   "the same stored (c) and a Winston-Lutz session deflated (d); pl_crc32 and the inflate launch alone between "
                   "stream events around a sustained loop (e); zlib.crc32 on one host thread (f); one process, alternating",
           "ct_members": args.slices, "ct_shape": [512, 512], "ct_dtype": "int16", "wl_members": args.wl_frames,
           "wl_shape": [args.wl_size, args.wl_size], "wl_dtype": "uint16",
           "archive_bytes": {k: len(v[0]) for k, v in sets.items()}, "ct_extracted_bytes": total,
           **{k + "_ms": [round(t, 2) for t in v] for k, v in ms.items()},
           "zipfile_read_ms": {k: [round(t, 2) for t in v] for k, v in read_ms.items()},
           "a_below_b_after_the_first": after_first("ct_deflated_load_zip", "ct_deflated_zipfile_load_frames"),
           "c_device_below_host_after_the_first": after_first("ct_stored_load_zip", "ct_stored_zipfile_load_frames"),
           "d_device_below_host_after_the_first": after_first("wl_deflated_load_zip", "wl_deflated_zipfile_load_frames"),
           "e_loop_calls": args.loop, "e_pl_crc32_ms": [round(t, 4) for t in crc_ms], "e_inflate_launch_ms": [round(t, 3) for t in inflate_ms],
           "e_pl_crc32_gb_per_s": round(total / (min(crc_ms) * 1e-3) / 1e9, 1),
           "e_inflate_output_gb_per_s": round(total / (min(inflate_ms) * 1e-3) / 1e9, 3),
           "f_zlib_crc32_one_thread_ms": [round(t, 2) for t in host_crc_ms],
           "f_zlib_crc32_gb_per_s": round(total / (min(host_crc_ms) * 1e-3) / 1e9, 2),
           "crc_pair_faster_than_zlib": max(crc_ms) < min(host_crc_ms),
           "same_pixels_and_crcs": bool(equal)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not equal:
        sys.exit(1)


if __name__ == "__main__":
    main()
