"""The checked Deflate path: what the checksums cost.

    python scripts/time_verify.py [--slices 128] [--files 64] [--size 1024] [--reps 3] [--loop 20] [--big-mib 1024]
                                  [--parent DIR] [--out FILE.json]

  a   ``pl_adler32`` over the members of a CT volume resident on the device (--slices files of 512 x 512 int16 with their
      headers: the buffer scripts/time_zip_batch.py times ``pl_crc32`` on), ``pl_crc32`` over the same ranges next to it, each
      alone between stream events around a sustained loop of --loop calls; ``zlib.adler32`` over the same bytes on one host thread;
      both pairs again over --big-mib MiB of random bytes in 64 ranges (beyond the 256 MiB memory-side cache: HBM's rate)
  b   ``png.load_frames`` of --files PNG files of --size x --size uint16 (PIL's files, scripts/time_png_batch.py's stack) with
      ``verify=False`` and ``verify=True``, alternating, --reps rounds each after a warm-up call of each; a repetition is the
      host clock from the files' bytes to a device synchronise; and the device part of both (``decode_png_streams``) between
      stream events
  c   with --parent DIR (a checkout of the parent commit with its library built): ``load_frames`` of the same files as plain
      calls in child processes, DIR's package and this one alternating, --reps rounds each: ``verify=False`` must cost what the
      parent's ``load_frames`` costs

Prints one JSON line (and writes it to --out).  --only-load is the child of (c)."""
from __future__ import annotations

import argparse
import io
import json
import os
import subprocess
import sys
import time
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def png_files(args):
    from PIL import Image

    from pylinac_amd import dicom
    from pylinac_amd.synthetic import pf_frames

    frames = dicom._to_numpy(pf_frames(args.distinct, args.size, args.size, seed0=2900))
    files = []
    for f in frames:
        out = io.BytesIO()
        Image.fromarray(f).save(out, format="PNG")
        files.append(out.getvalue())
    pick = [k % args.distinct for k in range(args.files)]
    return [files[k] for k in pick], frames[pick]


def only_load(args):
    import torch

    from pylinac_amd import png

    dev = torch.device("cuda:0")
    files, frames = png_files(args)
    want = torch.from_numpy(frames.view(np.int16)).to(dev)
    png.load_frames(files[:2], device=dev)
    png.load_frames(files, device=dev)
    ms, same = [], True
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = png.load_frames(files, device=dev).frames
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        same = same and torch.equal(x.view(torch.int16), want)
        del x
    print(json.dumps({"load_frames_ms": [round(t, 2) for t in ms], "same_pixels": bool(same)}))
    if not same:
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=128)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop", type=int, default=20)
    ap.add_argument("--big-mib", type=int, default=1024)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--package-root", default=os.path.dirname(HERE))
    ap.add_argument("--only-load", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    if args.only_load:
        return only_load(args)
    import torch

    import dicom_rle_checks as enc                          # the Part-10 writer of the tests (the product writes no DICOM)
    from pylinac_amd import _lib, dicom, png, zipstack
    from pylinac_amd.synthetic import catphan_volume

    dev = torch.device("cuda:0")
    ok = True

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

    # a: the Adler pair and the CRC pair over the volume's members
    volume = catphan_volume(seed=4100, n_slices=args.slices, size=512)
    sink = io.BytesIO()
    with zipfile.ZipFile(sink, "w") as zf:
        for k, f in enumerate(volume):
            zf.writestr(zipfile.ZipInfo(f"series/IM{k:04d}.dcm"), enc.native_file(f[None]), compress_type=zipfile.ZIP_STORED)
    stack = zipstack.extract(sink.getvalue(), device=dev)
    n, total, max_len = len(stack.members), int(stack.sizes.sum()), int(stack.sizes.max())
    lib = _lib.load()
    table = torch.from_numpy(np.concatenate([stack.offsets, stack.sizes])).to(dev)
    value = {k: torch.zeros(n, dtype=torch.uint32, device=dev) for k in ("adler32", "crc32")}
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    work = {k: torch.empty(int(getattr(lib, f"pl_{k}_work_bytes")(n, max_len)), dtype=torch.uint8, device=dev) for k in value}
    stream = torch.cuda.current_stream(dev).cuda_stream

    def checksum(which):
        def call():
            _lib.check(getattr(lib, f"pl_{which}")(stack.buffer.data_ptr(), stack.buffer.numel(), table[:n].data_ptr(), table[n:].data_ptr(),
                                                   n, max_len, value[which].data_ptr(), status.data_ptr(), work[which].data_ptr(), stream),
                       f"pl_{which}")
        return call

    adler_ms, crc_ms = [], []
    for _ in range(args.reps):                              # alternating
        adler_ms.append(looped(checksum("adler32"), args.loop))
        crc_ms.append(looped(checksum("crc32"), args.loop))
    blobs = [dicom._to_numpy(stack.member(k)).tobytes() for k in range(n)]
    as_list = lambda t: [int(v) & 0xFFFFFFFF for v in t.cpu().view(torch.int32).tolist()]   # noqa: E731
    ok = ok and as_list(value["adler32"]) == [zlib.adler32(b) for b in blobs] and as_list(value["crc32"]) == [zlib.crc32(b) for b in blobs]
    ok = ok and bool((status == 0).all())
    host_adler_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for b in blobs:
            zlib.adler32(b)
        host_adler_ms.append((time.perf_counter() - t0) * 1e3)
    del blobs

    # a2: the same pairs over a buffer beyond the 256 MiB memory-side cache: --big-mib of random bytes in 64 ranges
    big_n = 64
    big_len = (args.big_mib << 20) // big_n
    host_big = np.random.default_rng(2100).integers(0, 256, big_n * big_len, dtype=np.uint8)
    big = torch.from_numpy(host_big).to(dev)
    big_table = torch.from_numpy(np.concatenate([np.arange(big_n, dtype=np.int64) * big_len, np.full(big_n, big_len, dtype=np.int64)])).to(dev)
    big_value = {k: torch.zeros(big_n, dtype=torch.uint32, device=dev) for k in value}
    big_status = torch.zeros(big_n, dtype=torch.int32, device=dev)
    big_work = {k: torch.empty(int(getattr(lib, f"pl_{k}_work_bytes")(big_n, big_len)), dtype=torch.uint8, device=dev) for k in value}

    def big_checksum(which):
        def call():
            _lib.check(getattr(lib, f"pl_{which}")(big.data_ptr(), big.numel(), big_table[:big_n].data_ptr(), big_table[big_n:].data_ptr(),
                                                   big_n, big_len, big_value[which].data_ptr(), big_status.data_ptr(),
                                                   big_work[which].data_ptr(), stream), f"pl_{which}")
        return call

    big_adler_ms, big_crc_ms = [], []
    for _ in range(args.reps):
        big_adler_ms.append(looped(big_checksum("adler32"), 5))
        big_crc_ms.append(looped(big_checksum("crc32"), 5))
    ok = ok and as_list(big_value["adler32"]) == [zlib.adler32(host_big[k * big_len:(k + 1) * big_len]) for k in range(big_n)]
    ok = ok and as_list(big_value["crc32"]) == [zlib.crc32(host_big[k * big_len:(k + 1) * big_len]) for k in range(big_n)]
    ok = ok and bool((big_status == 0).all())
    del big, host_big

    # b: load_frames with and without the checks
    files, frames = png_files(args)
    want = torch.from_numpy(frames.view(np.int16)).to(dev)

    def clocked(verify):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = png.load_frames(files, device=dev, verify=verify)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, s.frames

    extra = {}
    images, dbuf, off, ln, frame, idat_bytes = png._stage(files, dev, extra)

    def device_part(verify):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        x, st = png.decode_png_streams(dbuf, off, ln, frame, args.files, args.size, args.size, 16, device=dev, idat_bytes=idat_bytes,
                                       verify=verify, chunks=extra["chunks"] if verify else None)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), x, st

    for v in (False, True):                                 # warm-up: code objects and the allocator's pools
        clocked(v)
        device_part(v)
    load_ms = {False: [], True: []}
    part_ms = {False: [], True: []}
    for _ in range(args.reps):
        for v in (False, True):
            t, x = clocked(v)
            load_ms[v].append(t)
            ok = ok and torch.equal(x.view(torch.int16), want)
            del x
    for _ in range(args.reps):
        for v in (False, True):
            t, x, st = device_part(v)
            part_ms[v].append(t)
            ok = ok and torch.equal(x.view(torch.int16), want) and bool((st == 0).all())
            del x

    # c: this package's load_frames against the parent commit's, child processes alternating
    ab = None
    if args.parent:
        ab = {"parent": [], "this": []}
        for _ in range(2):
            for name, root in (("parent", args.parent), ("this", os.path.dirname(HERE))):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-load", "--package-root", root, "--files", str(args.files),
                                    "--size", str(args.size), "--distinct", str(args.distinct), "--reps", str(args.reps)],
                                   capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
                    sys.exit(1)
                got = json.loads(r.stdout.strip().splitlines()[-1])
                ab[name].append(got["load_frames_ms"])
                ok = ok and got["same_pixels"]

    res = {"what": "pl_adler32 and pl_crc32 over a CT volume's members between stream events around a sustained loop, zlib.adler32 on "
                   "one host thread (a); png.load_frames with verify=False / True alternating, and their device part between stream "
                   "events (b); load_frames of the parent commit and of this one in alternating child processes (c)",
           "a_ranges": n, "a_bytes": total, "a_loop_calls": args.loop,
           "a_pl_adler32_ms": [round(t, 4) for t in adler_ms], "a_pl_crc32_ms": [round(t, 4) for t in crc_ms],
           "a_pl_adler32_gb_per_s": round(total / (min(adler_ms) * 1e-3) / 1e9, 1),
           "a_pl_crc32_gb_per_s": round(total / (min(crc_ms) * 1e-3) / 1e9, 1),
           "a_zlib_adler32_one_thread_ms": [round(t, 2) for t in host_adler_ms],
           "a_zlib_adler32_gb_per_s": round(total / (min(host_adler_ms) * 1e-3) / 1e9, 2),
           "a2_bytes": big_n * big_len, "a2_ranges": big_n, "a2_loop_calls": 5,
           "a2_pl_adler32_ms": [round(t, 4) for t in big_adler_ms], "a2_pl_crc32_ms": [round(t, 4) for t in big_crc_ms],
           "a2_pl_adler32_gb_per_s": round(big_n * big_len / (min(big_adler_ms) * 1e-3) / 1e9, 1),
           "a2_pl_crc32_gb_per_s": round(big_n * big_len / (min(big_crc_ms) * 1e-3) / 1e9, 1),
           "b_files": args.files, "b_shape": [args.size, args.size], "b_dtype": "uint16", "b_chunks": int(extra["chunks"][0].size),
           "b_load_frames_verify_false_ms": [round(t, 2) for t in load_ms[False]],
           "b_load_frames_verify_true_ms": [round(t, 2) for t in load_ms[True]],
           "b_device_decode_verify_false_ms": [round(t, 3) for t in part_ms[False]],
           "b_device_decode_verify_true_ms": [round(t, 3) for t in part_ms[True]],
           "c_parent_load_frames_ms": ab["parent"] if ab else None, "c_this_load_frames_ms": ab["this"] if ab else None,
           "same_values": bool(ok)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
