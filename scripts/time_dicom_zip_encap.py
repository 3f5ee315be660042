"""ZIP archives of RLE Lossless and JPEG Lossless DICOM files: ``dicom.load_zip(encapsulated=True)`` against the path without it
-- ``zipfile`` reading every member on one host thread, then ``dicom.load_frames(jpeg_lossless=True)`` -- in one process.

    timeout 900 python scripts/time_dicom_zip_encap.py [--slices 128] [--distinct 4] [--reps 3] [--loop 20] [--out FILE.json]

  a   --slices members of 512 x 512 int16 CT-like slices (``dicom_jpegll_checks.ct_slices``, the generator of
      scripts/time_dicom_jpeg_lossless.py; --distinct different slices, repeated) as JPEG Lossless, archived at Deflate level 6
  b   the same slices as RLE Lossless members
  c   the same slices as native members
each loaded with ``load_zip`` and with ``zipfile`` + ``load_frames``; then, between stream events around a sustained loop of
--loop calls over the extracted JPEG archive: ``pl_zip_extract`` (the yardstick), the ``pl_dicom_encap_index`` call, and for a
variant whose every frame is split into three fragments the ``pl_copy_ranges`` call that lays them end to end.

The variants alternate over --reps repetitions after a warm-up call of each; a repetition is the host clock from the archive's
bytes to a device synchronise.  Prints one JSON line (and writes it to --out)."""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=128)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import dicom_jpegll_checks as jl                        # the Part-10 writers of the tests (the product writes no DICOM)
    import dicom_rle_checks as rl
    from pylinac_amd import dicom, zipstack

    dev = torch.device("cuda:0")
    distinct = jl.ct_slices(args.distinct, args.size)
    order = [k % args.distinct for k in range(args.slices)]
    frames = distinct[order]

    def archive(files):
        out = io.BytesIO()
        with zipfile.ZipFile(out, "w") as zf:
            for k, j in enumerate(order):
                zf.writestr(zipfile.ZipInfo(f"series/IM{k:04d}.dcm"), files[j], compress_type=zipfile.ZIP_DEFLATED, compresslevel=6)
        return out.getvalue()

    sets = {"jpegll": archive([jl.jpegll_file(f[None]) for f in distinct]), "rle": archive([rl.rle_file(f[None]) for f in distinct]),
            "native": archive([rl.native_file(f[None]) for f in distinct])}
    split = archive([jl.split_file(f[None], (1000, 40000)) for f in distinct])

    def on_device(data):
        t0 = time.perf_counter()
        x, _, _ = dicom.load_zip(data, device=dev, encapsulated=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    def on_host(data):
        t0 = time.perf_counter()
        with zipfile.ZipFile(io.BytesIO(data)) as zf:
            blobs = [zf.read(i) for i in zf.infolist()]
        t1 = time.perf_counter()
        x, _ = dicom.load_frames(blobs, device=dev, jpeg_lossless=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x, (t1 - t0) * 1e3

    def same(x):
        return bool(np.array_equal(dicom._to_numpy(x), frames))

    for data in sets.values():                              # warm-up: code objects and the allocator's pools
        on_device(data)
        on_host(data)
    ms = {f"{name}_{path}": [] for name in sets for path in ("load_zip", "zipfile_load_frames")}
    read_ms = {name: [] for name in sets}
    equal = True
    for _ in range(args.reps):
        for name, data in sets.items():
            t, x = on_device(data)
            ms[f"{name}_load_zip"].append(t)
            equal = equal and same(x)
            del x
            t, x, t_read = on_host(data)
            ms[f"{name}_zipfile_load_frames"].append(t)
            read_ms[name].append(t_read)
            equal = equal and same(x)
            del x
    t_split, x = on_device(split)
    equal = equal and same(x)
    del x

    # the calls alone: pl_zip_extract (the yardstick), the index call, the copy call of the split variant
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

    alone = {}
    for name, data in (("jpegll", sets["jpegll"]), ("split", split)):
        members, what, host, dbuf = zipstack.stage(data, dev)
        stack = zipstack.run(members, what, host, dbuf)
        out = torch.empty_like(stack.buffer)
        spec = ([m.data_offset for m in members], [m.compressed_size for m in members], [m.method for m in members],
                [m.crc32 for m in members], stack.offsets, stack.sizes)
        first = stack.offsets + np.asarray([dicom.read_part10(dicom._to_numpy(stack.member(k)).tobytes(), jpeg_lossless=True)[0].PixelData[0]
                                            for k in range(args.distinct)], dtype=np.int64)[order]
        first_d, end_d = torch.from_numpy(first).to(dev), torch.from_numpy(stack.offsets + stack.sizes).to(dev)
        index = dicom.index_encapsulated(stack.buffer, first_d, end_d, 16, 1, device=dev)
        frags, _, info, _ = index.host()
        equal = equal and not info[:, 0].any()
        alone[f"{name}_pl_zip_extract_ms"] = [round(looped(lambda: zipstack.extract_members(dbuf, *spec, device=dev, out=out), args.loop), 4)
                                              for _ in range(args.reps)]
        alone[f"{name}_pl_dicom_encap_index_ms"] = [
            round(looped(lambda: dicom.index_encapsulated(stack.buffer, first_d, end_d, 16, 1, device=dev, block=index.block), args.loop), 4)
            for _ in range(args.reps)]
        alone[f"{name}_fragments"] = int(info[:, 1].sum())
        if name == "split":
            moves = frags[:, :3].reshape(-1, 3)
            dst = np.concatenate([[0], np.cumsum((moves[:, 1] + 3) & ~3)[:-1]])
            staging = torch.empty(int(((moves[:, 1] + 3) & ~3).sum()), dtype=torch.uint8, device=dev)
            so, ln, do = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (moves[:, 0], moves[:, 1], dst))
            longest = int(moves[:, 1].max())
            from pylinac_amd import _lib
            status = torch.empty(len(dst), dtype=torch.int32, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream

            def copy_call():
                _lib.check(_lib.load().pl_copy_ranges(stack.buffer.data_ptr(), stack.buffer.numel(), staging.data_ptr(), staging.numel(),
                                                      so.data_ptr(), ln.data_ptr(), do.data_ptr(), len(dst), longest, status.data_ptr(),
                                                      stream), "pl_copy_ranges")

            alone["split_pl_copy_ranges_ms"] = [round(looped(copy_call, args.loop), 4) for _ in range(args.reps)]
            alone["split_copied_bytes"] = int(moves[:, 1].sum())
            alone["split_pl_copy_ranges_gb_per_s_read_plus_written"] = round(2 * int(moves[:, 1].sum()) / (min(alone["split_pl_copy_ranges_ms"]) * 1e-3) / 1e9, 1)
            equal = equal and not bool(status.any())
            got = dicom._to_numpy(staging)
            src = dicom._to_numpy(stack.buffer)
            equal = equal and all(np.array_equal(got[d:d + n], src[s:s + n]) for (s, n, _), d in zip(moves.tolist()[:12], dst.tolist()[:12]))

    res = {"what": "dicom.load_zip(encapsulated=True) against zipfile on one host thread + dicom.load_frames(jpeg_lossless=True) for a "
                   "CT-like series archived at Deflate level 6 as JPEG Lossless (a), RLE Lossless (b) and native (c) members; "
                   "pl_zip_extract, pl_dicom_encap_index and (every frame in three fragments) pl_copy_ranges alone between stream "
                   "events around a sustained loop; one process, alternating",
           "members": args.slices, "distinct_slices": args.distinct, "shape": [args.size, args.size], "dtype": "int16",
           "archive_bytes": {k: len(v) for k, v in sets.items()},
           **{k + "_ms": [round(t, 2) for t in v] for k, v in ms.items()},
           "zipfile_read_ms": {k: [round(t, 2) for t in v] for k, v in read_ms.items()},
           "split_jpegll_load_zip_ms": round(t_split, 2), "loop_calls": args.loop, **alone,
           "same_pixels": bool(equal)}
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
