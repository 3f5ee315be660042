"""Checks of pl_median3_threshold_profile_fwxm_u16 -- the EPID step's threshold launch with the tail (mean profile -> peaks ->
FWXM record -> record row) run inside it by the workgroup that finishes a frame last -- shared by tests/test_gpu_step_tail.py
(MI355X) and tests/test_emulated_step_tail.py (the CPU emulator of tests/hipemu).

The reference in every case is the sequence of launches it replaces, on the same inputs:
pl_median3_threshold_colsum_u16 -> pl_colsum_to_mean -> pl_find_peaks -> pl_fwxm_record, compared BIT FOR BIT.  Every output
buffer of both sides starts from the same sentinel fill, so "equal" also means that the new launch writes no element the
reference leaves alone (rows of frames without a peak, rows outside a sub-range).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

# the smallest shapes at which each mechanism of the launch can go wrong (a band = 128 rows, a column group = 512 columns)
SHAPES = ((1, 2, 8),          # one workgroup per frame: the first arrival is the last
          (2, 128, 64),       # exactly one band, a partial column group
          (3, 200, 520),      # two bands (the second short), two column groups (the second 8 columns wide), three thresholds
          (2, 130, 1032),     # three column groups, the last nearly empty; a second band of two rows
          (2, 3, 2056))       # the first width whose staged search would pass 48 KiB of LDS: the non-staging instantiation
KEYS_INT = ("out", "cnt", "idx", "lb", "rb", "status")
KEYS_F64 = ("prof", "props", "fwxm", "record")


def frames_for(n, h, w, seed):
    """uint16 [n,h,w]: a Gaussian bump across the columns (one FWXM peak) on a pedestal, plus noise"""
    rng = np.random.default_rng(seed)
    _, xx = np.mgrid[:h, :w]
    base = 20000 * np.exp(-0.5 * ((xx - w * 0.55) / (w * 0.18)) ** 2) + 3000
    return np.clip(base[None] + rng.normal(0, 400, (n, h, w)), 0, 65535).astype(np.uint16)


def new_outputs(x, n=None):
    """every output of the tail for n frames shaped like x's, filled with sentinels"""
    import torch

    dev = x.device
    n = x.shape[0] if n is None else n
    w = x.shape[2]
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)
    f64 = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=dev)
    out = torch.empty((n, *x.shape[1:]), dtype=torch.uint16, device=dev)
    out.view(torch.int16).fill_(-2)
    return dict(out=out, prof=f64(n, w), cnt=i32(n), idx=i32(n, 1), lb=i32(n, 1), rb=i32(n, 1), props=f64(n, 6, 1), status=i32(n),
                fwxm=f64(n, 8), record=f64(n, 9))


def _ptr(t, row):
    return t.data_ptr() + row * (t[0].numel() * t.element_size() if t.dim() > 1 else t.element_size())


def run_reference(x, thr, o, lo=0, m=None):
    """the four launches the new one replaces (+ the record as pipeline.EpidResult.record() assembles it), frames [lo, lo + m)"""
    import torch

    from pylinac_amd import _lib, ops
    from pylinac_amd._lib import check

    lib = _lib.load()
    n, h, w = x.shape
    m = n - lo if m is None else m
    st = torch.cuda.current_stream().cuda_stream
    prm = ops.make_peak_params(w, fwxm_height=0.5, max_number=1)
    colsum = torch.empty((m, w), dtype=torch.int64, device=x.device)
    check(lib.pl_median3_threshold_colsum_u16(_ptr(x, lo), _ptr(o["out"], lo), m, h, w, _ptr(thr, lo), colsum.data_ptr(), st), "colsum")
    check(lib.pl_colsum_to_mean(colsum.data_ptr(), m, w, h, _ptr(o["prof"], lo), st), "mean")
    check(lib.pl_find_peaks(_ptr(o["prof"], lo), m, w, w, C.byref(prm), 1, _ptr(o["cnt"], lo), _ptr(o["idx"], lo), _ptr(o["lb"], lo),
                            _ptr(o["rb"], lo), _ptr(o["props"], lo), _ptr(o["status"], lo), st), "peaks")
    check(lib.pl_fwxm_record(_ptr(o["cnt"], lo), _ptr(o["idx"], lo), _ptr(o["props"], lo), 1, m, _ptr(o["fwxm"], lo), st), "fwxm")
    o["record"][lo:lo + m] = torch.cat([thr[lo:lo + m].double()[:, None], o["fwxm"][lo:lo + m]], 1)
    return o


def run_in_launch(x, thr, o, ws, lo=0, m=None):
    """the one launch, frames [lo, lo + m), on workspace `ws` (int64 [n][w + 1], zero on entry)"""
    import torch

    from pylinac_amd import _lib, ops
    from pylinac_amd._lib import check

    lib = _lib.load()
    n, h, w = x.shape
    m = n - lo if m is None else m
    st = torch.cuda.current_stream().cuda_stream
    prm = ops.make_peak_params(w, fwxm_height=0.5, max_number=1)
    assert lib.pl_median3_threshold_profile_fwxm_covers(h, w, C.byref(prm)) == 1, (h, w)
    check(lib.pl_median3_threshold_profile_fwxm_u16(
        _ptr(x, lo), _ptr(o["out"], lo), m, h, w, _ptr(thr, lo), C.byref(prm), 1, _ptr(o["prof"], lo), _ptr(o["cnt"], lo),
        _ptr(o["idx"], lo), _ptr(o["lb"], lo), _ptr(o["rb"], lo), _ptr(o["props"], lo), _ptr(o["status"], lo), _ptr(o["fwxm"], lo),
        _ptr(o["record"], lo), _ptr(ws, lo), st), "in-launch tail")
    return o


def assert_same(a, b, tag):
    """every field equal bit for bit; float64 fields: NaN at the same places, equal elsewhere"""
    import torch

    for k in KEYS_INT:
        assert torch.equal(a[k].cpu(), b[k].cpu()), (tag, k)
    for k in KEYS_F64:
        p, q = a[k].cpu(), b[k].cpu()
        assert torch.equal(torch.isnan(p), torch.isnan(q)), (tag, k, "NaN positions")
        zero = torch.zeros((), dtype=torch.float64)
        assert torch.equal(torch.where(torch.isnan(p), zero, p), torch.where(torch.isnan(q), zero, q)), (tag, k)


def _thresholds(n, dev):
    import torch

    # frame 1 keeps everything, frame 2 (where there is one) nothing: 70000 lies above every uint16
    return torch.tensor(([9000, 0, 70000] * n)[:n], dtype=torch.int32, device=dev)


_REFERENCE = {}


def reference_case(dev, shape, seed=17):
    """(frames, thresholds, reference outputs) of a shape: computed once per device and shared (read-only) by the checks"""
    import torch

    key = (str(dev), shape, seed)
    if key not in _REFERENCE:
        n, h, w = shape
        x = torch.from_numpy(frames_for(n, h, w, seed)).to(dev)
        thr = _thresholds(n, dev)
        _REFERENCE[key] = (x, thr, run_reference(x, thr, new_outputs(x)))
    return _REFERENCE[key]


def check_shape(dev, shape):
    """one call on a fresh workspace == the reference; the record is cat(thr, fwxm); the workspace is zero again"""
    import torch

    x, thr, ref = reference_case(dev, shape)
    n, h, w = shape
    ws = torch.zeros((n, w + 1), dtype=torch.int64, device=dev)
    got = run_in_launch(x, thr, new_outputs(x), ws)
    assert_same(ref, got, shape)
    rec, want = got["record"].cpu(), torch.cat([thr.double()[:, None], got["fwxm"]], 1).cpu()
    assert torch.equal(torch.isnan(rec), torch.isnan(want)) and torch.equal(rec[~torch.isnan(rec)], want[~torch.isnan(want)]), shape
    assert int(ws.cpu().abs().sum()) == 0, (shape, "workspace not returned to zero")
    return n


def check_threshold_above_maximum(dev):
    """a frame among others whose threshold lies above its maximum: thresholded frame and profile all zero, no peak, the
    record's fields NaN / zero exactly where the reference has them"""
    import torch

    shape = (3, 200, 520)
    x, thr, ref = reference_case(dev, shape)
    assert int(thr[2]) > int(x[2].cpu().to(torch.int32).max())
    ws = torch.zeros((3, 521), dtype=torch.int64, device=dev)
    got = run_in_launch(x, thr, new_outputs(x), ws)
    assert_same(ref, got, "threshold above maximum")
    assert int(got["out"][2].cpu().to(torch.int32).abs().sum()) == 0 and float(got["prof"][2].cpu().abs().sum()) == 0.0
    assert int(got["cnt"][2]) == 0 and int(got["status"][2]) == 0
    rec = got["record"][2].cpu()
    assert float(rec[0]) == 70000.0 and float(rec[1]) == 0.0 and bool(torch.isnan(rec[2:]).all())
    assert int(got["cnt"][0]) == 1 and int(got["cnt"][1]) == 1      # the neighbours do have their peak


def check_workspace_reuse(dev, shape=(3, 200, 520)):
    """three consecutive calls on the SAME workspace with different frames and thresholds, nothing re-zeroed in between: a
    ticket or a column sum that was not returned to zero shows in the second call"""
    import torch

    n, h, w = shape
    ws = torch.zeros((n, w + 1), dtype=torch.int64, device=dev)
    for call in range(3):
        x = torch.from_numpy(frames_for(n, h, w, 30 + call)).to(dev)
        thr = torch.roll(_thresholds(n, dev), call) + 500 * call
        ref = run_reference(x, thr, new_outputs(x))
        got = run_in_launch(x, thr, new_outputs(x), ws)
        assert_same(ref, got, ("call", call))
    assert int(ws.cpu().abs().sum()) == 0


def check_sub_range(dev, shape=(4, 130, 520), lo=1, m=2):
    """frames [lo, lo + m) of a larger batch through pointer offsets (EpidPipeline.run_from_host's chunks): those rows equal the
    reference's, every row outside the range keeps its sentinel, and so does the workspace outside the range (poisoned here)"""
    import torch

    n, h, w = shape
    x = torch.from_numpy(frames_for(n, h, w, 23)).to(dev)
    thr = torch.tensor([9000, 4000, 12000, 0], dtype=torch.int32, device=dev)
    ref = run_reference(x, thr, new_outputs(x), lo, m)
    ws = torch.full((n, w + 1), 0x5A5A5A5A, dtype=torch.int64, device=dev)
    ws[lo:lo + m] = 0
    got = run_in_launch(x, thr, new_outputs(x), ws, lo, m)
    assert_same(ref, got, "sub-range")
    fresh = new_outputs(x)
    for k in KEYS_INT + KEYS_F64:
        for rows in (slice(0, lo), slice(lo + m, n)):
            p, q = got[k][rows].cpu(), fresh[k][rows].cpu()
            if p.dtype == torch.float64:
                assert bool(torch.isnan(p).all()), ("sub-range: written outside", k)
            else:
                assert torch.equal(p, q), ("sub-range: written outside", k)
    wsc = ws.cpu()
    assert int(wsc[lo:lo + m].abs().sum()) == 0 and bool((wsc[:lo] == 0x5A5A5A5A).all()) and bool((wsc[lo + m:] == 0x5A5A5A5A).all())


def check_pipeline(dev, shape=(4, 256, 512)):
    """EpidPipeline.run with the tail inside the launch (the default) == the same pipeline switched to the separate launches and
    to the colparts tail: every field of EpidResult and record(); the same through run_from_host's chunks; twice, so that the
    second step runs on the workspace the first one left"""
    import torch

    from pylinac_amd.pipeline import EpidPipeline
    from pylinac_amd.synthetic import epid_open_field_frames

    n, h, w = shape
    fr = epid_open_field_frames(n, h, w, seed0=1000, device=dev)
    new = EpidPipeline(n, h, w, dev)
    assert new.tail == "in_launch"

    def snapshot(res):
        d = {k: getattr(res, k).cpu().clone() for k in ("frames", "profile", "threshold", "fwxm", "status")}
        d["record"] = res.record().cpu().clone()
        return d

    def same(a, b, tag):
        for k in a:
            p, q = a[k], b[k]
            if p.dtype == torch.float64:
                assert torch.equal(torch.isnan(p), torch.isnan(q)) and torch.equal(p[~torch.isnan(p)], q[~torch.isnan(q)]), (tag, k)
            else:
                assert torch.equal(p, q), (tag, k)

    want = snapshot(EpidPipeline(n, h, w, dev, tail="separate").run(fr))
    assert int((want["fwxm"][:, 0] == 1).sum()) == n                    # the open fields do have their peak
    assert torch.equal(want["record"][:, 0], want["threshold"].double())
    same(want, snapshot(EpidPipeline(n, h, w, dev, tail="colparts").run(fr)), "colparts")
    first = new.run(fr)
    assert first.record_table is not None
    same(want, snapshot(first), "step 1")
    same(want, snapshot(new.run(fr)), "step 2")
    if dev.type == "cuda" and fr.device.type == "cuda":                 # (the emulated device has no copy stream)
        same(want, snapshot(new.run_from_host(fr.cpu().pin_memory(), chunks=3)), "run_from_host")
        torch.cuda.synchronize()
