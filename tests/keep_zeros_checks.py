"""Checks of pl_median3_threshold_profile_fwxm_cells_keep_u16 -- the EPID step's threshold launch with a table of the cells
(32 rows x 64 columns) of `out` that hold zeros already, which it does not store again -- shared by
tests/test_gpu_keep_zeros.py (MI355X) and tests/test_emulated_keep_zeros.py (the CPU emulator of tests/hipemu).

The reference everywhere is pl_median3_threshold_profile_fwxm_cells_u16 on the same inputs with a FRESH `out` filled with
0xFFFF; frames, profile, peaks, fwxm and record are compared bit for bit, and the workspace must be zero afterwards.  The side
under test keeps ONE `out` (0xFFFF before the first call) and ONE table (0x5A before the first call: `reset` must not read it)
across its calls.

Shapes: n = 3, h = 70 (row groups of 32, 32 and 6 rows in one band that is not full), w = 584 (a full wave of 512 columns and a
partial wave whose last cell is 8 columns wide) and 576 (ends on a cell).  The cell table handed to both sides is the true
cell maxima of scipy's 3x3 median: the smallest table the contract allows, so "maximum == threshold" is decided by the launch.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import step_tail_checks as checks

N, H = 3, 70
WIDTHS = (584, 576)
THR = 15000
SENTINEL = 0x1234


def cell_max(x):
    """[n][ceil(h/32)][ceil(w/64)]: maximum of scipy's 3x3 median over each cell"""
    from scipy.ndimage import median_filter

    n, h, w = x.shape
    med = np.stack([median_filter(f, size=3, mode="reflect") for f in x])
    rg, cc = -(-h // 32), -(-w // 64)
    pad = np.zeros((n, rg * 32, cc * 64), dtype=x.dtype)
    pad[:, :h, :w] = med
    return pad.reshape(n, rg, 32, cc, 64).max(axis=(2, 4))


def cells_all_zero(out):
    """[n][ceil(h/32)][ceil(w/64)] bool: every pixel of the cell (its part inside the frame) is 0"""
    n, h, w = out.shape
    rg, cc = -(-h // 32), -(-w // 64)
    pad = np.zeros((n, rg * 32, cc * 64), dtype=out.dtype)
    pad[:, :h, :w] = out
    return pad.reshape(n, rg, 32, cc, 64).max(axis=(2, 4)) == 0


def _blocks(w, places, seed):
    """uint16 [3, 70, w]: noise far below THR and 4 x 4 blocks (their medians survive in 12 pixels); places = per frame
    [(row, column, value), ...]"""
    x = np.random.default_rng(seed).integers(50, 150, (N, H, w)).astype(np.uint16)
    for i, frame in enumerate(places):
        for r, c, v in frame:
            x[i, r:r + 4, c:c + 4] = v
    return x


def batch_a(w):
    """blocks across a lane-group edge (columns 63 | 64) and the wave edge (511 | 512); across a row-group edge (rows 31 | 32)
    and on a corner of four cells; in the frame's corner, plus one whose median EQUALS the threshold (needed) and one at
    threshold - 1 (below)"""
    return _blocks(w, ([(10, 62, 30000), (50, 510, 30000)],
                       [(30, 200, 30000), (30, 62, 30000)],
                       [(H - 4, w - 4, 30000), (4, 70, THR), (40, 300, THR - 1)]), 9)


def batch_b(w):
    """the same kinds of places, in other frames: every cell batch_a needs is below here and the other way round"""
    return _blocks(w, ([(30, 200, 30000), (H - 4, w - 4, 30000)],
                       [(10, 62, 30000), (40, 300, THR)],
                       [(50, 510, 30000), (30, 62, 30000)]), 10)


def thresholds(dev, value=THR):
    import torch

    return torch.full((N,), value, dtype=torch.int32, device=dev)


def _fill(t, pattern):
    import torch

    (t.view(torch.int16) if t.dtype == torch.uint16 else t.view(torch.int8)).fill_(pattern)
    return t


def outputs_ffff(x):
    o = checks.new_outputs(x)
    _fill(o["out"], -1)                                        # 0xFFFF: a pixel the launch does not store shows
    return o


def _tail_args(prm, o, ws, lo, st):
    p = checks._ptr
    return (C.byref(prm), 1, p(o["prof"], lo), p(o["cnt"], lo), p(o["idx"], lo), p(o["lb"], lo), p(o["rb"], lo), p(o["props"], lo),
            p(o["status"], lo), p(o["fwxm"], lo), p(o["record"], lo), p(ws, lo), st)


def run_cells(x, thr, table, lo=0, m=None):
    """the reference: the cells launch on fresh outputs (0xFFFF / sentinels), frames [lo, lo + m)"""
    import torch

    from pylinac_amd import _lib, ops
    from pylinac_amd._lib import check

    lib = _lib.load()
    n, h, w = x.shape
    m = n - lo if m is None else m
    o = outputs_ffff(x)
    ws = torch.zeros((n, w + 1), dtype=torch.int64, device=x.device)
    prm = ops.make_peak_params(w, fwxm_height=0.5, max_number=1)
    p = checks._ptr
    check(lib.pl_median3_threshold_profile_fwxm_cells_u16(
        p(x, lo), p(o["out"], lo), m, h, w, p(thr, lo), p(table, lo),
        *_tail_args(prm, o, ws, lo, torch.cuda.current_stream().cuda_stream)), "cells tail")
    assert int(ws.cpu().abs().sum()) == 0, "reference: workspace not returned to zero"
    return o


class Kept:
    """ONE `out` (0xFFFF) and ONE kept-zero table (0x5A) for a sequence of calls of the launch under test"""

    def __init__(self, dev, w):
        import torch

        self.dev, self.w = dev, w
        self.out = _fill(torch.empty((N, H, w), dtype=torch.uint16, device=dev), -1)
        self.zeroed = _fill(torch.empty((N, -(-H // 32), -(-w // 64)), dtype=torch.uint8, device=dev), 0x5A)
        self.ws = torch.zeros((N, w + 1), dtype=torch.int64, device=dev)

    def run(self, x, thr, table, reset, lo=0, m=None):
        """-> every output of the call (fresh sentinel buffers, except `out` = the kept one)"""
        import torch

        from pylinac_amd import _lib, ops
        from pylinac_amd._lib import check

        lib = _lib.load()
        n, h, w = x.shape
        m = n - lo if m is None else m
        o = checks.new_outputs(x)
        o["out"] = self.out
        prm = ops.make_peak_params(w, fwxm_height=0.5, max_number=1)
        p = checks._ptr
        check(lib.pl_median3_threshold_profile_fwxm_cells_keep_u16(
            p(x, lo), p(self.out, lo), m, h, w, p(thr, lo), p(table, lo), p(self.zeroed, lo), reset,
            *_tail_args(prm, o, self.ws, lo, torch.cuda.current_stream().cuda_stream)), "keep tail")
        assert int(self.ws.cpu().abs().sum()) == 0, "workspace not returned to zero"
        return o

    def poke(self, frame, row, col, value=SENTINEL):
        """write into `out` behind the launch's back"""
        import torch

        self.out.view(torch.int16)[frame, row, col] = value

    def pixel(self, frame, row, col):
        import torch

        return int(self.out.view(torch.int16)[frame, row, col]) & 0xFFFF


def assert_table(kept, table_np, thr, frames=slice(None), tag=""):
    """entry set => the cell of `out` is all zero; cellmax < t => entry set; cellmax >= t => entry clear"""
    z = kept.zeroed.cpu().numpy()[frames] != 0
    out = kept.out.cpu().numpy()[frames]
    t = thr.cpu().numpy()[frames][:, None, None]
    assert cells_all_zero(out)[z].all(), (tag, "an entry is set over a cell that is not all zero")
    below = table_np[frames] < t
    assert (z == below).all(), (tag, "entries differ from cellmax < threshold", np.argwhere(z != below).tolist())


_CASES = {}


def case(dev, w):
    """(frames A, frames B, table A, table B, numpy tables) on the device, computed once"""
    import torch

    key = (str(dev), w)
    if key not in _CASES:
        a, b = batch_a(w), batch_b(w)
        ta, tb = cell_max(a), cell_max(b)
        up = lambda v: torch.from_numpy(v).to(dev)
        _CASES[key] = (up(a), up(b), up(ta), up(tb), ta, tb)
    return _CASES[key]


def check_sequence(dev, w):
    """A -> B -> A on one `out` + table, reset on the first call only: equal to the reference after every call, and the table
    invariant holds; cells go below -> needed -> below and needed -> below -> needed"""
    xa, xb, ta, tb, ta_np, tb_np = case(dev, w)
    thr = thresholds(dev)
    flips = (ta_np >= THR) != (tb_np >= THR)
    assert flips.sum() >= 8 and ((ta_np >= THR) & flips).any() and ((tb_np >= THR) & flips).any()
    assert (ta_np == THR).any() and (ta_np == THR - 1).any() and (tb_np == THR).any()    # maximum == threshold: needed
    kept = Kept(dev, w)
    for call, (x, t, t_np) in enumerate(((xa, ta, ta_np), (xb, tb, tb_np), (xa, ta, ta_np))):
        got = kept.run(x, thr, t, reset=1 if call == 0 else 0)
        checks.assert_same(run_cells(x, thr, t), got, ("call", call))
        assert_table(kept, t_np, thr, tag=("call", call))
    z = kept.zeroed.cpu().numpy()
    assert not z[2, 0, 1] and z[2, 1, 4]                       # batch A: (4, 70) holds THR, (40, 300) holds THR - 1


def check_stores_are_skipped(dev, w):
    """a pixel written behind the launch's back into a cell whose entry is set survives the next call (the cell is not stored)
    and is gone after a call with reset; a needed cell and a cell whose entry is clear are stored whatever they held"""
    xa, _, ta, _, ta_np, _ = case(dev, w)
    thr = thresholds(dev)
    kept = Kept(dev, w)
    ref = run_cells(xa, thr, ta)
    checks.assert_same(ref, kept.run(xa, thr, ta, reset=1), "first call")
    # frame 0: row group 2 needs nothing (its wave takes the path without loads): pixel (66, 200) lies in its cell (2, 3); row
    # group 0 holds the block at (10, 62) (its wave loads and computes): pixel (3, 330) lies in its cell (0, 5), which is below
    assert (ta_np[0, 2] < THR).all() and ta_np[0, 0, 0] >= THR and ta_np[0, 0, 5] < THR
    kept.poke(0, 66, 200)
    kept.poke(0, 3, 330)
    kept.poke(0, 11, 63, 0x4321)                               # in the needed cell (0, 0): stored over
    got = kept.run(xa, thr, ta, reset=0)
    assert kept.pixel(0, 66, 200) == SENTINEL and kept.pixel(0, 3, 330) == SENTINEL, "a skipped cell was stored"
    assert kept.pixel(0, 11, 63) == 30000
    kept.poke(0, 66, 200, 0)
    kept.poke(0, 3, 330, 0)
    checks.assert_same(ref, got, "everything but the two sentinels")
    kept.poke(0, 66, 200)
    kept.poke(0, 3, 330)
    checks.assert_same(ref, kept.run(xa, thr, ta, reset=1), "reset rewrites")
    assert_table(kept, ta_np, thr, tag="after reset")


def check_sub_range(dev, w):
    """frames [1, 3) through pointer offsets: frame 0's pixels and entries are left alone"""
    import torch

    xa, xb, ta, tb, _, tb_np = case(dev, w)
    thr = thresholds(dev)
    kept = Kept(dev, w)
    kept.run(xa, thr, ta, reset=1)
    _fill(kept.out[0], 0x0BAD)
    _fill(kept.zeroed[0], 0x77)
    got = kept.run(xb, thr, tb, reset=0, lo=1, m=2)
    ref = run_cells(xb, thr, tb, lo=1, m=2)
    assert bool((kept.out[0].view(torch.int16).cpu() == 0x0BAD).all()), "frame 0 was stored"
    assert bool((kept.zeroed[0].cpu() == 0x77).all()), "frame 0's entries were written"
    _fill(got["out"][0], -1)                                   # (the reference's frame 0 is its untouched 0xFFFF)
    checks.assert_same(ref, got, "sub-range")
    assert_table(kept, tb_np, thr, frames=slice(1, 3), tag="sub-range")


def check_threshold_above_everything(dev, w):
    """nothing is needed: the first call stores zeros everywhere and sets every entry, the second stores NOTHING (every pixel
    of `out`, overwritten with 0xFFFF in between, keeps it) while profile, peaks and record equal the reference's"""
    import torch

    xa, _, ta, _, ta_np, _ = case(dev, w)
    thr = thresholds(dev, 70000)
    kept = Kept(dev, w)
    ref = run_cells(xa, thr, ta)
    checks.assert_same(ref, kept.run(xa, thr, ta, reset=1), "first call")
    assert int(kept.out.cpu().to(torch.int32).abs().sum()) == 0 and bool((kept.zeroed.cpu() != 0).all())
    _fill(kept.out, -1)
    got = kept.run(xa, thr, ta, reset=0)
    assert bool((kept.out.view(torch.int16).cpu() == -1).all()), "a pixel was stored"
    got["out"] = ref["out"]
    checks.assert_same(ref, got, "second call: everything but the frames")
    assert bool((kept.zeroed.cpu() != 0).all())
    kept.run(xa, thr, ta, reset=1)
    assert int(kept.out.cpu().to(torch.int32).abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------------- pipeline level
PIPE_SHAPE = (4, 128, 576)


def _stretched(fr):
    """bench.py's "#2w" recipe: the frames stretched to the full 16-bit range (every frame takes the full-range Otsu kernel)"""
    import torch

    q = torch.quantile(fr[0].to(torch.float32).flatten()[::16], torch.tensor([0.01, 0.99], device=fr.device))
    lo_q, hi_q = float(q[0]), float(q[1])
    blk = ((fr.to(torch.float32) - lo_q) * (64500.0 / (hi_q - lo_q)) + 500.0).round().clamp(0, 65535)
    wide = torch.empty_like(fr)
    wide.view(torch.int16)[:] = blk.to(torch.int32).bitwise_and_(0xFFFF).to(torch.int16)
    return wide


def _snapshot(res):
    d = {k: getattr(res, k).cpu().clone() for k in ("frames", "profile", "threshold", "fwxm", "status")}
    d["record"] = res.record().cpu().clone()
    return d


def _same(a, b, tag):
    import torch

    for k in a:
        p, q = a[k], b[k]
        if p.dtype == torch.float64:
            assert torch.equal(torch.isnan(p), torch.isnan(q)) and torch.equal(p[~torch.isnan(p)], q[~torch.isnan(q)]), (tag, k)
        else:
            assert torch.equal(p, q), (tag, k)


def _against_oracle(snap, frames_np, tag):
    from oracle import pylinac_oracle as oracle

    ref_out, ref_prof, ref_rec = oracle.epid_pipeline(frames_np)
    assert np.array_equal(snap["frames"].numpy(), ref_out), (tag, "thresholded frames differ")
    assert np.array_equal(snap["profile"].numpy(), ref_prof), (tag, "profiles differ")
    rec = snap["record"].numpy()
    assert np.array_equal(rec[:, :3], ref_rec[:, :3]), (tag, "threshold / peak index differ")
    assert np.allclose(rec, ref_rec, rtol=1e-12, atol=0, equal_nan=True), (tag, "peak record differs")


def _pipe_table_ok(pipe, tag):
    z = pipe.zeroed.cpu().numpy() != 0
    assert cells_all_zero(pipe.out.cpu().numpy())[z].all(), (tag, "an entry is set over a cell that is not all zero")
    below = pipe.cellmax.cpu().numpy().astype(np.int64) < pipe.thr.cpu().numpy()[:, None, None]
    assert (z == below).all(), (tag, "entries differ from cellmax < threshold")
    return float(below.mean())


def check_pipeline(dev):
    """two batches (fields at different places) alternately through ONE EpidPipeline, three runs: each == the oracle and == a
    fresh EpidPipeline(keep_zeros=False); an external write into `out` shows until forget_out(); the full-range stretch (whose
    cell table the full-range Otsu kernel writes) once, on the same pipeline"""
    import torch

    from pylinac_amd.pipeline import EpidPipeline
    from pylinac_amd.synthetic import epid_open_field_frames

    n, h, w = PIPE_SHAPE
    # (30 mm fields: 89 pixels inside the 128 x 576 frame, centres up to +-5 pixels apart; made on the host for both backends)
    batches = [epid_open_field_frames(n, h, w, seed0=s, field_mm=30.0).to(dev) for s in (1000, 5000)]
    want = []
    for i, fr in enumerate(batches):
        plain = EpidPipeline(n, h, w, dev, keep_zeros=False)
        want.append(_snapshot(plain.run(fr)))
        _against_oracle(want[i], fr.cpu().numpy(), ("keep_zeros=False", i))
    assert not torch.equal(want[0]["frames"], want[1]["frames"])
    pipe = EpidPipeline(n, h, w, dev)
    assert pipe.tail == "in_launch" and pipe.keep_zeros
    for run, i in enumerate((0, 1, 0)):
        _same(want[i], _snapshot(pipe.run(batches[i])), ("run", run))
        share = _pipe_table_ok(pipe, ("run", run))
        assert 0.2 < share < 0.95, share                       # there are cells to skip, and cells to store
    assert int(pipe.tail_ws.cpu().abs().sum()) == 0
    # an external write into a cell the table knows as zero: the next run leaves it (the contract), forget_out() repairs it
    z = pipe.zeroed.cpu().numpy()
    f, rg, cc = (int(v) for v in np.argwhere(z != 0)[0])
    pipe.out.view(torch.int16)[f, rg * 32 + 1, cc * 64 + 2] = SENTINEL
    got = _snapshot(pipe.run(batches[0]))
    assert int(got["frames"].view(torch.int16)[f, rg * 32 + 1, cc * 64 + 2]) == SENTINEL
    pipe.forget_out()
    _same(want[0], _snapshot(pipe.run(batches[0])), "after forget_out")
    _same(want[0], _snapshot(pipe.run(batches[0])), "the run after that")
    _pipe_table_ok(pipe, "after forget_out")
    wide = _stretched(batches[0])
    res = _snapshot(pipe.run(wide))
    assert bool((pipe.flag.cpu() == 1).all()), "the stretched frames did not take the full-range kernel"
    _against_oracle(res, wide.cpu().numpy(), "full range")
    _same(_snapshot(EpidPipeline(n, h, w, dev, keep_zeros=False).run(wide)), res, "full range")
    _pipe_table_ok(pipe, "full range")
    _same(want[1], _snapshot(pipe.run(batches[1])), "back to the window kernel")


# ------------------------------------------------------------------------------- the pipeline's bookkeeping, small enough
SMALL_SHAPE = (2, 64, 128)                                     # 2 x 2 cells per frame


def _small_batches(dev):
    """two batches of 2 x 64 x 128: noise and one bright rectangle per frame, in the top left cell (A) or in the bottom right
    one (B), so far inside it that the blurred edge stays in the cell: the other three cells lie below the Otsu threshold"""
    import torch

    n, h, w = SMALL_SHAPE
    out = []
    for seed, (r, c) in ((21, (6, 10)), (22, (42, 78))):
        x = np.random.default_rng(seed).integers(900, 1100, (n, h, w)).astype(np.uint16)
        for i in range(n):
            x[i, r + i:r + i + 14, c:c + 36] = 30000 + 1000 * i
        out.append(torch.from_numpy(x).to(dev))
    return out


def _partial_run(pipe, frames, lo, m):
    """one piece of a run_from_host pass: frames [lo, lo + m) only"""
    from unittest import mock

    import torch

    pipe._stage_free = []
    main = torch.cuda.current_stream()
    if hasattr(main, "wait_event"):
        ready = torch.cuda.Event()
        ready.record(main)
        return pipe.run(frames, chunks=[((lo, m), ready)])

    class Stream:                                              # the emulator's null stream knows no events
        cuda_stream = 0

        def wait_event(self, event):
            pass

    class Event:
        def record(self, stream=None):
            pass

    with mock.patch.object(torch.cuda, "current_stream", lambda device=None: Stream()), \
            mock.patch.object(torch.cuda, "Event", Event):
        return pipe.run(frames, chunks=[((lo, m), Event())])


def check_pipeline_bookkeeping(dev):
    """EpidPipeline's per-frame "entries describe out" state: partial passes, forget_out() followed by a partial pass, and
    keep_zeros switched off for one run and on again -- each result == a fresh EpidPipeline(keep_zeros=False)"""
    import torch

    from pylinac_amd.pipeline import EpidPipeline

    n, h, w = SMALL_SHAPE
    a, b = _small_batches(dev)
    want = [_snapshot(EpidPipeline(n, h, w, dev, keep_zeros=False).run(x)) for x in (a, b)]
    for snap in want:                                          # the layout the cases below rely on: one needed cell per frame
        assert (cells_all_zero(snap["frames"].numpy()).sum(axis=(1, 2)) == 3).all()
    assert not torch.equal(want[0]["frames"], want[1]["frames"])
    pipe = EpidPipeline(n, h, w, dev)
    assert pipe.tail == "in_launch" and pipe.keep_zeros and pipe._zeroed_valid == [False, False]
    _same(want[0], _snapshot(pipe.run(a)), "first run")
    assert pipe._zeroed_valid == [True, True]
    assert _pipe_table_ok(pipe, "first run") == 0.75
    # a partial pass: frame 1 of B, frame 0 stays what A left
    mixed = torch.cat([a[:1], b[1:]])
    _partial_run(pipe, mixed, 1, 1)
    got = pipe.out.cpu()
    assert torch.equal(got[0], want[0]["frames"][0]) and torch.equal(got[1], want[1]["frames"][1])
    _pipe_table_ok(pipe, "partial pass")
    # forget_out(), then a partial pass: frame 0 is known again, frame 1 is not -> the next full run rewrites everything,
    # a pixel written behind its back into a cell of frame 1 that was and stays zero included
    pipe.forget_out()
    _partial_run(pipe, mixed, 0, 1)
    assert pipe._zeroed_valid == [True, False]
    pipe.out.view(torch.int16)[1, 3, 100] = SENTINEL           # top right cell: below in A and in B
    _same(want[1], _snapshot(pipe.run(b)), "full run after forget_out + partial pass")
    assert pipe._zeroed_valid == [True, True]
    # keep_zeros off for one run: that run stores A's rectangle into a cell whose entry (from B) says zero; switched on again,
    # the next run must not trust that entry
    pipe.keep_zeros = False
    _same(want[0], _snapshot(pipe.run(a)), "keep_zeros=False")
    assert pipe._zeroed_valid == [False, False]
    pipe.keep_zeros = True
    _same(want[1], _snapshot(pipe.run(b)), "keep_zeros=True again")
    _same(want[1], _snapshot(pipe.run(b)), "and the run after it")
    _pipe_table_ok(pipe, "keep_zeros=True again")
    assert int(pipe.tail_ws.cpu().abs().sum()) == 0
