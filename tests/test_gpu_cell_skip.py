"""The cell table of the EPID step: pl_median3_otsu16_cells leaves the largest 3x3 median of every cell of 32 rows x 64
columns, pl_median3_threshold_profile_fwxm_cells_u16 stores zeros for the cells it proves below the threshold without
reading them.  Nothing may change: the references are the entry points without the table (pl_median3_otsu16,
pl_median3_threshold_profile_fwxm_u16), scipy's median_filter and oracle.epid_pipeline; every comparison is exact.

Shapes: h = 72 is three row groups, the last of 8 rows; w = 584 is a second column block of 9 lanes whose last cell is one
lane wide, w = 576 ends on a cell.  72 x 584 < 65 536 pixels keeps the Otsu stage at one workgroup per frame; the 1024^2
pipeline case (n = 4) takes several per frame.
"""
from __future__ import annotations

import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import step_tail_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu

H = 72
WIDTHS = (584, 576)


def cell_max_reference(x):
    """[n][ceil(h/32)][ceil(w/64)]: maximum of scipy's 3x3 median over each cell"""
    from scipy.ndimage import median_filter

    n, h, w = x.shape
    med = np.stack([median_filter(f, size=3, mode="reflect") for f in x])
    rg, cc = -(-h // 32), -(-w // 64)
    pad = np.zeros((n, rg * 32, cc * 64), dtype=x.dtype)
    pad[:, :h, :w] = med
    return pad.reshape(n, rg, 32, cc, 64).max(axis=(2, 4))


def otsu_stage(dev, x, cells: bool):
    """-> thr, min, max, flag (int32 [n], device) and, with `cells`, the table (every entry preset to 0x5A5A)"""
    import torch

    from pylinac_amd import _lib
    from pylinac_amd._lib import check

    lib = _lib.load()
    n, h, w = x.shape
    st = torch.cuda.current_stream().cuda_stream
    thr, mn, mx, flag = (torch.full((n,), -7, dtype=torch.int32, device=dev) for _ in range(4))
    hist = torch.zeros((n, 65536), dtype=torch.int32, device=dev)
    scratch = torch.empty_like(x)
    args = (x.data_ptr(), scratch.data_ptr(), _lib.PL_U16, n, h, w, None, None, thr.data_ptr(), mn.data_ptr(), mx.data_ptr(),
            flag.data_ptr(), hist.data_ptr())
    if not cells:
        check(lib.pl_median3_otsu16(*args, st), "pl_median3_otsu16")
        return thr, mn, mx, flag
    table = torch.empty((n, -(-h // 32), -(-w // 64)), dtype=torch.uint16, device=dev)
    table.view(torch.int16).fill_(0x5A5A)
    check(lib.pl_median3_otsu16_cells(*args, table.data_ptr(), st), "pl_median3_otsu16_cells")
    return thr, mn, mx, flag, table


def outputs_ffff(x):
    import torch

    o = checks.new_outputs(x)
    o["out"].view(torch.int16).fill_(-1)                       # 0xFFFF: a pixel the launch does not store shows
    return o


def old_tail(x, thr):
    """the third stage without the table: the reference"""
    import torch

    ws = torch.zeros((x.shape[0], x.shape[2] + 1), dtype=torch.int64, device=x.device)
    return checks.run_in_launch(x, thr, outputs_ffff(x), ws)


def cells_tail(x, thr, table):
    """the third stage with the table, every output preset; the workspace must come back all zero"""
    import torch

    from pylinac_amd import _lib, ops
    from pylinac_amd._lib import check

    lib = _lib.load()
    n, h, w = x.shape
    o = outputs_ffff(x)
    ws = torch.zeros((n, w + 1), dtype=torch.int64, device=x.device)
    prm = ops.make_peak_params(w, fwxm_height=0.5, max_number=1)
    check(lib.pl_median3_threshold_profile_fwxm_cells_u16(
        x.data_ptr(), o["out"].data_ptr(), n, h, w, thr.data_ptr(), table.data_ptr(), C.byref(prm), 1, o["prof"].data_ptr(),
        o["cnt"].data_ptr(), o["idx"].data_ptr(), o["lb"].data_ptr(), o["rb"].data_ptr(), o["props"].data_ptr(),
        o["status"].data_ptr(), o["fwxm"].data_ptr(), o["record"].data_ptr(), ws.data_ptr(),
        torch.cuda.current_stream().cuda_stream), "cells tail")
    assert int(ws.cpu().abs().sum()) == 0, "workspace not returned to zero"
    return o


def table_frames(w):
    """uint16 [5, 72, w]: a noisy bump (the window kernel tallies it), a constant frame (every wave flat), the bump with hot
    pixels at 0 / 65535, noise over the whole 16-bit range (too wide for the window: the full-range kernel), and a flat frame
    with a 0 .. 65535 ramp that the window's sample misses (the window kernel tallies it, spills, and the full-range kernel
    tallies it again)"""
    rng = np.random.default_rng(5)
    x = np.empty((5, H, w), dtype=np.uint16)
    x[0] = checks.frames_for(1, H, w, 3)[0]
    x[1] = 12345
    x[2] = x[0]
    pos = rng.integers(0, H * w, 24)
    x[2].reshape(-1)[pos] = np.where(rng.random(24) > 0.5, 65535, 0)
    x[2, 40:43, 100:103] = 65535                              # a hot spot large enough for its median to survive
    x[3] = rng.integers(0, 65536, (H, w))
    x[4] = 7
    x[4, 16:19] = np.linspace(0, 65535, w).astype(np.uint16)  # three equal rows: the ramp survives the median
    return x


_CASES = {}


def table_case(dev, w):
    """(frames, old second stage, new second stage, scipy's cell maxima), computed once"""
    import torch

    if w not in _CASES:
        x = table_frames(w)
        t = torch.from_numpy(x).to(dev)
        _CASES[w] = (t, otsu_stage(dev, t, False), otsu_stage(dev, t, True), cell_max_reference(x))
    return _CASES[w]


@pytest.mark.parametrize("w", WIDTHS)
def test_table_holds_the_cell_maxima_of_the_medians(dev, w):
    t, old, new, want = table_case(dev, w)
    for a, b, name in zip(old, new[:4], ("thr", "min", "max", "flag")):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), name
    flag = new[3].cpu().numpy()
    got = new[4].cpu().numpy()
    print("flags", flag.tolist())
    assert flag[0] == 0 and flag[1] == 0 and flag[3] == 1 and flag[4] == 1     # both tally kernels took part
    for i in range(len(flag)):
        if flag[i] == 0:
            assert np.array_equal(got[i], want[i]), ("window kernel", i)
        else:
            assert (got[i] >= want[i]).all(), ("full-range kernel", i)
    assert np.array_equal(got, want)                           # the full-range kernel records true maxima as well
    assert (got[1] == 12345).all()
    assert got[2].max() == 65535 and want[4].max() > 60000


@pytest.mark.parametrize("w", WIDTHS)
def test_third_stage_with_the_table_equals_the_one_without(dev, w):
    """the second stage's thresholds and table; then everything kept (thr = 0), nothing kept (thr above every value), and a
    table that knows nothing (all 65535)"""
    import torch

    t, _, new, _ = table_case(dev, w)
    thr, table = new[0], new[4]
    checks.assert_same(old_tail(t, thr), cells_tail(t, thr, table), "otsu thresholds")
    zero = torch.zeros_like(thr)
    checks.assert_same(old_tail(t, zero), cells_tail(t, zero, table), "thr = 0")
    above = torch.full_like(thr, 70000)
    got = cells_tail(t, above, table)
    checks.assert_same(old_tail(t, above), got, "thr above everything")
    assert int(got["out"].cpu().to(torch.int32).abs().sum()) == 0
    blind = torch.empty_like(table)
    blind.view(torch.int16).fill_(-1)
    checks.assert_same(old_tail(t, thr), cells_tail(t, thr, blind), "table of 65535")


# a 4 x 4 block of one value keeps its median in 12 pixels (all but the corners)
def _block(x, i, r, c, v):
    x[i, r:r + 4, c:c + 4] = v


def _survivors(r, c):
    return [(r + a, c + b) for a in range(4) for b in range(4) if (a in (1, 2)) or (b in (1, 2))]


def test_blocks_across_lane_group_wave_and_row_group_edges(dev):
    """one surviving block per frame, straddling columns 63 | 64 (two cells of a wave), 511 | 512 (two waves) and rows
    31 | 32 (two row groups); everything else lies far below the threshold, so all other cells are skipped"""
    import torch

    w = 584
    places = ((10, 62), (50, 510), (30, 200), (30, 62), (66, 574))      # the last two: a corner of four cells, the frame's corner
    x = np.random.default_rng(9).integers(50, 150, (len(places), H, w)).astype(np.uint16)
    for i, (r, c) in enumerate(places):
        _block(x, i, r, c, 30000)
    t = torch.from_numpy(x).to(dev)
    table = otsu_stage(dev, t, True)[4]
    assert np.array_equal(table.cpu().numpy(), cell_max_reference(x))
    thr = torch.full((len(places),), 15000, dtype=torch.int32, device=dev)
    got = cells_tail(t, thr, table)
    checks.assert_same(old_tail(t, thr), got, "blocks")
    out = got["out"].cpu().to(torch.int32).numpy()
    for i, (r, c) in enumerate(places):
        want = np.zeros((H, w), dtype=np.int32)
        for p in _survivors(r, c):
            want[p] = 30000
        assert np.array_equal(out[i], want), places[i]


def test_cell_maximum_equal_to_the_threshold_is_kept(dev):
    """a cell whose largest median equals thr survives (the pixel test is m >= thr), one at thr - 1 is zero"""
    import torch

    w, thr_v = 584, 20000
    x = np.full((1, H, w), 100, dtype=np.uint16)
    _block(x, 0, 4, 70, thr_v)                                 # cell (0, 1)
    _block(x, 0, 40, 300, thr_v - 1)                           # cell (1, 4)
    t = torch.from_numpy(x).to(dev)
    table = otsu_stage(dev, t, True)[4]
    tab = table.cpu().numpy()
    assert tab[0, 0, 1] == thr_v and tab[0, 1, 4] == thr_v - 1
    thr = torch.full((1,), thr_v, dtype=torch.int32, device=dev)
    got = cells_tail(t, thr, table)
    checks.assert_same(old_tail(t, thr), got, "edge of the comparison")
    out = got["out"][0].cpu().to(torch.int32).numpy()
    want = np.zeros((H, w), dtype=np.int32)
    for p in _survivors(4, 70):
        want[p] = thr_v
    assert np.array_equal(out, want)


def _stretched(fr):
    """bench.py's "#2w" recipe: the frames stretched to the full 16-bit range (every frame takes the full-range kernel)"""
    import torch

    q = torch.quantile(fr[0].to(torch.float32).flatten()[::16], torch.tensor([0.01, 0.99], device=fr.device))
    lo_q, hi_q = float(q[0]), float(q[1])
    blk = ((fr.to(torch.float32) - lo_q) * (64500.0 / (hi_q - lo_q)) + 500.0).round().clamp(0, 65535)
    wide = torch.empty_like(fr)
    wide.view(torch.int16)[:] = blk.to(torch.int32).bitwise_and_(0xFFFF).to(torch.int16)
    return wide


def _against_oracle(res, frames_np):
    from oracle import pylinac_oracle as oracle

    ref_out, ref_prof, ref_rec = oracle.epid_pipeline(frames_np)
    assert np.array_equal(res.frames.cpu().numpy(), ref_out), "thresholded frames differ"
    assert np.array_equal(res.profile.cpu().numpy(), ref_prof), "profiles differ"
    rec = res.record().cpu().numpy()
    assert np.array_equal(rec[:, :3], ref_rec[:, :3]), "threshold / peak index differ"
    assert np.allclose(rec, ref_rec, rtol=1e-12, atol=0, equal_nan=True), "peak record differs"


@pytest.mark.parametrize("wide", (False, True), ids=("open_field", "full_range"))
def test_pipeline_against_the_oracle(dev, wide):
    """EpidPipeline.run (n = 4 at 1024^2: several Otsu workgroups per frame) on open fields and on their full-range stretch
    == oracle.epid_pipeline; the table it left == scipy's cell maxima; run_from_host == run"""
    import torch

    from pylinac_amd.pipeline import EpidPipeline
    from pylinac_amd.synthetic import epid_open_field_frames

    n, h, w = 4, 1024, 1024
    fr = epid_open_field_frames(n, h, w, seed0=1000, device=dev)
    if wide:
        fr = _stretched(fr)
    pipe = EpidPipeline(n, h, w, dev)
    assert pipe.tail == "in_launch"
    res = pipe.run(fr)
    torch.cuda.synchronize()
    flags = pipe.flag.cpu().numpy()
    assert (flags == (1 if wide else 0)).all(), flags
    _against_oracle(res, fr.cpu().numpy())
    # (buf_b is the Gaussian plane, which the oracle comparison above has just proved through its medians)
    assert np.array_equal(pipe.cellmax.cpu().numpy(), cell_max_reference(pipe.buf_b.cpu().numpy()))
    assert int(pipe.tail_ws.cpu().abs().sum()) == 0
    if dev.type == "cuda" and fr.device.type == "cuda":        # (the emulated device has no copy stream)
        want = {k: getattr(res, k).cpu().clone() for k in ("frames", "profile", "threshold", "fwxm", "status")}
        want["record"] = res.record().cpu().clone()
        got = pipe.run_from_host(fr.cpu().pin_memory(), chunks=3)
        torch.cuda.synchronize()
        for k, v in want.items():
            g = (got.record() if k == "record" else getattr(got, k)).cpu()
            if v.dtype == torch.float64:
                assert torch.equal(torch.isnan(v), torch.isnan(g)), k
                v, g = v[~torch.isnan(v)], g[~torch.isnan(g)]
            assert torch.equal(v, g), k
