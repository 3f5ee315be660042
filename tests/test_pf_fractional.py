"""picketfence.analyze_batch on float64 frames with fractional values (``measure_fractional=True``) and on leaf windows of
49-64 rows, against the oracle's restatement of PicketFence.analyze run on exactly the same arrays
(``pf_measure(normalize(ground(a)))``): picket count, spacing, every position, both leaf ends and the NaN pattern, bit for
bit.  The ``-m gpu`` tests run on the device; the rest run the same checks on the CPU-emulated kernels (tests/hipemu) with
small cases."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import pylinac_oracle as o  # noqa: E402

SLOPE, INTERCEPT = 0.0173, -7.25


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


def _cases(g):
    for name, mlc, tr in zip(g["names"], g["mlcs"], g["transposed"]):
        raw = np.ascontiguousarray(g[f"{name}.cropped"])
        yield str(name), str(mlc), ("LEFT_RIGHT" if bool(tr) else "UP_DOWN"), raw, float(g[f"{name}.dpmm"])


def _rescale(raw, slope=SLOPE, intercept=INTERCEPT):
    a = raw.astype(np.float64) * slope
    a += intercept                                   # pydicom's apply_rescale order
    return a


def _analyze(arr, dev, dpmm, mlc, orient, **kw):
    from pylinac_amd import picketfence as ppf

    x = torch.from_numpy(np.ascontiguousarray(arr if arr.ndim == 3 else arr[None])).to(dev)
    return ppf.analyze_batch(x, dpmm, mlc=mlc, orientation=orient, separate_leaves=True, **kw)


def _assert_oracle(res, k, arr, dpmm, mlc, orient, tag, **kw):
    """frame k of `res` == the oracle on `arr` (the exactness contract); -> the oracle's result"""
    ref = o.pf_measure(o.normalize(o.ground(arr)), dpmm, mlc=mlc, orientation=orient, separate_leaves=True, **kw)
    P = len(ref["peak_idxs"])
    assert int(res.picket_count[k]) == P, tag
    assert float(res.spacing[k]) == ref["spacing"], tag
    assert np.array_equal(res.picket_idx[k, :P].cpu().numpy(), ref["peak_idxs"]), tag
    assert res.leaf_nums == [n for n, _, _ in ref["leaves"]], tag
    for key, got in (("position", res.position), ("left", res.left), ("right", res.right)):
        g, want = got[k, :, :P].cpu().numpy(), ref[key]
        assert np.array_equal(np.isnan(g), np.isnan(want)), (tag, key)
        assert np.array_equal(g[~np.isnan(g)], want[~np.isnan(want)]), (tag, key)
    measured = ~np.isnan(ref["position"])
    assert not (res.status[k, :, :P].cpu().numpy()[measured] == 3).any(), tag
    return ref


def _same(a, b):
    for x, y in ((a.position, b.position), (a.left, b.left), (a.right, b.right)):
        if not torch.equal(torch.nan_to_num(x, nan=-1.0), torch.nan_to_num(y, nan=-1.0)):
            return False
    return (torch.equal(a.status, b.status) and torch.equal(a.picket_count, b.picket_count)
            and torch.equal(torch.nan_to_num(a.spacing, nan=-1.0), torch.nan_to_num(b.spacing, nan=-1.0)))


def _tall_frames(n, h, w, pixel_mm, pickets, dtype=np.uint16):
    from pylinac_amd.synthetic import pf_frames

    raw = pf_frames(n, h, w, seed0=4100, pixel_mm=pixel_mm, pickets=pickets).numpy()
    return raw if dtype == np.uint16 else _rescale(raw)


# ---- the checks (device-agnostic) ---------------------------------------------------------------------------------------

def check_fractional_golden(g, dev, names=None):
    """every golden crop (both orientations) as raw * 0.0173 - 7.25 float64, plus an extreme slope and a large negative
    intercept on the first one"""
    seen = 0
    for name, mlc, orient, raw, dpmm in _cases(g):
        if names is not None and name not in names:
            continue
        arr = _rescale(raw)
        assert not np.array_equal(arr, np.round(arr))                      # fractional values: the bridge refuses this frame
        res = _analyze(arr, dev, dpmm, mlc, orient, measure_fractional=True)
        ref = _assert_oracle(res, 0, arr, dpmm, mlc, orient, name)
        assert int((~np.isnan(ref["position"])).sum()) > 50, name
        seen += 1
    assert seen == (len(g["names"]) if names is None else len(names))
    name, mlc, orient, raw, dpmm = next(iter(_cases(g)))
    for slope, intercept in ((1e-6, 0.37), (SLOPE, -1.0e4)):
        arr = _rescale(raw, slope, intercept)
        res = _analyze(arr, dev, dpmm, mlc, orient, measure_fractional=True)
        _assert_oracle(res, 0, arr, dpmm, mlc, orient, (name, slope, intercept))


def check_integer_valued_equals_bridge(g, dev):
    """integer-valued float64 through the float64 kernels == the uint16 path, bit for bit; a mixed batch (fractional +
    integer-valued) measures both frames"""
    name, mlc, orient, raw, dpmm = next(iter(_cases(g)))
    base = _analyze(raw, dev, dpmm, mlc, orient)
    for arr in (raw.astype(np.float64), raw.astype(np.float64) - 1024.0):
        got = _analyze(arr, dev, dpmm, mlc, orient, measure_fractional=True)
        assert _same(got, base)
    mixed = np.stack([_rescale(raw), raw.astype(np.float64) + 3.0])
    res = _analyze(mixed, dev, dpmm, mlc, orient, measure_fractional=True)
    _assert_oracle(res, 0, mixed[0], dpmm, mlc, orient, "mixed fractional")
    for x, y in ((res.position[1], base.position[0]), (res.left[1], base.left[0]), (res.right[1], base.right[0])):
        assert torch.equal(torch.nan_to_num(x, nan=-1.0), torch.nan_to_num(y, nan=-1.0))
    assert torch.equal(res.status[1], base.status[0])
    # the default is unchanged: the bridge refuses the fractional frame, the integer-valued one is measured
    dflt = _analyze(mixed, dev, dpmm, mlc, orient)
    assert bool((dflt.status[0] == 3).all()) and torch.equal(dflt.status[1], base.status[0])


def check_tall_windows(dev, n, h, w, pickets, mlc="MLCI"):
    """10 mm leaves at 0.17 mm per pixel: windows of 58-59 rows, in uint16 and as fractional float64; at 0.15 mm (66-67 rows)
    the windows are refused (status 3)"""
    from pylinac_amd import picketfence as ppf

    dpmm = 1 / 0.17
    for dtype in (np.uint16, np.float64):
        fr = _tall_frames(n, h, w, 0.17, pickets, dtype)
        kw = {"measure_fractional": True} if dtype == np.float64 else {}
        res = _analyze(fr, dev, dpmm, mlc, "UP_DOWN", **kw)
        for k in range(n):
            ref = _assert_oracle(res, k, fr[k], dpmm, mlc, "UP_DOWN", ("tall", dtype.__name__, k))
            assert int((~np.isnan(ref["position"])).sum()) >= len(ref["leaves"]) * 3
        leaves, centers, widths = ppf.mlc_arrangement(ppf.MLC_ARRANGEMENTS[mlc])
        rows = [int(c * dpmm + h / 2 + wd * dpmm / 2) - int(c * dpmm + h / 2 - wd * dpmm / 2)
                for _, c, wd in ppf.leaves_in_view((h, w), dpmm, leaves, centers, widths)]
        assert 48 < max(rows) <= 64
    dpmm = 1 / 0.15
    for dtype in (np.uint16, np.float64):
        fr = _tall_frames(1, h, w, 0.15, pickets, dtype)
        kw = {"measure_fractional": True} if dtype == np.float64 else {}
        res = _analyze(fr, dev, dpmm, mlc, "UP_DOWN", **kw)
        P = int(res.picket_count[0])
        assert P > 0 and bool((res.status[0, :, :P] == 3).all()) and bool(torch.isnan(res.position[0, :, :P]).all())


def check_refusals(g, dev):
    """NaN / +inf / -inf frames inside a batch: status 3 in every window of that frame only; float32 still raises"""
    name, mlc, orient, raw, dpmm = next(iter(_cases(g)))
    good = _rescale(raw)
    single = _analyze(good, dev, dpmm, mlc, orient, measure_fractional=True)
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        f = good.copy()
        f[raw.shape[0] // 2, raw.shape[1] // 3] = v
        bad.append(f)
    batch = np.stack([bad[0], good, bad[1], bad[2]])
    res = _analyze(batch, dev, dpmm, mlc, orient, measure_fractional=True)
    for k in (0, 2, 3):
        assert bool((res.status[k] == 3).all()) and bool(torch.isnan(res.position[k]).all()), k
        assert bool(torch.isnan(res.left[k]).all()) and bool(torch.isnan(res.right[k]).all()), k
    assert torch.equal(res.status[1], single.status[0])
    assert torch.equal(torch.nan_to_num(res.position[1], nan=-1.0), torch.nan_to_num(single.position[0], nan=-1.0))
    with pytest.raises(TypeError):
        _analyze(raw.astype(np.float32), dev, dpmm, mlc, orient, measure_fractional=True)


def check_dicom_end_to_end(g, dev):
    """Part-10 bytes with RescaleSlope 0.0173 / RescaleIntercept -7.25 -> dicom.load_frames -> analyze_batch -> the oracle"""
    import importlib.util

    from pylinac_amd import dicom

    spec = importlib.util.spec_from_file_location("make_dicom_golden", os.path.join(ROOT, "tests", "golden", "make_dicom_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    name, mlc, orient, raw, dpmm = next(iter(_cases(g)))
    extra = (((0x0028, 0x1052), "DS", b"-7.25 "), ((0x0028, 0x1053), "DS", b"0.0173"))
    frames, _ = dicom.load_frames([gen.part10(raw, extra=extra)], device=dev)
    assert frames.dtype == torch.float64
    arr = frames[0].cpu().numpy()
    assert np.array_equal(arr, _rescale(raw))
    res = _analyze(arr, dev, dpmm, mlc, orient, measure_fractional=True)
    res2 = o.pf_measure(o.normalize(o.ground(arr)), dpmm, mlc=mlc, orientation=orient)
    _assert_oracle(res, 0, arr, dpmm, mlc, orient, "dicom")
    assert int((~np.isnan(res2["position"])).sum()) > 50


# ---- on the MI355X -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_fractional_golden_vs_oracle(golden, gpu):
    check_fractional_golden(golden("picketfence_mlc"), gpu)


@pytest.mark.gpu
def test_fractional_pf_frames_vs_oracle(gpu):
    from pylinac_amd.synthetic import pf_frames

    raw = pf_frames(4, 768, 1024, seed0=2000).numpy()
    fr = _rescale(raw)
    res = _analyze(fr, gpu, 1 / 0.390625, "MILLENNIUM", "UP_DOWN", num_pickets=10, measure_fractional=True)
    for k in range(len(fr)):
        _assert_oracle(res, k, fr[k], 1 / 0.390625, "MILLENNIUM", "UP_DOWN", k, num_pickets=10)


@pytest.mark.gpu
def test_integer_valued_float64_equals_uint16(golden, gpu):
    check_integer_valued_equals_bridge(golden("picketfence_mlc"), gpu)


@pytest.mark.gpu
def test_tall_windows(gpu):
    check_tall_windows(gpu, 2, 768, 1024, pickets=10)


@pytest.mark.gpu
def test_fractional_refusals(golden, gpu):
    check_refusals(golden("picketfence_mlc"), gpu)


@pytest.mark.gpu
def test_fractional_dicom_end_to_end(golden, gpu):
    check_dicom_end_to_end(golden("picketfence_mlc"), gpu)


# ---- on the CPU-emulated kernels -----------------------------------------------------------------------------------------

def test_emulated_fractional_golden_vs_oracle(golden, emulated):
    check_fractional_golden(golden("picketfence_mlc"), emulated, names=("hd", "agility_lr"))


def test_emulated_integer_valued_float64_equals_uint16(golden, emulated):
    check_integer_valued_equals_bridge(golden("picketfence_mlc"), emulated)


def test_emulated_tall_windows(emulated):
    check_tall_windows(emulated, 1, 400, 512, pickets=5)


def test_emulated_fractional_refusals(golden, emulated):
    check_refusals(golden("picketfence_mlc"), emulated)
