"""field_analysis.analyze_batch (FieldAnalysis over a stack of frames) against the reference's own analyze() on the golden frame
(tests/golden/dropin_field.npz), its centres and strips (field_strips.npz), and the per-image class sequence of
test_gpu_dropin.py::test_field_analysis_call_sequence_on_the_class_api on every frame of a batch.  The ``-m gpu`` tests run on the
device; the rest run the same checks on the CPU-emulated kernels (tests/hipemu) with small cases."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from pylinac_amd.field_analysis import analyze_batch  # noqa: E402


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


# ---- the per-image class sequence (test_gpu_dropin.py:139-205), one frame -> (results, protocol, horiz, vert) ----------------
def per_image(frame, dpi, kw, dev, invert=False):
    from pylinac_amd import field_analysis as pfa
    from pylinac_amd.image import ArrayImage
    from pylinac_amd.profile import SingleProfile

    protocols = {"VARIAN": dict(symmetry=pfa.symmetry_point_difference, flatness=pfa.flatness_dose_difference),
                 "ELEKTA": dict(symmetry=pfa.symmetry_pdq_iec, flatness=pfa.flatness_dose_ratio),
                 "SIEMENS": dict(symmetry=pfa.symmetry_area, flatness=pfa.flatness_dose_difference), "NONE": {}}
    img = ArrayImage(frame.copy(), dpi=float(dpi))
    img.check_inversion_by_histogram()
    if invert:
        img.invert()
    frame_t = torch.from_numpy(np.ascontiguousarray(img.array)).to(dev)[None]
    centering = kw.get("centering", "Beam center")
    vpos, hpos = kw.get("vert_position", 0.5), kw.get("horiz_position", 0.5)
    if centering != "Manual":
        vpos, hpos = pfa.determine_center(frame_t, centering)
    hv, _, _ = pfa.horiz_values(frame_t, hpos, kw.get("horiz_width", 0))
    vv, _, _ = pfa.vert_values(frame_t, vpos, kw.get("vert_width", 0))
    edge = kw.get("edge_detection_method", "Inflection Derivative")
    common = dict(dpmm=img.dpmm, interpolation=kw.get("interpolation", "Linear"), interpolation_resolution_mm=0.1, ground=True,
                  edge_detection_method=edge, normalization_method=kw.get("normalization_method", "Beam center"),
                  edge_smoothing_ratio=0.003, hill_window_ratio=kw.get("hill_window_ratio", 0.15))
    hp, vp = SingleProfile(hv[0].cpu().numpy(), **common), SingleProfile(vv[0].cpu().numpy(), **common)
    ser, ifr = 0.2, 0.8
    v_pen, h_pen = vp.penumbra(20, 80), hp.penumbra(20, 80)
    res = {"top_penumbra_mm": v_pen["left penumbra width (exact) mm"], "bottom_penumbra_mm": v_pen["right penumbra width (exact) mm"],
           "left_penumbra_mm": h_pen["left penumbra width (exact) mm"], "right_penumbra_mm": h_pen["right penumbra width (exact) mm"]}
    if edge == "Inflection Hill":
        res.update(top_penumbra_percent_mm=abs(v_pen["left gradient (exact) %/mm"]), bottom_penumbra_percent_mm=abs(v_pen["right gradient (exact) %/mm"]),
                   left_penumbra_percent_mm=abs(h_pen["left gradient (exact) %/mm"]), right_penumbra_percent_mm=abs(h_pen["right gradient (exact) %/mm"]))
    res["geometric_center_index_x_y"] = (hp.geometric_center()["index (exact)"], vp.geometric_center()["index (exact)"])
    res["beam_center_index_x_y"] = (hp.beam_center()["index (exact)"], vp.beam_center()["index (exact)"])
    vfull, hfull = vp.field_data(in_field_ratio=1.0, slope_exclusion_ratio=ser), hp.field_data(in_field_ratio=1.0, slope_exclusion_ratio=ser)
    res.update(field_size_vertical_mm=vfull["width (exact) mm"], field_size_horizontal_mm=hfull["width (exact) mm"],
               beam_center_to_top_mm=vfull["left distance->beam center (exact) mm"],
               beam_center_to_bottom_mm=vfull["right distance->beam center (exact) mm"],
               beam_center_to_left_mm=hfull["left distance->beam center (exact) mm"],
               beam_center_to_right_mm=hfull["right distance->beam center (exact) mm"],
               cax_to_top_mm=vfull["left distance->CAX (exact) mm"], cax_to_bottom_mm=vfull["right distance->CAX (exact) mm"],
               cax_to_left_mm=hfull["left distance->CAX (exact) mm"], cax_to_right_mm=hfull["right distance->CAX (exact) mm"])
    hfd, vfd = hp.field_data(in_field_ratio=ifr, slope_exclusion_ratio=ser), vp.field_data(in_field_ratio=ifr, slope_exclusion_ratio=ser)
    res.update(top_position_index_x_y=(hfd['"top" index (exact)'], vfd['"top" index (exact)']),
               top_horizontal_distance_from_cax_mm=hfd['"top"->CAX (exact) mm'], top_vertical_distance_from_cax_mm=vfd['"top"->CAX (exact) mm'],
               top_horizontal_distance_from_beam_center_mm=hfd['"top"->beam center (exact) mm'],
               top_vertical_distance_from_beam_center_mm=vfd['"top"->beam center (exact) mm'],
               left_slope_percent_mm=hfd["left slope (%/mm)"], right_slope_percent_mm=hfd["right slope (%/mm)"],
               top_slope_percent_mm=vfd["left slope (%/mm)"], bottom_slope_percent_mm=vfd["right slope (%/mm)"])
    prot = {}
    for name, calc in protocols[kw["protocol"]].items():
        for tag, prof in (("horizontal", hp), ("vertical", vp)):
            prot[f"{name}_{tag}"] = calc(prof, ifr, slope_exclusion_ratio=ser)
    return res, prot, np.asarray(hp.values, float), np.asarray(vp.values, float)


def _cases(g):
    return json.loads(str(g["cases"]))


def _batch(stack, dev, dpi, kw, **extra):
    t = torch.from_numpy(np.ascontiguousarray(stack)).to(dev)
    return analyze_batch(t, _dpmm(dpi), **kw, **extra)


def _dpmm(dpi):
    from pylinac_amd.image import ArrayImage

    return ArrayImage(np.zeros((2, 2), np.uint16), dpi=float(dpi)).dpmm


def _tol(kw):
    return dict(rtol=1e-5, atol=1e-5) if kw.get("edge_detection_method") == "Inflection Hill" else dict(rtol=1e-9, atol=1e-9)


def _assert_frame(res, k, want, tol, tag):
    results, prot, hv, vv = want
    assert set(res.results) == set(results), (tag, set(res.results) ^ set(results))
    assert set(res.protocol) == set(prot), tag
    assert int(res.status[k]) == 0, (tag, int(res.status[k]))
    for key, v in results.items():
        assert np.allclose(res.results[key][k].numpy().reshape(-1), np.asarray(v, float).reshape(-1), **tol), (tag, key)
    for key, v in prot.items():
        assert np.allclose(float(res.protocol[key][k]), v, **tol), (tag, key)
    assert np.allclose(res.horiz[k].cpu().numpy(), hv, **tol) and np.allclose(res.vert[k].cpu().numpy(), vv, **tol), tag


def _same(a, b, ka, kb):
    for key in a.results:
        if not np.array_equal(a.results[key][ka].numpy(), b.results[key][kb].numpy(), equal_nan=True):
            return False
    for key in a.protocol:
        if not np.array_equal(a.protocol[key][ka].numpy(), b.protocol[key][kb].numpy(), equal_nan=True):
            return False
    return True


# ---- checks shared by the emulated and the device runs --------------------------------------------------------------------------
def check_golden_cases(g, dev, cases=None):
    frame, dpi = g["frame"], float(g["dpi"])
    stack = np.stack([frame, np.fliplr(frame), np.roll(frame, (7, -11), axis=(0, 1)) + 50])
    for n, kw in enumerate(_cases(g)):
        if cases is not None and n not in cases:
            continue
        tol = _tol(kw)
        res = _batch(stack, dev, dpi, kw)
        # frame 0 against the reference's own analyze()
        assert set(res.results) == {k.split(".", 2)[2] for k in g.files if k.startswith(f"{n}.results.")}, n
        for key, v in res.results.items():
            assert np.allclose(v[0].numpy().reshape(-1), g[f"{n}.results.{key}"], equal_nan=True, **tol), (n, key)
        for key, v in res.protocol.items():
            assert np.allclose(float(v[0]), g[f"{n}.protocol.{key}"], **tol), (n, key)
        assert np.allclose(res.horiz[0].cpu().numpy(), g[f"{n}.horiz"], **tol) and np.allclose(res.vert[0].cpu().numpy(), g[f"{n}.vert"], **tol)
        for k in range(3):
            _assert_frame(res, k, per_image(stack[k], dpi, kw, dev), tol, (n, k))


def check_centres_and_strips(g, dev):
    from pylinac_amd import ops
    from pylinac_amd.field_analysis import _strip_edges

    specs = g["specs"]
    for key, tol in (("frames", dict(rtol=0, atol=0)), ("frames_f64", dict(rtol=1e-12, atol=1e-9))):
        frames = g[key]
        t = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
        cols, rows = ops.field_center_sums(t)
        from pylinac_amd.profile import single_profile_fwhm_batch

        vp, hp = single_profile_fwhm_batch(rows), single_profile_fwhm_batch(cols)
        h, w = frames.shape[1:]
        beam = torch.stack([hp.beam_center()["index (exact)"] / w, vp.beam_center()["index (exact)"] / h], 1).cpu().numpy()
        geo = torch.stack([hp.geometric_center()["index (exact)"] / w, vp.geometric_center()["index (exact)"] / h], 1).cpu().numpy()
        for i in range(len(frames)):
            assert np.allclose(beam[i], g[f"{key}.{i}.center_beam"], rtol=0, atol=1e-12), (key, i)
            assert np.allclose(geo[i], g[f"{key}.{i}.center_geo"], rtol=0, atol=1e-12), (key, i)
            for j, (pos, width) in enumerate(specs):
                p = torch.tensor([[pos, pos]], dtype=torch.float64)
                hv, vv, edges = ops.field_strips(t[i:i + 1], p, width, width)
                assert np.allclose(hv[0].cpu().numpy(), g[f"{key}.{i}.h{j}"], **tol), (key, i, j)
                assert np.allclose(vv[0].cpu().numpy(), g[f"{key}.{i}.v{j}"], **tol), (key, i, j)
                assert list(edges[0].cpu().numpy()) == [*_strip_edges(h, pos, width), *_strip_edges(w, pos, width)], (key, i, j)
    # frames with different centres: every frame's strips sit where horiz_values / vert_values put them for that frame alone
    frame = g["frames"][0]
    stack = np.stack([frame, np.roll(frame, (23, -31), axis=(0, 1)), np.roll(frame, (-17, 9), axis=(0, 1))])
    t = torch.from_numpy(stack).to(dev)
    from pylinac_amd import field_analysis as pfa

    cols, rows = ops.field_center_sums(t)
    vp, hp = single_profile_fwhm_batch(rows), single_profile_fwhm_batch(cols)
    pos = torch.stack([hp.beam_center()["index (exact)"] / stack.shape[2], vp.beam_center()["index (exact)"] / stack.shape[1]], 1)
    hv, vv, edges = ops.field_strips(t, pos, 0.03, 0.03)
    assert len({tuple(e) for e in edges.cpu().numpy().tolist()}) == 3
    for i in range(3):
        vpos, hpos = pfa.determine_center(t[i:i + 1])
        # (the batched FWHM search of the sums can land one ulp from the single-profile one; the strip bounds are the same)
        assert np.allclose((vpos, hpos), (float(pos[i, 0]), float(pos[i, 1])), rtol=0, atol=1e-12), i
        h1, _, _ = pfa.horiz_values(t[i:i + 1], hpos, 0.03)
        v1, _, _ = pfa.vert_values(t[i:i + 1], vpos, 0.03)
        assert torch.equal(hv[i], h1[0]) and torch.equal(vv[i], v1[0]), i


def check_dtypes(g, dev, kw=None):
    kw = kw or {"protocol": "VARIAN"}
    frame, dpi = g["frame"], float(g["dpi"])
    stack = np.stack([frame, np.fliplr(frame)])
    half = stack // 2                                # (the frame has 65535 hot pixels: halved, it fits int16 unchanged)
    ref = _batch(half, dev, dpi, kw)
    for arr in (half.astype(np.int16), half.astype(np.float64)):
        got = _batch(arr, dev, dpi, kw)
        for k in range(2):
            assert _same(got, ref, k, k), arr.dtype
        assert torch.equal(got.horiz, ref.horiz) and torch.equal(got.vert, ref.vert)
    scaled = stack.astype(np.float64) * 0.0173 - 7.25
    got = _batch(scaled, dev, dpi, kw)
    for k in range(2):
        _assert_frame(got, k, per_image(scaled[k], dpi, kw, dev), _tol(kw), ("scaled", k))
    with pytest.raises(TypeError):
        _batch(stack.astype(np.float32), dev, dpi, kw)


def check_inversion(g, dev):
    from pylinac_amd.image import ArrayImage

    frame, dpi = g["frame"], float(g["dpi"])
    stack = np.stack([frame, 65535 - frame, np.fliplr(frame), 65535 - np.fliplr(frame)]).astype(np.uint16)
    kw = {"protocol": "VARIAN"}
    want = [ArrayImage(a.copy()).check_inversion_by_histogram() for a in stack]
    assert want == [False, True, False, True]
    for invert in (False, True):
        res = _batch(stack, dev, dpi, kw, invert=invert)
        assert res.inverted.tolist() == want
        for k in range(len(stack)):
            _assert_frame(res, k, per_image(stack[k], dpi, kw, dev, invert=invert), _tol(kw), (invert, k))


def check_status(g, dev):
    frame, dpi = g["frame"], float(g["dpi"])
    const = np.full_like(frame, 1234)
    kw = {"protocol": "VARIAN"}
    good = _batch(np.stack([frame, np.fliplr(frame)]), dev, dpi, kw)
    mixed = _batch(np.stack([frame, const, np.fliplr(frame)]), dev, dpi, kw)
    assert mixed.status.tolist()[0] == 0 and mixed.status.tolist()[2] == 0 and mixed.status.tolist()[1] != 0
    assert all(np.isnan(v[1].numpy()).all() for v in mixed.results.values())
    assert all(np.isnan(v[1].numpy()).all() for v in mixed.protocol.values())
    with pytest.raises(Exception):
        per_image(const, dpi, kw, dev)
    assert _same(mixed, good, 0, 0) and _same(mixed, good, 2, 1)


def _pairwise(a):
    n = len(a)
    if n < 8:
        r = -0.0
        for v in a:
            r += v
        return r
    if n <= 128:
        r = list(a[:8])
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] += a[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for v in a[i:]:
            res += v
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(a[:n2]) + _pairwise(a[n2:])


def check_kernels(dev, sizes=((3, 37, 53), (2, 64, 300))):
    """the centre-sum and strip kernels against numpy; the window kernel against field_data / the protocol formulas"""
    from pylinac_amd import field_analysis as pfa
    from pylinac_amd import ops
    from pylinac_amd.profile import SingleProfile

    rng = np.random.default_rng(7)
    for n, h, w in sizes:
        for dt in (np.uint16, np.int16, np.float64):
            if dt == np.float64:
                a = rng.normal(100.0, 30.0, (n, h, w))
            else:
                info = np.iinfo(dt)
                a = rng.integers(info.min, info.max, (n, h, w), endpoint=True).astype(dt)
            t = torch.from_numpy(a).to(dev)
            cols, rows = ops.field_center_sums(t)
            exact = dt != np.float64
            want_c, want_r = a.sum(1, dtype=np.float64 if not exact else np.int64), a.sum(2, dtype=np.float64 if not exact else np.int64)
            assert np.array_equal(cols.cpu().numpy(), want_c.astype(np.float64)) if exact else np.array_equal(cols.cpu().numpy(), np.add.reduce(a, 1))
            assert np.array_equal(rows.cpu().numpy(), want_r.astype(np.float64)) if exact else np.allclose(rows.cpu().numpy(), want_r, rtol=1e-14, atol=0)
            # per-frame bounds: a centre strip, a zero-width strip, strips on both borders
            pos = np.resize(np.array([[0.5, 0.5], [0.0, 1.0], [1.0, 0.0]]), (n, 2))
            for width in (0.0, 0.1):
                hv, vv, edges = ops.field_strips(t, torch.from_numpy(pos), width, width)
                for i in range(n):
                    b, tp = pfa._strip_edges(h, pos[i, 1], width)
                    l, r = pfa._strip_edges(w, pos[i, 0], width)
                    assert edges[i].tolist() == [b, tp, l, r]
                    wh, wv = np.mean(a[i, b:tp, :], 0), np.mean(a[i, :, l:r], 1)
                    if exact:
                        assert np.array_equal(hv[i].cpu().numpy(), wh, equal_nan=True), (dt, i, width)
                        assert np.array_equal(vv[i].cpu().numpy(), wv, equal_nan=True), (dt, i, width)
                    else:
                        assert np.array_equal(hv[i].cpu().numpy(), wh, equal_nan=True)
                        assert np.allclose(vv[i].cpu().numpy(), wv, rtol=1e-14, atol=0, equal_nan=True), (dt, i, width)
    # the window kernel on processed profiles of odd and even field lengths, one with an exact symmetry tie
    x = np.arange(120, dtype=np.float64)
    base = 1 / (1 + np.exp(-(x - 30) / 2.5)) - 1 / (1 + np.exp(-(x - 90) / 2.5))
    profs = [base * 1000 + 5, np.roll(base, 3) * 800 + 10 + x * 0.3, base * 1000 + 5 + rng.normal(0, 2, x.size)]
    for raw in profs:
        sp = SingleProfile(raw, dpmm=1.0, interpolation="Linear", edge_detection_method="FWHM", normalization_method="Beam center")
        xi = torch.from_numpy(np.asarray(sp.x_indices, float)).to(dev)
        vals = torch.from_numpy(np.asarray(sp.values, float))[None].to(dev)
        half = sp.fwxm_data(50)
        for ifr in (0.8, 0.77, 1.0):
            fd = sp.field_data(in_field_ratio=ifr, slope_exclusion_ratio=0.2)
            stats, top = ops.field_windows(xi, vals, torch.tensor([half["center index (exact)"]], dtype=torch.float64),
                                           torch.tensor([half["width (exact)"]], dtype=torch.float64), ifr, 0.2, len(sp.x_indices))
            s = dict(zip(ops.FIELD_WINDOW_STATS, stats[0].cpu().numpy().tolist()))
            fv = fd["field values"]
            assert s["field_lo"] == fd["left index (exact)"] and s["field_hi"] == fd["right index (exact)"]
            assert s["field_width"] == fd["width (exact)"] and int(s["n_field"]) == len(fv)
            assert s["max"] == fv.max() and s["min"] == fv.min() and s["cax_value"] == fd["beam center value (@rounded)"]
            assert s["symmetry_point_difference"] == pfa.symmetry_point_difference(sp, ifr)
            assert s["symmetry_pdq_iec"] == pfa.symmetry_pdq_iec(sp, ifr)
            assert s["symmetry_area"] == pfa.symmetry_area(sp, ifr)
            nf = len(fv)
            assert _pairwise(list(fv[: nf // 2])) == np.sum(fv[: nf // 2])
            assert np.isclose(s["left_slope"], fd["left slope"], rtol=1e-9, atol=1e-12)
            assert np.isclose(s["right_slope"], fd["right slope"], rtol=1e-9, atol=1e-12)
            ts, tn = int(s["top_start"]), int(s["top_len"])
            xs, ys = sp._sample_points_in_physical_window(fd["left inner index (exact)"], fd["right inner index (exact)"])
            assert np.array_equal(np.asarray(sp.x_indices)[ts:ts + tn], xs) and np.array_equal(top[0, :tn].cpu().numpy(), ys)
    # an exact tie of |point difference| between two positions: a symmetric profile with a step on the left half
    sym = np.concatenate([np.full(20, 1.0), np.full(40, 100.0), np.full(40, 100.0), np.full(20, 1.0)])
    sym[30], sym[89] = 90.0, 110.0
    sym[40], sym[79] = 110.0, 90.0
    sp = SingleProfile(sym, dpmm=1.0, interpolation=None, edge_detection_method="FWHM", normalization_method="Beam center")
    half = sp.fwxm_data(50)
    xi = torch.from_numpy(np.asarray(sp.x_indices, float)).to(dev)
    stats, _ = ops.field_windows(xi, torch.from_numpy(np.asarray(sp.values, float))[None].to(dev),
                                 torch.tensor([half["center index (exact)"]], dtype=torch.float64), torch.tensor([half["width (exact)"]], dtype=torch.float64), 0.8, 0.2, 8)
    s = dict(zip(ops.FIELD_WINDOW_STATS, stats[0].cpu().numpy().tolist()))
    assert s["symmetry_point_difference"] == pfa.symmetry_point_difference(sp, 0.8)
    assert s["symmetry_pdq_iec"] == pfa.symmetry_pdq_iec(sp, 0.8)


# ---- on the CPU-emulated kernels ------------------------------------------------------------------------------------------------
def test_emulated_golden_cases(golden, emulated):
    check_golden_cases(golden("dropin_field"), emulated, cases=(0, 1, 3))


def test_emulated_centres_and_strips(golden, emulated):
    check_centres_and_strips(golden("field_strips"), emulated)


def test_emulated_dtypes(golden, emulated):
    check_dtypes(golden("dropin_field"), emulated)


def test_emulated_inversion(golden, emulated):
    check_inversion(golden("dropin_field"), emulated)


def test_emulated_status(golden, emulated):
    check_status(golden("dropin_field"), emulated)


def test_emulated_kernels(emulated):
    check_kernels(emulated)


# ---- on the device --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_golden_cases(golden, gpu):
    check_golden_cases(golden("dropin_field"), gpu)


@pytest.mark.gpu
def test_centres_and_strips(golden, gpu):
    check_centres_and_strips(golden("field_strips"), gpu)


@pytest.mark.gpu
def test_dtypes(golden, gpu):
    check_dtypes(golden("dropin_field"), gpu)
    check_dtypes(golden("dropin_field"), gpu, {"protocol": "SIEMENS", "edge_detection_method": "Inflection Hill", "is_FFF": True,
                                                "interpolation": "Spline", "normalization_method": "Max", "hill_window_ratio": 0.1})


@pytest.mark.gpu
def test_inversion(golden, gpu):
    check_inversion(golden("dropin_field"), gpu)


@pytest.mark.gpu
def test_status(golden, gpu):
    check_status(golden("dropin_field"), gpu)


@pytest.mark.gpu
def test_kernels(gpu):
    check_kernels(gpu, sizes=((3, 37, 53), (2, 64, 300), (2, 1024, 1024)))


@pytest.mark.gpu
def test_epid_stack_against_the_class_sequence(gpu):
    from pylinac_amd import synthetic

    frames = synthetic.epid_open_field_frames(64, device=gpu)
    dpi = 25.4 / 0.336
    host = frames.cpu().numpy()
    for kw in ({"protocol": "VARIAN"},
               {"protocol": "SIEMENS", "edge_detection_method": "Inflection Hill", "is_FFF": True, "hill_window_ratio": 0.1}):
        res = analyze_batch(frames, _dpmm(dpi), **kw)
        assert (res.status == 0).all(), kw
        for k in range(0, 64, 8):
            _assert_frame(res, k, per_image(host[k], dpi, kw, gpu), _tol(kw), (kw["protocol"], k))
