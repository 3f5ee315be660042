"""Flatness / symmetry protocol formulas over ``SingleProfile.field_data`` (pylinac/field_analysis.py:37-231).

Same names and arguments as the reference's module-level calculators; they reduce the in-field values (a few
hundred floats already on the host) to one number each.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from math import ceil, floor

import numpy as np
import torch


def flatness_dose_difference(profile, in_field_ratio: float = 0.8, **kwargs) -> float:
    """Varian flatness (field_analysis.py:37-57)."""
    ser = kwargs.get("slope_exclusion_ratio", 0.2)
    dmax = profile.field_calculation(in_field_ratio=in_field_ratio, calculation="max", slope_exclusion_ratio=ser)
    dmin = profile.field_calculation(in_field_ratio=in_field_ratio, calculation="min", slope_exclusion_ratio=ser)
    return 100 * abs(dmax - dmin) / (dmax + dmin)


def flatness_dose_ratio(profile, in_field_ratio: float = 0.8, **kwargs) -> float:
    """Elekta flatness (field_analysis.py:60-76)."""
    dmax = profile.field_calculation(in_field_ratio=in_field_ratio, calculation="max")
    dmin = profile.field_calculation(in_field_ratio=in_field_ratio, calculation="min")
    return 100 * (dmax / dmin)


def symmetry_point_difference(profile, in_field_ratio: float, **kwargs) -> float:
    """Varian symmetry (field_analysis.py:91-113)."""
    field = profile.field_data(in_field_ratio=in_field_ratio,
                               slope_exclusion_ratio=kwargs.get("slope_exclusion_ratio", 0.2))
    fv = field["field values"]
    cax_value = field["beam center value (@rounded)"]
    sym_vals = [100 * (lt - rt) / cax_value for lt, rt in zip(fv, fv[::-1])]
    return sym_vals[int(np.argmax(np.abs(sym_vals)))]


def symmetry_pdq_iec(profile, in_field_ratio: float, **kwargs) -> float:
    """Elekta PDQ IEC symmetry (field_analysis.py:191-214)."""
    fv = profile.field_data(in_field_ratio=in_field_ratio,
                            slope_exclusion_ratio=kwargs.get("slope_exclusion_ratio", 0.2))["field values"]

    def calc_sym(lt, rt) -> float:
        sym1, sym2 = lt / rt, rt / lt
        sign = np.sign(sym1) if abs(sym1) > abs(sym2) else np.sign(sym2)
        return max(abs(lt / rt), abs(rt / lt)) * sign

    sym_values = [calc_sym(lt, rt) for lt, rt in zip(fv, fv[::-1])]
    return sym_values[int(np.argmax(np.abs(sym_values)))]


def symmetry_area(profile, in_field_ratio: float, **kwargs) -> float:
    """Siemens area symmetry (field_analysis.py:217-231)."""
    fv = profile.field_data(in_field_ratio=in_field_ratio,
                            slope_exclusion_ratio=kwargs.get("slope_exclusion_ratio", 0.2))["field values"]
    n = len(fv)
    area_left = np.sum(fv[: floor(n / 2)])
    area_right = np.sum(fv[ceil(n / 2):])
    return 100 * (area_left - area_right) / (area_left + area_right)


# ---------------------------------------------------------------------------------------------------------------
# Strip profiles and centre search (pylinac/field_analysis.py:488-506, 1068-1117)
# ---------------------------------------------------------------------------------------------------------------
def _strip_edges(length: int, position: float, width: float) -> tuple:
    """The reference's rounding of a strip of relative `width` about relative `position` along an axis of `length`."""
    lo = max(int(round(length * position - length * width / 2)), 0)
    hi = min(int(round(length * position + length * width / 2) + 1), length)
    return lo, hi


def horiz_values(frames, horiz_position: float, horiz_width: float):
    """``FieldAnalysis._get_horiz_values`` (:1094-1117) for a device batch -> (float64 [N, W] profiles
    ``np.mean(array[bottom:top, :], 0)``, bottom_edge, top_edge)."""
    from . import ops

    x = ops._frames(frames)
    bottom, top = _strip_edges(x.shape[1], horiz_position, horiz_width)
    return ops.reduce_axis(x[:, bottom:top, :].contiguous(), 0, "mean"), bottom, top


def vert_values(frames, vert_position: float, vert_width: float):
    """``FieldAnalysis._get_vert_values`` (:1068-1092) -> (float64 [N, H] ``np.mean(array[:, left:right], 1)``, left, right)."""
    from . import ops

    x = ops._frames(frames)
    left, right = _strip_edges(x.shape[2], vert_position, vert_width)
    return ops.reduce_axis(x[:, :, left:right].contiguous(), 1, "mean"), left, right


def determine_center(frame, centering="Beam center") -> tuple:
    """``FieldAnalysis._determine_center`` (:488-506) for one frame -> (vert_ratio, horiz_ratio): the row / column sums
    (device reductions) through ``SingleProfile`` with its defaults."""
    from . import ops
    from .profile import Centering, SingleProfile, _enum

    x = ops._frames(frame)
    if x.shape[0] != 1:
        raise ValueError("determine_center takes one frame")
    vert_sum = ops.reduce_axis(x, 1, "sum")[0].cpu().numpy()
    horiz_sum = ops.reduce_axis(x, 0, "sum")[0].cpu().numpy()
    v_prof, h_prof = SingleProfile(vert_sum), SingleProfile(horiz_sum)
    if _enum(centering, Centering) == Centering.GEOMETRIC_CENTER:
        horiz_ratio = v_prof.geometric_center()["index (exact)"] / x.shape[1]
        vert_ratio = h_prof.geometric_center()["index (exact)"] / x.shape[2]
    else:
        horiz_ratio = v_prof.beam_center()["index (exact)"] / x.shape[1]
        vert_ratio = h_prof.beam_center()["index (exact)"] / x.shape[2]
    return vert_ratio, horiz_ratio


# ---------------------------------------------------------------------------------------------------------------
# FieldAnalysis over a stack of frames (pylinac/field_analysis.py:440-561, 720-862)
# ---------------------------------------------------------------------------------------------------------------
_PROTOCOLS = {"VARIAN": ("symmetry_point_difference", "dose_difference"), "ELEKTA": ("symmetry_pdq_iec", "dose_ratio"),
              "SIEMENS": ("symmetry_area", "dose_difference"), "NONE": None}
_HOST_SYMMETRY = {"symmetry_point_difference": symmetry_point_difference, "symmetry_pdq_iec": symmetry_pdq_iec,
                  "symmetry_area": symmetry_area}
_HOST_FLATNESS = {"dose_difference": flatness_dose_difference, "dose_ratio": flatness_dose_ratio}

# per-profile quantities, one row per profile (horizontal profiles 0 .. N-1, vertical N .. 2N-1)
_Q = ("pen_l", "pen_r", "grad_l", "grad_r", "gc", "bc", "full_lo", "full_hi", "full_w", "slope_l", "slope_r", "top", "max", "min",
      "symmetry_point_difference", "symmetry_pdq_iec", "symmetry_area", "n_field")

STATUS_OK, STATUS_NO_CENTER, STATUS_NO_EDGE, STATUS_HILL_FIT, STATUS_EMPTY_FIELD = 0, 1, 2, 3, 4


@dataclass
class FieldBatchResult:
    """:func:`analyze_batch`'s answer for N frames."""

    results: dict           # FieldAnalysis._results keys -> float64 [N] (``*_index_x_y``: [N, 2])
    protocol: dict          # FieldAnalysis._extra_results keys -> float64 [N] (empty for protocol "NONE")
    horiz: torch.Tensor     # float64 [N, S] horiz_profile.values
    vert: torch.Tensor      # float64 [N, S'] vert_profile.values
    inverted: torch.Tensor  # bool [N] check_inversion_by_histogram flipped the frame
    status: torch.Tensor    # int32 [N] 0 ok, else the STATUS_* code (results NaN)


def _protocol_name(protocol) -> str:
    name = getattr(protocol, "name", protocol)
    name = "NONE" if name is None else str(name).upper()
    if name not in _PROTOCOLS:
        raise ValueError(f"unknown protocol {protocol!r}; one of {sorted(_PROTOCOLS)}")
    return name


def _inversion_flags(x: torch.Tensor) -> np.ndarray:
    """``ArrayImage.check_inversion_by_histogram`` (image.py:899-926) per frame: |p50 - p5| > |p50 - p95| with numpy's
    percentiles; one host read of the [N, 3] order statistics."""
    from . import ops
    from ._lib import check

    if x.dtype in (torch.uint16, torch.int16):
        p = ops.percentile(x, [5, 50, 95]).numpy()
    else:                                                # exact float64 order statistics (pl_order_stats_f64), numpy's _lerp
        n = x.shape[0]
        flat = x.reshape(n, -1)
        _, lo, hi, frac = ops._percentile_plan(flat.shape[1], [5, 50, 95])
        ranks = torch.tensor(np.concatenate([lo, hi]), dtype=torch.int64, device=x.device)
        st = torch.empty((n, 6), dtype=torch.float64, device=x.device)
        from . import _lib
        check(_lib.load().pl_order_stats_f64(flat.data_ptr(), n, flat.shape[1], ranks.data_ptr(), 6, st.data_ptr(),
                                             ops._stream()), "pl_order_stats_f64")
        st = st.cpu().numpy()
        a, b = st[:, :3], st[:, 3:]
        d = b - a
        p = np.where((frac >= 0.5)[None, :], b - d * (1 - frac), a + d * frac)
    return np.abs(p[:, 1] - p[:, 0]) > np.abs(p[:, 1] - p[:, 2])


def _edge_batch(values, edge, dpmm, interpolation, ground, interpolation_resolution_mm, normalization_method,
                edge_smoothing_ratio, hill_window_ratio):
    from .profile import (Edge, single_profile_fwhm_batch, single_profile_hill_batch,
                          single_profile_inflection_batch)

    kw = dict(dpmm=dpmm, interpolation=interpolation, ground=ground, interpolation_resolution_mm=interpolation_resolution_mm,
              normalization_method=normalization_method)
    if edge == Edge.FWHM:
        return single_profile_fwhm_batch(values, **kw)
    if edge == Edge.INFLECTION_DERIVATIVE:
        return single_profile_inflection_batch(values, edge_smoothing_ratio=edge_smoothing_ratio, **kw)
    return single_profile_hill_batch(values, edge_smoothing_ratio=edge_smoothing_ratio, hill_window_ratio=hill_window_ratio, **kw)


def _profile_quantities(b, edge, lower: int, upper: int, in_field_ratio: float, slope_exclusion_ratio: float):
    """The per-profile part of FieldAnalysis._results on the device -> (float64 [N, len(_Q)], top windows [N, tcap], edge
    status int32 [N]: 0 ok, STATUS_NO_EDGE, or STATUS_HILL_FIT for a Hill row the host must redo)."""
    from . import ops
    from .profile import Edge

    nan = float("nan")
    if edge == Edge.FWHM:
        half = b.fwxm_data(50)
        bc, span = half["center index (exact)"], half["width (exact)"]
        st = torch.where(half["peaks"] > 0, 0, STATUS_NO_EDGE).to(torch.int32)
    elif edge == Edge.INFLECTION_DERIVATIVE:
        left, right = b.edges[:, 0], b.edges[:, 1]
        bc, span = left + (right - left) / 2, right - left
        st = torch.where(b.status == 0, 0, STATUS_NO_EDGE).to(torch.int32)
    else:
        left, right = b.index[:, 0], b.index[:, 1]
        bc, span = left + (right - left) / 2, right - left
        st = torch.where(b.settled.all(dim=1), 0, STATUS_HILL_FIT).to(torch.int32)
    pen = b.penumbra(lower, upper)
    grad = ((pen["left gradient (exact) %/mm"], pen["right gradient (exact) %/mm"]) if edge == Edge.INFLECTION_HILL
            else (torch.full_like(bc, nan), torch.full_like(bc, nan)))
    gc = b.geometric_center()["index (exact)"]
    xi = torch.from_numpy(np.ascontiguousarray(b.x_indices)).to(b.values.device)
    s = b.values.shape[1]
    full, _ = ops.field_windows(xi, b.values, bc, span, 1.0, slope_exclusion_ratio, 1)
    # the "top" window holds slope_exclusion_ratio * in_field_ratio of a field no wider than the profile, plus the nearest-sample
    # tiers' spill; a row that needs more (edges outside the profile) is completed on the host
    per_unit = (s - 1) / max(float(b.x_indices[-1] - b.x_indices[0]), 1e-300)
    tcap = int(min(s, math.ceil(slope_exclusion_ratio * in_field_ratio * (b.x_indices[-1] - b.x_indices[0] + 1) * per_unit) + 8))
    part, top = ops.field_windows(xi, b.values, bc, span, in_field_ratio, slope_exclusion_ratio, tcap)
    k = {name: i for i, name in enumerate(ops.FIELD_WINDOW_STATS)}
    cols = [pen["left penumbra width (exact) mm"], pen["right penumbra width (exact) mm"], grad[0], grad[1], gc, bc,
            full[:, k["field_lo"]], full[:, k["field_hi"]], full[:, k["field_width"]], part[:, k["left_slope"]],
            part[:, k["right_slope"]], torch.full_like(bc, nan), part[:, k["max"]], part[:, k["min"]],
            part[:, k["symmetry_point_difference"]], part[:, k["symmetry_pdq_iec"]], part[:, k["symmetry_area"]],
            part[:, k["n_field"]], part[:, k["top_start"]], part[:, k["top_len"]]]
    return torch.stack(cols, dim=1), top, st


def _host_quantities(sp, lower, upper, in_field_ratio, slope_exclusion_ratio) -> np.ndarray:
    """The same row from the per-image class (``SingleProfile``), for Hill rows whose device fit did not settle: the batch's
    answer is then the class's answer."""
    pen = sp.penumbra(lower, upper)
    full = sp.field_data(in_field_ratio=1.0, slope_exclusion_ratio=slope_exclusion_ratio)
    fd = sp.field_data(in_field_ratio=in_field_ratio, slope_exclusion_ratio=slope_exclusion_ratio)
    fv = fd["field values"]
    kw = dict(slope_exclusion_ratio=slope_exclusion_ratio)
    row = [pen["left penumbra width (exact) mm"], pen["right penumbra width (exact) mm"],
           pen.get("left gradient (exact) %/mm", np.nan), pen.get("right gradient (exact) %/mm", np.nan),
           sp.geometric_center()["index (exact)"], sp.beam_center()["index (exact)"], full["left index (exact)"],
           full["right index (exact)"], full["width (exact)"], fd["left slope"], fd["right slope"], fd['"top" index (exact)'],
           fv.max() if len(fv) else np.nan, fv.min() if len(fv) else np.nan]
    row += [_HOST_SYMMETRY[name](sp, in_field_ratio, **kw) if len(fv) else np.nan for name in _Q[14:17]]
    row += [len(fv)]
    return np.asarray(row, dtype=np.float64)


def analyze_batch(frames, dpmm: float, protocol="VARIAN", centering="Beam center", vert_position: float = 0.5,
                  horiz_position: float = 0.5, vert_width: float = 0, horiz_width: float = 0, in_field_ratio: float = 0.8,
                  slope_exclusion_ratio: float = 0.2, invert: bool = False, is_FFF: bool = False, penumbra=(20, 80),
                  interpolation="Linear", interpolation_resolution_mm: float = 0.1, ground: bool = True,
                  normalization_method="Beam center", edge_detection_method="Inflection Derivative",
                  edge_smoothing_ratio: float = 0.003, hill_window_ratio: float = 0.15) -> FieldBatchResult:
    """``FieldAnalysis(frame)`` + ``analyze(...)`` (pylinac/field_analysis.py:440-561, 720-862) for every frame of a resident
    stack ``frames`` [N, H, W] (uint16, int16 or float64), with the arguments, defaults and spellings of the per-image class.

    Device pass, per stack: the inversion check (one host read of the [N, 3] percentiles; flagged frames are inverted on the
    device, then all of them again for ``invert=True``), the row / column sums in one read of each 16-bit frame
    (``pl_field_center_sums``), the centre search through ``single_profile_fwhm_batch``, the two strips at each frame's own
    centre (``pl_field_strips``), the profiles and their edges through the ``single_profile_*_batch`` constructors, and
    ``field_data``'s windows with the flatness / symmetry / slope reductions (``pl_field_windows``).  One device-to-host copy
    then brings the per-profile numbers and the "top" windows, whose quadratic fit and bounded maximum stay the reference's
    host routine (``np.polyfit`` + L-BFGS-B), one profile at a time.  ``is_FFF`` changes none of these numbers (the per-image
    sequence computes the "top" for every field).

    ``status`` per frame (every result NaN where it is not 0; a frame never changes another frame's numbers):
      0  ok
      1  no field in the row / column sums: the centre search finds no half-maximum peak (the class raises IndexError)
      2  a strip profile has no field edge: no FWHM peak, no derivative peak or valley, or more extrema than the search holds
      3  Inflection Hill: a penumbra fit failed on the device and on the host's ``curve_fit`` too (RuntimeError / TypeError)
      4  the in-field window holds no sample: the protocol's max / argmax of an empty array raises ValueError
    """
    from . import ops
    from .profile import Centering, Edge, Interpolation, Normalization, SingleProfile, _bounded_top, _enum

    if not 0 <= in_field_ratio <= 1.0 or not 0 <= slope_exclusion_ratio <= 1.0:
        raise ValueError("in_field_ratio and slope_exclusion_ratio must be within (0, 1)")
    if slope_exclusion_ratio >= in_field_ratio:
        raise ValueError("The exclusion region must be smaller than the field ratio")
    lower, upper = penumbra
    if lower > upper:
        raise ValueError("Upper penumbra value must be larger than the lower penumbra value")
    proto = _protocol_name(protocol)
    centering = _enum(centering, Centering)
    edge = _enum(edge_detection_method, Edge)
    interpolation = _enum(interpolation, Interpolation)
    normalization_method = _enum(normalization_method, Normalization)
    if not isinstance(frames, torch.Tensor):
        raise TypeError("frames must be a device tensor [N, H, W]")
    if frames.dtype not in (torch.uint16, torch.int16, torch.float64):
        raise TypeError(f"analyze_batch takes uint16, int16 or float64 frames; got {frames.dtype}")
    x = ops._frames(frames)
    n, h, w = x.shape
    dev = x.device

    # 1. inversion (FieldAnalysis.__init__ :470, analyze :751)
    flags = _inversion_flags(x)
    if flags.any():                                      # (copy_ per flagged frame: 16-bit tensors have no index_put)
        x = x.clone()
        for i in np.nonzero(flags)[0].tolist():
            x[i].copy_(ops.invert(x[i:i + 1])[0])
    if invert:
        x = ops.invert(x)

    status = torch.zeros(n, dtype=torch.int32, device=dev)
    # 2-3. centre (_determine_center :488-506): SingleProfile(np.sum(image, axis)) with its defaults
    if centering == Centering.MANUAL:
        pos = torch.tensor([[float(vert_position), float(horiz_position)]], dtype=torch.float64, device=dev).expand(n, 2)
    else:
        from .profile import single_profile_fwhm_batch

        cols, rows = ops.field_center_sums(x)
        v_prof, h_prof = single_profile_fwhm_batch(rows), single_profile_fwhm_batch(cols)
        v_half, h_half = v_prof.fwxm_data(50), h_prof.fwxm_data(50)
        if centering == Centering.GEOMETRIC_CENTER:
            horiz_ratio = v_prof.geometric_center()["index (exact)"] / h
            vert_ratio = h_prof.geometric_center()["index (exact)"] / w
        else:
            horiz_ratio = v_half["center index (exact)"] / h
            vert_ratio = h_half["center index (exact)"] / w
        found = (v_half["peaks"] > 0) & (h_half["peaks"] > 0)
        status = torch.where(found, status, torch.full_like(status, STATUS_NO_CENTER))
        nan = torch.full_like(horiz_ratio, float("nan"))
        pos = torch.stack([torch.where(found, vert_ratio, nan), torch.where(found, horiz_ratio, nan)], dim=1)

    # 4. strips (_get_horiz_values / _get_vert_values :1068-1117) at every frame's own centre
    horiz, vert, _ = ops.field_strips(x, pos.contiguous(), vert_width, horiz_width)

    # 5-6. profiles, edges, field_data windows and the protocol reductions
    args = (edge, dpmm, interpolation, ground, interpolation_resolution_mm, normalization_method, edge_smoothing_ratio,
            hill_window_ratio)
    hb, vb = _edge_batch(horiz, *args), _edge_batch(vert, *args)
    hq, htop, hst = _profile_quantities(hb, edge, lower, upper, in_field_ratio, slope_exclusion_ratio)
    vq, vtop, vst = _profile_quantities(vb, edge, lower, upper, in_field_ratio, slope_exclusion_ratio)

    # 7. one device-to-host copy
    sizes = [t.numel() for t in (hq, vq, htop, vtop, hst, vst, status)]
    packed = torch.cat([hq.reshape(-1), vq.reshape(-1), htop.reshape(-1), vtop.reshape(-1), hst.to(torch.float64),
                        vst.to(torch.float64), status.to(torch.float64)])
    host = ops.HostCopy(packed).numpy()
    parts = np.split(host, np.cumsum(sizes)[:-1])
    q = {"h": parts[0].reshape(n, -1).copy(), "v": parts[1].reshape(n, -1).copy()}
    tops = {"h": parts[2].reshape(n, -1), "v": parts[3].reshape(n, -1)}
    edge_st = {"h": parts[4].astype(np.int32), "v": parts[5].astype(np.int32)}
    st = parts[6].astype(np.int32)

    nq = len(_Q)
    for side, b, strips in (("h", hb, horiz), ("v", vb, vert)):
        qs, xi = q[side], np.asarray(b.x_indices, dtype=np.float64)
        for i in range(n):
            if st[i] != 0:
                continue
            if edge_st[side][i] == STATUS_NO_EDGE:
                st[i] = STATUS_NO_EDGE
                continue
            if edge_st[side][i] == STATUS_HILL_FIT:          # the reference's curve_fit, one profile at a time
                try:
                    sp = SingleProfile(strips[i].cpu().numpy(), dpmm=dpmm, interpolation=interpolation, ground=ground,
                                       interpolation_resolution_mm=interpolation_resolution_mm,
                                       normalization_method=normalization_method, edge_detection_method=edge,
                                       edge_smoothing_ratio=edge_smoothing_ratio, hill_window_ratio=hill_window_ratio)
                    qs[i, :nq] = _host_quantities(sp, lower, upper, in_field_ratio, slope_exclusion_ratio)
                except IndexError:
                    st[i] = STATUS_NO_EDGE
                except (RuntimeError, TypeError, ValueError):
                    st[i] = STATUS_HILL_FIT
                continue
            if proto != "NONE" and qs[i, _Q.index("n_field")] < 1:
                st[i] = STATUS_EMPTY_FIELD
                continue
            start, length = int(qs[i, nq]), int(qs[i, nq + 1])
            top_x = xi[start:start + length]
            if length <= tops[side].shape[1]:
                top_y = tops[side][i, :length]
            else:                                          # a window wider than the profile's field: y from the host copy
                from .profile import _Linear1d

                top_y = _Linear1d(xi, b.values[i].cpu().numpy(), extrapolate=True)(top_x)
            parabola = np.polyfit(top_x, top_y, deg=2)
            qs[i, _Q.index("top")] = _bounded_top(parabola, top_x[0] + abs(top_x[-1] - top_x[0]) / 2, top_x[0], top_x[-1])[0]

    H, V = ({name: q[s][:, j] for j, name in enumerate(_Q)} for s in ("h", "v"))
    d = dpmm
    res = {"top_penumbra_mm": V["pen_l"], "bottom_penumbra_mm": V["pen_r"], "left_penumbra_mm": H["pen_l"],
           "right_penumbra_mm": H["pen_r"]}
    if edge == Edge.INFLECTION_HILL:
        res.update(top_penumbra_percent_mm=np.abs(V["grad_l"]), bottom_penumbra_percent_mm=np.abs(V["grad_r"]),
                   left_penumbra_percent_mm=np.abs(H["grad_l"]), right_penumbra_percent_mm=np.abs(H["grad_r"]))
    res["geometric_center_index_x_y"] = np.stack([H["gc"], V["gc"]], axis=1)
    res["beam_center_index_x_y"] = np.stack([H["bc"], V["bc"]], axis=1)
    res.update(field_size_vertical_mm=V["full_w"] / d, field_size_horizontal_mm=H["full_w"] / d,
               beam_center_to_top_mm=np.abs(V["bc"] - V["full_lo"]) / d, beam_center_to_bottom_mm=np.abs(V["full_hi"] - V["bc"]) / d,
               beam_center_to_left_mm=np.abs(H["bc"] - H["full_lo"]) / d, beam_center_to_right_mm=np.abs(H["full_hi"] - H["bc"]) / d,
               cax_to_top_mm=np.abs(V["gc"] - V["full_lo"]) / d, cax_to_bottom_mm=np.abs(V["gc"] - V["full_hi"]) / d,
               cax_to_left_mm=np.abs(H["gc"] - H["full_lo"]) / d, cax_to_right_mm=np.abs(H["gc"] - H["full_hi"]) / d)
    res.update(top_position_index_x_y=np.stack([H["top"], V["top"]], axis=1),
               top_horizontal_distance_from_cax_mm=np.abs(H["top"] - H["gc"]) / d,
               top_vertical_distance_from_cax_mm=np.abs(V["top"] - V["gc"]) / d,
               top_horizontal_distance_from_beam_center_mm=(H["top"] - H["bc"]) / d,
               top_vertical_distance_from_beam_center_mm=(V["top"] - V["bc"]) / d,
               left_slope_percent_mm=H["slope_l"] * d * 100, right_slope_percent_mm=H["slope_r"] * d * 100,
               top_slope_percent_mm=V["slope_l"] * d * 100, bottom_slope_percent_mm=V["slope_r"] * d * 100)
    extra = {}
    if _PROTOCOLS[proto] is not None:
        sym, flat = _PROTOCOLS[proto]
        for tag, P in (("horizontal", H), ("vertical", V)):
            extra[f"symmetry_{tag}"] = P[sym]
            mx, mn = P["max"], P["min"]
            extra[f"flatness_{tag}"] = 100 * np.abs(mx - mn) / (mx + mn) if flat == "dose_difference" else 100 * (mx / mn)
    bad = st != 0
    to_t = lambda a: torch.from_numpy(np.where(bad if a.ndim == 1 else bad[:, None], np.nan, a).astype(np.float64))
    return FieldBatchResult(results={k: to_t(v) for k, v in res.items()}, protocol={k: to_t(v) for k, v in extra.items()},
                            horiz=hb.values, vert=vb.values, inverted=torch.from_numpy(flags.copy()),
                            status=torch.from_numpy(st.copy()))
