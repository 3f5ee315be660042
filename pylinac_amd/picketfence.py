"""Batched picket-fence measurement (BASELINE config #3).

Mirrors the per-image part of ``PicketFence.analyze`` for UP_DOWN pickets
(pylinac/picketfence.py:745-803): leaf profile -> FWXM picket positions -> picket spacing -> for every
leaf pair in view and every picket the MLC window, the ``_is_mlc_peak_in_window`` test and the FWXM
centre of the window's median profile.  The input batch is uint16 ``[N,H,W]`` frames AFTER the
constructor's crop (picketfence.py:214-215); ground()/normalize() (:322-323) are folded into the
kernels as the float64 quotient ``(a - min) / (max - min)``.  int16 frames and float64 frames holding
integers go through an exact uint16 bridge; float64 frames with fractional values (a rescaled DICOM
series) are measured on their own float64 kernels with ``measure_fractional=True``.

``evaluate_batch`` takes the returned ``[N, leaves, P]`` positions to the numbers a picket-fence user reads -- the line
fitted through every picket (``Picket.get_fit`` :1881-1899), every leaf's distance from its picket's line in mm
(``MLCValue.error``), ``max_error`` with its leaf and picket, ``abs_median_error``, ``percent_passing``, ``passed`` -- in one
launch, one workgroup per frame.  Dropping leaf rows without the modal number of kisses (:810-824) is not built: every
measured window takes part.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, ops
from ._lib import check

MLC_ARRANGEMENTS = {  # pylinac/picketfence.py:103-135
    "MILLENNIUM": [(10, 10), (40, 5), (10, 10)],
    "HD_MILLENNIUM": [(14, 5), (32, 2.5), (14, 5)],
    "BMOD": [(40, 4)],
    "AGILITY": [(80, 5)],
    "MLCI": [(40, 10)],
    "HALCYON_DISTAL": [(28, 10)],
    "HALCYON_PROXIMAL": [(29, 10)],
}


def mlc_arrangement(leaf_arrangement, offset: float = 0):
    """``MLCArrangement`` (picketfence.py:67-100) -> (leaf numbers, centers mm, widths mm)."""
    centers, widths = [], []
    rolling_edge = 0
    for leaf_num, width in leaf_arrangement:
        centers += np.arange(start=rolling_edge + width / 2, stop=leaf_num * width + rolling_edge + width / 2,
                             step=width).tolist()
        rolling_edge = centers[-1] + width / 2
        widths += [width] * leaf_num
    mean = np.mean(centers)
    centers = [c - mean + offset for c in centers]
    leaves = np.arange(1, len(centers) + 1, dtype=int)[::-1].tolist()
    return leaves, centers, widths


def leaves_in_view(shape, dpmm, leaves, centers, widths, analysis_width=0.4, orientation: str = "UP_DOWN"):
    """``PicketFence._leaves_in_view`` (picketfence.py:888-912): the leaves run across the rows (UP_DOWN pickets) or across the
    columns (LEFT_RIGHT)."""
    pixel_range = (shape[0] if orientation == "UP_DOWN" else shape[1]) / 2
    pixel_range -= max(widths[0] * analysis_width, widths[-1] * analysis_width) * dpmm
    return [(n, c, w) for n, c, w in zip(leaves, centers, widths) if abs(c) < pixel_range / dpmm]


def pairwise_plan(n: int):
    """numpy's pairwise summation tree for a contiguous run of ``n`` float64 values (numpy/_core/src/umath/loops_utils.h.src:
    more than 128 values are halved, the first half rounded down to a multiple of 8) -> (leaf starts, leaf lengths, postfix
    program: k >= 0 = leaf k's sum, -1 = add the two sums on top).  Feeds ``pl_scaled_rowmean``."""
    starts, lens, prog = [], [], []

    def rec(s, m):
        if m <= 128:
            prog.append(len(starts))
            starts.append(s)
            lens.append(m)
            return
        n2 = m // 2
        n2 -= n2 % 8
        rec(s, n2)
        rec(s + n2, m - n2)
        prog.append(-1)

    rec(0, int(n))
    return np.asarray(starts, np.int32), np.asarray(lens, np.int32), np.asarray(prog, np.int32)


@dataclass
class PFBatchResult:
    leaf_nums: list            # leaf numbers in view, row order of `position`
    picket_idx: torch.Tensor   # int32 [N, cap]   FWXM picket centres (pixel index)
    picket_count: torch.Tensor # int32 [N]
    spacing: torch.Tensor      # float64 [N]      picket spacing in pixels
    position: torch.Tensor     # float64 [N, leaves, cap] MLC positions in pixels (NaN = no measurement): the leaf-pair centre
    status: torch.Tensor       # int32 [N, leaves, cap]   0 ok, 1 no picket, 2 rejected window, 3 unsupported
    left: torch.Tensor | None = None    # separate_leaves: float64 [N, leaves, cap] positions of the two banks' leaf ends
    right: torch.Tensor | None = None   # (MLCValue.get_peak_positions' (left, right), picketfence.py:1616-1623)


_PLAN_CACHE: dict = {}


def analyze_batch(frames: torch.Tensor, dpmm: float, mlc: str = "MILLENNIUM", num_pickets: int | None = None,
                  leaf_analysis_width_ratio: float = 0.4, height_threshold: float = 0.5,
                  edge_threshold: float = 1.5, peak_sort: str = "peak_heights",
                  required_prominence: float = 0.2, fwxm: int = 50, cap: int | None = None,
                  orientation: str = "UP_DOWN", separate_leaves: bool = False, exact_deviation: bool = False,
                  measure_fractional: bool = False) -> PFBatchResult:
    """The per-image measurement of ``PicketFence.analyze`` (picketfence.py:745-803, 1605-1628) for a resident batch, in five
    launches: min / max (ground + normalize folded into every later read), leaf profile, picket peaks, picket table, and ONE
    kernel for all leaf x picket windows (window test, median profile, FWXM search, position).  ``orientation``: "UP_DOWN"
    (pickets run up-down: the leaf profile is ``np.mean(image, 0)``) or "LEFT_RIGHT" (``np.mean(image, 1)``, windows
    transposed).  ``separate_leaves``: also return both leaf-end positions per window.  ``cap`` = picket slots per frame
    (default ``num_pickets`` when given, else 16).  ``exact_deviation=True`` makes every window evaluate numpy's float64
    ``np.std`` sequence for the edge test instead of deciding it from exact integer row moments where the margin allows
    (identical results; a test knob).

    Input: uint16, int16 (range up to 32767) or float64 frames.  By default a float64 frame must hold integers (status 3 in
    every window of a frame that does not).  ``measure_fractional=True`` measures float64 batches whole on float64 kernels
    instead -- fractional values (``dicom.load_frames`` with a non-integer RescaleSlope) included, integer-valued frames with
    the same bits as the default; a frame holding a NaN or an infinity gets status 3 in every window.  Windows taller than 64
    rows (the leaf width in pixels) or wider than 128 columns (the picket spacing) get status 3; LEFT_RIGHT float64 frames
    may be at most 4096 columns wide."""
    x = ops._frames(frames)
    unfit = None
    f64 = bool(measure_fractional) and x.dtype == torch.float64     # q = (a - min) / (max - min) by true division
    if x.dtype in (torch.int16, torch.float64) and not f64:
        # what the reference's loader may hand over instead of uint16: a signed panel's int16, or float64 holding integers
        # (``dtype=float``; rescale tags with an integer slope and intercept).  ground() / normalize() (picketfence.py:322-323)
        # only see a - min, which pl_to_u16_exact forms exactly; frames it cannot represent -- non-integer float64 values,
        # an int16 range beyond 32767 where the reference's own ground() wraps -- come back with status 3 in every window
        x, unfit = ops.to_u16_exact(x)
    elif x.dtype != torch.uint16 and not f64:
        raise TypeError("analyze_batch takes uint16 frames, int16 frames, or float64 frames (holding integers unless "
                        "measure_fractional=True)")
    if orientation not in ("UP_DOWN", "LEFT_RIGHT"):
        raise ValueError("orientation must be 'UP_DOWN' or 'LEFT_RIGHT'")
    lr = orientation == "LEFT_RIGHT"
    if cap is None:
        cap = int(num_pickets) if num_pickets else 16
    n, h, w = x.shape
    dev = x.device
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    # ground()/normalize(): q = (a - min) / (max - min)
    vmin, vmax = ops.minmax(x)
    gmax = vmax - vmin
    travel = h if lr else w                               # length of the leaf profile = the pickets' travel axis
    leaf_prof = torch.empty((n, travel), dtype=torch.float64, device=dev)
    if lr:
        key = (w, str(dev))
        if key not in _PLAN_CACHE:
            _PLAN_CACHE[key] = tuple(torch.from_numpy(a).to(dev) for a in pairwise_plan(w))
        ls, ll, pg = _PLAN_CACHE[key]
        rowmean = lib.pl_scaled_rowmean_f64 if f64 else lib.pl_scaled_rowmean
        check(rowmean(x.data_ptr(), n, h, w, vmin.data_ptr(), gmax.data_ptr(), ls.data_ptr(), ll.data_ptr(),
                      ls.numel(), pg.data_ptr(), pg.numel(), leaf_prof.data_ptr(), st), "pl_scaled_rowmean")
    else:
        colmean = lib.pl_scaled_colmean_f64 if f64 else lib.pl_scaled_colmean
        check(colmean(x.data_ptr(), n, h, w, vmin.data_ptr(), gmax.data_ptr(), leaf_prof.data_ptr(), st), "pl_scaled_colmean")
    if f64:
        # a NaN or an infinity in a frame: an infinite minimum or maximum makes max - min non-finite, and every pixel is in one
        # leaf-profile sum, so a NaN pixel leaves a NaN there (a constant frame's 0 / 0 profile is the uint16 path's too)
        unfit = ~torch.isfinite(gmax) | (torch.isnan(leaf_prof).any(1) & (gmax > 0))
    leaf_prof = ops.normalize(leaf_prof.unsqueeze(1)).squeeze(1).contiguous()      # MultiProfile.normalize()
    peaks = ops.find_peaks_batch(leaf_prof, cap=cap, threshold=height_threshold, peak_separation=0.02,
                                 max_number=num_pickets, peak_sort=peak_sort,
                                 required_prominence=required_prominence)
    pk_idx = torch.empty((n, cap), dtype=torch.int32, device=dev)
    pk_val = torch.empty((n, cap), dtype=torch.float64, device=dev)
    spacing = torch.empty(n, dtype=torch.float64, device=dev)
    check(lib.pl_pf_pickets(peaks.count.data_ptr(), peaks.props.data_ptr(), cap, leaf_prof.data_ptr(), travel, n,
                            pk_idx.data_ptr(), pk_val.data_ptr(), spacing.data_ptr(), st), "pl_pf_pickets")
    # leaf geometry is image-independent: _get_mlc_window (picketfence.py:859-886): rows for UP_DOWN, columns for LEFT_RIGHT
    leaves, centers, widths = mlc_arrangement(MLC_ARRANGEMENTS[mlc])
    view = leaves_in_view((h, w), dpmm, leaves, centers, widths, leaf_analysis_width_ratio, orientation)
    across = w if lr else h                               # the axis the leaves are stacked along
    los, his = [], []
    for _, center, width in view:
        leaf_width_px = width * dpmm
        leaf_center_px = center * dpmm + across / 2
        los.append(max(int(leaf_center_px - leaf_width_px / 2), 0))
        his.append(min(int(leaf_center_px + leaf_width_px / 2), across))
    nl = len(view)
    if nl == 0:
        raise ValueError("no leaves in view")
    key = (tuple(los), tuple(his), str(dev))
    if key not in _PLAN_CACHE:
        _PLAN_CACHE[key] = (torch.tensor(los, dtype=torch.int32, device=dev), torch.tensor(his, dtype=torch.int32, device=dev))
    d_lo, d_hi = _PLAN_CACHE[key]
    m = n * nl * cap
    # the widest leaf in pixels: the kernel's LDS per wave follows it.  64 is the limit (status 3 beyond): 10 mm leaves (the
    # widest of every supported bank) on the finest supported panel at isocentre scale (aS1200, 0.336 mm at SID 1500) are 45,
    # on a 150 dpi film scan 59; up to 48 rows the kernel runs in its EPID configuration
    max_rows = min(max([b - t for t, b in zip(los, his)] + [1]), 64)
    fw = ops.make_peak_params(128, fwxm_height=fwxm / 100, max_number=1)                 # FWXMProfile.field_edge_idx
    rec = torch.empty((m, 3), dtype=torch.float64, device=dev)
    status = torch.empty(m, dtype=torch.int32, device=dev)
    import ctypes as C
    if f64:
        check(lib.pl_pf_measure_f64(x.data_ptr(), n, h, w, 1 if lr else 0, vmin.data_ptr(), gmax.data_ptr(),
                                    peaks.count.data_ptr(), pk_idx.data_ptr(), pk_val.data_ptr(), cap, spacing.data_ptr(),
                                    d_lo.data_ptr(), d_hi.data_ptr(), nl, max_rows, float(height_threshold),
                                    float(edge_threshold), C.byref(fw), rec.data_ptr(), status.data_ptr(), 0, 0, st),
              "pl_pf_measure_f64")
    else:
        check(lib.pl_pf_measure(x.data_ptr(), n, h, w, 1 if lr else 0, vmin.data_ptr(), gmax.data_ptr(), peaks.count.data_ptr(),
                                pk_idx.data_ptr(), pk_val.data_ptr(), cap, spacing.data_ptr(), d_lo.data_ptr(), d_hi.data_ptr(),
                                nl, max_rows, float(height_threshold), float(edge_threshold), 1 if exact_deviation else 0,
                                C.byref(fw), rec.data_ptr(), status.data_ptr(), 0, 0, st), "pl_pf_measure")
    rec = rec.view(n, nl, cap, 3)
    if unfit is not None:                                   # (device-side selects: no synchronisation)
        bad = (unfit != 0).view(n, 1, 1)
        status = torch.where(bad.expand(n, nl, cap).reshape(-1), torch.full_like(status, 3), status)
        rec = torch.where(bad.unsqueeze(-1), torch.full_like(rec, float("nan")), rec)
    return PFBatchResult([v[0] for v in view], pk_idx, peaks.count, spacing, rec[..., 0], status.view(n, nl, cap),
                         rec[..., 1] if separate_leaves else None, rec[..., 2] if separate_leaves else None)


PF_SUMMARY_FIELDS = ("n_measured", "max_error", "max_error_leaf", "max_error_picket", "abs_median_error", "percent_passing",
                     "passed", "percent_under_action")


@dataclass
class PFErrorsBatch:
    fit: torch.Tensor            # float64 [N, cap, 2]       slope, intercept of every picket's line (np.polyfit order), px
    picket_status: torch.Tensor  # int32 [N, cap]            0 ok, 1 slot beyond picket_count, 2 no line (< 2 leaves, Sxx == 0)
    error: torch.Tensor          # float64 [N, leaves, cap]  position - line at the leaf centre, mm (NaN = none)
    passed_window: torch.Tensor  # uint8 [N, leaves, cap]    |error| < tolerance
    summary: torch.Tensor        # float64 [N, 8]            PF_SUMMARY_FIELDS
    PF_SUMMARY_FIELDS = PF_SUMMARY_FIELDS


def leaf_markers(shape, dpmm: float, mlc="MILLENNIUM", orientation: str = "UP_DOWN", leaf_analysis_width_ratio: float = 0.4):
    """The leaves in view of a frame of ``shape`` with ``analyze_batch``'s arithmetic (``_leaves_in_view``, ``_get_mlc_window``)
    -> (leaf numbers, leaf_center_px, leaf_up_px): the centre ``across / 2 + center * dpmm`` and the upper marker coordinate
    ``leaf_center_px - leaf_width_px / 2 * leaf_analysis_width_ratio`` along the axis the leaves are stacked on.  ``mlc``: a
    bank's name, or a leaf arrangement ``[(number of leaves, width mm), ...]`` as the reference's ``MLCArrangement`` takes."""
    if orientation not in ("UP_DOWN", "LEFT_RIGHT"):
        raise ValueError("orientation must be 'UP_DOWN' or 'LEFT_RIGHT'")
    leaves, centers, widths = mlc_arrangement(MLC_ARRANGEMENTS[mlc] if isinstance(mlc, str) else list(mlc))
    view = leaves_in_view(tuple(shape), dpmm, leaves, centers, widths, leaf_analysis_width_ratio, orientation)
    across = shape[1] if orientation == "LEFT_RIGHT" else shape[0]
    center_px, up_px = [], []
    for _, center, width in view:
        leaf_width_px = width * dpmm
        leaf_center_px = center * dpmm + across / 2
        center_px.append(leaf_center_px)
        up_px.append(leaf_center_px - leaf_width_px / 2 * leaf_analysis_width_ratio)
    return [v[0] for v in view], center_px, up_px


def evaluate_batch(result: PFBatchResult, shape, dpmm: float, mlc="MILLENNIUM", orientation: str = "UP_DOWN",
                   leaf_analysis_width_ratio: float = 0.4, tolerance: float = 0.5,
                   action_tolerance: float | None = None) -> PFErrorsBatch:
    """What ``PicketFence.analyze`` computes after its measurement loop, for the ``analyze_batch`` result of frames of
    ``shape`` (H, W), in one launch and without a synchronisation: per picket the line ``np.polyfit(up, position, 1)`` over
    the leaves it measured, fitted over the leaf's upper marker coordinate; per window the error in mm, the position minus the
    line at the leaf's centre over ``dpmm``; per frame one ``summary`` row (``PF_SUMMARY_FIELDS``) -- the record a caller hands
    to ``dist.all_gather_records``.  The rule reproduces the reference's ``max_error``.  ``abs_median_error``
    is ``np.median`` of the |errors|, ``percent_passing`` counts |error| < tolerance (strictly), ``passed`` says that every
    measured window is under tolerance, ``percent_under_action`` is NaN without an ``action_tolerance``; a frame without a
    measured window has ``n_measured`` 0, ``passed`` 0 and NaN elsewhere.  ``max_error_leaf`` is the leaf NUMBER and
    ``max_error_picket`` the slot of the first maximum in leaf-major, then picket order (the reference's ``mlc_meas``).

    ``mlc``, ``orientation`` and ``leaf_analysis_width_ratio`` must be those of the ``analyze_batch`` call: the leaves in view
    must be ``result.leaf_nums`` (ValueError).  A ``separate_leaves`` result is refused: the reference's per-bank errors
    carry a nominal-gap offset that nothing here pins.  At most 4096 windows (leaves x picket slots) per frame."""
    if result.left is not None or result.right is not None:
        raise NotImplementedError("evaluate_batch takes the leaf-pair centres only (separate_leaves=False)")
    tolerance = float(tolerance)
    if not tolerance > 0:
        raise ValueError("tolerance must be positive")
    if action_tolerance is not None and not float(action_tolerance) < tolerance:
        raise ValueError("action_tolerance must be lower than tolerance")        # the reference's own rule (picketfence.py:702)
    nums, center_px, up_px = leaf_markers(shape, dpmm, mlc, orientation, leaf_analysis_width_ratio)
    if list(result.leaf_nums) != nums:
        raise ValueError("the leaves in view of this shape / dpmm / mlc / orientation are not result.leaf_nums")
    pos = ops._frames(result.position)
    if pos.dtype != torch.float64 or result.status.shape != pos.shape or result.status.dtype != torch.int32:
        raise TypeError("position float64 [N, leaves, cap] and status int32 of the same shape")
    n, nl, cap = pos.shape
    if nl != len(nums) or tuple(result.picket_count.shape) != (n,) or result.picket_count.dtype != torch.int32:
        raise ValueError("position [N, leaves, cap] does not go with leaf_nums / picket_count int32 [N]")
    dev = pos.device
    pos, st, cnt = pos.contiguous(), result.status.contiguous(), result.picket_count.contiguous()
    key = ("markers", tuple(nums), tuple(center_px), tuple(up_px), str(dev))
    if key not in _PLAN_CACHE:
        _PLAN_CACHE[key] = (torch.tensor(nums, dtype=torch.int32, device=dev),
                            torch.tensor(center_px, dtype=torch.float64, device=dev),
                            torch.tensor(up_px, dtype=torch.float64, device=dev))
    d_num, d_center, d_up = _PLAN_CACHE[key]
    fit = torch.empty((n, cap, 2), dtype=torch.float64, device=dev)
    pst = torch.empty((n, cap), dtype=torch.int32, device=dev)
    err = torch.empty((n, nl, cap), dtype=torch.float64, device=dev)
    ok = torch.empty((n, nl, cap), dtype=torch.uint8, device=dev)
    summary = torch.empty((n, len(PF_SUMMARY_FIELDS)), dtype=torch.float64, device=dev)
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    check(lib.pl_pf_errors(pos.data_ptr(), st.data_ptr(), cnt.data_ptr(), n, nl, cap, d_num.data_ptr(), d_center.data_ptr(),
                           d_up.data_ptr(), float(dpmm), tolerance,
                           float("nan") if action_tolerance is None else float(action_tolerance), fit.data_ptr(), pst.data_ptr(),
                           err.data_ptr(), ok.data_ptr(), summary.data_ptr(), stream), "pl_pf_errors")
    return PFErrorsBatch(fit, pst, err, ok, summary)
