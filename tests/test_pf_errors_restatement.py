"""The numpy restatement of the picket fits and leaf errors (tests/pf_errors_checks.py: `restate`) against the ``max_error``
the reference's own ``PicketFence.analyze()`` returned (picketfence.npz, picketfence_mlc.npz, bench_size.npz): EXACTLY equal.
No device is involved; this is what ties tests/test_emulated_pf_errors.py and tests/test_gpu_pf_errors.py, which compare
picketfence.evaluate_batch with the restatement, to the reference."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

import pf_errors_checks as checks  # noqa: E402


def test_restatement_equals_reference_max_error_on_the_seven_golden_frames(golden):
    seen = []
    for tag, raw, dpmm, mlc, orient, max_error in checks.golden_frames(golden):
        want = checks.restate_golden(tag, raw, dpmm, mlc, orient)
        assert want["summary"][1] == max_error, (tag, want["summary"][1], max_error)
        assert want["summary"][0] > 150 and (want["picket_status"] == 0).all()
        seen.append((mlc, orient))
    assert len(seen) == 7 and ("HD_MILLENNIUM", "UP_DOWN") in seen and ("AGILITY", "LEFT_RIGHT") in seen


def test_restatement_equals_reference_max_error_on_the_bench_size_tables(golden):
    for k, pos, st, nums, c_px, u_px, dpmm, max_error in checks.bench_size_tables(golden):
        want = checks.restate(pos, st, 10, nums, c_px, u_px, dpmm)
        assert want["summary"][0] == 500
        assert want["summary"][1] == max_error, (k, want["summary"][1], max_error)


def test_fitting_at_the_leaf_centre_is_not_the_rule(golden):
    """the upper marker as the fit's abscissa is pinned, not a matter of taste: on the HD Millennium (two leaf widths) the
    line through (centre, position) gives another max_error"""
    for tag, raw, dpmm, mlc, orient, max_error in checks.golden_frames(golden):
        if mlc != "HD_MILLENNIUM":
            continue
        pos, st, nums = checks.oracle_table(tag, raw, dpmm, mlc, orient)
        _, c_px, _ = checks.geometry(raw.shape, dpmm, mlc, orient)
        other = checks.restate(pos, st, pos.shape[1], nums, c_px, c_px, dpmm)["summary"][1]
        assert other != max_error and abs(other - max_error) < 1e-4


def test_two_largest_errors_of_every_golden_are_apart(golden):
    """what lets the device tests ask for the restatement's leaf and picket: no golden's maximum is a near tie"""
    for tag, raw, dpmm, mlc, orient, _ in checks.golden_frames(golden):
        a = np.abs(checks.restate_golden(tag, raw, dpmm, mlc, orient)["error"]).ravel()
        a = np.sort(a[~np.isnan(a)])
        assert a[-1] - a[-2] > 1e-4, tag
