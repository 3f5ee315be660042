"""picketfence.evaluate_batch / pl_pf_errors on the MI355X: the cases of tests/pf_errors_checks.py (the same on the CPU emulator:
tests/test_emulated_pf_errors.py)."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import pf_errors_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nl,cap,n", checks.SIZES)
def test_table_sizes_against_the_restatement(dev, nl, cap, n):
    checks.check_size(dev, nl, cap, n)


def test_one_leaf_picket_two_leaf_picket_empty_and_all_nan_frames(dev):
    checks.check_special(dev)


def test_even_and_odd_number_of_measured_windows(dev):
    checks.check_parity(dev)


@pytest.mark.parametrize("which", ["hd", "agility_lr"])
def test_banks_with_two_leaf_widths_and_left_right_pickets(dev, which):
    checks.check_bank(dev, which)


def test_constructed_tie_reports_the_first_window_in_leaf_major_order(dev):
    checks.check_tie(dev)


def test_frame_alone_equals_frame_in_batch_and_runs_repeat_bit_for_bit(dev):
    checks.check_independence(dev)


def test_limits_and_validation(dev):
    checks.check_limits_and_validation(dev)


def test_end_to_end_reference_max_error_on_the_seven_golden_frames(golden, dev):
    checks.check_end_to_end(golden, dev)
