"""picketfence.evaluate_batch / pl_pf_errors on the CPU emulator of tests/hipemu (kernel LOGIC where there is no GPU; the proof
on hardware is tests/test_gpu_pf_errors.py): the cases of tests/pf_errors_checks.py.  End to end the emulator measures two of
the seven golden frames (the two-width bank and the LEFT_RIGHT one): it takes seconds per frame over analyze_batch; all seven
run on the GPU."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import pf_errors_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


@pytest.mark.parametrize("nl,cap,n", checks.SIZES)
def test_emulated_table_sizes_against_the_restatement(emulated, nl, cap, n):
    checks.check_size(emulated, nl, cap, n)


def test_emulated_one_leaf_picket_two_leaf_picket_empty_and_all_nan_frames(emulated):
    checks.check_special(emulated)


def test_emulated_even_and_odd_number_of_measured_windows(emulated):
    checks.check_parity(emulated)


@pytest.mark.parametrize("which", ["hd", "agility_lr"])
def test_emulated_banks_with_two_leaf_widths_and_left_right_pickets(emulated, which):
    checks.check_bank(emulated, which)


def test_emulated_constructed_tie_reports_the_first_window_in_leaf_major_order(emulated):
    checks.check_tie(emulated)


def test_emulated_frame_alone_equals_frame_in_batch_and_runs_repeat_bit_for_bit(emulated):
    checks.check_independence(emulated)


def test_emulated_limits_and_validation(emulated):
    checks.check_limits_and_validation(emulated)


def test_emulated_end_to_end_reference_max_error_on_golden_frames(golden, emulated):
    checks.check_end_to_end(golden, emulated, tags=("hd", "agility_lr"))
