"""pl_median3_threshold_profile_fwxm_cells_keep_u16 and EpidPipeline(keep_zeros=True) on the MI355X: the cases of
tests/keep_zeros_checks.py (the same on the CPU emulator: tests/test_emulated_keep_zeros.py)."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import keep_zeros_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w", checks.WIDTHS)
def test_sequence_a_b_a_on_one_out_and_table(dev, w):
    checks.check_sequence(dev, w)


@pytest.mark.parametrize("w", checks.WIDTHS)
def test_stores_are_skipped_and_reset_rewrites(dev, w):
    checks.check_stores_are_skipped(dev, w)


@pytest.mark.parametrize("w", checks.WIDTHS)
def test_sub_range_leaves_the_other_frames_alone(dev, w):
    checks.check_sub_range(dev, w)


@pytest.mark.parametrize("w", checks.WIDTHS)
def test_threshold_above_every_maximum_stores_nothing_the_second_time(dev, w):
    checks.check_threshold_above_everything(dev, w)


def test_pipeline_alternating_batches_forget_out_and_full_range(dev):
    checks.check_pipeline(dev)


def test_pipeline_partial_passes_forget_out_and_keep_zeros_switch(dev):
    checks.check_pipeline_bookkeeping(dev)
