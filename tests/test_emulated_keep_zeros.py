"""pl_median3_threshold_profile_fwxm_cells_keep_u16 on the CPU emulator of tests/hipemu (kernel LOGIC where there is no GPU;
the proof on hardware is tests/test_gpu_keep_zeros.py): the launch-level cases of tests/keep_zeros_checks.py and
EpidPipeline's bookkeeping on 2 x 64 x 128 frames.  The 4 x 128 x 576 pipeline case stays with the GPU file: the emulator takes
a minute and a half over it."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import keep_zeros_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


@pytest.mark.parametrize("w", checks.WIDTHS)
def test_emulated_sequence_a_b_a_on_one_out_and_table(emulated, w):
    checks.check_sequence(emulated, w)


@pytest.mark.parametrize("w", checks.WIDTHS)
def test_emulated_stores_are_skipped_and_reset_rewrites(emulated, w):
    checks.check_stores_are_skipped(emulated, w)


@pytest.mark.parametrize("w", checks.WIDTHS)
def test_emulated_sub_range_leaves_the_other_frames_alone(emulated, w):
    checks.check_sub_range(emulated, w)


@pytest.mark.parametrize("w", checks.WIDTHS)
def test_emulated_threshold_above_every_maximum_stores_nothing_the_second_time(emulated, w):
    checks.check_threshold_above_everything(emulated, w)


def test_emulated_pipeline_partial_passes_forget_out_and_keep_zeros_switch(emulated):
    checks.check_pipeline_bookkeeping(emulated)
