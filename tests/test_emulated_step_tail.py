"""pl_median3_threshold_profile_fwxm_u16 on the CPU emulator of tests/hipemu (kernel LOGIC where there is no GPU; the proof on
hardware is tests/test_gpu_step_tail.py): the same cases from tests/step_tail_checks.py."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import step_tail_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


@pytest.mark.parametrize("shape", checks.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_emulated_in_launch_tail_vs_separate_launches(emulated, shape):
    assert checks.check_shape(emulated, shape) == shape[0]


def test_emulated_in_launch_tail_threshold_above_maximum(emulated):
    checks.check_threshold_above_maximum(emulated)


def test_emulated_in_launch_tail_workspace_returns_to_zero(emulated):
    checks.check_workspace_reuse(emulated)


def test_emulated_in_launch_tail_sub_range(emulated):
    checks.check_sub_range(emulated)
