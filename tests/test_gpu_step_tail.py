"""pl_median3_threshold_profile_fwxm_u16 on the MI355X: the EPID step's threshold launch with the tail inside it == the
launches it replaces, bit for bit (tests/step_tail_checks.py has the cases and why each shape is there)."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import step_tail_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", checks.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_in_launch_tail_vs_separate_launches(dev, shape):
    assert checks.check_shape(dev, shape) == shape[0]


def test_in_launch_tail_threshold_above_maximum(dev):
    checks.check_threshold_above_maximum(dev)


def test_in_launch_tail_workspace_returns_to_zero(dev):
    checks.check_workspace_reuse(dev)


def test_in_launch_tail_sub_range(dev):
    checks.check_sub_range(dev)


def test_pipeline_in_launch_tail_vs_old_paths(dev):
    checks.check_pipeline(dev)
