"""gauss2d_mm's leaner vector work on the MI355X: the cases of tests/gauss2d_fold_checks.py against scipy (the same on the
CPU emulator: tests/test_emulated_gauss2d_fold.py)."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import gauss2d_fold_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,sigma", [(c, s) for c in checks.CASES for s in checks.CASES[c][2]])
def test_frames_equal_scipy(dev, case, sigma):
    checks.check_case(dev, case, sigma)


def test_host_takes_scipy_taps_and_refuses_scaled_ones(dev):
    checks.check_host_taps(dev)
