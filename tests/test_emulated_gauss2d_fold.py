"""gauss2d_mm's leaner vector work on the CPU emulator of tests/hipemu (kernel LOGIC where there is no GPU; the proof on
hardware is tests/test_gpu_gauss2d_fold.py): the cases of tests/gauss2d_fold_checks.py against scipy, and the host's verdict
on the taps."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "hipemu"))

import gauss2d_fold_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    import build as emu_build  # tests/hipemu/build.py
    from emu_backend import emulated_device

    if "gaussian_mm.hip" not in emu_build.SOURCES:
        pytest.skip("no clang++ host compiler: gaussian_mm.hip is not in the emulated library")
    with emulated_device():
        yield torch.device("cuda:0")


@pytest.mark.parametrize("case,sigma", [(c, s) for c in checks.CASES for s in checks.CASES[c][2]])
def test_emulated_frames_equal_scipy(emulated, case, sigma):
    checks.check_case(emulated, case, sigma)


def test_emulated_host_takes_scipy_taps_and_refuses_scaled_ones(emulated):
    checks.check_host_taps(emulated)
