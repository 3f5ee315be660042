"""The edge sweeps of tests/edge_sweep_checks.py on the MI355X (the same on the CPU emulator: tests/test_emulated_kernels.py).
The emulator runs work-items one after another, rewrites inline assembly and is host clang at -O1: a race in the union-find,
an instruction that misbehaves or a device-compiler difference shows only here."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import edge_sweep_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [np.dtype(d).name for d in checks.STENCIL_DTYPES])
def test_stencils_awkward(dev, dtype):
    checks.check_stencils_awkward(dev, dtypes=(np.dtype(dtype).type,))


def test_label_zoo(dev):
    checks.check_label_zoo(dev, big=False)


@pytest.mark.parametrize("shape", list(checks.CONTENTION))
def test_label_zoo_big(dev, shape):
    checks.check_label_zoo(dev, big=True, only=(shape,))


def test_find_peaks_sweep(dev):
    checks.check_find_peaks_sweep(dev)


def test_reductions_sweep(dev):
    checks.check_reductions_sweep(dev)


def test_wl_xim_gamma_random(dev):
    checks.check_wl_xim_gamma_random(dev)


def test_pf_random_frames(dev):
    checks.check_pf_random_frames(dev)
