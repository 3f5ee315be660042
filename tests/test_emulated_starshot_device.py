"""starshot.wobble_batch / pl_starshot_wobble on the CPU emulator of tests/hipemu (kernel LOGIC where there is no GPU; the proof
on hardware is tests/test_gpu_starshot_device.py): the cases of tests/starshot_device_checks.py."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import starshot_device_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


@pytest.mark.parametrize("chunk", range(checks.CHUNKS))
def test_emulated_fit_equals_scipy_nelder_mead_on_300_seeded_sets(emulated, chunk):
    checks.check_fit_against_scipy(emulated, chunk)


@pytest.mark.parametrize("recursive", [True, False])
def test_emulated_constructed_cases_against_line_manager_and_accept(emulated, recursive):
    checks.check_constructed(emulated, recursive)


def test_emulated_golden_peaks_give_the_golden_wobble(golden, emulated):
    checks.check_goldens(golden, emulated)


def test_emulated_validation_and_row_independence(emulated):
    checks.check_validation(emulated)


def test_emulated_profile_tail_equals_star_profile_on_golden_frames(golden, emulated):
    checks.check_tail(golden, emulated, names=("inverted", "nofwhm"))


@pytest.mark.parametrize("which", ("inverted", "retry", "blank"))
def test_emulated_analyzers_false_equals_the_default_path(golden, emulated, which):
    checks.check_end_to_end(golden, emulated, which)


def test_emulated_ring_with_more_peaks_than_the_table_takes_the_class_path(golden, emulated):
    checks.check_fallback(golden, emulated)
