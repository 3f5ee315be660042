"""starshot.wobble_batch / pl_starshot_wobble on the MI355X: the cases of tests/starshot_device_checks.py (the same on the CPU
emulator: tests/test_emulated_starshot_device.py)."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import starshot_device_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("chunk", range(checks.CHUNKS))
def test_fit_equals_scipy_nelder_mead_on_300_seeded_sets(dev, chunk):
    checks.check_fit_against_scipy(dev, chunk)


@pytest.mark.parametrize("recursive", [True, False])
def test_constructed_cases_against_line_manager_and_accept(dev, recursive):
    checks.check_constructed(dev, recursive)


def test_golden_peaks_give_the_golden_wobble(golden, dev):
    checks.check_goldens(golden, dev)


def test_validation_and_row_independence(dev):
    checks.check_validation(dev)


def test_profile_tail_equals_star_profile_on_golden_frames(golden, dev):
    checks.check_tail(golden, dev)


@pytest.mark.parametrize("which", checks.E2E_STACKS)
def test_analyzers_false_equals_the_default_path(golden, dev, which):
    checks.check_end_to_end(golden, dev, which)


def test_ring_with_more_peaks_than_the_table_takes_the_class_path(golden, dev):
    checks.check_fallback(golden, dev)
