"""The offset-predicated row walk of the EPID step's threshold launch on the MI355X: the cases of
tests/threshold_walk_checks.py (the smaller ones also on the CPU emulator: tests/test_emulated_threshold_walk.py)."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import threshold_walk_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("place", checks.SEAM_PLACES)
def test_one_needed_cell_beside_the_seam_reset_then_kept_canary(dev, place):
    checks.check_seam_keep(dev, place)


@pytest.mark.parametrize("place", checks.SEAM_PLACES)
def test_one_needed_cell_beside_the_seam_without_the_kept_zero_table(dev, place):
    checks.check_seam_cells(dev, place)


@pytest.mark.parametrize("w", checks.RAGGED_WIDTHS)
@pytest.mark.parametrize("h", checks.RAGGED_HEIGHTS)
def test_ragged_rows_and_rings_deeper_than_the_frame(dev, h, w):
    checks.check_ragged(dev, h, w)


def test_frames_of_2_to_the_31_bytes_are_not_covered(dev):
    from pylinac_amd import _lib

    checks.check_size_guard(_lib.load())
