"""The offset-predicated row walk of the EPID step's threshold launch on the CPU emulator of tests/hipemu (kernel LOGIC where
there is no GPU; the proof on hardware is tests/test_gpu_threshold_walk.py): the ragged shapes of
tests/threshold_walk_checks.py, two of the seam places, and the size guard.  The other seam places stay with the GPU file."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import threshold_walk_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


@pytest.mark.parametrize("w", checks.RAGGED_WIDTHS)
@pytest.mark.parametrize("h", checks.RAGGED_HEIGHTS)
def test_emulated_ragged_rows_and_rings_deeper_than_the_frame(emulated, h, w):
    checks.check_ragged(emulated, h, w)


@pytest.mark.parametrize("place", checks.SEAM_PLACES[:2])
def test_emulated_one_needed_cell_beside_the_seam(emulated, place):
    checks.check_seam_keep(emulated, place)
    checks.check_seam_cells(emulated, place)


def test_emulated_frames_of_2_to_the_31_bytes_are_not_covered(emulated):
    from pylinac_amd import _lib

    checks.check_size_guard(_lib.load())
