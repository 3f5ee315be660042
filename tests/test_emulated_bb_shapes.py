"""The BB finder on the CPU emulator of tests/hipemu (kernel LOGIC where there is no GPU; the proof on hardware is
tests/test_gpu_bb_shapes.py): the subset of tests/bb_shape_checks.py that the emulator, at about ten seconds per window and
call, can afford -- the hull paths' switch, hole filling, a pair on the solidity bound, a pair on the size / circumference bound and the clipped uint16 frame."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bb_shape_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


@pytest.mark.parametrize("name", checks.EMULATED)
def test_emulated_bb_finder_on_shape_window(golden, emulated, name):
    checks.check_window(emulated, golden("bb_shapes"), name)


def test_emulated_bb_centroids_on_clipped_uint16_frame(golden, emulated):
    checks.check_u16(emulated, golden("bb_shapes"), (2,))
