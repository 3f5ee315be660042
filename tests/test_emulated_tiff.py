"""Strip TIFFs (tiff.load_frames / decode_tiff_strips / pl_tiff_decode) on the CPU emulator of tests/hipemu (kernel LOGIC where
there is no GPU; the proof on hardware is tests/test_gpu_tiff.py): every case of tests/tiff_checks.py.  The emulator runs a
fiber per work-item, so the 1024 x 1024 frames and the hand-over to an analyzer run on the GPU only."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import tiff_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


@pytest.mark.parametrize("predictor", [1, 2])
def test_emulated_ridge_with_noise_reaches_12_bits_clears_and_kwkwk(emulated, predictor):
    checks.check_ridge(emulated, predictor)


def test_emulated_constant_frame_is_kwkwk_chains_of_long_strings(emulated):
    checks.check_constant(emulated)


def test_emulated_uint8_frame(emulated):
    checks.check_uint8(emulated)


def test_emulated_random_frame_grows_under_lzw(emulated):
    checks.check_random(emulated)


@pytest.mark.parametrize("rows,cols", checks.SHAPES)
def test_emulated_small_and_odd_shapes(emulated, rows, cols):
    checks.check_shape(emulated, rows, cols)


def test_emulated_strip_geometry_and_odd_offsets(emulated):
    checks.check_strip_geometry(emulated)


def test_emulated_big_endian_files(emulated):
    checks.check_big_endian(emulated)


def test_emulated_packbits_strips(emulated):
    checks.check_packbits(emulated)


def test_emulated_rgb_collapses_like_pil_convert_i(emulated):
    checks.check_rgb(emulated)


def test_emulated_mixed_stack(emulated):
    checks.check_mixed_stack(emulated)


def test_emulated_dtype_and_sources(emulated, tmp_path):
    checks.check_dtype_and_sources(emulated, tmp_path)


def test_emulated_dpi_and_dpmm(emulated):
    checks.check_dpi(emulated)


def test_emulated_status_is_per_frame_and_check_raises(emulated, monkeypatch):
    checks.check_status(emulated, monkeypatch)


def test_emulated_window_outside_the_buffer_is_flagged_and_the_frame_untouched(emulated):
    checks.check_window_outside_the_buffer(emulated)


def test_emulated_refusals_and_the_ifd_walk(emulated):
    checks.check_refusals(emulated)


def test_emulated_c_abi_argument_checks(emulated):
    checks.check_c_abi_argument_checks(emulated)
