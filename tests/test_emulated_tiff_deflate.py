"""Deflate strips of pylinac_amd.tiff (load_frames(deflate=True), decode_tiff_strips with mask bit 8, pl_tiff_decode_ex) on the
CPU emulator of tests/hipemu (kernel LOGIC where there is no GPU; the proof on hardware is tests/test_gpu_tiff_deflate.py):
every case of tests/tiff_deflate_checks.py."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import tiff_deflate_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("name", sorted(checks.PIL_NAMES))
def test_emulated_pil_written_files_in_one_strip_and_in_strips_of_7_rows(emulated, name, predictor):
    checks.check_pil_written(emulated, name, predictor)


@pytest.mark.parametrize("rows,cols", checks.SHAPES)
def test_emulated_small_and_odd_shapes_in_strips_of_1_and_2_rows(emulated, rows, cols):
    checks.check_shape(emulated, rows, cols)


def test_emulated_hand_written_files_both_codes_byte_orders_predictors(emulated):
    checks.check_hand_written(emulated)


def test_emulated_zlib_levels_strategies_and_windows(emulated):
    checks.check_encoder_settings(emulated)


def test_emulated_constant_random_and_matches_at_distance_32768(emulated):
    checks.check_content(emulated)


def test_emulated_uint8_and_rgb_with_predictor_2(emulated):
    checks.check_uint8_and_rgb(emulated)


def test_emulated_mixed_stack_of_four_compressions(emulated):
    checks.check_mixed_stack(emulated)


def test_emulated_trailing_bytes_cut_trailer_and_longer_stream_are_accepted(emulated):
    checks.check_accepted_oddities(emulated)


def test_emulated_damaged_files_are_flagged_per_file_and_check_raises(emulated, monkeypatch):
    checks.check_damage(emulated, monkeypatch)


def test_emulated_window_outside_the_buffer_is_flagged_and_the_frame_untouched(emulated):
    checks.check_window_outside_the_buffer(emulated)


def test_emulated_refusals_with_and_without_the_keyword(emulated):
    checks.check_refusals(emulated)


def test_emulated_c_abi_argument_checks(emulated):
    checks.check_c_abi_argument_checks(emulated)
