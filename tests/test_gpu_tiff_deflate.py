"""Deflate strips of pylinac_amd.tiff (load_frames(deflate=True), decode_tiff_strips with mask bit 8, pl_tiff_decode_ex) on the
MI355X: every case of tests/tiff_deflate_checks.py (the same ones tests/test_emulated_tiff_deflate.py runs on the CPU emulator),
and a 1024 x 1024 uint16 picket-fence frame as Deflate + predictor 2 in PIL's 64 KiB strips (32 waves a file) and as ONE strip
(2 MiB of output from one wave)."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import tiff_deflate_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("name", sorted(checks.PIL_NAMES))
def test_pil_written_files_in_one_strip_and_in_strips_of_7_rows(dev, name, predictor):
    checks.check_pil_written(dev, name, predictor)


@pytest.mark.parametrize("rows,cols", checks.SHAPES)
def test_small_and_odd_shapes_in_strips_of_1_and_2_rows(dev, rows, cols):
    checks.check_shape(dev, rows, cols)


def test_hand_written_files_both_codes_byte_orders_predictors(dev):
    checks.check_hand_written(dev)


def test_zlib_levels_strategies_and_windows(dev):
    checks.check_encoder_settings(dev)


def test_constant_random_and_matches_at_distance_32768(dev):
    checks.check_content(dev)


def test_uint8_and_rgb_with_predictor_2(dev):
    checks.check_uint8_and_rgb(dev)


def test_mixed_stack_of_four_compressions(dev):
    checks.check_mixed_stack(dev)


def test_trailing_bytes_cut_trailer_and_longer_stream_are_accepted(dev):
    checks.check_accepted_oddities(dev)


def test_damaged_files_are_flagged_per_file_and_check_raises(dev, monkeypatch):
    checks.check_damage(dev, monkeypatch)


def test_window_outside_the_buffer_is_flagged_and_the_frame_untouched(dev):
    checks.check_window_outside_the_buffer(dev)


def test_refusals_with_and_without_the_keyword(dev):
    checks.check_refusals(dev)


def test_c_abi_argument_checks(dev):
    checks.check_c_abi_argument_checks(dev)


@pytest.fixture(scope="module")
def film_frames():
    from pylinac_amd.synthetic import pf_frames

    return checks.to_np(pf_frames(2, 1024, 1024, seed0=2600))


def test_detector_size_frame_in_64_kib_strips_and_the_stack_a_b_a(dev, film_frames):
    """two 1024 x 1024 uint16 picket-fence frames as Deflate + predictor 2 in PIL's default strips, encoded once each: 32
    zlib streams of 64 KiB of output a file, as the stack [A, B, A]: exactly what PIL reads"""
    from pylinac_amd import tiff

    files = [checks.pil_file(f, "tiff_adobe_deflate", predictor=2) for f in film_frames]
    info = tiff.read_tiff(files[0])
    assert len(info.strips) == 32 and all(rows * info.width * 2 == 65536 for _, _, _, rows in info.strips)
    assert all(files[0][o:o + 2] == b"\x78\x9c" for o, _, _, _ in info.strips)
    order = [0, 1, 0]
    stack = tiff.load_frames([files[k] for k in order], device=dev, check=False, deflate=True)
    assert stack.frames.dtype == torch.uint16 and stack.status.cpu().tolist() == [0, 0, 0]
    assert np.array_equal(checks.to_np(stack.frames), film_frames[order])


def test_detector_size_frame_as_one_strip(dev, film_frames):
    """the same frame as ONE strip: 2 MiB of output, 64 turns of the 32 KiB ring, from one wave"""
    from pylinac_amd import tiff

    f = checks.pil_file(film_frames[0], "tiff_adobe_deflate", predictor=2, rows_per_strip=1024)
    assert len(tiff.read_tiff(f).strips) == 1
    got, stack = checks.load(dev, [f])
    assert stack.status.cpu().tolist() == [0] and np.array_equal(got[0], film_frames[0])
