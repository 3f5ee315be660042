"""JPEG Lossless Pixel Data (dicom.load_frames(jpeg_lossless=True) / decode_jpeg_lossless_frames / pl_dicom_jpegll_decode) on the
MI355X: every case of tests/dicom_jpegll_checks.py (the same ones tests/test_emulated_dicom_jpegll.py runs on the CPU emulator),
a stack of three 512 x 512 int16 CT-like slices and one 1024 x 1024 uint16 frame -- more than a thousand input windows of one
wave's chain."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import dicom_jpegll_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision", checks.PRECISIONS)
@pytest.mark.parametrize("sel", checks.SELECTIONS)
def test_every_predictor_and_precision(dev, sel, precision):
    checks.check_predictor_precision(dev, sel, precision)


@pytest.mark.parametrize("shape", checks.SEAM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sel", [1, 4, 5, 6, 7])
def test_wave_seams(dev, sel, shape):
    checks.check_wave_seam(dev, sel, shape)


def test_category_extremes(dev):
    checks.check_category_extremes(dev)


@pytest.mark.parametrize("kind", checks.TABLES)
def test_huffman_tables(dev, kind):
    checks.check_table(dev, kind)


def test_byte_stuffing_at_every_alignment_and_at_the_scans_end(dev):
    checks.check_byte_stuffing(dev)


def test_restart_intervals(dev):
    checks.check_restart_intervals(dev)


def test_point_transform(dev):
    checks.check_point_transform(dev)


def test_header_variety(dev):
    checks.check_header_variety(dev)


@pytest.mark.parametrize("dtype", checks.CONTAINERS, ids=lambda d: d.__name__)
def test_containers_at_every_alignment_through_the_kernel_entry(dev, dtype):
    checks.check_container_kernel_entry(dev, dtype)


@pytest.mark.parametrize("name", checks.FIXTURES)
def test_loader_keywords_equal_the_native_load(golden, dev, name):
    checks.check_loader_fixture(golden, dev, name)


def test_loader_rescale_of_a_series_and_file_by_file(golden, dev):
    checks.check_loader_rescale_per_file(golden, dev)


def test_fragments_offset_tables_stacks_and_sources(golden, dev, tmp_path):
    checks.check_fragments_and_stacks(golden, dev, tmp_path)


def test_dicom_image_reads_a_jpeg_lossless_file(golden, dev):
    checks.check_dicom_image(golden, dev)


def test_status_is_per_frame_and_check_raises(dev):
    checks.check_status(dev)


def test_refusals_and_malformed_streams(dev):
    checks.check_refusals(dev)


def test_c_abi_argument_checks(dev):
    checks.check_c_abi_argument_checks(dev)


def test_pil_decodes_the_8_bit_streams_alike(dev):
    checks.check_pil_agrees(dev)


def test_three_ct_slices_of_512_x_512(dev):
    checks.check_ct_stack(dev)


def test_one_frame_of_1024_x_1024(dev):
    checks.check_large_frame(dev)
