"""JPEG Lossless Pixel Data (dicom.load_frames(jpeg_lossless=True) / decode_jpeg_lossless_frames / pl_dicom_jpegll_decode) on the
CPU emulator of tests/hipemu (kernel LOGIC where there is no GPU; the proof on hardware is tests/test_gpu_dicom_jpegll.py):
every case of tests/dicom_jpegll_checks.py but the frames of clinical size.  The emulator runs a fiber per work-item, so the
512 x 512 stack and the 1024 x 1024 frame run on the GPU only."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import dicom_jpegll_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


@pytest.mark.parametrize("precision", checks.PRECISIONS)
@pytest.mark.parametrize("sel", checks.SELECTIONS)
def test_emulated_every_predictor_and_precision(emulated, sel, precision):
    checks.check_predictor_precision(emulated, sel, precision)


@pytest.mark.parametrize("shape", checks.SEAM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sel", [1, 4, 5, 6, 7])
def test_emulated_wave_seams(emulated, sel, shape):
    checks.check_wave_seam(emulated, sel, shape)


def test_emulated_category_extremes(emulated):
    checks.check_category_extremes(emulated)


@pytest.mark.parametrize("kind", checks.TABLES)
def test_emulated_huffman_tables(emulated, kind):
    checks.check_table(emulated, kind)


def test_emulated_byte_stuffing_at_every_alignment_and_at_the_scans_end(emulated):
    checks.check_byte_stuffing(emulated)


def test_emulated_restart_intervals(emulated):
    checks.check_restart_intervals(emulated)


def test_emulated_point_transform(emulated):
    checks.check_point_transform(emulated)


def test_emulated_header_variety(emulated):
    checks.check_header_variety(emulated)


@pytest.mark.parametrize("dtype", checks.CONTAINERS, ids=lambda d: d.__name__)
def test_emulated_containers_at_every_alignment_through_the_kernel_entry(emulated, dtype):
    checks.check_container_kernel_entry(emulated, dtype)


@pytest.mark.parametrize("name", checks.FIXTURES)
def test_emulated_loader_keywords_equal_the_native_load(golden, emulated, name):
    checks.check_loader_fixture(golden, emulated, name)


def test_emulated_loader_rescale_of_a_series_and_file_by_file(golden, emulated):
    checks.check_loader_rescale_per_file(golden, emulated)


def test_emulated_fragments_offset_tables_stacks_and_sources(golden, emulated, tmp_path):
    checks.check_fragments_and_stacks(golden, emulated, tmp_path)


def test_emulated_dicom_image_reads_a_jpeg_lossless_file(golden, emulated):
    checks.check_dicom_image(golden, emulated)


def test_emulated_status_is_per_frame_and_check_raises(emulated):
    checks.check_status(emulated)


def test_emulated_refusals_and_malformed_streams(emulated):
    checks.check_refusals(emulated)


def test_emulated_c_abi_argument_checks(emulated):
    checks.check_c_abi_argument_checks(emulated)


def test_emulated_pil_decodes_the_8_bit_streams_alike(emulated):
    checks.check_pil_agrees(emulated)
