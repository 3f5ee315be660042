"""RLE Lossless Pixel Data (dicom.load_frames / decode_rle_frames / pl_dicom_rle_decode) on the CPU emulator of tests/hipemu
(kernel LOGIC where there is no GPU; the proof on hardware is tests/test_gpu_dicom_rle.py): every case of
tests/dicom_rle_checks.py.  The emulator runs a fiber per work-item, so the three 1024 x 1024 frames (more than 1000 chunks per
segment) and the hand-over to an analyzer run on the GPU only."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import dicom_rle_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


def test_emulated_every_entry_offset_of_a_chunk_occurs_and_decodes(emulated):
    checks.check_every_entry_offset(emulated)


@pytest.mark.parametrize("name", checks.SEAMS)
def test_emulated_chunk_seams(emulated, name):
    checks.check_chunk_seam(emulated, name)


def test_emulated_constant_plane_expands_64_times_the_chunk(emulated):
    checks.check_constant_plane(emulated)


def test_emulated_noise_plane_is_all_literals(emulated):
    checks.check_noise_plane(emulated)


@pytest.mark.parametrize("rows,cols", checks.SHAPES)
def test_emulated_small_and_odd_shapes(emulated, rows, cols):
    checks.check_small_shape(emulated, rows, cols)


def test_emulated_no_ops_runs_across_rows_and_the_pad_byte(emulated):
    checks.check_encoder_options(emulated)


@pytest.mark.parametrize("dtype", checks.CONTAINERS, ids=lambda d: d.__name__)
def test_emulated_containers_at_every_alignment_through_the_kernel_entry(emulated, dtype):
    checks.check_container_kernel_entry(emulated, dtype)


@pytest.mark.parametrize("dtype", checks.CONTAINERS, ids=lambda d: d.__name__)
def test_emulated_containers_through_the_loader(emulated, dtype):
    checks.check_container_loader(emulated, dtype)


@pytest.mark.parametrize("name", ["u16_explicit", "u16_explicit_shifted", "u16_sequence", "i16_ct", "u16_stored12_dirty",
                                  "i16_stored12_dirty", "u8_multiframe", "u8_odd", "i8", "u32", "u16_inverted_sign", "u16_epid_tags"])
def test_emulated_loader_keywords_equal_the_native_load(golden, emulated, name):
    checks.check_loader_fixture(golden, emulated, name)


def test_emulated_loader_rescale_of_a_series_and_file_by_file(golden, emulated):
    checks.check_loader_rescale_per_file(golden, emulated)


def test_emulated_multiframe_offset_tables_stacks_and_sources(golden, emulated, tmp_path):
    checks.check_loader_multiframe_and_stacks(golden, emulated, tmp_path)


def test_emulated_dicom_image_reads_an_rle_file(golden, emulated):
    checks.check_dicom_image(golden, emulated)


def test_emulated_status_is_per_frame_and_check_raises_or_warns_like_pydicom(emulated):
    checks.check_status(emulated)


def test_emulated_window_outside_the_buffer_is_flagged_and_the_frame_untouched(emulated):
    checks.check_window_outside_the_buffer(emulated)


def test_emulated_malformed_headers_other_syntaxes_and_mixtures_are_refused(golden, emulated):
    checks.check_malformed_and_refused(golden, emulated)


def test_emulated_c_abi_argument_checks(emulated):
    checks.check_c_abi_argument_checks(emulated)
