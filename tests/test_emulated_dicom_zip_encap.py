"""dicom.load_zip(encapsulated=True), dicom.index_encapsulated / pl_dicom_encap_index and dicom.copy_ranges / pl_copy_ranges on
the CPU emulator of tests/hipemu (kernel LOGIC where there is no GPU; the proof on hardware is
tests/test_gpu_dicom_zip_encap.py): every case of tests/dicom_zip_encap_checks.py but the GPU-only sizes.  The emulator runs a
fiber per work-item, so a member stays below about 100 KiB inflated here (the one with a 150 KiB header element excepted)."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import dicom_zip_encap_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


def test_emulated_rle_members_equal_load_frames(emulated):
    checks.check_rle_members(emulated)


def test_emulated_jpeg_lossless_members_equal_load_frames(emulated):
    checks.check_jpegll_members(emulated)


def test_emulated_frames_that_span_fragments_are_laid_end_to_end_by_one_copy(emulated):
    checks.check_spanning_fragments(emulated)


def test_emulated_headers_at_the_head_boundary_and_the_fallback_fetches(emulated):
    checks.check_head_boundary(emulated)


def test_emulated_forty_fragments_take_a_second_index_call(emulated):
    checks.check_capacity(emulated)


def test_emulated_header_longer_than_the_first_prefix(emulated):
    checks.check_long_header(emulated)


def test_emulated_damaged_item_sequences_in_load_frames_words(emulated):
    checks.check_damaged_items(emulated)


def test_emulated_damaged_rle_headers_and_jpeg_markers(emulated):
    checks.check_damaged_headers(emulated)


def test_emulated_scan_status_names_member_and_frame(emulated):
    checks.check_scan_status(emulated)


def test_emulated_mixed_kinds_other_syntaxes_defaults_and_verify(emulated):
    checks.check_kinds_and_defaults(emulated)


def test_emulated_index_kernel_against_the_restated_walk(emulated):
    checks.check_index_kernel(emulated)


def test_emulated_copy_kernel_against_numpy(emulated):
    checks.check_copy_kernel(emulated)


def test_emulated_c_abi_argument_checks(emulated):
    checks.check_c_abi_argument_checks(emulated)
