"""dicom.load_zip(encapsulated=True), dicom.index_encapsulated / pl_dicom_encap_index and dicom.copy_ranges / pl_copy_ranges on
the MI355X: every case of tests/dicom_zip_encap_checks.py (the same ones tests/test_emulated_dicom_zip_encap.py runs on the CPU
emulator), and what only the GPU runs: 64 members side by side (JPEG Lossless and RLE), a 3 MB copy at odd alignment and item
offsets beyond 2^31."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import dicom_zip_encap_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


def test_rle_members_equal_load_frames(dev):
    checks.check_rle_members(dev)


def test_jpeg_lossless_members_equal_load_frames(dev):
    checks.check_jpegll_members(dev)


def test_frames_that_span_fragments_are_laid_end_to_end_by_one_copy(dev):
    checks.check_spanning_fragments(dev)


def test_headers_at_the_head_boundary_and_the_fallback_fetches(dev):
    checks.check_head_boundary(dev)


def test_forty_fragments_take_a_second_index_call(dev):
    checks.check_capacity(dev)


def test_header_longer_than_the_first_prefix(dev):
    checks.check_long_header(dev)


def test_damaged_item_sequences_in_load_frames_words(dev):
    checks.check_damaged_items(dev)


def test_damaged_rle_headers_and_jpeg_markers(dev):
    checks.check_damaged_headers(dev)


def test_scan_status_names_member_and_frame(dev):
    checks.check_scan_status(dev)


def test_mixed_kinds_other_syntaxes_defaults_and_verify(dev):
    checks.check_kinds_and_defaults(dev)


def test_index_kernel_against_the_restated_walk(dev):
    checks.check_index_kernel(dev)


def test_index_kernel_offsets_beyond_two_gib(dev):
    checks.check_index_far_offsets(dev)


def test_copy_kernel_against_numpy(dev):
    checks.check_copy_kernel(dev)


def test_copy_kernel_three_megabytes_at_odd_alignment(dev):
    checks.check_copy_large(dev)


def test_c_abi_argument_checks(dev):
    checks.check_c_abi_argument_checks(dev)


@pytest.mark.parametrize("kind", ["jpegll", "rle"])
def test_volume_of_64_deflated_members_of_128_x_128(dev, kind):
    checks.check_volume(dev, checks.jl.jpegll_file if kind == "jpegll" else checks.rle.rle_file)
