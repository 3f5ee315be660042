"""Tier 2 of JPEG 2000 on the device (dicom.plan_jpeg2000_blocks / pl_dicom_j2k_plan) and
dicom.load_zip(encapsulated=True, jpeg2000=True) on the MI355X: every case of tests/dicom_zip_j2k_checks.py.  No stack is
larger than 5 frames of 29 x 35 or 3 streams of 129 x 67."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import dicom_j2k_checks as jk  # noqa: E402
import dicom_zip_j2k_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("block", jk.BLOCKS, ids=lambda b: f"cb{b[0]}")
def test_plan_equals_the_host_parser_on_noise_of_129x67(dev, block):
    checks.check_plan_geometry(dev, block)


def test_plan_equals_the_host_parser_on_small_shapes(dev):
    checks.check_plan_shapes(dev)


def test_plan_equals_the_host_parser_on_oblong_blocks_and_progression_orders(dev):
    checks.check_plan_oblong_and_orders(dev)


def test_plan_equals_the_host_parser_on_constant_low_signed_precinct_and_open_ended_streams(dev):
    checks.check_plan_contents(dev)


def test_plan_streams_use_every_codeword_class_of_table_b4(dev):
    passes = checks.check_plan_contents(dev) | checks.check_plan_geometry(dev, (32, 32))
    checks.check_pass_classes(passes)


def test_plan_status_is_per_frame(dev):
    checks.check_plan_status(dev)


def test_plan_c_abi_argument_checks(dev):
    checks.check_c_abi_argument_checks(dev)


def test_zip_members_stored_deflated_picked_and_multi_frame(dev):
    checks.check_members(dev)


def test_zip_frames_that_span_fragments_and_both_kinds_in_one_archive(dev):
    checks.check_spanning(dev)


def test_zip_rescale_dtypes_inversion_and_unused_bits(dev):
    checks.check_rescale_and_dtypes(dev)


def test_zip_main_headers_past_the_head_and_plt(dev):
    checks.check_long_headers(dev)


def test_zip_keyword_crc_and_kind_mixing(dev):
    checks.check_keyword_and_crc(dev)


def test_zip_refusals_equal_load_frames_behind_the_member_label(dev):
    checks.check_refusals_through_the_loader(dev)
