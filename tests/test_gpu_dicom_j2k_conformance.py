"""JPEG 2000 conformance on the MI355X: every case of tests/dicom_j2k_conformance_checks.py -- legal streams OpenJPEG's encoder
never writes, from the test-side writer tests/j2k_writer.py, through load_frames, plan_jpeg2000_blocks and load_zip.  No frame
is larger than 33 x 65 (64 x 64 for the one-block fixtures of group g); the pure-Python encode of all fixtures takes a few
seconds and is shared by the tests of a process."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import dicom_j2k_conformance_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


def test_writer_pillow_and_host_parser_agree_before_the_device_runs(dev):
    checks.check_writer_and_host_parser()


def test_empty_bands_and_resolutions_without_a_band(dev):
    checks.check_group(dev, "a/", checks.claims_a)


def test_stack_of_level_counts(dev):
    checks.check_stack_of_level_counts(dev)


def test_packet_header_that_ends_in_ff(dev):
    checks.check_group(dev, "b/", checks.claims_b)


def test_lblock_increments_and_a_length_of_more_than_32_bits(dev):
    checks.check_group(dev, "c/", checks.claims_c)


def test_guard_bits_and_exponents(dev):
    checks.check_group(dev, "d/", checks.claims_d)


def test_more_than_30_bit_planes_is_refused_per_frame(dev):
    checks.check_status_8(dev)


def test_blocks_excluded_between_included_ones(dev):
    checks.check_mixed_inclusion_stack(dev)


def test_segment_termination(dev):
    checks.check_group(dev, "g/", checks.claims_g)


def test_precision_and_sign_from_the_writer(dev):
    checks.check_group(dev, "h/", checks.claims_h)


def test_archive_of_every_group(dev):
    checks.check_archive_of_every_group(dev)
