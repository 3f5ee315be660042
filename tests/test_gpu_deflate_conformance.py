"""inflate_kernel on legal Deflate streams that zlib's encoder never writes (matches beyond distance 32 506 whose source and
target share ring slots, hand-written dynamic code sets, flushed streams, seeded random dynamic blocks) on the MI355X: every
case of tests/deflate_conformance_checks.py (the same ones tests/test_emulated_deflate_conformance.py runs on the CPU
emulator)."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import deflate_conformance_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


def test_matches_that_alias_in_the_ring_equal_zlib(dev):
    checks.check_ring_alias(dev)


def test_out_cap_inside_an_aliasing_match(dev):
    checks.check_ring_alias_capacity(dev)


def test_hand_written_code_sets_equal_zlib(dev):
    checks.check_code_sets(dev)


def test_code_sets_zlib_refuses_are_status_4(dev):
    checks.check_refused_sets(dev)


def test_end_of_block_only_set_is_accepted_as_zlib_does(dev):
    checks.check_eob_only_block(dev)


def test_sync_and_full_flushed_streams_equal_zlib(dev):
    checks.check_flushed_streams(dev)


def test_random_dynamic_blocks_equal_zlib(dev):
    checks.check_random_blocks(dev)


def test_random_dynamic_blocks_checked_equal_zlib(dev):
    checks.check_random_blocks_checked(dev)


def test_png_with_aliasing_matches_equals_pil(dev):
    checks.check_png_file(dev)


def test_tiff_strip_with_aliasing_matches_equals_pil(dev):
    checks.check_tiff_file(dev)


def test_zip_member_with_aliasing_matches_equals_zipfile(dev):
    checks.check_zip_member(dev)
