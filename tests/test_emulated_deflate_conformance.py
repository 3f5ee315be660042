"""inflate_kernel on legal Deflate streams that zlib's encoder never writes (matches beyond distance 32 506 whose source and
target share ring slots, hand-written dynamic code sets, flushed streams, seeded random dynamic blocks) on the CPU emulator of
tests/hipemu (kernel LOGIC where there is no GPU -- the emulator does not model implicit lock-step, so a copy that relies on
it fails here; the proof on hardware is tests/test_gpu_deflate_conformance.py): every case of
tests/deflate_conformance_checks.py."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import deflate_conformance_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


def test_fixtures_hold_the_branches_they_are_named_for():
    checks.check_ring_alias_fixtures()
    checks.check_code_set_fixtures()
    checks.random_streams()


def test_emulated_matches_that_alias_in_the_ring_equal_zlib(emulated):
    checks.check_ring_alias(emulated)


def test_emulated_out_cap_inside_an_aliasing_match(emulated):
    checks.check_ring_alias_capacity(emulated)


def test_emulated_hand_written_code_sets_equal_zlib(emulated):
    checks.check_code_sets(emulated)


def test_emulated_code_sets_zlib_refuses_are_status_4(emulated):
    checks.check_refused_sets(emulated)


def test_emulated_end_of_block_only_set_is_accepted_as_zlib_does(emulated):
    checks.check_eob_only_block(emulated)


def test_emulated_sync_and_full_flushed_streams_equal_zlib(emulated):
    checks.check_flushed_streams(emulated)


def test_emulated_random_dynamic_blocks_equal_zlib(emulated):
    checks.check_random_blocks(emulated)


def test_emulated_random_dynamic_blocks_checked_equal_zlib(emulated):
    checks.check_random_blocks_checked(emulated)


def test_emulated_png_with_aliasing_matches_equals_pil(emulated):
    checks.check_png_file(emulated)


def test_emulated_tiff_strip_with_aliasing_matches_equals_pil(emulated):
    checks.check_tiff_file(emulated)


def test_emulated_zip_member_with_aliasing_matches_equals_zipfile(emulated):
    checks.check_zip_member(emulated)
