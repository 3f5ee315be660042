"""The checked Deflate path (zipstack.adler32, png.inflate(verify=True), png.load_frames(verify=True); pl_adler32 /
pl_inflate_checked / pl_png_decode_checked) on the MI355X: every case of tests/verify_checks.py (the same ones
tests/test_emulated_verify.py runs on the CPU emulator)."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import verify_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


def test_adler32_equals_zlib_at_every_length_and_alignment(dev):
    checks.check_adler_random(dev)


@pytest.mark.parametrize("value", [0, 0xFF])
def test_adler32_of_constant_bytes(dev, value):
    checks.check_adler_constant(dev, value)


def test_adler32_at_the_buffers_end_and_outside_it(dev):
    checks.check_adler_edges(dev)


def test_checked_inflate_of_sound_streams_and_trailing_bytes(dev):
    checks.check_inflate_sound(dev)


def test_checked_inflate_flags_a_flipped_trailer(dev):
    checks.check_inflate_trailer_flipped(dev)


def test_checked_inflate_flags_a_flipped_byte_of_a_stored_block(dev):
    checks.check_inflate_stored_byte_flipped(dev)


def test_checked_inflate_flags_a_cut_trailer(dev):
    checks.check_inflate_trailer_cut(dev)


def test_checked_inflate_capacity_below_and_above_the_size(dev):
    checks.check_inflate_capacity(dev)


def test_checked_inflate_one_damaged_stream_among_several(dev):
    checks.check_inflate_one_damaged_among_several(dev)


@pytest.mark.parametrize("kind", ["grey16", "rgb8"])
def test_verified_sound_stack_equals_pil(dev, kind):
    checks.check_png_sound(dev, kind)


@pytest.mark.parametrize("kind", ["grey16", "rgb8"])
def test_damaged_png_files_are_flagged_per_file(dev, kind):
    checks.check_png_damage(dev, kind)


def test_check_raises_naming_the_file_and_the_check(dev, monkeypatch):
    checks.check_png_raises(dev, monkeypatch)


def test_c_abi_argument_checks(dev):
    checks.check_c_abi_argument_checks(dev)
