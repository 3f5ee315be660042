"""The checked Deflate path (zipstack.adler32, png.inflate(verify=True), png.load_frames(verify=True); pl_adler32 /
pl_inflate_checked / pl_png_decode_checked) on the CPU emulator of tests/hipemu (kernel LOGIC where there is no GPU; the proof
on hardware is tests/test_gpu_verify.py): every case of tests/verify_checks.py."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import verify_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


def test_emulated_adler32_equals_zlib_at_every_length_and_alignment(emulated):
    checks.check_adler_random(emulated)


@pytest.mark.parametrize("value", [0, 0xFF])
def test_emulated_adler32_of_constant_bytes(emulated, value):
    checks.check_adler_constant(emulated, value)


def test_emulated_adler32_at_the_buffers_end_and_outside_it(emulated):
    checks.check_adler_edges(emulated)


def test_emulated_checked_inflate_of_sound_streams_and_trailing_bytes(emulated):
    checks.check_inflate_sound(emulated)


def test_emulated_checked_inflate_flags_a_flipped_trailer(emulated):
    checks.check_inflate_trailer_flipped(emulated)


def test_emulated_checked_inflate_flags_a_flipped_byte_of_a_stored_block(emulated):
    checks.check_inflate_stored_byte_flipped(emulated)


def test_emulated_checked_inflate_flags_a_cut_trailer(emulated):
    checks.check_inflate_trailer_cut(emulated)


def test_emulated_checked_inflate_capacity_below_and_above_the_size(emulated):
    checks.check_inflate_capacity(emulated)


def test_emulated_checked_inflate_one_damaged_stream_among_several(emulated):
    checks.check_inflate_one_damaged_among_several(emulated)


@pytest.mark.parametrize("kind", ["grey16", "rgb8"])
def test_emulated_verified_sound_stack_equals_pil(emulated, kind):
    checks.check_png_sound(emulated, kind)


@pytest.mark.parametrize("kind", ["grey16", "rgb8"])
def test_emulated_damaged_png_files_are_flagged_per_file(emulated, kind):
    checks.check_png_damage(emulated, kind)


def test_emulated_check_raises_naming_the_file_and_the_check(emulated, monkeypatch):
    checks.check_png_raises(emulated, monkeypatch)


def test_emulated_c_abi_argument_checks(emulated):
    checks.check_c_abi_argument_checks(emulated)
