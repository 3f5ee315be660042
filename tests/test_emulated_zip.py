"""ZIP archives and CRC-32 (zipstack.crc32 / extract / read_zip, dicom.load_zip, pl_crc32 / pl_zip_extract) on the CPU emulator
of tests/hipemu (kernel LOGIC where there is no GPU; the proof on hardware is tests/test_gpu_zip.py): every case of
tests/zip_checks.py.  The emulator runs a fiber per work-item, so a member's output stays below about 100 KiB here; the
64-member volume and the 1024 x 1024 stored member run on the GPU only."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import zip_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


def test_emulated_crc32_equals_zlib_at_every_length_and_alignment(emulated):
    checks.check_crc_random(emulated)


@pytest.mark.parametrize("value", [0, 0xFF])
def test_emulated_crc32_of_constant_bytes(emulated, value):
    checks.check_crc_constant(emulated, value)


def test_emulated_crc32_at_the_buffers_end_and_outside_it(emulated):
    checks.check_crc_edges(emulated)


def test_emulated_archives_equal_zipfile_read(emulated):
    checks.check_archive_kinds(emulated)


def test_emulated_nine_members_at_every_residue_mod_16(emulated, tmp_path):
    checks.check_nine_members_every_residue(emulated, tmp_path)


def test_emulated_damage_is_flagged_per_member(emulated, monkeypatch):
    checks.check_damage(emulated, monkeypatch)


def test_emulated_refusals_of_read_zip(emulated):
    checks.check_refusals(emulated)


def test_emulated_load_zip_native_files_mixed_methods_and_subsets(emulated):
    checks.check_load_zip_native(emulated)


def test_emulated_load_zip_rescale_and_multi_frame(emulated):
    checks.check_load_zip_rescale(emulated)


def test_emulated_load_zip_header_longer_than_the_first_prefix(emulated):
    checks.check_load_zip_long_header(emulated)


def test_emulated_load_zip_refusals_and_verify(emulated):
    checks.check_load_zip_refusals(emulated)


def test_emulated_c_abi_argument_checks(emulated):
    checks.check_c_abi_argument_checks(emulated)
