"""Tier 2 of JPEG 2000 on the device (dicom.plan_jpeg2000_blocks / pl_dicom_j2k_plan) and
dicom.load_zip(encapsulated=True, jpeg2000=True) on the CPU emulator of tests/hipemu (kernel LOGIC where there is no GPU; the
proof on hardware is tests/test_gpu_dicom_zip_j2k.py): every plan-only check of tests/dicom_zip_j2k_checks.py, the refusals
(which decode next to nothing) and, of the whole load, one archive of two small members.
Tier 1 is slow on the emulator; the other loads are left to the GPU file."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import dicom_j2k_checks as jk  # noqa: E402
import dicom_zip_j2k_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


@pytest.mark.parametrize("block", jk.BLOCKS, ids=lambda b: f"cb{b[0]}")
def test_emulated_plan_equals_the_host_parser_on_noise_of_129x67(emulated, block):
    checks.check_plan_geometry(emulated, block)


def test_emulated_plan_equals_the_host_parser_on_small_shapes(emulated):
    checks.check_plan_shapes(emulated)


def test_emulated_plan_equals_the_host_parser_on_oblong_blocks_and_progression_orders(emulated):
    checks.check_plan_oblong_and_orders(emulated)


def test_emulated_plan_equals_the_host_parser_on_constant_low_signed_precinct_and_open_ended_streams(emulated):
    checks.check_plan_contents(emulated)


def test_emulated_plan_streams_use_every_codeword_class_of_table_b4(emulated):
    passes = checks.check_plan_contents(emulated) | checks.check_plan_geometry(emulated, (32, 32))
    checks.check_pass_classes(passes)


def test_emulated_plan_status_is_per_frame(emulated):
    checks.check_plan_status(emulated)


def test_emulated_plan_c_abi_argument_checks(emulated):
    checks.check_c_abi_argument_checks(emulated)


def test_emulated_zip_two_members(emulated):
    checks.check_members(emulated, full=False)


def test_emulated_zip_keyword_crc_and_kind_mixing(emulated):
    checks.check_keyword_and_crc(emulated)


def test_emulated_zip_refusals_equal_load_frames_behind_the_member_label(emulated):
    checks.check_refusals_through_the_loader(emulated)
