"""JPEG 2000 conformance (tests/dicom_j2k_conformance_checks.py: legal streams OpenJPEG's encoder never writes, from the
test-side writer tests/j2k_writer.py) on the CPU emulator of tests/hipemu -- kernel LOGIC where there is no GPU; the proof on
hardware is tests/test_gpu_dicom_j2k_conformance.py.  ``test_j2k_writer_and_host_parser`` needs no device at all: the writer
against Pillow, the host parser against the writer's record, every structural claim.  Every fixture of the GPU file runs here
as well."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import dicom_j2k_conformance_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


def test_j2k_writer_and_host_parser():
    found = checks.check_writer_and_host_parser()
    print({k: len(v) for k, v in found.items()})


def test_emulated_empty_bands_and_resolutions_without_a_band(emulated):
    checks.check_group(emulated, "a/", checks.claims_a)


def test_emulated_stack_of_level_counts(emulated):
    checks.check_stack_of_level_counts(emulated)


def test_emulated_packet_header_that_ends_in_ff(emulated):
    checks.check_group(emulated, "b/", checks.claims_b)


def test_emulated_lblock_increments_and_a_length_of_more_than_32_bits(emulated):
    checks.check_group(emulated, "c/", checks.claims_c)


def test_emulated_guard_bits_and_exponents(emulated):
    checks.check_group(emulated, "d/", checks.claims_d)


def test_emulated_more_than_30_bit_planes_is_refused_per_frame(emulated):
    checks.check_status_8(emulated)


def test_emulated_blocks_excluded_between_included_ones(emulated):
    checks.check_mixed_inclusion_stack(emulated)


def test_emulated_segment_termination(emulated):
    checks.check_group(emulated, "g/", checks.claims_g)


def test_emulated_precision_and_sign_from_the_writer(emulated):
    checks.check_group(emulated, "h/", checks.claims_h)


def test_emulated_archive_of_every_group(emulated):
    checks.check_archive_of_every_group(emulated)
