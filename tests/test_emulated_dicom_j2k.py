"""JPEG 2000 lossless Pixel Data (dicom.load_frames(jpeg2000=True) / decode_jpeg2000_frames / pl_dicom_j2k_decode) on the CPU
emulator of tests/hipemu (kernel LOGIC where there is no GPU; the proof on hardware is tests/test_gpu_dicom_j2k.py): every case
of tests/dicom_j2k_checks.py, but of the nine 16-bit noise streams of 129 x 67 only one.  The emulator runs a fiber per
work-item and a wave exchange per decoded symbol: such a frame takes eight seconds here, and its 8-bit form and the 16-bit
frames of 64 x 64 and 33 x 65 walk the same paths (several blocks per band, every bit plane)."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import dicom_j2k_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


GEOMETRY = [(s, d, b) for s in checks.SHAPES for d in (np.uint8, np.uint16) for b in checks.BLOCKS if (s, d) != ((129, 67), np.uint16)]


@pytest.mark.parametrize("shape,dtype,block", GEOMETRY, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v.__name__)
def test_emulated_geometry(emulated, shape, dtype, block):
    checks.check_geometry(emulated, shape, dtype, block)


def test_emulated_geometry_of_the_largest_frame_at_16_bits(emulated):
    """one of the nine streams the list above leaves to the GPU: two levels, 32 x 32 blocks, up to 3 x 2 blocks in a band (a
    tag tree of more than one level) with every bit plane of 16 coded"""
    checks.check_geometry(emulated, (129, 67), np.uint16, (32, 32), only=[2])


def test_emulated_all_five_progression_orders(emulated):
    checks.check_progression_orders(emulated)


def test_emulated_oblong_code_blocks(emulated):
    checks.check_oblong_blocks(emulated)


def test_emulated_psot_zero_and_skipped_segments(emulated):
    checks.check_psot_zero_and_skipped_segments(emulated)


@pytest.mark.parametrize("kind", checks.CONTENTS)
def test_emulated_content(emulated, kind):
    checks.check_content(emulated, kind)


@pytest.mark.parametrize("signed", [False, True], ids=["unsigned", "signed"])
@pytest.mark.parametrize("precision", checks.PRECISIONS)
def test_emulated_precision_and_sign(emulated, precision, signed):
    checks.check_precision_sign(emulated, precision, signed)


def test_emulated_eight_bit_signed_stream(emulated):
    checks.check_eight_bit_sign(emulated)


def test_emulated_uids_tables_fragments_and_stacks(emulated, tmp_path):
    checks.check_plumbing(emulated, tmp_path)


def test_emulated_rescale_dtypes_and_unused_bits_equal_the_native_load(emulated):
    checks.check_rescale_and_dtypes(emulated)


def test_emulated_dicom_image_reads_a_jpeg2000_file(emulated):
    checks.check_dicom_image(emulated)


def test_emulated_refusals_and_malformed_streams(emulated):
    checks.check_refusals(emulated)


def test_emulated_status_is_per_frame(emulated):
    checks.check_status(emulated)


def test_emulated_check_raises_naming_file_and_frame(emulated, monkeypatch):
    checks.check_status_through_the_loader(emulated, monkeypatch)


def test_emulated_c_abi_argument_checks(emulated):
    checks.check_c_abi_argument_checks(emulated)
