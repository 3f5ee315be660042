"""JPEG 2000 lossless Pixel Data (dicom.load_frames(jpeg2000=True) / decode_jpeg2000_frames / pl_dicom_j2k_decode) on the
MI355X: every case of tests/dicom_j2k_checks.py (the same ones tests/test_emulated_dicom_j2k.py runs on the CPU emulator).  No
stack is larger than 8 frames of 129 x 67."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import dicom_j2k_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("block", checks.BLOCKS, ids=lambda b: f"cb{b[0]}")
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=lambda d: d.__name__)
@pytest.mark.parametrize("shape", checks.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_geometry(dev, shape, dtype, block):
    checks.check_geometry(dev, shape, dtype, block)


def test_all_five_progression_orders(dev):
    checks.check_progression_orders(dev)


def test_oblong_code_blocks(dev):
    checks.check_oblong_blocks(dev)


def test_psot_zero_and_skipped_segments(dev):
    checks.check_psot_zero_and_skipped_segments(dev)


@pytest.mark.parametrize("kind", checks.CONTENTS)
def test_content(dev, kind):
    checks.check_content(dev, kind)


@pytest.mark.parametrize("signed", [False, True], ids=["unsigned", "signed"])
@pytest.mark.parametrize("precision", checks.PRECISIONS)
def test_precision_and_sign(dev, precision, signed):
    checks.check_precision_sign(dev, precision, signed)


def test_eight_bit_signed_stream(dev):
    checks.check_eight_bit_sign(dev)


def test_uids_tables_fragments_and_stacks(dev, tmp_path):
    checks.check_plumbing(dev, tmp_path)


def test_rescale_dtypes_and_unused_bits_equal_the_native_load(dev):
    checks.check_rescale_and_dtypes(dev)


def test_dicom_image_reads_a_jpeg2000_file(dev):
    checks.check_dicom_image(dev)


def test_refusals_and_malformed_streams(dev):
    checks.check_refusals(dev)


def test_status_is_per_frame(dev):
    checks.check_status(dev)


def test_check_raises_naming_file_and_frame(dev, monkeypatch):
    checks.check_status_through_the_loader(dev, monkeypatch)


def test_c_abi_argument_checks(dev):
    checks.check_c_abi_argument_checks(dev)
