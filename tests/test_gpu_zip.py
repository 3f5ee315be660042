"""ZIP archives and CRC-32 (zipstack.crc32 / extract / read_zip, dicom.load_zip, pl_crc32 / pl_zip_extract) on the MI355X: every
case of tests/zip_checks.py (the same ones tests/test_emulated_zip.py runs on the CPU emulator), a 64-member archive of
512 x 512 int16 slices (32 CRC tiles of pixels, 33 with the header, and 16 turns of the inflate ring per member) and one stored 1024 x 1024 uint16 member."""
from __future__ import annotations

import io
import sys
import zipfile
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import zip_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


def test_crc32_equals_zlib_at_every_length_and_alignment(dev):
    checks.check_crc_random(dev)


@pytest.mark.parametrize("value", [0, 0xFF])
def test_crc32_of_constant_bytes(dev, value):
    checks.check_crc_constant(dev, value)


def test_crc32_at_the_buffers_end_and_outside_it(dev):
    checks.check_crc_edges(dev)


def test_archives_equal_zipfile_read(dev):
    checks.check_archive_kinds(dev)


def test_nine_members_at_every_residue_mod_16(dev, tmp_path):
    checks.check_nine_members_every_residue(dev, tmp_path)


def test_damage_is_flagged_per_member(dev, monkeypatch):
    checks.check_damage(dev, monkeypatch)


def test_refusals_of_read_zip(dev):
    checks.check_refusals(dev)


def test_load_zip_native_files_mixed_methods_and_subsets(dev):
    checks.check_load_zip_native(dev)


def test_load_zip_rescale_and_multi_frame(dev):
    checks.check_load_zip_rescale(dev)


def test_load_zip_header_longer_than_the_first_prefix(dev):
    checks.check_load_zip_long_header(dev)


def test_load_zip_refusals_and_verify(dev):
    checks.check_load_zip_refusals(dev)


def test_c_abi_argument_checks(dev):
    checks.check_c_abi_argument_checks(dev)


def test_volume_of_64_deflated_slices_of_512_x_512(dev):
    """64 members of 512 x 512 int16, level 6, noise in the low byte: 512 KiB of pixels per member = 32 CRC tiles (33 with the
    data set's header) and sixteen turns of the 32 KiB inflate ring; equal to the frames written"""
    from pylinac_amd import dicom, zipstack

    rng = np.random.default_rng(2800)
    yy, xx = np.mgrid[0:512, 0:512]
    base = (-1000 + 1900 * np.exp(-((yy - 256) ** 2 + (xx - 250) ** 2) / 30000.0)).astype(np.int16) & ~np.int16(255)
    frames = (base[None] + rng.integers(0, 256, (64, 512, 512))).astype(np.int16)
    data = checks.dicom_zip([(f"CT{k:03d}.dcm", checks.rle.native_file(frames[k:k + 1])) for k in range(64)])
    members = zipstack.read_zip(data)
    assert len(members) == 64 and all(m.method == 8 and m.compressed_size < m.size for m in members)
    assert all(-(-m.size // checks.TILE) == 33 for m in members)
    x, metas, names = dicom.load_zip(data, device=dev)
    assert x.dtype == torch.int16 and len(names) == 64 and np.array_equal(checks.to_np(x), frames)


def test_one_stored_member_of_1024_x_1024_verified(dev):
    from pylinac_amd import dicom, zipstack

    rng = np.random.default_rng(2801)
    frame = rng.integers(0, 65536, (1, 1024, 1024)).astype(np.uint16)
    data = checks.dicom_zip([("epid.dcm", checks.rle.native_file(frame))], kinds=[zipfile.ZIP_STORED])
    stack = zipstack.extract(data, device=dev, check=False)
    assert stack.status.cpu().tolist() == [0] and stack.members[0].method == 0
    with zipfile.ZipFile(io.BytesIO(data)) as zf:
        assert checks.to_np(stack.member(0)).tobytes() == zf.read("epid.dcm")
    x, _, _ = dicom.load_zip(data, device=dev)
    assert np.array_equal(checks.to_np(x), frame)
    m = stack.members[0]
    bad = checks.patched(data, m.data_offset + m.size // 2, "<B", data[m.data_offset + m.size // 2] ^ 0x80)
    with pytest.raises(zipfile.BadZipFile, match="Bad CRC-32 for file 'epid.dcm'"):
        dicom.load_zip(bad, device=dev)
