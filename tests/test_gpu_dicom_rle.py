"""RLE Lossless Pixel Data (dicom.load_frames / decode_rle_frames / pl_dicom_rle_decode) on the MI355X: every case of
tests/dicom_rle_checks.py (the same ones tests/test_emulated_dicom_rle.py runs on the CPU emulator), three 1024 x 1024 uint16
frames -- more than 1000 chunks per segment, so pass 2 stages its table in several batches -- and the hand-over of a uint16
stack to winston_lutz.analyze_batch."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import dicom_rle_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


def test_every_entry_offset_of_a_chunk_occurs_and_decodes(dev):
    checks.check_every_entry_offset(dev)


@pytest.mark.parametrize("name", checks.SEAMS)
def test_chunk_seams(dev, name):
    checks.check_chunk_seam(dev, name)


def test_constant_plane_expands_64_times_the_chunk(dev):
    checks.check_constant_plane(dev)


def test_noise_plane_is_all_literals(dev):
    checks.check_noise_plane(dev)


@pytest.mark.parametrize("rows,cols", checks.SHAPES)
def test_small_and_odd_shapes(dev, rows, cols):
    checks.check_small_shape(dev, rows, cols)


def test_no_ops_runs_across_rows_and_the_pad_byte(dev):
    checks.check_encoder_options(dev)


@pytest.mark.parametrize("dtype", checks.CONTAINERS, ids=lambda d: d.__name__)
def test_containers_at_every_alignment_through_the_kernel_entry(dev, dtype):
    checks.check_container_kernel_entry(dev, dtype)


@pytest.mark.parametrize("dtype", checks.CONTAINERS, ids=lambda d: d.__name__)
def test_containers_through_the_loader(dev, dtype):
    checks.check_container_loader(dev, dtype)


@pytest.mark.parametrize("name", ["u16_explicit", "u16_explicit_shifted", "u16_sequence", "i16_ct", "u16_stored12_dirty",
                                  "i16_stored12_dirty", "u8_multiframe", "u8_odd", "i8", "u32", "u16_inverted_sign", "u16_epid_tags"])
def test_loader_keywords_equal_the_native_load(golden, dev, name):
    checks.check_loader_fixture(golden, dev, name)


def test_loader_rescale_of_a_series_and_file_by_file(golden, dev):
    checks.check_loader_rescale_per_file(golden, dev)


def test_multiframe_offset_tables_stacks_and_sources(golden, dev, tmp_path):
    checks.check_loader_multiframe_and_stacks(golden, dev, tmp_path)


def test_dicom_image_reads_an_rle_file(golden, dev):
    checks.check_dicom_image(golden, dev)


def test_status_is_per_frame_and_check_raises_or_warns_like_pydicom(dev):
    checks.check_status(dev)


def test_window_outside_the_buffer_is_flagged_and_the_frame_untouched(dev):
    checks.check_window_outside_the_buffer(dev)


def test_malformed_headers_other_syntaxes_and_mixtures_are_refused(golden, dev):
    checks.check_malformed_and_refused(golden, dev)


def test_c_abi_argument_checks(dev):
    checks.check_c_abi_argument_checks(dev)


def test_detector_size_stack_of_three(dev):
    """two 1024 x 1024 uint16 Winston-Lutz frames with dark-current noise (the low-byte plane barely compresses), encoded once
    each, as the stack [A, B, A]: exactly the source frames"""
    from pylinac_amd import dicom
    from pylinac_amd.synthetic import wl_frames

    frames = wl_frames(2, 1024, 1024, seed0=3200, noise_sigma=0.002)
    files = [checks.rle_file(f[None]) for f in frames]
    for f, data in zip(frames, files):
        (off, ln), = dicom.read_part10(data)[0].PixelDataFragments
        so, sl = checks.segment_table(data, [(off, ln)], 2)
        assert int(sl.max()) > 1000 * checks.K                                     # more than 1000 chunks in a segment
    order = [0, 1, 0]
    x, _ = dicom.load_frames([files[k] for k in order], device=dev, check=False)
    assert x.dtype == torch.uint16 and x._pl_status.cpu().tolist() == [0, 0, 0]
    assert np.array_equal(checks.to_np(x), frames[order])


def test_uint16_stack_goes_into_winston_lutz_analyze_batch(dev):
    """three seeded 256 x 256 Winston-Lutz frames written as RLE Lossless files: analyze_batch on load_frames(...) == the same
    call on the frames uploaded directly"""
    from pylinac_amd import dicom, winston_lutz
    from pylinac_amd.synthetic import wl_frames

    pixel_mm = 0.336
    frames = wl_frames(3, 256, 256, seed0=3100, pixel_mm=pixel_mm)
    x, _ = dicom.load_frames([checks.rle_file(f[None]) for f in frames], device=dev)
    assert x.dtype == torch.uint16 and np.array_equal(checks.to_np(x), frames)
    got = winston_lutz.analyze_batch(x, dpmm=1 / pixel_mm)
    want = winston_lutz.analyze_batch(torch.from_numpy(frames).to(dev), dpmm=1 / pixel_mm)
    assert np.isfinite(want["record"]).all() and (want["status"] == 0).all()
    for key in ("record", "status", "inverted", "crop"):
        assert np.array_equal(got[key], want[key]), key
