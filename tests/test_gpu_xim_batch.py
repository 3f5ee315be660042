"""xim.load_frames / xim.decode_xim_batch / pl_xim_decode_batch on the MI355X: the cases of tests/xim_batch_checks.py (the
same ones tests/test_emulated_xim_batch.py runs on the CPU emulator), a stack at detector size -- more than 256 chunks per
image, every band of the column pass -- and the hand-over of a uint16 stack to winston_lutz.analyze_batch."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import xim_batch_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


def test_golden_files_three_times_each_with_their_headers(golden, dev):
    checks.check_goldens(golden, dev)


def test_mixed_streams_at_every_alignment_through_the_kernel_entry(dev):
    checks.check_mixed_streams_kernel_entry(dev)


def test_stack_equals_each_file_alone_and_a_permuted_stack(dev):
    checks.check_mixed_streams_loader(dev)


@pytest.mark.parametrize("w,h", checks.SEAMS)
def test_chunk_seams(dev, w, h):
    checks.check_chunk_seam(dev, w, h)


@pytest.mark.parametrize("w,h", checks.EXTREME)
def test_extreme_shapes(dev, w, h):
    checks.check_extreme_shape(dev, w, h)


@pytest.mark.parametrize("bpp", (1, 2, 8))
def test_container_types_wrap_like_the_oracle(dev, bpp):
    checks.check_container(dev, bpp)


def test_status_is_per_image_and_check_raises_for_the_first_flagged_file(dev):
    checks.check_status(dev)


def test_window_outside_the_buffer_is_flagged_and_never_read(dev):
    checks.check_window_outside_the_buffer(dev)


def test_uint16_and_float64_are_numpy_astype_with_the_overflow_flag(dev):
    checks.check_conversions(dev)


def test_float64_of_an_int64_image_holding_2_53_plus_1(dev):
    checks.check_float64_beyond_2_53(dev)


def test_validation_sources_and_from_bytes(golden, dev, tmp_path):
    checks.check_validation(golden, dev, tmp_path)


def test_c_abi_argument_checks(dev):
    checks.check_c_abi_argument_checks(dev)


def test_detector_size_stack_of_three(dev):
    """two 1280 x 1280 int32 images built like the one of test_xim_reader_vs_reference_reader (other seeds, a few 2^21
    outliers: 4-byte differences), encoded once each, as the stack [A, B, A]: the container dtype and uint16"""
    from oracle import pylinac_oracle as o
    from pylinac_amd import xim as px

    imgs, files = [], []
    yy, xx = np.mgrid[0:1280, 0:1280]
    for seed in (7, 8):
        rng = np.random.default_rng(seed)
        img = (30000 + 20000 * np.sin(yy / (90.0 + seed)) * np.cos(xx / (140.0 - seed)) + rng.normal(0, 50, (1280, 1280))).round().astype(np.int64)
        img.ravel()[rng.integers(0, img.size, 50)] = 1 << 21
        imgs.append(img)
        files.append(o.xim_file_bytes(img, 4, checks.PROPS))
    order = [0, 1, 0]
    want = np.stack([imgs[k] for k in order])
    st = px.load_frames([files[k] for k in order], device=dev)
    assert np.array_equal(checks.to_np(st.frames), want.astype(np.int32)) and checks.to_np(st.status).tolist() == [0, 0, 0]
    st = px.load_frames([files[k] for k in order], dtype=np.uint16, device=dev, check=False)
    assert np.array_equal(checks.to_np(st.frames), want.astype(np.uint16)) and checks.to_np(st.status).tolist() == [4, 4, 4]
    with pytest.raises(ValueError, match="file 0.*uint16"):
        px.load_frames([files[k] for k in order], dtype=np.uint16, device=dev)


def test_uint16_stack_goes_into_winston_lutz_analyze_batch(dev):
    """three seeded 256 x 256 Winston-Lutz frames written as .xim: analyze_batch on load_frames(..., np.uint16).frames with
    the stack's dpmm == analyze_batch on the frames uploaded directly"""
    from oracle import pylinac_oracle as o
    from pylinac_amd import winston_lutz
    from pylinac_amd import xim as px
    from pylinac_amd.synthetic import wl_frames

    pixel_mm = 0.336
    frames = wl_frames(3, 256, 256, seed0=3100, pixel_mm=pixel_mm)
    files = [o.xim_file_bytes(f.astype(np.int64), 4, {"PixelWidth": pixel_mm / 10, "PixelHeight": pixel_mm / 10}) for f in frames]
    st = px.load_frames(files, dtype=np.uint16, device=dev)
    assert st.frames.dtype == torch.uint16 and np.array_equal(checks.to_np(st.frames), frames)
    assert st.dpmm == 1 / (10 * (pixel_mm / 10))
    got = winston_lutz.analyze_batch(st.frames, dpmm=st.dpmm)
    direct = torch.from_numpy(frames).to(dev)
    want = winston_lutz.analyze_batch(direct, dpmm=st.dpmm)
    assert np.isfinite(want["record"]).all() and (want["status"] == 0).all()
    for key in ("record", "status", "inverted", "crop"):
        assert np.array_equal(got[key], want[key]), key
