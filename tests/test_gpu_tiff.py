"""Strip TIFFs (tiff.load_frames / decode_tiff_strips / pl_tiff_decode) on the MI355X: every case of tests/tiff_checks.py (the
same ones tests/test_emulated_tiff.py runs on the CPU emulator), a 1024 x 1024 uint16 picket-fence frame as LZW + predictor 2
in 64 KiB strips and as ONE strip (2 MiB of output from one wave), the stack [A, B, A], and the hand-over of a uint16 stack to
picketfence.analyze_batch."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import tiff_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("predictor", [1, 2])
def test_ridge_with_noise_reaches_12_bits_clears_and_kwkwk(dev, predictor):
    checks.check_ridge(dev, predictor)


def test_constant_frame_is_kwkwk_chains_of_long_strings(dev):
    checks.check_constant(dev)


def test_uint8_frame(dev):
    checks.check_uint8(dev)


def test_random_frame_grows_under_lzw(dev):
    checks.check_random(dev)


@pytest.mark.parametrize("rows,cols", checks.SHAPES)
def test_small_and_odd_shapes(dev, rows, cols):
    checks.check_shape(dev, rows, cols)


def test_strip_geometry_and_odd_offsets(dev):
    checks.check_strip_geometry(dev)


def test_big_endian_files(dev):
    checks.check_big_endian(dev)


def test_packbits_strips(dev):
    checks.check_packbits(dev)


def test_rgb_collapses_like_pil_convert_i(dev):
    checks.check_rgb(dev)


def test_mixed_stack(dev):
    checks.check_mixed_stack(dev)


def test_dtype_and_sources(dev, tmp_path):
    checks.check_dtype_and_sources(dev, tmp_path)


def test_dpi_and_dpmm(dev):
    checks.check_dpi(dev)


def test_status_is_per_frame_and_check_raises(dev, monkeypatch):
    checks.check_status(dev, monkeypatch)


def test_window_outside_the_buffer_is_flagged_and_the_frame_untouched(dev):
    checks.check_window_outside_the_buffer(dev)


def test_refusals_and_the_ifd_walk(dev):
    checks.check_refusals(dev)


def test_c_abi_argument_checks(dev):
    checks.check_c_abi_argument_checks(dev)


@pytest.fixture(scope="module")
def film_frames():
    from pylinac_amd.synthetic import pf_frames

    return checks.to_np(pf_frames(2, 1024, 1024, seed0=2600))


def test_detector_size_frame_in_64_kib_strips_and_the_stack_a_b_a(dev, film_frames):
    """two 1024 x 1024 uint16 picket-fence frames as LZW + predictor 2 in PIL's default strips (32 rows = 64 KiB of output),
    encoded once each, as the stack [A, B, A]: exactly what PIL reads"""
    from pylinac_amd import tiff

    files = [checks.pil_file(f, "tiff_lzw", predictor=2) for f in film_frames]
    info = tiff.read_tiff(files[0])
    assert len(info.strips) == 32 and info.strips[0][3] * info.width * 2 == 65536
    order = [0, 1, 0]
    stack = tiff.load_frames([files[k] for k in order], device=dev, check=False)
    assert stack.frames.dtype == torch.uint16 and stack.status.cpu().tolist() == [0, 0, 0]
    assert np.array_equal(checks.to_np(stack.frames), film_frames[order])


def test_detector_size_frame_as_one_strip(dev, film_frames):
    """the same frame as ONE strip: 2 MiB of output, some hundred table epochs, from one wave"""
    from pylinac_amd import tiff

    f = checks.pil_file(film_frames[0], "tiff_lzw", predictor=2, rows_per_strip=1024)
    assert len(tiff.read_tiff(f).strips) == 1
    got, stack = checks.load(dev, [f])
    assert np.array_equal(got[0], film_frames[0])


def test_uint16_stack_goes_into_picketfence_analyze_batch(dev):
    """three seeded 256 x 256 picket-fence frames written as LZW + predictor 2 files: analyze_batch on load_frames(...).frames
    == the same call on the frames uploaded directly, key for key"""
    import dataclasses

    from pylinac_amd import picketfence, tiff
    from pylinac_amd.synthetic import pf_frames

    pixel_mm = 0.390625
    frames = pf_frames(3, 256, 256, seed0=2700, pixel_mm=pixel_mm, pickets=5)
    want_frames = checks.to_np(frames)
    files = [checks.pil_file(f, "tiff_lzw", predictor=2, rows_per_strip=32, dpi=(25.4 / pixel_mm,) * 2) for f in want_frames]
    stack = tiff.load_frames(files, device=dev)
    assert stack.frames.dtype == torch.uint16 and np.array_equal(checks.to_np(stack.frames), want_frames)
    assert abs(stack.dpmm - 1 / pixel_mm) < 1e-6 / pixel_mm                        # (PIL stores a float32 rational)
    got = picketfence.analyze_batch(stack.frames, dpmm=1 / pixel_mm, num_pickets=5)
    want = picketfence.analyze_batch(frames.to(dev), dpmm=1 / pixel_mm, num_pickets=5)
    assert int((want.status == 0).sum()) > 0 and want.picket_count.cpu().tolist() == [5, 5, 5]
    for key in (f.name for f in dataclasses.fields(want)):
        a, b = getattr(got, key), getattr(want, key)
        if isinstance(b, torch.Tensor):
            assert torch.equal(a, b) or np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True), key
        else:
            assert a == b, key
