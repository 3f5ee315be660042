"""PNG files and Deflate streams (png.load_frames / decode_png_streams / pl_png_decode / pl_inflate) on the MI355X: every case
of tests/png_checks.py (the same ones tests/test_emulated_png.py runs on the CPU emulator), two PIL files of 512 x 512 uint16
noise (9 IDAT chunks each, the 32 KiB ring turning over 16 times), and a 1024 x 1024 uint16 picket-fence file handed to
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

import png_checks as checks  # noqa: E402

pytestmark = pytest.mark.gpu

def test_inflate_fixtures_cover_every_branch_the_issue_names():
    checks.check_inflate_coverage()


@pytest.mark.parametrize("name", sorted(checks.inflate_fixtures()))
def test_inflate_equals_zlib_wrapped_and_raw(dev, name):
    checks.check_inflate_fixture(dev, name)


def test_inflate_eight_streams_at_odd_offsets_and_capacities(dev):
    checks.check_inflate_eight_streams(dev)


def test_inflate_status_bits(dev):
    checks.check_inflate_status(dev)


@pytest.mark.parametrize("rows,cols", checks.SHAPES)
def test_filters_on_every_row_and_mixed(dev, rows, cols):
    checks.check_filters(dev, rows, cols)


def test_paeth_ties(dev):
    checks.check_paeth_ties(dev)


@pytest.mark.parametrize("kind", ["ridge", "constant", "noise"])
def test_pil_files_at_levels_0_1_6_9(dev, kind):
    checks.check_pil_files(dev, kind)


def test_idat_seams_inside_a_code_and_inside_len(dev):
    checks.check_idat_seams(dev)


def test_mixed_stack(dev):
    checks.check_mixed_stack(dev)


def test_dtype_out_and_sources(dev, tmp_path):
    checks.check_dtype_and_sources(dev, tmp_path)


def test_dpi_dpmm_and_ancillary_chunks(dev):
    checks.check_dpi_and_chunks(dev)


def test_status_is_per_frame_and_check_raises(dev, monkeypatch):
    checks.check_status(dev, monkeypatch)


def test_segment_outside_the_buffer_is_flagged_and_the_frame_untouched(dev):
    checks.check_window_outside_the_buffer(dev)


def test_refusals_and_the_chunk_walk(dev):
    checks.check_refusals(dev)


def test_c_abi_argument_checks(dev):
    checks.check_c_abi_argument_checks(dev)


def test_two_files_of_512_x_512_noise_nine_idats_each(dev):
    """two PIL files of 512 x 512 uint16 noise: zlib stores it (stored blocks of 64 KiB - 1 crossing the 64 KiB IDAT chunks), 512
    KiB + 512 of output per stream = sixteen turns of the 32 KiB ring"""
    from pylinac_amd import png

    rng = np.random.default_rng(2600)
    frames = rng.integers(0, 65536, (2, 512, 512)).astype(np.uint16)
    files = [checks.pil_file(f) for f in frames]
    assert [len(png.read_png(f).idat) for f in files] == [9, 9]
    stack = png.load_frames(files, device=dev, check=False)
    assert stack.frames.dtype == torch.uint16 and stack.status.cpu().tolist() == [0, 0]
    assert np.array_equal(checks.to_np(stack.frames), frames)


def test_detector_size_file_goes_into_picketfence_analyze_batch(dev):
    """one 1024 x 1024 uint16 picket-fence frame written by PIL: analyze_batch on load_frames(...).frames == the same call on the
    frame uploaded directly, key for key"""
    import dataclasses

    from pylinac_amd import picketfence, png
    from pylinac_amd.synthetic import pf_frames

    pixel_mm = 0.390625
    frames = pf_frames(1, 1024, 1024, seed0=2700, pixel_mm=pixel_mm, pickets=10)
    want_frames = checks.to_np(frames)
    files = [checks.pil_file(f, dpi=(25.4 / pixel_mm,) * 2) for f in want_frames]
    stack = png.load_frames(files, device=dev)
    assert stack.frames.dtype == torch.uint16 and np.array_equal(checks.to_np(stack.frames), want_frames)
    assert abs(stack.dpmm - 1 / pixel_mm) < 1e-3 / pixel_mm                        # (pHYs holds whole pixels per metre)
    got = picketfence.analyze_batch(stack.frames, dpmm=1 / pixel_mm, num_pickets=10)
    want = picketfence.analyze_batch(frames.to(dev), dpmm=1 / pixel_mm, num_pickets=10)
    assert int((want.status == 0).sum()) > 0 and want.picket_count.cpu().tolist() == [10]
    for key in (f.name for f in dataclasses.fields(want)):
        a, b = getattr(got, key), getattr(want, key)
        if isinstance(b, torch.Tensor):
            assert torch.equal(a, b) or np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True), key
        else:
            assert a == b, key
