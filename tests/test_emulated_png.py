"""PNG files and Deflate streams (png.load_frames / decode_png_streams / pl_png_decode / pl_inflate) on the CPU emulator of
tests/hipemu (kernel LOGIC where there is no GPU; the proof on hardware is tests/test_gpu_png.py): every case of
tests/png_checks.py.  The emulator runs a fiber per work-item, so a file's output stays below about 100 KiB here; the
512 x 512 and 1024 x 1024 frames and the hand-over to an analyzer run on the GPU only."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import png_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


def test_inflate_fixtures_cover_every_branch_the_issue_names():
    checks.check_inflate_coverage()


@pytest.mark.parametrize("name", sorted(checks.inflate_fixtures()))
def test_emulated_inflate_equals_zlib_wrapped_and_raw(emulated, name):
    checks.check_inflate_fixture(emulated, name)


def test_emulated_inflate_eight_streams_at_odd_offsets_and_capacities(emulated):
    checks.check_inflate_eight_streams(emulated)


def test_emulated_inflate_status_bits(emulated):
    checks.check_inflate_status(emulated)


@pytest.mark.parametrize("rows,cols", checks.SHAPES)
def test_emulated_filters_on_every_row_and_mixed(emulated, rows, cols):
    checks.check_filters(emulated, rows, cols)


def test_emulated_paeth_ties(emulated):
    checks.check_paeth_ties(emulated)


@pytest.mark.parametrize("kind", ["ridge", "constant", "noise"])
def test_emulated_pil_files_at_levels_0_1_6_9(emulated, kind):
    checks.check_pil_files(emulated, kind)


def test_emulated_idat_seams_inside_a_code_and_inside_len(emulated):
    checks.check_idat_seams(emulated)


def test_emulated_mixed_stack(emulated):
    checks.check_mixed_stack(emulated)


def test_emulated_dtype_out_and_sources(emulated, tmp_path):
    checks.check_dtype_and_sources(emulated, tmp_path)


def test_emulated_dpi_dpmm_and_ancillary_chunks(emulated):
    checks.check_dpi_and_chunks(emulated)


def test_emulated_status_is_per_frame_and_check_raises(emulated, monkeypatch):
    checks.check_status(emulated, monkeypatch)


def test_emulated_segment_outside_the_buffer_is_flagged_and_the_frame_untouched(emulated):
    checks.check_window_outside_the_buffer(emulated)


def test_emulated_refusals_and_the_chunk_walk(emulated):
    checks.check_refusals(emulated)


def test_emulated_c_abi_argument_checks(emulated):
    checks.check_c_abi_argument_checks(emulated)
