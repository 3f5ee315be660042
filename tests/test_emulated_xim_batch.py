"""xim.load_frames / xim.decode_xim_batch / pl_xim_decode_batch on the CPU emulator of tests/hipemu (kernel LOGIC where there
is no GPU; the proof on hardware is tests/test_gpu_xim_batch.py): the cases of tests/xim_batch_checks.py.  The emulator runs a
fiber per work-item, so the detector-size stack and the hand-over to an analyzer run on the GPU only."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import xim_batch_checks as checks  # noqa: E402


@pytest.fixture(scope="module")
def emulated():
    from emu_backend import emulated_device

    with emulated_device():
        yield torch.device("cuda:0")


def test_emulated_golden_files_three_times_each_with_their_headers(golden, emulated):
    checks.check_goldens(golden, emulated)


def test_emulated_mixed_streams_at_every_alignment_through_the_kernel_entry(emulated):
    checks.check_mixed_streams_kernel_entry(emulated)


def test_emulated_stack_equals_each_file_alone_and_a_permuted_stack(emulated):
    checks.check_mixed_streams_loader(emulated)


@pytest.mark.parametrize("w,h", checks.SEAMS)
def test_emulated_chunk_seams(emulated, w, h):
    checks.check_chunk_seam(emulated, w, h)


@pytest.mark.parametrize("w,h", checks.EXTREME)
def test_emulated_extreme_shapes(emulated, w, h):
    checks.check_extreme_shape(emulated, w, h)


@pytest.mark.parametrize("bpp", (1, 2, 8))
def test_emulated_container_types_wrap_like_the_oracle(emulated, bpp):
    checks.check_container(emulated, bpp)


def test_emulated_status_is_per_image_and_check_raises_for_the_first_flagged_file(emulated):
    checks.check_status(emulated)


def test_emulated_window_outside_the_buffer_is_flagged_and_never_read(emulated):
    checks.check_window_outside_the_buffer(emulated)


def test_emulated_uint16_and_float64_are_numpy_astype_with_the_overflow_flag(emulated):
    checks.check_conversions(emulated)


def test_emulated_float64_of_an_int64_image_holding_2_53_plus_1(emulated):
    checks.check_float64_beyond_2_53(emulated)


def test_emulated_validation_sources_and_from_bytes(golden, emulated, tmp_path):
    checks.check_validation(golden, emulated, tmp_path)


def test_emulated_c_abi_argument_checks(emulated):
    checks.check_c_abi_argument_checks(emulated)
