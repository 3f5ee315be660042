"""pylinac_amd/_stack_io.pack_files, the packer under xim / tiff / png ``load_frames``, on the CPU (``device="cpu"``, no kernels):
every kind of source, every padding length, the short-read refusal and the empty list."""
from __future__ import annotations

import io
import os
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pylinac_amd import _stack_io  # noqa: E402

PAYLOADS = [bytes(range(10 * k + 1, 10 * k + 2 + k)) for k in range(5)]          # 1, 2, 3, 4 and 5 bytes, none of them 0


def _parse(seen):
    def parse(view, k, what):
        seen.append((bytes(view), k, what))
        return SimpleNamespace(size=len(view))

    return parse


def test_every_source_kind_lands_at_a_4_byte_boundary_with_zero_padding(tmp_path, monkeypatch):
    path = tmp_path / "one.bin"
    path.write_bytes(PAYLOADS[0])
    sources = [path, PAYLOADS[1], bytearray(PAYLOADS[2]), io.BytesIO(PAYLOADS[3]), np.frombuffer(PAYLOADS[4], dtype=np.uint8)]
    empty = torch.empty
    monkeypatch.setattr(_stack_io.torch, "empty", lambda *a, **kw: empty(*a, **kw).fill_(0xFF))
    seen = []
    images, starts, host, dbuf = _stack_io.pack_files(sources, "cpu", _parse(seen))
    assert starts == [0, 4, 8, 12, 16] and all(s % 4 == 0 for s in starts)
    assert host.dtype == torch.uint8 and host.numel() == 24 and not host.is_pinned()
    assert dbuf.dtype == torch.uint8 and dbuf.numel() == 24 and dbuf.device.type == "cpu"
    assert bool((dbuf == 0xFF).all())                                             # nothing is copied by the packer
    got = host.numpy()
    pads = set()
    for k, (st, data) in enumerate(zip(starts, PAYLOADS)):
        end = starts[k + 1] if k + 1 < len(starts) else host.numel()
        assert got[st:st + len(data)].tobytes() == data
        assert not got[st + len(data):end].any()
        pads.add(end - st - len(data))
    assert pads == {0, 1, 2, 3}
    assert seen == [(PAYLOADS[0], 0, f"file 0 ({path})")] + [(PAYLOADS[k], k, f"file {k}") for k in range(1, 5)]
    assert [x.size for x in images] == [1, 2, 3, 4, 5]
    assert [x.path for x in images] == [path, None, None, None, None]
    assert _stack_io.file_name(images, 0) == f"file 0 ({path})" and _stack_io.file_name(images, 3) == "file 3"


def test_a_file_that_shrinks_between_the_size_query_and_the_read_is_an_oserror(tmp_path, monkeypatch):
    path = tmp_path / "short.bin"
    path.write_bytes(PAYLOADS[4])
    size = os.path.getsize
    monkeypatch.setattr(_stack_io.os.path, "getsize", lambda p: size(p) + 1)
    with pytest.raises(OSError) as err:
        _stack_io.pack_files([str(path)], "cpu", _parse([]))
    assert str(err.value) == f"{path}: read 5 of 6 bytes"


def test_no_files_is_a_valueerror():
    with pytest.raises(ValueError) as err:
        _stack_io.pack_files([], "cpu", _parse([]))
    assert str(err.value) == "load_frames: no files"
