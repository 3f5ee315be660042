"""Shared checks of xim.load_frames / xim.decode_xim_batch / pl_xim_decode_batch (tests/test_emulated_xim_batch.py on the CPU
emulator, tests/test_gpu_xim_batch.py on the MI355X).  Every comparison is EQUALITY: the reference is oracle.xim_decode on
each image separately (itself pinned to the reference's reader by tests/test_oracle_golden.py) or the arrays of
tests/golden/xim.npz (decoded by the reference's own reader), followed by numpy's ``astype``.

Shapes stay small (a fiber per work-item on the emulator) and are chosen for the paths of the kernels: a workgroup takes 2048
differences (seams at 2047 / 2048 / 2049 and three chunks), a column-pass band is 64 rows (images of 2 .. 684 rows: one band,
a partial second band, eleven bands), a row is scanned by 256 lanes (widths 1, 41, 300, 683)."""
from __future__ import annotations

import io
import json
import struct

import numpy as np
import pytest
import torch

from oracle import pylinac_oracle as o
from pylinac_amd import xim as px

PROPS = {"PixelWidth": 0.0336, "PixelHeight": 0.0336}
SHORT = "XIM pixel buffer is shorter than its lookup table implies"


def to_np(t: torch.Tensor) -> np.ndarray:
    t = t.cpu()
    if t.dtype == torch.uint16:                       # (torch -> numpy has no uint16 bridge on every version)
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def split(data):
    """a compressed .xim file's bytes -> (w, h, bpp, (lookup offset, length), (pixel-buffer offset, length))"""
    data = bytes(data)
    w, h, _, bpp, comp = struct.unpack_from("<5i", data, 12)
    assert comp == 1
    (nl,) = struct.unpack_from("<i", data, 32)
    (nb,) = struct.unpack_from("<i", data, 36 + nl)
    return w, h, bpp, (36, nl), (36 + nl + 4, nb)


def exact_decode(lut: np.ndarray, stream: np.ndarray, w: int, h: int, bpp: int) -> np.ndarray:
    """oracle.xim_decode's formulation, statement by statement, with every sum over Python integers (object arrays) and ONE
    wrap into the container at the end -- the same ring arithmetic.  It exists for the 8-byte container alone, where
    oracle.xim_decode's ``v & ((1 << 64) - 1)`` is refused by numpy's int64; check_container pins it to oracle.xim_decode on
    the containers the oracle does evaluate."""
    n = w * h - w - 1
    codes = ((lut[:, None] >> np.array([0, 2, 4, 6])[None, :]) & 3).ravel()[:n].astype(np.int64)
    assert not (codes > 2).any()
    sizes = 1 << codes
    offs = (w + 1) * 4 + np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    b = stream.astype(np.int64)
    val = np.zeros(n, np.int64)
    for k in range(4):
        use = sizes > k
        val[use] |= b[offs[use] + k] << (8 * k)
    bits = 8 * sizes
    val = np.where(val >= (1 << (bits - 1)), val - (1 << bits), val)
    a = np.concatenate([stream[: (w + 1) * 4].view("<i4").astype(np.int64), val])
    a = a.astype(o.XIM_DTYPES[bpp]).astype(object).reshape(h, w)
    s_rows = np.cumsum(a[1:], axis=1)
    tot = s_rows[:, -1]
    c = np.concatenate([[-a[0, 0]], -a[0, 0] + np.cumsum(tot[:-1])])
    e = s_rows + c[:, None]
    out = np.vstack([a[0:1], a[0:1] + np.cumsum(e, axis=0)])
    m = 1 << (8 * bpp)
    return ((out + m // 2) % m - m // 2).astype(o.XIM_DTYPES[bpp])


def reference(data) -> np.ndarray:
    """oracle.xim_decode of ONE file (an 8-byte container: exact_decode)"""
    w, h, bpp, (lo, ll), (bo, bl) = split(data)
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    if bpp == 8:
        return exact_decode(raw[lo:lo + ll], raw[bo:bo + bl], w, h, bpp)
    return o.xim_decode(raw[lo:lo + ll], raw[bo:bo + bl], w, h, bpp)


def seeded_image(seed: int, h: int, w: int, noise: float, spikes: int = 0, base: float = 20000.0) -> np.ndarray:
    """a smooth blob + noise (its amplitude decides the mixture of 1- / 2- / 4-byte differences) + a few 2^20 outliers"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = base + 0.4 * base * np.exp(-(((yy - h / 2) / (h / 3 + 1)) ** 2 + ((xx - w / 2) / (w / 3 + 1)) ** 2)) + rng.normal(0, noise, (h, w))
    img = img.round().astype(np.int64)
    if spikes:
        img.ravel()[rng.integers(0, h * w, spikes)] = rng.choice([1 << 20, -(1 << 18)], spikes)
    return img


def xim_file(img: np.ndarray, bpp: int = 4, props=None) -> bytes:
    return o.xim_file_bytes(img, bpp, PROPS if props is None else props, histogram=(1, 2, 3))


def file_from_stream(lut: np.ndarray, stream: np.ndarray, w: int, h: int, bpp: int) -> bytes:
    """oracle.xim_file_bytes' layout around a given lookup table and pixel buffer (no histogram, PROPS)"""
    out = [b"VMS.XI\x00\x00", struct.pack("<6i", 1, w, h, 8 * bpp, bpp, 1), struct.pack("<i", len(lut)), lut.tobytes(),
           struct.pack("<i", len(stream)), stream.tobytes(), struct.pack("<i", w * h * bpp), struct.pack("<i", 0),
           struct.pack("<i", len(PROPS))]
    for name, value in PROPS.items():
        out.append(struct.pack("<i", len(name)) + name.encode() + struct.pack("<id", 1, value))
    return b"".join(out)


def assert_stack(dev, files, dtype=None, want_status=None):
    """load_frames(files, dtype) == [oracle.xim_decode(f).astype(dtype)] and the status words"""
    st = px.load_frames(files, dtype=dtype, device=dev, check=False)
    got = to_np(st.frames)
    want = np.stack([reference(f) for f in files])
    if dtype is not None:
        want = want.astype(dtype)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want)
    status = to_np(st.status)
    assert status.dtype == np.int32 and status.tolist() == (want_status or [0] * len(files))
    return st


# ---- 1
def check_goldens(golden, dev):
    g = golden("xim")
    for name in "abcd":
        f = g[f"{name}.file"].tobytes()
        st = px.load_frames([f, f, f], device=dev)
        want = g[f"{name}.array"]
        got = to_np(st.frames)
        assert got.dtype == want.dtype and got.shape == (3,) + want.shape, name
        for k in range(3):
            assert np.array_equal(got[k], want), (name, k)
        assert to_np(st.status).tolist() == [0, 0, 0]
        props = json.loads(str(g[f"{name}.props"]))
        assert st.dpmm == float(g[f"{name}.dpmm"])
        for x in st.images:
            assert not hasattr(x, "array")
            assert (x.img_height_px, x.img_width_px) == want.shape and x.format_id == "VMS.XI" and x.compression == 1
            assert x.bytes_per_pixel == want.dtype.itemsize and x.bits_per_pixel == 8 * want.dtype.itemsize
            assert x.dpmm == float(g[f"{name}.dpmm"]) and np.array_equal(x.histogram, g[f"{name}.histogram"])
            assert x.lookup_table.dtype == np.uint8 and x.lookup_table.size == (want.size - want.shape[1] - 1 + 3) // 4
            assert set(props) == set(x.properties)
            for k, v in props.items():
                assert np.array_equal(np.asarray(x.properties[k]), np.asarray(v)), k


# ---- 2
MIXED = [(11, 3.0, 0), (12, 60.0, 0), (13, 900.0, 0), (14, 40.0, 40), (15, 20000.0, 150)]     # seed, noise, outliers


def mixed_files():
    return [xim_file(seeded_image(seed, 37, 41, noise, spikes)) for seed, noise, spikes in MIXED]


def check_mixed_streams_kernel_entry(dev):
    files = mixed_files()
    assert len({len(f) for f in files}) == 5                                   # the five pixel buffers differ in length
    rng = np.random.default_rng(5)
    parts, spans, pos = [], [], 0
    for f, junk in zip(files, (0, 1, 2, 3, 5)):                                # a 4-byte boundary, then the junk, then the file
        junk += -pos % 4
        parts.append(rng.integers(0, 256, junk, dtype=np.uint8).tobytes() + f)
        w, h, bpp, (lo, ll), (bo, bl) = split(f)
        spans.append((pos + junk + lo, ll, pos + junk + bo, bl))
        pos += junk + len(f)
    assert {s[2] % 4 for s in spans} == {0, 1, 2, 3}                           # every alignment of a pixel buffer occurs
    lo, ll, bo, bl = (np.array(c, dtype=np.int64) for c in zip(*spans))
    buf = np.frombuffer(b"".join(parts), dtype=np.uint8)
    want = np.stack([reference(f) for f in files])
    for dtype in (None, np.uint16, np.float64):
        frames, status = px.decode_xim_batch(buf, lo, ll, bo, bl, 41, 37, 4, dtype=dtype, device=dev)
        assert frames.shape == (5, 37, 41) and status.dtype == torch.int32
        assert np.array_equal(to_np(frames), want if dtype is None else want.astype(dtype))
        wide = [4 * int(((w_ < 0) | (w_ > 65535)).any()) if dtype is np.uint16 else 0 for w_ in want]
        assert to_np(status).tolist() == wide
    # the lookup table of a 41 x 37 image ends in a byte with fewer than four codes and its last chunk is partial
    assert (41 * 37 - 41 - 1) % 4 != 0 and (41 * 37 - 41 - 1) % 2048 != 0


def check_mixed_streams_loader(dev):
    files = mixed_files()
    whole = to_np(assert_stack(dev, files).frames)
    for k, f in enumerate(files):                                              # the stack == each file alone
        assert np.array_equal(to_np(px.load_frames([f], device=dev).frames)[0], whole[k]), k
    perm = [3, 0, 4, 2, 1]
    assert np.array_equal(to_np(px.load_frames([files[k] for k in perm], device=dev).frames), whole[perm])


# ---- 3
SEAMS = [(64, 33), (683, 4), (50, 42), (64, 80)]       # W * H - W - 1 = 2047, 2048, 2049 and 5055 (three chunks)


def check_chunk_seam(dev, w, h):
    assert (w * h - w - 1) in (2047, 2048, 2049, 5055)
    assert_stack(dev, [xim_file(seeded_image(21, h, w, 50.0, 9)), xim_file(seeded_image(22, h, w, 2500.0, 0))])


# ---- 4
EXTREME = [(7, 2), (1, 5), (300, 3)]                   # one scanned row; three differences after a head of two; a wide row


def check_extreme_shape(dev, w, h):
    assert_stack(dev, [xim_file(seeded_image(31, h, w, 30.0, 1)), xim_file(seeded_image(32, h, w, 3000.0, 0))])


# ---- 5
def check_container(dev, bpp):
    # values around 20000 .. 28000 and 2^20 outliers wrap in int8 / int16 (as golden files c and d do); int64 holds them
    files = [xim_file(seeded_image(40 + bpp, 35, 29, 200.0, 6), bpp), xim_file(seeded_image(50 + bpp, 35, 29, 5.0, 0), bpp)]
    st = assert_stack(dev, files)
    assert st.frames.dtype == {1: torch.int8, 2: torch.int16, 8: torch.int64}[bpp]
    if bpp < 4:
        assert (reference(files[0]).astype(np.int64) != seeded_image(40 + bpp, 35, 29, 200.0, 6)).any()    # it did wrap
    for f in files:                       # exact_decode (the 8-byte reference) == oracle.xim_decode wherever the oracle evaluates
        w, h, _, (lo, ll), (bo, bl) = split(f)
        raw = np.frombuffer(f, dtype=np.uint8)
        for other in (1, 2, 4):
            assert np.array_equal(exact_decode(raw[lo:lo + ll], raw[bo:bo + bl], w, h, other),
                                  o.xim_decode(raw[lo:lo + ll], raw[bo:bo + bl], w, h, other))
    assert_stack(dev, files, np.float64)
    assert_stack(dev, files, np.uint16, [4 * int(((r < 0) | (r > 65535)).any()) for r in map(reference, files)])


# ---- 6
def status_files():
    files = [xim_file(seeded_image(60 + k, 37, 41, 80.0, 3)) for k in range(4)]
    good1 = files[1]
    w, h, bpp, (lo, ll), (bo, bl) = split(good1)
    bad = bytearray(good1)
    bad[lo + 100] = 0xFF                                                       # four size codes 3
    files[1] = bytes(bad)
    # file 2: the pixel buffer ends one byte early and says so; the byte that follows it (the uncompressed-size field, and
    # then file 3) is in the buffer: only the declared length keeps the last difference from being read
    w, h, bpp, (lo, ll), (bo, bl) = split(files[2])
    f2 = bytearray(files[2])
    del f2[bo + bl - 1]
    f2[bo - 4:bo] = struct.pack("<i", bl - 1)
    files[2] = bytes(f2)
    return files, good1


def check_status(dev):
    files, good1 = status_files()
    st = px.load_frames(files, device=dev, check=False)
    assert to_np(st.status).tolist() == [0, 1, 2, 0]
    got = to_np(st.frames)
    assert np.array_equal(got[0], reference(files[0])) and np.array_equal(got[3], reference(files[3]))
    with pytest.raises(KeyError) as e:                                         # file 1 comes first
        px.load_frames(files, device=dev)
    assert e.value.args == (3,)
    with pytest.raises(ValueError, match=SHORT):
        px.load_frames([files[0], good1, files[2], files[3]], device=dev)
    # the per-file path raises the same for each of the two
    with pytest.raises(KeyError):
        px.XIM.from_bytes(files[1], device=dev)
    with pytest.raises(ValueError, match=SHORT):
        px.XIM.from_bytes(files[2], device=dev)


def check_window_outside_the_buffer(dev):
    """kernel entry: a window that does not lie inside the buffer (or is shorter than the shape implies) is flagged, never read"""
    files = [xim_file(seeded_image(70 + k, 37, 41, 80.0, 3)) for k in range(3)]
    buf = np.frombuffer(b"".join(files), dtype=np.uint8)
    spans, pos = [], 0
    for f in files:
        w, h, bpp, (lo, ll), (bo, bl) = split(f)
        spans.append([pos + lo, ll, pos + bo, bl])
        pos += len(f)
    want = [reference(f) for f in files]
    for column, value in ((2, buf.size - 10), (0, -1), (1, 5), (3, 41 * 4), (2, 1 << 40)):
        s = np.array(spans, dtype=np.int64)
        s[1, column] = value
        frames, status = px.decode_xim_batch(buf, s[:, 0], s[:, 1], s[:, 2], s[:, 3], 41, 37, 4, device=dev)
        assert to_np(status).tolist() == [0, 2, 0], (column, value)
        got = to_np(frames)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])


# ---- 7
def int64_image_holding(target: int, w: int, h: int):
    """(lookup table, pixel buffer) of a w x h int64 image whose LAST pixel is ``target``: the decoder's sums are linear in
    the differences -- the difference at (row q >= 1, any column) enters the last pixel 1 + (h - 1 - q) times -- so 4-byte
    differences taken greedily from the largest weight down reach a value no image-space encoder could state."""
    big = (1 << 31) - 1
    diffs = np.zeros(w * h - w - 1, dtype=np.int64)
    rest = target
    for i in range(diffs.size):
        q = (i + w + 1) // w
        d = min(big, rest // (h - q))
        diffs[i] = d
        rest -= d * (h - q)
        if rest == 0:
            break
    assert rest == 0
    lut = np.full((diffs.size + 3) // 4, 0xAA, dtype=np.uint8)                # size code 2 everywhere: 4-byte differences
    stream = np.concatenate([np.zeros(w + 1, "<i4").view(np.uint8), diffs.astype("<i4").view(np.uint8)])
    return lut, stream


def check_float64_beyond_2_53(dev):
    w, h = 300, 170
    lut, stream = int64_image_holding((1 << 53) + 1, w, h)
    want = exact_decode(lut, stream, w, h, 8)
    assert np.array_equal(want.astype(np.int32), o.xim_decode(lut, stream, w, h, 4))       # (the ring's image in int32)
    assert want.dtype == np.int64 and want[-1, -1] == (1 << 53) + 1 and (want > (1 << 53)).sum() >= 1
    f = file_from_stream(lut, stream, w, h, 8)
    st = assert_stack(dev, [f, f], np.float64)
    assert to_np(st.frames)[1, -1, -1] == float(1 << 53)                       # round to nearest even
    assert_stack(dev, [f])


def check_conversions(dev):
    h, w = 37, 41
    inside = [seeded_image(80 + k, h, w, 60.0, 0) for k in range(3)]
    assert all(0 <= im.min() and im.max() <= 65535 for im in inside)
    assert_stack(dev, [xim_file(im) for im in inside], np.uint16)
    assert_stack(dev, [xim_file(im) for im in inside], np.float64)
    both, row0, head = inside[0].copy(), inside[1].copy(), inside[2].copy()
    both[5, 7], both[9, 3] = 70000, -1
    row0[0, 4] = 70000                                                         # row 0 ...
    head[1, 0] = -1                                                            # ... and the last value of the plain head
    files = [xim_file(inside[0]), xim_file(both), xim_file(row0), xim_file(head)]
    st = assert_stack(dev, files, np.uint16, [0, 4, 4, 4])
    got = to_np(st.frames)
    assert got[1, 5, 7] == 70000 - 65536 and got[1, 9, 3] == 65535 and got[2, 0, 4] == 4464 and got[3, 1, 0] == 65535
    with pytest.raises(ValueError, match="file 1.*uint16"):
        px.load_frames(files, dtype=np.uint16, device=dev)
    assert_stack(dev, files, np.float64)
    assert_stack(dev, files)


# ---- 8
def check_validation(golden, dev, tmp_path):
    a = xim_file(seeded_image(90, 37, 41, 60.0))
    for other in (xim_file(seeded_image(91, 37, 40, 60.0)), xim_file(seeded_image(91, 36, 41, 60.0)),
                  xim_file(seeded_image(91, 37, 41, 60.0), 2)):
        with pytest.raises(ValueError, match="file 2 differs"):
            px.load_frames([a, a, other, other], device=dev)
    raw = seeded_image(92, 37, 41, 60.0).astype("<i4")
    plain = b"".join([b"VMS.XI\x00\x00", struct.pack("<6i", 1, 41, 37, 32, 4, 0), struct.pack("<i", raw.nbytes), raw.tobytes(),
                      struct.pack("<ii", 0, 0)])
    with pytest.raises(ValueError, match=r"file 1 is not compressed.*XIM\(path\)"):
        px.load_frames([a, plain], device=dev)
    assert np.array_equal(to_np(px.XIM.from_bytes(plain, device=dev).array), raw)       # ... which XIM reads as before
    odd = bytearray(a)
    odd[24:28] = struct.pack("<i", 3)
    with pytest.raises(ValueError, match="unsupported bytes per pixel"):
        px.load_frames([bytes(odd)], device=dev)
    for bad in (np.float32, np.int32, "nonsense"):
        with pytest.raises(TypeError):
            px.load_frames([a], dtype=bad, device=dev)
    with pytest.raises(ValueError, match="no files"):
        px.load_frames([], device=dev)
    # paths, bytes and file objects are the same source
    path = tmp_path / "a.xim"
    path.write_bytes(a)
    st = px.load_frames([str(path), path, a, io.BytesIO(a), bytearray(a)], device=dev)
    assert np.array_equal(to_np(st.frames), np.stack([reference(a)] * 5))
    assert [x.path for x in st.images] == [str(path), path, None, None, None]
    # a stack whose files disagree in dpmm has no common value
    b = xim_file(seeded_image(90, 37, 41, 60.0), props={"PixelWidth": 0.04, "PixelHeight": 0.04})
    st = px.load_frames([a, b], device=dev)
    assert st.images[0].dpmm == 1 / (10 * 0.0336) and st.images[1].dpmm == 1 / (10 * 0.04)
    with pytest.raises(ValueError, match="dpmm"):
        st.dpmm
    # XIM.from_bytes == XIM(path) on a golden file
    g = golden("xim")
    gp = tmp_path / "g.xim"
    gp.write_bytes(g["a.file"].tobytes())
    one, two = px.XIM(str(gp), device=dev), px.XIM.from_bytes(g["a.file"].tobytes(), device=dev)
    assert np.array_equal(to_np(one.array), g["a.array"]) and np.array_equal(to_np(two.array), g["a.array"])
    assert one.path == str(gp) and two.path is None
    skip = ("path", "array", "_spans")
    assert {k for k in vars(one) if k not in skip} == {k for k in vars(two) if k not in skip}
    for k in vars(one):
        if k in skip:
            continue
        u, v = getattr(one, k), getattr(two, k)
        if k == "properties":
            assert set(u) == set(v) and all(np.array_equal(np.asarray(u[p]), np.asarray(v[p])) for p in u)
        else:
            assert np.array_equal(np.asarray(u), np.asarray(v)), k
    lazy = px.XIM.from_bytes(g["a.file"].tobytes(), read_pixels=False)
    assert not hasattr(lazy, "array") and lazy.dpmm == one.dpmm


def check_c_abi_argument_checks(dev):
    """pl_xim_decode_batch: invalid argument (1) for height < 2, n < 1 and a bad out_kind, unsupported (2) for the bytes per pixel"""
    from pylinac_amd import _lib

    lib = _lib.load()
    buf = torch.zeros(256, dtype=torch.uint8, device=dev)
    idx = torch.zeros(4, dtype=torch.int64, device=dev)
    st = torch.zeros(4, dtype=torch.int32, device=dev)
    p, q, s = buf.data_ptr(), idx.data_ptr(), st.data_ptr()

    def call(n, w, h, bpp, kind):
        return lib.pl_xim_decode_batch(p, 256, q, q, q, q, n, w, h, bpp, kind, p, s, p, None)

    assert call(1, 4, 1, 4, 0) == 1 and call(0, 4, 4, 4, 0) == 1 and call(1, 4, 4, 4, 3) == 1 and call(1, 4, 4, 4, -1) == 1
    assert call(1, 4, 4, 3, 0) == 2 and b"unsupported bytes per pixel" in lib.pl_last_error()
    assert lib.pl_xim_batch_work_bytes(1, 4, 1, 4, 0) == -1 and lib.pl_xim_batch_work_bytes(2, 41, 37, 4, 0) > 0
    # the T-typed plane of a converted stack is part of the work area
    assert (lib.pl_xim_batch_work_bytes(3, 41, 37, 4, 1) - lib.pl_xim_batch_work_bytes(3, 41, 37, 4, 0)) == 3 * 41 * 37 * 4
    with pytest.raises(ValueError, match="unsupported bytes per pixel"):
        px.decode_xim_batch(buf, idx, idx, idx, idx, 4, 4, 3, device=dev)
