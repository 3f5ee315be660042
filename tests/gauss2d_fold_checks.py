"""Checks of gauss2d_mm (csrc/gaussian_mm.hip: both axes of scipy's Gaussian on 16-bit frames in one launch, on the matrix
cores) where its vector work was cut: the carry chain of uint16 frames runs without the constant 32896 and the stores add it
back as packed 16-bit halves, a pass makes ONE undecided test for all of its tiles, and row groups inside the frame load
through the scalar offset.  Shared by tests/test_gpu_gauss2d_fold.py (MI355X) and tests/test_emulated_gauss2d_fold.py (the CPU
emulator of tests/hipemu).

The reference everywhere is scipy.ndimage.gaussian_filter on the integer frame, compared with array_equal.

Shapes (CASES; uint16 unless said), every one at sigma 5 (radius 20, the EPID step's), the first also at sigma 1 (radius 4) and
sigma 6 (radius 24, the largest the kernel covers): other host constants.
    2 x  64 x  64   the smallest frame covered: the prologue mixes reflected row groups and inner ones, waves have spare tiles
    2 x  80 x  66   w % 4 == 2 (a column quad across the right edge), a ragged strip, a partial last step with masked rows
    1 x 144 x 272   two strips, the second 16 columns wide
    1 x 272 x  96   two row segments: the second starts at r_begin > 0, its "rows above" are real rows
    1 x  96 x 128   int16

Contents of every case (frame()): seeded full-range noise; a block of 40 rows x 70 columns (cut at the frame's edge) of 40000
-- a constant neighbourhood has S within 1e-11 of an integer: the undecided tiers, whole constant tiles and single outputs;
a 48 x 48 block of the smallest value and one of the largest: outputs exactly 0 and 65535, where floor(S) - 32896 sits at
the two ends of its 16-bit range and a packed add that carried between halves, or wrapped, would show; eight isolated pixels
of the smallest / largest value in the noise.  The blocks are written after the 40000 block and win where a small frame
makes them overlap.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

# (n, h, w), dtype, sigmas
CASES = {
    "2x64x64": ((2, 64, 64), np.uint16, (5, 1, 6)),
    "2x80x66": ((2, 80, 66), np.uint16, (5,)),
    "1x144x272": ((1, 144, 272), np.uint16, (5,)),
    "1x272x96": ((1, 272, 96), np.uint16, (5,)),
    "1x96x128_int16": ((1, 96, 128), np.int16, (5,)),
}
HOST_SIGMAS = (0.9, 1, 1.5, 2, 2.5, 3, 3.3, 4, 4.5, 5, 5.5, 6)

# gaussian_mm.hip's two predicates have C++ linkage (they are not part of the C ABI): their Itanium names
_COVERS = "_Z20pl_gauss_mm2d_coversPKvS0_iii"
_TAPS = "_Z26pl_gauss_mm2d_taps_coveredPKdi"

_frames: dict = {}
_wants: dict = {}


def frame(case):
    """the case's input, built once and never written again"""
    if case not in _frames:
        (n, h, w), dt, _ = CASES[case]
        rng = np.random.default_rng(sorted(CASES).index(case) + 20)
        a = rng.integers(0, 65536, (n, h, w))
        a[-1, h - 40:, : min(70, w)] = 40000
        a[0, :48, :48] = 0
        a[-1, :48, w - 48:] = 65535
        free = np.ones((n, h, w), bool)
        free[-1, h - 40:, : min(70, w)] = free[0, :48, :48] = free[-1, :48, w - 48:] = False
        spots = np.flatnonzero(free)
        a.ravel()[rng.choice(spots, 8, replace=False)] = [0, 65535] * 4
        a = (a - (32768 if dt == np.int16 else 0)).astype(dt)
        a.setflags(write=False)
        _frames[case] = a
    return _frames[case]


def weights(sigma):
    """scipy's taps (ndimage._filters._gaussian_kernel1d, order 0) and radius"""
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return np.ascontiguousarray(phi / phi.sum()), radius


def want(case, sigma):
    from scipy import ndimage

    if (case, sigma) not in _wants:
        ref = np.stack([ndimage.gaussian_filter(f, sigma) for f in frame(case)])
        ref.setflags(write=False)
        _wants[(case, sigma)] = ref
    return _wants[(case, sigma)]


def _library():
    from pylinac_amd import _lib

    return _lib.load()


def _predicate(name, argtypes):
    fn = getattr(_library(), name)       # AttributeError: the library does not have gaussian_mm.hip's predicate
    fn.argtypes, fn.restype = argtypes, C.c_int
    return fn


def taps_covered(wts, radius):
    wts = np.ascontiguousarray(wts, dtype=np.float64)
    return _predicate(_TAPS, [C.c_void_p, C.c_int])(wts.ctypes.data, radius)


def check_case(dev, case, sigma):
    import torch

    from pylinac_amd import ops

    a, ref = frame(case), want(case, sigma)
    lo, hi = np.iinfo(a.dtype).min, np.iinfo(a.dtype).max
    assert (ref == lo).any() and (ref == hi).any(), "the blocks must give outputs at both ends of the range"
    wts, radius = weights(sigma)
    x = torch.from_numpy(a.copy()).to(dev)
    out = torch.full_like(x, 12345)
    n, h, w = a.shape
    assert _predicate(_COVERS, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int])(x.data_ptr(), out.data_ptr(), h, w, radius) == 1
    assert taps_covered(wts, radius) == 1, sigma
    ops.gaussian_filter(x, sigma, out=out)
    got = out.cpu().numpy()
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f"{case} sigma {sigma}: {len(bad)} outputs differ, first at {bad[0].tolist()}: " \
                          f"{got[tuple(bad[0])]} for {ref[tuple(bad[0])]}"
    assert np.array_equal(x.cpu().numpy(), a), "the input was written"


def check_host_taps(dev):
    """mm_make_params on the host: scipy's taps of every sigma from 0.9 to 6 are taken (and the smallest frame then comes out
    as scipy's); taps scaled by 1 + 2^-20 -- their sum is no longer 1 to 2^-33, so 32896 * sum(wq) + M does not split into
    32896 * 2^40 and a 32-bit rest, nor is the error bound below M -- are refused, and pl_gaussian2d then gives what scipy gives
    for those taps through its two passes."""
    import torch
    from scipy import ndimage

    from pylinac_amd import _lib, ops

    a = frame("2x64x64")[:1]
    x = torch.from_numpy(a.copy()).to(dev)
    for sigma in HOST_SIGMAS:
        wts, radius = weights(sigma)
        assert taps_covered(wts, radius) == 1, sigma
        got = ops.gaussian_filter(x, sigma).cpu().numpy()
        assert np.array_equal(got, ndimage.gaussian_filter(a[0], sigma)[None]), sigma
    wts, radius = weights(5)
    scaled = np.ascontiguousarray(wts * (1.0 + 2.0 ** -20))
    assert taps_covered(scaled, radius) == 0
    ref = ndimage.correlate1d(ndimage.correlate1d(a[0], scaled, axis=0), scaled, axis=1)
    out, tmp = torch.empty_like(x), torch.empty_like(x)
    d_w = torch.from_numpy(scaled).to(dev)
    lib = _lib.load()
    rc = lib.pl_gaussian2d(x.data_ptr(), out.data_ptr(), tmp.data_ptr(), _lib.PL_U16, 1, a.shape[1], a.shape[2], d_w.data_ptr(),
                           scaled.ctypes.data, radius, None)
    assert rc == 0, lib.pl_last_error().decode()
    assert np.array_equal(out.cpu().numpy()[0], ref)
