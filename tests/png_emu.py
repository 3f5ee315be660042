"""TEST INFRASTRUCTURE ONLY: csrc/png.hip on the CPU emulator of tests/hipemu.

tests/hipemu/build.py builds the files it lists by name, and png.hip is not among them.  This module compiles png.hip
(with runtime.hip for the error plumbing and the emulator itself) into a library of its own next to the emulated one, with
build.py's own rewriting rules and compiler flags, exactly as tests/tiff_emu.py does for tiff.hip, and `emulated_device()`
here is tests/emu_backend.py's context with `pl_inflate` and the two `pl_png_*` entry points taken from that library and
everything else from the emulated library proper.  Each library carries its own copy of the emulator's state and of
the last error message; `pl_last_error` answers from the library that was called last.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import pathlib
import subprocess
import sys
from unittest import mock

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "hipemu"))

SOURCES = ["png.hip", "runtime.hip"]
OWN = ("pl_png_", "pl_inflate")


def build() -> pathlib.Path:
    import build as emu_build  # tests/hipemu/build.py

    emu_build.build()                                  # the emulated library proper, and the rewritten pl_common.h beside it
    lib = emu_build.BUILD / "libpylinac_emu_png.so"
    csrc, here = emu_build.CSRC, emu_build.HERE
    inputs = [csrc / s for s in SOURCES] + list(csrc.glob("*.h")) + [here / "hipemu.cpp", here / "hip" / "hip_runtime.h",
                                                                     ROOT / "include" / "pylinac_hip.h", emu_build.LIB,
                                                                     pathlib.Path(emu_build.__file__), pathlib.Path(__file__)]
    if lib.exists() and all(lib.stat().st_mtime >= p.stat().st_mtime for p in inputs):
        return lib
    cpps = []
    for s in SOURCES:
        out = emu_build.BUILD / (pathlib.Path(s).stem + "_png_emu.cpp")
        out.write_text(f'#line 1 "{csrc / s}"\n' + emu_build._rewrite((csrc / s).read_text()))
        cpps.append(str(out))
    subprocess.run([emu_build.CXX, "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-ffp-contract=off",
                    "-fno-fast-math", "-Wno-attributes", "-Wno-unknown-pragmas", f"-I{here}", f"-I{emu_build.BUILD}", f"-I{csrc}",
                    *cpps, str(here / "hipemu.cpp"), "-o", str(lib)], check=True)
    return lib


class _TwoLibraries:
    """The emulated library with the Deflate / PNG entry points of the second one."""

    def __init__(self, main, png):
        self._main, self._png, self._last = main, png, main

    def __getattr__(self, name):
        if name == "pl_last_error":
            return self._last.pl_last_error
        owner = self._png if name.startswith(OWN) else self._main
        fn = getattr(owner, name)
        if not name.startswith("pl_"):
            return fn

        def call(*args):
            self._last = owner
            return fn(*args)

        return call


@contextlib.contextmanager
def emulated_device():
    from emu_backend import emulated_device as plain
    from pylinac_amd import _lib as binding

    extra = C.CDLL(str(build()))
    extra.pl_last_error.restype = C.c_char_p
    for name, (argtypes, restype) in binding.SIGNATURES.items():
        if name.startswith(OWN):
            fn = getattr(extra, name)                  # AttributeError here: the entry point is missing from png.hip
            fn.argtypes, fn.restype = argtypes, restype
    with plain() as main:
        both = _TwoLibraries(main, extra)
        with mock.patch.object(binding, "_lib", both):
            yield both
