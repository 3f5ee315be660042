"""Shared checks of inflate_kernel (pylinac_amd/csrc/png.hip) on legal Deflate streams that zlib's ENCODER never writes, but
libdeflate, zopfli, 7-Zip, miniz, Java and Go do: tests/test_emulated_deflate_conformance.py on the CPU emulator,
tests/test_gpu_deflate_conformance.py on the MI355X.  The reference is zlib's DECODER: ``zlib.decompressobj(-15)`` for raw
streams, ``verify_checks.zlib_verdict`` for wrapped ones.  Before the device is asked anything every sound fixture must
decompress there to the expected bytes and every corrupt one must raise.  All comparisons are byte equality and exact status
words; there is no tolerance anywhere.

The streams come from ``dynamic_block`` (a dynamic-Huffman block from code lengths and tokens, its length sequence either one
symbol a length or any list of 16 / 17 / 18 operations, ``rle_ops`` coding the literal and distance lengths as ONE sequence),
and from ``png_checks.fixed_block`` / ``stored_block``.  ``png_checks.inflate_trace`` proves, on the CPU, that the branch a
case is named for occurs in its fixture.  A match with distance + length > 32768 ("ring alias") reads slots of the 32 KiB
ring that the same match writes: zlib's encoder stops at distance 32 506."""
from __future__ import annotations

import io
import struct
import zipfile
import zlib

import numpy as np
import pytest

import png_checks as pc
import tiff_deflate_checks as tdc
import zip_checks as zc
from png_checks import BitWriter, fixed_block, inflate_trace, run_inflate, stored_block, wrap
from pylinac_amd import png
from verify_checks import run_checked, zlib_verdict

RING = 32768
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LENS = [4] * 13 + [5] * 6                                                       # a complete set over all 19 symbols
CL_EXTRA = {16: 2, 17: 3, 18: 7}
GAPS = [1, 2, 3, 31, 63, 64, 65, 127, 129, 255, 257]                               # 32768 - distance


# ---- the reference ----------------------------------------------------------------------------------------------------------
def zraw(raw: bytes) -> bytes:
    """zlib's verdict on a RAW stream: its output; the stream must end where the bytes end"""
    d = zlib.decompressobj(-15)
    out = d.decompress(raw)
    assert d.eof and not d.unused_data
    return out


def zlib_refuses(raw: bytes):
    with pytest.raises(zlib.error):
        zlib.decompressobj(-15).decompress(raw)
    with pytest.raises(ValueError):
        inflate_trace(raw)


# ---- a dynamic-block writer (test files only) ---------------------------------------------------------------------------------
def canonical(lens) -> dict:
    """symbol -> (code, length): RFC 1951's assignment, also for an incomplete set"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def expand(ops) -> list:
    out = []
    for sym, extra in ops:
        if sym < 16:
            out.append(sym)
        elif sym == 16:
            out += [out[-1]] * (3 + extra)
        else:
            out += [0] * ((3 if sym == 17 else 11) + extra)
    return out


def rle_ops(seq) -> list:
    """the code-length operations of a length sequence, runs coded greedily with 16 / 17 / 18.  Given the literal/length
    lengths followed by the distance lengths, runs cross the HLIT boundary wherever the values allow (libdeflate does that;
    zlib's encoder sends the two sets one after the other)"""
    ops, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                n = min(run, 138)
                ops.append((18, n - 11))
                run -= n
            if run >= 3:
                ops.append((17, run - 3))
                run = 0
            ops += [(0, 0)] * run
        else:
            ops.append((v, 0))
            run -= 1
            while run >= 3:
                n = min(run, 6)
                ops.append((16, n - 3))
                run -= n
            ops += [(v, 0)] * run
        i = j
    assert expand(ops) == list(seq)
    return ops


def _length_symbol(length: int):
    k = max(i for i, b in enumerate(pc._LEN_BASE) if b <= length) if length < 258 else 28
    return 257 + k, length - pc._LEN_BASE[k]


def _distance_symbol(dist: int):
    d = max(i for i, b in enumerate(pc._DIST_BASE) if b <= dist)
    return d, dist - pc._DIST_BASE[d]


def dynamic_block(lit_lens, dist_lens, tokens, final: bool = True, w: BitWriter | None = None, cl_ops=None, hlit: int | None = None,
                  hdist: int | None = None) -> BitWriter:
    """a dynamic-Huffman block.  ``lit_lens`` / ``dist_lens``: code lengths by symbol (a list, or {symbol: length}); the codes
    are the canonical ones.  HLIT / HDIST: the smallest that hold the coded symbols unless given.  The 19 code-length lengths
    are CL_LENS (HCLEN = 19).  ``cl_ops``: the length sequence as (16 | 17 | 18 | length, extra) operations over the literal
    lengths followed by the distance lengths (None: one symbol per length).  Tokens as in ``png_checks.fixed_block`` -- an int
    is a literal, (length, distance) a match, ("sym", s) a raw literal/length symbol, ("dsym", s) a raw distance symbol --
    plus ("lsym", sym, extra, dsym, dextra): a raw length symbol and a raw distance symbol with chosen extra bits, and
    ("code", value, n): n raw bits written as a Huffman code (a code no symbol has)"""
    def listed(lens, least, most):
        if isinstance(lens, dict):
            lens = [lens.get(s, 0) for s in range(max(lens) + 1)] if lens else []
        lens = list(lens)
        while len(lens) > least and lens[-1] == 0:
            lens.pop()
        return lens + [0] * (least - len(lens))

    lit = listed(lit_lens, 257, 286)
    dist = listed(dist_lens, 1, 30)
    lit += [0] * ((hlit or 0) - len(lit))
    dist += [0] * ((hdist or 0) - len(dist))
    assert 257 <= len(lit) <= 286 and 1 <= len(dist) <= 30 and (hlit in (None, len(lit))) and (hdist in (None, len(dist)))
    seq = lit + dist
    cl_ops = [(l, 0) for l in seq] if cl_ops is None else list(cl_ops)
    assert expand(cl_ops) == seq
    w = w or BitWriter()
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(len(lit) - 257, 5), w.bits(len(dist) - 1, 5), w.bits(15, 4)
    for s in CL_ORDER:
        w.bits(CL_LENS[s], 3)
    clc = canonical(CL_LENS)
    for sym, extra in cl_ops:
        w.code(*clc[sym])
        if sym >= 16:
            w.bits(extra, CL_EXTRA[sym])
    litc, distc = canonical(lit), canonical(dist)
    for t in tokens:
        if isinstance(t, int):
            w.code(*litc[t])
        elif t[0] == "sym":
            w.code(*litc[t[1]])
        elif t[0] == "dsym":
            w.code(*distc[t[1]])
        elif t[0] == "code":
            w.code(t[1], t[2])
        else:
            if t[0] == "lsym":
                _, sym, extra, dsym, dextra = t
            else:
                (sym, extra), (dsym, dextra) = _length_symbol(t[0]), _distance_symbol(t[1])
            w.code(*litc[sym])
            w.bits(extra, pc._LEN_EXTRA[sym - 257])
            w.code(*distc[dsym])
            w.bits(dextra, pc._DIST_EXTRA[dsym])
    w.code(*litc[256])
    return w


def noise(seed: int, n: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def good_neighbour():
    return pc.inflate_fixtures()["text_fixed"]


# ---- 1: matches whose source and target share ring slots --------------------------------------------------------------------
_ALIAS = None


def alias_streams():
    """name -> (raw stream, zlib's output, trace); built once"""
    global _ALIAS
    if _ALIAS is not None:
        return _ALIAS
    out = {}
    for g in GAPS:                                                                 # 33 000 random bytes, then the three matches
        d = RING - g
        w = stored_block(noise(100 + g, 33000), final=False)
        out[f"gap {g}"] = fixed_block([(258, d), (258, d), (max(3, g + 1), d), 7], w=w).done()
    # the same distances with length <= 32768 - distance: no slot is read and written by one match
    w = stored_block(noise(99, 33000), final=False)
    out["controls"] = fixed_block([t for g in GAPS if g >= 3 for t in ((min(g, 258), RING - g), g & 255)], w=w).done()
    # the literals through the fixed codes instead of a stored block
    out["fixed literals"] = fixed_block(list(noise(98, 33000)) + [(258, RING - 1), (258, RING - 64), (3, RING - 2)]).done()
    # a match that begins 100 bytes before a 4 KiB flush boundary (36 864), and one 1 byte before it
    w = stored_block(noise(97, 36764), final=False)
    out["flush boundary"] = fixed_block([(258, RING - 1), 5] + [(258, RING - 65)] * 15 + [(66, RING - 3), (258, RING - 31)], w=w).done()
    # the TARGET straddles the ring's wrap (output position 32 668: slots 32 668 .. 32 767, 0 .. 157) ...
    w = stored_block(noise(96, 32668), final=False)
    out["target wraps"] = fixed_block([(258, 32668), (200, RING - 129)], w=w).done()
    # ... and the SOURCE does (output position 65 179, distance 32 511: slots 32 668 .. 32 767, 0 .. 157)
    w = stored_block(noise(95, 65179), final=False)
    out["source wraps"] = fixed_block([(258, 32511)], w=w).done()
    done = {}
    for name, raw in out.items():
        want = zraw(raw)                                                           # the oracle validates the fixture
        got, tr = inflate_trace(raw)
        assert got == want and len(want) <= 65536, name
        done[name] = (raw, want, tr)
    _ALIAS = done
    return done


def check_ring_alias_fixtures():
    """the coverage conditions, through inflate_trace: nothing is asked of the device"""
    fx = alias_streams()
    for g in GAPS:
        tr = fx[f"gap {g}"][2]
        assert tr["alias"] == [(g, 258, 33000), (g, 258, 33258), (g, max(3, g + 1), 33516)] and tr["ring_alias"] == 3, g
    tr = fx["controls"][2]
    assert tr["ring_alias"] == 0 and tr["max_dist"] == RING - 3 and tr["dist_syms"] == {29}
    assert fx["fixed literals"][2]["types"] == {1} and fx["fixed literals"][2]["ring_alias"] == 3
    at = [a for _, _, a in fx["flush boundary"][2]["alias"]]
    assert at[0] == 36864 - 100 and 36864 + 4096 - 1 in at and all(a // 4096 < (a + 258) // 4096 for a in (at[0], 40959))
    assert fx["target wraps"][2]["alias"][0] == (100, 258, 32668) and fx["target wraps"][2]["ring_alias"] == 2
    g, n, a = fx["source wraps"][2]["alias"][0]
    assert (g, n, a) == (257, 258, 65179) and (a - (RING - g)) % RING == 32668 and a + n <= 65536
    seen = {g for _, _, tr in fx.values() for g, _, _ in tr["alias"]}
    assert set(GAPS) <= seen
    return fx


def check_ring_alias(dev):
    fx = check_ring_alias_fixtures()
    good_raw, good = good_neighbour()
    names = list(fx)
    raws = [good_raw] + [fx[n][0] for n in names] + [good_raw]
    wants = [good] + [fx[n][1] for n in names] + [good]
    # raw streams, plain mode, one launch, odd offsets
    got, status = run_inflate(dev, raws, [len(x) for x in wants], False, shift=1)
    assert status == [0] * len(raws), dict(zip(["good"] + names + ["good"], status))
    for n, g, want in zip(["good"] + names + ["good"], got, wants):
        assert g == want, (n, first_difference(g, want))
    # wrapped, checked mode, three foreign bytes behind every stream
    streams = [wrap(r, x) for r, x in zip(raws, wants)]
    for s, x in zip(streams, wants):
        assert zlib_verdict(s + b"xyz") == (x, len(s))
    got, status, used = run_checked(dev, [s + b"xyz" for s in streams], [len(x) for x in wants], shift=3)
    assert status == [0] * len(raws), dict(zip(["good"] + names + ["good"], status))
    assert used == [len(s) for s in streams]
    for n, g, want in zip(["good"] + names + ["good"], got, wants):
        assert g == want, (n, first_difference(g, want))


def first_difference(a: bytes, b: bytes):
    if len(a) != len(b):
        return ("lengths", len(a), len(b))
    x = np.flatnonzero(np.frombuffer(a, dtype=np.uint8) != np.frombuffer(b, dtype=np.uint8))
    return ("first byte", int(x[0]), "differing", int(x.size)) if x.size else None


def check_ring_alias_capacity(dev):
    """out_cap cut inside an aliasing match (the first one, the second one, the short one): the stored prefix is zlib's"""
    fx = check_ring_alias_fixtures()
    cases = [("gap 1", 33000 + 100), ("gap 1", 33258 + 77), ("gap 64", 33516 + 64), ("gap 257", 33000 + 257), ("source wraps", 65179 + 101)]
    raws = [fx[n][0] for n, _ in cases]
    wants = [fx[n][1] for n, _ in cases]
    caps = [c for _, c in cases]
    assert all(c < len(x) for c, x in zip(caps, wants))
    got, status, _ = run_checked(dev, [wrap(r, x) for r, x in zip(raws, wants)], caps)
    assert status == [png.INFLATE_OVERFLOW] * len(cases), status
    for (n, c), g, x in zip(cases, got, wants):
        assert len(g) == c and g == x[:c], (n, c, first_difference(g, x[:c]))
    got, status = run_inflate(dev, raws, caps, False)                              # plain mode: complete at out_cap
    assert status == [0] * len(cases), status
    for (n, c), g, x in zip(cases, got, wants):
        assert g == x[:c], (n, c, first_difference(g, x[:c]))


# ---- 2: code sets -----------------------------------------------------------------------------------------------------------
def chain(n: int) -> list:
    """n code lengths 1, 2, ..., n - 1, n - 1: complete, the longest code n - 1 bits"""
    return list(range(1, n)) + [n - 1]


_SETS = None


def code_set_streams():
    """name -> (raw stream, zlib's output, trace)"""
    global _SETS
    if _SETS is not None:
        return _SETS
    text = list(b"leaf 17 of bank B: 0.18 mm; ")
    out = {}
    small = {65: 2, 66: 2, 67: 3, 68: 3, 256: 3, 257: 3}                           # complete: 2/4 + 4/8
    # no distance code at all: HDIST = 1, its one length 0
    out["no distance code"] = dynamic_block(small, [0], [65, 66, 67, 68, 65, 65, 66]).done()
    # ONE distance code of one bit, at symbol 0 (distance 1) and at symbol 5 (distances 7, 8)
    lits = {65: 2, 66: 2, 67: 3, 256: 3, 257: 3, 270: 4, 285: 4}
    out["one distance code at symbol 0"] = dynamic_block(lits, [1], [65, 66, ("lsym", 257, 0, 0, 0), 67, ("lsym", 285, 0, 0, 0),
                                                                    ("lsym", 270, 1, 0, 0)]).done()
    out["one distance code at symbol 5"] = dynamic_block(lits, [0, 0, 0, 0, 0, 1], [65, 66, 67, 66, 65, 67, 67, 66, ("lsym", 257, 0, 5, 0),
                                                                                   ("lsym", 270, 0, 5, 1), ("lsym", 285, 0, 5, 1), 65]).done()
    # codes of 13, 14 and 15 bits in both sets: the canonical walk past the 12-bit and the 8-bit primary tables
    order = [256, 32, 257, 97, 258, 101, 264, 102, 265, 108, 284, 111, 49, 285, 55, 48]   # 1 .. 15, 15 bits in this order
    deep = dict(zip(order, chain(16)))
    lit_tokens = [s for s in order if s < 256]
    len_syms = [s for s in order if s > 256]
    assert len(len_syms) >= 3 and max(deep.values()) == 15
    ddeep = dict(zip([3, 0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], chain(16)))
    toks = lit_tokens * 3
    for k, ds in enumerate(sorted(ddeep, key=ddeep.get)):
        ls = len_syms[k % len(len_syms)]
        toks += [("lsym", ls, (1 << pc._LEN_EXTRA[ls - 257]) - 1 if k & 1 else 0, ds, (1 << pc._DIST_EXTRA[ds]) - 1 if k & 2 else 0),
                 lit_tokens[-1 - k % 3]]
    out["codes of 15 bits"] = dynamic_block(deep, ddeep, toks).done()
    # symbol 284 with extra bits 31: length 258 the long way
    out["284 + 31"] = dynamic_block({65: 2, 66: 2, 256: 2, 284: 2}, [1, 1], [65, 66, 66, 65, ("lsym", 284, 31, 1, 0), 66,
                                                                            ("lsym", 284, 31, 0, 0), ("lsym", 284, 30, 1, 0)]).done()
    # HLIT = 286 and HDIST = 30, every symbol coded
    full = [8] * 226 + [9] * 60
    dfull = [4, 4] + [5] * 28
    toks = text * 4 + [(258, 100), (3, 1), (130, 57), 0, 255, (17, 112), ("lsym", 285, 0, 29, 0)]
    out["HLIT 286 / HDIST 30"] = dynamic_block(full, dfull, toks[:-1], hlit=286, hdist=30).done()
    # repeats that begin in the literal/length lengths and end in the distance lengths
    four = {s: 4 for s in list(b"abcdefghijkl") + [256, 257, 258, 259]}
    seq = [four.get(s, 0) for s in range(260)] + [4] * 16
    out["16 across HLIT"] = dynamic_block(four, [4] * 16, list(b"abcabcl") + [(4, 3), (5, 7), (3, 1)], cl_ops=rle_ops(seq)).done()
    one = {65: 1, 256: 2, 257: 2}
    seq = [one.get(s, 0) for s in range(260)] + [0, 0, 0, 1]
    out["17 across HLIT"] = dynamic_block(one, [0, 0, 0, 1], [65, 65, 65, 65, 65, ("lsym", 257, 0, 3, 0)], cl_ops=rle_ops(seq), hlit=260).done()
    seq = [one.get(s, 0) for s in range(270)] + [0, 0, 0, 0, 0, 1]
    out["18 across HLIT"] = dynamic_block(one, [0, 0, 0, 0, 0, 1], [65] * 9 + [("lsym", 257, 0, 5, 1)], cl_ops=rle_ops(seq), hlit=270).done()
    done = {}
    for name, raw in out.items():
        want = zraw(raw)
        got, tr = inflate_trace(raw)
        assert got == want and tr["types"] == {2}, name
        done[name] = (raw, want, tr)
    _SETS = done
    return done


def check_code_set_fixtures():
    fx = code_set_streams()
    tr = {n: t for n, (_, _, t) in fx.items()}
    assert tr["no distance code"]["dist_codes"] == [0] and tr["no distance code"]["headers"] == [(258, 1)]
    assert tr["one distance code at symbol 0"]["dist_codes"] == [1] and tr["one distance code at symbol 0"]["dist_syms"] == {0}
    assert tr["one distance code at symbol 5"]["dist_codes"] == [1] and tr["one distance code at symbol 5"]["dist_syms"] == {5}
    assert tr["one distance code at symbol 5"]["max_dist_code"] == 1
    t = tr["codes of 15 bits"]
    assert t["max_lit_code"] == 15 and t["max_dist_code"] == 15 and len(t["dist_syms"]) == 16
    assert sorted({e - s for s, e in t["codes"]})[-3:] == [13, 14, 15]
    assert tr["284 + 31"]["len_syms"] == {284} and tr["284 + 31"]["len258"] == 2 and len(fx["284 + 31"][1]) == 4 + 258 + 1 + 258 + 257
    assert tr["HLIT 286 / HDIST 30"]["headers"] == [(286, 30)] and tr["HLIT 286 / HDIST 30"]["dist_codes"] == [30]
    for s in (16, 17, 18):
        assert tr[f"{s} across HLIT"]["cl_cross"] == {s}, s
    assert not any(t["cl_cross"] for n, t in tr.items() if "across" not in n)
    return fx


def check_code_sets(dev):
    fx = check_code_set_fixtures()
    good_raw, good = good_neighbour()
    names = list(fx)
    raws = [good_raw] + [fx[n][0] for n in names] + [good_raw]
    wants = [good] + [fx[n][1] for n in names] + [good]
    got, status = run_inflate(dev, raws, [len(x) for x in wants], False, shift=3)
    assert status == [0] * len(raws), dict(zip(["good"] + names + ["good"], status))
    for n, g, want in zip(["good"] + names + ["good"], got, wants):
        assert g == want, (n, first_difference(g, want))
    streams = [wrap(r, x) for r, x in zip(raws, wants)]
    for s, x in zip(streams, wants):
        assert zlib_verdict(s + b"xyz") == (x, len(s))
    got, status, used = run_checked(dev, [s + b"xyz" for s in streams], [len(x) for x in wants], shift=1)
    assert status == [0] * len(raws) and used == [len(s) for s in streams], dict(zip(["good"] + names + ["good"], status))
    for n, g, want in zip(["good"] + names + ["good"], got, wants):
        assert g == want, (n, first_difference(g, want))


def refused_sets():
    """name -> raw stream; zlib refuses every one ("invalid distance code", "invalid distances set", "invalid literal/lengths
    set"), and the kernel's word for each is status 4"""
    lits = {65: 2, 66: 2, 67: 3, 256: 3, 257: 3, 270: 4, 285: 4}
    pad = b"\0" * 8
    return {
        "the unused code of a one-code distance set": dynamic_block(lits, [1], [65, 66, ("sym", 257), ("code", 1, 1)]).done() + pad,
        "a length symbol without distance codes": dynamic_block(lits, [0], [65, 66, ("sym", 257)]).done() + pad,
        "one distance code of two bits": dynamic_block(lits, [2], [65, 66, ("lsym", 257, 0, 0, 0)]).done() + pad,
        "a literal/length set of one two-bit code": dynamic_block({256: 2}, [0], []).done() + pad,
    }


def eob_only_block(final: bool, w: BitWriter | None = None) -> BitWriter:
    """a dynamic block whose literal/length set is ONE code of one bit, for symbol 256: incomplete, and accepted by zlib's
    inftrees.c (its error condition is ``left > 0 && (type == CODES || max != 1)``)"""
    return dynamic_block({256: 1}, [0], [], final=final, w=w)


def check_refused_sets(dev):
    cases = refused_sets()
    for raw in cases.values():
        zlib_refuses(raw)
    good_raw, good = good_neighbour()
    names = list(cases)
    got, status = run_inflate(dev, [good_raw] + [cases[n] for n in names] + [good_raw], [len(good)] + [4096] * len(names) + [len(good)], False)
    assert status == [0] + [4] * len(names) + [0], dict(zip(["good"] + names + ["good"], status))
    assert got[0] == good and got[-1] == good                                      # the neighbours are not disturbed


def check_eob_only_block(dev):
    # as a non-final block in front of a fixed block with data
    text = list(b"an empty dynamic block came first") + [(20, 9)]
    raw = fixed_block(text, w=eob_only_block(final=False)).done()
    want = zraw(raw)
    got, tr = inflate_trace(raw)
    assert got == want and len(want) == 53 and tr["types"] == {1, 2} and tr["headers"] == [(257, 1)]
    # as the only block of a stream without output
    alone = eob_only_block(final=True).done()
    assert zraw(alone) == b"" and inflate_trace(alone)[0] == b""
    good_raw, good = good_neighbour()
    got, status = run_inflate(dev, [good_raw, raw, alone, good_raw], [len(good), len(want), 0, len(good)], False, shift=1)
    assert status == [0, 0, 0, 0] and got == [good, want, b"", good], status
    streams = [wrap(good_raw, good), wrap(raw, want), wrap(alone, b""), wrap(good_raw, good)]
    for s, x in zip(streams, [good, want, b"", good]):
        assert zlib_verdict(s + b"xyz") == (x, len(s))
    got, status, used = run_checked(dev, [s + b"xyz" for s in streams], [len(good), len(want), 0, len(good)], shift=3)
    assert status == [0, 0, 0, 0] and got == [good, want, b"", good] and used == [len(s) for s in streams], status


# ---- 3: flushed streams -----------------------------------------------------------------------------------------------------
def flushed(data: bytes, wbits: int) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, wbits)
    return (c.compress(data[:1000]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(data[1000:4000]) + c.flush(zlib.Z_FULL_FLUSH) +
            c.compress(data[4000:]) + c.flush(zlib.Z_SYNC_FLUSH) + c.flush())


def check_flushed_streams(dev):
    text = b"".join(b"gantry %d collimator %d couch %.1f; " % (k * 7 % 360, k * 11 % 360, (k % 50) / 10) for k in range(400))
    assert len(text) > 9000
    raw = flushed(text, -15)
    got, tr = inflate_trace(raw)
    assert zraw(raw) == text and got == text
    assert tr["stored_sizes"] == [0, 0, 0] and raw[-6:] == b"\x00\x00\xff\xff\x03\x00"   # three empty stored blocks, then an empty final one
    good_raw, good = good_neighbour()
    got, status = run_inflate(dev, [good_raw, raw, good_raw], [len(good), len(text), len(good)], False, shift=1)   # out_cap = the size
    assert status == [0, 0, 0] and got == [good, text, good], status
    z = flushed(text, 15)
    assert zlib_verdict(z + b"xyz") == (text, len(z))
    got, status, used = run_checked(dev, [z + b"xyz", wrap(good_raw, good)], [len(text), len(good)], shift=3)
    assert status == [0, 0] and got == [text, good] and used == [len(z), len(good_raw) + 6], status


# ---- 4: seeded random dynamic blocks ----------------------------------------------------------------------------------------
SEEDS = list(range(12))
DIST_SET_SIZES = [1, 2, 3, 5, 12, 30]


def kraft_lengths(rng, n: int) -> list:
    """n code lengths that fill the Kraft budget exactly (n = 1: one code of one bit), from splitting leaves at random, the
    deepest one six times out of ten: 15-bit codes occur"""
    if n == 1:
        return [1]
    d = [1, 1]
    while len(d) < n:
        cand = [i for i, x in enumerate(d) if x < 15]
        i = max(cand, key=lambda j: d[j]) if rng.random() < 0.6 else cand[int(rng.integers(len(cand)))]
        x = d.pop(i)
        d += [x + 1, x + 1]
    return d


def random_block(rng, produced: int, room: int, final: bool, w: BitWriter) -> int:
    """one dynamic block of random code sets and tokens behind `produced` bytes of output, at most `room` bytes of its own"""
    n_dist = int(rng.choice(DIST_SET_SIZES))
    dsyms = sorted(rng.choice(30, n_dist, replace=False).tolist())
    dl = kraft_lengths(rng, n_dist)
    rng.shuffle(dl)
    dist = dict(zip(dsyms, dl))
    n_lit = int(rng.integers(8, 287))
    while True:                                                                    # 256, a literal and a length symbol are coded
        others = rng.choice([s for s in range(286) if s != 256], n_lit - 1, replace=False).tolist()
        if min(others) < 256 < max(others):
            break
    lsyms = [256] + others
    ll = kraft_lengths(rng, len(lsyms))
    rng.shuffle(ll)
    lit = dict(zip(lsyms, ll))
    literals, lengths = [s for s in lsyms if s < 256], [s for s in lsyms if s > 256]
    tokens, made = [], 0
    for _ in range(int(rng.integers(40, 200))):
        if rng.random() < 0.5:
            if made + 1 > room:
                break
            tokens.append(literals[int(rng.integers(len(literals)))])
            made += 1
            continue
        ls, ds = lengths[int(rng.integers(len(lengths)))], dsyms[int(rng.integers(len(dsyms)))]
        eb, db = pc._LEN_EXTRA[ls - 257], pc._DIST_EXTRA[ds]
        extra = (1 << eb) - 1 if rng.random() < 0.25 else int(rng.integers(1 << eb))
        dextra = (1 << db) - 1 if rng.random() < 0.25 else int(rng.integers(1 << db))
        n, d = pc._LEN_BASE[ls - 257] + extra, pc._DIST_BASE[ds] + dextra
        if made + n > room:
            break
        assert d <= produced + made
        tokens.append(("lsym", ls, extra, ds, dextra))
        made += n
    hlit = 286 if rng.random() < 0.25 else None
    hdist = 30 if rng.random() < 0.25 else None
    ops = None
    if rng.random() < 0.67:
        lit_list = [lit.get(s, 0) for s in range(hlit or max(257, max(lit) + 1))]
        dist_list = [dist.get(s, 0) for s in range(hdist or max(dist) + 1)]
        ops = rle_ops(lit_list + dist_list)
    dynamic_block(lit, dist, tokens, final=final, w=w, cl_ops=ops, hlit=hlit, hdist=hdist)
    return made


def random_stream(seed: int) -> bytes:
    rng = np.random.default_rng(7000 + seed)
    w = stored_block(rng.integers(0, 256, 33000, dtype=np.uint8).tobytes(), final=False)
    blocks = int(rng.integers(1, 5))
    produced = 33000
    for b in range(blocks):
        produced += random_block(rng, produced, (65536 - produced) // (blocks - b), b == blocks - 1, w)
    return w.done()


_RANDOM = None


def random_streams():
    """seed -> (raw stream, zlib's output, trace), with the conditions over the whole set asserted: zlib alone decides them"""
    global _RANDOM
    if _RANDOM is not None:
        return _RANDOM
    out = {}
    for seed in SEEDS:
        raw = random_stream(seed)
        want = zraw(raw)                                                           # zlib accepts every stream
        got, tr = inflate_trace(raw)
        assert got == want and 33000 < len(want) <= 65536, seed
        out[seed] = (raw, want, tr)
    every = [t for _, _, t in out.values()]
    assert len(SEEDS) <= 24
    assert max(t["max_lit_code"] for t in every) == 15 and max(t["max_dist_code"] for t in every) == 15
    assert set().union(*(t["len_syms"] for t in every)) == set(range(257, 286))
    assert set().union(*(t["dist_syms"] for t in every)) == set(range(30))
    assert sum(t["dist_codes"].count(1) for t in every) >= 2
    assert sum(t["ring_alias"] for t in every) >= 5
    assert {16, 17, 18} <= set().union(*(t["cl_cross"] | t["cl_syms"] for t in every)) and any(t["cl_cross"] for t in every)
    _RANDOM = out
    return out


def check_random_blocks(dev):
    fx = random_streams()
    raws = [fx[s][0] for s in SEEDS]
    wants = [fx[s][1] for s in SEEDS]
    got, status = run_inflate(dev, raws, [len(x) for x in wants], False, shift=1)  # all streams in ONE launch
    assert status == [0] * len(SEEDS), dict(zip(SEEDS, status))
    for s, g, want in zip(SEEDS, got, wants):
        assert g == want, (s, first_difference(g, want))


def check_random_blocks_checked(dev):
    fx = random_streams()
    streams = [wrap(fx[s][0], fx[s][1]) for s in SEEDS]
    for s, z in zip(SEEDS, streams):
        assert zlib_verdict(z) == (fx[s][1], len(z))
    got, status, used = run_checked(dev, streams, [len(fx[s][1]) for s in SEEDS], shift=3)
    assert status == [0] * len(SEEDS) and used == [len(z) for z in streams], dict(zip(SEEDS, status))
    for s, g in zip(SEEDS, got):
        assert g == fx[s][1], (s, first_difference(g, fx[s][1]))


# ---- 5: through the loaders -------------------------------------------------------------------------------------------------
def alias_stream(data: bytes, dist: int) -> bytes:
    """a zlib stream of `data`, whose bytes from `dist` on repeat the bytes `dist` before them: the first `dist` bytes stored,
    the rest as matches at that distance (32768 - 258 < dist < 32768: every one of them aliases in the ring)"""
    assert RING - 258 < dist < RING and len(data) >= dist + 3 and data[dist:] == data[:len(data) - dist]
    w = stored_block(data[:dist], final=False)
    tokens, left = [], len(data) - dist
    while left:
        n = min(258, left)
        if left - n in (1, 2):
            n -= 3
        tokens.append((n, dist))
        left -= n
    raw = fixed_block(tokens, w=w).done()
    got, tr = inflate_trace(raw)
    assert got == data and zraw(raw) == data and tr["ring_alias"] == len(tokens) >= 7 and tr["max_dist"] == dist
    return wrap(raw, data)


def periodic_rows(seed: int, rows: int, cols: int, period: int) -> np.ndarray:
    a = np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)
    a[period:] = a[:rows - period]
    return a


def check_png_file(dev):
    """160 rows of 1 + 216 bytes, row r + 151 = row r: matches at distance 151 x 217 = 32 767"""
    a = periodic_rows(31, 160, 216, 151)
    f = pc.checked(a, stream=alias_stream(pc.filtered(a, (0,)), 151 * 217))        # PIL reads it back equal to the source
    pc.same_as_pil(dev, [f, pc.pil_file(a)])
    got, stack = pc.same_as_pil(dev, [pc.pil_file(a), f], verify=True)
    assert stack.status.cpu().tolist() == [0, 0] and np.array_equal(got[1], a)


def check_tiff_file(dev):
    """ONE strip of 160 rows of 217 bytes, row r + 151 = row r"""
    a = periodic_rows(32, 160, 217, 151)
    f = tdc.sound(a, pack=lambda raw: alias_stream(raw, 151 * 217), rows_per_strip=160)
    assert len(tdc.tiff.read_tiff(f).strips) == 1
    got, _ = tdc.same_as_pil(dev, [f, tdc.sound(a, rows_per_strip=160)])
    assert np.array_equal(got[0], a)


def deflated_member(name: str, stream: bytes, data: bytes, others=()) -> bytes:
    """an archive whose member `name` is the ready raw Deflate `stream` of `data`: written as a stored member holding the
    stream's bytes, then method, CRC-32 and uncompressed size patched in the local header and in the central directory"""
    z = zc.make_zip([(name, stream, zipfile.ZIP_STORED, None)] + list(others))
    cd = zc.central_entries(z)[0]
    local = struct.unpack_from("<I", z, cd + 42)[0]
    assert z[local:local + 4] == b"PK\x03\x04" and struct.unpack_from("<HH", z, local + 6) == (0, 0)    # no data descriptor, stored
    assert struct.unpack_from("<III", z, local + 14) == struct.unpack_from("<III", z, cd + 16) == (zlib.crc32(stream), len(stream), len(stream))
    crc = zlib.crc32(data)
    z = zc.patched(z, local + 8, "<H", 8)
    z = zc.patched(z, local + 14, "<III", crc, len(stream), len(data))
    z = zc.patched(z, cd + 10, "<H", 8)
    z = zc.patched(z, cd + 16, "<III", crc, len(stream), len(data))
    return z


def check_zip_member(dev):
    data = periodic_rows(33, 160, 217, 151).tobytes()
    stream = alias_stream(data, 151 * 217)[2:-4]                                   # the raw stream
    text = zc.payloads()[0]
    z = deflated_member("series/far.bin", stream, data, others=[("series/text.txt", text, zipfile.ZIP_DEFLATED, 6)])
    with zipfile.ZipFile(io.BytesIO(z)) as zf:
        assert zf.testzip() is None and [i.compress_type for i in zf.infolist()] == [8, 8]
    assert zc.stdlib_read(z) == {"series/far.bin": data, "series/text.txt": text}    # zipfile reads it back
    zc.same_as_stdlib(dev, z)
