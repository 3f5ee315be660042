"""Shared checks of pylinac_amd.png: read_png's chunk walk, load_frames, decode_png_streams, pl_png_decode and pl_inflate
(tests/test_emulated_png.py on the CPU emulator, tests/test_gpu_png.py on the MI355X).  Every pixel comparison is EQUALITY with
``np.asarray(PIL.Image.open(f))``, what the reference's FileImage hands its analyzers; RGB files against PIL's
``convert("I")``; ``pl_inflate`` against ``zlib.decompress``.  No tolerance anywhere.

PIL's adaptive filter choice and zlib's matcher leave branches of the decoder unvisited (zlib emits no distance above 32 506
and stores incompressible data), so the fixtures also come from writers of their own: ``write_png`` forces a filter type per
row, cuts the zlib stream into IDAT chunks at arbitrary byte positions and sets the ``zlib.compressobj`` options;
``fixed_block`` writes fixed-Huffman blocks token by token; ``stored_block`` stored ones.  ``inflate_trace`` is a plain
bit-serial inflate kept for its counters: the cases assert through it, BEFORE the device is asked anything, that the branch
they are named for occurs in the fixture, and PIL / zlib must read every sound fixture back equal to its source."""
from __future__ import annotations

import io
import re
import struct
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

from pylinac_amd import dicom, png

to_np = dicom._to_numpy


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def pil_array(data: bytes) -> np.ndarray:
    img = Image.open(io.BytesIO(data))
    if img.mode == "RGB":
        return np.asarray(img.convert("I"))
    a = np.asarray(img)
    return a.astype(a.dtype.newbyteorder("="))


def expected(a: np.ndarray) -> np.ndarray:
    return a if a.ndim == 2 else np.asarray(Image.fromarray(a).convert("I"))


def pil_file(a: np.ndarray, **kw) -> bytes:
    out = io.BytesIO()
    Image.fromarray(a).save(out, format="PNG", **kw)
    data = out.getvalue()
    assert np.array_equal(pil_array(data), expected(a))                            # the oracle validates the fixture
    return data


# ---- Deflate writers and the tracing inflate (test files only) ------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value: int, n: int):                                            # LSB first (header fields, extra bits)
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, value: int, n: int):                                            # a Huffman code: most significant bit first
        self.bits(int(format(value, f"0{n}b")[::-1], 2), n)

    def done(self) -> bytes:
        if self.n:
            self.out.append(self.acc & 0xFF)
            self.acc, self.n = 0, 0
        return bytes(self.out)


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
              8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def _fixed_lit(w: BitWriter, sym: int):
    if sym < 144:
        w.code(0x30 + sym, 8)
    elif sym < 256:
        w.code(0x190 + sym - 144, 9)
    elif sym < 280:
        w.code(sym - 256, 7)
    else:
        w.code(0xC0 + sym - 280, 8)


def fixed_block(tokens, final: bool = True, w: BitWriter | None = None) -> BitWriter:
    """a fixed-Huffman block from tokens: an int is a literal, (length, distance) a match with hand-chosen values, ("sym", s)
    a raw literal/length symbol and ("dsym", s) a raw distance symbol (for the corrupt cases)"""
    w = w or BitWriter()
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    for t in tokens:
        if isinstance(t, int):
            _fixed_lit(w, t)
        elif t[0] == "sym":
            _fixed_lit(w, t[1])
        elif t[0] == "dsym":
            w.code(t[1], 5)
        else:
            length, dist = t
            k = max(i for i, b in enumerate(_LEN_BASE) if b <= length) if length < 258 else 28
            _fixed_lit(w, 257 + k)
            w.bits(length - _LEN_BASE[k], _LEN_EXTRA[k])
            d = max(i for i, b in enumerate(_DIST_BASE) if b <= dist)
            w.code(d, 5)
            w.bits(dist - _DIST_BASE[d], _DIST_EXTRA[d])
    _fixed_lit(w, 256)
    return w


def stored_block(data: bytes, final: bool = True, w: BitWriter | None = None, nlen: int | None = None) -> BitWriter:
    w = w or BitWriter()
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    if w.n:
        w.bits(0, 8 - w.n)
    w.bits(len(data), 16)
    w.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    w.out += data
    return w


def wrap(raw: bytes, out: bytes = b"") -> bytes:
    """a raw Deflate stream in the zlib wrapper (the Adler-32 of `out`)"""
    return b"\x78\x01" + raw + struct.pack(">I", zlib.adler32(out))


def inflate_trace(raw: bytes, limit: int | None = None):
    """a bit-serial inflate of a RAW stream -> (bytes, trace): block types seen, the largest distance, counts of distance-1,
    length-258 and overlapping (1 < distance < length) matches, of matches whose source lies before a 4 KiB flush boundary of
    their target and of those at distance 32768, the code-length symbols used, the bit span of every Huffman code and the
    byte position of every stored block's LEN field; besides, ``ring_alias`` counts the matches with distance + length > 32768
    (the 32 KiB ring then holds source and target of the copy in the same slots) and ``alias`` lists (32768 - distance, length,
    output position) of each, ``max_lit_code`` / ``max_dist_code`` are the longest literal/length and distance codes that
    occur, ``len_syms`` / ``dist_syms`` the length and distance symbols used, ``stored_sizes`` the LEN of every stored block,
    and per dynamic block ``dist_codes`` has the number of distance codes, ``headers`` (HLIT, HDIST) and ``cl_cross`` the
    repeat symbols whose run begins in the literal/length lengths and ends in the distance lengths.  Incomplete sets pass as
    in zlib's inftrees.c: only ONE code of one bit (or, for distances, no code at all).  Raises ValueError for corrupt or
    truncated data."""
    pos = 0
    nbits = len(raw) * 8
    out = bytearray()
    tr = dict(types=set(), max_dist=0, dist1=0, len258=0, overlap=0, across_flush=0, dist32768=0, cl_syms=set(), codes=[],
              len_fields=[], ring_alias=0, alias=[], max_lit_code=0, max_dist_code=0, len_syms=set(), dist_syms=set(),
              stored_sizes=[], dist_codes=[], headers=[], cl_cross=set())

    def bits(n):
        nonlocal pos
        if pos + n > nbits:
            raise ValueError("truncated")
        v = (int.from_bytes(raw[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    def table(lens):
        count = [0] * 16
        for l in lens:
            count[l] += 1
        count[0] = 0
        left = 1
        for l in range(1, 16):
            left = (left << 1) - count[l]
            if left < 0:
                raise ValueError("over-subscribed")
        code, nxt = 0, [0] * 16
        for l in range(1, 16):
            code = (code + count[l - 1]) << 1
            nxt[l] = code
        t = {}
        for s, l in enumerate(lens):
            if l:
                t[(l, nxt[l])] = s
                nxt[l] += 1
        return t, left

    def symbol(t, longest=None):
        start, code = pos, 0
        for l in range(1, 16):
            code = (code << 1) | bits(1)
            if (l, code) in t:
                tr["codes"].append((start, pos))
                if longest:
                    tr[longest] = max(tr[longest], l)
                return t[(l, code)]
        raise ValueError("invalid code")

    fixed = None
    while True:
        last, typ = bits(1), bits(2)
        tr["types"].add(typ)
        if typ == 0:
            pos = (pos + 7) & ~7
            tr["len_fields"].append(pos >> 3)
            n, c = bits(16), bits(16)
            if n ^ c != 0xFFFF:
                raise ValueError("LEN != ~NLEN")
            if (pos >> 3) + n > len(raw):
                raise ValueError("truncated")
            tr["stored_sizes"].append(n)
            out += raw[pos >> 3:(pos >> 3) + n]
            pos += 8 * n
        elif typ == 3:
            raise ValueError("block type 3")
        else:
            if typ == 1:
                fixed = fixed or (table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)[0], table([5] * 32)[0])
                lit, dist = fixed
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[[16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][k]] = bits(3)
                clt, left = table(cl)
                if left:
                    raise ValueError("incomplete code-length set")
                lens = []
                while len(lens) < hlit + hdist:
                    s = symbol(clt)
                    if s < 16:
                        lens.append(s)
                        continue
                    tr["cl_syms"].add(s)
                    before = len(lens)
                    if s == 16:
                        if not lens:
                            raise ValueError("nothing to repeat")
                        lens += [lens[-1]] * (3 + bits(2))
                    else:
                        lens += [0] * ((3 + bits(3)) if s == 17 else (11 + bits(7)))
                    if before < hlit < len(lens):
                        tr["cl_cross"].add(s)
                if len(lens) > hlit + hdist:
                    raise ValueError("run past HLIT + HDIST")
                lit, left = table(lens[:hlit])
                if left and max(lens[:hlit]) != 1:                                 # (inftrees.c: left > 0 && max != 1)
                    raise ValueError("incomplete literal/length set")
                dist, left = table(lens[hlit:])
                if left and max(lens[hlit:]) > 1:
                    raise ValueError("incomplete distance set")
                tr["dist_codes"].append(len(dist))
                tr["headers"].append((hlit, hdist))
            while True:
                s = symbol(lit, "max_lit_code")
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise ValueError("length symbol")
                    n = _LEN_BASE[s - 257] + bits(_LEN_EXTRA[s - 257])
                    d = symbol(dist, "max_dist_code")
                    if d > 29:
                        raise ValueError("distance symbol")
                    tr["len_syms"].add(s), tr["dist_syms"].add(d)
                    d = _DIST_BASE[d] + bits(_DIST_EXTRA[d])
                    if d > len(out):
                        raise ValueError("distance before the start")
                    at = len(out)
                    tr["max_dist"] = max(tr["max_dist"], d)
                    tr["dist1"] += d == 1
                    tr["len258"] += n == 258
                    tr["overlap"] += 1 < d < n
                    tr["across_flush"] += (at - d) // 4096 < at // 4096
                    tr["dist32768"] += d == 32768
                    if d + n > 32768:
                        tr["ring_alias"] += 1
                        tr["alias"].append((32768 - d, n, at))
                    for k in range(n):
                        out.append(out[at - d + k])
                if limit is not None and len(out) >= limit:
                    return bytes(out[:limit]), tr
        if last:
            return bytes(out), tr


# ---- a PNG writer (test files only) ---------------------------------------------------------------------------------------
def chunk(kind: bytes, payload: bytes) -> bytes:
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def filtered(a: np.ndarray, filters) -> bytes:
    """the bytes the compressor sees: per row the filter-type byte and the filtered row (16-bit samples big-endian); a type
    above 4 is written as it is, over an unfiltered row"""
    h = a.shape[0]
    rows = a.astype(a.dtype.newbyteorder(">")).reshape(h, -1).view(np.uint8).astype(np.int32)
    bpp = a.dtype.itemsize * (1 if a.ndim == 2 else a.shape[2])
    out = bytearray()
    for r in range(h):
        t = filters[r % len(filters)]
        cur = rows[r]
        up = rows[r - 1] if r else np.zeros_like(cur)
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])[:cur.size]
        upleft = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]])[:cur.size]
        p = left + up - upleft
        pa, pb, pc = abs(p - left), abs(p - up), abs(p - upleft)
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
        pred = {1: left, 2: up, 3: (left + up) >> 1, 4: paeth}.get(t, 0)
        out.append(t)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def write_png(a: np.ndarray, filters=(0,), idat_split=(), zopts=None, chunks=(), stream: bytes | None = None, ihdr=None,
              between=None, signature: bytes = png.SIGNATURE) -> bytes:
    """[H, W] uint8 / uint16 or [H, W, 3] uint8 / uint16 -> a PNG.  ``filters``: the filter type of row r is
    filters[r % len]; ``zopts``: level / strategy / wbits / memLevel of ``zlib.compressobj``; ``idat_split``: byte positions
    of the zlib stream at which a new IDAT chunk begins (None: no IDAT at all); ``chunks``: (type, payload) before the first
    IDAT; ``between``: a chunk put after the first IDAT; ``stream``: the zlib stream itself (damaged ones); ``ihdr``: fields
    that replace the writer's own (bits, colour, compression, filter, interlace)."""
    h, w = a.shape[:2]
    if stream is None:
        z = dict(level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, memLevel=8)
        z.update(zopts or {})
        c = zlib.compressobj(z["level"], zlib.DEFLATED, z["wbits"], z["memLevel"], z["strategy"])
        stream = c.compress(filtered(a, filters)) + c.flush()
    head = dict(bits=8 * a.dtype.itemsize, colour=0 if a.ndim == 2 else 2, compression=0, filter=0, interlace=0)
    head.update(ihdr or {})
    out = signature + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, head["bits"], head["colour"], head["compression"],
                                                 head["filter"], head["interlace"]))
    for kind, payload in chunks:
        out += chunk(kind, payload)
    if idat_split is not None:
        cuts = [0] + sorted(idat_split) + [len(stream)]
        for k, (x, y) in enumerate(zip(cuts[:-1], cuts[1:])):
            out += chunk(b"IDAT", stream[x:y])
            if k == 0 and between is not None:
                out += chunk(*between)
    return out + chunk(b"IEND", b"")


def checked(a: np.ndarray, **kw) -> bytes:
    """write_png, with PIL reading the file back equal to the source first"""
    data = write_png(a, **kw)
    assert np.array_equal(pil_array(data), expected(a)), kw
    return data


def zlib_stream(data: bytes) -> bytes:
    info = png.read_png(data)
    return b"".join(data[o:o + n] for o, n in info.idat)


# ---- frames ---------------------------------------------------------------------------------------------------------------
def ridge(seed: int = 0, shape=(96, 130)) -> np.ndarray:
    rng = np.random.default_rng(seed)
    x = np.arange(shape[1], dtype=np.float64)
    return (30000 + 20000 * np.exp(-(x - shape[1] / 2) ** 2 / 200)[None, :] + rng.integers(0, 48, shape)).astype(np.uint16)


def rgb_frame(seed: int, shape) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.clip(rng.integers(0, 40, (*shape, 3)) + np.linspace(0, 215, shape[1])[None, :, None], 0, 255).astype(np.uint8)


def load(dev, files, **kw):
    stack = png.load_frames(files, device=dev, **kw)
    return to_np(stack.frames), stack


def same_as_pil(dev, files, **kw):
    got, stack = load(dev, files, **kw)
    for k, f in enumerate(files):
        want = pil_array(f)
        assert got[k].dtype == want.dtype and np.array_equal(got[k], want), k
    return got, stack


# ---- 1: pl_inflate against zlib.decompress --------------------------------------------------------------------------------
_FIXTURES = None


def inflate_fixtures():
    """name -> (raw Deflate stream, its output); built and traced once"""
    global _FIXTURES
    if _FIXTURES is not None:
        return _FIXTURES
    rng = np.random.default_rng(11)
    noise = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()

    def z(data, level=9, strategy=zlib.Z_DEFAULT_STRATEGY):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        return c.compress(data) + c.flush()

    text = b"".join(b"picket %d leaf %d error %.3f mm; " % (k % 10, k % 60, (k * 37 % 100) / 250) for k in range(900))
    far = list(noise[:20000]) + list(noise[20000:]) + [(258, 32768), 7, 9, (258, 32768), (100, 32768), (3, 1), (258, 1)]
    fx = {
        "noise_twice_then_zeros": noise + noise + bytes(3000) + noise[:500] + bytes(range(256)) * 3,
        "periods": b"ab" * 700 + b"abc" * 900 + b"abcdefg" * 500 + text[:3000] + b"x" * 5000,
        "text_dynamic": text,
    }
    out = {k: (z(v), v) for k, v in fx.items()}
    out["text_fixed"] = (z(text[:4000], 9, zlib.Z_FIXED), text[:4000])
    out["stored_two_blocks"] = (z(noise + noise + noise[:5000], 0), noise + noise + noise[:5000])
    out["rle"] = (z(bytes(20000) + text[:500], 6, zlib.Z_RLE), bytes(20000) + text[:500])
    out["huffman_only"] = (z(text[:6000], 6, zlib.Z_HUFFMAN_ONLY), text[:6000])
    raw = fixed_block(far).done()
    out["far_matches"] = (raw, inflate_trace(raw)[0])
    mixed = fixed_block([104, 105, (6, 2)], final=False)
    stored_block(b"stored in the middle", final=False, w=mixed)
    raw = fixed_block([33, (40, 20)], w=mixed).done()
    out["fixed_stored_fixed"] = (raw, inflate_trace(raw)[0])
    out["empty"] = (z(b""), b"")
    out["one_byte"] = (z(b"Q"), b"Q")
    out["exactly_32768"] = (z(noise[:1000] * 32 + noise[:768]), noise[:1000] * 32 + noise[:768])
    out["exactly_32769"] = (z(noise[:1000] * 32 + noise[:769]), noise[:1000] * 32 + noise[:769])
    for name, (raw, want) in out.items():
        assert zlib.decompress(raw, -15) == want and len(want) <= 100 * 1024, name  # the oracle validates the fixture
    _FIXTURES = out
    return out


def check_inflate_coverage():
    """the coverage condition: asserted through inflate_trace, nothing is asked of the device"""
    traces = {}
    for name, (raw, want) in inflate_fixtures().items():
        got, traces[name] = inflate_trace(raw)
        assert got == want, name
    every = traces.values()
    types = set().union(*(t["types"] for t in every))
    assert types == {0, 1, 2}, types
    assert set().union(*(t["cl_syms"] for t in every)) == {16, 17, 18}
    assert sum(t["dist1"] for t in every) > 0 and sum(t["len258"] for t in every) > 0 and sum(t["overlap"] for t in every) > 0
    assert traces["far_matches"]["dist32768"] == 3 and traces["far_matches"]["max_dist"] == 32768
    assert sum(t["across_flush"] for t in every) > 0
    assert max(t["max_dist"] for n, t in traces.items() if n != "far_matches") <= 32506
    assert [len(inflate_fixtures()[n][1]) for n in ("empty", "one_byte", "exactly_32768", "exactly_32769")] == [0, 1, 32768, 32769]
    return traces


def run_inflate(dev, streams, caps, wrapper, shift=0):
    """streams laid one after the other (`shift` bytes of padding first, then each where the one before ends: odd offsets)"""
    buf, off = bytearray(b"\xAA" * shift), []
    for s in streams:
        off.append(len(buf))
        buf += s
    out, out_off, out_len, status = png.inflate(np.frombuffer(bytes(buf), dtype=np.uint8), off, [len(s) for s in streams], caps,
                                                wrapper=wrapper, device=dev)
    flat = to_np(out)
    oo, ol = out_off.cpu().tolist(), out_len.cpu().tolist()
    return [flat[o:o + n].tobytes() for o, n in zip(oo, ol)], status.cpu().tolist()


def check_inflate_fixture(dev, name):
    raw, want = inflate_fixtures()[name]
    for wrapper in (True, False):
        data = wrap(raw, want) if wrapper else raw
        assert (zlib.decompress(data) if wrapper else zlib.decompress(data, -15)) == want
        got, status = run_inflate(dev, [data], [len(want)], wrapper, shift=1 if wrapper else 0)
        assert status == [0] and got[0] == want, (name, wrapper)


def check_inflate_eight_streams(dev):
    fx = inflate_fixtures()
    names = ["one_byte", "text_fixed", "empty", "periods", "fixed_stored_fixed", "rle", "huffman_only", "text_dynamic"]
    streams = [wrap(*fx[n]) for n in names]
    assert len({len(s) for s in streams}) == 8 and any(sum(map(len, streams[:k])) % 2 for k in range(8))
    got, status = run_inflate(dev, streams, [len(fx[n][1]) for n in names], True, shift=3)
    assert status == [0] * 8
    for n, g in zip(names, got):
        assert g == zlib.decompress(wrap(*fx[n])), n
    # a capacity below the stream's size: what lies beyond is never stored; one above it: the stream ends early (bit 2)
    raw, want = fx["text_dynamic"]
    buf, off = np.frombuffer(raw, dtype=np.uint8), [0, 0]
    out = torch.full((4096 + 70000,), 0x5A, dtype=torch.uint8, device=dev)
    _, _, out_len, status = png.inflate(buf, off, [len(raw)] * 2, [1000, len(want) + 5], wrapper=False, out_off=[16, 4096],
                                        device=dev, out=out)
    flat = to_np(out)
    assert out_len.cpu().tolist() == [1000, len(want)] and status.cpu().tolist() == [0, png.STATUS_SHORT]
    assert flat[16:1016].tobytes() == want[:1000] and (flat[1016:4096] == 0x5A).all() and (flat[:16] == 0x5A).all()
    assert flat[4096:4096 + len(want)].tobytes() == want and (flat[4096 + len(want):] == 0x5A).all()


def corrupt_streams():
    """name -> (raw stream, status bit); zlib refuses every one"""
    w = BitWriter()
    w.bits(1, 1), w.bits(3, 2)
    type3 = w.done() + b"\0\0"
    nlen = stored_block(b"abcdef", nlen=0x1234).done()
    w = BitWriter()
    w.bits(1, 1), w.bits(2, 2), w.bits(0, 5), w.bits(0, 5), w.bits(15, 4)
    for _ in range(19):
        w.bits(1, 3)                                                               # nineteen one-bit codes
    over = w.done() + b"\0" * 8
    w = BitWriter()
    w.bits(1, 1), w.bits(2, 2), w.bits(0, 5), w.bits(0, 5), w.bits(0, 4)
    for v in (2, 0, 0, 0):                                                         # ONE code-length code: incomplete
        w.bits(v, 3)
    incomplete = w.done() + b"\0" * 8
    w = BitWriter()
    w.bits(1, 1), w.bits(2, 2), w.bits(0, 5), w.bits(0, 5), w.bits(0, 4)
    for v in (1, 0, 0, 1):                                                         # codes for 16 and 0 ...
        w.bits(v, 3)
    w.code(1, 1)                                                                   # ... and a 16 with nothing to repeat
    repeat = w.done() + b"\0" * 8
    good = zlib.compressobj(9, zlib.DEFLATED, -15)
    good = good.compress(bytes(range(256)) * 40) + good.flush()
    return {
        "block type 3": (type3, 4),
        "NLEN mismatch": (nlen, 4),
        "over-subscribed": (over, 4),
        "incomplete": (incomplete, 4),
        "repeat without a length": (repeat, 4),
        "distance before the start": (fixed_block([97, (3, 5)]).done(), 4),
        "length symbol 286": (fixed_block([97, ("sym", 286), ("dsym", 0)]).done(), 4),
        "distance symbol 30": (fixed_block([97, 98, ("sym", 257), ("dsym", 30)]).done(), 4),
        "truncated": (good[:len(good) // 2], 2),
        "truncated stored": (stored_block(b"0123456789").done()[:9], 2),
    }


def check_inflate_status(dev):
    cases = corrupt_streams()
    for name, (raw, bit) in cases.items():
        with pytest.raises(zlib.error):
            zlib.decompress(raw, -15)
        with pytest.raises(ValueError):
            inflate_trace(raw)
    good_raw, good = inflate_fixtures()["text_fixed"]
    names = list(cases)
    streams = [good_raw] + [cases[n][0] for n in names] + [good_raw]
    got, status = run_inflate(dev, streams, [len(good)] + [4096] * len(names) + [len(good)], False)
    assert status == [0] + [cases[n][1] for n in names] + [0], dict(zip(["good"] + names + ["good"], status))
    assert got[0] == good and got[-1] == good                                      # the neighbours are not disturbed
    # the zlib wrapper: CM, CINFO, FCHECK, FDICT
    for head in (b"\x79\x01", b"\x88\x1c", b"\x78\x02", b"\x78\x20"):
        with pytest.raises(zlib.error):
            zlib.decompress(head + good_raw + struct.pack(">I", zlib.adler32(good)))
        assert run_inflate(dev, [head + good_raw], [len(good)], True)[1] == [4], head
    # descriptors: a window outside the buffer, a negative capacity
    buf = np.frombuffer(good_raw, dtype=np.uint8)
    _, _, out_len, status = png.inflate(buf, [0, 5, -1, 0], [len(buf), len(buf), 4, 1 << 40], [len(good)] * 4, wrapper=False, device=dev)
    assert status.cpu().tolist()[0] == 0 and status.cpu().tolist()[1] != 0 and status.cpu().tolist()[2:] == [1, 1]
    assert out_len.cpu().tolist()[2:] == [0, 0]


# ---- 2: filters -----------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 70), (5, 7), (63, 33), (64, 65), (65, 64), (130, 9)]
FILTER_SETS = [(0,), (1,), (2,), (3,), (4,), (0, 1, 2, 3, 4)]


def filter_frames(rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    return [rng.integers(0, 256, (rows, cols)).astype(np.uint8), rng.integers(0, 65536, (rows, cols)).astype(np.uint16),
            rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8)]


def check_filters(dev, rows, cols):
    for a in filter_frames(rows, cols):
        files = [checked(a, filters=f) for f in FILTER_SETS]
        for f in files:
            assert set(zlib.decompress(zlib_stream(f))[::1 + a[0].nbytes]) == set(FILTER_SETS[files.index(f)][:rows])
        got, _ = same_as_pil(dev, files)
        assert got.dtype == (np.int32 if a.ndim == 3 else a.dtype)


def check_paeth_ties(dev):
    for dtype in (np.uint8, np.uint16):
        const = np.full((70, 37), 200, dtype=dtype)
        board = ((np.indices((70, 37)).sum(axis=0) & 1) * 255).astype(dtype)
        for a in (const, board, np.stack([board.astype(np.uint8)] * 3, axis=2)):
            same_as_pil(dev, [checked(a, filters=(4,)), checked(a, filters=(3, 4)), checked(a, filters=(4, 2, 4, 1))])


# ---- 3: PIL's own files ---------------------------------------------------------------------------------------------------
def check_pil_files(dev, kind):
    rng = np.random.default_rng(3)
    shape = (96, 130)
    frames = {"ridge": ridge(0, shape), "constant": np.full(shape, 513, dtype=np.uint16),
              "noise": rng.integers(0, 65536, shape).astype(np.uint16)}
    a16 = frames[kind]
    for a in (a16, (a16 >> 8).astype(np.uint8), np.stack([(a16 >> 8).astype(np.uint8), (a16 & 255).astype(np.uint8),
                                                          (a16 >> 4).astype(np.uint8)], axis=2)):
        files = [pil_file(a, compress_level=level) for level in (0, 1, 6, 9)]
        types = [inflate_trace(zlib_stream(f)[2:])[1]["types"] for f in files]
        assert types[0] == {0} and all(0 in t if kind == "noise" else 2 in t for t in types[1:]), types   # (zlib stores noise)
        same_as_pil(dev, files)


# ---- 4: stacks, IDAT seams, sources, resolution, ancillary chunks ----------------------------------------------------------
def check_idat_seams(dev):
    """an IDAT seam inside a Huffman code and one inside a stored block's LEN field (and one per byte of a short stream)"""
    a = ridge(5, (40, 60))
    whole = checked(a, filters=(4, 1, 2))
    stream = zlib_stream(whole)
    trace = inflate_trace(stream[2:])[1]
    assert 2 in trace["types"]
    inside = [(e - 1) // 8 + 2 for s, e in trace["codes"] if s // 8 != (e - 1) // 8]       # a code begun in the byte before
    assert len(inside) > 10
    cuts = sorted(set(inside[3:200:7]))
    huff = checked(a, filters=(4, 1, 2), idat_split=cuts)
    assert len(png.read_png(huff).idat) == len(cuts) + 1 and zlib_stream(huff) == stream
    stored = checked(a, filters=(1,), zopts=dict(level=0))
    t0 = inflate_trace(zlib_stream(stored)[2:])[1]
    assert t0["types"] == {0} and t0["len_fields"]
    at = t0["len_fields"][0] + 2
    seam = checked(a, filters=(1,), zopts=dict(level=0), idat_split=[at + 1, at + 3, at + 900])
    assert zlib_stream(seam)[at:at + 2] == struct.pack("<H", min(len(filtered(a, (1,))), 65535))
    small = ridge(6, (4, 9))
    every = checked(small, filters=(3,), idat_split=range(1, len(zlib_stream(checked(small, filters=(3,))))))
    same_as_pil(dev, [whole, huff, stored, seam])
    same_as_pil(dev, [every])


def check_mixed_stack(dev):
    a = [ridge(10 + k, (48, 150)) for k in range(6)]
    files = [pil_file(a[0]), pil_file(a[1], compress_level=0), checked(a[2], filters=(4,), zopts=dict(level=9)),
             checked(a[3], filters=(0, 3), zopts=dict(strategy=zlib.Z_FIXED), idat_split=[1, 2, 700]),
             checked(a[4], filters=(2, 1), zopts=dict(strategy=zlib.Z_RLE), chunks=[(b"tEXt", b"Comment\0x")]),
             checked(a[5], filters=(1,), zopts=dict(strategy=zlib.Z_HUFFMAN_ONLY), chunks=[(b"tEXt", b"Comment\0xyz")])]
    starts, pos = set(), 0
    for f in files:                                                                # IDAT payloads at every offset mod 4
        for o, _ in png.read_png(f).idat:
            starts.add((pos + o) % 4)
        pos += (len(f) + 3) & ~3
    assert starts == {0, 1, 2, 3}, starts
    got, stack = same_as_pil(dev, files)
    assert [len(x.idat) for x in stack.images][3] == 4
    perm = [3, 1, 4, 0, 5, 2]
    assert np.array_equal(load(dev, [files[k] for k in perm])[0], got[perm])
    with pytest.raises(ValueError, match=r"file 1 differs from file 0 in width, height"):
        png.load_frames([files[0], pil_file(a[1][:, :-1])], device=dev)
    with pytest.raises(ValueError, match=r"file 1 differs from file 0"):
        png.load_frames([files[0], pil_file((a[1] >> 8).astype(np.uint8))], device=dev)


def check_dtype_and_sources(dev, tmp_path):
    a8 = (ridge(6, (31, 77)) >> 8).astype(np.uint8)
    files = [pil_file(a8), checked(a8, filters=(4, 3))]
    for dt in (np.uint16, np.float64):
        got, _ = load(dev, files, dtype=dt)
        assert got.dtype == dt and np.array_equal(got, np.stack([a8, a8]).astype(dt))
    a16 = ridge(6, (31, 80))                                                       # (rows of 160 bytes: the 16-byte store path)
    for dt in (None, np.uint16, np.float64):
        got, _ = load(dev, [pil_file(a16), checked(a16, filters=(3,))], dtype=dt)
        assert got.dtype == (dt or np.uint16) and np.array_equal(got, np.stack([a16, a16]).astype(dt or np.uint16))
    rgb = rgb_frame(7, (20, 32))
    got, _ = load(dev, [pil_file(rgb)], dtype=np.float64)
    assert np.array_equal(got[0], expected(rgb).astype(np.float64))
    out = torch.zeros((3, 31, 77), dtype=torch.uint8, device=dev)
    stack = png.load_frames(files, device=dev, out=out)
    assert stack.frames.data_ptr() == out.data_ptr() and np.array_equal(to_np(out)[:2], np.stack([a8, a8])) and not to_np(out)[2].any()
    with pytest.raises(ValueError, match="out must be"):
        png.load_frames(files, device=dev, out=out.to(torch.int32))
    with pytest.raises(TypeError, match="np.uint16 or np.float64"):
        png.load_frames(files, device=dev, dtype=np.float32)
    with pytest.raises(ValueError, match="no files"):
        png.load_frames([], device=dev)
    path = tmp_path / "a.png"
    path.write_bytes(files[0])
    got, stack = load(dev, [str(path), path, io.BytesIO(files[0]), bytearray(files[0])])
    assert np.array_equal(got, np.stack([a8] * 4)) and stack.images[0].path == str(path) and stack.images[2].path is None
    assert png.read_png(path).width == 77 and png.read_png(io.BytesIO(files[0])).height == 31


def check_dpi_and_chunks(dev):
    a = ridge(8, (8, 40))
    inch = pil_file(a, dpi=(150, 150))
    want = Image.open(io.BytesIO(inch)).info["dpi"][0]
    info = png.read_png(inch)
    assert info.dpi == want and info.dpmm == want / 25.4 and abs(want - 150) < 0.02
    none = pil_file(a)
    assert png.read_png(none).dpi is None and png.read_png(none).dpmm is None
    aspect = checked(a, chunks=[(b"pHYs", struct.pack(">IIB", 3, 2, 0))])             # unit 0: an aspect ratio only
    assert png.read_png(aspect).dpi is None and "dpi" not in Image.open(io.BytesIO(aspect)).info
    assert png.load_frames([inch, inch], device=dev).dpmm == want / 25.4
    assert png.load_frames([inch, none], device=dev, dpi=200).dpmm == 200 / 25.4     # dpi= overrides the chunks
    assert png.load_frames([none], device=dev).dpmm is None
    mixed = png.load_frames([inch, none], device=dev)
    with pytest.raises(ValueError, match="differ in dpmm"):
        mixed.dpmm
    # ancillary chunks before IDAT: skipped, as PIL's pixel values do not depend on them
    extra = [(b"gAMA", struct.pack(">I", 45455)), (b"pHYs", struct.pack(">IIB", 3937, 3937, 1)), (b"tEXt", b"Title\0film 7"),
             (b"tRNS", struct.pack(">H", 30001))]
    f = checked(a, filters=(4,), chunks=extra)
    img = Image.open(io.BytesIO(f))
    assert png.read_png(f).dpi == img.info["dpi"][0] and [c[0] for c in png.read_png(f).chunks][1:5] == [e[0] for e in extra]
    same_as_pil(dev, [f, none])


# ---- 5: status ------------------------------------------------------------------------------------------------------------
def status_files():
    a = [ridge(20 + k, (48, 60)) for k in range(8)]
    good = zlib_stream(checked(a[1], filters=(4,)))
    rows = filtered(a[0], (1,))
    files = [
        pil_file(a[0]),
        write_png(a[1], stream=good[:len(good) // 2]),                             # truncated IDAT
        write_png(a[2], stream=wrap(corrupt_streams()["block type 3"][0])),
        write_png(a[3], stream=wrap(stored_block(rows[:100], nlen=7).done())),
        write_png(a[4], stream=wrap(corrupt_streams()["over-subscribed"][0])),
        write_png(a[5], stream=wrap(fixed_block([1, 30, (10, 3)]).done())),        # a distance before the start of the output
        write_png(a[6], filters=(1, 5, 2)),                                        # a filter-type byte 5
        checked(a[7], filters=(3,)),
    ]
    want = [0, png.STATUS_SHORT, png.STATUS_CORRUPT_DEFLATE, png.STATUS_CORRUPT_DEFLATE, png.STATUS_CORRUPT_DEFLATE,
            png.STATUS_CORRUPT_DEFLATE, png.STATUS_FILTER, 0]
    for k, w in enumerate(want):                                                   # PIL refuses the same bytes
        if w:
            with pytest.raises(OSError):
                pil_array(files[k])
    return a, files, want


def check_status(dev, monkeypatch):
    a, files, want = status_files()
    stack = png.load_frames(files, device=dev, check=False)
    assert stack.status.cpu().tolist() == want
    got = to_np(stack.frames)
    assert np.array_equal(got[0], a[0]) and np.array_equal(got[7], a[7])           # the neighbours are bit-equal
    with pytest.raises(OSError, match=r"file 1: the image data ends"):
        png.load_frames(files, device=dev)
    with pytest.raises(OSError, match=r"file 1: corrupt Deflate"):
        png.load_frames([files[0], files[4]], device=dev)
    with pytest.raises(OSError, match=r"file 2: a filter-type byte"):
        png.load_frames([files[0], files[7], files[6]], device=dev)
    # check=False transfers nothing back: no tensor of the call is copied to the host
    calls = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *x, **k: (calls.append(self.data_ptr()), real(self, *x, **k))[1])
    stack = png.load_frames(files, device=dev, check=False)
    assert not calls
    stack = png.load_frames([files[0], files[7]], device=dev, check=True)
    assert set(calls) == {stack.status.data_ptr()}                                 # check=True: the status, and nothing else
    monkeypatch.undo()


def segment_table(files):
    buf, off, ln, frame = b"", [], [], []
    for k, f in enumerate(files):
        buf += b"\0" * (-len(buf) % 4)
        for o, c in png.read_png(f).idat:
            off.append(len(buf) + o), ln.append(c), frame.append(k)
        buf += f
    return np.frombuffer(buf, dtype=np.uint8), np.array(off, dtype=np.int64), np.array(ln, dtype=np.int64), np.array(frame, dtype=np.int32)


def check_window_outside_the_buffer(dev):
    a = [ridge(30 + k, (24, 100)) for k in range(3)]
    files = [checked(a[0], filters=(4,), idat_split=[100, 900]), pil_file(a[1]), checked(a[2], filters=(2,), idat_split=[50])]
    buf, off, ln, frame = segment_table(files)
    assert frame.tolist() == [0, 0, 0, 1, 2, 2]
    kw = dict(n=3, width=100, height=24, bits=16, device=dev)
    cases = {(1, "off", -1): 0, (3, "off", len(buf) - 3): 1, (4, "len", 1 << 40): 2, (5, "len", -5): 2, (0, "off", 1 << 50): 0,
             (3, "off", len(buf) + 1): 1, (0, "frame", 1): 1}
    for (s, what, value), bad in cases.items():
        o2, l2, f2 = off.copy(), ln.copy(), frame.copy()
        {"off": o2, "len": l2, "frame": f2}[what][s] = value
        out = torch.from_numpy(np.full((3, 24, 100), 0x5A5A, dtype=np.uint16).view(np.int16)).view(torch.uint16).to(dev)
        frames, status = png.decode_png_streams(buf, o2, l2, f2, out=out, **kw)
        st = status.cpu().tolist()
        assert st[bad] & 1 and (what == "frame" or [x & 1 for x in st] == [int(k == bad) for k in range(3)]), (s, what, st)
        got = to_np(frames)
        assert (got[bad] == 0x5A5A).all(), (s, what)                               # nothing of the frame is stored
        for k in range(3):
            if not st[k]:
                assert np.array_equal(got[k], a[k]), (s, what, k)
    # a frame index outside the stack: the segment is skipped, nobody else is disturbed
    f2 = frame.copy()
    f2[3] = 3
    frames, status = png.decode_png_streams(buf, off, ln, f2, **kw)
    assert status.cpu().tolist() == [0, png.STATUS_SHORT, 0] and np.array_equal(to_np(frames)[[0, 2]], np.stack([a[0], a[2]]))


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    a = ridge(40, (16, 40))
    a8 = (a >> 8).astype(np.uint8)
    rgb = np.stack([a8, a8, a8], axis=2)

    def pil_mode(img):
        out = io.BytesIO()
        img.save(out, format="PNG")
        return out.getvalue()

    good = pil_file(a)
    two = write_png(a, idat_split=[40], between=(b"tEXt", b"Comment\0between"))
    cases = [
        (pil_mode(Image.fromarray(a8).convert("P")), r"colour type 3 \(palette\)"),
        (pil_mode(Image.fromarray(a8).convert("LA")), r"colour type 4 \(grey \+ alpha\)"),
        (pil_mode(Image.fromarray(rgb).convert("RGBA")), r"colour type 6 \(RGBA\)"),
        (pil_mode(Image.fromarray(a8 > 200)), "bit depth 1 "),
        (write_png(a8, ihdr=dict(bits=4)), "bit depth 4 "),
        (write_png(np.stack([a, a, a], axis=2)), "bit depth 16 of an RGB"),
        (write_png(a, ihdr=dict(interlace=1)), "Adam7"),
        (write_png(a, ihdr=dict(compression=1)), "compression method 1"),
        (write_png(a, ihdr=dict(filter=1)), "filter method 1"),
        (write_png(a, signature=b"\x89PNG\r\n\x1a\r"), "not a PNG"),
        (good[:-20], "runs past the end of the file"),
        (write_png(a, idat_split=None), "no IDAT"),
        (two, "not consecutive"),
    ]
    assert [c[0] for c in png.read_png(two).chunks] == [b"IHDR", b"IDAT", b"tEXt", b"IDAT", b"IEND"]
    for data, text in cases:
        with pytest.raises(ValueError, match=r"file 1: .*(" + text + ")"):
            png.load_frames([good, data], device=dev)
    with pytest.raises(ValueError, match="file 2 differs from file 0"):
        png.load_frames([good, good, pil_file(a[:-1])], device=dev)
    # the chunk walk itself
    with pytest.raises(ValueError, match="not a PNG"):
        png.read_png(b"II*\0" + good[4:])
    with pytest.raises(ValueError, match="chunk header at offset"):
        png.read_png(good[:36])
    with pytest.raises(ValueError, match="first chunk is"):
        png.read_png(png.SIGNATURE + chunk(b"IDAT", b"x"))
    info = png.read_png(good)
    assert (info.width, info.height, info.bits, info.colour_type, info.interlace, info.samples) == (40, 16, 16, 0, 0, 1)


# ---- 7: the C ABI ---------------------------------------------------------------------------------------------------------
def check_c_abi_argument_checks(dev):
    """pl_png_decode / pl_inflate: unsupported (2) for samples the kernels do not decode, invalid argument (1) for null
    pointers, n = 0, n > 65535 and bad kinds -- all before any launch (the pointers below are never dereferenced);
    pl_png_work_bytes: -1 for the same"""
    from pylinac_amd import _lib

    lib = _lib.load()
    buf = torch.zeros(256, dtype=torch.uint8, device=dev)
    idx = torch.zeros(8, dtype=torch.int64, device=dev)
    st = torch.zeros(4, dtype=torch.int32, device=dev)
    p, q, s = buf.data_ptr(), idx.data_ptr(), st.data_ptr()

    def call(n=1, n_seg=1, bits=16, spp=1, kind=0, bytes_=p, out=p, work=p, frame=s, w=4, h=4, nbytes=256):
        return lib.pl_png_decode(bytes_, nbytes, q, q, frame, n_seg, n, w, h, bits, spp, out, kind, s, work, None)

    for bits, spp in ((12, 1), (1, 1), (4, 1), (32, 1), (16, 3), (8, 4), (8, 2)):
        assert call(bits=bits, spp=spp) == 2 and b"unsupported samples" in lib.pl_last_error()
        assert lib.pl_png_work_bytes(1, 1, 64, 4, 4, bits, spp) == -1
    assert call(n=0) == 1 and call(n=65536) == 1 and call(n_seg=0) == 1 and call(w=0) == 1 and call(h=0) == 1
    assert call(bytes_=None) == 1 and call(out=None) == 1 and call(work=None) == 1 and call(frame=None) == 1
    assert call(kind=3) == 1 and call(kind=-1) == 1 and call(nbytes=-1) == 1
    assert call(bytes_=p + 1) == 1 and b"4-byte" in lib.pl_last_error()
    assert call(work=p + 4) == 1 and b"16-byte" in lib.pl_last_error()
    assert lib.pl_png_work_bytes(0, 1, 64, 4, 4, 16, 1) == -1 and lib.pl_png_work_bytes(1, 0, 64, 4, 4, 16, 1) == -1
    assert lib.pl_png_work_bytes(1, 1, -1, 4, 4, 16, 1) == -1 and lib.pl_png_work_bytes(1, 1, 64, 46341, 46341, 8, 1) == -1
    small, big = lib.pl_png_work_bytes(3, 9, 64, 100, 24, 16, 1), lib.pl_png_work_bytes(3, 9, 6400, 100, 24, 16, 1)
    assert small >= 3 * 24 * 201 + 64 and small % 16 == 0 and big - small >= 6000

    def inflate(n=1, wrapper=1, bytes_=p, out=p, off=q, status=s, nbytes=256):
        return lib.pl_inflate(bytes_, nbytes, off, q, n, wrapper, out, q, q, q, status, None)

    assert inflate(n=0) == 1 and inflate(wrapper=2) == 1 and inflate(wrapper=-1) == 1 and inflate(nbytes=-1) == 1
    assert inflate(bytes_=None) == 1 and inflate(out=None) == 1 and inflate(off=None) == 1 and inflate(status=None) == 1
    assert inflate(bytes_=p + 2) == 1 and b"4-byte" in lib.pl_last_error()
    header = (Path(__file__).resolve().parent.parent / "include" / "pylinac_hip.h").read_text()
    assert re.search(r"int pl_png_decode\(", header) and re.search(r"int64_t pl_png_work_bytes\(", header)
    assert re.search(r"int pl_inflate\(", header) and lib.pl_abi_version() == 3
