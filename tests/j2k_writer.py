"""A test-side JPEG 2000 writer (ITU-T T.800) in plain Python / numpy, independent of pylinac_amd: exactly the subset the
device path decodes (one component, one tile, one tile-part, one layer, one precinct per resolution, code-block style 0, the
reversible 5/3 transform) with every choice an encoder is free to make as a parameter, so that tests can write the legal
streams OpenJPEG's encoder never writes.  The judge of what it writes is an independent decoder (Pillow's OpenJPEG), not this
file: tests/dicom_j2k_conformance_checks.py.

  forward 5/3   F.4.8 with the whole-sample symmetric extension; low band ceil(n / 2), high band floor(n / 2), a length of 1
                passes through; columns first, then rows (the inverse undoes rows last); any number of levels on any size.
  tier 1        Annex D: cleanup on the top plane, then significance propagation, magnitude refinement and cleanup per plane in
                stripes of four rows, run-length mode with the two UNIFORM bits, Table D.1 (HL transposed), D.2 / D.3, the three
                refinement contexts; Annex C: INITENC, CODEMPS / CODELPS, BYTEOUT, FLUSH.  ``termination``: "flush" is the
                standard FLUSH with a trailing FF dropped, "shortest" the shortest prefix of it that decodes to the same
                decisions when the decoder reads FF (1-bits) past its end -- found with an MQ decoder that replays the block's
                contexts; length 0 where that is what it takes.  The shortest prefix never ends in FF (the decoder reads FF past
                the end anyway, so the prefix without it decodes as well): "shortest+ff" keeps the FF that follows the shortest
                prefix in the FLUSHed form where one does, which is a segment that ENDS in FF, cut in front of a byte <= 8F.
  tier 2        Annex B: the zero-length bit, the inclusion and zero-bit-plane tag trees, Table B.4, Lblock, the lengths, a
                7-bit byte after FF, the header padded to a byte and a last byte FF followed by one stuffed byte.
  record        what was written, next to the bytes: ``Record.blocks`` has one row per included block in the column order of
                pylinac_amd.dicom._j2k_codestream (offset, length, passes, planes, orientation, x0, y0, w, h).
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field

import numpy as np

# T.800 Table C.2: Qe, NMPS, NLPS, SWITCH
MQ_TABLE = [
    (0x5601, 1, 1, 1), (0x3401, 2, 6, 0), (0x1801, 3, 9, 0), (0x0AC1, 4, 12, 0), (0x0521, 5, 29, 0), (0x0221, 38, 33, 0),
    (0x5601, 7, 6, 1), (0x5401, 8, 14, 0), (0x4801, 9, 14, 0), (0x3801, 10, 14, 0), (0x3001, 11, 17, 0), (0x2401, 12, 18, 0),
    (0x1C01, 13, 20, 0), (0x1601, 29, 21, 0), (0x5601, 15, 14, 1), (0x5401, 16, 14, 0), (0x5101, 17, 15, 0), (0x4801, 18, 16, 0),
    (0x3801, 19, 17, 0), (0x3401, 20, 18, 0), (0x3001, 21, 19, 0), (0x2801, 22, 19, 0), (0x2401, 23, 20, 0), (0x2201, 24, 21, 0),
    (0x1C01, 25, 22, 0), (0x1801, 26, 23, 0), (0x1601, 27, 24, 0), (0x1401, 28, 25, 0), (0x1201, 29, 26, 0), (0x1101, 30, 27, 0),
    (0x0AC1, 31, 28, 0), (0x09C1, 32, 29, 0), (0x08A1, 33, 30, 0), (0x0521, 34, 31, 0), (0x0441, 35, 32, 0), (0x02A1, 36, 33, 0),
    (0x0221, 37, 34, 0), (0x0141, 38, 35, 0), (0x0111, 39, 36, 0), (0x0085, 40, 37, 0), (0x0049, 41, 38, 0), (0x0025, 42, 39, 0),
    (0x0015, 43, 40, 0), (0x0009, 44, 41, 0), (0x0005, 45, 42, 0), (0x0001, 45, 43, 0), (0x5601, 46, 46, 0)]
_QE = [r[0] for r in MQ_TABLE]
_NMPS = [r[1] for r in MQ_TABLE]
_NLPS = [r[2] for r in MQ_TABLE]
_SWITCH = [r[3] for r in MQ_TABLE]

CX_SIGN, CX_REF, CX_RUN, CX_UNI, N_CX = 9, 14, 17, 18, 19     # 0 .. 8 zero coding, 9 .. 13 sign, 14 .. 16 refinement


def _initial_states() -> list:
    """Table D.7: the all-zero-neighbours context starts at state 4, the run-length context at 3, UNIFORM at 46"""
    states = [0] * N_CX
    states[0], states[CX_RUN], states[CX_UNI] = 4, 3, 46
    return states


# ---- the 5/3 transform ------------------------------------------------------------------------------------------------------
def _forward_1d(x: np.ndarray) -> np.ndarray:
    """axis 0 of an int64 array: interleaved samples -> the low band (ceil(n / 2)), then the high band"""
    n = x.shape[0]
    if n == 1:
        return x.copy()
    ext = np.concatenate([x, x[n - 2:n - 1]])                                     # x[n] = x[n - 2]
    high = ext[1:n:2] - ((ext[0:n - 1:2] + ext[2:n + 1:2]) >> 1)                  # y[2k + 1], k < floor(n / 2)
    nl, nh = (n + 1) // 2, n // 2
    before = np.concatenate([high[:1], high])[:nl]                                # y[2k - 1], y[-1] = y[1]
    after = np.concatenate([high, high[-1:]])[:nl]                                # y[2k + 1], y[n] = y[n - 2]
    low = x[0:n:2] + ((before + after + 2) >> 2)
    assert len(low) == nl and len(high) == nh
    return np.concatenate([low, high])


def forward_53(samples: np.ndarray, levels: int) -> np.ndarray:
    """[rows, cols] integers -> the coefficient plane: LL of the last level at the top left, every level's HL to its right, LH
    below it and HH diagonal (the layout the packets' rectangles refer to)"""
    plane = samples.astype(np.int64).copy()
    rows, cols = plane.shape
    for d in range(levels):
        rh, rw = (rows + (1 << d) - 1) >> d, (cols + (1 << d) - 1) >> d
        region = plane[:rh, :rw]
        region = _forward_1d(region)                                               # vertically (F.4.8: VER_SD first)
        plane[:rh, :rw] = _forward_1d(region.T).T                                  # then horizontally
    return plane


# ---- tier 1 -----------------------------------------------------------------------------------------------------------------
def _zero_coding_table(orient: int) -> list:
    """Table D.1 as [h][v][d] -> context; h, v <= 2, d <= 4"""
    def ll_lh(h, v, d):
        if h == 2:
            return 8
        if h == 1:
            return 7 if v >= 1 else 6 if d >= 1 else 5
        if v == 2:
            return 4
        if v == 1:
            return 3
        return 2 if d >= 2 else d

    def hh(h, v, d):
        hv = h + v
        if d >= 3:
            return 8
        if d == 2:
            return 7 if hv >= 1 else 6
        if d == 1:
            return 5 if hv >= 2 else 4 if hv == 1 else 3
        return 2 if hv >= 2 else hv

    if orient == 3:
        return [[[hh(h, v, d) for d in range(5)] for v in range(3)] for h in range(3)]
    if orient == 1:                                                                # HL: horizontal and vertical exchanged
        return [[[ll_lh(v, h, d) for d in range(5)] for v in range(3)] for h in range(3)]
    return [[[ll_lh(h, v, d) for d in range(5)] for v in range(3)] for h in range(3)]


_ZC = [_zero_coding_table(o) for o in range(4)]
# Tables D.2 / D.3: (horizontal, vertical contribution) -> (context, XOR bit)
_SC = {(1, 1): (13, 0), (1, 0): (12, 0), (1, -1): (11, 0), (0, 1): (10, 0), (0, 0): (9, 0), (0, -1): (10, 1), (-1, 1): (11, 1),
       (-1, 0): (12, 1), (-1, -1): (13, 1)}


def block_decisions(coeffs: np.ndarray, orient: int):
    """one code block [h, w] of signed coefficients -> (magnitude bit planes, contexts, decisions) of its 3 * planes - 2 passes"""
    h, w = coeffs.shape
    W = w + 2
    mag = [0] * ((h + 2) * W)
    neg = [0] * ((h + 2) * W)
    for y in range(h):
        row = coeffs[y].tolist()
        for x in range(w):
            v = row[x]
            mag[(y + 1) * W + x + 1] = -v if v < 0 else v
            neg[(y + 1) * W + x + 1] = 1 if v < 0 else 0
    planes = max(mag).bit_length()
    sig = [0] * ((h + 2) * W)
    chi = [0] * ((h + 2) * W)
    vis = [0] * ((h + 2) * W)
    ref = [0] * ((h + 2) * W)
    zc = _ZC[orient]
    cxs, ds = bytearray(), bytearray()

    def context(i):
        return zc[sig[i - 1] + sig[i + 1]][sig[i - W] + sig[i + W]][sig[i - W - 1] + sig[i - W + 1] + sig[i + W - 1] + sig[i + W + 1]]

    def sign(i):
        hc, vc = chi[i - 1] + chi[i + 1], chi[i - W] + chi[i + W]
        cx, flip = _SC[(max(-1, min(1, hc)), max(-1, min(1, vc)))]
        cxs.append(cx)
        ds.append(neg[i] ^ flip)
        sig[i] = 1
        chi[i] = -1 if neg[i] else 1

    def cleanup(p):
        for y0 in range(0, h, 4):
            rows = min(4, h - y0)
            for x in range(w):
                col = [(y0 + r + 1) * W + x + 1 for r in range(rows)]
                start = 0
                if rows == 4 and not any(sig[i] or vis[i] or context(i) for i in col):
                    first = next((r for r in range(4) if (mag[col[r]] >> p) & 1), None)
                    cxs.append(CX_RUN)
                    ds.append(0 if first is None else 1)
                    if first is None:
                        continue
                    cxs.append(CX_UNI)
                    ds.append(first >> 1)
                    cxs.append(CX_UNI)
                    ds.append(first & 1)
                    sign(col[first])
                    start = first + 1
                for i in col[start:]:
                    if not sig[i] and not vis[i]:
                        bit = (mag[i] >> p) & 1
                        cxs.append(context(i))
                        ds.append(bit)
                        if bit:
                            sign(i)
                for i in col:
                    vis[i] = 0

    def propagation(p):
        for y0 in range(0, h, 4):
            for x in range(w):
                for r in range(min(4, h - y0)):
                    i = (y0 + r + 1) * W + x + 1
                    if sig[i]:
                        continue
                    cx = context(i)
                    if cx == 0:                                                    # (context 0: no significant neighbour)
                        continue
                    bit = (mag[i] >> p) & 1
                    cxs.append(cx)
                    ds.append(bit)
                    vis[i] = 1
                    if bit:
                        sign(i)

    def refinement(p):
        for y0 in range(0, h, 4):
            for x in range(w):
                for r in range(min(4, h - y0)):
                    i = (y0 + r + 1) * W + x + 1
                    if not sig[i] or vis[i]:
                        continue
                    cxs.append(CX_REF + 2 if ref[i] else CX_REF + 1 if context(i) else CX_REF)
                    ds.append((mag[i] >> p) & 1)
                    ref[i] = 1

    if planes:
        cleanup(planes - 1)
        for p in range(planes - 2, -1, -1):
            propagation(p)
            refinement(p)
            cleanup(p)
    return planes, cxs, ds


def mq_encode(cxs, ds) -> bytes:
    """Annex C.2: the decisions under their contexts -> the FLUSHed codeword; a trailing FF is dropped"""
    index, mps = _initial_states(), [0] * N_CX
    out = bytearray([0])                                                           # the byte in front of the first (BP = BPST - 1)
    a, c, ct = 0x8000, 0, 12

    def byteout(c):
        if out[-1] == 0xFF:
            out.append((c >> 20) & 0xFF)
            return c & 0xFFFFF, 7
        if c >= 0x8000000:
            out[-1] += 1                                                           # (the carry; the byte was below FF)
            c &= 0x7FFFFFF
            if out[-1] == 0xFF:
                out.append((c >> 20) & 0xFF)
                return c & 0xFFFFF, 7
        out.append((c >> 19) & 0xFF)
        return c & 0x7FFFF, 8

    for cx, d in zip(cxs, ds):
        i = index[cx]
        qe = _QE[i]
        a -= qe
        if d == mps[cx]:                                                           # CODEMPS
            if a & 0x8000:
                c += qe
                continue
            if a < qe:
                a = qe
            else:
                c += qe
            index[cx] = _NMPS[i]
        else:                                                                      # CODELPS
            if a < qe:
                c += qe
            else:
                a = qe
            if _SWITCH[i]:
                mps[cx] ^= 1
            index[cx] = _NLPS[i]
        while True:                                                                # RENORME
            a <<= 1
            c <<= 1
            ct -= 1
            if ct == 0:
                c, ct = byteout(c)
            if a & 0x8000:
                break
    # FLUSH: SETBITS, two bytes out
    top = c + a
    c |= 0xFFFF
    if c >= top:
        c -= 0x8000
    c <<= ct
    c, ct = byteout(c)
    c <<= ct
    c, ct = byteout(c)
    assert out[0] == 0                                                             # no carry reaches the byte in front
    body = bytes(out[1:])
    return body[:-1] if body.endswith(b"\xff") else body


def mq_replay(data: bytes, length: int, cxs, ds, start=None, snapshots=None) -> bool:
    """Annex C.3: whether a decoder that is given ``data[:length]`` and reads FF past it decodes ``ds`` under ``cxs``.
    ``snapshots``: filled with (highest byte index looked at, the decoder before decision i) whenever that index grows;
    ``start``: such a snapshot to go on from."""
    def byte(p):
        return data[p] if p < length else 0xFF

    if start is None:
        index, mps = _initial_states(), [0] * N_CX
        cur = byte(0)
        c = cur << 16
        bp, first = 0, 0
        nx = byte(1)                                                               # BYTEIN
        if cur == 0xFF and nx > 0x8F:
            c += 0xFF00
            ct = 8
        elif cur == 0xFF:
            bp, cur, c, ct = 1, nx, c + (nx << 9), 7
        else:
            bp, cur, c, ct = 1, nx, c + (nx << 8), 8
        c = (c << 7) & 0xFFFFFFFF
        ct -= 7
        a, seen = 0x8000, 1
    else:
        seen, first, a, c, ct, bp, cur, index, mps = start
        index, mps = index[:], mps[:]
    marked = -1
    for i in range(first, len(cxs)):
        if snapshots is not None and seen > marked:
            snapshots.append((seen, i, a, c, ct, bp, cur, index[:], mps[:]))
            marked = seen
        cx = cxs[i]
        s = index[cx]
        qe = _QE[s]
        d = mps[cx]
        a -= qe
        if (c >> 16) < qe:
            lps = a >= qe
            a = qe
        else:
            c -= qe << 16
            if a & 0x8000:
                if d != ds[i]:
                    return False
                continue
            lps = a < qe
        if lps:
            d ^= 1
            if _SWITCH[s]:
                mps[cx] ^= 1
            index[cx] = _NLPS[s]
        else:
            index[cx] = _NMPS[s]
        if d != ds[i]:
            return False
        while True:                                                                # RENORMD
            if ct == 0:
                nx = byte(bp + 1)
                seen = max(seen, bp + 1)
                if cur == 0xFF:
                    if nx > 0x8F:
                        c += 0xFF00
                        ct = 8
                    else:
                        bp, cur, c, ct = bp + 1, nx, c + (nx << 9), 7
                else:
                    bp, cur, c, ct = bp + 1, nx, c + (nx << 8), 8
            a <<= 1
            c = (c << 1) & 0xFFFFFFFF
            ct -= 1
            if a & 0x8000:
                break
    return True


def shortest_prefix(full: bytes, cxs, ds) -> int:
    """the smallest L such that ``full[:L]`` followed by 1-bits decodes to the block's decisions (every L is tried: a decoder
    of ``full[:L]`` is the decoder of ``full`` until it first looks at byte L, and goes on from that snapshot)"""
    snapshots = []
    assert mq_replay(full, len(full), cxs, ds, snapshots=snapshots)               # the encoder's own output decodes
    at = 0
    for length in range(len(full)):
        start = None
        if length >= 2:
            while at + 1 < len(snapshots) and snapshots[at + 1][0] < length:
                at += 1
            start = snapshots[at] if snapshots and snapshots[at][0] < length else None
        if mq_replay(full, length, cxs, ds, start=start):
            return length
    return len(full)


# ---- tier 2 -----------------------------------------------------------------------------------------------------------------
class BitWriter:
    """B.10.1: most significant bit first; the byte after FF carries 7 bits"""

    def __init__(self):
        self.out, self.acc, self.room = bytearray(), 0, 8

    def put(self, bit: int):
        self.room -= 1
        self.acc |= (bit & 1) << self.room
        if self.room == 0:
            self._byte()

    def _byte(self):
        self.out.append(self.acc)
        self.room = 7 if self.acc == 0xFF else 8
        self.acc = 0

    def bits(self, value: int, n: int):
        for k in range(n - 1, -1, -1):
            self.put((value >> k) & 1)

    def finish(self) -> tuple[bytes, bool]:
        """-> (the header's bytes, whether a stuffed byte follows a last byte FF)"""
        if self.room != (7 if self.out and self.out[-1] == 0xFF else 8):
            self._byte()                                                           # the rest of the last byte: zeros
        if self.out and self.out[-1] == 0xFF:
            self.out.append(0)
            return bytes(self.out), True
        return bytes(self.out), False


class TagTree:
    """B.10.2, the encoder's side: ``values`` [h][w] of the leaves; a node's value is the minimum of its children"""

    def __init__(self, values):
        level = [list(r) for r in values]
        self.levels = [level]
        while len(level) > 1 or len(level[0]) > 1:
            h, w = len(level), len(level[0])
            level = [[min(level[y][x] for y in range(2 * Y, min(2 * Y + 2, h)) for x in range(2 * X, min(2 * X + 2, w)))
                      for X in range((w + 1) // 2)] for Y in range((h + 1) // 2)]
            self.levels.append(level)
        self.low = [[[0] * len(l[0]) for _ in l] for l in self.levels]
        self.known = [[[False] * len(l[0]) for _ in l] for l in self.levels]

    @property
    def depth(self) -> int:
        return len(self.levels)

    def encode(self, bw: BitWriter, x: int, y: int, threshold: int):
        low = 0
        for l in range(len(self.levels) - 1, -1, -1):
            Y, X = y >> l, x >> l
            low = max(low, self.low[l][Y][X])
            value = self.levels[l][Y][X]
            while low < threshold:
                if low >= value:
                    if not self.known[l][Y][X]:
                        bw.put(1)
                        self.known[l][Y][X] = True
                    break
                bw.put(0)
                low += 1
            self.low[l][Y][X] = low


def put_passes(bw: BitWriter, n: int):
    """Table B.4"""
    assert 1 <= n <= 164
    if n == 1:
        bw.put(0)
    elif n == 2:
        bw.bits(0b10, 2)
    elif n <= 5:
        bw.bits(0b11, 2)
        bw.bits(n - 3, 2)
    elif n <= 36:
        bw.bits(0b1111, 4)
        bw.bits(n - 6, 5)
    else:
        bw.bits(0b111111111, 9)
        bw.bits(n - 37, 7)


@dataclass
class Band:
    r: int
    orient: int
    x0: int
    y0: int
    w: int
    h: int
    exponent: int
    ncx: int = 0
    ncy: int = 0
    included: list = field(default_factory=list)            # [ncy][ncx] bool
    zero_planes: list = field(default_factory=list)         # [ncy][ncx] (of included blocks; None otherwise)
    tree_depth: int = 0


@dataclass
class Packet:
    r: int
    start: int = 0
    header_end: int = 0                                     # behind the stuffed byte where there is one
    end: int = 0
    stuffed: bool = False
    empty: bool = False                                     # written as the single byte 00
    bands: list = field(default_factory=list)               # every band of the resolution, the empty ones too


@dataclass
class Segment:
    data: bytes                                             # as written
    full: bytes                                             # the FLUSHed form
    decisions: int
    length_bits: int                                        # the width of its length field
    lblock: int


@dataclass
class Record:
    blocks: list = field(default_factory=list)              # (offset, length, passes, planes, orient, x0, y0, w, h)
    segments: list = field(default_factory=list)            # one Segment per row of ``blocks``
    packets: list = field(default_factory=list)
    coefficients: np.ndarray | None = None
    first_packet: int = 0


GAIN = {0: 0, 1: 1, 2: 1, 3: 2}


def default_exponents(precision: int, levels: int) -> list:
    """what OpenJPEG writes: precision + the band's gain, in QCD's order (LL, then HL, LH, HH from the lowest resolution up)"""
    return [precision] + [precision + g for _ in range(levels) for g in (1, 1, 2)]


def encode(frame: np.ndarray, precision: int | None = None, signed: bool | None = None, levels: int = 0, block=(64, 64), guard: int = 2,
           exponents=None, lblock_extra=0, empty_packet: str = "00", progression: int = 0, psot: bool = True,
           termination: str = "flush", forged=None):
    """[rows, cols] integers -> (the codestream, its Record).

    ``precision`` / ``signed``: Ssiz (default: the dtype's); ``block``: (width, height) of a code block, powers of two from 4 to 64
    with at most 4096 samples; ``guard``: 0 .. 7; ``exponents``: 3 * levels + 1 values 0 .. 31 in QCD's order (default:
    ``default_exponents``); ``lblock_extra``: k, or a function of the block's index in the stream -> k: Lblock grows by the least
    increment + k; ``empty_packet``: a packet without an included block is the byte "00", or "80": the bit 1 and one exclusion
    bit per unsettled tag-tree node; ``progression``: the byte of SGcod; ``psot``: Psot stated, or 0; ``termination``: "flush" |
    "shortest" | "shortest+ff";``forged``: (planes, passes, body) written for every block in place of its own coding (refusal fixtures)."""
    frame = np.asarray(frame)
    rows, cols = frame.shape
    bits = 8 * frame.dtype.itemsize
    precision = bits if precision is None else precision
    signed = frame.dtype.kind == "i" if signed is None else signed
    half = 1 << (precision - 1)
    wide = frame.astype(np.int64)
    assert (wide.min() >= -half and wide.max() < half) if signed else (wide.min() >= 0 and wide.max() < 2 * half)
    assert 0 <= levels <= 32 and 0 <= guard <= 7 and empty_packet in ("00", "80") and termination in ("flush", "shortest", "shortest+ff")
    cbw, cbh = block
    xcb, ycb = cbw.bit_length() - 1, cbh.bit_length() - 1
    assert (1 << xcb, 1 << ycb) == (cbw, cbh) and 2 <= xcb <= 10 and 2 <= ycb <= 10 and xcb + ycb <= 12
    exponents = default_exponents(precision, levels) if exponents is None else list(exponents)
    assert len(exponents) == 3 * levels + 1 and all(0 <= e <= 31 for e in exponents)
    extra = lblock_extra if callable(lblock_extra) else (lambda k: lblock_extra)
    plane = forward_53(wide if signed else wide - half, levels)

    head = b"\xff\x4f"
    head += struct.pack(">HHHIIIIIIIIHBBB", 0xFF51, 41, 0, cols, rows, 0, 0, cols, rows, 0, 0, 1, (precision - 1) | (0x80 if signed else 0), 1, 1)
    head += struct.pack(">HHBBHBBBBBB", 0xFF52, 12, 0, progression, 1, 0, levels, xcb - 2, ycb - 2, 0, 1)
    head += struct.pack(">HHB", 0xFF5C, 4 + 3 * levels, guard << 5) + bytes(e << 3 for e in exponents)
    sot = len(head)
    head += struct.pack(">HHHIBB", 0xFF90, 10, 0, 0, 0, 1) + b"\xff\x93"
    out = bytearray(head)
    rec = Record(coefficients=plane, first_packet=len(out))
    res = [((cols + (1 << d) - 1) >> d, (rows + (1 << d) - 1) >> d) for d in range(levels, -1, -1)]
    for r, (rw, rh) in enumerate(res):
        if r == 0:
            bands = [Band(r, 0, 0, 0, rw, rh, exponents[0])]
        else:
            lw, lh = res[r - 1]
            bands = [Band(r, 1, lw, 0, rw - lw, lh, exponents[3 * r - 2]), Band(r, 2, 0, lh, lw, rh - lh, exponents[3 * r - 1]),
                     Band(r, 3, lw, lh, rw - lw, rh - lh, exponents[3 * r])]
        w_blk, h_blk = min(cbw, 1 << (15 - (r > 0))), min(cbh, 1 << (15 - (r > 0)))
        packet = Packet(r, start=len(out), bands=bands)
        coded = []                                           # per band: {(cx, cy): (planes, passes, body, full, decisions)}
        for band in bands:
            blocks = {}
            if band.w and band.h:
                band.ncx, band.ncy = -(-band.w // w_blk), -(-band.h // h_blk)
                band.included = [[False] * band.ncx for _ in range(band.ncy)]
                band.zero_planes = [[None] * band.ncx for _ in range(band.ncy)]
                for cy in range(band.ncy):
                    for cx in range(band.ncx):
                        x0, y0 = band.x0 + cx * w_blk, band.y0 + cy * h_blk
                        w, h = min(w_blk, band.w - cx * w_blk), min(h_blk, band.h - cy * h_blk)
                        coeffs = plane[y0:y0 + h, x0:x0 + w]
                        if forged is not None:
                            blocks[cx, cy] = (forged[0], forged[1], forged[2], forged[2], 0, (x0, y0, w, h))
                        elif coeffs.any():
                            planes, cxs, ds = block_decisions(coeffs, band.orient)
                            full = mq_encode(cxs, ds)
                            body = full
                            if termination != "flush":
                                cut = shortest_prefix(full, cxs, ds)
                                if termination == "shortest+ff" and full[cut:cut + 1] == b"\xff":
                                    cut += 1                 # (the decoder reads the same bytes: FF, then FF for ever)
                                    assert mq_replay(full, cut, cxs, ds)
                                body = full[:cut]
                            blocks[cx, cy] = (planes, 3 * planes - 2, body, full, len(cxs), (x0, y0, w, h))
                        else:
                            continue
                        mb = guard + band.exponent - 1
                        assert blocks[cx, cy][0] <= mb, f"{blocks[cx, cy][0]} bit planes where guard + exponent - 1 = {mb}"
                        band.included[cy][cx] = True
                        band.zero_planes[cy][cx] = mb - blocks[cx, cy][0]
            coded.append(blocks)
        bw = BitWriter()
        bodies = []
        if not any(coded) and empty_packet == "00":
            bw.put(0)
            packet.empty = True
        else:
            bw.put(1)
            for band, blocks in zip(bands, coded):
                if not (band.w and band.h):
                    continue
                inclusion = TagTree([[0 if inc else 1 for inc in row] for row in band.included])
                big = 1 << 20                                # (the minimum over an excluded block's siblings decides a node)
                zeros = TagTree([[big if z is None else z for z in row] for row in band.zero_planes])
                band.tree_depth = inclusion.depth
                for cy in range(band.ncy):
                    for cx in range(band.ncx):
                        inclusion.encode(bw, cx, cy, 1)
                        if not band.included[cy][cx]:
                            continue
                        planes, passes, body, full, decisions, rect = blocks[cx, cy]
                        zeros.encode(bw, cx, cy, band.zero_planes[cy][cx] + 1)
                        put_passes(bw, passes)
                        grow = passes.bit_length() - 1
                        least = max(0, len(body).bit_length() - (3 + grow))
                        k = least + extra(len(rec.blocks) + len(bodies))
                        bw.bits((1 << k) - 1, k)
                        bw.put(0)
                        bw.bits(len(body), 3 + k + grow)
                        bodies.append((body, passes, planes, band.orient, rect, Segment(body, full, decisions, 3 + k + grow, 3 + k)))
        header, packet.stuffed = bw.finish()
        out += header
        packet.header_end = len(out)
        for body, passes, planes, orient, rect, seg in bodies:
            rec.blocks.append((len(out), len(body), passes, planes, orient, *rect))
            rec.segments.append(seg)
            out += body
        packet.end = len(out)
        rec.packets.append(packet)
    if psot:
        out[sot + 6:sot + 10] = struct.pack(">I", len(out) - sot)
    out += b"\xff\xd9"
    return bytes(out), rec
