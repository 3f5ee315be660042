// JPEG 2000 lossless Pixel Data (transfer syntaxes 1.2.840.10008.1.2.4.90 and .91 with a reversible stream: ITU-T T.800, one
// component, one tile, one quality layer, the 5/3 transform, code-block style 0) -> the native little-endian frame buffer
// pl_dicom_decode reads, next to jpeg_lossless.hip.  The host parses each frame's main header; the packet headers (tier 2,
// T.800 Annex B) are parsed on the host while the file is still host bytes (dicom.load_frames) or here, by j2k_tier2_kernel,
// where the stream lies on the device (dicom.load_zip).  Either way tier 1 sees one descriptor per code block of the whole
// stack (PL_J2K_BLOCK_FIELDS int64 values: frame, segment offset and length, coding passes, magnitude bit planes, subband
// orientation, the rectangle it fills in the frame's coefficient plane; a frame outside 0 .. n_frames - 1 marks a row that
// is not used) and four parameters per frame (decomposition levels, precision, signed, 0).
//
// j2k_tier2_kernel: ONE wave per frame, one launch for the stack, nothing read back (pl_dicom_j2k_plan).
//   input    one int64 row and one byte table per frame say what the host read of the headers (include/pylinac_hip.h);
//            kJ2kHdrWin bytes of the stream at a time go to LDS, a dword per lane, and the reader takes a byte from LDS
//            (readfirstlane): after a byte FF the next one carries 7 bits.  Nothing outside [stream start, tile-part end) is read.
//   packets  dicom.py's _j2k_codestream restated: per resolution the zero-length bit, per non-empty subband (LL | HL, LH, HH)
//            the inclusion and the zero-bit-plane tag tree, the passes (Table B.4), Lblock from 3, the length of
//            Lblock + floor(log2 passes) bits, the header byte-aligned (one stuffed byte after a final FF), then the body.
//   trees    a node is (value, lower bound), two int32 in the frame's slice of d_work, root first; ONE path for every tree
//            size.  The lanes reset a subband's trees together, a workgroup fence follows; on the chain every lane stores
//            the same pair and loads back what it stored itself (ordinary vector loads: the pointer is neither const nor
//            __restrict__).
//   output   the frame owns one row of d_blocks for every code block of its geometry.  An included block's row is written a
//            field per lane while the header is read; at the header's end the packet's rows are read back, checked in the
//            host's order (passes, planes, length) and given their offsets.  The rows left over receive frame = -1, which
//            tier 1 skips; d_info: status, count, two details (the first fault; a flagged frame has no rows).
//
// j2k_tier1_kernel: ONE wave per code block, one launch for the stack, nothing read back.
//   input    kJ2kWin bytes of the segment at a time go to LDS by the dword (aligned global dwords, funnel-shifted by the
//            segment's misalignment; only dwords that hold a byte of the segment are read); the reader takes a dword from LDS
//            (readfirstlane) for every four bytes.
//   MQ       T.800 Annex C in its software form (C.3.2 ff.): A, C and CT in scalar registers.  A context's LDS word IS its
//            row of the probability table (Qe, NMPS, NLPS, SWITCH) with the MPS in bit 31, so a decision costs ONE LDS read
//            on its chain; a state change copies the next row over the context's word off the chain.  FF followed by a byte
//            above 8F ends the data, as does the segment's end: 1-bits are fed from there on.
//   passes   Annex D over stripes of four rows: cleanup on the top plane, then significance propagation, magnitude
//            refinement and cleanup per plane.  The state of a stripe column is ONE LDS word: the significance and the signs
//            of its rows -1 .. 4 (the rows of the stripes above and below are mirrored into it when they change), `visited`
//            and `refined` of its rows 0 .. 3.  A column's contexts come out of three such words (left, own, right) that
//            stay in scalar registers while the walk moves right: one LDS read per stripe column and pass.  Neighbours
//            outside the block are insignificant (a border of zero words).
//   chain    the decoder is ONE wave-uniform chain per block: every lane runs it on the scalar path and all lanes store the
//            same words (idempotent ORs and plain stores), so no lane ever waits for another.  The 64 lanes share the copy of
//            the segment, the clearing of the LDS state and the store of the finished rectangle; they do not share the
//            context work (DESIGN.md section 5.20 says what that costs).
//   output   magnitudes (bit 31: the sign) in LDS; the finished block goes to its rectangle of the frame's int32 plane.
// LDS: 16 KiB magnitudes + 4.6 KiB column words + 1 KiB window + 0.3 KiB tables: 22 KiB a wave.
//
// j2k_idwt_kernel: the inverse reversible 5/3 transform (Annex F.3), one launch per level and axis over the stack, between the
// two planes of a frame in the work buffer (rows: plane 0 -> plane 1, columns: plane 1 -> plane 0; the planes 0 of all frames
// lie together in the buffer's first half, so that one memset clears them and nothing else), a sample per lane.
// j2k_store_kernel: the DC shift of unsigned streams, the clamp to the P-bit range, the container samples into d_native.
//
// A translation unit of its own in the library.  The CPU emulator of the tests builds a fixed list of files, dicom.hip among
// them: there dicom.hip includes this file after pl_common.h (PL_J2K_IN_DICOM), which is why nothing here may collide with
// dicom.hip's, jpeg_lossless.hip's or dicom_encap.hip's names.
#ifndef PL_J2K_IN_DICOM
#include "pl_common.h"
#endif

namespace {

constexpr int kJ2kWin = 1024;                               // bytes of a segment staged at a time
constexpr int kJ2kSide = 64, kJ2kArea = 4096;               // a code block: at most 64 on a side and 4096 samples
constexpr int kJ2kPitch = kJ2kSide + 2;                     // column words of a stripe, with the border columns
constexpr int kJ2kStripes = kJ2kSide / 4 + 2;               // with the border stripes
constexpr int kJ2kMaxPlanes = 30;                           // bit 31 of a magnitude holds the sign
constexpr int kJ2kMaxSegment = 1 << 28;
constexpr int kJ2kF = PL_J2K_BLOCK_FIELDS;

// a stripe column's word: rows -1 .. 4 are bits 0 .. 5 (significance) and 6 .. 11 (sign), rows 0 .. 3 bits 12 .. 15 (visited in
// this bit plane) and 16 .. 19 (refined before)
__device__ __forceinline__ unsigned j2k_sig(int r) { return 1u << (r + 1); }
__device__ __forceinline__ unsigned j2k_sgn(int r) { return 1u << (r + 7); }
__device__ __forceinline__ unsigned j2k_pi(int r) { return 4096u << r; }
__device__ __forceinline__ unsigned j2k_mu(int r) { return 65536u << r; }
constexpr unsigned kJ2kSigAll = 0x3fu, kJ2kPiAll = 0xf000u;

// contexts: 0 .. 8 zero coding, 9 .. 13 sign, 14 .. 16 magnitude refinement, 17 run length, 18 UNIFORM
constexpr int kJ2kCxRun = 17, kJ2kCxUni = 18, kJ2kContexts = 19;

// T.800 Table C.2: Qe | NMPS << 16 | NLPS << 22 | SWITCH << 28
#define PL_J2K_ROW(qe, nmps, nlps, sw) ((unsigned)(qe) | ((unsigned)(nmps) << 16) | ((unsigned)(nlps) << 22) | ((unsigned)(sw) << 28))
__device__ const unsigned kJ2kMqTable[47] = {
    PL_J2K_ROW(0x5601, 1, 1, 1),   PL_J2K_ROW(0x3401, 2, 6, 0),   PL_J2K_ROW(0x1801, 3, 9, 0),   PL_J2K_ROW(0x0AC1, 4, 12, 0),
    PL_J2K_ROW(0x0521, 5, 29, 0),  PL_J2K_ROW(0x0221, 38, 33, 0), PL_J2K_ROW(0x5601, 7, 6, 1),   PL_J2K_ROW(0x5401, 8, 14, 0),
    PL_J2K_ROW(0x4801, 9, 14, 0),  PL_J2K_ROW(0x3801, 10, 14, 0), PL_J2K_ROW(0x3001, 11, 17, 0), PL_J2K_ROW(0x2401, 12, 18, 0),
    PL_J2K_ROW(0x1C01, 13, 20, 0), PL_J2K_ROW(0x1601, 29, 21, 0), PL_J2K_ROW(0x5601, 15, 14, 1), PL_J2K_ROW(0x5401, 16, 14, 0),
    PL_J2K_ROW(0x5101, 17, 15, 0), PL_J2K_ROW(0x4801, 18, 16, 0), PL_J2K_ROW(0x3801, 19, 17, 0), PL_J2K_ROW(0x3401, 20, 18, 0),
    PL_J2K_ROW(0x3001, 21, 19, 0), PL_J2K_ROW(0x2801, 22, 19, 0), PL_J2K_ROW(0x2401, 23, 20, 0), PL_J2K_ROW(0x2201, 24, 21, 0),
    PL_J2K_ROW(0x1C01, 25, 22, 0), PL_J2K_ROW(0x1801, 26, 23, 0), PL_J2K_ROW(0x1601, 27, 24, 0), PL_J2K_ROW(0x1401, 28, 25, 0),
    PL_J2K_ROW(0x1201, 29, 26, 0), PL_J2K_ROW(0x1101, 30, 27, 0), PL_J2K_ROW(0x0AC1, 31, 28, 0), PL_J2K_ROW(0x09C1, 32, 29, 0),
    PL_J2K_ROW(0x08A1, 33, 30, 0), PL_J2K_ROW(0x0521, 34, 31, 0), PL_J2K_ROW(0x0441, 35, 32, 0), PL_J2K_ROW(0x02A1, 36, 33, 0),
    PL_J2K_ROW(0x0221, 37, 34, 0), PL_J2K_ROW(0x0141, 38, 35, 0), PL_J2K_ROW(0x0111, 39, 36, 0), PL_J2K_ROW(0x0085, 40, 37, 0),
    PL_J2K_ROW(0x0049, 41, 38, 0), PL_J2K_ROW(0x0025, 42, 39, 0), PL_J2K_ROW(0x0015, 43, 40, 0), PL_J2K_ROW(0x0009, 44, 41, 0),
    PL_J2K_ROW(0x0005, 45, 42, 0), PL_J2K_ROW(0x0001, 45, 43, 0), PL_J2K_ROW(0x5601, 46, 46, 0)};
#undef PL_J2K_ROW

// the aligned dword at byte `at` (a multiple of 4) of the buffer; a last dword that the buffer holds only in part is read by
// the byte
__device__ __forceinline__ unsigned j2k_dword(const unsigned char* __restrict__ bytes, int64_t nbytes, int64_t at) {
  if (at + 4 <= nbytes) return *reinterpret_cast<const unsigned*>(bytes + at);
  unsigned v = 0;
  for (int k = 0; k < 4; ++k)
    if (at + k < nbytes) v |= (unsigned)bytes[at + k] << (8 * k);
  return v;
}

// the wave-uniform MQ decoder over one segment
struct J2kMq {
  unsigned a, c, cur, word;                                 // cur: the byte at bp; word: the staged dword that holds byte bp + 1
  int ct, bp, len, base;                                    // base: the segment byte the window begins with
  int64_t off;
};

// segment bytes [m.base, m.base + kJ2kWin) -> s_win, all lanes
__device__ __forceinline__ void j2k_stage(const J2kMq& m, const unsigned char* __restrict__ bytes, int64_t nbytes, unsigned* s_win, int lane) {
  const int64_t first = m.off + m.base, end = m.off + m.len;
  const int sh = (int)(first & 3) * 8;
  __syncthreads();
  for (int i = lane; i < kJ2kWin / 4; i += PL_WAVE) {
    const int64_t at = (first & ~(int64_t)3) + 4 * (int64_t)i;
    unsigned v = 0;
    if (at < end) {
      v = j2k_dword(bytes, nbytes, at) >> sh;
      if (sh && at + 4 < end) v |= j2k_dword(bytes, nbytes, at + 4) << (32 - sh);
    }
    s_win[i] = v;
  }
  __syncthreads();
}

// byte p of the segment (p only ever grows by one); beyond the segment: FF
__device__ __forceinline__ unsigned j2k_byte(J2kMq& m, int p, const unsigned char* __restrict__ bytes, int64_t nbytes, unsigned* s_win, int lane) {
  if (p >= m.len) return 0xffu;
  bool fresh = (p & 3) == 0 || p == 0;
  if (p >= m.base + kJ2kWin) {
    m.base = p & ~3;
    j2k_stage(m, bytes, nbytes, s_win, lane);
    fresh = true;
  }
  const int q = p - m.base;
  if (fresh) m.word = __builtin_amdgcn_readfirstlane(s_win[q >> 2]);
  return (m.word >> (8 * (q & 3))) & 0xffu;
}

#define PL_J2K_IO bytes, nbytes, s_win, lane

__device__ __forceinline__ void j2k_bytein(J2kMq& m, const unsigned char* __restrict__ bytes, int64_t nbytes, unsigned* s_win, int lane) {
  // (a byte is looked at once: the reader's dword follows bp + 1)
  if (m.cur == 0xffu) {
    const unsigned nx = m.bp + 1 < m.len ? j2k_byte(m, m.bp + 1, PL_J2K_IO) : 0xffu;
    if (nx > 0x8fu) {
      m.c += 0xff00u, m.ct = 8;                             // a marker, or the segment's end: 1-bits from here on
      if (m.bp + 1 < m.len) m.len = m.bp + 1;               // (the marker's byte is not taken again)
    } else {
      ++m.bp, m.cur = nx, m.c += nx << 9, m.ct = 7;
    }
  } else if (m.bp + 1 < m.len) {
    const unsigned nx = j2k_byte(m, m.bp + 1, PL_J2K_IO);
    ++m.bp, m.cur = nx, m.c += nx << 8, m.ct = 8;
  } else {
    m.bp = m.len, m.cur = 0xffu, m.c += 0xff00u, m.ct = 8;
  }
}

__device__ __forceinline__ unsigned j2k_decode(J2kMq& m, int cx, unsigned* s_cx, const unsigned* s_rows,
                                               const unsigned char* __restrict__ bytes, int64_t nbytes, unsigned* s_win, int lane) {
  const unsigned e = __builtin_amdgcn_readfirstlane(s_cx[cx]);
  const unsigned qe = e & 0xffffu;
  unsigned d = e >> 31;
  bool lps;                                                 // the state moves along NLPS
  m.a -= qe;
  if ((m.c >> 16) < qe) {
    lps = m.a >= qe;
    m.a = qe;
  } else {
    m.c -= qe << 16;
    if (m.a & 0x8000u) return d;
    lps = m.a < qe;
  }
  unsigned mps = d;
  if (lps) d ^= 1u, mps ^= (e >> 28) & 1u;
  const unsigned next = lps ? (e >> 22) & 63u : (e >> 16) & 63u;
  s_cx[cx] = s_rows[next] | (mps << 31);
  do {
    if (m.ct == 0) j2k_bytein(m, PL_J2K_IO);
    m.a <<= 1, m.c <<= 1, --m.ct;
  } while (!(m.a & 0x8000u));
  return d;
}

// the zero-coding context (Table D.1) from the sums of significant horizontal, vertical and diagonal neighbours
__device__ __forceinline__ int j2k_zc(int orient, int h, int v, int d) {
  if (orient == 3) {
    const int hv = h + v;
    if (d >= 3) return 8;
    if (d == 2) return hv >= 1 ? 7 : 6;
    if (d == 1) return hv >= 2 ? 5 : hv == 1 ? 4 : 3;
    return hv >= 2 ? 2 : hv;
  }
  if (orient == 1) {                                        // HL: the roles of the two axes are exchanged
    const int t = h;
    h = v, v = t;
  }
  if (h == 2) return 8;
  if (h == 1) return v >= 1 ? 7 : d >= 1 ? 6 : 5;
  if (v == 2) return 4;
  if (v == 1) return 3;
  return d >= 2 ? 2 : d;
}

// +1 / -1 / 0: what the neighbour in row r of column word w adds to a sign context (Table D.2)
__device__ __forceinline__ int j2k_chi(unsigned w, int r) {
  return (int)((w >> (r + 1)) & 1u) * (1 - 2 * (int)((w >> (r + 7)) & 1u));
}

struct J2kBlock {
  int w, h, orient, bp;                                     // bp: the bit plane being decoded
  unsigned* s_flags;
  unsigned* s_mag;
  unsigned* s_cx;
  const unsigned* s_rows;
};

// the neighbour sums of row r of the column between wl and wr
__device__ __forceinline__ void j2k_sums(unsigned wl, unsigned wc, unsigned wr, int r, int& h, int& v, int& d) {
  const unsigned l3 = wl >> r, c3 = wc >> r, r3 = wr >> r;
  h = (int)((l3 >> 1) & 1u) + (int)((r3 >> 1) & 1u);
  v = (int)(c3 & 1u) + (int)((c3 >> 2) & 1u);
  d = (int)(l3 & 1u) + (int)((l3 >> 2) & 1u) + (int)(r3 & 1u) + (int)((r3 >> 2) & 1u);
}

// row r of column x in stripe s becomes significant: its sign (D.3.2), its first magnitude bit, the mirrored rows
__device__ __forceinline__ void j2k_become(const J2kBlock& b, J2kMq& m, int s, int x, int r, unsigned wl, unsigned& wc, unsigned wr,
                                           const unsigned char* __restrict__ bytes, int64_t nbytes, unsigned* s_win, int lane) {
  int hc = j2k_chi(wl, r) + j2k_chi(wr, r), vc = j2k_chi(wc, r - 1) + j2k_chi(wc, r + 1);
  hc = hc > 1 ? 1 : hc < -1 ? -1 : hc;
  vc = vc > 1 ? 1 : vc < -1 ? -1 : vc;
  unsigned flip = 0;
  if (hc < 0 || (hc == 0 && vc < 0)) flip = 1u, hc = -hc, vc = -vc;
  const int cx = hc == 1 ? 12 + vc : 9 + vc;
  const unsigned neg = j2k_decode(m, cx, b.s_cx, b.s_rows, PL_J2K_IO) ^ flip;
  wc |= j2k_sig(r) | (neg ? j2k_sgn(r) : 0u);
  b.s_mag[(4 * s + r) * b.w + x] = (1u << b.bp) | (neg << 31);
  if (r == 0) b.s_flags[s * kJ2kPitch + 1 + x] |= j2k_sig(4) | (neg ? j2k_sgn(4) : 0u);
  if (r == 3) b.s_flags[(s + 2) * kJ2kPitch + 1 + x] |= j2k_sig(-1) | (neg ? j2k_sgn(-1) : 0u);
}

// one coding pass over the block: PASS 0 significance propagation, 1 magnitude refinement, 2 cleanup (D.3.1, D.3.3, D.3.4)
template <int PASS>
__device__ __forceinline__ void j2k_pass(const J2kBlock& b, J2kMq& m, const unsigned char* __restrict__ bytes, int64_t nbytes,
                                         unsigned* s_win, int lane) {
  for (int s = 0; 4 * s < b.h; ++s) {
    const int nrows = b.h - 4 * s < 4 ? b.h - 4 * s : 4;
    unsigned* row = b.s_flags + (s + 1) * kJ2kPitch + 1;
    unsigned wl = 0, wc = __builtin_amdgcn_readfirstlane(row[0]);
    for (int x = 0; x < b.w; ++x) {
      const unsigned wr = x + 1 < b.w ? __builtin_amdgcn_readfirstlane(row[x + 1]) : 0u;
      const unsigned before = wc;
      if (PASS == 0) {
        if ((wl | wc | wr) & kJ2kSigAll) {
          for (int r = 0; r < nrows; ++r) {
            if (wc & j2k_sig(r)) continue;
            int h, v, d;
            j2k_sums(wl, wc, wr, r, h, v, d);
            if (h + v + d == 0) continue;
            wc |= j2k_pi(r);
            if (j2k_decode(m, j2k_zc(b.orient, h, v, d), b.s_cx, b.s_rows, PL_J2K_IO)) j2k_become(b, m, s, x, r, wl, wc, wr, PL_J2K_IO);
          }
        }
      } else if (PASS == 1) {
        for (int r = 0; r < nrows; ++r) {
          if (!(wc & j2k_sig(r)) || (wc & j2k_pi(r))) continue;
          int h, v, d;
          j2k_sums(wl, wc, wr, r, h, v, d);
          const int cx = (wc & j2k_mu(r)) ? 16 : h + v + d ? 15 : 14;
          const unsigned bit = j2k_decode(m, cx, b.s_cx, b.s_rows, PL_J2K_IO);
          b.s_mag[(4 * s + r) * b.w + x] |= bit << b.bp;
          wc |= j2k_mu(r);
        }
      } else {
        int r = 0;
        bool coded = true;
        if (nrows == 4 && !((wl | wc | wr) & kJ2kSigAll)) {  // four insignificant samples with no significant neighbour
          if (!j2k_decode(m, kJ2kCxRun, b.s_cx, b.s_rows, PL_J2K_IO)) {
            coded = false;
          } else {
            r = (int)j2k_decode(m, kJ2kCxUni, b.s_cx, b.s_rows, PL_J2K_IO) << 1;
            r |= (int)j2k_decode(m, kJ2kCxUni, b.s_cx, b.s_rows, PL_J2K_IO);
            j2k_become(b, m, s, x, r, wl, wc, wr, PL_J2K_IO);
            ++r;
          }
        }
        for (; coded && r < nrows; ++r) {
          if (wc & (j2k_sig(r) | j2k_pi(r))) continue;
          int h, v, d;
          j2k_sums(wl, wc, wr, r, h, v, d);
          if (j2k_decode(m, j2k_zc(b.orient, h, v, d), b.s_cx, b.s_rows, PL_J2K_IO)) j2k_become(b, m, s, x, r, wl, wc, wr, PL_J2K_IO);
        }
        wc &= ~kJ2kPiAll;
      }
      if (wc != before) row[x] = wc;
      wl = wc, wc = wr;
    }
  }
}

__global__ void __launch_bounds__(PL_WAVE)
j2k_tier1_kernel(const unsigned char* __restrict__ bytes, int64_t nbytes, const int64_t* __restrict__ blocks, int64_t n_frames,
                 int rows, int cols, int32_t* __restrict__ planes, int32_t* __restrict__ status) {
  __shared__ unsigned s_mag[kJ2kArea];
  __shared__ unsigned s_flags[kJ2kStripes * kJ2kPitch];
  __shared__ unsigned s_win[kJ2kWin / 4];
  __shared__ unsigned s_rows[48];
  __shared__ unsigned s_cx[kJ2kContexts + 1];
  const int lane = threadIdx.x;
  const int64_t* q = blocks + (int64_t)blockIdx.x * kJ2kF;
  const int64_t f = q[0], off = q[1], len = q[2], passes = q[3], nplanes = q[4], orient = q[5], x0 = q[6], y0 = q[7], w = q[8], h = q[9];
  if (f < 0 || f >= n_frames) return;                       // no frame to flag: nothing is read or stored
  // (differences of lengths, never sums of an offset and a length: nothing here can overflow)
  bool bad = off < 0 || len < 0 || off > nbytes || len > nbytes - off || len > kJ2kMaxSegment;
  bad = bad || w < 1 || h < 1 || w > kJ2kSide || h > kJ2kSide || x0 < 0 || y0 < 0 || x0 > cols - w || y0 > rows - h;
  bad = bad || orient < 0 || orient > 3 || nplanes < 1 || nplanes > kJ2kMaxPlanes || passes != 3 * nplanes - 2;
  if (bad) {
    if (lane == 0) atomicOr(&status[f], 1);
    return;
  }
  for (int i = lane; i < (int)(w * h); i += PL_WAVE) s_mag[i] = 0;
  for (int i = lane; i < kJ2kStripes * kJ2kPitch; i += PL_WAVE) s_flags[i] = 0;
  if (lane < 47) s_rows[lane] = kJ2kMqTable[lane];
  if (lane < kJ2kContexts) s_cx[lane] = kJ2kMqTable[lane == 0 ? 4 : lane == kJ2kCxRun ? 3 : lane == kJ2kCxUni ? 46 : 0];
  J2kMq m;
  m.off = off, m.len = (int)len, m.base = 0, m.word = 0, m.bp = 0;
  j2k_stage(m, bytes, nbytes, s_win, lane);                 // (its barriers close the initialisation above as well)
  // ---- INITDEC (C.3.5) ------------------------------------------------------------------------------------------------------
  m.cur = m.len > 0 ? j2k_byte(m, 0, PL_J2K_IO) : 0xffu;
  m.c = m.cur << 16;
  m.ct = 0;
  j2k_bytein(m, PL_J2K_IO);
  m.c <<= 7, m.ct -= 7, m.a = 0x8000u;
  // ---- the passes -----------------------------------------------------------------------------------------------------------
  J2kBlock b;
  b.w = (int)w, b.h = (int)h, b.orient = (int)orient, b.s_flags = s_flags, b.s_mag = s_mag, b.s_cx = s_cx, b.s_rows = s_rows;
  b.bp = (int)nplanes - 1;
  j2k_pass<2>(b, m, PL_J2K_IO);
  for (b.bp = (int)nplanes - 2; b.bp >= 0; --b.bp) {
    j2k_pass<0>(b, m, PL_J2K_IO);
    j2k_pass<1>(b, m, PL_J2K_IO);
    j2k_pass<2>(b, m, PL_J2K_IO);
  }
  __syncthreads();
  // ---- the rectangle --------------------------------------------------------------------------------------------------------
  int32_t* out = planes + f * ((int64_t)rows * cols);
  for (int i = lane; i < b.w * b.h; i += PL_WAVE) {
    const unsigned v = s_mag[i];
    const int y = i / b.w, x = i - y * b.w, mag = (int)(v & 0x7fffffffu);
    out[(y0 + y) * cols + x0 + x] = (v >> 31) ? -mag : mag;
  }
}

#undef PL_J2K_IO

// One level of the inverse 5/3 transform along one axis (F.3.8.2 with the whole-sample symmetric extension of F.3.7) for the
// frames that have at least `level` levels: the rw x rh region of src (low band first, ceil(n / 2) samples, then the high band)
// -> the same region of dst, interleaved.
__global__ void __launch_bounds__(256)
j2k_idwt_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst, const int32_t* __restrict__ params, int level,
                int rows, int cols, int rw, int rh, int horizontal) {
  const int64_t f = blockIdx.y;
  const int levels = params[f * 4];
  if (levels < level || levels > PL_J2K_MAX_LEVELS) return;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)rw * rh) return;
  const int y = (int)(idx / rw), x = (int)(idx - (int64_t)y * rw);
  const int64_t frame = f * ((int64_t)rows * cols);
  const int n = horizontal ? rw : rh, pos = horizontal ? x : y;
  const int64_t stride = horizontal ? 1 : cols, base = frame + (horizontal ? (int64_t)y * cols : x);
  const int nl = (n + 1) >> 1, nh = n >> 1;
  const int32_t* lo = src + base;
  const int32_t* hi = src + base + nl * stride;
  int out;
  if (nh == 0) {
    out = lo[0];                                            // one sample: it passes through
  } else {
    auto even = [&](int k) {                                // x[2k]; x[-1] = x[1], x[n] = x[n - 2]
      const int a = hi[(k ? k - 1 : 0) * stride], c = hi[(k < nh ? k : nh - 1) * stride];
      return lo[k * stride] - ((a + c + 2) >> 2);
    };
    const int k = pos >> 1;
    if (!(pos & 1)) {
      out = even(k);
    } else {
      const int e0 = even(k), e1 = k + 1 < nl ? even(k + 1) : e0;
      out = hi[k * stride] + ((e0 + e1) >> 1);
    }
  }
  dst[base + pos * stride] = out;
}

// plane 0 of every frame -> d_native: the DC shift 2^(P - 1) of unsigned streams, the clamp to the P-bit range
__global__ void __launch_bounds__(256)
j2k_store_kernel(const int32_t* __restrict__ planes, const int32_t* __restrict__ params, int max_levels, int rows, int cols, int bps,
                 unsigned char* __restrict__ native, int32_t* __restrict__ status) {
  const int64_t f = blockIdx.y;
  const int levels = params[f * 4], prec = params[f * 4 + 1], sgn = params[f * 4 + 2];
  if (levels < 0 || levels > max_levels || prec < 1 || prec > 8 * bps || (sgn != 0 && sgn != 1)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&status[f], 1);
    return;
  }
  const int64_t size = (int64_t)rows * cols, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= size) return;
  const int half = 1 << (prec - 1);
  int v = planes[f * size + i] + (sgn ? 0 : half);
  const int lo = sgn ? -half : 0, top = sgn ? half - 1 : 2 * half - 1;
  v = v < lo ? lo : v > top ? top : v;
  unsigned char* out = native + f * size * bps;
  if (bps == 1) out[i] = (unsigned char)v;
  else if (((uintptr_t)out & 1u) == 0) reinterpret_cast<unsigned short*>(out)[i] = (unsigned short)v;
  else out[2 * i] = (unsigned char)v, out[2 * i + 1] = (unsigned char)((unsigned)v >> 8);
}

// ---- tier 2: the packet headers --------------------------------------------------------------------------------------------
constexpr int kJ2kPlanF = PL_J2K_PLAN_FIELDS, kJ2kPlanT = PL_J2K_PLAN_TABLE;
constexpr int kJ2kHdrWin = 256;                             // bytes of the stream staged at a time (a dword per lane)
constexpr int64_t kJ2kMaxStream = 1 << 27;                  // bytes of a frame's window: a tag-tree value stays below kJ2kOpen
constexpr int kJ2kOpen = 1 << 30;                           // the value of a tag-tree node no 1-bit has settled yet
constexpr int64_t kJ2kLong = (int64_t)1 << 40;              // a segment length is followed exactly up to here

// the bits of a packet header (B.10.1), most significant first: after a byte FF the next byte carries 7 bits
struct __attribute__((aligned(8))) J2kNode {                 // a tag-tree node: its value (kJ2kOpen until known), the lower bound read so far
  int value, low;
};

struct J2kBits {
  int64_t pos, end, base;                                   // base: the byte the staged window begins with
  unsigned buf;
  int ct;
  bool dry;                                                 // a bit beyond `end` was asked for (it reads as 0)
};

#define PL_J2K_HDR bytes, s_hdr, lane

__device__ __forceinline__ unsigned j2k_hdr_bit(J2kBits& b, const unsigned char* __restrict__ bytes, unsigned* s_hdr, int lane) {
  if (b.ct == 0) {
    if (b.pos >= b.end) {
      b.dry = true;
      return 0u;
    }
    if (b.pos >= b.base + kJ2kHdrWin) {                     // (pos only ever grows)
      b.base = b.pos;
      __syncthreads();
      unsigned v = 0;
      for (int k = 0; k < 4; ++k) {
        const int64_t at = b.base + 4 * lane + k;
        if (at < b.end) v |= (unsigned)bytes[at] << (8 * k);
      }
      s_hdr[lane] = v;
      __syncthreads();
    }
    const int q = (int)(b.pos - b.base);
    b.ct = b.buf == 0xffu ? 7 : 8;
    b.buf = (__builtin_amdgcn_readfirstlane(s_hdr[q >> 2]) >> (8 * (q & 3))) & 0xffu;
    ++b.pos;
  }
  --b.ct;
  return (b.buf >> b.ct) & 1u;
}

__device__ __forceinline__ int64_t j2k_hdr_bits(J2kBits& b, int n, const unsigned char* __restrict__ bytes, unsigned* s_hdr, int lane) {
  int64_t v = 0;
  for (int i = 0; i < n && !b.dry; ++i) {
    const int64_t bit = j2k_hdr_bit(b, PL_J2K_HDR);
    v = v >= kJ2kLong ? v : (v << 1) | bit;                 // (a length beyond 2^40 reaches beyond every tile-part)
  }
  return v;
}

// The nodes of the tag tree over w x h leaves (B.10.2) lie root first: a level's nodes follow those of the level above.
__device__ __forceinline__ int j2k_tree_levels(int w, int h) {
  int n = 1;
  while (((w + (1 << (n - 1)) - 1) >> (n - 1)) > 1 || ((h + (1 << (n - 1)) - 1) >> (n - 1)) > 1) ++n;
  return n;
}

__device__ __forceinline__ int64_t j2k_tree_nodes(int w, int h) {
  int64_t n = 0;
  for (int l = j2k_tree_levels(w, h) - 1; l >= 0; --l) n += (int64_t)((w + (1 << l) - 1) >> l) * ((h + (1 << l) - 1) >> l);
  return n;
}

// whether the value of leaf (x, y) is below `threshold`, reading only the bits that settles.  A node is (value, lower bound);
// every lane stores the same pair and loads back what it stored itself.
__device__ __forceinline__ bool j2k_tag(J2kNode* tree, int w, int h, int levels, int x, int y, int threshold, J2kBits& b,
                                        const unsigned char* __restrict__ bytes, unsigned* s_hdr, int lane) {
  int low = 0, value = kJ2kOpen, off = 0;
  for (int l = levels - 1; l >= 0; --l) {
    const int wl = (w + (1 << l) - 1) >> l, hl = (h + (1 << l) - 1) >> l;
    const int at = off + (y >> l) * wl + (x >> l);
    const J2kNode node = tree[at];
    value = __builtin_amdgcn_readfirstlane(node.value);
    const int known = __builtin_amdgcn_readfirstlane(node.low);
    low = low > known ? low : known;
    while (low < threshold && low < value && !b.dry) {
      if (j2k_hdr_bit(b, PL_J2K_HDR)) value = low;
      else ++low;
    }
    tree[at] = J2kNode{value, low};
    off += wl * hl;
  }
  return value < threshold;
}

// the number of coding passes of a code block (Table B.4): codewords for 1, 2, 3 .. 5, 6 .. 36, 37 .. 164
__device__ __forceinline__ int j2k_hdr_passes(J2kBits& b, const unsigned char* __restrict__ bytes, unsigned* s_hdr, int lane) {
  if (!j2k_hdr_bit(b, PL_J2K_HDR)) return 1;
  if (!j2k_hdr_bit(b, PL_J2K_HDR)) return 2;
  int v = (int)j2k_hdr_bits(b, 2, PL_J2K_HDR);
  if (v < 3) return 3 + v;
  v = (int)j2k_hdr_bits(b, 5, PL_J2K_HDR);
  return v < 31 ? 6 + v : 37 + (int)j2k_hdr_bits(b, 7, PL_J2K_HDR);
}

// what the plan states of resolution r: the code-block size, or false for more than one precinct / an exponent 0 above r = 0
__device__ __forceinline__ bool j2k_res_blocks(const unsigned char* __restrict__ table, bool stated, int r, int rw, int rh, int xcb, int ycb,
                                               int& cbw, int& cbh) {
  const int ppx = stated ? table[49 + r] & 15 : 15, ppy = stated ? table[49 + r] >> 4 : 15;
  if (((rw + (1 << ppx) - 1) >> ppx) > 1 || ((rh + (1 << ppy) - 1) >> ppy) > 1) return false;
  if (r && (ppx == 0 || ppy == 0)) return false;
  const int px = ppx - (r > 0), py = ppy - (r > 0);
  cbw = 1 << (xcb < px ? xcb : px), cbh = 1 << (ycb < py ? ycb : py);
  return true;
}

// band b (0 .. 2; at r = 0 only 0) of resolution r -> orientation, origin and size in the coefficient plane
__device__ __forceinline__ void j2k_band(int r, int k, int rw, int rh, int lw, int lh, int& orient, int& bx, int& by, int& bw, int& bh) {
  if (r == 0) orient = 0, bx = 0, by = 0, bw = rw, bh = rh;
  else if (k == 0) orient = 1, bx = lw, by = 0, bw = rw - lw, bh = lh;
  else if (k == 1) orient = 2, bx = 0, by = lh, bw = lw, bh = rh - lh;
  else orient = 3, bx = lw, by = lh, bw = rw - lw, bh = rh - lh;
}

// ONE wave per frame, a wave-uniform chain as tier 1: the frame's packet headers (Annex B: one packet per resolution of the one
// tile, one precinct, one layer) -> its rows of d_blocks and its row of d_info.  `work`: two trees of max_nodes (value, lower
// bound) pairs per frame, written and read back inside this launch (hence no __restrict__ and no const on it or on `blocks`).
__global__ void __launch_bounds__(PL_WAVE)
j2k_tier2_kernel(const unsigned char* __restrict__ bytes, int64_t nbytes, const int64_t* __restrict__ plan,
                 const unsigned char* __restrict__ tables, int rows, int cols, int64_t* blocks, int64_t n_blocks,
                 int32_t* __restrict__ info, J2kNode* work, int64_t max_nodes) {
  __shared__ unsigned s_hdr[kJ2kHdrWin / 4];
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x;
  const int64_t* p = plan + f * kJ2kPlanF;
  const unsigned char* table = tables + f * kJ2kPlanT;
  const int64_t start = p[0], len = p[1], first = p[2], stated_end = p[3], coding = p[4], row0 = p[5], nrows = p[6];
  const int levels = (int)(coding & 255), xcb = (int)((coding >> 8) & 255), ycb = (int)((coding >> 16) & 255);
  const int guard = (int)((coding >> 24) & 255);
  const bool stated = (coding >> 32) & 1;
  int32_t* out = info + f * 4;
  // ---- the plan row (differences of lengths, never sums of an offset and a length) ------------------------------------------
  bool bad = start < 0 || len < 0 || start > nbytes || len > nbytes - start || len > kJ2kMaxStream;
  bad = bad || first < 0 || first > len || stated_end < 0 || stated_end > len || (stated_end && first > stated_end);
  bad = bad || (coding >> 33) != 0 || levels > PL_J2K_MAX_LEVELS || xcb < 2 || ycb < 2 || xcb > 6 || ycb > 6 || guard > 7;
  bad = bad || row0 < 0 || nrows < 0 || row0 > n_blocks || nrows > n_blocks - row0 || p[7] != 0;
  int64_t count = 0;
  for (int r = 0; !bad && r <= levels; ++r) {                // every code block of the geometry has a row
    const int d = levels - r, rw = (cols + (1 << d) - 1) >> d, rh = (rows + (1 << d) - 1) >> d;
    const int lw = (cols + (2 << d) - 1) >> (d + 1), lh = (rows + (2 << d) - 1) >> (d + 1);
    int cbw, cbh;
    bad = !j2k_res_blocks(table, stated, r, rw, rh, xcb, ycb, cbw, cbh);
    for (int k = 0; !bad && k < (r ? 3 : 1); ++k) {
      int orient, bx, by, bw, bh;
      j2k_band(r, k, rw, rh, lw, lh, orient, bx, by, bw, bh);
      if (bw == 0 || bh == 0) continue;
      const int ncx = (bw + cbw - 1) / cbw, ncy = (bh + cbh - 1) / cbh;
      bad = table[r ? 3 * r - 3 + orient : 0] > 31 || j2k_tree_nodes(ncx, ncy) > max_nodes;
      count += (int64_t)ncx * ncy;
    }
  }
  bad = bad || count != nrows;
  int64_t end = start + (stated_end ? stated_end : len);
  if (!bad && !stated_end) {                                 // Psot = 0: up to EOC, which an item's pad byte may follow
    const unsigned b1 = len >= 1 ? bytes[start + len - 1] : 0u, b2 = len >= 2 ? bytes[start + len - 2] : 0u;
    const unsigned b3 = len >= 3 ? bytes[start + len - 3] : 0u;
    if (len >= 2 && b2 == 0xffu && b1 == 0xd9u) end -= 2;
    else if (len >= 3 && b3 == 0xffu && b2 == 0xd9u) end -= 3;
    end = __builtin_amdgcn_readfirstlane((int)(end - start)) + start;
    bad = start + first > end;
  }
  if (bad) {                                                 // nothing but the status is written
    if (lane == 0) out[0] = 1, out[1] = 0, out[2] = 0, out[3] = 0;
    return;
  }
  // ---- the packets ----------------------------------------------------------------------------------------------------------
  int64_t* mine = blocks + row0 * kJ2kF;
  J2kNode* inclusion = work + f * 2 * max_nodes;
  J2kNode* zero_planes = inclusion + max_nodes;
  J2kBits b;
  b.pos = start + first, b.end = end, b.base = b.pos - kJ2kHdrWin, b.dry = false;
  int status = 0, detail0 = 0, detail1 = 0;
  int64_t done = 0;                                          // rows filled by the packets before this one
  for (int r = 0; !status && r <= levels; ++r) {
    const int d = levels - r, rw = (cols + (1 << d) - 1) >> d, rh = (rows + (1 << d) - 1) >> d;
    const int lw = (cols + (2 << d) - 1) >> (d + 1), lh = (rows + (2 << d) - 1) >> (d + 1);
    int cbw = 0, cbh = 0;
    j2k_res_blocks(table, stated, r, rw, rh, xcb, ycb, cbw, cbh);
    b.buf = 0, b.ct = 0;
    int64_t found = done;
    if (j2k_hdr_bit(b, PL_J2K_HDR)) {                        // (0: an empty packet)
      for (int k = 0; !b.dry && k < (r ? 3 : 1); ++k) {
        int orient, bx, by, bw, bh;
        j2k_band(r, k, rw, rh, lw, lh, orient, bx, by, bw, bh);
        if (bw == 0 || bh == 0) continue;
        const int exponent = table[r ? 3 * r - 3 + orient : 0];
        const int ncx = (bw + cbw - 1) / cbw, ncy = (bh + cbh - 1) / cbh;
        const int tl = j2k_tree_levels(ncx, ncy);
        const int nodes = (int)j2k_tree_nodes(ncx, ncy);
        __syncthreads();
        for (int i = lane; i < nodes; i += PL_WAVE) inclusion[i] = J2kNode{kJ2kOpen, 0}, zero_planes[i] = J2kNode{kJ2kOpen, 0};
        __syncthreads();
        for (int cy = 0; !b.dry && cy < ncy; ++cy) {
          for (int cx = 0; !b.dry && cx < ncx; ++cx) {
            if (!j2k_tag(inclusion, ncx, ncy, tl, cx, cy, 1, b, PL_J2K_HDR)) continue;
            int z = 1;
            while (!b.dry && !j2k_tag(zero_planes, ncx, ncy, tl, cx, cy, z, b, PL_J2K_HDR)) ++z;
            const int passes = j2k_hdr_passes(b, PL_J2K_HDR);
            int lblock = 3;
            while (j2k_hdr_bit(b, PL_J2K_HDR)) ++lblock;
            for (int v = passes; v > 1; v >>= 1) ++lblock;    // + floor(log2 passes) bits
            const int64_t length = j2k_hdr_bits(b, lblock, PL_J2K_HDR);
            if (b.dry) break;
            const int x0 = bx + cx * cbw, y0 = by + cy * cbh;
            const int w = cbw < bw - cx * cbw ? cbw : bw - cx * cbw, h = cbh < bh - cy * cbh ? cbh : bh - cy * cbh;
            // the row, a field per lane (the offset follows once the header's end is known)
            const int64_t v = lane == 0 ? f : lane == 2 ? length : lane == 3 ? passes : lane == 4 ? guard + exponent - z :
                              lane == 5 ? orient : lane == 6 ? x0 : lane == 7 ? y0 : lane == 8 ? w : lane == 9 ? h : 0;
            if (lane < kJ2kF) mine[found * kJ2kF + lane] = v;
            ++found;
          }
        }
      }
    }
    // the header's end: the rest of its last byte is dropped, and a last byte FF is followed by one stuffed byte
    if (!b.dry && b.buf == 0xffu) {
      if (b.pos >= b.end) b.dry = true;
      else ++b.pos;
    }
    if (b.dry) {
      status = 2, detail0 = r;
      break;
    }
    __syncthreads();                                         // (the rows above: written a field per lane, read by every lane)
    for (int64_t i = done; !status && i < found; ++i) {      // the packet's body: the segments in the order of their blocks
      const int64_t* q = mine + i * kJ2kF;
      const int64_t length = q[2];
      const int passes = __builtin_amdgcn_readfirstlane((int)q[3]), nplanes = __builtin_amdgcn_readfirstlane((int)q[4]);
      const int lo = __builtin_amdgcn_readfirstlane((int)length), hi = __builtin_amdgcn_readfirstlane((int)(length >> 32));
      const int64_t seg = ((int64_t)hi << 32) | (unsigned)lo;
      if (passes != 3 * nplanes - 2 || nplanes < 1) status = 4, detail0 = passes, detail1 = nplanes;
      else if (nplanes > kJ2kMaxPlanes) status = 8, detail0 = nplanes;
      else if (seg > b.end - b.pos) status = 16;
      else {
        if (lane == 0) mine[i * kJ2kF + 1] = b.pos;
        b.pos += seg;
      }
    }
    done = found;
  }
  if (status) done = 0;                                      // a flagged frame has no rows
  __syncthreads();                                           // (a row's fields were written by other lanes than the one that fills it)
  for (int64_t i = done + lane; i < nrows; i += PL_WAVE) mine[i * kJ2kF] = -1;
  if (lane == 0) out[0] = status, out[1] = (int32_t)done, out[2] = detail0, out[3] = detail1;
}

#undef PL_J2K_HDR

}  // namespace

extern "C" int64_t pl_dicom_j2k_plan_work_bytes(int64_t n_frames, int64_t max_nodes) {
  if (n_frames < 1 || n_frames > 65535 || max_nodes < 1 || max_nodes > (1 << 24)) return -1;
  return n_frames * max_nodes * 16;                         // two trees a frame, a node is two int32 values
}

extern "C" int pl_dicom_j2k_plan(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_plan, const unsigned char* d_tables,
                                 int64_t n_frames, int rows, int cols, int64_t* d_blocks, int64_t n_blocks, int32_t* d_info,
                                 void* d_work, int64_t max_nodes, void* stream) {
  PL_REQUIRE(d_bytes && d_plan && d_tables && d_info && d_work, "null pointer");
  PL_REQUIRE(n_blocks == 0 || d_blocks, "null pointer");
  PL_REQUIRE(n_frames >= 1 && n_frames <= 65535, "1 <= n_frames <= 65535");
  PL_REQUIRE(n_blocks >= 0 && n_blocks < 2147483647, "0 <= n_blocks < 2^31");
  PL_REQUIRE(rows >= 1 && cols >= 1 && rows <= 65535 && cols <= 65535 && nbytes >= 0, "bad shape");
  PL_REQUIRE(max_nodes >= 1 && max_nodes <= (1 << 24), "1 <= max_nodes <= 2^24");
  PL_REQUIRE(((uintptr_t)d_work & 15u) == 0, "d_work on a 16-byte boundary");
  hipLaunchKernelGGL(j2k_tier2_kernel, dim3((unsigned)n_frames), dim3(PL_WAVE), 0, (hipStream_t)stream, d_bytes, nbytes, d_plan,
                     d_tables, rows, cols, d_blocks, n_blocks, d_info, (J2kNode*)d_work, max_nodes);
  return pl_check_launch("pl_dicom_j2k_plan");
}

extern "C" int64_t pl_dicom_j2k_work_bytes(int64_t n_frames, int rows, int cols) {
  if (n_frames < 1 || n_frames > 65535 || rows < 1 || cols < 1 || rows > 65535 || cols > 65535) return -1;
  return n_frames * 2 * (int64_t)rows * cols * 4;          // two int32 planes a frame: [2][n_frames][rows * cols]
}

extern "C" int pl_dicom_j2k_decode(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_blocks, int64_t n_blocks,
                                   const int32_t* d_params, int64_t n_frames, int max_levels, int rows, int cols,
                                   int bytes_per_sample, unsigned char* d_native, int32_t* d_status, void* d_work, void* stream) {
  if (bytes_per_sample != 1 && bytes_per_sample != 2) {
    pl_set_error("pl_dicom_j2k_decode: unsupported bytes_per_sample %d (BitsAllocated 8 or 16)", bytes_per_sample);
    return PL_ERR_UNSUPPORTED;
  }
  if (max_levels > PL_J2K_MAX_LEVELS) {
    pl_set_error("pl_dicom_j2k_decode: unsupported max_levels %d (at most %d decomposition levels)", max_levels, PL_J2K_MAX_LEVELS);
    return PL_ERR_UNSUPPORTED;
  }
  PL_REQUIRE(d_bytes && d_params && d_native && d_status && d_work, "null pointer");
  PL_REQUIRE(n_blocks == 0 || d_blocks, "null pointer");
  PL_REQUIRE(n_frames >= 1 && n_frames <= 65535, "1 <= n_frames <= 65535");
  PL_REQUIRE(n_blocks >= 0 && n_blocks < 2147483647, "0 <= n_blocks < 2^31");
  PL_REQUIRE(rows >= 1 && cols >= 1 && rows <= 65535 && cols <= 65535 && nbytes >= 0 && max_levels >= 0, "bad shape");
  PL_REQUIRE(((uintptr_t)d_bytes & 3u) == 0 && ((uintptr_t)d_work & 15u) == 0, "d_bytes on a 4-byte and d_work on a 16-byte boundary");
  hipStream_t st = (hipStream_t)stream;
  const int64_t size = (int64_t)rows * cols;
  int32_t* planes = (int32_t*)d_work;
  // (the planes 0, the buffer's first half, are zeroed: a block that is not included has the coefficient 0; a plane 1 is
  // written before it is read)
  if (hipMemsetAsync(d_status, 0, (size_t)n_frames * 4, st) != hipSuccess ||
      hipMemsetAsync(d_work, 0, (size_t)(n_frames * size * 4), st) != hipSuccess) {
    pl_set_error("pl_dicom_j2k_decode: memset failed");
    return PL_ERR_HIP;
  }
  if (n_blocks > 0)
    hipLaunchKernelGGL(j2k_tier1_kernel, dim3((unsigned)n_blocks), dim3(PL_WAVE), 0, st, d_bytes, nbytes, d_blocks, n_frames, rows,
                       cols, planes, d_status);
  for (int level = max_levels; level >= 1; --level) {
    const int rw = (int)((cols + (1ll << (level - 1)) - 1) >> (level - 1)), rh = (int)((rows + (1ll << (level - 1)) - 1) >> (level - 1));
    if (rw <= 1 && rh <= 1) continue;                       // a single sample passes through both axes
    const dim3 grid((unsigned)pl_cdiv((int64_t)rw * rh, 256), (unsigned)n_frames);
    hipLaunchKernelGGL(j2k_idwt_kernel, grid, dim3(256), 0, st, planes, planes + n_frames * size, d_params, level, rows, cols, rw, rh, 1);
    hipLaunchKernelGGL(j2k_idwt_kernel, grid, dim3(256), 0, st, planes + n_frames * size, planes, d_params, level, rows, cols, rw, rh, 0);
  }
  hipLaunchKernelGGL(j2k_store_kernel, dim3((unsigned)pl_cdiv(size, 256), (unsigned)n_frames), dim3(256), 0, st, planes, d_params,
                     max_levels, rows, cols, bytes_per_sample, d_native, d_status);
  return pl_check_launch("pl_dicom_j2k_decode");
}
