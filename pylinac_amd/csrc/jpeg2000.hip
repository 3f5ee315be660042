// JPEG 2000 lossless Pixel Data (transfer syntaxes 1.2.840.10008.1.2.4.90 and .91 with a reversible stream: ITU-T T.800, one
// component, one tile, one quality layer, the 5/3 transform, code-block style 0) -> the native little-endian frame buffer
// pl_dicom_decode reads, next to jpeg_lossless.hip.  The host parses each frame's main header and its packet headers (tier 2,
// T.800 Annex B) while the file is still host bytes; the device sees one descriptor per included code block of the whole
// stack (PL_J2K_BLOCK_FIELDS int64 values: frame, segment offset and length, coding passes, magnitude bit planes, subband
// orientation, the rectangle it fills in the frame's coefficient plane) and four parameters per frame (decomposition levels,
// precision, signed, 0).
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

}  // namespace

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
