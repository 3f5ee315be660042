// JPEG Lossless Pixel Data (transfer syntaxes 1.2.840.10008.1.2.4.57 and .70: ITU-T T.81 process 14, Huffman coding, one
// component) -> the native little-endian frame buffer pl_dicom_decode reads, next to the RLE Lossless passes of dicom.hip.
// The host parses each frame's JPEG header (T.81 Annex B) while the file is still host bytes; the device sees, per frame, the
// window of the entropy-coded segment, four parameters (precision P, selection value, point transform Pt, restart interval
// in samples) and the one Huffman table SOS selects (BITS[16], HUFFVAL[17]).
//
// jl_decode_kernel: ONE wave per frame, one launch for the stack, nothing read back.
//   tables   first code / count / offset per length in LDS (lane 0), a 9-bit look-up table (length << 8 | category) filled by
//            all lanes; a code longer than 9 bits walks the lengths 10 .. 16 (F.2.2.3).  A table with more than 17 symbols,
//            a category above 16 or a Kraft sum above 1 is an unsound parameter (bit 0).
//   input    kJlWindow raw bytes at a time go to LDS (byte loads: the scan starts at any alignment); every lane classifies
//            16 of them with one byte of look-ahead: FF 00 -> the data byte FF, FF FF -> fill, FF xx -> a marker, which ends
//            the window's data; the kept bytes are compacted behind what the reader has not consumed yet (a wave scan of the
//            counts).  A window that is not the scan's last leaves a trailing FF to the next one.
//   tokens   the wave-uniform loop of png.hip's inflate: a 64-bit accumulator refilled by the dword from LDS
//            (readfirstlane), the category from the table, `SSSS` extra bits (category 16: the difference 32768 and no extra
//            bits; a leading zero bit: v - (2^SSSS - 1)).  Lane (column & 63) keeps the difference.
//   rows     after 64 differences (or the row's end) the whole wave reconstructs them (H.1.2, modulo 2^16): the first row of
//            the scan or of a restart interval and the selection values 1, 4 and 5 are an inclusive wave scan (for 4, x - Rb is
//            the running sum of the differences; for 5 the addends hold (Rb - Rc) >> 1), 2 and 3 are element-wise, 6 and 7 are
//            nonlinear in Ra and run as a lane loop over v_readlane.  The previous and the current row live in LDS
//            (2 x kJlMaxCols x 2 bytes); the samples, shifted left by Pt, go straight to the frame's slot.
//   restarts at the end of an interval (whole rows, H.1.1) the bits up to the byte boundary are dropped, the marker
//            FF D0 + (k mod 8) must follow, the prediction starts over.  One chain per frame: intervals are NOT decoded in
//            parallel.
// LDS: 32 KiB of rows + 1 KiB raw window + 1 KiB + 64 compacted data + 1 KiB table: 35.3 KiB a wave.
//
// A translation unit of its own in the library.  The CPU emulator of the tests builds a fixed list of files, dicom.hip among
// them: there dicom.hip includes this file after pl_common.h (PL_JPEGLL_IN_DICOM), which is why nothing here may collide with
// dicom.hip's names.
#ifndef PL_JPEGLL_IN_DICOM
#include "pl_common.h"
#endif

namespace {

constexpr int kJlWindow = 1024;                             // raw bytes staged at a time (64 lanes x 16)
constexpr int kJlAhead = 9 * 32;                            // bits the reader holds before eight tokens (a token: 32 at most)
constexpr int kJlData = kJlWindow + 64;                     // compacted bytes: the unconsumed tail (36), a window, the zero pad
constexpr int kJlMaxCols = PL_DICOM_JPEGLL_MAX_COLS;
constexpr int kJlLutBits = 9;

struct JlTables {
  int first[17], cnt[17], offs[17];                         // per code length 1 .. 16 (F.2.2.3)
  unsigned char val[20];                                    // HUFFVAL
};

// the wave-uniform reader over the compacted bytes of s_data
struct JlReader {
  unsigned long long acc;                                   // the next nb bits, left-aligned
  int nb, pos, len;                                         // pos: the next dword of s_data to take (a byte index), len: its bytes
  int64_t rp, rend;                                         // the next raw byte to stage, the scan's end
  int ended, marker;                                        // ended: no raw byte follows what s_data holds; marker: the code
  int64_t marker_at;                                        //   that ended it (0: the window's end) and where its FF lies

  __device__ __forceinline__ int used() const { return pos * 8 - nb; }           // bits consumed of s_data
  __device__ __forceinline__ int left() const { return len * 8 - used(); }
  __device__ __forceinline__ void take(const unsigned* s_data) {                  // afterwards nb > 32
    if (nb <= 32) {
      const unsigned w = pos < kJlData ? __builtin_amdgcn_readfirstlane(s_data[pos >> 2]) : 0u;
      acc |= (unsigned long long)__builtin_bswap32(w) << (32 - nb);
      pos += 4, nb += 32;
    }
  }
  __device__ __forceinline__ void drop(int n) { acc <<= n, nb -= n; }
};

// the next window of raw bytes behind the reader's unconsumed tail
__device__ __forceinline__ void jl_fill(JlReader& r, const unsigned char* __restrict__ bytes, unsigned char* s_raw, unsigned* s_data32, int lane) {
  unsigned char* s_data = reinterpret_cast<unsigned char*>(s_data32);
  const int used = r.used(), from = used >> 3;
  const int keep = r.len > from ? r.len - from : 0;         // (a fill happens below kJlAhead bits left: at most 36 bytes)
  const unsigned char moved = lane < keep ? s_data[from + lane] : 0;
  const int64_t span = r.rend - r.rp;
  const int n = span < kJlWindow ? (int)span : kJlWindow;
  __syncthreads();
  if (lane < keep) s_data[lane] = moved;
  if (lane == 0) s_raw[0] = 0;                              // (the byte before a window is never a pending FF)
  for (int i = lane; i < n; i += PL_WAVE) s_raw[1 + i] = bytes[r.rp + i];
  const bool final = r.rp + n == r.rend;
  if (lane == 0) s_raw[1 + n] = 0x01;                       // the scan's end behind a dangling FF: a marker that is none
  __syncthreads();
  // a trailing FF waits for its second byte in the next window
  const int n_eff = (!final && n > 0 && __builtin_amdgcn_readfirstlane((unsigned)s_raw[n]) == 0xffu) ? n - 1 : n;
  unsigned kept = 0;
  int mark = kJlWindow;
  for (int j = 15; j >= 0; --j) {
    const int i = lane * 16 + j;
    if (i >= n_eff) continue;
    const unsigned b = s_raw[1 + i], p = s_raw[i], nx = s_raw[2 + i];
    if (b == 0xffu && nx != 0u && nx != 0xffu) mark = i;
    if ((b != 0xffu && !(b == 0u && p == 0xffu)) || (b == 0xffu && nx == 0u)) kept |= 1u << j;
  }
  const unsigned long long marks = __ballot(mark < kJlWindow);
  // (the lanes own ascending ranges; readlane keeps the reader's state in scalar registers)
  const int m_at = marks ? __builtin_amdgcn_readlane(mark, __ffsll(marks) - 1) : kJlWindow;
  for (int j = 0; j < 16; ++j)
    if (lane * 16 + j >= m_at) kept &= ~(1u << j);
  const int mine = __popc(kept);
  int incl = mine;
  for (int o = 1; o < PL_WAVE; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  const int total = __builtin_amdgcn_readlane(incl, PL_WAVE - 1);
  int at = keep + incl - mine;
  for (int j = 0; j < 16; ++j)
    if ((kept >> j) & 1u) s_data[at++] = s_raw[1 + lane * 16 + j];
  __syncthreads();
  r.len = keep + total;
  if (lane < 16) s_data[r.len + lane] = 0;                  // what a peek beyond the data sees
  __syncthreads();
  if (m_at < kJlWindow) {
    r.ended = 1, r.marker = (int)__builtin_amdgcn_readfirstlane((unsigned)s_raw[2 + m_at]), r.marker_at = r.rp + m_at;
    if (final && m_at == n - 1) r.marker = 0;               // the dangling FF: the window's end
  } else {
    r.rp += n_eff;
    if (r.rp >= r.rend) r.ended = 1, r.marker = 0;
  }
  r.acc = 0, r.nb = 0, r.pos = 0;
  r.take(s_data32);
  r.drop(used & 7);
}

__device__ __forceinline__ unsigned jl_scan16(unsigned v, int lane) {          // inclusive wave sum (the callers mask to 16 bits)
  for (int o = 1; o < PL_WAVE; o <<= 1) {
    const unsigned t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

__global__ void __launch_bounds__(PL_WAVE)
jl_decode_kernel(const unsigned char* __restrict__ bytes, int64_t nbytes, const int64_t* __restrict__ scan_off,
                 const int64_t* __restrict__ scan_len, const int32_t* __restrict__ params, const unsigned char* __restrict__ huff,
                 int rows, int cols, int bps, unsigned char* __restrict__ native, int32_t* __restrict__ status) {
  __shared__ unsigned short s_row[2][kJlMaxCols];
  __shared__ unsigned char s_raw[kJlWindow + 8];
  __shared__ unsigned s_data[kJlData / 4 + 8];
  __shared__ unsigned short s_lut[1 << kJlLutBits];
  __shared__ JlTables s_t;
  const int lane = threadIdx.x;
  const int64_t f = blockIdx.x;
  const int64_t off = scan_off[f], len = scan_len[f];
  const int prec = params[f * 4], sel = params[f * 4 + 1], pt = params[f * 4 + 2], ri = params[f * 4 + 3];
  const unsigned char* h = huff + f * 33;
  // ---- the parameters and the table -----------------------------------------------------------------------------------------
  // (differences of lengths, never sums of an offset and a length: nothing here can overflow)
  bool bad = off < 0 || len < 0 || off > nbytes || len > nbytes - off;
  bad = bad || prec < 2 || prec > 16 || prec > 8 * bps || sel < 1 || sel > 7 || pt < 0 || pt >= prec || ri < 0 || ri % cols != 0;
  {
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
      const int c = h[l - 1];
      if (lane == 0) s_t.first[l] = code, s_t.cnt[l] = c, s_t.offs[l] = k;
      k += c, code += c;
      bad = bad || code > (1 << l);
      code <<= 1;
    }
    bad = bad || k > 17;
    for (int i = 0; i < 17; ++i) bad = bad || (i < k && h[16 + i] > 16);
    if (lane < 17) s_t.val[lane] = h[16 + lane];
  }
  if (bad) {                                                // nothing of the frame is read or stored
    if (lane == 0) status[f] = 1;
    return;
  }
  __syncthreads();
  for (int e = lane; e < (1 << kJlLutBits); e += PL_WAVE) {
    unsigned entry = 0;
    for (int l = 1; l <= kJlLutBits; ++l) {
      const int d = (e >> (kJlLutBits - l)) - s_t.first[l];
      if (d >= 0 && d < s_t.cnt[l]) {
        entry = ((unsigned)l << 8) | s_t.val[s_t.offs[l] + d];
        break;
      }
    }
    s_lut[e] = (unsigned short)entry;
  }
  __syncthreads();
  // ---- the scan -------------------------------------------------------------------------------------------------------------
  JlReader r;
  r.acc = 0, r.nb = 0, r.pos = 0, r.len = 0, r.rp = off, r.rend = off + len, r.ended = 0, r.marker = 0, r.marker_at = 0;
  unsigned char* out = native + f * ((int64_t)rows * cols * bps);
  const bool out_even = ((uintptr_t)out & 1u) == 0;
  const unsigned init = 1u << (prec - pt - 1);
  const int ri_rows = ri / cols;
  int flag = 0, interval = 0;
  for (int row = 0; row < rows && !flag; ++row) {
    bool first_row = row == 0;
    if (ri_rows > 0 && row > 0 && row % ri_rows == 0) {     // the end of a restart interval
      r.drop(r.nb & 7);
      while (!r.ended && r.left() <= 0) jl_fill(r, bytes, s_raw, s_data, lane);
      if (r.left() > 0) flag = 4;                           // data where the marker belongs
      else if (r.marker >= 0xd0 && r.marker <= 0xd7) {
        if (r.marker == 0xd0 + (interval & 7)) {
          r.rp = r.marker_at + 2, r.ended = r.rp >= r.rend, r.marker = 0;
          r.len = 0, r.acc = 0, r.nb = 0, r.pos = 0;
        } else flag = 4;
      } else flag = 2;
      if (flag) break;
      ++interval;
      first_row = true;
    }
    unsigned short* cur = s_row[row & 1];
    const unsigned short* prev = s_row[(row & 1) ^ 1];
    unsigned left = 0;                                      // the sample before the chunk (wave-uniform)
    for (int c0 = 0; c0 < cols && !flag; c0 += PL_WAVE) {
      const int n = cols - c0 < PL_WAVE ? cols - c0 : PL_WAVE;
      unsigned mine = 0;
      for (int k = 0; k < n; ++k) {
        // a token takes at most 32 bits: enough for the next eight, or everything there is
        if ((k & 7) == 0)
          while (!r.ended && r.left() < kJlAhead) jl_fill(r, bytes, s_raw, s_data, lane);
        r.take(s_data);
        const unsigned top = (unsigned)(r.acc >> 48);
        const unsigned e = __builtin_amdgcn_readfirstlane((unsigned)s_lut[top >> (16 - kJlLutBits)]);
        int l = (int)(e >> 8), ssss = (int)(e & 0xffu);
        if (l == 0) {
          for (int q = kJlLutBits + 1; q <= 16; ++q) {
            const int d = (int)(top >> (16 - q)) - __builtin_amdgcn_readfirstlane(s_t.first[q]);
            if (d >= 0 && d < __builtin_amdgcn_readfirstlane(s_t.cnt[q])) {
              l = q;
              ssss = (int)__builtin_amdgcn_readfirstlane((unsigned)s_t.val[__builtin_amdgcn_readfirstlane(s_t.offs[q]) + d]);
              break;
            }
          }
          if (l == 0) {                                     // no code: corrupt, unless the data ends inside it
            flag = r.left() < 16 ? 2 : 4;
            break;
          }
        }
        // without a branch: nx extra bits (none for the categories 0 and 16), EXTEND (F.2.2.1), 32768 for category 16
        const int nx = ssss & 15;
        const unsigned v = (unsigned)(((r.acc << l) >> 1) >> (63 - nx));
        r.drop(l + nx);
        const unsigned diff = v + (v < ((1u << nx) >> 1) ? 1u - (1u << nx) : 0u) + ((unsigned)(ssss >> 4) << 15);
        if (lane == k) mine = diff & 0xffffu;
      }
      if (!flag && r.left() < 0) flag = 2;                  // a token reached beyond the data (the pad behind it is zeros)
      if (flag) break;
      // ---- H.1.2: the chunk's samples from its differences ---------------------------------------------------------------------
      __syncthreads();                                      // the row above is complete
      const int c = c0 + lane;
      const bool on = lane < n;
      unsigned rb = 0, rc = 0;
      if (!first_row && on) rb = prev[c], rc = c > 0 ? prev[c - 1] : 0u;
      unsigned x;
      if (first_row) {
        x = (c0 ? left : init) + jl_scan16(mine, lane);
      } else if (sel == 1) {
        x = (c0 ? left : 0u) + jl_scan16(c == 0 ? rb + mine : mine, lane);
      } else if (sel == 2) {
        x = rb + mine;
      } else if (sel == 3) {
        x = (c == 0 ? rb : rc) + mine;
      } else if (sel == 4) {
        const unsigned base = c0 ? left - (unsigned)prev[c0 - 1] : 0u;
        x = base + jl_scan16(mine, lane) + rb;
      } else if (sel == 5) {
        const unsigned add = c == 0 ? rb : (unsigned)(((int)rb - (int)rc) >> 1);
        x = (c0 ? left : 0u) + jl_scan16(add + mine, lane);
      } else {                                              // 6, 7: serial in Ra
        unsigned ra = left;
        x = 0;
        const unsigned above = rb | (rc << 16);
        for (int k = 0; k < n; ++k) {
          const unsigned dk = (unsigned)__builtin_amdgcn_readlane((int)mine, k);
          const unsigned ak = (unsigned)__builtin_amdgcn_readlane((int)above, k);
          const unsigned rbk = ak & 0xffffu, rck = ak >> 16;
          unsigned px;
          if (c0 + k == 0) px = rbk;
          else if (sel == 6) px = rbk + (unsigned)(((int)ra - (int)rck) >> 1);
          else px = (ra + rbk) >> 1;
          ra = (px + dk) & 0xffffu;
          if (lane == k) x = ra;
        }
      }
      x &= 0xffffu;
      left = (unsigned)__builtin_amdgcn_readlane((int)x, n - 1);
      if (on) {
        cur[c] = (unsigned short)x;
        const unsigned v = x << pt;
        const int64_t at = (int64_t)row * cols + c;
        if (bps == 1) out[at] = (unsigned char)v;
        else if (out_even) reinterpret_cast<unsigned short*>(out)[at] = (unsigned short)v;
        else out[2 * at] = (unsigned char)v, out[2 * at + 1] = (unsigned char)(v >> 8);
      }
    }
  }
  if (flag && lane == 0) status[f] = flag;
}

}  // namespace

extern "C" int64_t pl_dicom_jpegll_work_bytes(int64_t n_frames, int rows, int cols) {
  if (n_frames < 1 || n_frames > 65535 || rows < 1 || cols < 1 || cols > kJlMaxCols) return -1;
  return 0;                                                 // the rows are buffered in LDS
}

extern "C" int pl_dicom_jpegll_decode(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_scan_off,
                                      const int64_t* d_scan_len, const int32_t* d_params, const unsigned char* d_huff,
                                      int64_t n_frames, int rows, int cols, int bytes_per_sample, unsigned char* d_native,
                                      int32_t* d_status, void* d_work, void* stream) {
  (void)d_work;
  if (bytes_per_sample != 1 && bytes_per_sample != 2) {
    pl_set_error("pl_dicom_jpegll_decode: unsupported bytes_per_sample %d (BitsAllocated 8 or 16)", bytes_per_sample);
    return PL_ERR_UNSUPPORTED;
  }
  if (cols > kJlMaxCols) {
    pl_set_error("pl_dicom_jpegll_decode: unsupported cols %d (a row of at most %d samples is buffered)", cols, kJlMaxCols);
    return PL_ERR_UNSUPPORTED;
  }
  PL_REQUIRE(d_bytes && d_scan_off && d_scan_len && d_params && d_huff && d_native && d_status, "null pointer");
  PL_REQUIRE(n_frames >= 1 && n_frames <= 65535, "1 <= n_frames <= 65535");
  PL_REQUIRE(rows >= 1 && cols >= 1 && nbytes >= 0, "bad shape");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(d_status, 0, (size_t)n_frames * 4, st) != hipSuccess) {
    pl_set_error("pl_dicom_jpegll_decode: memset failed");
    return PL_ERR_HIP;
  }
  hipLaunchKernelGGL(jl_decode_kernel, dim3((unsigned)n_frames), dim3(PL_WAVE), 0, st, d_bytes, nbytes, d_scan_off, d_scan_len,
                     d_params, d_huff, rows, cols, bytes_per_sample, d_native, d_status);
  return pl_check_launch("pl_dicom_jpegll_decode");
}
