// Strip TIFFs (TIFF 6.0: uncompressed, PackBits 32773, LZW 5 and Deflate 8 / 32946 with the horizontal predictor) -> typed frames on the device:
// the step BEFORE the hot path for scanned film, next to dicom.hip and xim.hip.  The reference hands its analyzers
// `np.asarray(PIL.Image.open(f))` (libtiff); the arithmetic here is libtiff's:
//   * a strip holds rows_in_strip x row_bytes bytes (row_bytes = width x samples x bits / 8), rows one after the other;
//   * LZW (tif_lzw.c, new-style streams): codes MSB first, 9 bits after a Clear (256), EOI = 257, the width grows when the
//     next free entry reaches 511 / 1023 / 2047 ("early change"), entries are added from 258 on, one per code after the first;
//   * Predictor 2 (tif_predict.c horAcc8 / horAcc16): every row is an inclusive prefix sum per channel in the sample width,
//     for big-endian ("MM") files after the byte swap;
//   * RGB -> one band as PIL's convert("I") of an RGB image: (19595 R + 38470 G + 7471 B + 0x8000) >> 16.
// Whole files lie anywhere in one device buffer; a per-strip descriptor (offset, length, frame, first row, rows, compression)
// says where every strip lies and where it goes, so files of one stack may differ in compression, predictor, byte order and
// strip layout.  The launches (a fixed number, whatever the stack):
//   1 tiff_check_kernel   a thread per strip: the descriptor and the window [offset, offset + length) against the buffer;
//                         a bad strip flags its FRAME (status bit 0) and is never read; the PackBits stream table
//   2 tiff_raw_kernel     uncompressed strips: a coalesced dword copy at any source alignment (v_alignbit funnel)
//   3-5                   PackBits strips: dicom.hip's three chunked passes (pl_packbits_expand), a strip = one stream
//   6 tiff_lzw_kernel     LZW strips, one wave per strip (below)
//   7 tiff_finish_kernel  a wave per row of the staged bytes: byte swap, predictor scan, RGB collapse, store as out_kind
// Launches 2, 3-5 and 6 are left out when the caller's `compressions` mask says no strip needs them.
//
// Deflate strips (Compression 8 and 32946, mask bit 8: pl_tiff_decode_ex only) add five launches between 6 and 7, left out
// like the others: tiff_deflate_table_kernel (where every strip's bytes go, and which strips are not the inflate's),
// png.hip's inflate_kernel<true> with the zlib wrapper (pl_inflate_launch: one wave per strip, straight into the staged area --
// a strip is one contiguous zlib stream, nothing is gathered), adler32.hip's pair over what was stored (pl_adler32_launch, for
// the strips whose stream ended where it should with its field present) and tiff_deflate_verdict_kernel (per strip -> bits 1,
// 3 and 4 of its frame's status).  Always checked: libtiff hands zlib the whole strip, and a wrong Adler-32 is an error there.
//
// LZW without a string table.  Let q be the position (in code order) of the last Clear before code position p.  Entry
// 258 + j is made when the (j + 2)-th code after the Clear is read, and is the string of the (j + 1)-th code followed by the
// first byte of the next one -- which lie side by side in the OUTPUT.  So a code c >= 258 at position p names position
// r = q + c - 257 (valid iff q + 1 <= r <= p - 1; r = p - 1 is the KwKwK case) and its string is the len[r] + 1 output bytes
// from off[r] on: len[p] = len[r] + 1, off = the exclusive scan of len.  The code width depends only on p - q.  One loop
// iteration of the wave:
//   A  lane i reads the code at bit position bitpos + i * width (input staged in LDS 1 KiB at a time); the accepted prefix
//      ends at the first Clear (inclusive), EOI, the width-change position or the end of the input (ballots);
//   B  len: from the ring of the current table epoch in LDS (len / off of the last 4096 positions since the Clear) when r lies
//      before this iteration's codes, else by pointer jumping among the lanes (six shuffle rounds: a chain of KwKwK codes);
//   C  off: a wave scan plus the running total; the strip is complete at rows x row_bytes, what follows is dropped;
//   D  expansion in sub-batches of consecutive codes whose sources end before the sub-batch begins (only its first code may
//      name r >= first - 1): a lane copies a short string itself, the wave copies a long one (> 8 bytes) together; the last
//      byte of a KwKwK string is its own first byte.  A workgroup-scope release / acquire pair between sub-batches makes the
//      bytes of one visible to the next (one wave, one CU: a wait, no cache maintenance).
#include "pl_common.h"

namespace {

constexpr int kTfThreads = 256;
constexpr int kTfNone = 1, kTfLzw = 5, kTfPackbits = 32773;
constexpr int kTfDeflate = 8, kTfDeflateOld = 32946;        // Adobe Deflate and the older code: one codec in libtiff
constexpr int kTfRing = 4096;                               // table positions since a Clear that a code can name: 1 .. 3838
constexpr int kTfWindow = 1024;                             // input bytes staged in LDS at a time
constexpr int kTfLong = 8;                                  // strings longer than this are copied by the whole wave

struct TfStrip {
  bool ok;                                                  // descriptor and window are sound
  int frame, row0, rows, comp;
  int64_t off, len;
};

__device__ __forceinline__ bool tf_is_deflate(int comp) { return comp == kTfDeflate || comp == kTfDeflateOld; }

__device__ __forceinline__ TfStrip tf_strip(const int64_t* __restrict__ strip_off, const int64_t* __restrict__ strip_len,
                                            const int32_t* __restrict__ desc, int64_t s, int64_t nbytes, int64_t max_strip_bytes,
                                            int64_t n_frames, int height, int compressions) {
  TfStrip t;
  t.frame = desc[4 * s], t.row0 = desc[4 * s + 1], t.rows = desc[4 * s + 2], t.comp = desc[4 * s + 3];
  t.off = strip_off[s], t.len = strip_len[s];
  const int bit = t.comp == kTfNone ? 1 : (t.comp == kTfPackbits ? 2 : (t.comp == kTfLzw ? 4 : (tf_is_deflate(t.comp) ? 8 : 0)));
  // (differences of lengths, never sums of an offset and a length: nothing here can overflow)
  t.ok = t.frame >= 0 && t.frame < n_frames && t.row0 >= 0 && t.rows >= 1 && t.row0 < height && t.rows <= height - t.row0 &&
         t.off >= 0 && t.len >= 0 && t.off <= nbytes && t.len <= nbytes - t.off && t.len <= max_strip_bytes &&
         (bit & compressions) != 0;
  return t;
}

// launch 1
__global__ void __launch_bounds__(kTfThreads)
tiff_check_kernel(const int64_t* __restrict__ strip_off, const int64_t* __restrict__ strip_len, const int32_t* __restrict__ desc,
                  int64_t n_strips, int64_t nbytes, int64_t max_strip_bytes, int64_t n_frames, int height, int64_t row_bytes,
                  int compressions, int64_t* __restrict__ pb_off, int64_t* __restrict__ pb_len, int64_t* __restrict__ pb_expect,
                  int64_t* __restrict__ pb_dst, int32_t* __restrict__ pb_frame, int32_t* __restrict__ status) {
  const int64_t s = (int64_t)blockIdx.x * kTfThreads + threadIdx.x;
  if (s >= n_strips) return;
  const TfStrip t = tf_strip(strip_off, strip_len, desc, s, nbytes, max_strip_bytes, n_frames, height, compressions);
  if (!t.ok && t.frame >= 0 && t.frame < n_frames) atomicOr(status + t.frame, 1);
  if (pb_off) {                                             // the PackBits passes see every strip; the others as empty streams
    const bool mine = t.ok && t.comp == kTfPackbits;
    pb_off[s] = mine ? t.off : 0;
    pb_len[s] = mine ? t.len : 0;
    pb_expect[s] = mine ? t.rows * row_bytes : 0;
    pb_dst[s] = mine ? ((int64_t)t.frame * height + t.row0) * row_bytes : 0;
    pb_frame[s] = mine ? t.frame : 0;
  }
}

// launch 2
__global__ void __launch_bounds__(kTfThreads)
tiff_raw_kernel(const unsigned char* __restrict__ bytes, int64_t nbytes, const int64_t* __restrict__ strip_off,
                const int64_t* __restrict__ strip_len, const int32_t* __restrict__ desc, int64_t max_strip_bytes,
                int64_t n_frames, int height, int64_t row_bytes, int compressions, unsigned char* __restrict__ staged,
                int32_t* __restrict__ status) {
  const int64_t s = blockIdx.x;                             // (blockIdx.y: the strip's pieces)
  const TfStrip t = tf_strip(strip_off, strip_len, desc, s, nbytes, max_strip_bytes, n_frames, height, compressions);
  if (!t.ok || t.comp != kTfNone) return;
  const int64_t expect = t.rows * row_bytes;
  const int64_t n = t.len < expect ? t.len : expect;
  if (t.len < expect && blockIdx.y == 0 && threadIdx.x == 0) atomicOr(status + t.frame, 2);
  unsigned char* dst = staged + ((int64_t)t.frame * height + t.row0) * row_bytes;
  const unsigned char* src = bytes + t.off;
  int64_t head = (int64_t)((4u - (unsigned)((uintptr_t)dst & 3u)) & 3u);       // bytes up to the first aligned destination dword
  if (head > n) head = n;
  const int64_t nd = (n - head) >> 2, tail0 = head + 4 * nd;
  if (blockIdx.y == 0) {
    if ((int64_t)threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    const int64_t k = tail0 + threadIdx.x;
    if (k < n) dst[k] = src[k];
  }
  const int64_t from = t.off + head;                        // the buffer byte of the first dword
  const unsigned sh = (unsigned)(from & 3) * 8u;
  const unsigned* base = reinterpret_cast<const unsigned*>(bytes + (from & ~(int64_t)3));
  const int64_t last_dword = ((nbytes + 3) >> 2) - 1 - ((from & ~(int64_t)3) >> 2);
  unsigned* out = reinterpret_cast<unsigned*>(dst + head);
  for (int64_t v = (int64_t)blockIdx.y * kTfThreads + threadIdx.x; v < nd; v += (int64_t)gridDim.y * kTfThreads) {
    unsigned d = base[v];
    if (sh) {                                               // (wave-uniform: a property of the strip)
      const unsigned e = base[v + 1 <= last_dword ? v + 1 : last_dword];       // beyond the buffer only bits nothing uses
      d = __builtin_amdgcn_alignbit(e, d, sh);
    }
    out[v] = d;
  }
}

// ---- launch 6: LZW -------------------------------------------------------------------------------------------------------
// every lane calls these (wave-uniform control flow throughout the kernel)
__device__ __forceinline__ unsigned tf_wave_inclusive(unsigned v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// global bytes written by some lanes of the wave and read by others
__device__ __forceinline__ void tf_output_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ void __launch_bounds__(PL_WAVE)
tiff_lzw_kernel(const unsigned char* __restrict__ bytes, int64_t nbytes, const int64_t* __restrict__ strip_off,
                const int64_t* __restrict__ strip_len, const int32_t* __restrict__ desc, int64_t max_strip_bytes,
                int64_t n_frames, int height, int64_t row_bytes, int compressions, unsigned char* staged,
                int32_t* __restrict__ status) {
  __shared__ unsigned short s_len[kTfRing];
  __shared__ unsigned s_off[kTfRing];
  __shared__ unsigned char s_in[kTfWindow + 4];
  const int64_t s = blockIdx.x;
  const int lane = threadIdx.x;
  const TfStrip t = tf_strip(strip_off, strip_len, desc, s, nbytes, max_strip_bytes, n_frames, height, compressions);
  if (!t.ok || t.comp != kTfLzw) return;
  const unsigned expect = (unsigned)(t.rows * row_bytes);   // (frame bytes < 2^31: checked on the host)
  unsigned char* out = staged + ((int64_t)t.frame * height + t.row0) * row_bytes;
  const unsigned char* src = bytes + t.off;
  const int64_t nbits = t.len * 8;
  int64_t bitpos = 0, win0 = -(int64_t)kTfWindow;           // the staged window holds input bytes win0 .. win0 + kTfWindow - 1
  int kk0 = 1, width = 9;                                   // lane 0's code is the kk0-th since the Clear (a strip begins as if cleared)
  unsigned total = 0;
  bool corrupt = false;
  while (total < expect) {
    // A: codes
    const int64_t byte0 = bitpos >> 3;
    if (byte0 + 64 * 12 / 8 + 3 > win0 + kTfWindow || byte0 < win0) {
      pl_wave_sync();
      win0 = byte0;
      for (int k = lane; k < kTfWindow; k += PL_WAVE) s_in[k] = win0 + k < t.len ? src[win0 + k] : (unsigned char)0;
      pl_wave_sync();
    }
    const int64_t bit = bitpos + (int64_t)lane * width;
    const int limit = width == 9 ? 255 - kk0 : (width == 10 ? 767 - kk0 : (width == 11 ? 1791 - kk0 : 64));
    const bool have = bit + width <= nbits && lane < limit;
    int c = 0;
    if (have) {
      const int b = (int)((bit >> 3) - win0);
      const unsigned w24 = ((unsigned)s_in[b] << 16) | ((unsigned)s_in[b + 1] << 8) | (unsigned)s_in[b + 2];
      c = (int)((w24 >> (24 - (int)(bit & 7) - width)) & ((1u << width) - 1u));
    }
    const unsigned long long havem = __ballot(have);
    if (havem == 0) break;                                  // the input ends before the strip is complete
    int m = __popcll(havem);                                // (a prefix of the lanes: both conditions are monotone)
    const unsigned long long stopm = __ballot(have && (c == 256 || c == 257));
    bool cleared = false, ended = false;
    if (stopm) {
      const int first = __ffsll(stopm) - 1;
      const int cf = __shfl(c, first, 64);
      cleared = cf == 256;
      ended = !cleared;
      m = first + (cleared ? 1 : 0);
    }
    const int kk = kk0 + lane;
    const int rr = c - 257;                                 // the named position, counted like kk
    const unsigned long long badm = __ballot(lane < m && c >= 258 && (rr < 1 || rr > kk - 1));
    if (badm) {                                             // libtiff: "Corrupted LZW table" -- unless the strip is complete before it
      m = __ffsll(badm) - 1;
      corrupt = ended = true;
      cleared = false;
    }
    const bool acc = lane < m && c != 256;                  // the codes that produce output
    const bool isref = acc && c >= 258;
    // B: lengths
    unsigned val = acc ? 1u : 0u;
    int ptr = -1;
    if (isref) {
      if (rr < kk0) val += s_len[rr & (kTfRing - 1)];
      else ptr = rr - kk0;
    }
    if (__ballot(ptr >= 0)) {
#pragma unroll
      for (int round = 0; round < 6; ++round) {
        const int from = ptr >= 0 ? ptr : lane;
        const unsigned pv = __shfl(val, from, 64);
        const int pp = __shfl(ptr, from, 64);
        if (ptr >= 0) {
          val += pv;
          ptr = pp;
        }
      }
    }
    // C: offsets
    const unsigned inc = tf_wave_inclusive(val, lane);
    const unsigned at = total + inc - val;
    const unsigned sum = __shfl(inc, 63, 64);
    const unsigned at_named = __shfl(at, isref && rr >= kk0 ? rr - kk0 : lane, 64);
    unsigned from = 0;
    if (isref) from = rr < kk0 ? s_off[rr & (kTfRing - 1)] : at_named;
    pl_wave_sync();                                         // (the ring reads above, before the writes below)
    if (acc && kk < kTfRing) {
      s_len[kk] = (unsigned short)val;
      s_off[kk] = at;
    }
    // D: expansion
    int b0 = 0;
    while (b0 < m) {
      const unsigned long long dep = __ballot(isref && lane > b0 && rr >= kk0 + b0 - 1);
      const int b1 = dep ? __ffsll(dep) - 1 : m;
      const bool inb = acc && lane >= b0 && lane < b1;
      const bool wide = inb && isref && val > (unsigned)kTfLong;
      if (inb && !wide) {
        if (!isref) {
          if (at < expect) out[at] = (unsigned char)c;
        } else {
          for (unsigned k = 0; k < val && at + k < expect; ++k) {          // (sources lie before their targets: inside too)
            unsigned g = from + k;
            if (g == at) g = from;                          // KwKwK: the string's last byte is its own first byte
            out[at + k] = out[g];
          }
        }
      }
      unsigned long long widem = __ballot(wide);
      while (widem) {
        const int l = __ffsll(widem) - 1;
        widem &= widem - 1;
        const unsigned a = __shfl(at, l, 64), f = __shfl(from, l, 64), n = __shfl(val, l, 64);
        for (unsigned k = lane; k < n && a + k < expect; k += PL_WAVE) {
          unsigned g = f + k;
          if (g == a) g = f;
          out[a + k] = out[g];
        }
      }
      tf_output_sync();
      b0 = b1;
    }
    total += sum;
    bitpos += (int64_t)m * width;
    kk0 = cleared ? 1 : min(kk0 + m, 1 << 24);               // (positions beyond the ring only need to stay large)
    width = cleared ? 9 : (kk0 >= 1791 ? 12 : (kk0 >= 767 ? 11 : (kk0 >= 255 ? 10 : 9)));
    pl_wave_sync();                                         // (the ring writes, before the next iteration's reads)
    if (ended) break;
  }
  if (lane == 0) {
    if (total < expect) atomicOr(status + t.frame, corrupt ? 4 : 2);
  }
}

// ---- the Deflate launches (mask bit 8; pl_tiff_decode_ex) --------------------------------------------------------------------
// A strip of Compression 8 / 32946 is ONE zlib stream, contiguous in the file: png.hip's inflate_kernel<true> reads it where it
// lies (the caller's strip_off / strip_len ARE its stream table) and stores straight into the staged area.  This kernel fills
// the rest of what it reads: where a strip's bytes go, how many they are, and a per-STRIP status word whose bit 0 tells the
// inflate to leave the strip alone (another compression, an unsound descriptor, a window outside the buffer).
__global__ void __launch_bounds__(kTfThreads)
tiff_deflate_table_kernel(const int64_t* __restrict__ strip_off, const int64_t* __restrict__ strip_len,
                          const int32_t* __restrict__ desc, int64_t n_strips, int64_t nbytes, int64_t max_strip_bytes,
                          int64_t n_frames, int height, int64_t row_bytes, int compressions, int64_t* __restrict__ out_off,
                          int64_t* __restrict__ out_cap, int32_t* __restrict__ strip_status) {
  const int64_t s = (int64_t)blockIdx.x * kTfThreads + threadIdx.x;
  if (s >= n_strips) return;
  const TfStrip t = tf_strip(strip_off, strip_len, desc, s, nbytes, max_strip_bytes, n_frames, height, compressions);
  const bool mine = t.ok && tf_is_deflate(t.comp);
  out_off[s] = mine ? ((int64_t)t.frame * height + t.row0) * row_bytes : 0;
  out_cap[s] = mine ? t.rows * row_bytes : 0;
  strip_status[s] = mine ? 0 : 1;
}

// What libtiff's ZIPDecode makes of a strip, as bits of its FRAME's status.  libtiff hands zlib the whole strip and room for
// rows x row_bytes bytes, and is content once they are filled: the input may end anywhere after that (a cut Adler-32 field), the
// stream may go on.  A field that is there and differs is zlib's "incorrect data check".  Strips the inflate skipped (bit 0 of
// the strip's word) left out_len and the flags unwritten: nothing of them is read.
__global__ void __launch_bounds__(kTfThreads)
tiff_deflate_verdict_kernel(const int32_t* __restrict__ desc, int64_t n_strips, int64_t n_frames,
                            const int32_t* __restrict__ strip_status, const int64_t* __restrict__ out_cap,
                            const int64_t* __restrict__ out_len, int32_t* __restrict__ status) {
  const int64_t s = (int64_t)blockIdx.x * kTfThreads + threadIdx.x;
  if (s >= n_strips) return;
  const int st = strip_status[s];
  if (st & 1) return;
  int bits = 0;
  if ((st & 2) && out_len[s] < out_cap[s]) bits |= 2;       // the input ended first, or the stream ended below the strip's size
  if (st & 4) bits |= 8;                                    // corrupt Deflate, a bad zlib header and FDICT included
  if (st & 16) bits |= 16;                                  // the Adler-32 of what was stored differs from the stream's field
  const int f = desc[4 * s];
  if (bits && f >= 0 && f < n_frames) atomicOr(status + f, bits);
}

// ---- the last launch: byte order, predictor, RGB collapse, store -----------------------------------------------------------
// OUT: 0 the container dtype (uint8 / uint16; int32 for RGB), 1 uint16, 2 float64 -- `array.astype(dtype)` of the container
template <int OUT>
__device__ __forceinline__ void tf_store(void* __restrict__ out, int64_t i, unsigned v, int container_bytes) {
  if constexpr (OUT == 0) {
    if (container_bytes == 1) static_cast<unsigned char*>(out)[i] = (unsigned char)v;
    else if (container_bytes == 2) static_cast<unsigned short*>(out)[i] = (unsigned short)v;
    else static_cast<int*>(out)[i] = (int)v;
  } else if constexpr (OUT == 1) {
    static_cast<unsigned short*>(out)[i] = (unsigned short)v;
  } else {
    static_cast<double*>(out)[i] = (double)v;
  }
}

// BYTES per sample, SPP samples per pixel (1 grey, 3 RGB of 8 bits)
template <int BYTES, int SPP, int OUT>
__global__ void __launch_bounds__(kTfThreads)
tiff_finish_kernel(const unsigned char* __restrict__ staged, const int32_t* __restrict__ frame_flags, int width, int height,
                   void* __restrict__ out, const int32_t* __restrict__ status) {
  const int64_t f = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int row = (int)blockIdx.x * (kTfThreads / PL_WAVE) + (threadIdx.x >> 6);
  if (row >= height || (status[f] & 1)) return;             // (wave-uniform)
  const int flags = frame_flags[f];
  const bool predictor = (flags & 1) != 0, big_endian = (flags & 2) != 0;
  const int64_t row_bytes = (int64_t)width * SPP * BYTES;
  const unsigned char* src = staged + (f * height + row) * row_bytes;
  const int64_t o0 = (f * height + row) * (int64_t)width;
  constexpr unsigned kMask = BYTES == 1 ? 0xffu : 0xffffu;
  unsigned carry[SPP];
#pragma unroll
  for (int ch = 0; ch < SPP; ++ch) carry[ch] = 0;
  for (int x0 = 0; x0 < width; x0 += PL_WAVE) {             // (uniform trip count: the scans are called by every lane)
    const int x = x0 + lane;
    unsigned v[SPP];
#pragma unroll
    for (int ch = 0; ch < SPP; ++ch) {
      v[ch] = 0;
      if (x < width) {
        if constexpr (BYTES == 1) {
          v[ch] = src[(int64_t)x * SPP + ch];
        } else {                                            // (rows of 16-bit samples start on even bytes of the staging area)
          const unsigned w = reinterpret_cast<const unsigned short*>(src)[x];
          v[ch] = big_endian ? ((w >> 8) | (w << 8)) & 0xffffu : w;
        }
      }
    }
    if (predictor) {
#pragma unroll
      for (int ch = 0; ch < SPP; ++ch) {
        const unsigned inc = tf_wave_inclusive(v[ch], lane) + carry[ch];
        carry[ch] = __shfl(inc, 63, 64);
        v[ch] = inc & kMask;
      }
    }
    if (x < width) {
      if constexpr (SPP == 3) {
        tf_store<OUT>(out, o0 + x, (19595u * v[0] + 38470u * v[1] + 7471u * v[2] + 0x8000u) >> 16, 4);
      } else {
        tf_store<OUT>(out, o0 + x, v[0], BYTES);
      }
    }
  }
}

struct TfLayout {
  int64_t staged, pb_off, pb_len, pb_expect, pb_dst, pb_frame, pb_work;
  int64_t df_out_off, df_out_cap, df_out_len, df_status, df_trailer, df_judge, df_slots, frame_bytes, total;
};

// max_mask: 7 for pl_tiff_decode (as ever), 15 for pl_tiff_decode_ex
__host__ bool tf_layout(int64_t n_frames, int64_t n_strips, int64_t max_strip_bytes, int width, int height, int bits,
                        int samples_per_pixel, int compressions, int max_mask, TfLayout* lay) {
  if (n_frames < 1 || n_frames > 65535 || n_strips < 1 || n_strips > ((int64_t)1 << 31) - 1) return false;
  if (width < 1 || height < 1 || max_strip_bytes < 0 || max_strip_bytes > ((int64_t)1 << 36)) return false;
  if (!((samples_per_pixel == 1 && (bits == 8 || bits == 16)) || (samples_per_pixel == 3 && bits == 8))) return false;
  if (compressions < 1 || compressions > max_mask) return false;
  const int64_t frame_bytes = (int64_t)width * height * samples_per_pixel * (bits / 8);
  if (frame_bytes > ((int64_t)1 << 31) - 1) return false;
  if ((compressions & 2) && n_strips > 65535) return false; // the PackBits passes put the stream on a grid axis
  auto up = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
  int64_t at = 0;
  lay->frame_bytes = frame_bytes;
  lay->staged = at, at += up(n_frames * frame_bytes);
  lay->pb_off = lay->pb_len = lay->pb_expect = lay->pb_dst = lay->pb_frame = lay->pb_work = -1;
  if (compressions & 2) {
    lay->pb_off = at, at += up(n_strips * 8);
    lay->pb_len = at, at += up(n_strips * 8);
    lay->pb_expect = at, at += up(n_strips * 8);
    lay->pb_dst = at, at += up(n_strips * 8);
    lay->pb_frame = at, at += up(n_strips * 4);
    lay->pb_work = at, at += up(pl_packbits_work_bytes(n_strips, max_strip_bytes));
  }
  lay->df_out_off = lay->df_out_cap = lay->df_out_len = lay->df_status = lay->df_trailer = lay->df_judge = lay->df_slots = -1;
  if (compressions & 8) {
    // a strip holds at most the frame: the bound of the Adler tiles (the host is not told the strips' rows)
    const int64_t slots = pl_adler32_slots_bytes(n_strips, frame_bytes);
    if (slots < 0) return false;
    lay->df_out_off = at, at += up(n_strips * 8);
    lay->df_out_cap = at, at += up(n_strips * 8);
    lay->df_out_len = at, at += up(n_strips * 8);
    lay->df_status = at, at += up(n_strips * 4);
    lay->df_trailer = at, at += up(n_strips * 4);
    lay->df_judge = at, at += up(n_strips * 4);             // (zeroed together with the trailers)
    lay->df_slots = at, at += slots;
  }
  lay->total = at;
  return true;
}

#define TF_REQUIRE(cond, msg)              \
  do {                                     \
    if (!(cond)) {                         \
      pl_set_error("%s: %s", who, msg);    \
      return PL_ERR_INVALID_ARG;           \
    }                                      \
  } while (0)

// pl_tiff_decode (max_mask 7) and pl_tiff_decode_ex (max_mask 15): one body, the Deflate launches only under mask bit 8
__host__ int tf_decode(const char* who, int max_mask, const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_strip_off,
                       const int64_t* d_strip_len, const int32_t* d_strip_desc, int64_t n_strips, int64_t max_strip_bytes,
                       const int32_t* d_frame_flags, int64_t n_frames, int width, int height, int bits, int samples_per_pixel,
                       int compressions, void* d_out, int out_kind, int32_t* d_status, unsigned char* d_work, void* stream) {
  if (!((samples_per_pixel == 1 && (bits == 8 || bits == 16)) || (samples_per_pixel == 3 && bits == 8))) {
    pl_set_error("%s: unsupported samples (%d x %d bits): grey of 8 or 16 bits, RGB of 8", who, samples_per_pixel, bits);
    return PL_ERR_UNSUPPORTED;
  }
  TF_REQUIRE(d_bytes && d_strip_off && d_strip_len && d_strip_desc && d_frame_flags && d_out && d_status && d_work, "null pointer");
  TF_REQUIRE(((uintptr_t)d_bytes & 3) == 0, "the byte buffer must start on a 4-byte boundary (strips inside it may start anywhere)");
  TF_REQUIRE(((uintptr_t)d_work & 15) == 0, "d_work must start on a 16-byte boundary");
  TF_REQUIRE(out_kind >= 0 && out_kind <= 2, "out_kind 0 (container dtype), 1 (uint16) or 2 (float64)");
  TF_REQUIRE(nbytes >= 0, "bad buffer size");
  TfLayout lay;
  TF_REQUIRE(tf_layout(n_frames, n_strips, max_strip_bytes, width, height, bits, samples_per_pixel, compressions, max_mask, &lay),
             max_mask == 7 ? "1 <= n_frames <= 65535, n_strips >= 1 (<= 65535 with PackBits), width, height >= 1, a frame below 2 GiB, "
                             "compressions a mask of 1 (none) | 2 (PackBits) | 4 (LZW)"
                           : "1 <= n_frames <= 65535, n_strips >= 1 (<= 65535 with PackBits), width, height >= 1, a frame below 2 GiB "
                             "(at most 65535 x 16 KiB with Deflate), compressions a mask of 1 (none) | 2 (PackBits) | 4 (LZW) | 8 (Deflate)");
  hipStream_t st = (hipStream_t)stream;
  bool zeroed = hipMemsetAsync(d_status, 0, (size_t)n_frames * 4, st) == hipSuccess;
  if (compressions & 8)
    zeroed = zeroed && hipMemsetAsync(d_work + lay.df_trailer, 0, (size_t)(lay.df_slots - lay.df_trailer), st) == hipSuccess;
  if (!zeroed) {
    pl_set_error("%s: memset failed", who);
    return PL_ERR_HIP;
  }
  const int ib = bits / 8;
  const int64_t row_bytes = (int64_t)width * samples_per_pixel * ib;
  unsigned char* staged = d_work + lay.staged;
  const bool packbits = (compressions & 2) != 0;
  int64_t* pb_off = packbits ? reinterpret_cast<int64_t*>(d_work + lay.pb_off) : nullptr;
  int64_t* pb_len = packbits ? reinterpret_cast<int64_t*>(d_work + lay.pb_len) : nullptr;
  int64_t* pb_expect = packbits ? reinterpret_cast<int64_t*>(d_work + lay.pb_expect) : nullptr;
  int64_t* pb_dst = packbits ? reinterpret_cast<int64_t*>(d_work + lay.pb_dst) : nullptr;
  int32_t* pb_frame = packbits ? reinterpret_cast<int32_t*>(d_work + lay.pb_frame) : nullptr;
  hipLaunchKernelGGL(tiff_check_kernel, dim3((unsigned)pl_cdiv(n_strips, kTfThreads)), dim3(kTfThreads), 0, st, d_strip_off,
                     d_strip_len, d_strip_desc, n_strips, nbytes, max_strip_bytes, n_frames, height, row_bytes, compressions,
                     pb_off, pb_len, pb_expect, pb_dst, pb_frame, d_status);
  if (compressions & 1) {
    int64_t bx = pl_cdiv(max_strip_bytes / 4, (int64_t)kTfThreads * 4);
    if (bx < 1) bx = 1;
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(tiff_raw_kernel, dim3((unsigned)n_strips, (unsigned)bx), dim3(kTfThreads), 0, st, d_bytes, nbytes,
                       d_strip_off, d_strip_len, d_strip_desc, max_strip_bytes, n_frames, height, row_bytes, compressions,
                       staged, d_status);
  }
  if (packbits)
    pl_packbits_expand(d_bytes, nbytes, pb_off, pb_len, n_strips, max_strip_bytes, staged, d_status, d_work + lay.pb_work,
                       PlPackbitsGeom{pb_expect, pb_dst, pb_frame}, st);
  if (compressions & 4)
    hipLaunchKernelGGL(tiff_lzw_kernel, dim3((unsigned)n_strips), dim3(PL_WAVE), 0, st, d_bytes, nbytes, d_strip_off, d_strip_len,
                       d_strip_desc, max_strip_bytes, n_frames, height, row_bytes, compressions, staged, d_status);
  if (compressions & 8) {
    int64_t* out_off = reinterpret_cast<int64_t*>(d_work + lay.df_out_off);
    int64_t* out_cap = reinterpret_cast<int64_t*>(d_work + lay.df_out_cap);
    int64_t* out_len = reinterpret_cast<int64_t*>(d_work + lay.df_out_len);
    int32_t* strip_status = reinterpret_cast<int32_t*>(d_work + lay.df_status);
    uint32_t* trailer = reinterpret_cast<uint32_t*>(d_work + lay.df_trailer);
    int32_t* judge = reinterpret_cast<int32_t*>(d_work + lay.df_judge);
    const dim3 per_strip((unsigned)pl_cdiv(n_strips, kTfThreads));
    hipLaunchKernelGGL(tiff_deflate_table_kernel, per_strip, dim3(kTfThreads), 0, st, d_strip_off, d_strip_len, d_strip_desc, n_strips,
                       nbytes, max_strip_bytes, n_frames, height, row_bytes, compressions, out_off, out_cap, strip_status);
    // a stream that goes on beyond the strip's rows is no error (libtiff stops reading there): overflow 0, not judged
    pl_inflate_launch(true, d_bytes, nbytes, d_strip_off, d_strip_len, n_strips, 1, staged, out_off, out_cap, out_len, strip_status,
                      PnChecked{trailer, judge, nullptr, lay.frame_bytes, 0}, st);
    pl_adler32_launch(staged, n_frames * lay.frame_bytes, out_off, out_len, n_strips, lay.frame_bytes, judge, trailer, 16, nullptr,
                      strip_status, d_work + lay.df_slots, st);
    hipLaunchKernelGGL(tiff_deflate_verdict_kernel, per_strip, dim3(kTfThreads), 0, st, d_strip_desc, n_strips, n_frames,
                       strip_status, out_cap, out_len, d_status);
  }
  const dim3 grid((unsigned)pl_cdiv(height, kTfThreads / PL_WAVE), (unsigned)n_frames);
#define TF_FINISH(BYTES, SPP, OUT)                                                                                            \
  hipLaunchKernelGGL((tiff_finish_kernel<BYTES, SPP, OUT>), grid, dim3(kTfThreads), 0, st, staged, d_frame_flags, width, height, \
                     d_out, d_status)
#define TF_OUT(BYTES, SPP)                     \
  if (out_kind == 0) TF_FINISH(BYTES, SPP, 0); \
  else if (out_kind == 1) TF_FINISH(BYTES, SPP, 1); \
  else TF_FINISH(BYTES, SPP, 2)
  if (samples_per_pixel == 3) { TF_OUT(1, 3); }
  else if (ib == 1) { TF_OUT(1, 1); }
  else { TF_OUT(2, 1); }
#undef TF_OUT
#undef TF_FINISH
  return pl_check_launch(who);
}
#undef TF_REQUIRE

}  // namespace

extern "C" int64_t pl_tiff_work_bytes(int64_t n_frames, int64_t n_strips, int64_t max_strip_bytes, int width, int height,
                                      int bits, int samples_per_pixel, int compressions) {
  TfLayout lay;
  return tf_layout(n_frames, n_strips, max_strip_bytes, width, height, bits, samples_per_pixel, compressions, 7, &lay) ? lay.total : -1;
}

extern "C" int64_t pl_tiff_work_bytes_ex(int64_t n_frames, int64_t n_strips, int64_t max_strip_bytes, int width, int height,
                                         int bits, int samples_per_pixel, int compressions) {
  TfLayout lay;
  return tf_layout(n_frames, n_strips, max_strip_bytes, width, height, bits, samples_per_pixel, compressions, 15, &lay) ? lay.total : -1;
}

extern "C" int pl_tiff_decode(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_strip_off,
                              const int64_t* d_strip_len, const int32_t* d_strip_desc, int64_t n_strips,
                              int64_t max_strip_bytes, const int32_t* d_frame_flags, int64_t n_frames, int width, int height,
                              int bits, int samples_per_pixel, int compressions, void* d_out, int out_kind, int32_t* d_status,
                              unsigned char* d_work, void* stream) {
  return tf_decode("pl_tiff_decode", 7, d_bytes, nbytes, d_strip_off, d_strip_len, d_strip_desc, n_strips, max_strip_bytes,
                   d_frame_flags, n_frames, width, height, bits, samples_per_pixel, compressions, d_out, out_kind, d_status, d_work,
                   stream);
}

extern "C" int pl_tiff_decode_ex(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_strip_off,
                                 const int64_t* d_strip_len, const int32_t* d_strip_desc, int64_t n_strips,
                                 int64_t max_strip_bytes, const int32_t* d_frame_flags, int64_t n_frames, int width, int height,
                                 int bits, int samples_per_pixel, int compressions, void* d_out, int out_kind, int32_t* d_status,
                                 unsigned char* d_work, void* stream) {
  return tf_decode("pl_tiff_decode_ex", 15, d_bytes, nbytes, d_strip_off, d_strip_len, d_strip_desc, n_strips, max_strip_bytes,
                   d_frame_flags, n_frames, width, height, bits, samples_per_pixel, compressions, d_out, out_kind, d_status, d_work,
                   stream);
}
