// Adler-32 (zlib.adler32, RFC 1950) of byte ranges resident on the device: the checksum a zlib stream ends with, next to the
// CRC-32 of zip_kernels.h.  Users: pl_adler32 (here), pl_inflate_checked and pl_png_decode_checked (png.hip, through
// pl_adler32_launch of pl_common.h).
//
// The arithmetic.  M = 65521.  For the bytes d_0 .. d_(n-1) of a range
//   A = 1 + sum d_i                          mod M
//   B = sum over i of the running A          mod M   =   n + sum (n - i) d_i
//   adler32 = B << 16 | A
// so a piece p of the range (a tile, or a thread's bytes inside a tile) is described by (S, W, m): S = the sum of its bytes,
// W = sum (m - i) d_i with i counted inside the piece, m its length.  Pieces combine as zlib's adler32_combine does, without
// the "1", which belongs to the whole range and is added once by the fold:
//   S = S1 + S2,   W = W1 + m2 . S1 + W2        (every byte of piece 1 is counted m2 more times)
// A piece that is followed by r more bytes of the range therefore contributes W + r . S to B, and pieces are computed in any
// order and folded with plain sums.
//   ad_tile_kernel  grid (range, tile of 16 KiB), 256 threads.  The aligned 16-byte pieces that hold the tile go to LDS as
//                   they lie (never a dword that holds no byte of the range); dword i at index
//                   (i % 16) * 257 + i / 16, so that the threads' walk -- thread t owns bytes 64 t .. 64 t + 63, funnelled
//                   with v_alignbit for an odd source alignment -- reads consecutive banks (the staging of
//                   zp_crc_tile_kernel).  A thread's 64 bytes: S <= 16 320 and W <= 530 400; with the r <= 16 320 bytes that
//                   follow it inside the tile W + r . S stays below 2.7e8, which fits 32 bits -- the SUM of those over a tile
//                   of 0xFF bytes (3.4e10) does not, so every thread reduces its term modulo M before the block adds them.
//                   One (S mod M, W mod M) pair into the tile's slot.
//   ad_fold_kernel  one wave per range: A = 1 + sum S_k, B = len + sum (W_k + (bytes after tile k) . S_k), every product of
//                   two residues (< 2^32) formed in 64 bits.  Length 0 gives 1.
// Slots instead of atomics: the order of the launches is the only synchronisation.
//
// A translation unit of its own in the library.  The CPU emulator of the tests builds a fixed list of files, png.hip among
// them: there png.hip includes this file after pl_common.h (PL_ADLER32_IN_PNG), which is why nothing here may collide with
// png.hip's names.
#ifndef PL_ADLER32_IN_PNG
#include "pl_common.h"
#endif

namespace {

constexpr unsigned kAdMod = 65521u;
constexpr int kAdTile = 16384;
constexpr int kAdThreads = 256;
constexpr int kAdOwn = kAdTile / kAdThreads;                // 64 bytes a thread
constexpr int kAdRowStride = kAdThreads + 1;                // LDS: dword i at (i % 16) * 257 + i / 16
constexpr int64_t kAdMaxLen = (int64_t)65535 * kAdTile;     // the tiles of a range are blockIdx.y

// four more bytes (the dword w, byte 0 first): W += 4 S + 4 b0 + 3 b1 + 2 b2 + b3, S += b0 + b1 + b2 + b3
__device__ __forceinline__ void ad_word(unsigned w, unsigned& s, unsigned& ws) {
#ifdef PL_HIPEMU
  const unsigned b0 = w & 255u, b1 = (w >> 8) & 255u, b2 = (w >> 16) & 255u, b3 = w >> 24;
  ws += 4u * s + 4u * b0 + 3u * b1 + 2u * b2 + b3;
  s += b0 + b1 + b2 + b3;
#else
  ws = __builtin_amdgcn_udot4(w, 0x01020304u, ws + 4u * s, false);
  s = __builtin_amdgcn_udot4(w, 0x01010101u, s, false);
#endif
}

// (differences of lengths, never sums of an offset and a length: nothing here can overflow)
__device__ __forceinline__ bool ad_range_ok(int64_t off, int64_t len, int64_t nbytes, int64_t max_len) {
  return off >= 0 && len >= 0 && off <= nbytes && len <= nbytes - off && len <= max_len;
}

// gate: null, or one word per range -- a range whose word is 0 is skipped by both kernels (nothing read, nothing written)
__global__ void __launch_bounds__(kAdThreads)
ad_tile_kernel(const unsigned char* __restrict__ bytes, int64_t nbytes, const int64_t* __restrict__ r_off,
               const int64_t* __restrict__ r_len, int64_t max_len, int64_t max_tiles, const int32_t* __restrict__ gate,
               uint2* __restrict__ slots) {
  __shared__ unsigned s_tile[16 * kAdRowStride];
  __shared__ unsigned s_part[2 * (kAdThreads / PL_WAVE)];
  const int64_t r = blockIdx.x, k = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (PL_WAVE - 1);
  if (gate && !gate[r]) return;
  const int64_t off = r_off[r], len = r_len[r];
  if (!ad_range_ok(off, len, nbytes, max_len) || k * kAdTile >= len) return;
  const int64_t start = off + k * kAdTile;                  // the tile: tl bytes from byte `start` of the buffer
  const int tl = len - k * kAdTile < kAdTile ? (int)(len - k * kAdTile) : kAdTile;
  // the aligned 16-byte pieces that hold the tile, as ADDRESSES.  Only dwords that hold a byte of the RANGE are read (the
  // checked inflate is not told how large its caller's output buffer is): the first and the last piece of a range may reach
  // beyond them and go dword by dword, zeros for what lies outside
  const uintptr_t base = reinterpret_cast<uintptr_t>(bytes), a0 = base + (uintptr_t)start, a16 = a0 & ~(uintptr_t)15;
  const uintptr_t first = (base + (uintptr_t)off) & ~(uintptr_t)3;
  const uintptr_t end = (base + (uintptr_t)(off + len) + 3u) & ~(uintptr_t)3;  // (the dword that holds the last byte is read whole)
  const int skew = (int)(a0 - a16);                          // 0 .. 15: the tile's first byte inside piece 0
  const int pieces = (skew + tl + 15) >> 4;                  // <= 1025
  for (int p = tid; p < pieces; p += kAdThreads) {
    const uintptr_t a = a16 + (uintptr_t)p * 16u;
    uint4 q;
    if (a >= first && a + 16u <= end) {
      q = *reinterpret_cast<const uint4*>(a);
    } else {
      unsigned d[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) d[i] = (a + 4u * i >= first && a + 4u * i + 4u <= end) ? *reinterpret_cast<const unsigned*>(a + 4u * i) : 0u;
      q = uint4{d[0], d[1], d[2], d[3]};
    }
    const int i0 = 4 * p;                                    // dwords i0 .. i0 + 3: four rows, one column
    const int col = i0 >> 4, row = i0 & 15;
    s_tile[row * kAdRowStride + col] = q.x, s_tile[(row + 1) * kAdRowStride + col] = q.y;
    s_tile[(row + 2) * kAdRowStride + col] = q.z, s_tile[(row + 3) * kAdRowStride + col] = q.w;
  }
  __syncthreads();
  // the thread's bytes: 64 t .. of the tile = dwords 16 t + ds .. of the staged ones, shifted by sh bits
  const int ds = skew >> 2;
  const unsigned sh = (unsigned)(skew & 3) * 8u;
  int mine = tl - tid * kAdOwn;
  mine = mine < 0 ? 0 : (mine > kAdOwn ? kAdOwn : mine);
  unsigned sum = 0, term = 0;
  if (mine > 0) {
    const int have = (mine + 3) >> 2;                        // dwords that hold a byte of the thread's (staged: the next one too,
    unsigned d[kAdOwn / 4 + 1];                              //  whenever a byte of it is used)
#pragma unroll
    for (int j = 0; j <= kAdOwn / 4; ++j) {
      const int i = 16 * tid + j + ds;
      d[j] = (j < have || (j == have && sh)) && (i >> 2) < pieces ? s_tile[(i & 15) * kAdRowStride + (i >> 4)] : 0u;
    }
    // all 64 positions, the bytes beyond `mine` as zeros: W64 = sum (64 - i) d_i counts every byte (64 - mine) times too often
    unsigned ws = 0;
#pragma unroll
    for (int j = 0; j < kAdOwn / 4; ++j) {
      unsigned w = sh ? __builtin_amdgcn_alignbit(d[j + 1], d[j], sh) : d[j];
      const int valid = mine - 4 * j;                        // bytes of this dword that are the thread's
      if (valid < 4) w &= valid <= 0 ? 0u : (1u << (8 * valid)) - 1u;
      ad_word(w, sum, ws);
    }
    const unsigned after = (unsigned)(tl - tid * kAdOwn - mine);                // bytes of the tile after the thread's
    term = (ws - (unsigned)(kAdOwn - mine) * sum + after * sum) % kAdMod;      // < 2.7e8 before the reduction
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                        // S <= 16 384 x 255, the terms' sum <= 256 x 65 520
    sum += (unsigned)__shfl_xor((int)sum, o, 64);
    term += (unsigned)__shfl_xor((int)term, o, 64);
  }
  if (lane == 0) s_part[2 * (tid / PL_WAVE)] = sum, s_part[2 * (tid / PL_WAVE) + 1] = term;
  __syncthreads();
  if (tid == 0) {
    unsigned s = 0, w = 0;
#pragma unroll
    for (int v = 0; v < kAdThreads / PL_WAVE; ++v) s += s_part[2 * v], w += s_part[2 * v + 1];
    slots[r * max_tiles + k] = uint2{s % kAdMod, w % kAdMod};
  }
}

// expected: null, or the Adler-32 every range should have -- a mismatch ORs `mismatch` into its status
__global__ void __launch_bounds__(PL_WAVE)
ad_fold_kernel(int64_t nbytes, const int64_t* __restrict__ r_off, const int64_t* __restrict__ r_len, int64_t max_len,
               int64_t max_tiles, const uint2* __restrict__ slots, const int32_t* __restrict__ gate,
               const uint32_t* __restrict__ expected, int mismatch, uint32_t* __restrict__ adler_out, int32_t* __restrict__ status) {
  const int64_t r = blockIdx.x;
  const int lane = threadIdx.x;
  if (gate && !gate[r]) return;
  const int64_t off = r_off[r], len = r_len[r];
  if (!ad_range_ok(off, len, nbytes, max_len)) {
    if (lane == 0) atomicOr(status + r, 1);
    return;
  }
  const int64_t tiles = (len + kAdTile - 1) / kAdTile;
  unsigned long long a = 0, b = 0;                          // at most 65 535 tiles, every term below 2^33
  for (int64_t k = lane; k < tiles; k += PL_WAVE) {
    const uint2 t = slots[r * max_tiles + k];
    const int64_t tl = len - k * kAdTile < kAdTile ? len - k * kAdTile : kAdTile;
    const unsigned long long after = (unsigned long long)((len - k * kAdTile - tl) % (int64_t)kAdMod);
    a += t.x;
    b += t.y + after * t.x % kAdMod;
  }
  unsigned ra = (unsigned)(a % kAdMod), rb = (unsigned)(b % kAdMod);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                        // 64 residues
    ra += (unsigned)__shfl_xor((int)ra, o, 64);
    rb += (unsigned)__shfl_xor((int)rb, o, 64);
  }
  const unsigned A = (1u + ra) % kAdMod, B = (unsigned)((uint64_t)(len % (int64_t)kAdMod) + rb) % kAdMod;
  const uint32_t adler = (B << 16) | A;
  if (lane == 0) {
    if (adler_out) adler_out[r] = adler;
    if (expected && expected[r] != adler) atomicOr(status + r, mismatch);
  }
}

}  // namespace

int64_t pl_adler32_slots_bytes(int64_t n_ranges, int64_t max_len) {
  if (n_ranges < 1 || n_ranges > ((int64_t)1 << 31) - 1 || max_len < 0 || max_len > kAdMaxLen) return -1;
  const int64_t max_tiles = max_len ? (max_len + kAdTile - 1) / kAdTile : 1;
  if (n_ranges > ((int64_t)1 << 50) / max_tiles) return -1;
  return (n_ranges * max_tiles * 8 + 15) & ~(int64_t)15;
}

void pl_adler32_launch(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_off, const int64_t* d_len, int64_t n_ranges,
                       int64_t max_len, const int32_t* d_gate, const uint32_t* d_expected, int mismatch, uint32_t* d_adler,
                       int32_t* d_status, unsigned char* d_slots, hipStream_t st) {
  const int64_t max_tiles = max_len ? (max_len + kAdTile - 1) / kAdTile : 1;
  uint2* slots = reinterpret_cast<uint2*>(d_slots);
  hipLaunchKernelGGL(ad_tile_kernel, dim3((unsigned)n_ranges, (unsigned)max_tiles), dim3(kAdThreads), 0, st, d_bytes, nbytes, d_off,
                     d_len, max_len, max_tiles, d_gate, slots);
  hipLaunchKernelGGL(ad_fold_kernel, dim3((unsigned)n_ranges), dim3(PL_WAVE), 0, st, nbytes, d_off, d_len, max_len, max_tiles, slots,
                     d_gate, d_expected, mismatch, d_adler, d_status);
}

extern "C" int64_t pl_adler32_work_bytes(int64_t n_ranges, int64_t max_len) { return pl_adler32_slots_bytes(n_ranges, max_len); }

extern "C" int pl_adler32(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_off, const int64_t* d_len, int64_t n_ranges,
                          int64_t max_len, uint32_t* d_adler, int32_t* d_status, unsigned char* d_work, void* stream) {
  PL_REQUIRE(d_bytes && d_off && d_len && d_adler && d_status && d_work, "null pointer");
  PL_REQUIRE(((uintptr_t)d_bytes & 3) == 0, "the byte buffer must start on a 4-byte boundary (ranges inside it may start anywhere)");
  PL_REQUIRE(((uintptr_t)d_work & 7) == 0, "d_work must start on an 8-byte boundary");
  PL_REQUIRE(nbytes >= 0 && nbytes <= ((int64_t)1 << 40), "bad buffer size");
  PL_REQUIRE(pl_adler32_slots_bytes(n_ranges, max_len) >= 0, "1 <= n_ranges < 2^31, 0 <= max_len <= 65535 x 16 KiB");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(d_status, 0, (size_t)n_ranges * 4, st) != hipSuccess) {
    pl_set_error("pl_adler32: memset failed");
    return PL_ERR_HIP;
  }
  pl_adler32_launch(d_bytes, nbytes, d_off, d_len, n_ranges, max_len, nullptr, nullptr, 0, d_adler, d_status, d_work, st);
  return pl_check_launch("pl_adler32");
}
