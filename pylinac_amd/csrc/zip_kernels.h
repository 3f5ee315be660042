// CRC-32 (zlib.crc32) of byte ranges resident on the device, and the members of a ZIP archive -> their bytes: the second half of
// png.hip, which includes this file after inflate_kernel (file-local there).  The reference's users hand it archives
// (`CatPhan504.from_zip`, `DicomImageStack.from_zip`): 80 - 300 independent raw Deflate streams, the shape inflate_kernel is
// good at.  What `zipfile` adds to `zlib.decompress(data, -15)` is the CRC-32 of every member it reads.
//
// The arithmetic.  The reflected polynomial P = 0xEDB88320: bit 31 of a word is x^0, x^8 is 0x00800000, a step of the CRC
// register is a multiplication by x.  With raw(p) the register run from 0 over the bytes p, no final inversion,
//   crc32(D) = 0xFFFFFFFF ^ (0xFFFFFFFF . x^(8 L))  ^  XOR over pieces p of  raw(p) . x^(8 . bytes of D after p)
// where `.` is the product modulo P (gfx950 has no carry-less multiply: 32 shift-and-xor steps).  Pieces are therefore
// computed in any order and folded with XOR.
//   zp_crc_tile_kernel  grid (range, tile of 16 KiB), 256 threads.  The aligned 16-byte pieces that hold the tile go to LDS
//                       as they lie (piece = the caller's allocation rounded to dwords, never a dword outside it); dword i at
//                       index (i % 16) * 257 + i / 16, so that the threads' walk -- thread t owns bytes 64 t .. 64 t + 63,
//                       funnelled with v_alignbit for an odd source alignment -- reads consecutive banks.  raw() is
//                       slice-by-4 over tables in LDS (4 KiB a block; measured 1.5 x the table-free form,
//                       scripts/ubench/crc32_variants.hip); then the power for the bytes after the thread's inside the tile
//                       (a constant table for a full tile, binary exponentiation for the last one), XOR over the block, the
//                       power for the bytes after the tile, ONE word into the tile's slot.
//   zp_crc_fold_kernel  one wave per range: XOR of the slots, the init term, inversion.  Length 0 gives 0.
// Slots instead of an atomic XOR: the order of the launches is the only synchronisation.
//
// pl_zip_extract: zip_check_kernel (every descriptor; the tables inflate_kernel reads), inflate_kernel with wrapper 0 and the
// member's size as capacity (a member that is not Deflate is an empty stream of capacity 0 there: an exiting wave), the
// stored members' funnel copy (after the inflate launch, which stores out_len for every stream it is given), the CRC pair
// over the OUTPUT.
namespace {

constexpr unsigned kZpPoly = 0xEDB88320u;
constexpr unsigned kZpOne = 0x80000000u;                     // x^0
constexpr int kZpTile = 16384;
constexpr int kZpThreads = 256;
constexpr int kZpOwn = kZpTile / kZpThreads;                // 64 bytes a thread
constexpr int kZpRowStride = kZpThreads + 1;                // LDS: dword i at (i % 16) * 257 + i / 16
constexpr int kZpPowers = 40;                               // x^(8 . 2^k), k < 40: lengths below 2^40
constexpr int64_t kZpMaxLen = (int64_t)65535 * kZpTile;     // the tiles of a range are blockIdx.y

__host__ __device__ constexpr unsigned zp_step(unsigned v) { return (v >> 1) ^ ((v & 1u) ? kZpPoly : 0u); }   // v . x

// a . b modulo P
__host__ __device__ constexpr unsigned zp_mul(unsigned a, unsigned b) {
  unsigned r = 0;
  for (int i = 0; i < 32; ++i) {
    r ^= (a & (kZpOne >> i)) ? b : 0u;
    b = zp_step(b);
  }
  return r;
}

struct ZpTables {
  unsigned pow2[kZpPowers];                                  // x^(8 . 2^k)
  unsigned after[kZpThreads];                                // x^(8 . 64 . k): k threads' bytes follow inside a full tile
  unsigned slice[4][256];                                    // slice-by-4: slice[k][b] = the register b, 8 (k + 1) steps on
};

constexpr ZpTables zp_make_tables() {
  ZpTables t{};
  unsigned p = kZpOne;
  for (int i = 0; i < 8; ++i) p = zp_step(p);
  for (int k = 0; k < kZpPowers; ++k) {
    t.pow2[k] = p;
    p = zp_mul(p, p);
  }
  unsigned q = kZpOne;
  for (int k = 0; k < kZpThreads; ++k) {
    t.after[k] = q;
    q = zp_mul(q, t.pow2[6]);                                // 64 bytes
  }
  for (int b = 0; b < 256; ++b) {
    unsigned v = (unsigned)b;
    for (int i = 0; i < 8; ++i) v = zp_step(v);
    t.slice[0][b] = v;
  }
  for (int k = 1; k < 4; ++k)
    for (int b = 0; b < 256; ++b) t.slice[k][b] = (t.slice[k - 1][b] >> 8) ^ t.slice[0][t.slice[k - 1][b] & 255u];
  return t;
}

__device__ const ZpTables kZp = zp_make_tables();

// the register after 32 more message bits / after 8: slice-by-4 over the block's copy of the tables in LDS
__device__ __forceinline__ unsigned zp_word(unsigned crc, unsigned w, const unsigned* tab) {
  crc ^= w;
  return tab[768 + (crc & 255u)] ^ tab[512 + ((crc >> 8) & 255u)] ^ tab[256 + ((crc >> 16) & 255u)] ^ tab[crc >> 24];
}
__device__ __forceinline__ unsigned zp_byte(unsigned crc, unsigned b, const unsigned* tab) {
  return (crc >> 8) ^ tab[(crc ^ b) & 255u];
}

// x^(8 n) in every lane of the wave; every lane calls this with the same n (0 <= n < 2^40): lane k holds the factor of bit k,
// a butterfly multiplies them
__device__ __forceinline__ unsigned zp_xpow8_wave(int64_t n, int lane) {
  unsigned f = (lane < kZpPowers && ((n >> lane) & 1)) ? kZp.pow2[lane] : kZpOne;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) f = zp_mul(f, (unsigned)__shfl_xor((int)f, o, 64));
  return f;
}

// a lane on its own (n < 2^14: the bytes after a thread's inside a partial tile)
__device__ __forceinline__ unsigned zp_xpow8_lane(unsigned n) {
  unsigned f = kZpOne;
  for (int k = 0; k < 14; ++k)
    if ((n >> k) & 1u) f = zp_mul(f, kZp.pow2[k]);
  return f;
}

// (differences of lengths, never sums of an offset and a length: nothing here can overflow)
__device__ __forceinline__ bool zp_range_ok(int64_t off, int64_t len, int64_t nbytes, int64_t max_len) {
  return off >= 0 && len >= 0 && off <= nbytes && len <= nbytes - off && len <= max_len;
}

__global__ void __launch_bounds__(kZpThreads)
zp_crc_tile_kernel(const unsigned char* __restrict__ bytes, int64_t nbytes, const int64_t* __restrict__ r_off,
                   const int64_t* __restrict__ r_len, int64_t max_len, int64_t max_tiles, const int32_t* __restrict__ status,
                   unsigned* __restrict__ slots) {
  __shared__ unsigned s_tile[16 * kZpRowStride];
  __shared__ unsigned s_tab[4 * 256];
  __shared__ unsigned s_part[kZpThreads / PL_WAVE];
  const int64_t r = blockIdx.x, k = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (PL_WAVE - 1);
  if (status[r]) return;                                    // (pl_zip_extract: a member already flagged)
  const int64_t off = r_off[r], len = r_len[r];
  if (!zp_range_ok(off, len, nbytes, max_len) || k * kZpTile >= len) return;
  const int64_t start = off + k * kZpTile;                  // the tile: tl bytes from byte `start` of the buffer
  const int tl = len - k * kZpTile < kZpTile ? (int)(len - k * kZpTile) : kZpTile;
  // the aligned 16-byte pieces that hold the tile, as ADDRESSES (the buffer itself starts on a dword only); the first and
  // the last piece may reach beyond the buffer's dwords: those go dword by dword, zeros for what lies outside
  const uintptr_t first = reinterpret_cast<uintptr_t>(bytes), a0 = first + (uintptr_t)start, a16 = a0 & ~(uintptr_t)15;
  const uintptr_t end = first + (uintptr_t)((nbytes + 3) & ~(int64_t)3);       // (the dword that holds the last byte is read whole)
  const int skew = (int)(a0 - a16);                          // 0 .. 15: the tile's first byte inside piece 0
  const int pieces = (skew + tl + 15) >> 4;                  // <= 1025
  for (int i = tid; i < 4 * 256; i += kZpThreads) s_tab[i] = kZp.slice[i >> 8][i & 255];
  for (int p = tid; p < pieces; p += kZpThreads) {
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
    s_tile[row * kZpRowStride + col] = q.x, s_tile[(row + 1) * kZpRowStride + col] = q.y;
    s_tile[(row + 2) * kZpRowStride + col] = q.z, s_tile[(row + 3) * kZpRowStride + col] = q.w;
  }
  __syncthreads();
  // the thread's bytes: 64 t .. of the tile = dwords 16 t + ds .. of the staged ones, shifted by sh bits
  const int ds = skew >> 2;
  const unsigned sh = (unsigned)(skew & 3) * 8u;
  int mine = tl - tid * kZpOwn;
  mine = mine < 0 ? 0 : (mine > kZpOwn ? kZpOwn : mine);
  unsigned crc = 0;
  if (mine > 0) {
    const int have = (mine + 3) >> 2;                        // dwords that hold a byte of the thread's (staged: the next one too,
    unsigned d[kZpOwn / 4 + 1];                              //  whenever a byte of it is used)
#pragma unroll
    for (int j = 0; j <= kZpOwn / 4; ++j) {
      const int i = 16 * tid + j + ds;
      d[j] = (j < have || (j == have && sh)) && (i >> 2) < pieces ? s_tile[(i & 15) * kZpRowStride + (i >> 4)] : 0u;
    }
#pragma unroll
    for (int j = 0; j < kZpOwn / 4; ++j) {
      const unsigned w = sh ? __builtin_amdgcn_alignbit(d[j + 1], d[j], sh) : d[j];
      if (4 * j + 4 <= mine) {
        crc = zp_word(crc, w, s_tab);
      } else {
        for (int b = 0; b < mine - 4 * j; ++b) crc = zp_byte(crc, (w >> (8 * b)) & 0xffu, s_tab);
      }
    }
    const int after = tl - tid * kZpOwn - mine;              // bytes of the tile after the thread's
    crc = zp_mul(crc, tl == kZpTile ? kZp.after[kZpThreads - 1 - tid] : zp_xpow8_lane((unsigned)after));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) crc ^= (unsigned)__shfl_xor((int)crc, o, 64);
  if (lane == 0) s_part[tid / PL_WAVE] = crc;
  __syncthreads();
  if (tid < PL_WAVE) {                                      // the first wave, every lane: the power is a butterfly over the wave
    unsigned v = 0;
#pragma unroll
    for (int w = 0; w < kZpThreads / PL_WAVE; ++w) v ^= s_part[w];
    const unsigned f = zp_xpow8_wave(len - k * kZpTile - tl, lane);
    if (tid == 0) slots[r * max_tiles + k] = zp_mul(v, f);
  }
}

// expected: null, or the CRC-32 every range should have -- a mismatch sets bit 3 of its status (pl_zip_extract)
__global__ void __launch_bounds__(PL_WAVE)
zp_crc_fold_kernel(int64_t nbytes, const int64_t* __restrict__ r_off, const int64_t* __restrict__ r_len, int64_t max_len,
                   int64_t max_tiles, const unsigned* __restrict__ slots, const uint32_t* __restrict__ expected,
                   uint32_t* __restrict__ crc_out, int32_t* __restrict__ status) {
  const int64_t r = blockIdx.x;
  const int lane = threadIdx.x;
  if (status[r]) return;
  const int64_t off = r_off[r], len = r_len[r];
  if (!zp_range_ok(off, len, nbytes, max_len)) {
    if (lane == 0) atomicOr(status + r, 1);
    return;
  }
  const int64_t tiles = (len + kZpTile - 1) / kZpTile;
  unsigned v = 0;
  for (int64_t k = lane; k < tiles; k += PL_WAVE) v ^= slots[r * max_tiles + k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v ^= (unsigned)__shfl_xor((int)v, o, 64);
  const unsigned init = zp_mul(0xFFFFFFFFu, zp_xpow8_wave(len, lane));
  const uint32_t crc = 0xFFFFFFFFu ^ init ^ v;
  if (lane == 0) {
    if (crc_out) crc_out[r] = crc;
    if (expected && expected[r] != crc) atomicOr(status + r, 8);
  }
}

__host__ int64_t zp_crc_slots_bytes(int64_t n_ranges, int64_t max_len) {
  if (n_ranges < 1 || n_ranges > ((int64_t)1 << 31) - 1 || max_len < 0 || max_len > kZpMaxLen) return -1;
  const int64_t max_tiles = max_len ? (max_len + kZpTile - 1) / kZpTile : 1;
  if (n_ranges > ((int64_t)1 << 50) / max_tiles) return -1;
  return (n_ranges * max_tiles * 4 + 15) & ~(int64_t)15;
}

// the two launches (status: zeroed or filled by the caller's earlier launches)
__host__ void zp_crc_launch(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_off, const int64_t* d_len, int64_t n_ranges,
                            int64_t max_len, const uint32_t* d_expected, uint32_t* d_crc, int32_t* d_status, unsigned char* d_slots,
                            hipStream_t st) {
  const int64_t max_tiles = max_len ? (max_len + kZpTile - 1) / kZpTile : 1;
  unsigned* slots = reinterpret_cast<unsigned*>(d_slots);
  hipLaunchKernelGGL(zp_crc_tile_kernel, dim3((unsigned)n_ranges, (unsigned)max_tiles), dim3(kZpThreads), 0, st, d_bytes, nbytes, d_off,
                     d_len, max_len, max_tiles, d_status, slots);
  hipLaunchKernelGGL(zp_crc_fold_kernel, dim3((unsigned)n_ranges), dim3(PL_WAVE), 0, st, nbytes, d_off, d_len, max_len, max_tiles,
                     slots, d_expected, d_crc, d_status);
}

// ---- the members of an archive ----------------------------------------------------------------------------------------------
constexpr int kZpStored = 0, kZpDeflate = 8;

struct ZpMember {
  bool ok;
  int method;
  int64_t in_off, in_len, out_off, size;
};

__device__ __forceinline__ ZpMember zp_member(const int64_t* __restrict__ in_off, const int64_t* __restrict__ in_len,
                                              const int32_t* __restrict__ method, const int64_t* __restrict__ out_off,
                                              const int64_t* __restrict__ out_size, int64_t m, int64_t nbytes, int64_t out_bytes,
                                              int64_t max_size) {
  ZpMember t;
  t.method = method[m], t.in_off = in_off[m], t.in_len = in_len[m], t.out_off = out_off[m], t.size = out_size[m];
  t.ok = (t.method == kZpStored || t.method == kZpDeflate) && zp_range_ok(t.in_off, t.in_len, nbytes, nbytes) &&
         zp_range_ok(t.out_off, t.size, out_bytes, max_size) && (t.method != kZpStored || t.in_len == t.size);
  return t;
}

__global__ void __launch_bounds__(kZpThreads)
zip_check_kernel(const int64_t* __restrict__ in_off, const int64_t* __restrict__ in_len, const int32_t* __restrict__ method,
                 const int64_t* __restrict__ out_off, const int64_t* __restrict__ out_size, int64_t n_members, int64_t nbytes,
                 int64_t out_bytes, int64_t max_size, int64_t* __restrict__ inf_off, int64_t* __restrict__ inf_len,
                 int64_t* __restrict__ inf_cap, int32_t* __restrict__ status) {
  const int64_t m = (int64_t)blockIdx.x * kZpThreads + threadIdx.x;
  if (m >= n_members) return;
  const ZpMember t = zp_member(in_off, in_len, method, out_off, out_size, m, nbytes, out_bytes, max_size);
  const bool deflate = t.ok && t.method == kZpDeflate;      // every other member: an empty stream of capacity 0
  inf_off[m] = deflate ? t.in_off : 0;
  inf_len[m] = deflate ? t.in_len : 0;
  inf_cap[m] = deflate ? t.size : 0;
  status[m] = t.ok ? 0 : 1;
}

// the stored members (the dword funnel of tiff_raw_kernel), and out_len of every member that is not Deflate
__global__ void __launch_bounds__(kZpThreads)
zip_stored_kernel(const unsigned char* __restrict__ bytes, int64_t nbytes, const int64_t* __restrict__ in_off,
                  const int64_t* __restrict__ in_len, const int32_t* __restrict__ method, const int64_t* __restrict__ out_off,
                  const int64_t* __restrict__ out_size, int64_t out_bytes, int64_t max_size, unsigned char* __restrict__ out,
                  int64_t* __restrict__ out_len) {
  const int64_t m = blockIdx.x;                             // (blockIdx.y: the member's pieces)
  const ZpMember t = zp_member(in_off, in_len, method, out_off, out_size, m, nbytes, out_bytes, max_size);
  if (t.ok && t.method == kZpDeflate) return;
  if (blockIdx.y == 0 && threadIdx.x == 0) out_len[m] = t.ok ? t.size : 0;
  if (!t.ok) return;
  const int64_t n = t.size;
  unsigned char* dst = out + t.out_off;
  const unsigned char* src = bytes + t.in_off;
  int64_t head = (int64_t)((4u - (unsigned)((uintptr_t)dst & 3u)) & 3u);       // bytes up to the first aligned destination dword
  if (head > n) head = n;
  const int64_t nd = (n - head) >> 2, tail0 = head + 4 * nd;
  if (blockIdx.y == 0) {
    if ((int64_t)threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    const int64_t k = tail0 + threadIdx.x;
    if (k < n) dst[k] = src[k];
  }
  const int64_t from = t.in_off + head;                     // the buffer byte of the first dword
  const unsigned sh = (unsigned)(from & 3) * 8u;
  const unsigned* base = reinterpret_cast<const unsigned*>(bytes + (from & ~(int64_t)3));
  const int64_t last_dword = ((nbytes + 3) >> 2) - 1 - ((from & ~(int64_t)3) >> 2);
  unsigned* o = reinterpret_cast<unsigned*>(dst + head);
  for (int64_t v = (int64_t)blockIdx.y * kZpThreads + threadIdx.x; v < nd; v += (int64_t)gridDim.y * kZpThreads) {
    unsigned d = base[v];
    if (sh) {                                               // (uniform: a property of the member)
      const unsigned e = base[v + 1 <= last_dword ? v + 1 : last_dword];       // beyond the buffer only bits nothing uses
      d = __builtin_amdgcn_alignbit(e, d, sh);
    }
    o[v] = d;
  }
}

struct ZpLayout {
  int64_t inf_off, inf_len, inf_cap, slots, total;
};

__host__ bool zp_layout(int64_t n, int64_t max_size, ZpLayout* lay) {
  if (n < 1 || n > ((int64_t)1 << 31) - 1 || max_size < 0 || max_size > kZpMaxLen) return false;
  const int64_t slots = zp_crc_slots_bytes(n, max_size);
  if (slots < 0) return false;
  auto up = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
  int64_t at = 0;
  lay->inf_off = at, at += up(n * 8);
  lay->inf_len = at, at += up(n * 8);
  lay->inf_cap = at, at += up(n * 8);
  lay->slots = at, at += slots;
  lay->total = at;
  return true;
}

}  // namespace

extern "C" int64_t pl_crc32_work_bytes(int64_t n_ranges, int64_t max_len) { return zp_crc_slots_bytes(n_ranges, max_len); }

extern "C" int pl_crc32(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_off, const int64_t* d_len, int64_t n_ranges,
                        int64_t max_len, uint32_t* d_crc, int32_t* d_status, unsigned char* d_work, void* stream) {
  PL_REQUIRE(d_bytes && d_off && d_len && d_crc && d_status && d_work, "null pointer");
  PL_REQUIRE(((uintptr_t)d_bytes & 3) == 0, "the byte buffer must start on a 4-byte boundary (ranges inside it may start anywhere)");
  PL_REQUIRE(((uintptr_t)d_work & 3) == 0, "d_work must start on a 4-byte boundary");
  PL_REQUIRE(nbytes >= 0 && nbytes <= ((int64_t)1 << 40), "bad buffer size");
  PL_REQUIRE(zp_crc_slots_bytes(n_ranges, max_len) >= 0, "1 <= n_ranges < 2^31, 0 <= max_len <= 65535 x 16 KiB");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(d_status, 0, (size_t)n_ranges * 4, st) != hipSuccess) {
    pl_set_error("pl_crc32: memset failed");
    return PL_ERR_HIP;
  }
  zp_crc_launch(d_bytes, nbytes, d_off, d_len, n_ranges, max_len, nullptr, d_crc, d_status, d_work, st);
  return pl_check_launch("pl_crc32");
}

extern "C" int64_t pl_zip_work_bytes(int64_t n_members, int64_t max_size) {
  ZpLayout lay;
  return zp_layout(n_members, max_size, &lay) ? lay.total : -1;
}

extern "C" int pl_zip_extract(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_in_off, const int64_t* d_in_len,
                              const int32_t* d_method, const uint32_t* d_crc_expected, int64_t n_members, int64_t max_size,
                              unsigned char* d_out, int64_t out_bytes, const int64_t* d_out_off, const int64_t* d_out_size,
                              int verify, int64_t* d_out_len, int32_t* d_status, unsigned char* d_work, void* stream) {
  PL_REQUIRE(d_bytes && d_in_off && d_in_len && d_method && d_crc_expected && d_out && d_out_off && d_out_size && d_out_len &&
                 d_status && d_work,
             "null pointer");
  PL_REQUIRE(((uintptr_t)d_bytes & 3) == 0, "the byte buffer must start on a 4-byte boundary (members inside it may start anywhere)");
  PL_REQUIRE(((uintptr_t)d_out & 3) == 0, "d_out must start on a 4-byte boundary");
  PL_REQUIRE(((uintptr_t)d_work & 15) == 0, "d_work must start on a 16-byte boundary");
  PL_REQUIRE(verify == 0 || verify == 1, "verify 0 or 1");
  PL_REQUIRE(nbytes >= 0 && nbytes <= ((int64_t)1 << 40) && out_bytes >= 0 && out_bytes <= ((int64_t)1 << 40), "bad buffer size");
  ZpLayout lay;
  PL_REQUIRE(zp_layout(n_members, max_size, &lay), "1 <= n_members < 2^31, 0 <= max_size <= 65535 x 16 KiB");
  hipStream_t st = (hipStream_t)stream;
  int64_t* inf_off = reinterpret_cast<int64_t*>(d_work + lay.inf_off);
  int64_t* inf_len = reinterpret_cast<int64_t*>(d_work + lay.inf_len);
  int64_t* inf_cap = reinterpret_cast<int64_t*>(d_work + lay.inf_cap);
  hipLaunchKernelGGL(zip_check_kernel, dim3((unsigned)pl_cdiv(n_members, kZpThreads)), dim3(kZpThreads), 0, st, d_in_off, d_in_len,
                     d_method, d_out_off, d_out_size, n_members, nbytes, out_bytes, max_size, inf_off, inf_len, inf_cap, d_status);
  hipLaunchKernelGGL(inflate_kernel<false>, dim3((unsigned)n_members), dim3(PL_WAVE), 0, st, d_bytes, nbytes, inf_off, inf_len, 0,
                     d_out, d_out_off, inf_cap, d_out_len, d_status, PnChecked{});
  int64_t pieces = pl_cdiv(max_size, (int64_t)kZpThreads * 4 * 16);
  pieces = pieces < 1 ? 1 : (pieces > 64 ? 64 : pieces);
  hipLaunchKernelGGL(zip_stored_kernel, dim3((unsigned)n_members, (unsigned)pieces), dim3(kZpThreads), 0, st, d_bytes, nbytes, d_in_off,
                     d_in_len, d_method, d_out_off, d_out_size, out_bytes, max_size, d_out, d_out_len);
  if (verify)
    zp_crc_launch(d_out, out_bytes, d_out_off, d_out_size, n_members, max_size, d_crc_expected, nullptr, d_status,
                  d_work + lay.slots, st);
  return pl_check_launch("pl_zip_extract");
}
