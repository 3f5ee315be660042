// Deflate (RFC 1951, with or without the zlib wrapper of RFC 1950) and PNG files (ISO/IEC 15948: grey of 8 or 16 bits, RGB
// of 8 bits, non-interlaced) -> typed frames on the device: the step BEFORE the hot path for scanned film and portal-dose
// exports, next to tiff.hip.  The reference hands its analyzers `np.asarray(PIL.Image.open(f))` (zlib + PIL's PngDecoder);
// the arithmetic here is theirs:
//   * a PNG's pixel data is ONE zlib stream cut into IDAT chunks at arbitrary byte positions;
//   * the inflated stream holds height rows of 1 + row_bytes bytes: a filter-type byte (0 None, 1 Sub, 2 Up, 3 Average,
//     4 Paeth), then the row; filters act per byte at distance bpp = bytes per pixel, modulo 256; the row above the first
//     and the bytes left of a row are zeros; Paeth's ties go to the left, then to the row above;
//   * 16-bit samples are big-endian; RGB -> one band as PIL's convert("I"): (19595 R + 38470 G + 7471 B + 0x8000) >> 16.
// Whole files lie anywhere in one device buffer; a per-segment descriptor (offset, length, frame) names every IDAT payload
// in stream order.  The launches (four, whatever the stack):
//   1 png_check_kernel     ONE block: every descriptor against the buffer, a prefix sum of the sound lengths (where each
//                          payload goes in the compacted area), the start of each frame's stream; an unsound descriptor
//                          or a frame whose segments are not consecutive flags the FRAME (status bit 0): never read,
//                          nothing of it stored
//   2 png_gather_kernel    the payloads side by side: a coalesced dword copy at any source alignment (v_alignbit funnel),
//                          so the bit reader never sees a chunk seam
//   3 inflate_kernel       one wave per stream (below); pl_inflate is this launch alone
//   4 png_unfilter_kernel  one wave per frame: filter reversal as a skewed wavefront over 64 rows, byte order, RGB collapse,
//                          store as out_kind
//
// inflate_kernel.  The bit buffer (64 bits), the input position and the output position are wave-uniform: every value read
// from LDS on the way goes through v_readfirstlane, so the token loop is scalar code with scalar branches.
//   input    staged in LDS 1 KiB at a time as aligned dwords (the stream may start at any byte), read 32 bits at a time
//   tables   built by the whole wave from the code lengths: a tally per length (LDS atomics), the Kraft sum, the canonical
//            first code per length; a symbol's rank among its length = ballots over 64 symbols at a time; every symbol
//            fills its slots of a primary lookup (12 bits literal/length, 8 bits distance, 7 bits code lengths; the entry is
//            symbol << 4 | length) and its place in the list of symbols sorted by (length, symbol), which the canonical walk
//            over the longer lengths uses for codes the primary lookup does not hold
//   tokens   lane p looks up the code that would begin at bit p of the buffer (ONE LDS instruction); the chain of code lengths
//            is then walked over the lanes' entries with v_readlane, so a run of literals costs one round trip to LDS and the
//            lanes at which a literal begins store their symbols together; a length / distance pair is decoded on its own
//   output   the stream's last 32 KiB live in an LDS ring; a literal is one LDS byte store, a match is copied by the whole
//            wave inside the ring (byte k of the match is byte k mod distance of the source, which lies wholly before the
//            match: byte-serial semantics for overlapping matches, distance 1 included), a stored block is copied by the wave
//            from the staged input's memory into the ring.  Whenever 4 KiB are complete they leave for global memory in 16-byte
//            pieces (64 lanes x 4; byte stores when the destination is not on a 16-byte boundary, as for tiff.hip's Deflate
//            strips of odd row_bytes); nothing the wave stored to global memory is ever read back, so there is no release /
//            acquire pair in this kernel.  Output beyond out_cap is never stored.
// status per stream: bit 0 unsound descriptor, bit 1 the input ended first or the stream ended below out_cap, bit 2 corrupt
// Deflate (see include/pylinac_hip.h for the list).
//
// png_unfilter_kernel.  Average and Paeth need the byte to the left and the row above, so a row is a serial chain and so is
// the column.  Lane k of the wave owns row r0 + k of a band of 64 rows and, at step t, reconstructs CHUNK t - k of its row
// (16 bytes of a grey row, 48 = 16 pixels of an RGB row): "up" is lane k - 1's chunk of the step before (one DPP move per
// dword), "up-left" the tail of the chunk it received a step earlier, "left" the tail of its own previous chunk.  Lane 0 reads
// the band's predecessor row, which lane 63 of the band before left in a row buffer (zeros for the first band), between a
// workgroup-scope release / acquire pair as in tiff_lzw_kernel.  A band takes chunks + 63 steps; every lane loads its next
// chunk (aligned dwords, funnelled) one step ahead, and stores a chunk's samples in 16-byte pieces when the output rows are
// 16-byte aligned (element stores otherwise, and for a row's last partial chunk).
//
// zip_kernels.h (included near the end: inflate_kernel is file-local) holds the other users of the Deflate half: CRC-32 of byte
// ranges (pl_crc32) and the members of a ZIP archive (pl_zip_extract).
//
// The checked mode (pl_inflate_checked, pl_png_decode_checked; the entry points follow zip_kernels.h, whose CRC launches the
// second one uses).  inflate_kernel<true> decodes on to the end of the stream and leaves, per stream, the Adler-32 field it
// found there and whether it is to be judged (PnChecked); the Adler pair of adler32.hip (pl_adler32_launch) then runs over what
// was stored and compares.  pl_png_decode_checked adds pl_crc32's pair over every chunk of the files (type + data, against the
// CRC the chunk stores) and png_chunk_verdict_kernel, which flags the chunk's frame: nine launches, whatever the stack.
// inflate_kernel<false> is the kernel pl_inflate, pl_png_decode and pl_zip_extract launch, as before.
#include "pl_common.h"

// adler32.hip is a translation unit of its own in the library; the CPU emulator of the tests builds a fixed list of files
// that holds this one, so there it is compiled as a part of this file
#ifdef PL_HIPEMU
#define PL_ADLER32_IN_PNG
#include "adler32.hip"
#endif

namespace {

constexpr int kPnThreads = 256;
constexpr int kPnRing = 32768;                              // the Deflate window
constexpr int kPnFlush = 4096;                              // bytes that leave the ring together
constexpr int kPnWindow = 1024;                             // input bytes staged in LDS at a time
constexpr int kPnLitBits = 12, kPnDistBits = 8, kPnClBits = 7;

__device__ __forceinline__ void pn_output_sync() {          // global bytes written by a lane of the wave and read by another
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ unsigned pn_rev16(unsigned x) {
  x = ((x & 0x5555u) << 1) | ((x >> 1) & 0x5555u);
  x = ((x & 0x3333u) << 2) | ((x >> 2) & 0x3333u);
  x = ((x & 0x0f0fu) << 4) | ((x >> 4) & 0x0f0fu);
  return ((x & 0xffu) << 8) | (x >> 8);
}

// ---- launches 1 and 2: check, scan, gather ---------------------------------------------------------------------------------
struct PnSeg {
  bool ok;
  int frame;
  int64_t off, len;
};

__device__ __forceinline__ PnSeg pn_seg(const int64_t* __restrict__ seg_off, const int64_t* __restrict__ seg_len,
                                        const int32_t* __restrict__ seg_frame, int64_t s, int64_t nbytes, int64_t n_frames) {
  PnSeg t;
  t.frame = seg_frame[s], t.off = seg_off[s], t.len = seg_len[s];
  // (differences of lengths, never sums of an offset and a length: nothing here can overflow)
  t.ok = t.frame >= 0 && t.frame < n_frames && t.off >= 0 && t.len >= 0 && t.off <= nbytes && t.len <= nbytes - t.off;
  return t;
}

__global__ void __launch_bounds__(kPnThreads)
png_check_kernel(const int64_t* __restrict__ seg_off, const int64_t* __restrict__ seg_len, const int32_t* __restrict__ seg_frame,
                 int64_t n_segments, int64_t nbytes, int64_t n_frames, int64_t frame_stride,
                 int64_t frame_bytes, int64_t* __restrict__ seg_pos, int32_t* __restrict__ head, int64_t* __restrict__ stream_off,
                 int64_t* __restrict__ stream_len, int64_t* __restrict__ out_off, int64_t* __restrict__ out_cap,
                 int32_t* __restrict__ status) {
  __shared__ int64_t s_part[kPnThreads];
  __shared__ int64_t s_carry;
  const int tid = threadIdx.x;
  for (int64_t f = tid; f < n_frames; f += kPnThreads) {
    head[f] = 0;
    stream_off[f] = 0, stream_len[f] = 0;                   // a frame without segments: an empty stream
    out_off[f] = f * frame_stride, out_cap[f] = frame_bytes;
  }
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < n_segments; base += kPnThreads) {
    const int64_t s = base + tid;
    PnSeg t;
    t.ok = false, t.frame = -1, t.off = 0, t.len = 0;
    if (s < n_segments) t = pn_seg(seg_off, seg_len, seg_frame, s, nbytes, n_frames);
    const int64_t mine = t.ok ? t.len : 0;
    s_part[tid] = mine;
    __syncthreads();
    for (int o = 1; o < kPnThreads; o <<= 1) {              // inclusive scan of the block's lengths
      const int64_t u = tid >= o ? s_part[tid - o] : 0;
      __syncthreads();
      s_part[tid] += u;
      __syncthreads();
    }
    const int64_t carry = s_carry;
    const int64_t pos = carry + s_part[tid] - mine;
    __syncthreads();
    if (tid == kPnThreads - 1) {                            // (no overflow, whatever the lengths)
      const int64_t sum = carry + s_part[tid];
      s_carry = sum < ((int64_t)1 << 50) ? sum : (int64_t)1 << 50;
    }
    if (s < n_segments) {
      seg_pos[s] = t.ok ? pos : -1;
      const bool in_stack = t.frame >= 0 && t.frame < n_frames;
      if (in_stack && !t.ok) atomicOr(status + t.frame, 1);
      if (in_stack && (s == 0 || seg_frame[s - 1] != t.frame)) {               // the first segment of a run
        if (atomicCAS(head + t.frame, 0, 1) != 0) atomicOr(status + t.frame, 1);   // a second run: IDATs are consecutive
        else stream_off[t.frame] = pos;
      }
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kPnThreads)
png_gather_kernel(const unsigned char* __restrict__ bytes, int64_t nbytes, const int64_t* __restrict__ seg_off,
                  const int64_t* __restrict__ seg_len, const int32_t* __restrict__ seg_frame, int64_t n_segments, int64_t n_frames,
                  const int64_t* __restrict__ seg_pos, const int64_t* __restrict__ stream_off, int64_t* __restrict__ stream_len,
                  unsigned char* __restrict__ compact, const int32_t* __restrict__ status) {
  const int64_t s = blockIdx.x;                             // (blockIdx.y: the segment's pieces)
  const PnSeg t = pn_seg(seg_off, seg_len, seg_frame, s, nbytes, n_frames);
  const int64_t pos = seg_pos[s];
  if (!t.ok || pos < 0 || (status[t.frame] & 1)) return;
  if (blockIdx.y == 0 && threadIdx.x == 0 && (s + 1 == n_segments || seg_frame[s + 1] != t.frame))
    stream_len[t.frame] = pos + t.len - stream_off[t.frame];                   // the last segment of the frame's run
  const int64_t n = t.len;
  unsigned char* dst = compact + pos;
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
  for (int64_t v = (int64_t)blockIdx.y * kPnThreads + threadIdx.x; v < nd; v += (int64_t)gridDim.y * kPnThreads) {
    unsigned d = base[v];
    if (sh) {                                               // (uniform: a property of the segment)
      const unsigned e = base[v + 1 <= last_dword ? v + 1 : last_dword];       // beyond the buffer only bits nothing uses
      d = __builtin_amdgcn_alignbit(e, d, sh);
    }
    out[v] = d;
  }
}

// ---- launch 3: inflate -----------------------------------------------------------------------------------------------------
struct PnCodes {                                            // one canonical code set in LDS
  int cnt[16], first[16], offs[16], next[16];
};

// every lane calls this (wave-uniform control flow).  lens[0 .. n): code lengths 0 .. 15.  -> 0 complete, 1 over-subscribed,
// 2 incomplete; *coded = symbols with a code, *longest = the longest code
__device__ int pn_build(const unsigned char* lens, int n, unsigned short* tab, int tbits, unsigned short* sorted, PnCodes* cs,
                        int lane, int* coded, int* longest) {
  if (lane < 16) cs->cnt[lane] = 0;
  for (int i = lane; i < (1 << tbits); i += PL_WAVE) tab[i] = 0;
  pl_wave_sync();
  for (int i = lane; i < n; i += PL_WAVE) {
    const int l = lens[i];
    if (l) atomicAdd(&cs->cnt[l], 1);
  }
  pl_wave_sync();
  int code = 0, off = 0, kraft = 0, prev = 0, longl = 0;
  for (int l = 1; l <= 15; ++l) {
    const int c = __builtin_amdgcn_readfirstlane(cs->cnt[l]);
    code = (code + prev) << 1;
    if (lane == 0) cs->first[l] = code, cs->offs[l] = off, cs->next[l] = 0;
    off += c, kraft += c << (15 - l), prev = c;
    if (c) longl = l;
  }
  *coded = off, *longest = longl;
  pl_wave_sync();
  if (kraft > 32768) return 1;
  for (int base = 0; base < n; base += PL_WAVE) {
    const int i = base + lane;
    const int l = i < n ? lens[i] : 0;
    int rank = 0;
    for (int b = 1; b <= 15; ++b) {                         // the rank of a symbol among those of its length, in symbol order
      const unsigned long long m = __ballot(l == b);
      if (m == 0) continue;
      const int r0 = __builtin_amdgcn_readfirstlane(cs->next[b]);
      if (l == b) rank = r0 + __popcll(m & ((1ull << lane) - 1ull));
      pl_wave_sync();
      if (lane == 0) cs->next[b] = r0 + __popcll(m);
      pl_wave_sync();
    }
    if (l) {
      const int c = cs->first[l] + rank;
      sorted[cs->offs[l] + rank] = (unsigned short)i;
      if (l <= tbits) {
        const unsigned short e = (unsigned short)((i << 4) | l);
        for (int j = (int)(pn_rev16((unsigned)c) >> (16 - l)); j < (1 << tbits); j += 1 << l) tab[j] = e;
      }
    }
  }
  pl_wave_sync();
  return kraft < 32768 ? 2 : 0;
}

// the symbol whose code the low bits of `bits` begin with (Huffman codes arrive most significant bit first); -> the symbol
// and *len its code length, *len = 0 when no code matches (an incomplete set)
__device__ __forceinline__ int pn_symbol(unsigned bits, const unsigned short* tab, int tbits, const unsigned short* sorted,
                                         const PnCodes* cs, int* len) {
  const unsigned e = __builtin_amdgcn_readfirstlane((unsigned)tab[bits & ((1u << tbits) - 1u)]);
  if (e & 15u) {
    *len = (int)(e & 15u);
    return (int)(e >> 4);
  }
  const unsigned rev = pn_rev16(bits & 0xffffu) >> 1;       // the first 15 bits as a code, first bit on top
  for (int l = tbits + 1; l <= 15; ++l) {
    const int d = (int)(rev >> (15 - l)) - __builtin_amdgcn_readfirstlane(cs->first[l]);
    if (d >= 0 && d < __builtin_amdgcn_readfirstlane(cs->cnt[l])) {
      *len = l;
      return (int)__builtin_amdgcn_readfirstlane((unsigned)sorted[__builtin_amdgcn_readfirstlane(cs->offs[l]) + d]);
    }
  }
  *len = 0;
  return 0;
}

struct PnIn {                                               // the bit reader: all wave-uniform
  unsigned long long buf;
  int nbits;
  int64_t pos, win0;                                        // the next input byte to enter `buf`; the window's first byte
};

// A match with dist + n > kPnRing (every lane calls this; zlib's encoder never writes one: it stops at distance 32 506).  The
// ring holds kPnRing bytes of output, so the slot byte k of the match is read from is the slot byte k + (kPnRing - dist) of the
// SAME match is stored to (dist = 32768: the lane's own slot).  64 bytes at a time: every lane loads its byte, the wave meets,
// then the lanes store -- a later byte's store never precedes an earlier byte's load, within a step by the barrier and across
// steps by their order, without any reliance on the lanes running in lock-step.  Kept out of line, behind a branch marked
// unlikely: inlined, or unmarked, it cost the whole of inflate_kernel 0.3 - 5 % through the register allocation around it; as it
// stands the common path pays one scalar compare a match (profiles/deflate_conformance_time.md).
__device__ __attribute__((noinline)) void pn_copy_alias(unsigned char* ring, unsigned op, unsigned dist, unsigned n, int lane) {
  for (unsigned k0 = 0; k0 < n; k0 += PL_WAVE) {
    const unsigned k = k0 + (unsigned)lane;
    const unsigned char held = k < n ? ring[(op + k - dist) & (kPnRing - 1)] : (unsigned char)0;
    pl_wave_sync();
    if (k < n) ring[(op + k) & (kPnRing - 1)] = held;
  }
}

// CHECKED (pl_inflate_checked, pl_png_decode_checked, tiff.hip's Deflate strips): what the wave reports besides, per stream
// (PnChecked, pl_common.h).  In that mode it does not stop at out_cap bytes but decodes on to the end-of-block code of the
// BFINAL block -- storing nothing beyond out_cap, and giving up at the first byte beyond it, which settles the verdict -- drops
// the bits up to the next byte boundary and reads the four bytes there: the stream's Adler-32 field.
template <bool CHECKED>
__global__ void __launch_bounds__(PL_WAVE)
inflate_kernel(const unsigned char* __restrict__ bytes, int64_t nbytes, const int64_t* __restrict__ in_off,
               const int64_t* __restrict__ in_len, int wrapper, unsigned char* __restrict__ out, const int64_t* __restrict__ out_off,
               const int64_t* __restrict__ out_cap, int64_t* __restrict__ out_len, int32_t* __restrict__ status, PnChecked chk) {
  __shared__ uint4 s_ring4[kPnRing / 16];
  __shared__ unsigned s_in[kPnWindow / 4 + 4];
  __shared__ unsigned short s_lit[1 << kPnLitBits], s_dist[1 << kPnDistBits], s_cl[1 << kPnClBits];
  __shared__ unsigned short s_litsym[288], s_distsym[32], s_clsym[19];
  __shared__ unsigned char s_lens[320 + 8];
  __shared__ PnCodes s_lc, s_dc, s_cc;
  unsigned char* ring = reinterpret_cast<unsigned char*>(s_ring4);
  const int64_t s = blockIdx.x;
  const int lane = threadIdx.x;
  if (status[s] & 1) return;                                // (pl_png_decode: a frame the check flagged)
  const int64_t off = in_off[s], len = in_len[s], cap64 = out_cap[s], dst0 = out_off[s];
  if (!(off >= 0 && len >= 0 && off <= nbytes && len <= nbytes - off && cap64 >= 0 && cap64 < ((int64_t)1 << 31) && dst0 >= 0) ||
      (CHECKED && cap64 > chk.max_out)) {
    if (lane == 0) {
      atomicOr(status + s, 1);
      out_len[s] = 0;
      if (CHECKED && chk.in_used) chk.in_used[s] = 0;
    }
    return;
  }
  const unsigned cap = (unsigned)cap64;
  const unsigned lim = CHECKED ? cap + 1u : cap;            // where the token loops stop: one byte beyond out_cap tells enough
  unsigned char* dst = out + dst0;
  const bool aligned = ((uintptr_t)dst & 15u) == 0;
  const int64_t last_dword = ((nbytes < off + len ? nbytes : off + len) + 3) / 4 - 1;      // of the buffer, and of the stream
  const unsigned* words = reinterpret_cast<const unsigned*>(bytes);
  PnIn in;
  in.buf = 0, in.nbits = 0, in.pos = 0, in.win0 = -(int64_t)(2 * kPnWindow);
  unsigned op = 0, flushed = 0;
  int flag = 0;                                             // 2 short, 4 corrupt
  int tables = 0;                                           // what s_lit / s_dist hold: 1 the fixed codes, 2 a dynamic block's
  bool careful = false;                                     // near the end of the input: no literal runs

  // at least 33 bits in the buffer (beyond the stream's end: whatever follows it, or zeros; `over` tells)
  auto refill = [&]() {
    if (in.nbits > 32) return;
    if (in.pos + 8 > in.win0 + kPnWindow || in.pos < in.win0) {
      pl_wave_sync();
      in.win0 = in.pos - ((off + in.pos) & 3);              // (the window starts on a dword of the buffer)
      const int64_t w0 = (off + in.win0) >> 2;
      for (int i = lane; i < kPnWindow / 4 + 4; i += PL_WAVE) s_in[i] = w0 + i <= last_dword ? words[w0 + i] : 0u;
      pl_wave_sync();
    }
    const int b = (int)(in.pos - in.win0);
    const unsigned lo = s_in[b >> 2], hi = s_in[(b >> 2) + 1];
    const unsigned v = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_alignbit(hi, lo, (unsigned)(b & 3) * 8u));
    in.buf |= (unsigned long long)v << in.nbits;
    in.nbits += 32, in.pos += 4;
  };
  auto take = [&](int n) -> unsigned {                      // n <= 32 bits, after a refill
    const unsigned v = (unsigned)(in.buf & ((1ull << n) - 1ull));
    in.buf >>= n, in.nbits -= n;
    return v;
  };
  auto over = [&]() -> bool { return in.pos * 8 - in.nbits > len * 8; };       // more bits consumed than the stream has
  auto flush = [&]() {                                      // kPnFlush bytes of the ring -> global memory
    pl_wave_sync();
    const unsigned r0 = flushed & (kPnRing - 1);
#pragma unroll
    for (int j = 0; j < kPnFlush / 16 / PL_WAVE; ++j) {
      const unsigned piece = (unsigned)(j * PL_WAVE + lane) * 16u;
      const unsigned g = flushed + piece;
      if (aligned && g + 16u <= cap) {
        *reinterpret_cast<uint4*>(dst + g) = s_ring4[(r0 + piece) >> 4];
      } else {
        for (unsigned b = 0; b < 16u && g + b < cap; ++b) dst[g + b] = ring[r0 + piece + b];
      }
    }
    flushed += kPnFlush;
  };

  if (len == 0 || nbytes == 0) flag = 2;
  if (!flag && wrapper) {                                   // RFC 1950: CMF, FLG
    refill();
    const unsigned cmf = take(8), flg = take(8);
    if (over()) flag = 2;
    else if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) flag = 4;
  }
  bool last = false;
  while (!flag && !last && op < lim) {
    refill();
    last = take(1) != 0;
    const unsigned type = take(2);
    if (over()) {
      flag = 2;
      break;
    }
    if (type == 3) {
      flag = 4;
      break;
    }
    if (type == 0) {                                        // ---- stored
      take(in.nbits & 7);
      refill();
      const unsigned n16 = take(16), c16 = take(16);
      if (over()) {
        flag = 2;
        break;
      }
      if ((n16 ^ c16) != 0xffffu) {
        flag = 4;
        break;
      }
      int64_t from = in.pos - (in.nbits >> 3);              // (whole bytes are left in the buffer)
      unsigned left = n16;
      if ((int64_t)left > len - from) left = (unsigned)(len - from), flag = 2;   // the input ends inside the block
      in.buf = 0, in.nbits = 0, in.pos = from + left;
      const unsigned char* src = bytes + off;
      while (left && op < lim) {
        unsigned n = left < 1024u ? left : 1024u;
        if (n > lim - op) n = lim - op;
        for (unsigned k = lane; k < n; k += PL_WAVE) ring[(op + k) & (kPnRing - 1)] = src[from + k];
        op += n, from += n, left -= n;
        while (op - flushed >= (unsigned)kPnFlush) flush();
      }
      continue;
    }
    // ---- the code sets
    if (type == 1) {
      if (tables != 1) {
        pl_wave_sync();
        for (int i = lane; i < 320; i += PL_WAVE) s_lens[i] = (unsigned char)(i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : (i < 288 ? 8 : 5))));
        pl_wave_sync();
        int coded, longest;
        pn_build(s_lens, 288, s_lit, kPnLitBits, s_litsym, &s_lc, lane, &coded, &longest);
        pn_build(s_lens + 288, 32, s_dist, kPnDistBits, s_distsym, &s_dc, lane, &coded, &longest);
        tables = 1;
      }
    } else {
      refill();
      const int hlit = (int)take(5) + 257, hdist = (int)take(5) + 1, hclen = (int)take(4) + 4;
      if (hlit > 286 || hdist > 30) {
        flag = over() ? 2 : 4;
        break;
      }
      pl_wave_sync();
      if (lane < 19) s_lens[lane] = 0;
      pl_wave_sync();
      for (int i = 0; i < hclen; ++i) {
        refill();
        const unsigned v = take(3);
        const int at = i < 3 ? 16 + i : (i == 3 ? 0 : ((i & 1) ? 7 - (i - 5) / 2 : 8 + (i - 4) / 2));   // 16 17 18 0 8 7 9 6 10 5 ...
        if (lane == 0) s_lens[at] = (unsigned char)v;
      }
      if (over()) {
        flag = 2;
        break;
      }
      pl_wave_sync();
      int coded, longest;
      if (pn_build(s_lens, 19, s_cl, kPnClBits, s_clsym, &s_cc, lane, &coded, &longest) != 0) {
        flag = 4;
        break;
      }
      tables = 0;
      const int total = hlit + hdist;
      int i = 0, before = -1;
      while (i < total) {
        refill();
        int l;
        const int sym = pn_symbol((unsigned)in.buf, s_cl, kPnClBits, s_clsym, &s_cc, &l);
        if (l == 0) {
          flag = over() ? 2 : 4;
          break;
        }
        take(l);
        int rep = 1, v = sym;
        if (sym == 16) {
          if (before < 0) {
            flag = over() ? 2 : 4;
            break;
          }
          v = before, rep = 3 + (int)take(2);
        } else if (sym == 17) {
          v = 0, rep = 3 + (int)take(3);
        } else if (sym == 18) {
          v = 0, rep = 11 + (int)take(7);
        }
        if (over()) {
          flag = 2;
          break;
        }
        if (rep > total - i) {
          flag = 4;
          break;
        }
        for (int k = lane; k < rep; k += PL_WAVE) s_lens[i + k] = (unsigned char)v;
        i += rep, before = v;
      }
      if (flag) break;
      pl_wave_sync();
      if (__builtin_amdgcn_readfirstlane((int)s_lens[256]) == 0) {             // no end-of-block code
        flag = 4;
        break;
      }
      // the distance lengths to a place of their own: the literal/length set is built from s_lens[0 .. hlit)
      unsigned char keep = 0;
      if (lane < hdist) keep = s_lens[hlit + lane];
      pl_wave_sync();
      if (lane < 32) s_lens[288 + lane] = lane < hdist ? keep : (unsigned char)0;
      pl_wave_sync();
      const int lk = pn_build(s_lens, hlit, s_lit, kPnLitBits, s_litsym, &s_lc, lane, &coded, &longest);
      // the one incomplete literal/length set zlib's inftrees.c allows: ONE code of one bit (the end-of-block code, by the
      // check above: a block without output)
      if (lk == 1 || (lk == 2 && !(coded == 1 && longest == 1))) {
        flag = 4;
        break;
      }
      const int dk = pn_build(s_lens + 288, 32, s_dist, kPnDistBits, s_distsym, &s_dc, lane, &coded, &longest);
      // incomplete distance sets RFC 1951 allows: no distance code at all (literals only), or ONE code of one bit
      if (dk == 1 || (dk == 2 && !(coded == 0 || (coded == 1 && longest == 1)))) {
        flag = 4;
        break;
      }
      tables = 2;
    }
    // ---- the tokens of the block
    for (;;) {
      while (op - flushed >= (unsigned)kPnFlush) flush();
      refill();
      if (!careful) {
        // a run of literals from ONE round trip to LDS: lane p looks up the code that would begin at bit p of the buffer, the
        // chain of code lengths is walked over the lanes' entries with v_readlane, and the lanes at which a literal begins
        // store their symbols together.  A code of the primary lookup lies wholly inside the kPnLitBits bits it was found by.
        const unsigned el = s_lit[(unsigned)(in.buf >> lane) & ((1u << kPnLitBits) - 1u)];
        const unsigned room = lim - op;
        unsigned long long starts = 0;
        int at = 0;
        unsigned n = 0;
        while (at + kPnLitBits <= in.nbits && n < room) {
          const unsigned e = (unsigned)__builtin_amdgcn_readlane((int)el, at);
          if ((e & 15u) == 0u || (e >> 4) >= 256u) break;
          starts |= 1ull << at;
          at += (int)(e & 15u), ++n;
        }
        if (n) {
          if (in.pos * 8 - in.nbits + at > len * 8) {       // bits beyond the stream's end: one token at a time from here on
            careful = true;
          } else {
            if ((starts >> lane) & 1ull)
              ring[(op + (unsigned)__popcll(starts & ((1ull << lane) - 1ull))) & (kPnRing - 1)] = (unsigned char)(el >> 4);
            op += n;
            in.buf = at < 64 ? in.buf >> at : 0ull, in.nbits -= at;
            if (op >= lim) break;
            continue;
          }
        }
      }
      int l;
      const int sym = pn_symbol((unsigned)in.buf, s_lit, kPnLitBits, s_litsym, &s_lc, &l);
      if (l == 0) {
        flag = over() ? 2 : 4;
        break;
      }
      take(l);
      if (sym < 256) {
        if (over()) {
          flag = 2;
          break;
        }
        if (lane == 0) ring[op & (kPnRing - 1)] = (unsigned char)sym;
        ++op;
        if (op >= lim) break;
        continue;
      }
      if (sym == 256) {
        if (over()) flag = 2;
        break;
      }
      if (sym >= 286) {
        flag = over() ? 2 : 4;
        break;
      }
      unsigned n;
      if (sym < 265) n = (unsigned)(sym - 254);
      else if (sym == 285) n = 258u;
      else {
        const int e = (sym - 261) >> 2;
        n = 3u + ((4u + (unsigned)((sym - 265) & 3)) << e) + take(e);
      }
      refill();
      const int dsym = pn_symbol((unsigned)in.buf, s_dist, kPnDistBits, s_distsym, &s_dc, &l);
      if (l == 0 || dsym >= 30) {
        flag = over() ? 2 : 4;
        break;
      }
      take(l);
      unsigned dist;
      if (dsym < 4) dist = (unsigned)dsym + 1u;
      else {
        const int e = (dsym >> 1) - 1;
        dist = 1u + ((2u + (unsigned)(dsym & 1)) << e) + take(e);
      }
      if (over()) {
        flag = 2;
        break;
      }
      if (dist > op) {                                      // before the start of the output
        flag = 4;
        break;
      }
      if (n > lim - op) n = lim - op;
      pl_wave_sync();
      // byte k of the match = byte k mod dist of the `dist` bytes before it.  Those bytes lie wholly before the match in the
      // OUTPUT; in the RING they do only while dist + n <= kPnRing: beyond that, source and target share slots and the copy
      // is pn_copy_alias's.  In the three branches below every lane reads slots that this token does not write
      if (__builtin_expect(dist + n > (unsigned)kPnRing, 0)) {
        pn_copy_alias(ring, op, dist, n, lane);
      } else if (dist >= n) {
        for (unsigned k = lane; k < n; k += PL_WAVE) ring[(op + k) & (kPnRing - 1)] = ring[(op + k - dist) & (kPnRing - 1)];
      } else if (dist == 1) {
        const unsigned char v = ring[(op - 1u) & (kPnRing - 1)];
        for (unsigned k = lane; k < n; k += PL_WAVE) ring[(op + k) & (kPnRing - 1)] = v;
      } else {
        for (unsigned k = lane; k < n; k += PL_WAVE) ring[(op + k) & (kPnRing - 1)] = ring[(op - dist + k % dist) & (kPnRing - 1)];
      }
      pl_wave_sync();
      op += n;
      if (op >= lim) break;
    }
  }
  // what is left in the ring
  pl_wave_sync();
  while (op - flushed >= (unsigned)kPnFlush) flush();
  const unsigned stored = op < cap ? op : cap;
  for (unsigned g = flushed + lane; g < stored; g += PL_WAVE) dst[g] = ring[g & (kPnRing - 1)];
  if constexpr (!CHECKED) {
    if (lane == 0) {
      if (!flag && op < cap) flag = 2;                      // the stream ended below its expected size
      if (op >= cap && flag == 2) flag = 0;                 // complete before the input ran out
      if (flag) atomicOr(status + s, flag);
      out_len[s] = op;
    }
  } else {
    // the loop ended at the BFINAL block's end-of-block code (`last`, no flag, op <= cap), at a byte beyond out_cap, or with
    // a flag.  Here the input running out is NOT forgiven by a full output: zlib reports an incomplete stream
    const bool beyond = op > cap;
    int64_t used = in.pos - (in.nbits >> 3);                // whole bytes consumed: the bits up to the byte boundary go
    if (used > len) used = len;
    unsigned field = 0;
    int verdict = 0;
    if (!flag && !beyond) {
      if (op < cap) flag = 2;                               // the stream ended below its expected size
      if (len - used < 4) {
        flag |= 2, used = len;                              // the final block ended, the field is cut: zlib's Error -5
      } else {
        const unsigned char* t = bytes + off + used;
        field = ((unsigned)t[0] << 24) | ((unsigned)t[1] << 16) | ((unsigned)t[2] << 8) | (unsigned)t[3];
        used += 4;
        verdict = flag == 0;
      }
    }
    if (lane == 0) {
      if (flag) atomicOr(status + s, flag);
      if (beyond && !flag && chk.overflow) atomicOr(status + s, chk.overflow);
      out_len[s] = stored;
      chk.trailer[s] = field, chk.judge[s] = verdict;
      if (chk.in_used) chk.in_used[s] = used;
    }
  }
}

// ---- launch 4: filter reversal, byte order, RGB collapse, store ------------------------------------------------------------
// OUT: 0 the container dtype (uint8 / uint16; int32 for RGB), 1 uint16, 2 float64 -- `array.astype(dtype)` of the container
template <int BYTES, int SPP, int OUT>
struct PnGeom {
  static constexpr int kBpp = BYTES * SPP;
  static constexpr int kChunk = SPP == 3 ? 48 : 16;         // bytes a lane reconstructs per step
  static constexpr int kWords = kChunk / 4;
  static constexpr int kPixels = kChunk / kBpp;             // 16 (grey 8, RGB) or 8 (grey 16)
  static constexpr int kElem = OUT == 0 ? (SPP == 3 ? 4 : BYTES) : (OUT == 1 ? 2 : 8);
  static constexpr int kOutWords = kPixels * kElem / 4;
};

__device__ __forceinline__ unsigned pn_byte(const unsigned* w, int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xffu; }

template <int BYTES, int SPP, int OUT>
__global__ void __launch_bounds__(PL_WAVE)
png_unfilter_kernel(const unsigned char* __restrict__ inflated, int64_t frame_stride, unsigned char* prev_rows, int64_t prev_stride,
                    int width, int height, const int64_t* __restrict__ inflated_len, void* __restrict__ out, int32_t* __restrict__ status) {
  using G = PnGeom<BYTES, SPP, OUT>;
  const int64_t f = blockIdx.x;
  const int lane = threadIdx.x;
  if (status[f] & 1) return;
  const int row_bytes = width * G::kBpp;                    // (a frame is below 2 GiB)
  const int chunks = (row_bytes + G::kChunk - 1) / G::kChunk;
  const unsigned char* frame = inflated + f * frame_stride;
  unsigned char* prev = prev_rows + f * prev_stride;
  const bool wide = (((int64_t)width * G::kElem) & 15) == 0 && ((uintptr_t)out & 15u) == 0;   // output rows on 16-byte boundaries
  const int64_t produced = inflated_len[f];
  bool bad_filter = false;
  for (int r0 = 0; r0 < height; r0 += PL_WAVE) {
    const int r = r0 + lane;
    const bool active = r < height;
    const bool more = r0 + PL_WAVE < height;                // another band follows: lane 63 leaves its row behind
    const unsigned char* rowp = frame + (int64_t)(active ? r : 0) * (1 + row_bytes);
    int ft = active ? rowp[0] : 0;
    if (ft > 4) bad_filter = bad_filter || (int64_t)r * (1 + row_bytes) < produced, ft = 0;   // (a byte the stream never produced is not judged)
    // the row's bytes start at rowp + 1: aligned dwords, funnelled
    const unsigned* rw = reinterpret_cast<const unsigned*>((uintptr_t)(rowp + 1) & ~(uintptr_t)3);
    const unsigned sh = (unsigned)((uintptr_t)(rowp + 1) & 3u) * 8u;
    unsigned nxt[G::kWords], rec[G::kWords], up[G::kWords], upn[G::kWords];
    unsigned left_tail = 0, up_tail = 0;
    auto load_chunk = [&](int c) {                          // chunk c of the lane's row -> nxt (the dwords lie inside the work area)
      unsigned d[G::kWords + 1];
#pragma unroll
      for (int i = 0; i <= G::kWords; ++i) d[i] = rw[c * G::kWords + i];
#pragma unroll
      for (int i = 0; i < G::kWords; ++i) nxt[i] = sh ? __builtin_amdgcn_alignbit(d[i + 1], d[i], sh) : d[i];
    };
    auto load_prev = [&](int c) {                           // lane 0: chunk c of the row above the band -> upn
#pragma unroll
      for (int i = 0; i < G::kWords / 4; ++i) {
        const uint4 q = r0 ? reinterpret_cast<const uint4*>(prev)[c * (G::kWords / 4) + i] : uint4{0u, 0u, 0u, 0u};
        upn[4 * i] = q.x, upn[4 * i + 1] = q.y, upn[4 * i + 2] = q.z, upn[4 * i + 3] = q.w;
      }
    };
#pragma unroll
    for (int i = 0; i < G::kWords; ++i) nxt[i] = rec[i] = up[i] = upn[i] = 0;
    if (active && chunks > 0) load_chunk(0);                // (lane k's first chunk is due at step k: loaded early, once)
    if (lane == 0) load_prev(0);
    for (int t = 0; t < chunks + PL_WAVE - 1; ++t) {
      const int c = t - lane;
      unsigned got[G::kWords];
#pragma unroll
      for (int i = 0; i < G::kWords; ++i) got[i] = (unsigned)pl_wave_from_prev((int)rec[i]);   // lane k - 1's chunk of the step before
      if (!(active && c >= 0 && c < chunks)) continue;
      unsigned cur[G::kWords];
#pragma unroll
      for (int i = 0; i < G::kWords; ++i) cur[i] = nxt[i];
      up_tail = c ? up[G::kWords - 1] : 0u;
#pragma unroll
      for (int i = 0; i < G::kWords; ++i) up[i] = lane == 0 ? upn[i] : got[i];
      left_tail = c ? rec[G::kWords - 1] : 0u;
      if (c + 1 < chunks) {                                 // one step ahead
        load_chunk(c + 1);
        if (lane == 0) load_prev(c + 1);
      }
#pragma unroll
      for (int i = 0; i < G::kWords; ++i) rec[i] = 0;
#pragma unroll
      for (int j = 0; j < G::kChunk; ++j) {
        const int raw = (int)pn_byte(cur, j);
        const int b = (int)pn_byte(up, j);
        int a, cc;
        if (j >= G::kBpp) {
          a = (int)pn_byte(rec, j - G::kBpp), cc = (int)pn_byte(up, j - G::kBpp);
        } else {
          a = (int)((left_tail >> (8 * (4 - G::kBpp + j))) & 0xffu), cc = (int)((up_tail >> (8 * (4 - G::kBpp + j))) & 0xffu);
        }
        const int p = a + b - cc;
        const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - cc);
        const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : cc);
        const int pred = ft == 1 ? a : (ft == 2 ? b : (ft == 3 ? (a + b) >> 1 : (ft == 4 ? paeth : 0)));
        rec[j >> 2] |= (unsigned)((raw + pred) & 0xff) << (8 * (j & 3));
      }
      if (more && lane == PL_WAVE - 1) {
#pragma unroll
        for (int i = 0; i < G::kWords / 4; ++i)
          reinterpret_cast<uint4*>(prev)[c * (G::kWords / 4) + i] = uint4{rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3]};
      }
      // the chunk's samples
      unsigned v[G::kPixels];
#pragma unroll
      for (int q = 0; q < G::kPixels; ++q) {
        if constexpr (SPP == 3) {
          v[q] = (19595u * pn_byte(rec, 3 * q) + 38470u * pn_byte(rec, 3 * q + 1) + 7471u * pn_byte(rec, 3 * q + 2) + 0x8000u) >> 16;
        } else if constexpr (BYTES == 2) {
          v[q] = (pn_byte(rec, 2 * q) << 8) | pn_byte(rec, 2 * q + 1);
        } else {
          v[q] = pn_byte(rec, q);
        }
      }
      const int x0 = c * G::kPixels;
      const int64_t o0 = (f * height + r) * (int64_t)width + x0;               // in elements
      if (wide && x0 + G::kPixels <= width) {
        unsigned w[G::kOutWords];
#pragma unroll
        for (int i = 0; i < G::kOutWords; ++i) w[i] = 0;
#pragma unroll
        for (int q = 0; q < G::kPixels; ++q) {
          if constexpr (G::kElem == 1) w[q >> 2] |= v[q] << (8 * (q & 3));
          else if constexpr (G::kElem == 2) w[q >> 1] |= v[q] << (16 * (q & 1));
          else if constexpr (G::kElem == 4) w[q] = v[q];
          else {
            const long long bits = __double_as_longlong((double)v[q]);
            w[2 * q] = (unsigned)bits, w[2 * q + 1] = (unsigned)(bits >> 32);
          }
        }
        uint4* o = reinterpret_cast<uint4*>(static_cast<unsigned char*>(out) + o0 * G::kElem);
#pragma unroll
        for (int i = 0; i < G::kOutWords / 4; ++i) o[i] = uint4{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
      } else {
#pragma unroll
        for (int q = 0; q < G::kPixels; ++q) {
          if (x0 + q < width) {
            if constexpr (G::kElem == 1) static_cast<unsigned char*>(out)[o0 + q] = (unsigned char)v[q];
            else if constexpr (G::kElem == 2) static_cast<unsigned short*>(out)[o0 + q] = (unsigned short)v[q];
            else if constexpr (G::kElem == 4) static_cast<int*>(out)[o0 + q] = (int)v[q];
            else static_cast<double*>(out)[o0 + q] = (double)v[q];
          }
        }
      }
    }
    if (more) pn_output_sync();                             // lane 63's row, before lane 0 of the next band reads it
  }
  if (__ballot(bad_filter) && lane == 0) atomicOr(status + f, 8);
}

struct PnLayout {
  int64_t inflated, frame_stride, frame_bytes, prev, prev_stride, seg_pos, head, stream_off, stream_len, out_off, out_cap, out_len,
      compact, total;
};

// (the compacted streams come last: nothing but their size depends on idat_bytes, which pl_png_decode is not told)
__host__ bool pn_layout(int64_t n, int64_t n_segments, int64_t idat_bytes, int width, int height, int bits, int samples, PnLayout* lay) {
  if (n < 1 || n > 65535 || n_segments < 1 || n_segments > ((int64_t)1 << 31) - 1) return false;
  if (width < 1 || height < 1 || idat_bytes < 0 || idat_bytes > ((int64_t)1 << 40)) return false;
  if (!((samples == 1 && (bits == 8 || bits == 16)) || (samples == 3 && bits == 8))) return false;
  const int64_t row_bytes = (int64_t)width * samples * (bits / 8);
  lay->frame_bytes = (int64_t)height * (1 + row_bytes);
  if (lay->frame_bytes > ((int64_t)1 << 31) - 1) return false;
  auto up = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
  int64_t at = 0;
  lay->frame_stride = up(lay->frame_bytes);
  lay->inflated = at, at += n * lay->frame_stride + 128;    // (the unfilter kernel loads whole chunks: a row's last one may end beyond it)
  lay->prev_stride = up(row_bytes) + 64;
  lay->prev = at, at += n * lay->prev_stride;
  lay->seg_pos = at, at += up(n_segments * 8);
  lay->stream_off = at, at += up(n * 8);
  lay->stream_len = at, at += up(n * 8);
  lay->out_off = at, at += up(n * 8);
  lay->out_cap = at, at += up(n * 8);
  lay->out_len = at, at += up(n * 8);
  lay->head = at, at += up(n * 4);
  lay->compact = at, at += up(idat_bytes) + 16;
  lay->total = at;
  return true;
}

// ---- the checked decode: chunk CRCs and the stream's Adler-32 (pl_png_decode_checked) ---------------------------------------
// (zip_kernels.h, included at the end of this file)
__host__ int64_t zp_crc_slots_bytes(int64_t n_ranges, int64_t max_len);
__host__ void zp_crc_launch(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_off, const int64_t* d_len, int64_t n_ranges,
                            int64_t max_len, const uint32_t* d_expected, uint32_t* d_crc, int32_t* d_status, unsigned char* d_slots,
                            hipStream_t st);

struct PnVerify {                                           // the chunk table, and where the checked mode's words live in d_work
  const int64_t* chunk_off;
  const int64_t* chunk_len;
  const uint32_t* chunk_crc;
  const int32_t* chunk_frame;
  int64_t n_chunks, max_chunk_len;
  int64_t trailer, judge, adler_slots, chunk_status, crc_slots;
};

// a chunk whose CRC-32 differs from the stored one (bit 3 of its own status, set by the CRC fold) or whose window lies outside
// the buffer (bit 0) flags its frame
__global__ void __launch_bounds__(kPnThreads)
png_chunk_verdict_kernel(const int32_t* __restrict__ chunk_status, const int32_t* __restrict__ chunk_frame, int64_t n_chunks,
                         int64_t n_frames, int32_t* __restrict__ status) {
  const int64_t c = (int64_t)blockIdx.x * kPnThreads + threadIdx.x;
  if (c >= n_chunks || chunk_status[c] == 0) return;
  const int f = chunk_frame[c];
  if (f >= 0 && f < n_frames) atomicOr(status + f, 16);
}

// the extra words lie where the plain layout has its compacted streams, which move behind them (they stay last)
__host__ bool pn_checked_layout(int64_t n, int64_t n_segments, int64_t idat_bytes, int width, int height, int bits, int samples,
                                int64_t n_chunks, int64_t max_chunk_len, PnLayout* lay, PnVerify* v) {
  if (!pn_layout(n, n_segments, idat_bytes, width, height, bits, samples, lay)) return false;
  const int64_t adler = pl_adler32_slots_bytes(n, lay->frame_bytes);
  const int64_t crc = zp_crc_slots_bytes(n_chunks, max_chunk_len);
  if (adler < 0 || crc < 0) return false;
  auto up = [](int64_t x) { return (x + 15) & ~(int64_t)15; };
  int64_t at = lay->compact;
  v->trailer = at, at += up(n * 4);
  v->judge = at, at += up(n * 4);                           // (zeroed together with the trailers)
  v->adler_slots = at, at += adler;
  v->chunk_status = at, at += up(n_chunks * 4);
  v->crc_slots = at, at += crc;
  lay->compact = at, at += up(idat_bytes) + 16;
  lay->total = at;
  v->n_chunks = n_chunks, v->max_chunk_len = max_chunk_len;
  return true;
}

// the launches of pl_png_decode (v null: four) and of pl_png_decode_checked (nine: the Adler pair after the inflate launch,
// the CRC pair and the chunks' verdict at the end)
__host__ int pn_run(const char* who, const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_seg_off, const int64_t* d_seg_len,
                    const int32_t* d_seg_frame, int64_t n_segments, int64_t n, int width, int height, int bits, int samples,
                    void* d_out, int out_kind, int32_t* d_status, unsigned char* d_work, const PnLayout& lay, const PnVerify* v,
                    hipStream_t st) {
  bool zeroed = hipMemsetAsync(d_status, 0, (size_t)n * 4, st) == hipSuccess;
  if (v) {
    zeroed = zeroed && hipMemsetAsync(d_work + v->trailer, 0, (size_t)(v->adler_slots - v->trailer), st) == hipSuccess &&
             hipMemsetAsync(d_work + v->chunk_status, 0, (size_t)v->n_chunks * 4, st) == hipSuccess;
  }
  if (!zeroed) {
    pl_set_error("%s: memset failed", who);
    return PL_ERR_HIP;
  }
  int64_t* seg_pos = reinterpret_cast<int64_t*>(d_work + lay.seg_pos);
  int64_t* stream_off = reinterpret_cast<int64_t*>(d_work + lay.stream_off);
  int64_t* stream_len = reinterpret_cast<int64_t*>(d_work + lay.stream_len);
  int64_t* out_off = reinterpret_cast<int64_t*>(d_work + lay.out_off);
  int64_t* out_cap = reinterpret_cast<int64_t*>(d_work + lay.out_cap);
  int64_t* out_len = reinterpret_cast<int64_t*>(d_work + lay.out_len);
  int32_t* head = reinterpret_cast<int32_t*>(d_work + lay.head);
  unsigned char* compact = d_work + lay.compact;
  unsigned char* inflated = d_work + lay.inflated;
  hipLaunchKernelGGL(png_check_kernel, dim3(1), dim3(kPnThreads), 0, st, d_seg_off, d_seg_len, d_seg_frame, n_segments, nbytes, n,
                     lay.frame_stride, lay.frame_bytes, seg_pos, head, stream_off, stream_len, out_off, out_cap, d_status);
  hipLaunchKernelGGL(png_gather_kernel, dim3((unsigned)n_segments, 4), dim3(kPnThreads), 0, st, d_bytes, nbytes, d_seg_off, d_seg_len,
                     d_seg_frame, n_segments, n, seg_pos, stream_off, stream_len, compact, d_status);
  // (the streams were laid out by the check kernel inside the compacted area: its size is the caller's idat_bytes)
  if (!v) {
    pl_inflate_launch(false, compact, (int64_t)1 << 50, stream_off, stream_len, n, 1, inflated, out_off, out_cap, out_len, d_status,
                      PnChecked{}, st);
  } else {
    // a stream that goes on beyond the frame is no error for a PNG (PIL stops reading there): its checksum is not judged
    uint32_t* trailer = reinterpret_cast<uint32_t*>(d_work + v->trailer);
    int32_t* judge = reinterpret_cast<int32_t*>(d_work + v->judge);
    pl_inflate_launch(true, compact, (int64_t)1 << 50, stream_off, stream_len, n, 1, inflated, out_off, out_cap, out_len, d_status,
                      PnChecked{trailer, judge, nullptr, lay.frame_bytes, 0}, st);
    pl_adler32_launch(inflated, (int64_t)1 << 50, out_off, out_len, n, lay.frame_bytes, judge, trailer, 32, nullptr, d_status,
                      d_work + v->adler_slots, st);
  }
  unsigned char* prev = d_work + lay.prev;
#define PN_FINISH(BYTES, SPP, OUT)                                                                                          \
  hipLaunchKernelGGL((png_unfilter_kernel<BYTES, SPP, OUT>), dim3((unsigned)n), dim3(PL_WAVE), 0, st, inflated, lay.frame_stride, \
                     prev, lay.prev_stride, width, height, out_len, d_out, d_status)
#define PN_OUT(BYTES, SPP)                         \
  if (out_kind == 0) PN_FINISH(BYTES, SPP, 0);     \
  else if (out_kind == 1) PN_FINISH(BYTES, SPP, 1); \
  else PN_FINISH(BYTES, SPP, 2)
  if (samples == 3) { PN_OUT(1, 3); }
  else if (bits == 8) { PN_OUT(1, 1); }
  else { PN_OUT(2, 1); }
#undef PN_OUT
#undef PN_FINISH
  if (v) {
    int32_t* chunk_status = reinterpret_cast<int32_t*>(d_work + v->chunk_status);
    zp_crc_launch(d_bytes, nbytes, v->chunk_off, v->chunk_len, v->n_chunks, v->max_chunk_len, v->chunk_crc, nullptr, chunk_status,
                  d_work + v->crc_slots, st);
    hipLaunchKernelGGL(png_chunk_verdict_kernel, dim3((unsigned)pl_cdiv(v->n_chunks, kPnThreads)), dim3(kPnThreads), 0, st, chunk_status,
                       v->chunk_frame, v->n_chunks, n, d_status);
  }
  return pl_check_launch(who);
}

}  // namespace

// the one place inflate_kernel is launched from outside zip_kernels.h (pl_common.h: tiff.hip's Deflate strips come through here)
void pl_inflate_launch(bool checked, const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_in_off, const int64_t* d_in_len,
                       int64_t n_streams, int wrapper, unsigned char* d_out, const int64_t* d_out_off, const int64_t* d_out_cap,
                       int64_t* d_out_len, int32_t* d_status, PnChecked chk, hipStream_t st) {
  if (checked)
    hipLaunchKernelGGL(inflate_kernel<true>, dim3((unsigned)n_streams), dim3(PL_WAVE), 0, st, d_bytes, nbytes, d_in_off, d_in_len,
                       wrapper, d_out, d_out_off, d_out_cap, d_out_len, d_status, chk);
  else
    hipLaunchKernelGGL(inflate_kernel<false>, dim3((unsigned)n_streams), dim3(PL_WAVE), 0, st, d_bytes, nbytes, d_in_off, d_in_len,
                       wrapper, d_out, d_out_off, d_out_cap, d_out_len, d_status, chk);
}

extern "C" int pl_inflate(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_in_off, const int64_t* d_in_len,
                          int64_t n_streams, int wrapper, unsigned char* d_out, const int64_t* d_out_off, const int64_t* d_out_cap,
                          int64_t* d_out_len, int32_t* d_status, void* stream) {
  PL_REQUIRE(d_bytes && d_in_off && d_in_len && d_out && d_out_off && d_out_cap && d_out_len && d_status, "null pointer");
  PL_REQUIRE(((uintptr_t)d_bytes & 3) == 0, "the byte buffer must start on a 4-byte boundary (streams inside it may start anywhere)");
  PL_REQUIRE(n_streams >= 1 && n_streams <= ((int64_t)1 << 31) - 1, "1 <= n_streams < 2^31");
  PL_REQUIRE(wrapper == 0 || wrapper == 1, "wrapper 0 (raw Deflate) or 1 (zlib)");
  PL_REQUIRE(nbytes >= 0, "bad buffer size");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(d_status, 0, (size_t)n_streams * 4, st) != hipSuccess) {
    pl_set_error("pl_inflate: memset failed");
    return PL_ERR_HIP;
  }
  pl_inflate_launch(false, d_bytes, nbytes, d_in_off, d_in_len, n_streams, wrapper, d_out, d_out_off, d_out_cap, d_out_len, d_status,
                    PnChecked{}, st);
  return pl_check_launch("pl_inflate");
}

extern "C" int64_t pl_png_work_bytes(int64_t n, int64_t n_segments, int64_t idat_bytes, int width, int height, int bits,
                                     int samples) {
  PnLayout lay;
  return pn_layout(n, n_segments, idat_bytes, width, height, bits, samples, &lay) ? lay.total : -1;
}

extern "C" int pl_png_decode(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_seg_off, const int64_t* d_seg_len,
                             const int32_t* d_seg_frame, int64_t n_segments, int64_t n, int width, int height, int bits,
                             int samples, void* d_out, int out_kind, int32_t* d_status, unsigned char* d_work, void* stream) {
  if (!((samples == 1 && (bits == 8 || bits == 16)) || (samples == 3 && bits == 8))) {
    pl_set_error("pl_png_decode: unsupported samples (%d x %d bits): grey of 8 or 16 bits, RGB of 8", samples, bits);
    return PL_ERR_UNSUPPORTED;
  }
  PL_REQUIRE(d_bytes && d_seg_off && d_seg_len && d_seg_frame && d_out && d_status && d_work, "null pointer");
  PL_REQUIRE(((uintptr_t)d_bytes & 3) == 0, "the byte buffer must start on a 4-byte boundary (segments inside it may start anywhere)");
  PL_REQUIRE(((uintptr_t)d_work & 15) == 0, "d_work must start on a 16-byte boundary");
  PL_REQUIRE(out_kind >= 0 && out_kind <= 2, "out_kind 0 (container dtype), 1 (uint16) or 2 (float64)");
  PL_REQUIRE(nbytes >= 0 && nbytes <= ((int64_t)1 << 40), "bad buffer size");
  PnLayout lay;
  PL_REQUIRE(pn_layout(n, n_segments, 0, width, height, bits, samples, &lay),
             "1 <= n <= 65535, n_segments >= 1, width, height >= 1, a frame (with its filter bytes) below 2 GiB");
  return pn_run("pl_png_decode", d_bytes, nbytes, d_seg_off, d_seg_len, d_seg_frame, n_segments, n, width, height, bits, samples, d_out,
                out_kind, d_status, d_work, lay, nullptr, (hipStream_t)stream);
}

#include "zip_kernels.h"

// ---- the checked entry points (after zip_kernels.h: the chunk CRCs go through its launches) ---------------------------------
namespace {

struct PnInflateLayout {
  int64_t trailer, judge, slots, total;
};

__host__ bool pn_inflate_layout(int64_t n, int64_t max_out, PnInflateLayout* lay) {
  const int64_t slots = pl_adler32_slots_bytes(n, max_out);
  if (slots < 0) return false;
  auto up = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
  int64_t at = 0;
  lay->trailer = at, at += up(n * 4);
  lay->judge = at, at += up(n * 4);
  lay->slots = at, at += slots;
  lay->total = at;
  return true;
}

}  // namespace

extern "C" int64_t pl_inflate_checked_work_bytes(int64_t n_streams, int64_t max_out) {
  PnInflateLayout lay;
  return pn_inflate_layout(n_streams, max_out, &lay) ? lay.total : -1;
}

extern "C" int pl_inflate_checked(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_in_off, const int64_t* d_in_len,
                                  int64_t n_streams, unsigned char* d_out, const int64_t* d_out_off, const int64_t* d_out_cap,
                                  int64_t max_out, int64_t* d_out_len, int64_t* d_in_used, int32_t* d_status, unsigned char* d_work,
                                  void* stream) {
  PL_REQUIRE(d_bytes && d_in_off && d_in_len && d_out && d_out_off && d_out_cap && d_out_len && d_in_used && d_status && d_work,
             "null pointer");
  PL_REQUIRE(((uintptr_t)d_bytes & 3) == 0, "the byte buffer must start on a 4-byte boundary (streams inside it may start anywhere)");
  PL_REQUIRE(((uintptr_t)d_out & 3) == 0, "d_out must start on a 4-byte boundary");
  PL_REQUIRE(((uintptr_t)d_work & 15) == 0, "d_work must start on a 16-byte boundary");
  PL_REQUIRE(nbytes >= 0, "bad buffer size");
  PnInflateLayout lay;
  PL_REQUIRE(pn_inflate_layout(n_streams, max_out, &lay), "1 <= n_streams < 2^31, 0 <= max_out <= 65535 x 16 KiB");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(d_status, 0, (size_t)n_streams * 4, st) != hipSuccess ||
      hipMemsetAsync(d_work, 0, (size_t)lay.slots, st) != hipSuccess) {
    pl_set_error("pl_inflate_checked: memset failed");
    return PL_ERR_HIP;
  }
  uint32_t* trailer = reinterpret_cast<uint32_t*>(d_work + lay.trailer);
  int32_t* judge = reinterpret_cast<int32_t*>(d_work + lay.judge);
  pl_inflate_launch(true, d_bytes, nbytes, d_in_off, d_in_len, n_streams, 1, d_out, d_out_off, d_out_cap, d_out_len, d_status,
                    PnChecked{trailer, judge, d_in_used, max_out, 16}, st);
  // the checksum of what was STORED, for the streams that ended where they should (the caller owns d_out: its size is unknown
  // here, and the Adler kernels read no dword outside a range)
  pl_adler32_launch(d_out, (int64_t)1 << 50, d_out_off, d_out_len, n_streams, max_out, judge, trailer, 8, nullptr, d_status,
                    d_work + lay.slots, st);
  return pl_check_launch("pl_inflate_checked");
}

extern "C" int64_t pl_png_checked_work_bytes(int64_t n, int64_t n_segments, int64_t idat_bytes, int width, int height, int bits,
                                             int samples, int64_t n_chunks, int64_t max_chunk_len) {
  PnLayout lay;
  PnVerify v;
  return pn_checked_layout(n, n_segments, idat_bytes, width, height, bits, samples, n_chunks, max_chunk_len, &lay, &v) ? lay.total : -1;
}

extern "C" int pl_png_decode_checked(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_seg_off, const int64_t* d_seg_len,
                                     const int32_t* d_seg_frame, int64_t n_segments, int64_t n, int width, int height, int bits,
                                     int samples, void* d_out, int out_kind, int32_t* d_status, unsigned char* d_work,
                                     const int64_t* d_chunk_off, const int64_t* d_chunk_len, const uint32_t* d_chunk_crc,
                                     const int32_t* d_chunk_frame, int64_t n_chunks, int64_t max_chunk_len, void* stream) {
  if (!((samples == 1 && (bits == 8 || bits == 16)) || (samples == 3 && bits == 8))) {
    pl_set_error("pl_png_decode_checked: unsupported samples (%d x %d bits): grey of 8 or 16 bits, RGB of 8", samples, bits);
    return PL_ERR_UNSUPPORTED;
  }
  PL_REQUIRE(d_bytes && d_seg_off && d_seg_len && d_seg_frame && d_out && d_status && d_work, "null pointer");
  PL_REQUIRE(d_chunk_off && d_chunk_len && d_chunk_crc && d_chunk_frame, "null pointer (the chunk table)");
  PL_REQUIRE(((uintptr_t)d_bytes & 3) == 0, "the byte buffer must start on a 4-byte boundary (segments inside it may start anywhere)");
  PL_REQUIRE(((uintptr_t)d_work & 15) == 0, "d_work must start on a 16-byte boundary");
  PL_REQUIRE(out_kind >= 0 && out_kind <= 2, "out_kind 0 (container dtype), 1 (uint16) or 2 (float64)");
  PL_REQUIRE(nbytes >= 0 && nbytes <= ((int64_t)1 << 40), "bad buffer size");
  PnLayout lay;
  PnVerify v;
  PL_REQUIRE(pn_checked_layout(n, n_segments, 0, width, height, bits, samples, n_chunks, max_chunk_len, &lay, &v),
             "1 <= n <= 65535, n_segments >= 1, width, height >= 1, a frame (with its filter bytes) of at most 65535 x 16 KiB, "
             "1 <= n_chunks < 2^31, 0 <= max_chunk_len <= 65535 x 16 KiB");
  v.chunk_off = d_chunk_off, v.chunk_len = d_chunk_len, v.chunk_crc = d_chunk_crc, v.chunk_frame = d_chunk_frame;
  return pn_run("pl_png_decode_checked", d_bytes, nbytes, d_seg_off, d_seg_len, d_seg_frame, n_segments, n, width, height, bits,
                samples, d_out, out_kind, d_status, d_work, lay, &v, (hipStream_t)stream);
}
