// DICOM native (uncompressed) Pixel Data -> typed frames on the device: the step BEFORE the hot path (SURVEY.md section 8 row
// f1; pylinac/core/image.py:1383-1444 `DicomImage.__init__`: `self.metadata.pixel_array` -> optional `.astype(dtype)` ->
// `_rescale_dicom_values` :363-389).  The arithmetic is pydicom's (pinned `pydicom>=2.0,<3` in the reference's
// pyproject.toml:40; its source is absent from /root/reference): pixel_data_handlers/numpy_handler.py `get_pixeldata` =
// `np.frombuffer(PixelData[:expected_len], dtype=pixel_dtype(ds))` with pixel_dtype = '<' or '>' by transfer syntax, 'u' or
// 'i' by PixelRepresentation, BitsAllocated / 8 bytes -- the CONTAINER value, bits above BitsStored included -- reshaped to
// (NumberOfFrames, Rows, Columns); `apply_rescale` (= apply_modality_lut) = `arr.astype(float64) * RescaleSlope`, then
// `+= RescaleIntercept` (two roundings).  `unused_bits` = 1 adds what pydicom >= 3 does by default for native data
// (`correct_unused_bits`): unsigned samples keep their low BitsStored bits, signed samples are sign-extended from bit
// BitsStored - 1.
//
// One launch decodes a BATCH of frames that lie anywhere in one device buffer (whole Part-10 files copied as they are, or a
// multi-frame Pixel Data element): frame f starts at byte d_offsets[f], at ANY alignment.  A lane takes 16 source bytes per
// step as an aligned 4-dword load plus the dword that follows, funnel-shifted by the frame's misalignment (v_alignbit), so
// the stream stays coalesced whatever the file layout; the kernel is a copy: HBM-bound, 2 x the frame bytes (container
// output) or 1 + 8 / BitsAllocated-bytes x (float64 output).
#include "pl_common.h"

// jpeg_lossless.hip, jpeg2000.hip and dicom_encap.hip are translation units of their own in the library; the CPU emulator of the tests
// builds a fixed list of files that holds this one, so there they are compiled as parts of this file
#ifdef PL_HIPEMU
#define PL_JPEGLL_IN_DICOM
#include "jpeg_lossless.hip"
#define PL_ENCAP_IN_DICOM
#include "dicom_encap.hip"
#define PL_J2K_IN_DICOM
#include "jpeg2000.hip"
#endif

namespace {

constexpr int kDcThreads = 256;

struct alignas(4) DcU4 { unsigned x, y, z, w; };

__device__ __forceinline__ unsigned dc_bswap16x2(unsigned v) { return __builtin_amdgcn_perm(v, v, 0x02030001u); }
__device__ __forceinline__ unsigned dc_bswap32(unsigned v) { return __builtin_amdgcn_perm(v, v, 0x00010203u); }

// one container sample (already in little-endian order) -> its value as a signed 64-bit integer
template <int IB>
__device__ __forceinline__ long long dc_value(unsigned raw, bool is_signed, int stored, bool fix_unused) {
  constexpr int BITS = IB * 8;
  unsigned v = raw;
  if (fix_unused && stored < BITS) {
    if (is_signed) {
      const int sh = 32 - stored;
      return (long long)((int)(v << sh) >> sh);
    }
    v &= (1u << stored) - 1u;
    return (long long)v;
  }
  if (is_signed) {
    const int sh = 32 - BITS;
    return (long long)((int)(v << sh) >> sh);
  }
  return (long long)v;
}

template <typename OutT>
__device__ __forceinline__ OutT dc_out(long long v, bool rescale, double slope, double intercept) {
  if constexpr (sizeof(OutT) == 8) {
    double d = (double)v;                                   // arr.astype(np.float64): exact for every container value
    if (rescale) {
      d = d * slope;                                        // two IEEE operations, like numpy's (no FMA: -ffp-contract=off)
      d = d + intercept;
    }
    return d;
  } else {
    return (float)v;                                        // arr.astype(np.float32): RN of the integer, like numpy's cast
  }
}

// IB = bytes per container sample; MODE 0: container output (same width, the bits as stored or with the unused bits fixed),
// 1: float32, 2: float64 (+ optional rescale)
template <int IB, int MODE>
__global__ void __launch_bounds__(kDcThreads)
dicom_decode_kernel(const unsigned char* __restrict__ bytes, int64_t nbytes, const int64_t* __restrict__ offsets,
                    int64_t samples /* per frame */, int is_signed, int stored, int big_endian, int fix_unused, int rescale,
                    double slope, double intercept, void* __restrict__ out, int32_t* __restrict__ status) {
  const int64_t f = blockIdx.y;
  const int64_t off = offsets[f];
  const int64_t frame_bytes = samples * IB;
  // a frame that does not lie inside the buffer is reported, not read (pydicom: "The length of the pixel data in the
  // dataset doesn't match the expected length" -> ValueError)
  const bool inside = off >= 0 && off + frame_bytes <= nbytes;
  if (blockIdx.x == 0 && threadIdx.x == 0) status[f] = inside ? 0 : 1;
  if (!inside) return;
  const unsigned sh = (unsigned)(off & 3) * 8u;
  const unsigned* base = reinterpret_cast<const unsigned*>(bytes + (off & ~(int64_t)3));
  const int64_t last_dword = ((nbytes + 3) >> 2) - 1 - ((off & ~(int64_t)3) >> 2);   // the last dword of the buffer, from base
  const int64_t nvec = frame_bytes >> 4;                   // whole 16-byte steps
  constexpr int SPV = 16 / IB;                             // samples per step
  const bool fixu = fix_unused != 0, sgn = is_signed != 0, resc = rescale != 0;
  auto fix_dword = [&](unsigned d) -> unsigned {           // container output: byte order + unused bits, in place
    if (IB == 2) {
      if (big_endian) d = dc_bswap16x2(d);
      if (fixu && stored < 16) {
        if (sgn) {                                         // sign-extend each half from bit stored - 1
          const int sx = 32 - stored;
          const int lo = (int)(d << (16 + (16 - stored))) >> sx;          // low sample moved to the top, then down
          const int hi = (int)((d >> 16) << sx) >> sx;
          d = ((unsigned)lo & 0xffffu) | ((unsigned)hi << 16);
        } else {
          const unsigned m = (1u << stored) - 1u;
          d &= m | (m << 16);
        }
      }
    } else if (IB == 4) {
      if (big_endian) d = dc_bswap32(d);
      if (fixu && stored < 32) {
        if (sgn) d = (unsigned)(((int)(d << (32 - stored))) >> (32 - stored));
        else d &= (1u << stored) - 1u;
      }
    } else {
      if (fixu && stored < 8) {
        unsigned r = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          unsigned s = (d >> (8 * b)) & 0xffu;
          if (sgn) s = (unsigned)(((int)(s << (32 - stored))) >> (32 - stored)) & 0xffu;
          else s &= (1u << stored) - 1u;
          r |= s << (8 * b);
        }
        d = r;
      }
    }
    return d;
  };
  for (int64_t v = (int64_t)blockIdx.x * kDcThreads + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * kDcThreads) {
    const DcU4 q = *reinterpret_cast<const DcU4*>(base + 4 * v);
    unsigned d[4] = {q.x, q.y, q.z, q.w};
    if (sh) {                                              // (wave-uniform: a property of the frame)
      const int64_t nx = 4 * v + 4;
      const unsigned e = base[nx <= last_dword ? nx : last_dword];     // beyond the buffer only bits nothing uses are needed
      d[0] = __builtin_amdgcn_alignbit(d[1], d[0], sh);
      d[1] = __builtin_amdgcn_alignbit(d[2], d[1], sh);
      d[2] = __builtin_amdgcn_alignbit(d[3], d[2], sh);
      d[3] = __builtin_amdgcn_alignbit(e, d[3], sh);
    }
    if constexpr (MODE == 0) {
      DcU4 o{fix_dword(d[0]), fix_dword(d[1]), fix_dword(d[2]), fix_dword(d[3])};
      *reinterpret_cast<DcU4*>(static_cast<unsigned char*>(out) + f * frame_bytes + 16 * v) = o;
    } else {
      using OutT = typename std::conditional<MODE == 1, float, double>::type;
      OutT* o = static_cast<OutT*>(out) + f * samples + v * SPV;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        unsigned w = d[k];
        if (IB == 2 && big_endian) w = dc_bswap16x2(w);
        if (IB == 4 && big_endian) w = dc_bswap32(w);
#pragma unroll
        for (int j = 0; j < 4 / IB; ++j) {
          const unsigned raw = IB == 4 ? w : (IB == 2 ? (w >> (16 * j)) & 0xffffu : (w >> (8 * j)) & 0xffu);
          o[k * (4 / IB) + j] = dc_out<OutT>(dc_value<IB>(raw, sgn, stored, fixu), resc, slope, intercept);
        }
      }
    }
  }
  // the frame's last bytes (fewer than 16): one sample per lane of the first workgroup, byte loads
  if (blockIdx.x == 0) {
    const int64_t s0 = nvec * SPV;
    for (int64_t s = s0 + threadIdx.x; s < samples; s += kDcThreads) {
      const unsigned char* p = bytes + off + s * IB;
      unsigned raw = 0;
#pragma unroll
      for (int b = 0; b < IB; ++b) raw |= (unsigned)p[b] << (8 * (big_endian ? IB - 1 - b : b));
      if constexpr (MODE == 0) {
        const long long val = dc_value<IB>(raw, sgn, stored, fixu);
        unsigned char* o = static_cast<unsigned char*>(out) + f * frame_bytes + s * IB;
#pragma unroll
        for (int b = 0; b < IB; ++b) o[b] = (unsigned char)((unsigned long long)val >> (8 * b));
      } else {
        using OutT = typename std::conditional<MODE == 1, float, double>::type;
        static_cast<OutT*>(out)[f * samples + s] = dc_out<OutT>(dc_value<IB>(raw, sgn, stored, fixu), resc, slope, intercept);
      }
    }
  }
}

}  // namespace

extern "C" int pl_dicom_decode(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_offsets, int64_t n, int rows,
                               int cols, int bits_allocated, int bits_stored, int pixel_representation, int big_endian,
                               int unused_bits, void* d_out, int out_dtype, int rescale, double slope, double intercept,
                               int32_t* d_status, void* stream) {
  PL_REQUIRE(d_bytes && d_offsets && d_out && d_status, "null pointer");
  PL_REQUIRE(((uintptr_t)d_bytes & 3) == 0, "the byte buffer must start on a 4-byte boundary (frames inside it may start anywhere)");
  PL_REQUIRE(n >= 0 && n <= 65535 && rows > 0 && cols > 0 && nbytes >= 0, "bad shape");
  PL_REQUIRE(bits_allocated == 8 || bits_allocated == 16 || bits_allocated == 32, "BitsAllocated 8, 16 or 32");
  PL_REQUIRE(bits_stored >= 1 && bits_stored <= bits_allocated, "1 <= BitsStored <= BitsAllocated");
  PL_REQUIRE(pixel_representation == 0 || pixel_representation == 1, "PixelRepresentation 0 (unsigned) or 1 (two's complement)");
  const int ib = bits_allocated / 8;
  // the container dtype of pydicom's pixel_dtype: 8-bit PL_U8, 16-bit PL_U16 / PL_I16 by PixelRepresentation, 32-bit PL_I32
  // (wider-than-16 unsigned types travel as their same-width signed bits, as everywhere in this ABI; so does int8 as PL_U8)
  const int container = ib == 1 ? PL_U8 : (ib == 2 ? (pixel_representation ? PL_I16 : PL_U16) : PL_I32);
  PL_REQUIRE(out_dtype == container || out_dtype == PL_F32 || out_dtype == PL_F64,
             "output: the container dtype of BitsAllocated / PixelRepresentation, float32 or float64");
  PL_REQUIRE(!rescale || out_dtype == PL_F64, "the rescale is float64 arithmetic");
  if (n == 0) return PL_OK;
  const int64_t samples = (int64_t)rows * cols;
  const int mode = out_dtype == container ? 0 : (out_dtype == PL_F32 ? 1 : 2);
  // the container form stores 16-byte vectors at 4-byte alignment: frames of a byte count that is no multiple of 4 (odd
  // 8- or 16-bit frames) would misalign the next frame's stores
  PL_REQUIRE(mode != 0 || n == 1 || (samples * ib) % 4 == 0, "container output of a batch needs rows * cols * bytes % 4 == 0");
  const int64_t nvec = samples * ib / 16;
  int64_t bx = pl_cdiv(nvec, (int64_t)kDcThreads * 4);
  if (bx < 1) bx = 1;
  if (bx > 4096) bx = 4096;
  const dim3 grid((unsigned)bx, (unsigned)n);
  hipStream_t st = (hipStream_t)stream;
#define DC_LAUNCH(IB, MODE)                                                                                              \
  hipLaunchKernelGGL((dicom_decode_kernel<IB, MODE>), grid, dim3(kDcThreads), 0, st, d_bytes, nbytes, d_offsets, samples, \
                     pixel_representation, bits_stored, big_endian, unused_bits, rescale, slope, intercept, d_out, d_status)
#define DC_MODE(IB)                          \
  if (mode == 0) DC_LAUNCH(IB, 0);           \
  else if (mode == 1) DC_LAUNCH(IB, 1);      \
  else DC_LAUNCH(IB, 2)
  if (ib == 1) { DC_MODE(1); }
  else if (ib == 2) { DC_MODE(2); }
  else { DC_MODE(4); }
#undef DC_MODE
#undef DC_LAUNCH
  return pl_check_launch("pl_dicom_decode");
}

// ---------------------------------------------------------------------------------------------------------------------
// RLE Lossless Pixel Data (transfer syntax 1.2.840.10008.1.2.5; PS3.5 Annex G and section A.4.2) -> the NATIVE frame buffer
// pl_dicom_decode reads.  The arithmetic is pydicom 2.x's pixel_data_handlers/rle_handler.py: `_rle_decode_frame` takes
// segment s of a frame (SamplesPerPixel 1: BitsAllocated / 8 segments, the MOST significant byte plane first) through
// `_rle_decode_segment`, a PackBits walk: control byte c, then
//   c < 128: the next c + 1 bytes are copied (fewer when the segment ends first);
//   c > 128: the next byte is repeated 257 - c times (nothing when the segment has ended);
//   c = 128: nothing;
// until the segment's bytes are used up.  The first rows * cols decoded bytes are the plane; fewer is pydicom's ValueError
// ("The amount of decoded RLE segment data doesn't match the expected amount"), more its "non-conformant padding" warning.
//
// A walk is a chain of control bytes -- up to a million dependent steps for a 1024 x 1024 plane -- and no lane walks one.
// Every segment is cut into chunks of kRleChunk INPUT bytes.  A control byte before a chunk starts a run that ends at most
// 128 bytes into it (c = 127 at the chunk's last byte: 1 + 128 bytes), so the chunk's first true control byte lies at an
// ENTRY OFFSET 0 .. 128 -- 129 cases, whatever came before:
//   pass 1 (chunks x segments x frames): next[i] / out[i] for every position of the chunk as if it were a control byte, then
//          pointer doubling in LDS (at most kRleRounds rounds): for each entry offset, where the walk leaves the chunk (an entry
//          offset of the next one) and how many bytes it produces inside it -> a [chunks][129] table of (count << 8 | exit);
//   pass 2 (segments x frames): the chain e_0 = 0, e_{j+1} = exit[j][e_j], off_{j+1} = off_j + count[j][e_j] over the table,
//          staged into LDS a batch of rows at a time; the final offset gives the status bits (short / extra);
//   pass 3 (chunks x segments x frames): the chunk knows its entry and its output offset: the same next[] at up to ten doubling
//          levels marks the positions the walk visits, a scan over the marked controls gives every run its output offset,
//          and groups of 16 lanes expand the runs into byte (bytes_per_sample - 1 - s) of the little-endian samples.
// Every byte a lane reads lies inside its segment's [offset, offset + length) window, which every pass checks against the
// buffer first: a frame with a window outside it (or longer than max_segment_bytes, which sizes the tables) is flagged with
// status bit 0 and touched by no pass.
namespace {

constexpr int kRleChunk = PL_DICOM_RLE_CHUNK;              // input bytes per chunk
constexpr int kRleThreads = 256;
constexpr int kRlePer = kRleChunk / kRleThreads;           // positions per lane
constexpr int kRleEntries = 129;                           // entry offsets 0 .. 128
constexpr int kRleRounds = 10;                             // 2^kRleRounds >= kRleChunk: a walk makes at most one step per byte
constexpr int kRleBatch = 64;                              // table rows pass 2 stages at a time (64 * 129 * 4 = 33 KB of LDS)
constexpr int kRleGroup = 16;                              // lanes that expand one run
static_assert(kRleChunk >= 129 && kRleChunk % kRleThreads == 0 && (1 << kRleRounds) >= kRleChunk, "chunk size");
static_assert((int64_t)kRleChunk * 64 < (1 << 24), "a chunk's output count shares a word with its exit offset");
static_assert(kRleThreads >= kRleEntries, "one lane per entry offset");

struct RleWindow {
  const unsigned char* seg;                                // this workgroup's segment
  int64_t len;
  bool ok;                                                 // every segment window of the FRAME lies inside the buffer
};

__device__ __forceinline__ RleWindow rle_window(const unsigned char* __restrict__ bytes, int64_t nbytes,
                                                const int64_t* __restrict__ seg_off, const int64_t* __restrict__ seg_len,
                                                int64_t frame, int segments, int seg, int64_t max_segment_bytes) {
  RleWindow w;
  w.ok = true;
  for (int s = 0; s < segments; ++s) {
    const int64_t o = seg_off[frame * segments + s], l = seg_len[frame * segments + s];
    // (differences of lengths, never sums of an offset and a length: nothing here can overflow)
    w.ok = w.ok && o >= 0 && l >= 0 && o <= nbytes && l <= nbytes - o && l <= max_segment_bytes;
  }
  w.seg = bytes + (w.ok ? seg_off[frame * segments + seg] : 0);
  w.len = w.ok ? seg_len[frame * segments + seg] : 0;
  return w;
}

// position p of a chunk read as a control byte c; `after` = the segment's bytes that follow p (<= 0: p is its last byte)
// -> the position of the next control byte and the bytes this one produces
__device__ __forceinline__ void rle_step(unsigned c, int p, int64_t after, int& next, int& out) {
  if (c < 128u) {
    const int n = (int)c + 1;
    next = p + 1 + n;
    out = after >= n ? n : (after > 0 ? (int)after : 0);
  } else if (c > 128u) {
    next = p + 2;
    out = after > 0 ? 257 - (int)c : 0;
  } else {
    next = p + 1;
    out = 0;
  }
}

// exclusive prefix of `mine` over the kRleThreads lanes of a workgroup (every lane calls it)
template <typename U>
__device__ __forceinline__ U rle_block_exclusive(U mine, U* s_w) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  U inc = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const U v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  U off = inc - mine;
  for (int q = 0; q < wv; ++q) off += s_w[q];
  return off;
}

// pass 1
__global__ void __launch_bounds__(kRleThreads)
rle_table_kernel(const unsigned char* __restrict__ bytes, int64_t nbytes, const int64_t* __restrict__ seg_off,
                 const int64_t* __restrict__ seg_len, int segments, int64_t max_segment_bytes, int64_t n_chunks,
                 unsigned* __restrict__ table, int32_t* __restrict__ status, PlPackbitsGeom geom) {
  // nodes 0 .. kRleChunk + 128: a node at or beyond the chunk's bytes is an exit (it points at itself and produces nothing)
  __shared__ unsigned short s_next[kRleChunk + kRleEntries];
  __shared__ unsigned s_out[kRleChunk + kRleEntries];
  const int64_t frame = blockIdx.z, j = blockIdx.x;
  const int seg = blockIdx.y;
  const RleWindow win = rle_window(bytes, nbytes, seg_off, seg_len, frame, segments, seg, max_segment_bytes);
  if (!win.ok) {
    if (j == 0 && seg == 0 && threadIdx.x == 0) atomicOr(status + (geom.status_index ? geom.status_index[frame] : frame), 1);
    return;
  }
  const int64_t rem = win.len - j * kRleChunk;              // the segment's bytes from this chunk's first one on
  if (rem <= 0) return;                                     // (uniform) the segment has fewer chunks than the longest one
  const int clen = rem < kRleChunk ? (int)rem : kRleChunk;
  const unsigned char* src = win.seg + j * kRleChunk;
  unsigned char held[kRlePer];                              // the lane's bytes, loaded back to back (one memory latency, not four)
#pragma unroll
  for (int k = 0; k < kRlePer; ++k) {
    const int p = threadIdx.x + k * kRleThreads;
    held[k] = src[p < clen ? p : clen - 1];
  }
#pragma unroll
  for (int k = 0; k < kRlePer + 1; ++k) {
    const int p = threadIdx.x + k * kRleThreads;
    if (p >= kRleChunk + kRleEntries) break;
    int nx = p, out = 0;
    if (p < clen) rle_step(held[k < kRlePer ? k : 0], p, rem - 1 - p, nx, out);     // (p < clen <= kRleChunk: k < kRlePer)
    s_next[p] = (unsigned short)nx;
    s_out[p] = (unsigned)out;
  }
  __syncthreads();
  for (int r = 0; r < kRleRounds; ++r) {
    int nx[kRlePer];
    unsigned add[kRlePer];
#pragma unroll
    for (int k = 0; k < kRlePer; ++k) {
      const int a = s_next[threadIdx.x + k * kRleThreads];
      nx[k] = s_next[a];
      add[k] = s_out[a];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRlePer; ++k) {
      const int p = threadIdx.x + k * kRleThreads;
      s_next[p] = (unsigned short)nx[k];
      s_out[p] += add[k];
    }
    // the table asks for the 129 entry offsets alone: done once each of them has left the chunk (a chunk of literal runs
    // takes nine steps, four rounds).  Lane e reads the word it has just written itself.
    const int pending = threadIdx.x < kRleEntries && (int)s_next[threadIdx.x] < clen;
    if (!__syncthreads_or(pending)) break;
  }
  if (threadIdx.x < kRleEntries) {
    const int e = threadIdx.x;
    const int ex = (int)s_next[e] - kRleChunk;              // (a short last chunk: nobody follows its exit)
    table[(((frame * segments + seg) * n_chunks) + j) * kRleEntries + e] = (s_out[e] << 8) | (unsigned)(ex > 0 ? ex : 0);
  }
}

// pass 2
__global__ void __launch_bounds__(kRleThreads)
rle_chain_kernel(const unsigned char* __restrict__ bytes, int64_t nbytes, const int64_t* __restrict__ seg_off,
                 const int64_t* __restrict__ seg_len, int segments, int64_t max_segment_bytes, int64_t n_chunks,
                 int64_t samples, const unsigned* __restrict__ table, int64_t* __restrict__ chunk_off,
                 unsigned char* __restrict__ chunk_entry, int32_t* __restrict__ status, PlPackbitsGeom geom) {
  __shared__ unsigned s_tab[kRleBatch * kRleEntries];
  __shared__ int64_t s_off[kRleBatch];
  __shared__ unsigned char s_entry[kRleBatch];
  const int64_t frame = blockIdx.y;
  const int seg = blockIdx.x;
  const RleWindow win = rle_window(bytes, nbytes, seg_off, seg_len, frame, segments, seg, max_segment_bytes);
  if (!win.ok) return;
  const int64_t nck = (win.len + kRleChunk - 1) / kRleChunk, row0 = (frame * segments + seg) * n_chunks;
  unsigned e = 0;                                           // (lane 0's: the chain)
  int64_t off = 0;
  for (int64_t b0 = 0; b0 < nck; b0 += kRleBatch) {
    const int nb = nck - b0 < kRleBatch ? (int)(nck - b0) : kRleBatch;
    const unsigned* rows = table + (row0 + b0) * kRleEntries;
    for (int i = threadIdx.x; i < nb * kRleEntries; i += kRleThreads) s_tab[i] = rows[i];
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 0; k < nb; ++k) {
        s_entry[k] = (unsigned char)e;
        s_off[k] = off;
        const unsigned v = s_tab[k * kRleEntries + e];
        e = v & 0xffu;
        off += (int64_t)(v >> 8);                           // 64-bit: garbage may claim 128 output bytes per 2 input bytes
      }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nb; k += kRleThreads) {
      chunk_entry[row0 + b0 + k] = s_entry[k];
      chunk_off[row0 + b0 + k] = s_off[k];
    }
    __syncthreads();
  }
  if (geom.expect) {                                        // streams of another container: short is all they report
    if (threadIdx.x == 0 && off < geom.expect[frame]) atomicOr(status + geom.status_index[frame], 2);
    return;
  }
  if (threadIdx.x == 0 && off != samples) atomicOr(status + frame, off < samples ? 2 : 4);
}

// pass 3
__global__ void __launch_bounds__(kRleThreads)
rle_expand_kernel(const unsigned char* __restrict__ bytes, int64_t nbytes, const int64_t* __restrict__ seg_off,
                  const int64_t* __restrict__ seg_len, int segments, int64_t max_segment_bytes, int64_t n_chunks,
                  int64_t samples, const int64_t* __restrict__ chunk_off, const unsigned char* __restrict__ chunk_entry,
                  unsigned char* __restrict__ native, PlPackbitsGeom geom) {
  __shared__ unsigned char s_in[kRleChunk + 128];           // the chunk and the literal bytes a run may take beyond it
  __shared__ unsigned short s_lvl[kRleRounds][kRleChunk];   // level r: the control byte 2^r steps on (kRleChunk: none)
  __shared__ unsigned char s_mark[kRleChunk];
  __shared__ unsigned short s_run_pos[kRleChunk];
  __shared__ unsigned s_run_off[kRleChunk];
  __shared__ unsigned char s_run_len[kRleChunk];            // (stored as length - 1: 1 .. 128)
  __shared__ unsigned long long s_w[kRleThreads / PL_WAVE];
  __shared__ int s_runs;
  const int64_t frame = blockIdx.z, j = blockIdx.x;
  const int seg = blockIdx.y;
  const RleWindow win = rle_window(bytes, nbytes, seg_off, seg_len, frame, segments, seg, max_segment_bytes);
  if (!win.ok) return;
  const int64_t rem = win.len - j * kRleChunk;
  if (rem <= 0) return;
  if (geom.expect) samples = geom.expect[frame];            // (uniform) the stream's own output size
  const int64_t row = (frame * segments + seg) * n_chunks + j;
  const int clen = rem < kRleChunk ? (int)rem : kRleChunk;
  const int staged = rem < kRleChunk + 128 ? (int)rem : kRleChunk + 128;
  const unsigned char* src = win.seg + j * kRleChunk;
  // the chunk's record and the lane's bytes, loaded back to back (one memory latency)
  const int64_t off0 = chunk_off[row];
  const int entry = chunk_entry[row];
  unsigned char held[kRlePer + 1];
#pragma unroll
  for (int k = 0; k < kRlePer + 1; ++k) {
    const int p = threadIdx.x + k * kRleThreads;
    held[k] = src[p < staged ? p : staged - 1];
  }
  if (off0 >= samples) return;                              // (uniform) everything this chunk produces is dropped
#pragma unroll
  for (int k = 0; k < kRlePer + 1; ++k) {
    const int p = threadIdx.x + k * kRleThreads;
    if (p < staged) s_in[p] = held[k];
  }
  __syncthreads();
  // a lane takes kRlePer CONSECUTIVE positions (the scan below runs over positions in order)
  const int p0 = threadIdx.x * kRlePer;
  int outs[kRlePer];
#pragma unroll
  for (int k = 0; k < kRlePer; ++k) {
    const int p = p0 + k;
    int nx = kRleChunk;
    outs[k] = 0;
    if (p < clen) rle_step(s_in[p], p, rem - 1 - p, nx, outs[k]);
    s_lvl[0][p] = (unsigned short)(nx < clen ? nx : kRleChunk);
    s_mark[p] = p == entry && p < clen ? 1 : 0;
  }
  __syncthreads();
  // level r is needed while the walk from the entry makes more than 2^r steps inside the chunk (uniform: one LDS word)
  int levels = 1;
  for (int r = 1; r < kRleRounds && s_lvl[r - 1][entry] < kRleChunk; ++r) {
#pragma unroll
    for (int k = 0; k < kRlePer; ++k) {
      const int a = s_lvl[r - 1][p0 + k];
      s_lvl[r][p0 + k] = a < kRleChunk ? s_lvl[r - 1][a] : (unsigned short)kRleChunk;
    }
    __syncthreads();
    levels = r + 1;
  }
  // before round r the marks are the walk's steps 0, 2^(r+1), 2 * 2^(r+1), ...; the round adds the steps half way between
  // (a lane that sees a mark of this same round marks a position the walk visits as well: every mark is a true one)
  for (int r = levels - 1; r >= 0; --r) {
#pragma unroll
    for (int k = 0; k < kRlePer; ++k) {
      const int a = s_lvl[r][p0 + k];
      if (s_mark[p0 + k] && a < kRleChunk) s_mark[a] = 1;
    }
    __syncthreads();
  }
  // runs that produce something, in order: (index, output offset) by one scan of (1, out) pairs
  unsigned long long mine = 0;
#pragma unroll
  for (int k = 0; k < kRlePer; ++k)
    if (s_mark[p0 + k] && outs[k] > 0) mine += ((unsigned long long)outs[k] << 32) | 1ull;
  unsigned long long run = rle_block_exclusive(mine, s_w);
#pragma unroll
  for (int k = 0; k < kRlePer; ++k) {
    if (s_mark[p0 + k] && outs[k] > 0) {
      const unsigned idx = (unsigned)run;
      s_run_pos[idx] = (unsigned short)(p0 + k);
      s_run_off[idx] = (unsigned)(run >> 32);
      s_run_len[idx] = (unsigned char)(outs[k] - 1);
      run += ((unsigned long long)outs[k] << 32) | 1ull;
    }
  }
  if (threadIdx.x == kRleThreads - 1) s_runs = (int)(unsigned)run;
  __syncthreads();
  const int n_runs = s_runs, g = threadIdx.x / kRleGroup, l = threadIdx.x % kRleGroup;
  unsigned char* plane = geom.dst ? native + geom.dst[frame] : native + frame * samples * segments + (segments - 1 - seg);
  for (int q = g; q < n_runs; q += kRleThreads / kRleGroup) {
    const int p = s_run_pos[q], n = (int)s_run_len[q] + 1;
    const int64_t at = off0 + s_run_off[q];
    const bool literal = s_in[p] < 128u;
    for (int t = l; t < n; t += kRleGroup)
      if (at + t < samples) plane[(at + t) * segments] = s_in[p + 1 + (literal ? t : 0)];
  }
}

}  // namespace

extern "C" int64_t pl_dicom_rle_work_bytes(int64_t n_frames, int segments, int64_t max_segment_bytes) {
  if (n_frames < 1 || n_frames > 65535 || (segments != 1 && segments != 2 && segments != 4)) return -1;
  if (max_segment_bytes < 0 || max_segment_bytes > ((int64_t)1 << 36)) return -1;
  const int64_t n_chunks = pl_cdiv(max_segment_bytes > 0 ? max_segment_bytes : 1, kRleChunk);
  const int64_t rows = n_frames * segments * n_chunks;
  // chunk offsets (int64) | table (uint32 x 129) | chunk entries (uint8); every part 16-byte aligned
  return ((rows * 8 + 15) & ~(int64_t)15) + ((rows * kRleEntries * 4 + 15) & ~(int64_t)15) + ((rows + 15) & ~(int64_t)15);
}

// the three launches over validated arguments (d_work: pl_dicom_rle_work_bytes() bytes, 16-byte aligned)
static void rle_launch(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_seg_off, const int64_t* d_seg_len,
                       int64_t n_frames, int segments, int64_t max_segment_bytes, int64_t samples, unsigned char* d_native,
                       int32_t* d_status, unsigned char* d_work, PlPackbitsGeom geom, hipStream_t st) {
  const int64_t n_chunks = pl_cdiv(max_segment_bytes > 0 ? max_segment_bytes : 1, kRleChunk);
  const int64_t table_rows = n_frames * segments * n_chunks;
  int64_t* chunk_off = reinterpret_cast<int64_t*>(d_work);
  size_t at = (size_t)((table_rows * 8 + 15) & ~(int64_t)15);
  unsigned* table = reinterpret_cast<unsigned*>(d_work + at);
  at += (size_t)((table_rows * kRleEntries * 4 + 15) & ~(int64_t)15);
  unsigned char* chunk_entry = d_work + at;
  const dim3 blk(kRleThreads), per_chunk((unsigned)n_chunks, (unsigned)segments, (unsigned)n_frames);
  hipLaunchKernelGGL(rle_table_kernel, per_chunk, blk, 0, st, d_bytes, nbytes, d_seg_off, d_seg_len, segments,
                     max_segment_bytes, n_chunks, table, d_status, geom);
  hipLaunchKernelGGL(rle_chain_kernel, dim3((unsigned)segments, (unsigned)n_frames), blk, 0, st, d_bytes, nbytes, d_seg_off,
                     d_seg_len, segments, max_segment_bytes, n_chunks, samples, table, chunk_off, chunk_entry, d_status, geom);
  hipLaunchKernelGGL(rle_expand_kernel, per_chunk, blk, 0, st, d_bytes, nbytes, d_seg_off, d_seg_len, segments,
                     max_segment_bytes, n_chunks, samples, chunk_off, chunk_entry, d_native, geom);
}

// the same passes for PackBits streams of another container (pl_common.h: tiff.hip's strips); no argument is checked here
int64_t pl_packbits_work_bytes(int64_t n_streams, int64_t max_stream_bytes) {
  return pl_dicom_rle_work_bytes(n_streams, 1, max_stream_bytes);
}
void pl_packbits_expand(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_off, const int64_t* d_len,
                        int64_t n_streams, int64_t max_stream_bytes, unsigned char* d_out, int32_t* d_status,
                        unsigned char* d_work, PlPackbitsGeom geom, hipStream_t st) {
  rle_launch(d_bytes, nbytes, d_off, d_len, n_streams, 1, max_stream_bytes, 0, d_out, d_status, d_work, geom, st);
}

extern "C" int pl_dicom_rle_decode(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_seg_off,
                                   const int64_t* d_seg_len, int64_t n_frames, int segments, int64_t max_segment_bytes,
                                   int rows, int cols, unsigned char* d_native, int32_t* d_status, unsigned char* d_work,
                                   void* stream) {
  if (segments != 1 && segments != 2 && segments != 4) {
    pl_set_error("pl_dicom_rle_decode: unsupported segment count %d (BitsAllocated 8, 16 or 32 with SamplesPerPixel 1)", segments);
    return PL_ERR_UNSUPPORTED;
  }
  PL_REQUIRE(d_bytes && d_seg_off && d_seg_len && d_native && d_status && d_work, "null pointer");
  PL_REQUIRE(n_frames >= 1 && n_frames <= 65535, "1 <= n_frames <= 65535");
  PL_REQUIRE(rows >= 1 && cols >= 1 && nbytes >= 0, "bad shape");
  PL_REQUIRE(max_segment_bytes >= 0 && max_segment_bytes <= ((int64_t)1 << 36), "bad max_segment_bytes");
  PL_REQUIRE(((uintptr_t)d_work & 15) == 0, "d_work must start on a 16-byte boundary");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(d_status, 0, (size_t)n_frames * 4, st) != hipSuccess) {
    pl_set_error("pl_dicom_rle_decode: memset failed");
    return PL_ERR_HIP;
  }
  rle_launch(d_bytes, nbytes, d_seg_off, d_seg_len, n_frames, segments, max_segment_bytes, (int64_t)rows * cols, d_native,
             d_status, d_work, PlPackbitsGeom{nullptr, nullptr, nullptr}, st);
  return pl_check_launch("pl_dicom_rle_decode");
}
