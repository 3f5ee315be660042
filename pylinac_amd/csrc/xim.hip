// Varian XIM compressed-pixel decoding (SURVEY.md section 8 "next" row f1).
//
// Replaces: XIM._parse_lookup_table / _get_diffs / _parse_compressed_bytes (pylinac/core/image.py:1180-1296): the
// reference walks the variable-length difference stream run by run and then rebuilds the image one row at a time
// (cumsum per row in a Python loop, ~1 s per 1280 x 1280 image).  Both steps are scans:
//   * byte offset of difference i = exclusive prefix sum of the sizes 1 << code_i (2-bit codes, 4 per lookup byte)
//   * with S_r = row-wise prefix sums of the raw differences, the reference's recurrence is
//       P[r] = P[r-1] + S_r + c_r,   c_1 = -P[0][0],   c_r = c_{r-1} + S_{r-1}[W-1]
//     (derivation and check against the reference decoder: oracle/pylinac_oracle.py xim_decode), i.e. a row scan,
//     a scan of the row totals and a column scan -- all in the array dtype's wrap-around arithmetic (the pixel
//     array is int8/16/32/64 by bytes_per_pixel; 64-bit unsigned accumulators truncated at the store are the same
//     ring arithmetic).
#include "pl_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kItems = 8;                       // differences per lane = two lookup bytes
constexpr int kChunk = kThreads * kItems;       // differences per workgroup

__device__ __forceinline__ unsigned code_of(const unsigned char* __restrict__ lut, int64_t i) {
  return (lut[i >> 2] >> (2 * (i & 3))) & 3u;
}

// pass 1: bytes consumed by each chunk of kChunk differences (+ flag if a code 3 occurs)
__global__ void __launch_bounds__(kThreads)
xim_chunk_bytes_kernel(const unsigned char* __restrict__ lut, int64_t n_diffs, unsigned* __restrict__ chunk_bytes,
                       int* __restrict__ status) {
  __shared__ unsigned s_w[kThreads / PL_WAVE];
  const int64_t base = (int64_t)blockIdx.x * kChunk + (int64_t)threadIdx.x * kItems;
  unsigned sum = 0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int64_t i = base + k;
    if (i < n_diffs) {
      const unsigned c = code_of(lut, i);
      bad |= c == 3u;
      sum += 1u << c;
    }
  }
  if (bad) atomicOr(status, 1);
  sum = pl_wave_reduce(sum, [](unsigned a, unsigned b) { return a + b; });
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
    for (int q = 0; q < kThreads / PL_WAVE; ++q) t += s_w[q];
    chunk_bytes[blockIdx.x] = t;
  }
}

// pass 2: exclusive scan of the chunk totals (one workgroup; a few hundred to a few thousand chunks)
__global__ void __launch_bounds__(kThreads)
xim_scan_chunks_kernel(unsigned* __restrict__ chunk_bytes, int n_chunks) {
  __shared__ unsigned s_part[kThreads];
  const int per = (n_chunks + kThreads - 1) / kThreads;
  const int lo = threadIdx.x * per, hi = min(lo + per, n_chunks);
  unsigned sum = 0;
  for (int i = lo; i < hi; ++i) sum += chunk_bytes[i];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned run = 0;
    for (int q = 0; q < kThreads; ++q) { const unsigned v = s_part[q]; s_part[q] = run; run += v; }
  }
  __syncthreads();
  unsigned run = s_part[threadIdx.x];
  for (int i = lo; i < hi; ++i) { const unsigned v = chunk_bytes[i]; chunk_bytes[i] = run; run += v; }
}

// pass 3: every difference finds its byte offset and is read, sign-extended and stored in the array dtype;
// the first W + 1 pixels are plain int32
template <typename T>
__global__ void __launch_bounds__(kThreads)
xim_gather_kernel(const unsigned char* __restrict__ lut, const unsigned char* __restrict__ stream,
                  int64_t stream_bytes, int64_t n_diffs, int64_t n_plain, const unsigned* __restrict__ chunk_off,
                  T* __restrict__ a, int* __restrict__ status) {
  __shared__ unsigned s_w[kThreads / PL_WAVE];
  const int64_t base = (int64_t)blockIdx.x * kChunk + (int64_t)threadIdx.x * kItems;
  unsigned sizes[kItems], mine = 0;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int64_t i = base + k;
    sizes[k] = (i < n_diffs) ? (1u << (code_of(lut, i) & 3u)) : 0u;
    mine += sizes[k];
  }
  // exclusive scan of `mine` over the workgroup
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned inc = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  unsigned off = chunk_off[blockIdx.x] + (inc - mine);
  for (int q = 0; q < wv; ++q) off += s_w[q];
  const int64_t data0 = n_plain * 4;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int64_t i = base + k;
    if (i >= n_diffs) break;
    const unsigned sz = sizes[k];
    const int64_t p = data0 + off;
    if (sz > 4u || p + sz > stream_bytes) { atomicOr(status, sz > 4u ? 1 : 2); off += sz; continue; }
    unsigned v = 0;
    for (unsigned q = 0; q < sz; ++q) v |= (unsigned)stream[p + q] << (8 * q);
    int sv = sz == 1 ? (int)(signed char)v : (sz == 2 ? (int)(short)v : (int)v);
    a[n_plain + i] = (T)sv;
    off += sz;
  }
  // the uncompressed head (first row + first pixel of the second row): little-endian int32
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_plain; i += (int64_t)gridDim.x * kThreads) {
    const unsigned char* q = stream + i * 4;
    const unsigned v = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16) | ((unsigned)q[3] << 24);
    a[i] = (T)(int)v;
  }
}

// row-wise inclusive prefix sums of rows 1 .. H-1 (in place) + the row totals
template <typename T>
__global__ void __launch_bounds__(kThreads)
xim_row_scan_kernel(T* __restrict__ a, int w, unsigned long long* __restrict__ row_total) {
  __shared__ unsigned long long s_w[kThreads / PL_WAVE];
  const int r = blockIdx.x + 1;
  T* row = a + (size_t)r * w;
  const int per = (w + kThreads - 1) / kThreads;
  const int lo = threadIdx.x * per, hi = min(lo + per, w);
  unsigned long long sum = 0;
  for (int c = lo; c < hi; ++c) sum += (unsigned long long)(long long)row[c];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long inc = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  unsigned long long run = inc - sum;
  for (int q = 0; q < wv; ++q) run += s_w[q];
  for (int c = lo; c < hi; ++c) {
    run += (unsigned long long)(long long)row[c];
    row[c] = (T)(long long)run;
  }
  if (threadIdx.x == kThreads - 1) {
    unsigned long long t = 0;
    for (int q = 0; q < kThreads / PL_WAVE; ++q) t += s_w[q];
    row_total[r] = t;
  }
}

// c_1 = -P[0][0], c_r = c_{r-1} + total_{r-1}
template <typename T>
__global__ void xim_carry_kernel(const T* __restrict__ a, int h, unsigned long long* __restrict__ row_total) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  unsigned long long c = 0ull - (unsigned long long)(long long)a[0];
  for (int r = 1; r < h; ++r) {
    const unsigned long long t = row_total[r];
    row_total[r] = c;            // becomes c_r
    c += t;
  }
}

// P[r][c] = P[r-1][c] + S_r[c] + c_r
template <typename T>
__global__ void __launch_bounds__(kThreads)
xim_col_scan_kernel(T* __restrict__ a, int h, int w, const unsigned long long* __restrict__ carry) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= w) return;
  unsigned long long acc = (unsigned long long)(long long)a[c];
  for (int r = 1; r < h; ++r) {
    acc += (unsigned long long)(long long)a[(size_t)r * w + c] + carry[r];
    a[(size_t)r * w + c] = (T)(long long)acc;
  }
}

template <typename T>
int xim_decode_t(const unsigned char* lut, int64_t lut_bytes, const unsigned char* stream, int64_t stream_bytes, int w,
                 int h, T* out, unsigned char* work, hipStream_t st) {
  const int64_t n_plain = (int64_t)w + 1, n_diffs = (int64_t)w * h - w - 1;
  if (stream_bytes < n_plain * 4 || lut_bytes * 4 < n_diffs) { pl_set_error("pl_xim_decode: stream or lookup table too short"); return PL_ERR_INVALID_ARG; }
  const int n_chunks = (int)pl_cdiv(n_diffs > 0 ? n_diffs : 1, kChunk);
  int* status = reinterpret_cast<int*>(work);
  unsigned* chunk = reinterpret_cast<unsigned*>(work + 16);
  unsigned long long* row_total = reinterpret_cast<unsigned long long*>(work + 16 + (((size_t)n_chunks * 4 + 15) & ~(size_t)15));
  if (hipMemsetAsync(status, 0, 16, st) != hipSuccess) { pl_set_error("pl_xim_decode: memset failed"); return PL_ERR_HIP; }
  hipLaunchKernelGGL(xim_chunk_bytes_kernel, dim3(n_chunks), dim3(kThreads), 0, st, lut, n_diffs, chunk, status);
  hipLaunchKernelGGL(xim_scan_chunks_kernel, dim3(1), dim3(kThreads), 0, st, chunk, n_chunks);
  hipLaunchKernelGGL(xim_gather_kernel<T>, dim3(n_chunks), dim3(kThreads), 0, st, lut, stream, stream_bytes, n_diffs,
                     n_plain, chunk, out, status);
  if (h > 1) {
    hipLaunchKernelGGL(xim_row_scan_kernel<T>, dim3(h - 1), dim3(kThreads), 0, st, out, w, row_total);
    hipLaunchKernelGGL(xim_carry_kernel<T>, dim3(1), dim3(64), 0, st, out, h, row_total);
    hipLaunchKernelGGL(xim_col_scan_kernel<T>, dim3((unsigned)pl_cdiv(w, kThreads)), dim3(kThreads), 0, st, out, h, w,
                       row_total);
  }
  return pl_check_launch("pl_xim_decode");
}

// ---------------------------------------------------------------------------------------------------------------------
// The STACK form (pl_xim_decode_batch): N images of one (W, H, bytes_per_pixel) anywhere inside one device buffer (whole
// .xim files copied as they are), the image index in a grid dimension, no launch whose shape depends on N and nothing read
// back.  Passes 1-4 are the kernels above with per-image windows; the two steps that were serial per image are not:
//   * the carries c_r come from a workgroup-wide scan of the row totals (one workgroup per image);
//   * the column pass is split into bands of kBandRows rows: pass 6 sums S_r[c] + c_r over each band and column, pass 7
//     starts every (image, band, 256-column tile) workgroup at P[0][c] + the sums of the bands above it and walks its own
//     band only.  All of it in the ring of 64-bit unsigned sums truncated at the store: any association gives the same bits.
// Every byte a lane reads lies inside its image's [offset, offset + length) window, which pass 1 has checked against the
// buffer; an image whose windows fail that check is flagged (status bit 1) and touched by no later pass.
constexpr int kBandRows = 64;

struct XimWindow {
  const unsigned char* lut;
  const unsigned char* stream;
  int64_t stream_bytes;
  bool ok;
};

__device__ __forceinline__ XimWindow xim_window(const unsigned char* __restrict__ buffer, int64_t buffer_bytes,
                                                const int64_t* __restrict__ lut_off, const int64_t* __restrict__ lut_len,
                                                const int64_t* __restrict__ buf_off, const int64_t* __restrict__ buf_len,
                                                int64_t img, int64_t n_diffs, int64_t n_plain) {
  const int64_t lo = lut_off[img], ll = lut_len[img], bo = buf_off[img], bl = buf_len[img];
  XimWindow w;
  // (differences of lengths, never sums of an offset and a length: nothing here can overflow)
  w.ok = lo >= 0 && ll >= 0 && lo <= buffer_bytes && ll <= buffer_bytes - lo && ll >= (n_diffs + 3) / 4 &&
         bo >= 0 && bl >= 0 && bo <= buffer_bytes && bl <= buffer_bytes - bo && bl >= n_plain * 4;
  w.lut = buffer + lo;
  w.stream = buffer + bo;
  w.stream_bytes = bl;
  return w;
}

// exclusive prefix of `mine` over the kThreads lanes of a workgroup (every lane calls it; s_w: kThreads / PL_WAVE entries)
template <typename U>
__device__ __forceinline__ U xim_block_exclusive(U mine, U* s_w) {
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

// pass 1 (grid: chunks x images): window check + bytes consumed by each chunk + flag for a size code 3
__global__ void __launch_bounds__(kThreads)
ximb_chunk_bytes_kernel(const unsigned char* __restrict__ buffer, int64_t buffer_bytes, const int64_t* __restrict__ lut_off,
                        const int64_t* __restrict__ lut_len, const int64_t* __restrict__ buf_off,
                        const int64_t* __restrict__ buf_len, int64_t n_diffs, int64_t n_plain, int chunk_stride,
                        unsigned* __restrict__ chunk_bytes, int* __restrict__ status) {
  __shared__ unsigned s_w[kThreads / PL_WAVE];
  const int64_t img = blockIdx.y;
  const XimWindow win = xim_window(buffer, buffer_bytes, lut_off, lut_len, buf_off, buf_len, img, n_diffs, n_plain);
  if (!win.ok) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status + img, 2);
    return;
  }
  const int64_t base = (int64_t)blockIdx.x * kChunk + (int64_t)threadIdx.x * kItems;
  unsigned sum = 0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int64_t i = base + k;
    if (i < n_diffs) {
      const unsigned c = code_of(win.lut, i);
      bad |= c == 3u;
      sum += 1u << c;
    }
  }
  if (bad) atomicOr(status + img, 1);
  sum = pl_wave_reduce(sum, [](unsigned a, unsigned b) { return a + b; });
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
    for (int q = 0; q < kThreads / PL_WAVE; ++q) t += s_w[q];
    chunk_bytes[img * chunk_stride + blockIdx.x] = t;
  }
}

// pass 2 (grid: images): exclusive scan of an image's chunk totals; a lane takes ceil(n_chunks / kThreads) consecutive ones
__global__ void __launch_bounds__(kThreads)
ximb_scan_chunks_kernel(unsigned* __restrict__ chunk_bytes, int n_chunks, int chunk_stride, const int* __restrict__ status) {
  __shared__ unsigned s_w[kThreads / PL_WAVE];
  const int64_t img = blockIdx.x;
  if (status[img] & 2) return;                               // (uniform: the window check of pass 1)
  unsigned* chunk = chunk_bytes + img * chunk_stride;
  const int per = (n_chunks + kThreads - 1) / kThreads;
  const int lo = min((int)threadIdx.x * per, n_chunks), hi = min(lo + per, n_chunks);
  unsigned sum = 0;
  for (int i = lo; i < hi; ++i) sum += chunk[i];
  unsigned run = xim_block_exclusive(sum, s_w);
  for (int i = lo; i < hi; ++i) { const unsigned v = chunk[i]; chunk[i] = run; run += v; }
}

// pass 3 (grid: chunks x images): the gather of xim_gather_kernel into the image's T-typed plane
template <typename T>
__global__ void __launch_bounds__(kThreads)
ximb_gather_kernel(const unsigned char* __restrict__ buffer, int64_t buffer_bytes, const int64_t* __restrict__ lut_off,
                   const int64_t* __restrict__ lut_len, const int64_t* __restrict__ buf_off,
                   const int64_t* __restrict__ buf_len, int64_t n_diffs, int64_t n_plain, int chunk_stride,
                   const unsigned* __restrict__ chunk_off, T* __restrict__ plane, int* __restrict__ status) {
  __shared__ unsigned s_w[kThreads / PL_WAVE];
  const int64_t img = blockIdx.y;
  const XimWindow win = xim_window(buffer, buffer_bytes, lut_off, lut_len, buf_off, buf_len, img, n_diffs, n_plain);
  if (!win.ok) return;
  // bit 0 is final since pass 1.  With a code 3 the table implies no stream length: only bit 0 is reported then.
  const bool has3 = (status[img] & 1) != 0;
  T* a = plane + img * (n_plain + n_diffs);
  const int64_t base = (int64_t)blockIdx.x * kChunk + (int64_t)threadIdx.x * kItems;
  unsigned sizes[kItems], mine = 0;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int64_t i = base + k;
    sizes[k] = (i < n_diffs) ? (1u << (code_of(win.lut, i) & 3u)) : 0u;
    mine += sizes[k];
  }
  unsigned off = chunk_off[img * chunk_stride + blockIdx.x] + xim_block_exclusive(mine, s_w);
  const int64_t data0 = n_plain * 4;
  bool is_short = false;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int64_t i = base + k;
    if (i >= n_diffs) break;
    const unsigned sz = sizes[k];
    const int64_t p = data0 + off;
    off += sz;
    if (sz > 4u) continue;                                   // size code 3: flagged by pass 1
    if (p + sz > win.stream_bytes) { is_short = true; continue; }
    unsigned v = 0;
    for (unsigned q = 0; q < sz; ++q) v |= (unsigned)win.stream[p + q] << (8 * q);
    const int sv = sz == 1 ? (int)(signed char)v : (sz == 2 ? (int)(short)v : (int)v);
    a[n_plain + i] = (T)sv;
  }
  if (is_short && !has3) atomicOr(status + img, 2);
  // the uncompressed head (first row + first pixel of the second row): little-endian int32 at any alignment
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_plain; i += (int64_t)gridDim.x * kThreads) {
    const unsigned char* q = win.stream + i * 4;
    const unsigned v = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16) | ((unsigned)q[3] << 24);
    a[i] = (T)(int)v;
  }
}

// pass 4 (grid: rows 1 .. H-1 x images): xim_row_scan_kernel per image
template <typename T>
__global__ void __launch_bounds__(kThreads)
ximb_row_scan_kernel(T* __restrict__ plane, int w, int h, unsigned long long* __restrict__ row_total,
                     const int* __restrict__ status) {
  __shared__ unsigned long long s_w[kThreads / PL_WAVE];
  const int64_t img = blockIdx.y;
  if (status[img] & 2) return;      // (uniform, final since pass 3) a flagged window or a short stream: the frame is not finished
  const int r = blockIdx.x + 1;
  T* row = plane + (img * h + r) * w;
  const int per = (w + kThreads - 1) / kThreads;
  const int lo = min((int)threadIdx.x * per, w), hi = min(lo + per, w);
  unsigned long long sum = 0;
  for (int c = lo; c < hi; ++c) sum += (unsigned long long)(long long)row[c];
  unsigned long long run = xim_block_exclusive(sum, s_w);
  for (int c = lo; c < hi; ++c) {
    run += (unsigned long long)(long long)row[c];
    row[c] = (T)(long long)run;
  }
  if (threadIdx.x == kThreads - 1) row_total[img * h + r] = run;     // the last lane's inclusive sum = the row's total
}

// pass 5 (grid: images): c_1 = -P[0][0], c_r = c_{r-1} + total_{r-1} as a workgroup-wide exclusive scan of the totals
template <typename T>
__global__ void __launch_bounds__(kThreads)
ximb_carry_kernel(const T* __restrict__ plane, int w, int h, unsigned long long* __restrict__ row_total,
                  const int* __restrict__ status) {
  __shared__ unsigned long long s_w[kThreads / PL_WAVE];
  const int64_t img = blockIdx.x;
  if (status[img] & 2) return;
  unsigned long long* tot = row_total + img * h;
  const int rows = h - 1, per = (rows + kThreads - 1) / kThreads;
  const int lo = 1 + min((int)threadIdx.x * per, rows), hi = min(lo + per, h);
  unsigned long long sum = 0;
  for (int r = lo; r < hi; ++r) sum += tot[r];
  unsigned long long run = xim_block_exclusive(sum, s_w) - (unsigned long long)(long long)plane[img * h * w];
  for (int r = lo; r < hi; ++r) { const unsigned long long t = tot[r]; tot[r] = run; run += t; }
}

// pass 6 (grid: column tiles x bands but the last x images): band_sum[b][c] = sum over the band's rows of S_r[c] + c_r
template <typename T>
__global__ void __launch_bounds__(kThreads)
ximb_band_sum_kernel(const T* __restrict__ plane, int w, int h, int n_bands, const unsigned long long* __restrict__ carry,
                     unsigned long long* __restrict__ band_sum, const int* __restrict__ status) {
  const int64_t img = blockIdx.z;
  if (status[img] & 2) return;
  const int c = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
  if (c >= w) return;
  const int r0 = 1 + b * kBandRows, r1 = min(r0 + kBandRows, h);
  const T* col = plane + img * h * w + c;
  const unsigned long long* cr = carry + img * h;
  unsigned long long acc = 0;
#pragma unroll 8
  for (int r = r0; r < r1; ++r) acc += (unsigned long long)(long long)col[(int64_t)r * w] + cr[r];
  band_sum[(img * (n_bands - 1) + b) * w + c] = acc;
}

// the final store: KIND 0 the container type, 1 astype(uint16) (wrap-around; `wide` = a value outside 0 .. 65535 was seen),
// 2 astype(float64) (exact below 2^53, round-to-nearest-even beyond)
template <typename T, int KIND>
struct XimOut;
template <typename T>
struct XimOut<T, 0> { using type = T; };
template <typename T>
struct XimOut<T, 1> { using type = unsigned short; };
template <typename T>
struct XimOut<T, 2> { using type = double; };

template <typename T, int KIND>
__device__ __forceinline__ typename XimOut<T, KIND>::type xim_convert(T v, bool& wide) {
  if constexpr (KIND == 1) {
    wide |= (long long)v < 0 || (long long)v > 65535;
    return (unsigned short)v;
  } else if constexpr (KIND == 2) {
    return (double)(long long)v;
  } else {
    return v;
  }
}

// pass 7 (grid: column tiles x bands x images): P[r][c] = P[r-1][c] + S_r[c] + c_r inside the band, started from
// P[0][c] + the sums of the bands above; KIND 0 works in place (out == plane: a lane reads and writes its own column only)
template <typename T, int KIND>
__global__ void __launch_bounds__(kThreads)
ximb_col_scan_kernel(const T* plane, int w, int h, int n_bands, const unsigned long long* __restrict__ carry,
                     const unsigned long long* __restrict__ band_sum, typename XimOut<T, KIND>::type* out,
                     int* __restrict__ status) {
  constexpr int kStep = 8;
  const int64_t img = blockIdx.z;
  if (status[img] & 2) return;
  const int c = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
  if (c >= w) return;
  const int r0 = 1 + b * kBandRows, r1 = min(r0 + kBandRows, h);
  const T* col = plane + img * h * w + c;
  auto* ocol = out + img * h * w + c;
  const unsigned long long* cr = carry + img * h;
  const unsigned long long* bs = band_sum + img * (n_bands - 1) * w + c;
  bool wide = false;
  unsigned long long acc = (unsigned long long)(long long)col[0];
  if (KIND != 0 && b == 0) ocol[0] = xim_convert<T, KIND>(col[0], wide);          // row 0 is stored as it is
  for (int q = 0; q < b; ++q) acc += bs[(int64_t)q * w];
  for (int r = r0; r < r1; r += kStep) {
    unsigned long long v[kStep];
#pragma unroll
    for (int k = 0; k < kStep; ++k)
      v[k] = r + k < r1 ? (unsigned long long)(long long)col[(int64_t)(r + k) * w] + cr[r + k] : 0ull;
#pragma unroll
    for (int k = 0; k < kStep; ++k) {
      acc += v[k];
      if (r + k < r1) ocol[(int64_t)(r + k) * w] = xim_convert<T, KIND>((T)(long long)acc, wide);
    }
  }
  if (wide) atomicOr(status + img, 4);
}

template <typename T>
int xim_decode_batch_t(const unsigned char* buffer, int64_t buffer_bytes, const int64_t* lut_off, const int64_t* lut_len,
                       const int64_t* buf_off, const int64_t* buf_len, int n, int w, int h, int out_kind, void* out,
                       int* status, unsigned char* work, hipStream_t st) {
  const int64_t n_plain = (int64_t)w + 1, n_diffs = (int64_t)w * h - w - 1;
  const int n_chunks = (int)pl_cdiv(n_diffs > 0 ? n_diffs : 1, kChunk);
  const int chunk_stride = (n_chunks + 3) & ~3;
  const int n_bands = (int)pl_cdiv(h - 1, kBandRows);
  // d_work: chunk table | row totals -> carries | band sums | (out_kind != 0) the T-typed planes; every part 16-byte aligned
  unsigned* chunk = reinterpret_cast<unsigned*>(work);
  size_t at = (size_t)n * chunk_stride * 4;
  unsigned long long* row_total = reinterpret_cast<unsigned long long*>(work + at);
  at += (((size_t)n * h * 8) + 15) & ~(size_t)15;
  unsigned long long* band_sum = reinterpret_cast<unsigned long long*>(work + at);
  at += (((size_t)n * (n_bands - 1) * w * 8) + 15) & ~(size_t)15;
  T* plane = out_kind == 0 ? static_cast<T*>(out) : reinterpret_cast<T*>(work + at);
  if (hipMemsetAsync(status, 0, (size_t)n * 4, st) != hipSuccess) { pl_set_error("pl_xim_decode_batch: memset failed"); return PL_ERR_HIP; }
  const dim3 blk(kThreads);
  hipLaunchKernelGGL(ximb_chunk_bytes_kernel, dim3(n_chunks, n), blk, 0, st, buffer, buffer_bytes, lut_off, lut_len, buf_off,
                     buf_len, n_diffs, n_plain, chunk_stride, chunk, status);
  hipLaunchKernelGGL(ximb_scan_chunks_kernel, dim3(n), blk, 0, st, chunk, n_chunks, chunk_stride, status);
  hipLaunchKernelGGL(ximb_gather_kernel<T>, dim3(n_chunks, n), blk, 0, st, buffer, buffer_bytes, lut_off, lut_len, buf_off,
                     buf_len, n_diffs, n_plain, chunk_stride, chunk, plane, status);
  hipLaunchKernelGGL(ximb_row_scan_kernel<T>, dim3(h - 1, n), blk, 0, st, plane, w, h, row_total, status);
  hipLaunchKernelGGL(ximb_carry_kernel<T>, dim3(n), blk, 0, st, plane, w, h, row_total, status);
  const unsigned tiles = (unsigned)pl_cdiv(w, kThreads);
  if (n_bands > 1)
    hipLaunchKernelGGL(ximb_band_sum_kernel<T>, dim3(tiles, n_bands - 1, n), blk, 0, st, plane, w, h, n_bands, row_total,
                       band_sum, status);
  const dim3 grid(tiles, n_bands, n);
  if (out_kind == 0)
    hipLaunchKernelGGL((ximb_col_scan_kernel<T, 0>), grid, blk, 0, st, plane, w, h, n_bands, row_total, band_sum,
                       static_cast<T*>(out), status);
  else if (out_kind == 1)
    hipLaunchKernelGGL((ximb_col_scan_kernel<T, 1>), grid, blk, 0, st, plane, w, h, n_bands, row_total, band_sum,
                       static_cast<unsigned short*>(out), status);
  else
    hipLaunchKernelGGL((ximb_col_scan_kernel<T, 2>), grid, blk, 0, st, plane, w, h, n_bands, row_total, band_sum,
                       static_cast<double*>(out), status);
  return pl_check_launch("pl_xim_decode_batch");
}

}  // namespace

extern "C" int64_t pl_xim_batch_work_bytes(int n, int width, int height, int bytes_per_pixel, int out_kind) {
  if (n < 1 || width < 1 || height < 2 || out_kind < 0 || out_kind > 2) return -1;
  if (bytes_per_pixel != 1 && bytes_per_pixel != 2 && bytes_per_pixel != 4 && bytes_per_pixel != 8) return -1;
  const int64_t n_diffs = (int64_t)width * height - width - 1;
  const int64_t n_chunks = pl_cdiv(n_diffs > 0 ? n_diffs : 1, kChunk);
  const int64_t n_bands = pl_cdiv(height - 1, kBandRows);
  int64_t total = (int64_t)n * ((n_chunks + 3) & ~(int64_t)3) * 4;
  total += ((int64_t)n * height * 8 + 15) & ~(int64_t)15;
  total += ((int64_t)n * (n_bands - 1) * width * 8 + 15) & ~(int64_t)15;
  if (out_kind != 0) total += (int64_t)n * height * width * bytes_per_pixel;
  return total > 0 ? total : 16;
}

extern "C" int pl_xim_decode_batch(const unsigned char* d_buffer, int64_t buffer_bytes, const int64_t* d_lut_off,
                                   const int64_t* d_lut_len, const int64_t* d_buf_off, const int64_t* d_buf_len, int n,
                                   int width, int height, int bytes_per_pixel, int out_kind, void* d_out,
                                   int32_t* d_status, unsigned char* d_work, void* stream) {
  PL_REQUIRE(d_buffer && d_lut_off && d_lut_len && d_buf_off && d_buf_len && d_out && d_status && d_work, "null pointer");
  PL_REQUIRE(n >= 1 && n <= 65535, "1 <= n <= 65535");
  PL_REQUIRE(width > 0 && height >= 2, "bad shape (a one-row image has no lookup table: the reference raises IndexError)");
  PL_REQUIRE((int64_t)width * height <= ((int64_t)1 << 30) && height - 1 <= 65535 * kBandRows, "image too large");
  PL_REQUIRE(buffer_bytes >= 0, "bad buffer size");
  if (bytes_per_pixel != 1 && bytes_per_pixel != 2 && bytes_per_pixel != 4 && bytes_per_pixel != 8) {
    pl_set_error("pl_xim_decode_batch: unsupported bytes per pixel %d", bytes_per_pixel);   // the reference raises ValueError
    return PL_ERR_UNSUPPORTED;
  }
  PL_REQUIRE(out_kind >= 0 && out_kind <= 2, "out_kind: 0 container, 1 uint16, 2 float64");
  PL_REQUIRE(((uintptr_t)d_work & 15) == 0, "d_work must start on a 16-byte boundary");
  const int out_bytes = out_kind == 0 ? bytes_per_pixel : (out_kind == 1 ? 2 : 8);
  PL_REQUIRE(((uintptr_t)d_out & (uintptr_t)(out_bytes - 1)) == 0, "d_out must be aligned to its element size");
  hipStream_t st = (hipStream_t)stream;
#define XIMB_CALL(T)                                                                                                     \
  return xim_decode_batch_t<T>(d_buffer, buffer_bytes, d_lut_off, d_lut_len, d_buf_off, d_buf_len, n, width, height,      \
                               out_kind, d_out, d_status, d_work, st)
  switch (bytes_per_pixel) {
    case 1: XIMB_CALL(signed char);
    case 2: XIMB_CALL(short);
    case 4: XIMB_CALL(int);
    default: XIMB_CALL(long long);
  }
#undef XIMB_CALL
}

extern "C" int64_t pl_xim_work_bytes(int width, int height) {
  const int64_t n_diffs = (int64_t)width * height - width - 1;
  const int64_t n_chunks = pl_cdiv(n_diffs > 0 ? n_diffs : 1, kChunk);
  return 16 + ((n_chunks * 4 + 15) & ~(int64_t)15) + (int64_t)height * 8;
}

extern "C" int pl_xim_decode(const unsigned char* d_lookup, int64_t lookup_bytes, const unsigned char* d_stream,
                             int64_t stream_bytes, int width, int height, int bytes_per_pixel, void* d_out,
                             unsigned char* d_work, void* stream) {
  PL_REQUIRE(d_lookup && d_stream && d_out && d_work, "null pointer");
  PL_REQUIRE(width > 0 && height > 0, "bad shape");
  hipStream_t st = (hipStream_t)stream;
  switch (bytes_per_pixel) {
    case 1: return xim_decode_t<signed char>(d_lookup, lookup_bytes, d_stream, stream_bytes, width, height, (signed char*)d_out, d_work, st);
    case 2: return xim_decode_t<short>(d_lookup, lookup_bytes, d_stream, stream_bytes, width, height, (short*)d_out, d_work, st);
    case 4: return xim_decode_t<int>(d_lookup, lookup_bytes, d_stream, stream_bytes, width, height, (int*)d_out, d_work, st);
    case 8: return xim_decode_t<long long>(d_lookup, lookup_bytes, d_stream, stream_bytes, width, height, (long long*)d_out, d_work, st);
    default:
      pl_set_error("pl_xim_decode: unsupported bytes per pixel %d", bytes_per_pixel);   // the reference raises ValueError
      return PL_ERR_UNSUPPORTED;
  }
}
