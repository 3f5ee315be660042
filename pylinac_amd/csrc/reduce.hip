// Profile extraction: axis reductions of a frame.
//
// Replaces the ad-hoc numpy reductions the analyzers use in place of an Image.profile():
//   np.mean(image, axis)   pylinac/picketfence.py:747-750, pylinac/field_analysis.py:1094-1117
//   np.sum(array, axis)    pylinac/picketfence.py:1513-1514, pylinac/field_analysis.py:488-506
//   np.max(central, axis)  pylinac/starshot.py:216-217
// Integer frames are summed in int64 (exact; numpy's float64/uint64 accumulation of integers is
// exact as well, so any order agrees), float frames are accumulated in the frame's own precision,
// sequentially along axis 0 (numpy's order for a C-contiguous frame) and by a wave tree along
// axis 1 (numpy uses pairwise summation there: equal to ~1 ulp, not bitwise).
//
// pl_threshold_colsum_u16 fuses BaseImage.threshold (pylinac/core/image.py:797-800) with the
// axis-0 column sums of the thresholded frame: one read and one write of the frame, 16-byte
// accesses (4 independent loads in flight per lane), per-lane uint32 partial sums over a 128-row
// band, one uint64 atomic per column/band.
#include "pl_common.h"
#include "median3_rows.h"
#include "peaks_device.h"

namespace {

constexpr int kThreads = 256;

template <typename T> struct Acc { using type = long long; };
template <> struct Acc<float> { using type = float; };
template <> struct Acc<double> { using type = double; };
template <typename A> struct AccIsFloat { static constexpr bool value = false; };
template <> struct AccIsFloat<float> { static constexpr bool value = true; };
template <> struct AccIsFloat<double> { static constexpr bool value = true; };

template <typename T>
__device__ __forceinline__ double finish(typename Acc<T>::type acc, int op, int count) {
  using A = typename Acc<T>::type;
  if (op == PL_MEAN) {
    if constexpr (!AccIsFloat<A>::value) return (double)acc / (double)count;  // float64 mean of integers
    else return (double)(A)(acc / (A)count);                            // mean in the frame's precision
  }
  return (double)acc;
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
reduce_axis0_kernel(const T* __restrict__ in, int h, int w, int col_tiles, int op,
                    double* __restrict__ out) {
  using A = typename Acc<T>::type;
  const int ct = blockIdx.x % col_tiles;
  const size_t frame = blockIdx.x / col_tiles;
  const int c = ct * kThreads + threadIdx.x;
  if (c >= w) return;
  const T* p = in + frame * (size_t)h * w + c;
  if (op == PL_SUM || op == PL_MEAN) {
    A acc = 0;
    for (int r = 0; r < h; ++r) acc += (A)p[(size_t)r * w];
    out[frame * w + c] = finish<T>(acc, op, h);
  } else {
    T best = p[0];
    for (int r = 1; r < h; ++r) {
      T v = p[(size_t)r * w];
      best = (op == PL_MAX) ? (v > best ? v : best) : (v < best ? v : best);
    }
    out[frame * w + c] = (double)best;
  }
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
reduce_axis1_kernel(const T* __restrict__ in, int64_t rows_total, int w, int op,
                    double* __restrict__ out) {
  using A = typename Acc<T>::type;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kThreads / PL_WAVE) + (threadIdx.x >> 6);
  if (row >= rows_total) return;
  const T* p = in + row * (size_t)w;
  if (op == PL_SUM || op == PL_MEAN) {
    A acc = 0;
    for (int c = lane; c < w; c += PL_WAVE) acc += (A)p[c];
    acc = pl_wave_reduce(acc, [](A a, A b) { return a + b; });
    if (lane == 0) out[row] = finish<T>(acc, op, w);
  } else {
    T best = p[lane < w ? lane : 0];
    for (int c = lane; c < w; c += PL_WAVE) {
      T v = p[c];
      best = (op == PL_MAX) ? (v > best ? v : best) : (v < best ? v : best);
    }
    best = pl_wave_reduce(best, [op](T a, T b) { return (op == PL_MAX) ? (a > b ? a : b) : (a < b ? a : b); });
    if (lane == 0) out[row] = (double)best;
  }
}

// ------------------------------------------------------------- fused threshold + column sums
constexpr int kBandRows = 128;
constexpr int kTcThreads = 128;  // 128 lanes x 8 columns = 1024 columns per sweep
constexpr int kTcUnroll = 4;     // independent 16-byte loads in flight per lane

__global__ void __launch_bounds__(kTcThreads)
threshold_colsum_kernel(const unsigned short* __restrict__ in, unsigned short* __restrict__ out, int h,
                        int w, int bands, const int32_t* __restrict__ thr,
                        unsigned long long* __restrict__ colsum) {
  const unsigned id = pl_xcd_remap(blockIdx.x, gridDim.x);
  const int band = id % bands;
  const size_t frame = id / bands;
  const int t = thr[frame];
  const int r0 = band * kBandRows;
  const int r1 = (r0 + kBandRows < h) ? r0 + kBandRows : h;
  const unsigned short* f = in + frame * (size_t)h * w;
  unsigned short* o = out + frame * (size_t)h * w;
  unsigned long long* cs = colsum + frame * (size_t)w;
  const bool vec = ((w & 7) == 0) && ((reinterpret_cast<uintptr_t>(f) & 15) == 0) &&
                   ((reinterpret_cast<uintptr_t>(o) & 15) == 0);
  if (vec) {
    for (int c = threadIdx.x * 8; c < w; c += kTcThreads * 8) {
      unsigned s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      auto apply = [&](uint4 q) -> uint4 {
        union { uint4 q; unsigned short e[8]; } u;
        u.q = q;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const unsigned short v = ((int)u.e[k] >= t) ? u.e[k] : (unsigned short)0;
          u.e[k] = v;
          s[k] += v;
        }
        return u.q;
      };
      int r = r0;
      for (; r + kTcUnroll <= r1; r += kTcUnroll) {
        uint4 q[kTcUnroll];
#pragma unroll
        for (int k = 0; k < kTcUnroll; ++k) q[k] = *reinterpret_cast<const uint4*>(f + (size_t)(r + k) * w + c);
#pragma unroll
        for (int k = 0; k < kTcUnroll; ++k) *reinterpret_cast<uint4*>(o + (size_t)(r + k) * w + c) = apply(q[k]);
      }
      for (; r < r1; ++r)
        *reinterpret_cast<uint4*>(o + (size_t)r * w + c) = apply(*reinterpret_cast<const uint4*>(f + (size_t)r * w + c));
#pragma unroll
      for (int k = 0; k < 8; ++k) atomicAdd(cs + c + k, (unsigned long long)s[k]);
    }
  } else {
    for (int c = threadIdx.x; c < w; c += kTcThreads) {
      unsigned s = 0;
      for (int r = r0; r < r1; ++r) {
        unsigned short v = f[(size_t)r * w + c];
        v = ((int)v >= t) ? v : (unsigned short)0;
        o[(size_t)r * w + c] = v;
        s += v;
      }
      atomicAdd(cs + c, (unsigned long long)s);
    }
  }
}

// The same with the 3x3 MEDIAN of the frame as the thresholded quantity, computed on the fly (pl_median3_rows): the median
// plane is never written.  One workgroup = 4 waves = one block of 512 columns x one band of 128 rows; wave v walks row group v
// (32 rows) of the band; the four waves' column sums meet in LDS and leave as one 64-bit atomic per column.
constexpr int kMtRows = 32;                        // rows per wave: two halo rows are re-read per wave
constexpr int kMtWaves = kBandRows / kMtRows;      // 4
struct MtTile { size_t frame; int band, cg; };
// The walk whose loads are predicated by offset (CELLS): rows in flight per lane, and the waves per SIMD its kernel is compiled
// for (128 VGPRs, no scratch).  Measured on the bench frames and on a flood field at 4 / 6 / 8 rows and three / four waves
// (DESIGN.md 5.4): four rows at four waves is the fastest on the bench frames that does not slow the flood field.
constexpr int kMtAheadCells = 4;
constexpr int kMtWavesPerSimdCells = 4;

// The pixel work of one workgroup: thresholded medians stored, the four waves' column sums of the tile met in s_cs (complete
// and visible to every lane on return); -> which tile of which frame this workgroup had.
// CELLS: cellmax[frame][row group of 32][cell of 64 columns] >= the largest median of the cell (pl_median3_otsu16_cells; a
// wave's 32 x 512 tile is eight cells, a lane's cell is lane >> 3).  A cell whose maximum lies below the threshold is all zero
// whatever its medians are: `need` = the cell can hold a survivor.  A wave without a needed cell stores its zeros and reads
// nothing; otherwise a lane loads when it or a lane next to it needs (a block's first / last median takes a column from the
// neighbouring lane; the wave's outermost lanes fetch theirs from memory themselves, and every wave loads its own halo rows).
// What a lane stores is decided by `need` alone, never by a median computed next to a lane that did not load.
// KEEP (with CELLS): keep.zeroed[frame][row group][cell] (cellmax's geometry, one byte each) != 0 says that every pixel of the
// cell of `out` is 0 right now.  A cell that is not needed and whose entry is set is not stored again; one whose entry is clear
// is stored as zeros and its entry set; a needed cell is stored and its entry cleared (whatever its pixels turn out to be).  A
// wave without a needed cell and with every entry set issues no load and no store after the table look-ups.  keep.reset != 0:
// every entry reads as clear (everything is stored, the entries written are right) -- how a table starts.  The cell's first
// lane, which is in the frame whenever one of the cell is, reads and writes the entry (plain accesses: one wave per entry and
// launch, stream order carries it to the next launch); the other seven take the verdict from a ballot.
template <bool KEEP>
struct MtKeep {};
template <>
struct MtKeep<true> {
  unsigned char* zeroed;
  int reset;
};

template <bool CELLS, bool KEEP = false>
__device__ __forceinline__ MtTile median3_threshold_tile(const unsigned short* __restrict__ in, unsigned short* __restrict__ out,
                                                         int h, int w, int bands, int col_groups, const int32_t* __restrict__ thr,
                                                         unsigned* s_cs, const unsigned short* __restrict__ cellmax,
                                                         MtKeep<KEEP> keep = {}) {
  static_assert(CELLS || !KEEP, "the kept-zero table goes with the cell table");
  unsigned id = pl_xcd_remap(blockIdx.x, gridDim.x);
  const int cg = id % col_groups;
  id /= col_groups;
  const int band = id % bands;
  const size_t frame = id / bands;
  const int t = thr[frame];
  const int lane = threadIdx.x & (PL_WAVE - 1), wave = threadIdx.x / PL_WAVE;
  const int c0 = (cg * PL_WAVE + lane) * 8;
  const bool on = c0 < w;
  const int rg = band * kBandRows + kMtRows * wave;     // the wave's first row; rows beyond the frame produce nothing
  const unsigned short* f = in + frame * (size_t)h * w;
  unsigned short* o = out + frame * (size_t)h * w;
  for (int i = threadIdx.x; i < PL_WAVE * 8; i += kMtWaves * PL_WAVE) s_cs[i] = 0;
  __syncthreads();
  unsigned s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool need = true, load = true, store = on;         // KEEP: `store` = the lane's cell of `out` has to be written
  unsigned long long needed = ~0ull;                // the wave's lanes that need
  if (CELLS && rg < h) {
    const int cell_cols = (w + 63) / 64, row_groups = (h + kMtRows - 1) / kMtRows;
    // a lane beyond the frame looks up the wave's first cell (lane 0 is always in the frame): no look-up under a branch
    const size_t cell = (frame * row_groups + rg / kMtRows) * cell_cols + ((on ? c0 : cg * PL_WAVE * 8) >> 6);
    const int cmax = cellmax[cell];
    // KEEP: the entry is read next to the maximum, one wait for both; it counts in the cell's first lane and without `reset`
    [[maybe_unused]] int entry = 0;
    if constexpr (KEEP) entry = keep.zeroed[cell];
    // the same comparison as the pixel test m >= t: a cell whose maximum equals the threshold is needed
    need = on && cmax >= t;
    needed = __ballot(need);
    load = (((needed << 1) | needed | (needed >> 1)) >> lane) & 1ull;
    if constexpr (KEEP) {
      const bool head = on && (lane & 7) == 0;
      const bool was = head && !keep.reset && entry != 0;
      if (head && (keep.reset || was == need)) keep.zeroed[cell] = need ? 0 : 1;
      const unsigned long long kept = __ballot(was);          // bit 8 * cell: the cell's zeros are in `out` already
      store = on && (need || !((kept >> (lane & ~7)) & 1ull));
    }
  }
  if (rg < h && needed == 0ull) {                   // wave-uniform: nothing of this tile survives -- zeros, and zero column sums
    const int r1 = rg + kMtRows < h ? rg + kMtRows : h;
    if (KEEP ? store : on)
      for (int r = rg; r < r1; ++r) *reinterpret_cast<uint4*>(o + (size_t)r * w + c0) = uint4{0u, 0u, 0u, 0u};
  } else if (rg < h) {                              // wave-uniform
    if constexpr (CELLS) {
      // `load` and `store` are run-time predicates here: both by OFFSET, not by branch (pl_median3_rows, BYOFFSET) -- the row's
      // store is a buffer store on `out`'s frame that a lane which must not store aims beyond it, and nothing returns early, so
      // the walk's loop is one block whose outstanding loads the compiler counts.  A lane that does not need adds zeros to its
      // column sums (`need` implies `on`, a loading lane and loading neighbours), whatever it digested.
      const __amdgpu_buffer_rsrc_t os = pl_make_rsrc_bounded(o, (unsigned)h * (unsigned)w * 2u);
      const unsigned voff = store ? (unsigned)c0 * 2u : kPlBufferNowhere;
      pl_median3_rows<unsigned short, kMtRows, kMtAheadCells, true>(f, h, w, c0, lane, rg, [&](int r, const int (&m)[8]) {
        unsigned v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          v[k] = need && m[k] >= t ? (unsigned)m[k] : 0u;
          s[k] += v[k];
        }
        pl_buffer_store_u128(uint4{v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)}, os, voff,
                             (unsigned)r * (unsigned)w * 2u);
      }, load);
    } else {
      pl_median3_rows<unsigned short, kMtRows>(f, h, w, c0, lane, rg, [&](int r, const int (&m)[8]) {
        if (!on) return;
        unsigned v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          v[k] = m[k] >= t ? (unsigned)m[k] : 0u;
          s[k] += v[k];
        }
        *reinterpret_cast<uint4*>(o + (size_t)r * w + c0) =
            uint4{v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)};
      });
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) atomicAdd(&s_cs[lane * 8 + k], s[k]);     // 32 rows x 65535 per wave, 4 waves: < 2^32
  }
  __syncthreads();
  return MtTile{frame, band, cg};
}

// PARTS: the band's column sums are STORED as uint32 parts[frame][band][column] (128 rows x 65535 < 2^32) instead of added to
// colsum[frame][column] with 64-bit atomics -- no zeroed table, no atomics; pl_colparts_profile_fwxm adds the bands up.
template <bool PARTS>
__global__ void __launch_bounds__(kMtWaves * PL_WAVE)
median3_threshold_colsum_kernel(const unsigned short* __restrict__ in, unsigned short* __restrict__ out, int h, int w, int bands,
                                int col_groups, const int32_t* __restrict__ thr, unsigned long long* __restrict__ colsum,
                                uint32_t* __restrict__ parts) {
  __shared__ unsigned s_cs[PL_WAVE * 8];
  const MtTile t = median3_threshold_tile<false>(in, out, h, w, bands, col_groups, thr, s_cs, nullptr);
  if (PARTS) {
    uint32_t* ps = parts + (t.frame * (size_t)bands + t.band) * (size_t)w + (size_t)t.cg * PL_WAVE * 8;
    for (int i = threadIdx.x; i < PL_WAVE * 8; i += kMtWaves * PL_WAVE)
      if (t.cg * PL_WAVE * 8 + i < w) ps[i] = s_cs[i];
  } else {
    unsigned long long* cs = colsum + t.frame * (size_t)w + (size_t)t.cg * PL_WAVE * 8;
    for (int i = threadIdx.x; i < PL_WAVE * 8; i += kMtWaves * PL_WAVE)
      if (t.cg * PL_WAVE * 8 + i < w) atomicAdd(cs + i, (unsigned long long)s_cs[i]);
  }
}

// The same pass with the REST of the EPID step behind it, frame by frame, in the same launch: the workgroup that finishes a
// frame LAST turns the frame's column sums into the mean profile, searches its peak and writes the FWXM record and the record
// row (profile_fwxm_frame: what pl_colsum_to_mean -> pl_find_peaks -> pl_fwxm_record do), while the other workgroups are still
// thresholding later frames.  kMtWaves * PL_WAVE == kPkThreads: the search is written for exactly this workgroup.
//
// Hand-over of the column sums between workgroups (any XCD), no fences -- every access to the shared words is a device-scope
// atomic, as in otsu16_window_kernel's merge: ws[frame][0 .. w) takes the tiles' sums by RETURNING 64-bit adds whose values are
// consumed before the barrier, so every add of the workgroup has been performed when thread 0 takes the frame's arrival ticket
// ws[frame][w]; the workgroup whose ticket is the last of bands x col_groups reads each sum with an exchange that puts the zero
// back, and zeroes the ticket: the workspace is all zero again when the launch ends.
// CELLS: the pixel pass skips what the cell table proves to lie below the threshold (median3_threshold_tile).
// KEEP: and does not store again the zeros that `keep`'s table says are in `out` already.
// (a pack of nothing, or of the one MtKeep<true>: without it the kernel's arguments are what they were)
template <bool STAGE, bool CELLS, typename... KEEP>
__global__ void __launch_bounds__(kMtWaves * PL_WAVE) __attribute__((amdgpu_waves_per_eu(CELLS ? kMtWavesPerSimdCells : 1)))
median3_threshold_tail_kernel(const unsigned short* __restrict__ in, unsigned short* __restrict__ out, int h, int w, int bands,
                              int col_groups, const int32_t* __restrict__ thr, const unsigned short* __restrict__ cellmax,
                              unsigned long long* __restrict__ ws,
                              pl_peak_params prm, int cap, int maxc, double* __restrict__ profile, int32_t* __restrict__ d_count,
                              int32_t* __restrict__ d_idx, int32_t* __restrict__ d_lb, int32_t* __restrict__ d_rb,
                              double* __restrict__ d_props, int32_t* __restrict__ d_status, double* __restrict__ fwxm,
                              double* __restrict__ record, KEEP... keep) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
  __shared__ unsigned s_cs[PL_WAVE * 8];
  __shared__ Scan scan;
  __shared__ double s_red[2 * (kPkThreads / PL_WAVE)];
  __shared__ int s_cnt, s_last;
  static_assert(kMtWaves * PL_WAVE == kPkThreads, "the peak search is written for this workgroup size");
  const MtTile t = median3_threshold_tile<CELLS, sizeof...(KEEP) != 0>(in, out, h, w, bands, col_groups, thr, s_cs, cellmax, keep...);
  unsigned long long* cs = ws + t.frame * (size_t)(w + 1);
  unsigned* ticket = reinterpret_cast<unsigned*>(cs + w);
  unsigned seen = 0;
  for (int i = threadIdx.x; i < PL_WAVE * 8; i += kMtWaves * PL_WAVE) {
    const int col = t.cg * PL_WAVE * 8 + i;
    const unsigned c = s_cs[i];
    if (col < w && c) seen |= atomicAdd(cs + col, (unsigned long long)c) == ~0ull ? 1u : 0u;   // RETURNING: the wave waits for its adds
  }
  // (a column sum cannot reach 2^64 - 1: `seen` stays 0; it exists so that the returned values are consumed before the barrier)
  if (seen) s_last = 2;
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(ticket, 1u) == (unsigned)(bands * col_groups - 1) ? 1 : 0;
  __syncthreads();
  if (s_last == 0) return;                                 // not the last workgroup of this frame
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int64_t frame = (int64_t)t.frame;
  const PeakLds L{smem_all, &scan, s_red, &s_cnt};
  double* fw = fwxm + frame * 8;
  profile_fwxm_frame<STAGE>([&](int i) { return atomicExch(cs + i, 0ull); }, w, h, prm, cap, maxc, L, (int)threadIdx.x,
                            profile + frame * (int64_t)w, d_count + frame, d_idx + frame * cap, d_lb + frame * cap,
                            d_rb + frame * cap, d_props + frame * 6 * (int64_t)cap, d_status + frame, fw);
  if (threadIdx.x == 0) {                                  // the lane that wrote fw
    double* rec = record + frame * 9;
    rec[0] = (double)thr[frame];
#pragma unroll
    for (int k = 0; k < 8; ++k) rec[1 + k] = fw[k];
  }
}

__global__ void colsum_to_mean_kernel(const unsigned long long* __restrict__ cs, int64_t total, int h,
                                      double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) out[i] = (double)cs[i] / (double)h;  // np.mean of integers: float64 sum / count
}


// ------------------------------------------------------------- FieldAnalysis: centre sums and strips
// pl_field_center_sums: np.sum(frame, 0) and np.sum(frame, 1) of a 16-bit frame in one read.  A workgroup takes a band of
// kCsBand rows; wave w sums rows w, w + 4, ... of the band.  A row's sum is the wave's (int64, exact); a column's partial sum
// over the wave's rows stays in the wave's own LDS slice (int32: at most 64 rows of |v| <= 65535 per wave and band, lane-owned
// columns, no atomics), the four slices are added and one int64 atomic per column and band goes to d_cols.
constexpr int kCsBand = 256;
constexpr int kCsWaves = kThreads / PL_WAVE;

template <typename T>
__global__ void __launch_bounds__(kThreads)
field_center_sums_kernel(const T* __restrict__ in, int h, int w, int bands, unsigned long long* __restrict__ cols,
                         double* __restrict__ rows) {
  extern __shared__ int cs_lds[];                       // [kCsWaves][w]
  const int band = blockIdx.x % bands;
  const size_t frame = blockIdx.x / bands;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int* mine = cs_lds + (size_t)wave * w;
  for (int c = lane; c < w; c += PL_WAVE) mine[c] = 0;
  const int r0 = band * kCsBand, r1 = min(r0 + kCsBand, h);
  const T* f = in + frame * (size_t)h * w;
  for (int r = r0 + wave; r < r1; r += kCsWaves) {
    const T* p = f + (size_t)r * w;
    long long acc = 0;
    for (int c = lane; c < w; c += PL_WAVE) {
      const int v = (int)p[c];
      acc += v;
      mine[c] += v;
    }
    acc = pl_wave_reduce(acc, [](long long a, long long b) { return a + b; });
    if (lane == 0) rows[frame * h + r] = (double)acc;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < w; c += kThreads) {
    long long s = 0;
    for (int k = 0; k < kCsWaves; ++k) s += cs_lds[(size_t)k * w + c];
    atomicAdd(cols + frame * w + c, (unsigned long long)s);
  }
}

// _strip_edges (FieldAnalysis._get_horiz_values / _get_vert_values): lo = max(int(round(L * pos - L * width / 2)), 0),
// hi = min(int(round(L * pos + L * width / 2) + 1), L); python's round is half-to-even = rint.  A non-finite position
// (the centre search found no field) gives the empty strip [0, 0).
__device__ __forceinline__ void strip_edges(int length, double pos, double width, int& lo, int& hi) {
  const double a = (double)length * pos, b = (double)length * width / 2.0;
  const double l = rint(a - b), u = rint(a + b);
  if (!(l == l) || !(u == u) || fabs(l) > 1e9 || fabs(u) > 1e9) { lo = 0; hi = 0; return; }
  lo = max((int)l, 0);
  hi = min((int)u + 1, length);
  if (hi < lo) hi = lo;                                   // an empty slice, as python's a[lo:hi]
}

// pl_field_strips: per frame f with centre ratios pos[f] = (vert_ratio, horiz_ratio)
//   horiz[f] = np.mean(frame[bottom:top, :], 0)   [w]   (rows from horiz_ratio * h)
//   vert[f]  = np.mean(frame[:, left:right], 1)   [h]   (columns from vert_ratio * w)
// Blocks 0 .. col_tiles - 1 of a frame: one column per lane, rows summed in order (reduce_axis0_kernel's order); the
// remaining blocks: one row per wave, the strip's columns lane-strided and wave-reduced (reduce_axis1_kernel's order on
// the sliced copy).  Only the strip's rows and columns are read.  Block 0 writes edges[f] = bottom, top, left, right.
template <typename T>
__global__ void __launch_bounds__(kThreads)
field_strips_kernel(const T* __restrict__ in, int h, int w, const double* __restrict__ pos, double vwidth, double hwidth,
                    int col_tiles, int row_groups, double* __restrict__ horiz, double* __restrict__ vert,
                    int32_t* __restrict__ edges) {
  using A = typename Acc<T>::type;
  const int per_frame = col_tiles + row_groups;
  const size_t frame = blockIdx.x / per_frame;
  const int part = blockIdx.x % per_frame;
  const T* f = in + frame * (size_t)h * w;
  int bottom, top, left, right;
  strip_edges(h, pos[2 * frame + 1], hwidth, bottom, top);
  strip_edges(w, pos[2 * frame], vwidth, left, right);
  if (part == 0 && threadIdx.x == 0) {
    int32_t* e = edges + frame * 4;
    e[0] = bottom; e[1] = top; e[2] = left; e[3] = right;
  }
  if (part < col_tiles) {
    const int c = part * kThreads + threadIdx.x;
    if (c >= w) return;
    A acc = 0;
    for (int r = bottom; r < top; ++r) acc += (A)f[(size_t)r * w + c];
    horiz[frame * w + c] = finish<T>(acc, PL_MEAN, top - bottom);
  } else {
    const int r = (part - col_tiles) * (kThreads / PL_WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= h) return;
    const T* p = f + (size_t)r * w + left;
    const int n = right - left;
    A acc = 0;
    for (int c = lane; c < n; c += PL_WAVE) acc += (A)p[c];
    acc = pl_wave_reduce(acc, [](A a, A b) { return a + b; });
    if (lane == 0) vert[frame * h + r] = finish<T>(acc, PL_MEAN, n);
  }
}

}  // namespace

extern "C" int pl_colsum_to_mean(const unsigned long long* d_colsum, int64_t n, int w, int h,
                                 double* d_out, void* stream) {
  PL_REQUIRE(d_colsum && d_out, "null pointer");
  PL_REQUIRE(n >= 0 && w > 0 && h > 0, "bad shape");
  if (n == 0) return PL_OK;
  const int64_t total = n * w;
  hipLaunchKernelGGL(colsum_to_mean_kernel, dim3((unsigned)pl_cdiv(total, 256)), dim3(256), 0,
                     (hipStream_t)stream, d_colsum, total, h, d_out);
  return pl_check_launch("pl_colsum_to_mean");
}

extern "C" int pl_reduce_axis(const void* in, int dtype, int64_t n, int h, int w, int axis, int op,
                              double* d_out, void* stream) {
  PL_REQUIRE(in && d_out, "null pointer");
  PL_REQUIRE(n >= 0 && h > 0 && w > 0, "bad shape");
  PL_REQUIRE(axis == 0 || axis == 1, "axis must be 0 or 1");
  PL_REQUIRE(op >= PL_SUM && op <= PL_MIN, "bad op");
  if (n == 0) return PL_OK;
  hipStream_t st = (hipStream_t)stream;
  if (axis == 0) {
    int col_tiles = (int)pl_cdiv(w, kThreads);
    PL_REQUIRE(n * col_tiles <= 0x7fffffffLL, "batch too large");
    PL_DISPATCH_DTYPE(dtype, T,
                      hipLaunchKernelGGL(reduce_axis0_kernel<T>, dim3((unsigned)(n * col_tiles)),
                                         dim3(kThreads), 0, st, (const T*)in, h, w, col_tiles, op, d_out));
  } else {
    int64_t rows = n * h;
    int64_t blocks = pl_cdiv(rows, kThreads / PL_WAVE);
    PL_REQUIRE(blocks <= 0x7fffffffLL, "batch too large");
    PL_DISPATCH_DTYPE(dtype, T,
                      hipLaunchKernelGGL(reduce_axis1_kernel<T>, dim3((unsigned)blocks), dim3(kThreads), 0,
                                         st, (const T*)in, rows, w, op, d_out));
  }
  return pl_check_launch("pl_reduce_axis");
}

extern "C" int pl_threshold_colsum_u16(const uint16_t* in, uint16_t* out, int64_t n, int h, int w,
                                       const int32_t* d_thr, unsigned long long* d_colsum,
                                       void* stream) {
  PL_REQUIRE(in && out && d_thr && d_colsum, "null pointer");
  PL_REQUIRE(n >= 0 && h > 0 && w > 0, "bad shape");
  if (n == 0) return PL_OK;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(d_colsum, 0, (size_t)n * w * sizeof(unsigned long long), st);
  if (e != hipSuccess) { pl_set_error("pl_threshold_colsum_u16: memset: %s", hipGetErrorString(e)); return PL_ERR_HIP; }
  int bands = (int)pl_cdiv(h, kBandRows);
  PL_REQUIRE(n * bands <= 0x7fffffffLL, "batch too large");
  hipLaunchKernelGGL(threshold_colsum_kernel, dim3((unsigned)(n * bands)), dim3(kTcThreads), 0, st, in, out,
                     h, w, bands, d_thr, d_colsum);
  return pl_check_launch("pl_threshold_colsum_u16");
}

extern "C" int pl_median3_threshold_colsum_u16(const uint16_t* in, uint16_t* out, int64_t n, int h, int w,
                                               const int32_t* d_thr, unsigned long long* d_colsum, void* stream) {
  PL_REQUIRE(in && out && d_thr && d_colsum && in != out, "null or aliased pointers");
  PL_REQUIRE(n >= 0 && h > 0 && w > 0, "bad shape");
  PL_REQUIRE(pl_median3_rows_covers(in, h, w) && (reinterpret_cast<uintptr_t>(out) & 15) == 0,
             "needs h > 1, width % 8 == 0 and 16-byte aligned frames (run pl_median2d + pl_threshold_colsum_u16 otherwise)");
  if (n == 0) return PL_OK;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(d_colsum, 0, (size_t)n * w * sizeof(unsigned long long), st);
  if (e != hipSuccess) { pl_set_error("pl_median3_threshold_colsum_u16: memset: %s", hipGetErrorString(e)); return PL_ERR_HIP; }
  const int bands = (int)pl_cdiv(h, kBandRows), col_groups = (int)pl_cdiv(w / 8, PL_WAVE);
  PL_REQUIRE(n * bands * col_groups <= 0x7fffffffLL, "batch too large");
  hipLaunchKernelGGL(median3_threshold_colsum_kernel<false>, dim3((unsigned)(n * bands * col_groups)), dim3(kMtWaves * PL_WAVE), 0, st,
                     in, out, h, w, bands, col_groups, d_thr, d_colsum, (uint32_t*)nullptr);
  return pl_check_launch("pl_median3_threshold_colsum_u16");
}

// rows per band of pl_median3_threshold_colparts_u16's partial sums: bands = ceil(h / pl_colparts_band_rows())
extern "C" int pl_colparts_band_rows(void) { return kBandRows; }

// The same pass with the column sums left as per-band partial sums d_parts uint32[n][bands][w] (plain stores: nothing to zero,
// no atomics); pl_colparts_profile_fwxm (peaks.hip) turns them into the mean profile and its FWXM record.
extern "C" int pl_median3_threshold_colparts_u16(const uint16_t* in, uint16_t* out, int64_t n, int h, int w,
                                                 const int32_t* d_thr, uint32_t* d_parts, void* stream) {
  PL_REQUIRE(in && out && d_thr && d_parts && in != out, "null or aliased pointers");
  PL_REQUIRE(n >= 0 && h > 0 && w > 0, "bad shape");
  PL_REQUIRE(pl_median3_rows_covers(in, h, w) && (reinterpret_cast<uintptr_t>(out) & 15) == 0,
             "needs h > 1, width % 8 == 0 and 16-byte aligned frames (run pl_median2d + pl_threshold_colsum_u16 otherwise)");
  if (n == 0) return PL_OK;
  const int bands = (int)pl_cdiv(h, kBandRows), col_groups = (int)pl_cdiv(w / 8, PL_WAVE);
  PL_REQUIRE(n * bands * col_groups <= 0x7fffffffLL, "batch too large");
  hipLaunchKernelGGL(median3_threshold_colsum_kernel<true>, dim3((unsigned)(n * bands * col_groups)), dim3(kMtWaves * PL_WAVE), 0,
                     (hipStream_t)stream, in, out, h, w, bands, col_groups, d_thr, (unsigned long long*)nullptr, d_parts);
  return pl_check_launch("pl_median3_threshold_colparts_u16");
}

// smallest dynamic LDS of median3_threshold_tail_kernel's peak search that keeps the pass's three workgroups per CU (133 VGPRs:
// three waves per SIMD; 3 x (48 KiB + 2.4 KiB of static LDS) < 160 KiB): the region staged in LDS if that fits, the candidate
// tables alone otherwise; 0 = neither fits (regions beyond 3 000 samples).  (The CELLS instantiations are compiled for four
// waves per SIMD; their fourth workgroup per CU fits where this is at most ~37 KiB, three run otherwise.)
static size_t step_tail_lds(const pl_peak_params* params, int w, bool* stage_x, int* maxc) {
  const int lo = params->region_lo < 0 ? 0 : params->region_lo;
  const int hi = params->region_hi > w ? w : params->region_hi;
  const int m = hi > lo ? hi - lo : 0;
  constexpr size_t kMax = 48 * 1024;
  *stage_x = true;
  size_t lds = peak_search_lds(m, true, maxc);
  if (lds <= kMax) return lds;
  *stage_x = false;
  lds = peak_search_lds(m, false, maxc);
  return lds <= kMax ? lds : 0;
}

// 1: pl_median3_threshold_profile_fwxm_u16 takes frames of this shape with these search parameters (16-byte aligned planes
// assumed); 0: run pl_median3_threshold_colsum_u16 / pl_median2d + pl_threshold_colsum_u16 and the separate tail launches
extern "C" int pl_median3_threshold_profile_fwxm_covers(int h, int w, const pl_peak_params* params) {
  bool stage_x;
  int maxc;
  return params && pl_median3_rows_covers(nullptr, h, w) && pl_median3_rows_bounded_covers(h, w) && step_tail_lds(params, w, &stage_x, &maxc) != 0 ? 1 : 0;
}

namespace {
template <bool CELLS, bool KEEP = false>
int step_tail_launch(const char* who, const uint16_t* in, uint16_t* out, int64_t n, int h, int w, const int32_t* d_thr,
                     const uint16_t* d_cellmax, const pl_peak_params* params, int cap, double* d_profile, int32_t* d_count,
                     int32_t* d_idx, int32_t* d_left_base, int32_t* d_right_base, double* d_props, int32_t* d_status,
                     double* d_fwxm, double* d_record, unsigned long long* d_ws, void* stream, MtKeep<KEEP> keep = {}) {
  auto bad = [&](const char* msg) {
    pl_set_error("%s: %s", who, msg);
    return PL_ERR_INVALID_ARG;
  };
  if (!(in && out && d_thr && in != out)) return bad("null or aliased pointers");
  if (!(params && d_profile && d_count && d_idx && d_left_base && d_right_base && d_props && d_status && d_fwxm && d_record && d_ws &&
        (d_cellmax || !CELLS)))
    return bad("null pointer");
  if constexpr (KEEP)
    if (!keep.zeroed) return bad("null pointer");
  if (!(n >= 0 && h > 0 && w > 0 && cap > 0)) return bad("bad shape");
  if (params->distance < 1) return bad("distance must be >= 1");
  if (!(pl_median3_rows_covers(in, h, w) && (reinterpret_cast<uintptr_t>(out) & 15) == 0))
    return bad("needs h > 1, width % 8 == 0 and 16-byte aligned frames (run the separate launches otherwise)");
  if (CELLS && !pl_median3_rows_bounded_covers(h, w)) return bad("frames of 2^31 bytes or more (run the separate launches)");
  bool stage_x;
  int maxc;
  const size_t lds = step_tail_lds(params, w, &stage_x, &maxc);
  if (lds == 0) return bad("search region too long for the one-launch form (run the separate launches)");
  if (n == 0) return PL_OK;
  const int bands = (int)pl_cdiv(h, kBandRows), col_groups = (int)pl_cdiv(w / 8, PL_WAVE);
  if (n * bands * col_groups > 0x7fffffffLL) return bad("batch too large");
  const dim3 grid((unsigned)(n * bands * col_groups)), block(kMtWaves * PL_WAVE);
  if constexpr (KEEP) {
    if (stage_x)
      hipLaunchKernelGGL((median3_threshold_tail_kernel<true, CELLS, MtKeep<true>>), grid, block, lds, (hipStream_t)stream, in, out, h,
                         w, bands, col_groups, d_thr, d_cellmax, d_ws, *params, cap, maxc, d_profile, d_count, d_idx, d_left_base,
                         d_right_base, d_props, d_status, d_fwxm, d_record, keep);
    else
      hipLaunchKernelGGL((median3_threshold_tail_kernel<false, CELLS, MtKeep<true>>), grid, block, lds, (hipStream_t)stream, in, out,
                         h, w, bands, col_groups, d_thr, d_cellmax, d_ws, *params, cap, maxc, d_profile, d_count, d_idx, d_left_base,
                         d_right_base, d_props, d_status, d_fwxm, d_record, keep);
  } else if (stage_x)
    hipLaunchKernelGGL((median3_threshold_tail_kernel<true, CELLS>), grid, block, lds, (hipStream_t)stream, in, out, h, w, bands,
                       col_groups, d_thr, d_cellmax, d_ws, *params, cap, maxc, d_profile, d_count, d_idx, d_left_base, d_right_base,
                       d_props, d_status, d_fwxm, d_record);
  else
    hipLaunchKernelGGL((median3_threshold_tail_kernel<false, CELLS>), grid, block, lds, (hipStream_t)stream, in, out, h, w, bands,
                       col_groups, d_thr, d_cellmax, d_ws, *params, cap, maxc, d_profile, d_count, d_idx, d_left_base, d_right_base,
                       d_props, d_status, d_fwxm, d_record);
  return pl_check_launch(who);
}
}  // namespace

// median -> threshold -> column sums -> mean profile -> peaks -> FWXM record -> record row in ONE launch: see
// median3_threshold_tail_kernel.  d_ws uint64[n][w + 1] must be ALL ZERO on entry and is all zero again when the launch has
// run (zero it once, when it is allocated; nothing else may touch it while a launch is in flight): per frame w column sums and
// the arrival ticket.
extern "C" int pl_median3_threshold_profile_fwxm_u16(const uint16_t* in, uint16_t* out, int64_t n, int h, int w, const int32_t* d_thr,
                                                     const pl_peak_params* params, int cap, double* d_profile, int32_t* d_count,
                                                     int32_t* d_idx, int32_t* d_left_base, int32_t* d_right_base, double* d_props,
                                                     int32_t* d_status, double* d_fwxm, double* d_record,
                                                     unsigned long long* d_ws, void* stream) {
  return step_tail_launch<false>(__func__, in, out, n, h, w, d_thr, nullptr, params, cap, d_profile, d_count, d_idx, d_left_base,
                                 d_right_base, d_props, d_status, d_fwxm, d_record, d_ws, stream);
}

// The same launch with pl_median3_otsu16_cells' table of the SAME plane: d_cellmax uint16 [n][ceil(h / 32)][ceil(w / 64)], every
// entry >= the largest 3x3 median of its cell (65535 = never skip).  Same results, bit for bit, every output pixel stored;
// cells whose maximum lies below the frame's threshold are not read.
extern "C" int pl_median3_threshold_profile_fwxm_cells_u16(const uint16_t* in, uint16_t* out, int64_t n, int h, int w,
                                                           const int32_t* d_thr, const uint16_t* d_cellmax,
                                                           const pl_peak_params* params, int cap, double* d_profile,
                                                           int32_t* d_count, int32_t* d_idx, int32_t* d_left_base,
                                                           int32_t* d_right_base, double* d_props, int32_t* d_status,
                                                           double* d_fwxm, double* d_record, unsigned long long* d_ws,
                                                           void* stream) {
  return step_tail_launch<true>(__func__, in, out, n, h, w, d_thr, d_cellmax, params, cap, d_profile, d_count, d_idx, d_left_base,
                                d_right_base, d_props, d_status, d_fwxm, d_record, d_ws, stream);
}

// The cells launch on an `out` whose zeros are remembered: d_zeroed uint8 [n][ceil(h / 32)][ceil(w / 64)] != 0 = the cell of
// `out` is all zero; such a cell is not stored again while it stays below the threshold.  reset != 0: the table is not read
// (everything is stored, correct entries are written).  Every output as pl_median3_threshold_profile_fwxm_cells_u16.
extern "C" int pl_median3_threshold_profile_fwxm_cells_keep_u16(const uint16_t* in, uint16_t* out, int64_t n, int h, int w,
                                                                const int32_t* d_thr, const uint16_t* d_cellmax,
                                                                uint8_t* d_zeroed, int reset, const pl_peak_params* params,
                                                                int cap, double* d_profile, int32_t* d_count, int32_t* d_idx,
                                                                int32_t* d_left_base, int32_t* d_right_base, double* d_props,
                                                                int32_t* d_status, double* d_fwxm, double* d_record,
                                                                unsigned long long* d_ws, void* stream) {
  return step_tail_launch<true, true>(__func__, in, out, n, h, w, d_thr, d_cellmax, params, cap, d_profile, d_count, d_idx,
                                      d_left_base, d_right_base, d_props, d_status, d_fwxm, d_record, d_ws, stream,
                                      MtKeep<true>{d_zeroed, reset});
}

extern "C" int pl_field_center_sums(const void* in, int dtype, int64_t n, int h, int w, unsigned long long* d_cols,
                                    double* d_rows, void* stream) {
  PL_REQUIRE(in && d_cols && d_rows, "null pointer");
  PL_REQUIRE(n >= 0 && h > 0 && w > 0, "bad shape");
  PL_REQUIRE(dtype == PL_U16 || dtype == PL_I16, "pl_field_center_sums takes uint16 / int16 frames");
  PL_REQUIRE((int64_t)w * kCsWaves * 4 <= 65536, "frame wider than 4096 columns");
  if (n == 0) return PL_OK;
  const int bands = (int)pl_cdiv(h, kCsBand);
  PL_REQUIRE(n * bands <= 0x7fffffffLL, "batch too large");
  hipStream_t st = (hipStream_t)stream;
  PL_REQUIRE(hipMemsetAsync(d_cols, 0, (size_t)n * w * sizeof(unsigned long long), st) == hipSuccess, "memset failed");
  const size_t lds = (size_t)w * kCsWaves * sizeof(int);
  if (dtype == PL_U16)
    hipLaunchKernelGGL(field_center_sums_kernel<unsigned short>, dim3((unsigned)(n * bands)), dim3(kThreads), lds, st,
                       (const unsigned short*)in, h, w, bands, d_cols, d_rows);
  else
    hipLaunchKernelGGL(field_center_sums_kernel<short>, dim3((unsigned)(n * bands)), dim3(kThreads), lds, st,
                       (const short*)in, h, w, bands, d_cols, d_rows);
  return pl_check_launch("pl_field_center_sums");
}

extern "C" int pl_field_strips(const void* in, int dtype, int64_t n, int h, int w, const double* d_pos, double vert_width,
                               double horiz_width, double* d_horiz, double* d_vert, int32_t* d_edges, void* stream) {
  PL_REQUIRE(in && d_pos && d_horiz && d_vert && d_edges, "null pointer");
  PL_REQUIRE(n >= 0 && h > 0 && w > 0, "bad shape");
  PL_REQUIRE(dtype == PL_U16 || dtype == PL_I16 || dtype == PL_F64, "pl_field_strips takes uint16 / int16 / float64 frames");
  if (n == 0) return PL_OK;
  const int col_tiles = (int)pl_cdiv(w, kThreads), row_groups = (int)pl_cdiv(h, kThreads / PL_WAVE);
  PL_REQUIRE(n * (col_tiles + row_groups) <= 0x7fffffffLL, "batch too large");
  PL_DISPATCH_DTYPE(dtype, T,
                    hipLaunchKernelGGL(field_strips_kernel<T>, dim3((unsigned)(n * (col_tiles + row_groups))), dim3(kThreads),
                                       0, (hipStream_t)stream, (const T*)in, h, w, d_pos, vert_width, horiz_width, col_tiles,
                                       row_groups, d_horiz, d_vert, d_edges));
  return pl_check_launch("pl_field_strips");
}
