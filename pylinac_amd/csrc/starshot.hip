// Starshot wobble fit for a table of datasets (pylinac/starshot.py:306-401 behind the star profile): the radiation lines of
// LineManager, its "lines pass the focus" test, the smallest circle touching every line by a REPLAY of
// scipy.optimize.minimize(method="Nelder-Mead", options={"fatol": 0.001}) and the accept test of the retry sweep.
//
//   pl_starshot_roll     StarProfile.get_peaks' first step for a table of rings: roll every ring to its FIRST minimum.
//   pl_starshot_peaks    its last steps: the peak search with a height per ring (the reference hands find_peaks
//                        min_peak_height * local_max of the frame), the FWHM centre index, and the peaks' image coordinates.
//   pl_starshot_wobble   one lane per dataset, 64 datasets per wave (a workgroup is one wave).
//
// Between roll and peaks the rings go through the library's own batched Gaussian and ground launches: no launch is per ring.
//
// The reference's optimiser stops where its comparisons tell it to, so the replay reproduces scipy's float64 sequence
// operation for operation (the library is built with -ffp-contract=off): three parameters (x, y and a z the objective
// ignores but the simplex carries), default coefficients rho 1, chi 2, psi 0.5, sigma 0.5, xatol 1e-4, fatol 1e-3, 600
// iterations / 600 evaluations.  scipy sorts the four vertices with np.argsort, an insertion sort at this size: stable,
// lowest index first (the start simplex always holds one exact tie: the vertex displaced in z has x0's value).
//
// The loop is serial and latency-bound.  A lane keeps its simplex in registers and its lines in its own column of an LDS
// table laid out [line][component][lane] (consecutive lanes read consecutive float64: conflict-free, no lane reads another's
// column, so the kernel has no barrier).  Lanes of a wave take different branches of an iteration; the second trial point of
// an iteration (expansion, outside or inside contraction) is ONE evaluation site with per-lane coefficients: c1 * xbar + c2 *
// worst with c2 = -2, -0.5 or +0.5 (a - b * w and a + (-b) * w are the same float64).
#include <math.h>

#include "pl_common.h"
#include "peaks_device.h"

namespace {

constexpr int kSsMaxLines = 32;
constexpr int kSsMaxIter = 600, kSsMaxFun = 600;      // N * 200, N = 3

// np.max / np.min of two values: a NaN wins
__device__ __forceinline__ double ss_npmax(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double ss_npmin(double a, double b) { return (a < b || a != a) ? a : b; }
// numpy's sort order: a NaN is larger than everything
__device__ __forceinline__ bool ss_lt(double a, double b) { return a < b || (b != b && a == a); }

// Line.distance_to (pylinac/core/geometry.py:565-584) of the line lp1 -> lp1 + a to (px, py, 0); every z is 0:
// |cross(lp2 - lp1, lp1 - pt)| / |lp2 - lp1| with numpy's cross (multiply, multiply, subtract per component) and np.sum of
// three squares, left to right
__device__ __forceinline__ double ss_distance(double p1x, double p1y, double a0, double a1, double px, double py) {
  const double a2 = 0.0, b0 = p1x - px, b1 = p1y - py, b2 = 0.0;
  const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
  const double num = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
  const double den = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
  return num / den;
}

struct SsVertex {
  double x, y, z, f;
};

__device__ __forceinline__ void ss_order(SsVertex& lo, SsVertex& hi) {       // one step of the stable insertion sort
  if (ss_lt(hi.f, lo.f)) { const SsVertex t = lo; lo = hi; hi = t; }
}
__device__ __forceinline__ void ss_sort(SsVertex& s0, SsVertex& s1, SsVertex& s2, SsVertex& s3) {
  ss_order(s0, s1);
  ss_order(s1, s2); ss_order(s0, s1);
  ss_order(s2, s3); ss_order(s1, s2); ss_order(s0, s1);
}

__global__ void __launch_bounds__(PL_WAVE)
ss_wobble_kernel(const double* __restrict__ points, const int32_t* __restrict__ count, const double* __restrict__ focus, int m,
                 int cap, double dpmm, double max_wobble_diameter, double tolerance, int recursive, double* __restrict__ record,
                 double* __restrict__ lines, int32_t* __restrict__ status) {
  __shared__ double s_line[kSsMaxLines * 4 * PL_WAVE];               // [line][p1x, p1y, a0, a1][lane]
  const int lane = threadIdx.x;
  const int row = blockIdx.x * PL_WAVE + lane;
  if (row >= m) return;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  const int half_cap = cap >> 1;
  const int n = count[row];
  const double* pts = points + (size_t)row * cap * 2;
  double* ln_out = lines + (size_t)row * half_cap * 4;
  double* rec = record + (size_t)row * 9;
  const double fx = focus[row * 2], fy = focus[row * 2 + 1];
  const double limit = 10.0 * dpmm;

  int st = 0;
  if (n > cap) st = 4;
  else if (n < 6 || (n & 1)) st = 1;
  const int nl = st == 0 ? n >> 1 : 0;                                // int(len(points) / 2)
  // LineManager: line k joins peaks[k] and peaks[k + nl]; ValueError when one lies farther than 10 * dpmm from the focus
  for (int k = 0; k < half_cap; ++k) {
    double p1x = qnan, p1y = qnan, p2x = qnan, p2y = qnan;
    if (k < nl) {
      p1x = pts[2 * k]; p1y = pts[2 * k + 1];
      p2x = pts[2 * (k + nl)]; p2y = pts[2 * (k + nl) + 1];
      const double a0 = p2x - p1x, a1 = p2y - p1y;
      double* s = s_line + (k * 4) * PL_WAVE + lane;
      s[0] = p1x; s[PL_WAVE] = p1y; s[2 * PL_WAVE] = a0; s[3 * PL_WAVE] = a1;
      if (ss_distance(p1x, p1y, a0, a1, fx, fy) > limit) st = 2;
    }
    ln_out[4 * k] = p1x; ln_out[4 * k + 1] = p1y; ln_out[4 * k + 2] = p2x; ln_out[4 * k + 3] = p2y;
  }
  if (st != 0) {
    for (int j = 0; j < 9; ++j) rec[j] = qnan;
    rec[7] = (double)nl;
    rec[8] = 0.0;
    status[row] = st;
    return;
  }

  int nfev = 0;
  // the objective: max over the lines (Python's max: a later value replaces the running one only when it is greater);
  // false = scipy's evaluation budget is spent (_MaxFuncCallError: the iteration is abandoned where it stands)
  auto eval = [&](double px, double py, double& f) -> bool {
    if (nfev >= kSsMaxFun) return false;
    ++nfev;
    double best = 0.0;
    for (int k = 0; k < nl; ++k) {
      const double* s = s_line + (k * 4) * PL_WAVE + lane;
      const double d = ss_distance(s[0], s[PL_WAVE], s[2 * PL_WAVE], s[3 * PL_WAVE], px, py);
      if (k == 0 || d > best) best = d;
    }
    f = best;
    return true;
  };

  // the start simplex: x0 = (fx, fy, 0); vertex k + 1 moves coordinate k to 1.05 * itself, or to 0.00025 from zero
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  SsVertex s0{fx, fy, 0.0, inf}, s1{fx != 0.0 ? 1.05 * fx : 0.00025, fy, 0.0, inf},
      s2{fx, fy != 0.0 ? 1.05 * fy : 0.00025, 0.0, inf}, s3{fx, fy, 0.00025, inf};
  eval(s0.x, s0.y, s0.f);
  eval(s1.x, s1.y, s1.f);
  eval(s2.x, s2.y, s2.f);
  eval(s3.x, s3.y, s3.f);
  ss_sort(s0, s1, s2, s3);

  int iterations = 1;
  while (nfev < kSsMaxFun && iterations < kSsMaxIter) {
    double dx = ss_npmax(fabs(s1.x - s0.x), fabs(s1.y - s0.y));
    dx = ss_npmax(dx, fabs(s1.z - s0.z));
    dx = ss_npmax(dx, fabs(s2.x - s0.x)); dx = ss_npmax(dx, fabs(s2.y - s0.y)); dx = ss_npmax(dx, fabs(s2.z - s0.z));
    dx = ss_npmax(dx, fabs(s3.x - s0.x)); dx = ss_npmax(dx, fabs(s3.y - s0.y)); dx = ss_npmax(dx, fabs(s3.z - s0.z));
    const double df = ss_npmax(ss_npmax(fabs(s0.f - s1.f), fabs(s0.f - s2.f)), fabs(s0.f - s3.f));
    if (dx <= 1e-4 && df <= 1e-3) break;
    do {
      const double bx = ((s0.x + s1.x) + s2.x) / 3.0, by = ((s0.y + s1.y) + s2.y) / 3.0, bz = ((s0.z + s1.z) + s2.z) / 3.0;
      const SsVertex w = s3;
      SsVertex r{2.0 * bx - w.x, 2.0 * by - w.y, 2.0 * bz - w.z, 0.0};        // (1 + rho) * xbar - rho * worst, rho = 1
      if (!eval(r.x, r.y, r.f)) break;
      bool shrink = false;
      if (!(r.f < s0.f) && r.f < s2.f) {
        s3 = r;
      } else {
        // expansion 3 * xbar - 2 * w; outside contraction 1.5 * xbar - 0.5 * w; inside contraction 0.5 * xbar + 0.5 * w
        const bool expand = r.f < s0.f, outside = !expand && r.f < w.f;
        const double c1 = expand ? 3.0 : (outside ? 1.5 : 0.5), c2 = expand ? -2.0 : (outside ? -0.5 : 0.5);
        SsVertex t{c1 * bx + c2 * w.x, c1 * by + c2 * w.y, c1 * bz + c2 * w.z, 0.0};
        if (!eval(t.x, t.y, t.f)) break;
        if (expand) s3 = t.f < r.f ? t : r;
        else if (outside) { if (t.f <= r.f) s3 = t; else shrink = true; }
        else { if (t.f < w.f) s3 = t; else shrink = true; }
      }
      if (shrink) {                                                          // sim[j] = sim[0] + sigma * (sim[j] - sim[0])
        s1.x = s0.x + 0.5 * (s1.x - s0.x); s1.y = s0.y + 0.5 * (s1.y - s0.y); s1.z = s0.z + 0.5 * (s1.z - s0.z);
        if (!eval(s1.x, s1.y, s1.f)) break;
        s2.x = s0.x + 0.5 * (s2.x - s0.x); s2.y = s0.y + 0.5 * (s2.y - s0.y); s2.z = s0.z + 0.5 * (s2.z - s0.z);
        if (!eval(s2.x, s2.y, s2.f)) break;
        s3.x = s0.x + 0.5 * (s3.x - s0.x); s3.y = s0.y + 0.5 * (s3.y - s0.y); s3.z = s0.z + 0.5 * (s3.z - s0.z);
        if (!eval(s3.x, s3.y, s3.f)) break;
      }
      ++iterations;
    } while (false);
    ss_sort(s0, s1, s2, s3);
  }

  // Starshot._find_wobble_minimize and the accept test of _get_reasonable_wobble
  const double fun = ss_npmin(ss_npmin(s0.f, s1.f), ss_npmin(s2.f, s3.f));
  const double radius_mm = fun / dpmm, diameter_mm = radius_mm * 2.0;
  const double ex = s0.x - fx, ey = s0.y - fy;
  const bool near = sqrt((ex * ex + ey * ey) + 0.0) < limit;
  const bool accept = (diameter_mm < max_wobble_diameter && near) || !recursive;
  rec[0] = s0.x; rec[1] = s0.y; rec[2] = fun; rec[3] = radius_mm; rec[4] = diameter_mm;
  rec[5] = (double)iterations; rec[6] = (double)nfev; rec[7] = (double)nl;
  rec[8] = diameter_mm < tolerance ? 1.0 : 0.0;
  status[row] = accept ? 0 : 3;
}

// ---- the profile tail ---------------------------------------------------------------------------------------------------------
// np.roll(values, -np.where(values == values.min())[0][0]): one workgroup per ring.  A lane walks its samples in ascending
// order and replaces its minimum on a strict <, the tree keeps the lower index of equal minima: the FIRST minimum.
__global__ void __launch_bounds__(kPkThreads)
ss_roll_kernel(const double* __restrict__ x, int len, double* __restrict__ out, int32_t* __restrict__ roll) {
  __shared__ double s_v[kPkThreads];
  __shared__ int s_i[kPkThreads];
  const int tid = threadIdx.x;
  const double* xr = x + (size_t)blockIdx.x * len;
  double best = xr[0];
  int bi = 0;
  for (int i = tid; i < len; i += kPkThreads) {
    const double v = xr[i];
    if (v < best) { best = v; bi = i; }
  }
  s_v[tid] = best;
  s_i[tid] = bi;
  __syncthreads();
  for (int o = kPkThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      const double ov = s_v[tid + o];
      const int oi = s_i[tid + o];
      if (ov < s_v[tid] || (ov == s_v[tid] && oi < s_i[tid])) { s_v[tid] = ov; s_i[tid] = oi; }
    }
    __syncthreads();
  }
  const int r = s_i[0];
  double* dst = out + (size_t)blockIdx.x * len;
  for (int i = tid; i < len; i += kPkThreads) {
    int j = i + r;
    if (j >= len) j -= len;
    dst[i] = xr[j];
  }
  if (tid == 0) roll[blockIdx.x] = r;
}

// find_peaks on the processed ring with the ring's own height (a value in [0, 1] is a ratio of the ring's range, as
// _parse_peak_args has it), then what StarProfile makes of the result: the index of every `peaks` entry -- int(round(lt + (rt -
// lt) / 2)), Python's round = half to even, for the FWHM search, the peak's own index otherwise -- and CircleProfile._map_peaks:
// x = cos_table[(idx + roll) % size] * radius + centre x (np.roll moved the coordinates with the values), a multiply and an add.
// The tables are numpy's cos / sin of circle_radians, uploaded by the caller: a device cos would not carry their bits.
template <bool STAGE>
__global__ void __launch_bounds__(kPkThreads)
ss_peaks_kernel(const double* __restrict__ x, int len, const double* __restrict__ thr, const int32_t* __restrict__ roll,
                const double* __restrict__ tab_cos, const double* __restrict__ tab_sin, const double* __restrict__ geom, int fwhm,
                pl_peak_params prm, int cap, int maxc, int32_t* __restrict__ d_count, int32_t* __restrict__ d_idx,
                int32_t* __restrict__ d_lb, int32_t* __restrict__ d_rb, double* __restrict__ d_props,
                int32_t* __restrict__ d_status, int32_t* __restrict__ d_pidx, double* __restrict__ d_points) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
  __shared__ Scan scan;
  __shared__ double s_red[2 * (kPkThreads / PL_WAVE)];
  __shared__ int s_cnt;
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  const PeakLds L{smem_all, &scan, s_red, &s_cnt};
  pl_peak_params p = prm;
  const double t = thr[row];
  p.threshold = t;
  p.threshold_is_ratio = (t >= 0.0 && t <= 1.0) ? 1 : 0;
  find_peaks_profile<STAGE, kPkThreads>(x + row * len, len, p.region_lo, p.region_hi, p, cap, maxc, L, tid, d_count + row,
                                        d_idx + row * cap, d_lb + row * cap, d_rb + row * cap, d_props + row * 6 * cap,
                                        d_status + row);
  __syncthreads();                                  // the ring's output rows (global memory) are this workgroup's own
  const int c = d_count[row];
  const bool whole = d_status[row] == 0;            // otherwise the search ran out of room: the caller takes another path
  const double radius = geom[row * 3], cx = geom[row * 3 + 1], cy = geom[row * 3 + 2];
  const int r = roll[row];
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  for (int k = tid; k < cap; k += kPkThreads) {
    int idx = -1;
    double px = qnan, py = qnan;
    if (whole && k < c) {
      if (fwhm) {
        const double lt = d_props[row * 6 * cap + 4 * cap + k], rt = d_props[row * 6 * cap + 5 * cap + k];
        idx = (int)rint(lt + (rt - lt) / 2);
      } else {
        idx = d_idx[row * cap + k];
      }
      idx = idx < 0 ? 0 : (idx >= len ? len - 1 : idx);      // (the interpolated edges lie inside the ring)
      int j = idx + r;
      if (j >= len) j -= len;
      px = tab_cos[j] * radius + cx;
      py = tab_sin[j] * radius + cy;
    }
    d_pidx[row * cap + k] = idx;
    d_points[(row * cap + k) * 2] = px;
    d_points[(row * cap + k) * 2 + 1] = py;
  }
  __syncthreads();
  if (tid == 0 && !whole) d_count[row] = cap + 1;
}

}  // namespace

/* roll to the first minimum: see pylinac_hip.h */
extern "C" int pl_starshot_roll(const double* d_x, int64_t n, int len, double* d_out, int32_t* d_roll, void* stream) {
  PL_REQUIRE(d_x && d_out && d_roll && d_x != d_out, "null pointer or in-place call");
  PL_REQUIRE(n >= 0 && n <= 0x7fffffffLL && len > 0, "bad shape");
  if (n == 0) return PL_OK;
  hipLaunchKernelGGL(ss_roll_kernel, dim3((unsigned)n), dim3(kPkThreads), 0, (hipStream_t)stream, d_x, len, d_out, d_roll);
  return pl_check_launch("pl_starshot_roll");
}

/* peak search with a height per ring, peak indices and image coordinates: see pylinac_hip.h */
extern "C" int pl_starshot_peaks(const double* d_x, int64_t n, int len, const double* d_threshold, const int32_t* d_roll,
                                 const double* d_cos, const double* d_sin, const double* d_geom, int fwhm,
                                 const pl_peak_params* params, int cap, int32_t* d_count, int32_t* d_idx, int32_t* d_left_base,
                                 int32_t* d_right_base, double* d_props, int32_t* d_status, int32_t* d_peak_idx,
                                 double* d_points, void* stream) {
  PL_REQUIRE(d_x && d_threshold && d_roll && d_cos && d_sin && d_geom && params && d_count && d_idx && d_left_base &&
                 d_right_base && d_props && d_status && d_peak_idx && d_points, "null pointer");
  PL_REQUIRE(n >= 0 && n <= 0x7fffffffLL && len > 0 && cap > 0, "bad shape");
  PL_REQUIRE(params->distance >= 1, "distance must be >= 1");
  if (n == 0) return PL_OK;
  const int lo = params->region_lo < 0 ? 0 : params->region_lo;
  const int hi = params->region_hi > len ? len : params->region_hi;
  const int m = hi > lo ? hi - lo : 0;
  const bool stage_x = m <= kStageMax;
  int maxc;
  const size_t lds = peak_search_lds(m, stage_x, &maxc);
  static std::atomic<bool> attr_set{false};
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)ss_peaks_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)ss_peaks_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (e != hipSuccess) { pl_set_error("pl_starshot_peaks: LDS attribute: %s", hipGetErrorString(e)); return PL_ERR_HIP; }
    attr_set = true;
  }
  if (stage_x)
    hipLaunchKernelGGL(ss_peaks_kernel<true>, dim3((unsigned)n), dim3(kPkThreads), lds, (hipStream_t)stream, d_x, len,
                       d_threshold, d_roll, d_cos, d_sin, d_geom, fwhm, *params, cap, maxc, d_count, d_idx, d_left_base,
                       d_right_base, d_props, d_status, d_peak_idx, d_points);
  else
    hipLaunchKernelGGL(ss_peaks_kernel<false>, dim3((unsigned)n), dim3(kPkThreads), lds, (hipStream_t)stream, d_x, len,
                       d_threshold, d_roll, d_cos, d_sin, d_geom, fwhm, *params, cap, maxc, d_count, d_idx, d_left_base,
                       d_right_base, d_props, d_status, d_peak_idx, d_points);
  return pl_check_launch("pl_starshot_peaks");
}

/* the wobble fit of a table of datasets: see pylinac_hip.h */
extern "C" int pl_starshot_wobble(const double* d_points, const int32_t* d_count, const double* d_focus, int64_t m, int cap,
                                  double dpmm, double max_wobble_diameter, double tolerance, int recursive, double* d_record,
                                  double* d_lines, int32_t* d_fit_status, void* stream) {
  PL_REQUIRE(d_points && d_count && d_focus && d_record && d_lines && d_fit_status, "null pointer");
  PL_REQUIRE(m >= 0 && m <= 0x7fffffffLL - PL_WAVE, "bad number of datasets");
  PL_REQUIRE(cap >= 2 && cap <= 2 * kSsMaxLines && (cap & 1) == 0, "cap: an even number of peaks, at most 64");
  PL_REQUIRE(dpmm > 0.0, "dpmm must be positive");
  if (m == 0) return PL_OK;
  hipLaunchKernelGGL(ss_wobble_kernel, dim3((unsigned)pl_cdiv(m, PL_WAVE)), dim3(PL_WAVE), 0, (hipStream_t)stream, d_points,
                     d_count, d_focus, (int)m, cap, dpmm, max_wobble_diameter, tolerance, recursive, d_record, d_lines,
                     d_fit_status);
  return pl_check_launch("pl_starshot_wobble");
}
