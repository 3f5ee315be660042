// 1-D resampling of profiles.
//
// Replaces: scipy.interpolate.interp1d(x, y, kind="linear" | "cubic", bounds_error=False,
// fill_value="extrapolate") as called at pylinac/core/profile.py:1349-1358 (SingleProfile._interpolate:
// a detector profile of ~10^2-10^3 samples resampled to ~10x as many on linspace(x0-offset, xN+offset)).
//
// kind 0 (linear): scipy's _call_linear formula exactly -- hi = clip(searchsorted(x, xq, "left"), 1, L-1),
//   slope = (y_hi - y_lo) / (x_hi - x_lo), out = slope * (xq - x_lo) + y_lo; float64, no FMA: bit-identical.
// kind 1 (cubic): scipy builds make_interp_spline(x, y, k=3) = the not-a-knot interpolating cubic spline and
//   evaluates its B-spline form.  That spline is unique, so it is computed here in the classical form: second
//   derivatives M from the tridiagonal system with the two not-a-knot rows folded in (Thomas algorithm, one
//   lane per profile: L is small and the recurrence is sequential), then the piecewise cubic is evaluated
//   per query (end pieces extrapolate, as BSpline(extrapolate=True) does).  Agreement with scipy: ~1e-13
//   relative (different but equally stable arithmetic); tests state 1e-10.
#include "pl_common.h"

namespace {

constexpr int kThreads = 256;

// first index i in [0, n) with x[i] >= v (np.searchsorted side="left"), n if none
__device__ __forceinline__ int lower_bound(const double* __restrict__ x, int n, double v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (x[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ void interp_linear_kernel(const double* __restrict__ x, int64_t x_stride, const double* __restrict__ y,
                                     int L, const double* __restrict__ xq, int S, int64_t total,
                                     double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int q = (int)(i % S);
  const int64_t p = i / S;
  const double* xs = x + p * x_stride;
  const double* ys = y + p * (int64_t)L;
  const double v = xq[q];
  int hi = lower_bound(xs, L, v);
  hi = hi < 1 ? 1 : (hi > L - 1 ? L - 1 : hi);
  const int lo = hi - 1;
  const double slope = (ys[hi] - ys[lo]) / (xs[hi] - xs[lo]);
  out[i] = slope * (v - xs[lo]) + ys[lo];
}

// second derivatives of the not-a-knot cubic spline; work: 2 L doubles per profile (c', d')
__global__ void spline_moments_kernel(const double* __restrict__ x, int64_t x_stride, const double* __restrict__ y,
                                      int L, int64_t n_profiles, double* __restrict__ M,
                                      double* __restrict__ work) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= n_profiles) return;
  const double* xs = x + p * x_stride;
  const double* ys = y + p * (int64_t)L;
  double* m = M + p * (int64_t)L;
  double* cp = work + p * 2 * (int64_t)L;
  double* dp = cp + L;
  const int n = L;
  auto h = [&](int i) { return xs[i + 1] - xs[i]; };
  auto rhs = [&](int i) { return 6.0 * ((ys[i + 1] - ys[i]) / h(i) - (ys[i] - ys[i - 1]) / h(i - 1)); };
  // unknowns M_1 .. M_{n-2}; row i: a_i M_{i-1} + b_i M_i + c_i M_{i+1} = r_i
  auto row = [&](int i, double& a, double& b, double& c, double& r) {
    a = h(i - 1);
    b = 2.0 * (h(i - 1) + h(i));
    c = h(i);
    r = rhs(i);
    if (i == 1) {  // M_0 = (1 + h0/h1) M_1 - (h0/h1) M_2
      const double t = h(0) / h(1);
      b += h(0) * (1.0 + t);
      c -= h(0) * t;
      a = 0.0;
    }
    if (i == n - 2) {  // M_{n-1} = (1 + h_{n-2}/h_{n-3}) M_{n-2} - (h_{n-2}/h_{n-3}) M_{n-3}
      const double t = h(n - 2) / h(n - 3);
      b += h(n - 2) * (1.0 + t);
      a -= h(n - 2) * t;
      c = 0.0;
    }
  };
  double a, b, c, r;
  row(1, a, b, c, r);
  cp[1] = c / b;
  dp[1] = r / b;
  for (int i = 2; i <= n - 2; ++i) {
    row(i, a, b, c, r);
    const double den = b - a * cp[i - 1];
    cp[i] = c / den;
    dp[i] = (r - a * dp[i - 1]) / den;
  }
  m[n - 2] = dp[n - 2];
  for (int i = n - 3; i >= 1; --i) m[i] = dp[i] - cp[i] * m[i + 1];
  {
    const double t0 = h(0) / h(1);
    m[0] = (1.0 + t0) * m[1] - t0 * m[2];
    const double t1 = h(n - 2) / h(n - 3);
    m[n - 1] = (1.0 + t1) * m[n - 2] - t1 * m[n - 3];
  }
}

__global__ void spline_eval_kernel(const double* __restrict__ x, int64_t x_stride, const double* __restrict__ y,
                                   const double* __restrict__ M, int L, const double* __restrict__ xq, int S,
                                   int64_t total, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int q = (int)(i % S);
  const int64_t p = i / S;
  const double* xs = x + p * x_stride;
  const double* ys = y + p * (int64_t)L;
  const double* m = M + p * (int64_t)L;
  const double v = xq[q];
  int hi = lower_bound(xs, L, v);
  hi = hi < 1 ? 1 : (hi > L - 1 ? L - 1 : hi);
  const int lo = hi - 1;
  const double hh = xs[hi] - xs[lo];
  const double a = xs[hi] - v, b = v - xs[lo];
  out[i] = (m[lo] * a * a * a + m[hi] * b * b * b) / (6.0 * hh) + (ys[lo] / hh - m[lo] * hh / 6.0) * a +
           (ys[hi] / hh - m[hi] * hh / 6.0) * b;
}

// np.gradient(y) with unit spacing, edge_order 1: central differences inside, one-sided at the two ends
__global__ void gradient_kernel(const double* __restrict__ y, int L, int64_t total, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int k = (int)(i % L);
  const double* p = y + (i - k);
  out[i] = k == 0 ? p[1] - p[0] : (k == L - 1 ? p[L - 1] - p[L - 2] : (p[k + 1] - p[k - 1]) / 2.0);
}

// ---- scipy.ndimage.zoom(values, zoom, order=3, mode="nearest", grid_mode) of 1-D profiles --------------------
// (ProfileBase.as_resampled, pylinac/core/profile.py:353-390; PhysicalProfileMixin.as_resampled :950-1011 with grid_mode).  scipy pads the input with 12 edge samples, runs the cubic
// B-spline prefilter (pole sqrt(3) - 2, mirror initialisation) over the padded array and evaluates the four-tap spline
// at i * (L - 1) / (S - 1) + 12 with clamped tap indices.  The prefilter is a sequential recursion: one lane per profile.
constexpr int kZoomPad = 12;

__global__ void zoom_prefilter_kernel(const double* __restrict__ y, int L, int64_t n_profiles, double* __restrict__ work) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= n_profiles) return;
  const double* v = y + p * (int64_t)L;
  const int n = L + 2 * kZoomPad;
  double* c = work + p * (int64_t)n;
  const double z = sqrt(3.0) - 2.0;
  const double gain = (1.0 - z) * (1.0 - 1.0 / z);
  for (int i = 0; i < n; ++i) {
    const int k = i - kZoomPad;
    c[i] = v[k < 0 ? 0 : (k > L - 1 ? L - 1 : k)] * gain;
  }
  double z_i = z;
  const double z_n_1 = pow(z, (double)(n - 1));
  double c0 = c[0] + z_n_1 * c[n - 1];
  for (int i = 1; i < n - 1; ++i) {
    c0 += z_i * (c[i] + z_n_1 * c[n - 1 - i]);
    z_i *= z;
  }
  c[0] = c0 / (1.0 - z_n_1 * z_n_1);
  for (int i = 1; i < n; ++i) c[i] += z * c[i - 1];
  c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1.0);
  for (int i = n - 2; i >= 0; --i) c[i] = z * (c[i + 1] - c[i]);
}

__global__ void zoom_eval_kernel(const double* __restrict__ work, int L, int S, int grid_mode, int64_t total,
                                 double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int q = (int)(i % S);
  const int64_t p = i / S;
  const int n = L + 2 * kZoomPad;
  const double* c = work + p * (int64_t)n;
  // grid_mode: samples are cell centres (zoom = L / S, shift = zoom / 2 - 1 / 2); otherwise the end points coincide
  const double zoom = grid_mode ? (double)L / (double)S : (S > 1 ? (double)(L - 1) / (double)(S - 1) : 1.0);
  const double shift = grid_mode ? 0.5 * zoom - 0.5 : 0.0;
  const double cc = zoom * (double)q + shift + (double)kZoomPad;
  const double fl = floor(cc);
  const double yv = cc - fl, zv = 1.0 - yv;
  const double w1 = (yv * yv * (yv - 2.0) * 3.0 + 4.0) / 6.0;
  const double w2 = (zv * zv * (zv - 2.0) * 3.0 + 4.0) / 6.0;
  const double w0 = zv * zv * zv / 6.0;
  const double w3 = 1.0 - w0 - w1 - w2;
  const int start = (int)fl - 1;
  auto at = [&](int k) { return c[k < 0 ? 0 : (k > n - 1 ? n - 1 : k)]; };
  double t = 0.0;
  t += at(start) * w0;
  t += at(start + 1) * w1;
  t += at(start + 2) * w2;
  t += at(start + 3) * w3;
  out[i] = t;
}


// ------------------------------------------------------------- FieldAnalysis: SingleProfile.field_data windows
// pl_field_windows: SingleProfile.field_data (pylinac/core/profile.py:1463-1633) and the protocol reductions over its "field
// values" (pylinac/field_analysis.py:37-231) for every processed profile, one wave per profile:
//   field = [anchor -/+ in_field_ratio * span / 2], core = [anchor -/+ slope_exclusion_ratio * field.width / 2]
//   grid  = x_indices + (anchor - round(anchor)); first / last = the grid samples nearest the field's ends (first on a tie)
//   field values f = y(grid[first .. last]), y = scipy's linear interp1d of the profile (extrapolating)
//   max / min (Varian, Elekta flatness), 100 (f_k - f_{n-1-k}) / y(round(anchor)) at numpy's first argmax of |.|, the PDQ
//   IEC ratio max(|l / r|, |r / l|) * sign at its first argmax, the Siemens area sums over f[: n // 2] and f[ceil(n / 2):]
//   (numpy's pairwise summation, bit for bit), the two edge-slope regressions over _sample_points_in_physical_window
//   (field.lo .. core.lo and core.hi .. field.hi), and the "top" window core.lo .. core.hi, whose samples go to d_top for the
//   host's polyfit / L-BFGS-B.  float64 in the reference's operation order, no contraction (the build's -ffp-contract=off).
constexpr int kFwStats = 16;

__device__ __forceinline__ double fw_lookup(const double* __restrict__ xi, const double* __restrict__ v, int S, double q) {
  int hi = lower_bound(xi, S, q);
  hi = hi < 1 ? 1 : (hi > S - 1 ? S - 1 : hi);
  const int lo = hi - 1;
  const double slope = (v[hi] - v[lo]) / (xi[hi] - xi[lo]);
  return slope * (q - xi[lo]) + v[lo];
}

// np.abs((xi + d) - p).argmin() over the whole wave: the smallest value, the lowest index among equal ones
__device__ __forceinline__ int fw_nearest(const double* __restrict__ xi, int S, double d, double p) {
  const int lane = threadIdx.x & 63;
  double best = INFINITY;
  int bi = S;
  for (int j = lane; j < S; j += PL_WAVE) {
    const double a = fabs((xi[j] + d) - p);
    if (a < best) { best = a; bi = j; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  return bi < S ? bi : 0;
}

// np.searchsorted(xi, p, side) on the ascending x_indices: the number of samples < p ("left") or <= p ("right")
__device__ __forceinline__ int fw_count(const double* __restrict__ xi, int S, double p, bool right) {
  const int lane = threadIdx.x & 63;
  int c = 0;
  for (int j = lane; j < S; j += PL_WAVE) c += right ? (xi[j] <= p) : (xi[j] < p);
  return pl_wave_reduce(c, [](int a, int b) { return a + b; });
}

// SingleProfile._sample_points_in_physical_window (profile.py:1237-1283) -> [start, stop) of x_indices
__device__ __forceinline__ void fw_window(const double* __restrict__ xi, int S, double a, double b, int& start, int& stop) {
  const double lo = a <= b ? a : b, hi = a <= b ? b : a;
  start = fw_count(xi, S, lo, false);
  stop = fw_count(xi, S, hi, true);
  if (stop - start < 3) {
    const int p = fw_nearest(xi, S, 0.0, lo), q = fw_nearest(xi, S, 0.0, hi);
    start = min(p, q);
    stop = max(p, q) + 1;
  }
  if (stop - start < 3) {
    const int end = min(S, max(0, fw_nearest(xi, S, 0.0, (lo + hi) / 2.0) - 1) + 3);
    start = max(0, end - 3);
    stop = end;
  }
}

// scipy.stats.linregress' slope over the window's samples (x_indices, y(x_indices))
__device__ __forceinline__ double fw_slope(const double* __restrict__ xi, const double* __restrict__ v, int S, int start, int stop) {
  const int lane = threadIdx.x & 63;
  const int n = stop - start;
  auto add = [](double a, double b) { return a + b; };
  double sx = 0.0, sy = 0.0;
  for (int j = start + lane; j < stop; j += PL_WAVE) { sx += xi[j]; sy += fw_lookup(xi, v, S, xi[j]); }
  const double xm = pl_wave_reduce(sx, add) / n, ym = pl_wave_reduce(sy, add) / n;
  double sxx = 0.0, sxy = 0.0;
  for (int j = start + lane; j < stop; j += PL_WAVE) {
    const double dx = xi[j] - xm, dy = fw_lookup(xi, v, S, xi[j]) - ym;
    sxx += dx * dx;
    sxy += dx * dy;
  }
  return (pl_wave_reduce(sxy, add) / n) / (pl_wave_reduce(sxx, add) / n);
}

// numpy's pairwise_sum (loops_utils.h: < 8 sequential from -0.0, <= 128 eight accumulators, else split at n / 2 rounded
// down to a multiple of 8) without recursion: one lane walks the tree with a stack in LDS
struct FwFrame { int start, n, stage; double left; };

__device__ __forceinline__ double fw_leaf(const double* a, int n) {
  if (n < 8) {
    double res = -0.0;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
    r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) res += a[i];
  return res;
}

__device__ __forceinline__ int fw_split(int n) { const int n2 = n / 2; return n2 - n2 % 8; }

__device__ double fw_pairwise(const double* a, int n, FwFrame* st) {
  if (n <= 128) return fw_leaf(a, n);
  int top = 0;
  st[top++] = FwFrame{0, n, 0, 0.0};
  for (;;) {
    FwFrame& f = st[top - 1];
    if (f.n > 128) {
      f.stage = 1;
      st[top++] = FwFrame{f.start, fw_split(f.n), 0, 0.0};
      continue;
    }
    double r = fw_leaf(a + f.start, f.n);
    --top;
    while (top > 0) {
      FwFrame& p = st[top - 1];
      if (p.stage == 1) {
        p.left = r;
        p.stage = 2;
        const int n2 = fw_split(p.n);
        st[top++] = FwFrame{p.start + n2, p.n - n2, 0, 0.0};
        break;
      }
      r = p.left + r;
      --top;
    }
    if (top == 0) return r;
  }
}

__global__ void __launch_bounds__(PL_WAVE)
field_windows_kernel(const double* __restrict__ xi, const double* __restrict__ values, int S,
                     const double* __restrict__ anchor, const double* __restrict__ span, double in_field_ratio,
                     double slope_exclusion_ratio, int tcap, double* __restrict__ stats, double* __restrict__ top_y,
                     double* __restrict__ fv_scratch) {
  __shared__ FwFrame stack[32];
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  const double* v = values + row * (int64_t)S;
  double* o = stats + row * kFwStats;
  double* fv = fv_scratch + row * (int64_t)S;
  const double c = anchor[row], sp = span[row];
  if (!(fabs(c) < 1e9) || !(fabs(sp) < 1e9)) {            // no edges: nothing to measure (NaN in, NaN out)
    if (lane < kFwStats) o[lane] = (lane == 13 || lane == 14 || lane == 5) ? 0.0 : NAN;
    return;
  }
  const double full = in_field_ratio * sp;
  const double flo = c - full / 2.0, fhi = c + full / 2.0;
  const double fwidth = fhi - flo;
  const double core = slope_exclusion_ratio * fwidth;
  const double clo = c - core / 2.0, chi = c + core / 2.0;
  const double rc = rint(c), d = c - rc;
  const int first = fw_nearest(xi, S, d, flo), last = fw_nearest(xi, S, d, fhi);
  const int n = last - first + 1;
  const double cax = fw_lookup(xi, v, S, rc);
  double mx = -INFINITY, mn = INFINITY;
  for (int k = lane; k < n; k += PL_WAVE) {
    const double f = fw_lookup(xi, v, S, xi[first + k] + d);
    fv[k] = f;
    mx = f > mx ? f : mx;
    mn = f < mn ? f : mn;
  }
  mx = pl_wave_reduce(mx, [](double a, double b) { return a > b ? a : b; });
  mn = pl_wave_reduce(mn, [](double a, double b) { return a < b ? a : b; });
  __syncthreads();
  // point difference and PDQ IEC: first argmax of |.| (strict > per lane over ascending k, lowest k across lanes)
  double pd = NAN, pd_abs = -1.0, pq = NAN, pq_abs = -1.0;
  int pd_k = n, pq_k = n;
  for (int k = lane; k < n; k += PL_WAVE) {
    const double lt = fv[k], rt = fv[n - 1 - k];
    const double s1 = (100.0 * (lt - rt)) / cax;
    if (fabs(s1) > pd_abs) { pd_abs = fabs(s1); pd = s1; pd_k = k; }
    const double q1 = lt / rt, q2 = rt / lt;
    const double a1 = fabs(q1), a2 = fabs(q2);
    const double sgn_src = a1 > a2 ? q1 : q2;
    const double sgn = sgn_src > 0.0 ? 1.0 : (sgn_src < 0.0 ? -1.0 : (sgn_src == 0.0 ? 0.0 : sgn_src));
    const double mxq = a2 > a1 ? a2 : a1;                    // python's max(a, b): b only if b > a
    const double s2 = mxq * sgn;
    if (fabs(s2) > pq_abs) { pq_abs = fabs(s2); pq = s2; pq_k = k; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double oa = __shfl_xor(pd_abs, off, 64), ov = __shfl_xor(pd, off, 64);
    const int ok = __shfl_xor(pd_k, off, 64);
    if (oa > pd_abs || (oa == pd_abs && ok < pd_k)) { pd_abs = oa; pd = ov; pd_k = ok; }
    const double qa = __shfl_xor(pq_abs, off, 64), qv = __shfl_xor(pq, off, 64);
    const int qk = __shfl_xor(pq_k, off, 64);
    if (qa > pq_abs || (qa == pq_abs && qk < pq_k)) { pq_abs = qa; pq = qv; pq_k = qk; }
  }
  int ls, le, rs, re, ts, te;
  fw_window(xi, S, flo, clo, ls, le);
  fw_window(xi, S, chi, fhi, rs, re);
  fw_window(xi, S, clo, chi, ts, te);
  const double slope_l = fw_slope(xi, v, S, ls, le), slope_r = fw_slope(xi, v, S, rs, re);
  const int tn = te - ts;
  for (int j = lane; j < tn && j < tcap; j += PL_WAVE) top_y[row * (int64_t)tcap + j] = fw_lookup(xi, v, S, xi[ts + j]);
  if (lane == 0) {
    double area = NAN;
    if (n > 0) {
      const int half_lo = n / 2, half_hi = (n + 1) / 2;
      const double al = fw_pairwise(fv, half_lo, stack), ar = fw_pairwise(fv + half_hi, n - half_hi, stack);
      area = (100.0 * (al - ar)) / (al + ar);
    }
    o[0] = flo; o[1] = fhi; o[2] = fwidth; o[3] = clo; o[4] = chi; o[5] = (double)n;
    o[6] = n > 0 ? mx : NAN; o[7] = n > 0 ? mn : NAN; o[8] = pd; o[9] = pq; o[10] = area;
    o[11] = slope_l; o[12] = slope_r; o[13] = (double)ts; o[14] = (double)tn; o[15] = cax;
  }
}

}  // namespace

extern "C" int pl_zoom1d_cubic(const double* y, int64_t n_profiles, int length, int out_length, int grid_mode,
                               double* work, double* out, void* stream) {
  PL_REQUIRE(y && work && out, "null pointer");
  PL_REQUIRE(n_profiles >= 0 && length >= 2 && out_length >= 1, "bad shape");
  if (n_profiles == 0) return PL_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = n_profiles * (int64_t)out_length;
  PL_REQUIRE(pl_cdiv(total, kThreads) <= 0x7fffffffLL, "batch too large for one launch");
  hipLaunchKernelGGL(zoom_prefilter_kernel, dim3((unsigned)pl_cdiv(n_profiles, kThreads)), dim3(kThreads), 0, st, y,
                     length, n_profiles, work);
  hipLaunchKernelGGL(zoom_eval_kernel, dim3((unsigned)pl_cdiv(total, kThreads)), dim3(kThreads), 0, st, work, length,
                     out_length, grid_mode ? 1 : 0, total, out);
  return pl_check_launch("pl_zoom1d_cubic");
}

extern "C" int pl_gradient1d(const double* y, int64_t n_profiles, int length, double* out, void* stream) {
  PL_REQUIRE(y && out, "null pointer");
  PL_REQUIRE(n_profiles >= 0 && length >= 2, "np.gradient needs at least 2 samples");
  if (n_profiles == 0) return PL_OK;
  const int64_t total = n_profiles * (int64_t)length;
  PL_REQUIRE(pl_cdiv(total, kThreads) <= 0x7fffffffLL, "batch too large for one launch");
  hipLaunchKernelGGL(gradient_kernel, dim3((unsigned)pl_cdiv(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     y, length, total, out);
  return pl_check_launch("pl_gradient1d");
}

extern "C" int pl_interp1d(const double* x, int64_t x_stride, const double* y, int64_t n_profiles, int length,
                           const double* xq, int n_query, int kind, double* work, double* out, void* stream) {
  PL_REQUIRE(x && y && xq && out, "null pointer");
  PL_REQUIRE(n_profiles >= 0 && n_query >= 0, "bad shape");
  PL_REQUIRE(kind == 0 || kind == 1, "kind must be 0 (linear) or 1 (cubic)");
  PL_REQUIRE(x_stride == 0 || x_stride >= length, "x_stride must be 0 (shared abscissae) or >= length");
  if (kind == 0) PL_REQUIRE(length >= 2, "linear interpolation needs >= 2 samples");
  if (kind == 1) {
    // scipy: "The number of derivatives at boundaries does not match" below k+1 points
    PL_REQUIRE(length >= 4, "cubic interpolation needs >= 4 samples");
    PL_REQUIRE(work, "cubic interpolation needs a workspace of 3 * n_profiles * length doubles");
  }
  if (n_profiles == 0 || n_query == 0) return PL_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = n_profiles * (int64_t)n_query;
  PL_REQUIRE(pl_cdiv(total, kThreads) <= 0x7fffffffLL, "batch too large for one launch");
  if (kind == 0) {
    hipLaunchKernelGGL(interp_linear_kernel, dim3((unsigned)pl_cdiv(total, kThreads)), dim3(kThreads), 0, st, x,
                       x_stride, y, length, xq, n_query, total, out);
  } else {
    double* M = work;
    double* scratch = work + n_profiles * (int64_t)length;
    hipLaunchKernelGGL(spline_moments_kernel, dim3((unsigned)pl_cdiv(n_profiles, kThreads)), dim3(kThreads), 0, st,
                       x, x_stride, y, length, n_profiles, M, scratch);
    hipLaunchKernelGGL(spline_eval_kernel, dim3((unsigned)pl_cdiv(total, kThreads)), dim3(kThreads), 0, st, x,
                       x_stride, y, M, length, xq, n_query, total, out);
  }
  return pl_check_launch("pl_interp1d");
}

extern "C" int pl_field_windows(const double* d_x_indices, const double* d_values, int64_t n, int s, const double* d_anchor,
                                const double* d_span, double in_field_ratio, double slope_exclusion_ratio, int tcap,
                                double* d_stats, double* d_top, double* d_scratch, void* stream) {
  PL_REQUIRE(d_x_indices && d_values && d_anchor && d_span && d_stats && d_top && d_scratch, "null pointer");
  PL_REQUIRE(n >= 0 && s >= 2 && tcap >= 1, "bad shape");
  PL_REQUIRE(s <= (1 << 21), "profile too long");
  if (n == 0) return PL_OK;
  PL_REQUIRE(n <= 0x7fffffffLL, "batch too large");
  hipLaunchKernelGGL(field_windows_kernel, dim3((unsigned)n), dim3(PL_WAVE), 0, (hipStream_t)stream, d_x_indices, d_values, s,
                     d_anchor, d_span, in_field_ratio, slope_exclusion_ratio, tcap, d_stats, d_top, d_scratch);
  return pl_check_launch("pl_field_windows");
}
