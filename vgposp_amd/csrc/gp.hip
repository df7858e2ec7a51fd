// Exact-GP log marginal likelihood and its gradient from the inverted Cholesky factor.
//
// Replaces, for tfd.GaussianProcess(kernel, X, noise).log_prob(y) (gp_functions.py:166-172,
// main.py:105, 3D_sin_wave.py:172) and the TF autodiff behind tf_train_gp_adam
// (gp_functions.py:179-182):
//     C = K + (noise + jitter) I = L L^T,   M = L^-1   (potrf.hip, invert=1)
//     z = M y,  LML = -0.5 |z|^2 - sum log L_ii - n/2 log(2 pi),  alpha = C^-1 y = M^T z
//     dLML/dtheta = 0.5 sum_ij (alpha alpha^T - C^-1)_ij dC_ij/dtheta
// The gradient pass regenerates dK/dtheta from X on the fly (no dK matrices in HBM) and reads the
// lower triangle of C^-1 once: it is HBM-bound at 4 n(n+1) bytes per batch entry.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "psd.h"

namespace vgposp {

constexpr double LOG_2PI = 1.8378770664093453;

// z[b][r] = sum_{c <= r} M[r][c] y[c]   (one wave per row)
__global__ __launch_bounds__(256) void trmv_rows_kernel(const double* M, int64_t n, int64_t lda,
                                                        int64_t stride, const double* y,
                                                        double* z) {
  const int b = blockIdx.y;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n) return;
  const double* row = M + b * stride + r * lda;
  double s = 0.0;
  for (int64_t c = lane; c <= r; c += 64) s += row[c] * y[c];
  s = wave_sum(s);
  if (lane == 0) z[b * n + r] = s;
}

// alpha[b][i] = sum_{r >= i} M[r][i] z[b][r]   (one thread per column, coalesced rows)
__global__ __launch_bounds__(256) void trmv_cols_kernel(const double* M, int64_t n, int64_t lda,
                                                        int64_t stride, const double* z,
                                                        double* alpha) {
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double* Mb = M + b * stride;
  const double* zb = z + b * n;
  double s0 = 0.0, s1 = 0.0;
  int64_t r = i;
  for (; r + 1 < n; r += 2) {
    s0 += Mb[r * lda + i] * zb[r];
    s1 += Mb[(r + 1) * lda + i] * zb[r + 1];
  }
  if (r < n) s0 += Mb[r * lda + i] * zb[r];
  alpha[b * n + i] = s0 + s1;
}

__device__ double block_sum_1024(double v) {
  __shared__ double sh[16];
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) sh[w] = v;
  __syncthreads();
  v = (l < (int)(blockDim.x >> 6)) ? sh[l] : 0.0;
  return wave_sum(v);
}

__global__ __launch_bounds__(1024) void lml_reduce_kernel(int64_t n, const double* z,
                                                          const double* Ldiag, double* out) {
  const int b = blockIdx.x;
  double q = 0.0, ld = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const double zi = z[b * n + i];
    q += zi * zi;
    ld += log(Ldiag[b * n + i]);
  }
  q = block_sum_1024(q);
  ld = block_sum_1024(ld);
  if (threadIdx.x == 0) out[b] = -0.5 * q - ld - 0.5 * (double)n * LOG_2PI;
}

// dK/damp and dK/dls at squared distance d2 (same formulas as kernel_matrix.hip).
__device__ __forceinline__ void kgrad(int kind, double d2, double a, double l, double& dka,
                                      double& dkl) {
  const double tla = 2.0 * log(a);
  double K;
  const double r0 = sqrt(d2);
  const double r = r0 / l;
  if (kind == VGPOSP_KERNEL_EQ) {
    K = exp(tla - 0.5 * d2 / (l * l));
    dkl = K * d2 / (l * l * l);
  } else if (kind == VGPOSP_KERNEL_MATERN12) {
    K = exp(tla - r);
    dkl = K * r / l;
  } else if (kind == VGPOSP_KERNEL_MATERN32) {
    const double s = 1.7320508075688772 * r;
    K = exp(tla + log1p(s) - s);
    dkl = a * a * exp(-s) * s * s / l;
  } else {
    const double s = 2.23606797749979 * r;
    K = exp(tla + log1p(s + s * s / 3.0) - s);
    dkl = a * a * exp(-s) * (s * s / 3.0) * (1.0 + s) / l;
  }
  dka = 2.0 * K / a;
}

constexpr int GR_ROWS = 16;

// Partial sums over 16-row stripes of the lower triangle:
//   part[b][blk] = (sum G dK/damp, sum G dK/dls, sum_i G_ii)   with symmetric weights.
__global__ __launch_bounds__(256) void lml_grad_kernel(int kind, const double* X, int64_t n,
                                                       int d, const double* amp,
                                                       const double* ls, const double* Cinv,
                                                       int64_t ldc, int64_t stride_c,
                                                       const double* alpha, double* part) {
  const int b = blockIdx.y;
  const double a = amp[b], l = ls[b];
  const double* Cb = Cinv + b * stride_c;
  const double* al = alpha + b * n;
  double sa = 0.0, sl = 0.0, sn = 0.0;
  const int64_t r0 = (int64_t)blockIdx.x * GR_ROWS;
  for (int rr = 0; rr < GR_ROWS; ++rr) {
    const int64_t i = r0 + rr;
    if (i >= n) break;
    const double ai = al[i];
    for (int64_t j = threadIdx.x; j <= i; j += 256) {
      double d2 = 0.0;
      for (int k = 0; k < d; ++k) {
        const double e = X[i * d + k] - X[j * d + k];
        d2 += e * e;
      }
      const double g = ai * al[j] - Cb[i * ldc + j];
      double dka, dkl;
      kgrad(kind, d2, a, l, dka, dkl);
      const double wgt = (j == i) ? 1.0 : 2.0;
      sa += wgt * g * dka;
      sl += wgt * g * dkl;
      if (j == i) sn += g;
    }
  }
  sa = wave_sum(sa);
  sl = wave_sum(sl);
  sn = wave_sum(sn);
  __shared__ double sh[3][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh[0][w] = sa;
    sh[1][w] = sl;
    sh[2][w] = sn;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const double v = sh[threadIdx.x][0] + sh[threadIdx.x][1] + sh[threadIdx.x][2] + sh[threadIdx.x][3];
    part[((int64_t)b * gridDim.x + blockIdx.x) * 3 + threadIdx.x] = v;
  }
}

__global__ __launch_bounds__(1024) void lml_grad_reduce_kernel(int64_t nblk, const double* part,
                                                               double* grad) {
  const int b = blockIdx.x;
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t e = threadIdx.x; e < nblk; e += blockDim.x)
    for (int q = 0; q < 3; ++q) s[q] += part[((int64_t)b * nblk + e) * 3 + q];
  for (int q = 0; q < 3; ++q) {
    const double v = block_sum_1024(s[q]);
    if (threadIdx.x == 0) grad[b * 3 + q] = 0.5 * v;
  }
}

// ---- the LML gradient of a FeatureScaled kernel ------------------------------------------------
// On points z = x / s (already divided): the three sums of lml_grad_kernel plus, per feature k,
//   sum G dK/ds_k = -(1 / s_k) sum G c(r) (z_ik - z_jk)^2      (c of psd.h's kvjp_entry),
// in the same pass over the lower triangle of C^-1.  A workgroup owns a 16-row stripe, whose points
// and alpha sit in LDS; a lane owns a column of each 256-column block and keeps that point and its
// alpha in registers for the 16 rows, so a point is read from global memory once per block and
// stripe, not once per entry.  Row by row the lanes read consecutive columns of C^-1 (coalesced).
constexpr int GS_MAXD = 8;

template <int KIND, int D>
__global__ __launch_bounds__(256) void lml_grad_scaled_kernel(const double* Z, int64_t n,
                                                              const double* amp, const double* ls,
                                                              const double* Cinv, int64_t ldc,
                                                              const double* alpha, double* part) {
  constexpr int NG = 3 + D;
  __shared__ double zr[GR_ROWS][D];
  __shared__ double ar[GR_ROWS];
  __shared__ double sh[NG][4];
  const int64_t r0 = (int64_t)blockIdx.x * GR_ROWS;
  const int rows = (int)min((int64_t)GR_ROWS, n - r0);
  for (int e = threadIdx.x; e < rows * D; e += 256) zr[e / D][e % D] = Z[r0 * D + e];
  if ((int)threadIdx.x < rows) ar[threadIdx.x] = alpha[r0 + threadIdx.x];
  __syncthreads();
  const double a = amp[0], l = ls[0];
  const double tla = 2.0 * log(a), inv_l = 1.0 / l, inv_l2 = inv_l * inv_l, two_over_a = 2.0 / a;
  double sa = 0.0, sl = 0.0, sn = 0.0, gs[D];
#pragma unroll
  for (int k = 0; k < D; ++k) gs[k] = 0.0;
  for (int64_t j = threadIdx.x; j < r0 + rows; j += 256) {
    double zj[D];
#pragma unroll
    for (int k = 0; k < D; ++k) zj[k] = Z[j * D + k];
    const double aj = alpha[j];
    // rows above column j (i < j) lie in the upper triangle: start at the first row i >= j
    for (int rr = (int)max((int64_t)0, j - r0); rr < rows; ++rr) {
      const int64_t i = r0 + rr;
      double diff[D], d2 = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        diff[k] = zr[rr][k] - zj[k];
        d2 += diff[k] * diff[k];
      }
      double K, dkl, cx;
      kvjp_entry<KIND>(d2, tla, inv_l, inv_l2, K, dkl, cx);
      const double g = ar[rr] * aj - Cinv[i * ldc + j];
      const double wg = (j == i ? 1.0 : 2.0) * g;
      sa += wg * K * two_over_a;
      sl += wg * dkl;
      if (j == i) sn += g;
      const double cf = wg * cx;
#pragma unroll
      for (int k = 0; k < D; ++k) gs[k] += cf * diff[k] * diff[k];
    }
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  sa = wave_sum(sa);
  sl = wave_sum(sl);
  sn = wave_sum(sn);
  if (lane == 0) {
    sh[0][w] = sa;
    sh[1][w] = sl;
    sh[2][w] = sn;
  }
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double v = wave_sum(gs[k]);
    if (lane == 0) sh[3 + k][w] = v;
  }
  __syncthreads();
  if (threadIdx.x < NG) {
    const double v = sh[threadIdx.x][0] + sh[threadIdx.x][1] + sh[threadIdx.x][2] + sh[threadIdx.x][3];
    part[(int64_t)blockIdx.x * NG + threadIdx.x] = v;
  }
}

// grad[q] = 0.5 sum over the stripes (fixed order), the scale entries times -1 / s_k.
__global__ __launch_bounds__(1024) void lml_grad_scaled_reduce_kernel(int64_t nblk, int d,
                                                                      const double* part,
                                                                      const double* scale,
                                                                      double* grad) {
  const int ng = 3 + d;
  for (int q = 0; q < ng; ++q) {
    double s = 0.0;
    for (int64_t e = threadIdx.x; e < nblk; e += blockDim.x) s += part[e * ng + q];
    const double v = block_sum_1024(s);
    if (threadIdx.x == 0) grad[q] = q < 3 ? 0.5 * v : -0.5 * v / scale[q - 3];
  }
}

template <int KIND>
static void launch_lml_grad_scaled(dim3 g, hipStream_t s, int d, const double* Z, int64_t n,
                                   const double* amp, const double* ls, const double* Cinv,
                                   int64_t ldc, const double* alpha, double* part) {
#define GS_CASE(DD)                                                                              \
  case DD:                                                                                       \
    hipLaunchKernelGGL((lml_grad_scaled_kernel<KIND, DD>), g, dim3(256), 0, s, Z, n, amp, ls,    \
                       Cinv, ldc, alpha, part);                                                  \
    break;
  switch (d) {
    GS_CASE(1) GS_CASE(2) GS_CASE(3) GS_CASE(4) GS_CASE(5) GS_CASE(6) GS_CASE(7) GS_CASE(8)
  }
#undef GS_CASE
}

// ---- row sums of squares (the marginal predictive variance) ----------------------------------
// s2 = diag(K_ss) - sum(Lk^2, axis=0) of plot_confidence_interval.py:51: the second term for a
// row-major strip V (one prediction point per row).  HBM / Infinity-Cache read-bound.
//
// A row belongs to a group of G lanes (G = 64: one wave per row; G = 32 / 16: two / four rows per
// wave for rows of at most 32 / 16 loads), and column c to lane (c / W) % G of its group (W = 2
// with 16-byte loads, 1 on the scalar path) whatever the grid, so a result does not depend on the
// launch geometry: four independent accumulators per lane in a fixed order, then the xor
// butterfly of wave_sum restricted to the group (steps G/2 ... 1; a group is never narrower than
// a 16-lane DPP row, below which the row_ror:4 step of common.h would no longer be lane ^ 4).
typedef double rs_d2v __attribute__((ext_vector_type(2)));

// Non-temporal loads: measured against plain loads (tools/bench_variance.py --alt-lib)
// they stream a 4 GiB strip 12 % faster and make no difference on a chunk strip that the GEMM
// has just left in the Infinity Cache.
#ifndef VG_ROWSUMSQ_NT
#define VG_ROWSUMSQ_NT 1
#endif

template <class T>
__device__ __forceinline__ T rs_load(const T* p) {
#if VG_ROWSUMSQ_NT
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}

template <int G>
__device__ __forceinline__ double group_sum(double v) {
  const auto add = [](double a, double b) { return a + b; };
  if constexpr (G >= 64) v = wave_step<32>(v, add);
  if constexpr (G >= 32) v = wave_step<16>(v, add);
  v = wave_step<8>(v, add);
  v = wave_step<4>(v, add);
  v = wave_step<2>(v, add);
  return wave_step<1>(v, add);
}

// This lane's share of sum_j p[j]^2, j < cols (gl = lane within the group).  VEC: p is 16-byte
// aligned.  Whole blocks of four loads per lane first (wave-uniform trip count, every load issued
// before the first use), then at most four predicated loads for the tail.
template <int G, bool VEC>
__device__ __forceinline__ double row_part(const double* __restrict__ p, int64_t cols, int gl) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if constexpr (VEC) {
    constexpr int64_t STEP = 2 * G;
    const int64_t pairs = cols & ~(int64_t)1;
    int64_t c = 0;
    for (; c + 4 * STEP <= pairs; c += 4 * STEP) {
      const rs_d2v* q = reinterpret_cast<const rs_d2v*>(p + c + 2 * gl);
      rs_d2v a[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = rs_load(q + u * G);
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] = fma(a[u].y, a[u].y, fma(a[u].x, a[u].x, s[u]));
    }
    rs_d2v a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t cc = c + 2 * gl + u * STEP;
      a[u] = rs_d2v{0.0, 0.0};
      if (cc < pairs) a[u] = rs_load(reinterpret_cast<const rs_d2v*>(p + cc));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] = fma(a[u].y, a[u].y, fma(a[u].x, a[u].x, s[u]));
    if (pairs < cols && gl == 0) {  // the odd last column
      const double x = p[pairs];
      s[1] = fma(x, x, s[1]);
    }
  } else {
    int64_t c = 0;
    for (; c + 4 * G <= cols; c += 4 * G) {
      double a[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = rs_load(p + c + gl + u * G);
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] = fma(a[u], a[u], s[u]);
    }
    double a[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t cc = c + gl + u * G;
      a[u] = 0.0;
      if (cc < cols) a[u] = rs_load(p + cc);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] = fma(a[u], a[u], s[u]);
  }
  return (s[0] + s[1]) + (s[2] + s[3]);
}

// out[i] = alpha sum_j V[i][j]^2 (+ beta out[i]).  Grid-stride over sets of RU * (64 / G) rows per
// wave: the RU row groups of a set are loaded together, so a wave with short rows still has
// several loads in flight.  A row index past the end is clamped for the loads and not stored, so
// every lane stays active through the butterflies.
template <int G, bool VEC, int RU>
__global__ __launch_bounds__(256) void row_sumsq_kernel(const double* __restrict__ V, int64_t rows,
                                                        int64_t cols, int64_t ldv, double alpha,
                                                        double beta, double* __restrict__ out) {
  constexpr int RPW = 64 / G;  // rows per wave and group
  const int lane = threadIdx.x & 63;
  const int gl = lane % G, sub = lane / G;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwave = (int64_t)gridDim.x * 4;
  const int64_t nset = (rows + RU * RPW - 1) / (RU * RPW);
  for (int64_t set = wave; set < nset; set += nwave) {
    double s[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int64_t i = min((set * RU + u) * RPW + sub, rows - 1);
      s[u] = row_part<G, VEC>(V + i * ldv, cols, gl);
    }
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const double t = group_sum<G>(s[u]);
      const int64_t i = (set * RU + u) * RPW + sub;
      if (gl == 0 && i < rows) out[i] = beta != 0.0 ? fma(alpha, t, beta * out[i]) : alpha * t;
    }
  }
}

template <int G, bool VEC, int RU>
static void launch_row_sumsq(hipStream_t s, const double* V, int64_t rows, int64_t cols,
                             int64_t ldv, double alpha, double beta, double* out) {
  constexpr int ROWS_PER_WG = 4 * RU * (64 / G);
  // capped: 8 workgroups of 4 waves per CU keep every SIMD's wave slots full on 256 CUs
  const int64_t nwg = std::min<int64_t>(ceil_div(rows, ROWS_PER_WG), 2048);
  hipLaunchKernelGGL((row_sumsq_kernel<G, VEC, RU>), dim3((unsigned)nwg), dim3(256), 0, s, V,
                     rows, cols, ldv, alpha, beta, out);
}

}  // namespace vgposp

using namespace vgposp;

extern "C" int vgposp_row_sumsq(const double* V, int64_t rows, int64_t cols, int64_t ldv,
                                double alpha, double beta, double* out, void* stream) {
  clear_error();
  VG_CHECK_ARG(rows >= 0, 2);
  VG_CHECK_ARG(cols >= 0, 3);
  VG_CHECK_ARG(ldv >= cols, 4);
  if (rows == 0) return 0;
  VG_CHECK_ARG(V != nullptr || cols == 0, 1);
  VG_CHECK_ARG(out != nullptr, 7);
  hipStream_t s = as_stream(stream);
  // 16-byte loads need every row start aligned: an aligned base and an even row stride
  const bool vec = (reinterpret_cast<uintptr_t>(V) % 16 == 0) && (ldv % 2 == 0);
  ProfScope ps("row_sumsq", s, 2.0 * (double)rows * (double)cols,
               8.0 * ((double)rows * (double)cols + (double)rows));
  // the group is as wide as a row has loads (a wave on a 64-column row of 16-byte loads would
  // leave half its lanes without one)
  const int64_t loads = vec ? (cols + 1) / 2 : cols;
  if (loads <= 16) {
    if (vec) launch_row_sumsq<16, true, 4>(s, V, rows, cols, ldv, alpha, beta, out);
    else launch_row_sumsq<16, false, 4>(s, V, rows, cols, ldv, alpha, beta, out);
  } else if (loads <= 32) {
    if (vec) launch_row_sumsq<32, true, 4>(s, V, rows, cols, ldv, alpha, beta, out);
    else launch_row_sumsq<32, false, 4>(s, V, rows, cols, ldv, alpha, beta, out);
  } else {
    if (vec) launch_row_sumsq<64, true, 2>(s, V, rows, cols, ldv, alpha, beta, out);
    else launch_row_sumsq<64, false, 2>(s, V, rows, cols, ldv, alpha, beta, out);
  }
  VG_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t vgposp_lml_workspace_bytes(int64_t n, int batch) {
  return (size_t)n * batch * sizeof(double);
}

extern "C" int vgposp_lml(const double* Minv, int64_t n, int64_t lda, int64_t stride, int batch,
                          const double* Ldiag, const double* y, double* alpha, double* out,
                          void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  VG_CHECK_ARG(Minv != nullptr, 1);
  VG_CHECK_ARG(n >= 1, 2);
  VG_CHECK_ARG(lda >= n, 3);
  VG_CHECK_ARG(batch >= 1 && batch <= 65535, 5);
  VG_CHECK_ARG(batch == 1 || stride >= lda * n, 4);
  VG_CHECK_ARG(Ldiag != nullptr, 6);
  VG_CHECK_ARG(y != nullptr, 7);
  VG_CHECK_ARG(out != nullptr, 9);
  VG_CHECK_ARG(ws != nullptr, 10);
  if (ws_bytes < vgposp_lml_workspace_bytes(n, batch)) {
    set_error("vgposp_lml: workspace too small");
    return VGPOSP_E_WS;
  }
  hipStream_t s = as_stream(stream);
  double* z = static_cast<double*>(ws);
  hipLaunchKernelGGL(trmv_rows_kernel, dim3((unsigned)ceil_div(n, 4), batch), dim3(256), 0, s,
                     Minv, n, lda, stride, y, z);
  VG_LAUNCH_CHECK();
  hipLaunchKernelGGL(lml_reduce_kernel, dim3(batch), dim3(1024), 0, s, n, z, Ldiag, out);
  VG_LAUNCH_CHECK();
  if (alpha) {
    hipLaunchKernelGGL(trmv_cols_kernel, dim3((unsigned)ceil_div(n, 256), batch), dim3(256), 0, s,
                       Minv, n, lda, stride, z, alpha);
    VG_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" size_t vgposp_lml_grad_workspace_bytes(int64_t n, int batch) {
  return (size_t)ceil_div(n, GR_ROWS) * batch * 3 * sizeof(double);
}

extern "C" int vgposp_lml_grad(int kind, const double* X, int64_t n, int d, const double* amp,
                               const double* ls, const double* Cinv, int64_t ldc,
                               int64_t stride_c, const double* alpha, int batch, double* grad,
                               void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  VG_CHECK_ARG(kind >= VGPOSP_KERNEL_EQ && kind <= VGPOSP_KERNEL_MATERN52, 1);
  VG_CHECK_ARG(X != nullptr, 2);
  VG_CHECK_ARG(n >= 1, 3);
  VG_CHECK_ARG(d >= 1, 4);
  VG_CHECK_ARG(amp != nullptr, 5);
  VG_CHECK_ARG(ls != nullptr, 6);
  VG_CHECK_ARG(Cinv != nullptr, 7);
  VG_CHECK_ARG(ldc >= n, 8);
  VG_CHECK_ARG(batch == 1 || stride_c >= ldc * n, 9);
  VG_CHECK_ARG(alpha != nullptr, 10);
  VG_CHECK_ARG(batch >= 1 && batch <= 65535, 11);
  VG_CHECK_ARG(grad != nullptr, 12);
  VG_CHECK_ARG(ws != nullptr, 13);
  if (ws_bytes < vgposp_lml_grad_workspace_bytes(n, batch)) {
    set_error("vgposp_lml_grad: workspace too small");
    return VGPOSP_E_WS;
  }
  hipStream_t s = as_stream(stream);
  const int64_t nblk = ceil_div(n, GR_ROWS);
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(lml_grad_kernel, dim3((unsigned)nblk, batch), dim3(256), 0, s, kind, X, n, d,
                     amp, ls, Cinv, ldc, stride_c, alpha, part);
  VG_LAUNCH_CHECK();
  hipLaunchKernelGGL(lml_grad_reduce_kernel, dim3(batch), dim3(1024), 0, s, nblk, part, grad);
  VG_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t vgposp_lml_grad_scaled_workspace_bytes(int64_t n) {
  if (n <= 0) return 0;
  return (size_t)ceil_div(n, GR_ROWS) * (3 + GS_MAXD) * sizeof(double);
}

extern "C" int vgposp_lml_grad_scaled(int kind, const double* Z, int64_t n, int d,
                                      const double* amp, const double* ls, const double* scale,
                                      const double* Cinv, int64_t ldc, const double* alpha,
                                      double* grad, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  VG_CHECK_ARG(kind >= VGPOSP_KERNEL_EQ && kind <= VGPOSP_KERNEL_MATERN52, 1);
  VG_CHECK_ARG(Z != nullptr, 2);
  VG_CHECK_ARG(n >= 1, 3);
  VG_CHECK_ARG(d >= 1 && d <= GS_MAXD, 4);
  VG_CHECK_ARG(amp != nullptr, 5);
  VG_CHECK_ARG(ls != nullptr, 6);
  VG_CHECK_ARG(scale != nullptr, 7);
  VG_CHECK_ARG(Cinv != nullptr, 8);
  VG_CHECK_ARG(ldc >= n, 9);
  VG_CHECK_ARG(alpha != nullptr, 10);
  VG_CHECK_ARG(grad != nullptr, 11);
  VG_CHECK_ARG(ws != nullptr, 12);
  VG_CHECK_WS(ws_bytes, vgposp_lml_grad_scaled_workspace_bytes(n));
  hipStream_t s = as_stream(stream);
  const int64_t nblk = ceil_div(n, GR_ROWS);
  double* part = static_cast<double*>(ws);
  const dim3 g((unsigned)nblk);
  switch (kind) {
    case VGPOSP_KERNEL_EQ: launch_lml_grad_scaled<VGPOSP_KERNEL_EQ>(g, s, d, Z, n, amp, ls, Cinv, ldc, alpha, part); break;
    case VGPOSP_KERNEL_MATERN12: launch_lml_grad_scaled<VGPOSP_KERNEL_MATERN12>(g, s, d, Z, n, amp, ls, Cinv, ldc, alpha, part); break;
    case VGPOSP_KERNEL_MATERN32: launch_lml_grad_scaled<VGPOSP_KERNEL_MATERN32>(g, s, d, Z, n, amp, ls, Cinv, ldc, alpha, part); break;
    default: launch_lml_grad_scaled<VGPOSP_KERNEL_MATERN52>(g, s, d, Z, n, amp, ls, Cinv, ldc, alpha, part); break;
  }
  VG_LAUNCH_CHECK();
  hipLaunchKernelGGL(lml_grad_scaled_reduce_kernel, dim3(1), dim3(1024), 0, s, nblk, d, part, scale,
                     grad);
  VG_LAUNCH_CHECK();
  return 0;
}
