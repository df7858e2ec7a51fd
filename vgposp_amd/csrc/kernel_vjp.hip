// Vector-Jacobian product of the PSD kernel matrix K(X1, X2) — the reverse pass of kernel assembly
// that TF autodiff runs through `kernel.matrix` when the reference trains a VGP
// (variational_Gaussian_process_example.py:95-102: AdamOptimizer.minimize over amplitude,
// length_scale and the inducing_index_points).  Given Kbar (+ an optional rank-1 term u w^T):
//   grad[0] = sum_ij Kbar_ij dK_ij/damp        = sum Kbar 2K/amp
//   grad[1] = sum_ij Kbar_ij dK_ij/dls
//   X1bar_i = sum_j  Kbar_ij dK_ij/dx1_i       = sum_j Kbar_ij c(r_ij) (x1_i - x2_j)
// K is recomputed, never read: one pass over Kbar, HBM-bound (8 B per entry).
//
// Layout: a workgroup owns 16 rows x 1024 columns; its X2 columns sit in LDS, each wave walks whole
// row segments (16 columns per lane, coalesced 512 B per row per wave) and keeps per-row X1bar
// sums in registers, so the cross-lane reduction happens once per 1024 entries.  Partials go to
// the workspace ([col-blocks][n1][d] and [blocks][2]) and a second kernel reduces them in a fixed
// order: results are deterministic.
//
// The scaled form (vgposp_kernel_vjp_scaled, FeatureScaled kernels) is the same kernel with D more
// accumulators per lane: on points z = x / s already divided by the per-feature scales,
//   dK_ij/ds_k = -c(r_ij) (z1_ik - z2_jk)^2 / s_k,
// so grad[2 + k] falls out of the same pass over Kbar; the reduce kernel applies the -1 / s_k, and
// the 1 / s_k that takes X1bar from z-space back to the unscaled X1.
#include "common.h"
#include "psd.h"

namespace vgposp {

constexpr int VJ_ROWS = 16;
constexpr int VJ_COLS = 1024;
constexpr int VJ_MAXD = 8;

template <int KIND, int D, bool SCALED>
__global__ __launch_bounds__(256) void kernel_vjp_kernel(const double* X1, int64_t n1,
                                                         const double* X2, int64_t n2,
                                                         const double* amp, const double* ls,
                                                         const double* Kbar, int64_t ldk,
                                                         const double* u, const double* w,
                                                         double* part_x, double* part_g) {
  constexpr int NG = SCALED ? 2 + D : 2;  // scalars per workgroup: amp, ls (and the D scales)
  __shared__ double x2s[VJ_COLS * D];
  __shared__ double red[NG][4];
  const int64_t c0 = (int64_t)blockIdx.x * VJ_COLS;
  const int64_t r0 = (int64_t)blockIdx.y * VJ_ROWS;
  for (int e = threadIdx.x; e < VJ_COLS * D; e += 256) {
    const int64_t col = c0 + e / D;
    x2s[e] = col < n2 ? X2[c0 * D + e] : 0.0;
  }
  __syncthreads();
  const double a = amp[0], l = ls[0];
  const double tla = 2.0 * log(a), inv_l = 1.0 / l, inv_l2 = inv_l * inv_l, two_over_a = 2.0 / a;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double ga = 0.0, gl = 0.0;
  double gs[D];
#pragma unroll
  for (int k = 0; k < D; ++k) gs[k] = 0.0;
  for (int rr = wave; rr < VJ_ROWS; rr += 4) {
    const int64_t i = r0 + rr;
    if (i >= n1) break;
    double x1[D], sx[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      x1[k] = X1[i * D + k];
      sx[k] = 0.0;
    }
    const double ui = u ? u[i] : 0.0;
    const double* krow = Kbar + i * ldk;
    for (int cc = lane; cc < VJ_COLS; cc += 64) {
      const int64_t j = c0 + cc;
      if (j >= n2) break;
      const double kb = krow[j] + (u ? ui * w[j] : 0.0);
      double diff[D], d2 = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        diff[k] = x1[k] - x2s[cc * D + k];
        d2 += diff[k] * diff[k];
      }
      double K, dkl, cx;
      kvjp_entry<KIND>(d2, tla, inv_l, inv_l2, K, dkl, cx);
      ga += kb * K * two_over_a;
      gl += kb * dkl;
      const double cf = kb * cx;
#pragma unroll
      for (int k = 0; k < D; ++k) sx[k] += cf * diff[k];
      if constexpr (SCALED) {
#pragma unroll
        for (int k = 0; k < D; ++k) gs[k] += cf * diff[k] * diff[k];
      }
    }
    if (part_x) {
#pragma unroll
      for (int k = 0; k < D; ++k) sx[k] = wave_sum(sx[k]);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) part_x[((int64_t)blockIdx.x * n1 + i) * D + k] = sx[k];
      }
    }
  }
  ga = wave_sum(ga);
  gl = wave_sum(gl);
  if (lane == 0) {
    red[0][wave] = ga;
    red[1][wave] = gl;
  }
  if constexpr (SCALED) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double v = wave_sum(gs[k]);
      if (lane == 0) red[2 + k][wave] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < NG) {
    const double v = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
    part_g[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * NG + threadIdx.x] = v;
  }
}

// X1bar[i][k] = sum over the column blocks of part_x[cb][i][k]: one wave per output, lanes stride
// over the blocks, fixed order (deterministic).  The last workgroup also reduces the ng scalars
// (2, or 2 + d with scales).  With `scale` (device [d]) X1bar is divided by s_k and the scale sums
// become grad[2 + k] = -sum / s_k.
__global__ __launch_bounds__(256) void kernel_vjp_reduce_kernel(int64_t n1, int d, int64_t ncb,
                                                                int64_t nblk, int ng,
                                                                const double* part_x,
                                                                const double* part_g,
                                                                const double* scale, double* grad,
                                                                double* X1bar) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t nout = X1bar ? n1 * d : 0;
  const int64_t nwg_x = (nout + 3) / 4;
  if ((int64_t)blockIdx.x < nwg_x) {
    const int64_t e = (int64_t)blockIdx.x * 4 + wv;
    if (e < nout) {
      double s = 0.0;
      for (int64_t cb = lane; cb < ncb; cb += 64) s += part_x[cb * n1 * d + e];
      s = wave_sum(s);
      if (scale) s /= scale[e % d];
      if (lane == 0) X1bar[e] = s;
    }
    return;
  }
  __shared__ double sh[2 + VJ_MAXD][4];
  for (int q = 0; q < ng; ++q) {
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < nblk; b += 256) s += part_g[ng * b + q];
    s = wave_sum(s);
    if (lane == 0) sh[q][wv] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < ng) {
    const int q = threadIdx.x;
    const double v = sh[q][0] + sh[q][1] + sh[q][2] + sh[q][3];
    grad[q] = q < 2 ? v : -v / scale[q - 2];
  }
}

int kernel_vjp_reduce_launch(int64_t n1, int d, int64_t ncb, int64_t nblk, int ng,
                             const double* part_x, const double* part_g, const double* scale,
                             double* grad, double* X1bar, hipStream_t s) {
  const int64_t nwg_x = X1bar ? ceil_div(n1 * d, 4) : 0;
  hipLaunchKernelGGL(kernel_vjp_reduce_kernel, dim3((unsigned)(nwg_x + 1)), dim3(256), 0, s, n1, d,
                     ncb, nblk, ng, part_x, part_g, scale, grad, X1bar);
  VG_LAUNCH_CHECK();
  return 0;
}

static void vjp_layout(int64_t n1, int64_t n2, int d, int ng, int64_t* ncb, int64_t* nrb,
                       size_t* bytes) {
  *ncb = ceil_div(n2, VJ_COLS);
  *nrb = ceil_div(n1, VJ_ROWS);
  *bytes = 8 * (size_t)((*ncb) * n1 * d + ng * (*ncb) * (*nrb)) + 256;
}

template <int KIND, bool SCALED>
static void launch_vjp(dim3 g, hipStream_t s, int d, const double* X1, int64_t n1,
                       const double* X2, int64_t n2, const double* amp, const double* ls,
                       const double* Kbar, int64_t ldk, const double* u, const double* w,
                       double* px, double* pg) {
#define VJ_CASE(DD)                                                                             \
  case DD:                                                                                      \
    hipLaunchKernelGGL((kernel_vjp_kernel<KIND, DD, SCALED>), g, dim3(256), 0, s, X1, n1, X2, n2, \
                       amp, ls, Kbar, ldk, u, w, px, pg);                                       \
    break;
  switch (d) {
    VJ_CASE(1) VJ_CASE(2) VJ_CASE(3) VJ_CASE(4) VJ_CASE(5) VJ_CASE(6) VJ_CASE(7) VJ_CASE(8)
  }
#undef VJ_CASE
}

template <bool SCALED>
static void launch_vjp_kind(int kind, dim3 g, hipStream_t s, int d, const double* X1, int64_t n1,
                            const double* X2, int64_t n2, const double* amp, const double* ls,
                            const double* Kbar, int64_t ldk, const double* u, const double* w,
                            double* px, double* pg) {
  switch (kind) {
    case VGPOSP_KERNEL_EQ: launch_vjp<VGPOSP_KERNEL_EQ, SCALED>(g, s, d, X1, n1, X2, n2, amp, ls, Kbar, ldk, u, w, px, pg); break;
    case VGPOSP_KERNEL_MATERN12: launch_vjp<VGPOSP_KERNEL_MATERN12, SCALED>(g, s, d, X1, n1, X2, n2, amp, ls, Kbar, ldk, u, w, px, pg); break;
    case VGPOSP_KERNEL_MATERN32: launch_vjp<VGPOSP_KERNEL_MATERN32, SCALED>(g, s, d, X1, n1, X2, n2, amp, ls, Kbar, ldk, u, w, px, pg); break;
    default: launch_vjp<VGPOSP_KERNEL_MATERN52, SCALED>(g, s, d, X1, n1, X2, n2, amp, ls, Kbar, ldk, u, w, px, pg); break;
  }
}

// Both entries after their argument checks: the pass over Kbar, then the fixed-order reduction.
// scale == nullptr is the isotropic entry (2 scalars per workgroup), else 2 + d.
static int vjp_run(int kind, const double* X1, int64_t n1, const double* X2, int64_t n2, int d,
                   const double* amp, const double* ls, const double* scale, const double* Kbar,
                   int64_t ldk, const double* u, const double* w, double* grad, double* X1bar,
                   void* ws, hipStream_t s) {
  const int ng = scale ? 2 + d : 2;
  int64_t ncb, nrb;
  size_t need;
  vjp_layout(n1, n2, d, ng, &ncb, &nrb, &need);
  double* px = static_cast<double*>(ws);
  double* pg = px + ncb * n1 * d;
  dim3 g((unsigned)ncb, (unsigned)nrb);
  {
    ProfScope ps(scale ? "kernel_vjp_scaled" : "kernel_vjp", s, 0.0,
                 8.0 * ((double)n1 * n2 + (double)(n1 + n2) * d));
    if (scale) launch_vjp_kind<true>(kind, g, s, d, X1, n1, X2, n2, amp, ls, Kbar, ldk, u, w, X1bar ? px : nullptr, pg);
    else launch_vjp_kind<false>(kind, g, s, d, X1, n1, X2, n2, amp, ls, Kbar, ldk, u, w, X1bar ? px : nullptr, pg);
    VG_LAUNCH_CHECK();
  }
  return kernel_vjp_reduce_launch(n1, d, ncb, ncb * nrb, ng, px, pg, scale, grad, X1bar, s);
}

static size_t vjp_bytes(int64_t n1, int64_t n2, int d, int ng) {
  if (n1 <= 0 || n2 <= 0 || d <= 0) return 0;
  int64_t ncb, nrb;
  size_t b;
  vjp_layout(n1, n2, d, ng, &ncb, &nrb, &b);
  return b;
}

}  // namespace vgposp

using namespace vgposp;

extern "C" size_t vgposp_kernel_vjp_workspace_bytes(int64_t n1, int64_t n2, int d) {
  return vjp_bytes(n1, n2, d, 2);
}

extern "C" int vgposp_kernel_vjp(int kind, const double* X1, int64_t n1, const double* X2,
                                 int64_t n2, int d, const double* amp, const double* ls,
                                 const double* Kbar, int64_t ldk, const double* u, const double* w,
                                 double* grad, double* X1bar, void* ws, size_t ws_bytes,
                                 void* stream) {
  clear_error();
  VG_CHECK_ARG(kind >= VGPOSP_KERNEL_EQ && kind <= VGPOSP_KERNEL_MATERN52, 1);
  VG_CHECK_ARG(X1 != nullptr, 2);
  VG_CHECK_ARG(n1 >= 1, 3);
  VG_CHECK_ARG(X2 != nullptr, 4);
  VG_CHECK_ARG(n2 >= 1, 5);
  VG_CHECK_ARG(d >= 1 && d <= VJ_MAXD, 6);
  VG_CHECK_ARG(amp != nullptr, 7);
  VG_CHECK_ARG(ls != nullptr, 8);
  VG_CHECK_ARG(Kbar != nullptr, 9);
  VG_CHECK_ARG(ldk >= n2, 10);
  VG_CHECK_ARG((u == nullptr) == (w == nullptr), 11);
  VG_CHECK_ARG(grad != nullptr, 13);
  VG_CHECK_ARG(ws != nullptr, 15);
  const size_t need = vjp_bytes(n1, n2, d, 2);
  if (ws_bytes < need) {
    set_error("vgposp_kernel_vjp: workspace %zu < %zu bytes", ws_bytes, need);
    return VGPOSP_E_WS;
  }
  return vjp_run(kind, X1, n1, X2, n2, d, amp, ls, nullptr, Kbar, ldk, u, w, grad, X1bar, ws,
                 as_stream(stream));
}

extern "C" size_t vgposp_kernel_vjp_scaled_workspace_bytes(int64_t n1, int64_t n2, int d) {
  return vjp_bytes(n1, n2, d, 2 + d);
}

extern "C" int vgposp_kernel_vjp_scaled(int kind, const double* Z1, int64_t n1, const double* Z2,
                                        int64_t n2, int d, const double* amp, const double* ls,
                                        const double* scale, const double* Kbar, int64_t ldk,
                                        const double* u, const double* w, double* grad,
                                        double* X1bar, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  VG_CHECK_ARG(kind >= VGPOSP_KERNEL_EQ && kind <= VGPOSP_KERNEL_MATERN52, 1);
  VG_CHECK_ARG(Z1 != nullptr, 2);
  VG_CHECK_ARG(n1 >= 1, 3);
  VG_CHECK_ARG(Z2 != nullptr, 4);
  VG_CHECK_ARG(n2 >= 1, 5);
  VG_CHECK_ARG(d >= 1 && d <= VJ_MAXD, 6);
  VG_CHECK_ARG(amp != nullptr, 7);
  VG_CHECK_ARG(ls != nullptr, 8);
  VG_CHECK_ARG(scale != nullptr, 9);
  VG_CHECK_ARG(Kbar != nullptr, 10);
  VG_CHECK_ARG(ldk >= n2, 11);
  VG_CHECK_ARG((u == nullptr) == (w == nullptr), 12);
  VG_CHECK_ARG(grad != nullptr, 14);
  VG_CHECK_ARG(ws != nullptr, 16);
  VG_CHECK_WS(ws_bytes, vjp_bytes(n1, n2, d, 2 + d));
  return vjp_run(kind, Z1, n1, Z2, n2, d, amp, ls, scale, Kbar, ldk, u, w, grad, X1bar, ws,
                 as_stream(stream));
}
