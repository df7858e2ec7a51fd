// Greedy sensor placement by variance reduction (A-optimal) and by entropy, all on device: the two
// rules Krause, Singh & Guestrin compare the mutual-information placement (greedy.hip) with.
//
// Sigma = cov_vv (n x n, symmetric PSD), A the sensors chosen so far (`placed` first), and
//   C = Sigma - Sigma_{:,A} Sigma_AA^-1 Sigma_{A,:}         the conditional covariance given A.
// Per round, for every y:
//   variance:  delta_y = sum_{v in T} C_vy^2 / C_yy   ( = tr_T(C) - tr_T(C after adding y): the
//              deltas of a run sum to the total reduction of the targets' posterior variance)
//   entropy:   delta_y = C_yy
//   C_yy < threshold -> delta_y = 0 (both rules).  The arg-max runs over S \ A (S the candidates),
//   ties to the LOWER index (wave_keymax).  Every round scores every free candidate: there is no
//   lazy cache, the variance rule is not submodular.
// Nothing is factored: the state is nom_y = C_yy, s_y = sum_{v in T} C_vy^2 and the rows W of the
// pivoted Cholesky of Sigma given A (W_u = C^{(u)}_{a_u,:} / sqrt(C^{(u)}_{a_u a_u}), so that
// C = Sigma - W^T W).  With a the pick, w the new row and t the 0/1 target mask, a round does
//   1. w_y   = (Sigma_ay - sum_u W_u[a] W_u[y]) / sqrt(nom_a)
//   2. g     = Sigma (w.t) - W^T (W (w.t))                    the one pass over Sigma
//   3. s_y  -= 2 w_y g_y - w_y^2 |w.t|^2
//   4. nom_y -= w_y^2
// from s_y = sum_{v in T} Sigma_vy^2, nom = diag Sigma.  Entropy needs 1 and 4 only.
//
// Only the entries j >= i of Sigma are read, and `diag` (when given) replaces its diagonal: that is
// what a buffer factored in place by vgposp_greedy_init still holds (Sigma strictly above the
// diagonal, L^-1 below), so the rules run on the MI path's buffer without a second copy of Sigma.
// The heavy step is vgposp_symv_upper: y = Sigma x from the upper triangle, every element loaded
// once and used for y_i and for y_j.  No float atomics anywhere: partial sums go to the workspace
// and are reduced in a fixed order, so two runs are bit-identical; nothing synchronises the host.
//
// Sigma need not be stored: for Sigma = diag(a) K(X, X) diag(a) + a diagonal vector the same
// rounds run with every entry generated from the points (SGen, ksymv_kernel, the critg / critgk
// entries).  The third source is a factor: Sigma = F F^T + diag(noise) with F [n][S] the centred
// samples of an empirical covariance (SFactor, the critf entries): a pass is two tall-skinny
// streams over F.  The targets may lie outside V, with their cross-covariance R stored
// (CrossStored) or generated (KGen).  On a factor with noise > 0 everywhere the mutual-information
// rule runs too, through Woodbury's identity (FmiWS, the fmi entries at the end of the namespace).
//
// The host side is written once: one start (crit_init_run) and one round (crit_step_run), both
// templates on where Sigma comes from (SigmaStored, SGen, SFactor) and on where the targets are
// (InV, CrossStored, KGen); every _init and _step entry of the six families checks its argument
// groups (check_sigma, check_cross, check_rule, check_round), lays out its workspace and calls
// them.
#include <algorithm>
#include <cfloat>
#include <type_traits>

#include "common.h"
#include "dense.h"
#include "psd.h"

namespace vgposp {

constexpr int SY_T = 512;     // rows and columns of a mat-vec tile
constexpr int SY_TH = 256;    // threads of a tile: one column pair each
constexpr int CR_CH = 1024;   // candidates per scoring workgroup
constexpr int CR_B = 256;     // elements per workgroup of the O(n t) kernels
constexpr int64_t CR_NMAX = (int64_t)1 << 21;

static size_t cr_align(size_t x) { return (x + 255) & ~(size_t)255; }

struct SymvWS {
  double *cpart, *rpart;  // [nt][n] each: column-direction sums per row tile, row-direction sums
  size_t bytes;           // per column tile
};

static SymvWS symv_layout(void* base, int64_t n) {
  SymvWS w{};
  const size_t slab = cr_align((size_t)ceil_div(n, SY_T) * n * 8);
  char* p = static_cast<char*>(base);
  w.cpart = (double*)p;
  w.rpart = (double*)(p ? p + slab : nullptr);
  w.bytes = 2 * slab;
  return w;
}

// One tile (bi, bj), bj >= bi, of y = A x for symmetric A given by its upper triangle:
//   cpart[bi][c] = sum_{r in tile rows, r <= c} e(r, c) x[r]        (towards y_c)
//   rpart[bj][r] = sum_{c in tile columns, c > r} e(r, c) x[c]      (towards y_r)
// e = A[r][c] (SQ: its square), the diagonal entry taken from `diag` when given and counted once,
// in the column sum.  Each thread owns the column pair (c, c + 1): one 16-byte non-temporal load
// per row (VEC: even lda, 16-byte aligned base; else two 8-byte loads), four rows in flight; its
// column sums stay in registers over the tile's rows, the row sums are wave reductions, one per
// row, collected in LDS and written once per tile (waves summed in a fixed order).  Below the
// diagonal nothing is loaded: in the diagonal tile a lane loads row r only for r < c, and the
// three entries (c, c), (c, c + 1), (c + 1, c + 1) of its pair one by one.  DT: the diagonal tile.
static_assert(SY_T == 2 * SY_TH && SY_TH == 256, "a column pair per thread, four waves per tile");

template <bool SQ, bool VEC, bool DT>
__device__ __forceinline__ void symv_tile(const double* __restrict__ A, int64_t n, int64_t lda,
                                          const double* __restrict__ diag,
                                          const double* __restrict__ x, int64_t r0, int64_t r1,
                                          int64_t c, double* __restrict__ cout,
                                          double* __restrict__ rout, double (*rows)[SY_T]) {
  typedef double d2v __attribute__((ext_vector_type(2)));
  const bool in0 = c < n, in1 = c + 1 < n;
  const double x0 = in0 ? x[c] : 0.0, x1 = in1 ? x[c + 1] : 0.0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double s0 = 0.0, s1 = 0.0, u0 = 0.0, u1 = 0.0;  // column c: s0 + s1, column c + 1: u0 + u1
  // the pair (r, c), (r, c + 1), zero where it is not an entry strictly above the diagonal
  auto load = [&](int64_t r) -> d2v {
    d2v m = {0.0, 0.0};
    if (!in0 || (DT && r > c)) return m;
    const double* p = A + r * lda + c;
    if (DT && r == c) {  // (c, c) is added after the loop; (c, c + 1) alone
      if (in1) m.y = p[1];
      return m;
    }
    if (VEC && in1) return __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p));
    m.x = __builtin_nontemporal_load(p);
    if (in1) m.y = __builtin_nontemporal_load(p + 1);
    return m;
  };
  auto row = [&](d2v m, int64_t r, double& a, double& b) {
    if (SQ) m = m * m;
    const double xr = x[r];
    a = fma(m.x, xr, a);
    b = fma(m.y, xr, b);
    const double v = wave_sum(fma(m.x, x0, m.y * x1));
    if (lane == 0) rows[wv][r - r0] = v;
  };
  int64_t r = r0;
  for (; r + 3 < r1; r += 4) {
    const d2v m0 = load(r), m1 = load(r + 1), m2 = load(r + 2), m3 = load(r + 3);
    row(m0, r, s0, u0);
    row(m1, r + 1, s1, u1);
    row(m2, r + 2, s0, u0);
    row(m3, r + 3, s1, u1);
  }
  for (; r < r1; ++r) row(load(r), r, s0, u0);
  double sc = s0 + s1, uc = u0 + u1;
  if (DT && in0) {  // the two diagonal entries of the pair: counted once, in the column sums
    double d00 = diag ? diag[c] : A[c * lda + c];
    if (SQ) d00 *= d00;
    sc = fma(d00, x0, sc);
    if (in1) {
      double d11 = diag ? diag[c + 1] : A[(c + 1) * lda + c + 1];
      if (SQ) d11 *= d11;
      uc = fma(d11, x1, uc);
    }
  }
  if (in0) cout[c] = sc;
  if (in1) cout[c + 1] = uc;
  __syncthreads();
  for (int64_t i = threadIdx.x; i < r1 - r0; i += SY_TH)
    rout[r0 + i] = (rows[0][i] + rows[1][i]) + (rows[2][i] + rows[3][i]);
}

// gate: a device flag or NULL; the kernel does nothing when *gate != 0 (the entropy rule's rounds).
template <bool SQ, bool VEC>
__global__ __launch_bounds__(SY_TH) void symv_upper_kernel(
    const double* __restrict__ A, int64_t n, int64_t lda, const double* __restrict__ diag,
    const double* __restrict__ x, SymvWS w, const double* __restrict__ gate) {
  __shared__ double rows[SY_TH / 64][SY_T];  // the waves' row sums
  const int64_t bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;  // below the diagonal
  if (gate && *gate != 0.0) return;
  const int64_t r0 = bi * SY_T, r1 = min(r0 + SY_T, n);
  const int64_t c = bj * SY_T + 2 * threadIdx.x;
  if (bi == bj)
    symv_tile<SQ, VEC, true>(A, n, lda, diag, x, r0, r1, c, w.cpart + bi * n, w.rpart + bj * n,
                             rows);
  else
    symv_tile<SQ, VEC, false>(A, n, lda, diag, x, r0, r1, c, w.cpart + bi * n, w.rpart + bj * n,
                              rows);
}

// y_i = (sum of the column-direction partials of the row tiles 0 .. i / SY_T, ascending)
//     + (sum of the row-direction partials of the column tiles i / SY_T .. nt - 1, ascending)
__global__ __launch_bounds__(CR_B) void symv_reduce_kernel(int64_t n, SymvWS w,
                                                           double* __restrict__ y,
                                                           const double* __restrict__ gate) {
  if (gate && *gate != 0.0) return;
  const int64_t i = (int64_t)blockIdx.x * CR_B + threadIdx.x;
  if (i >= n) return;
  const int64_t nt = (n + SY_T - 1) / SY_T, ti = i / SY_T;
  double cs = 0.0, rs = 0.0;
  for (int64_t b = 0; b <= ti; ++b) cs += w.cpart[b * n + i];
  for (int64_t b = ti; b < nt; ++b) rs += w.rpart[b * n + i];
  y[i] = cs + rs;
}

static bool symv_vec(const double* A, int64_t lda) {
  return (reinterpret_cast<uintptr_t>(A) % 16 == 0) && (lda % 2 == 0);
}

template <bool SQ>
static void symv_launch(const double* A, int64_t n, int64_t lda, const double* diag,
                        const double* x, double* y, const SymvWS& w, const double* gate,
                        hipStream_t s) {
  const unsigned nt = (unsigned)ceil_div(n, SY_T);
  {
    const double tri = 0.5 * (double)n * (n + 1);
    ProfScope ps(SQ ? "criteria_symv_sq" : "criteria_symv", s, (SQ ? 5.0 : 4.0) * tri, 8.0 * tri);
    if (symv_vec(A, lda))
      hipLaunchKernelGGL((symv_upper_kernel<SQ, true>), dim3(nt, nt), dim3(SY_TH), 0, s, A, n, lda,
                         diag, x, w, gate);
    else
      hipLaunchKernelGGL((symv_upper_kernel<SQ, false>), dim3(nt, nt), dim3(SY_TH), 0, s, A, n,
                         lda, diag, x, w, gate);
  }
  hipLaunchKernelGGL(symv_reduce_kernel, dim3((unsigned)ceil_div(n, CR_B)), dim3(CR_B), 0, s, n, w,
                     y, gate);
}

// ---- the greedy rounds ----
// prm (device): [0] threshold, [1] criterion (the gate of the variance-only kernels: non-zero for
// entropy).  piv: [0] nom_a of the pick, [1 + u] W_u[a].  dot: [u] = W_u . (w.t) for u <= round
// (u = round: |w.t|^2), from the per-workgroup partials dpart[u][chunk].
struct CritWS {
  double *prm, *nom, *s, *delta, *W, *wt, *g, *tvec, *piv, *dot, *dpart, *fval;
  long long* fidx;
  unsigned char* selmask;
  void* symv;
  size_t bytes;
};

// pass_bytes: the partials of the pass over Sigma (symv_layout for a stored Sigma, ksymv_layout for
// a generated one, 0 where the rounds never pass over it).
static CritWS crit_layout(void* base, int64_t n, int kmax, size_t pass_bytes) {
  CritWS w{};
  const int64_t nb = ceil_div(n, CR_B), nch = ceil_div(n, CR_CH);
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = p ? p + off : nullptr;
    off += cr_align(bytes);
    return r;
  };
  w.prm = (double*)take(8 * 8);
  w.nom = (double*)take(n * 8);
  w.s = (double*)take(n * 8);
  w.delta = (double*)take(n * 8);
  w.W = (double*)take((size_t)kmax * n * 8);
  w.wt = (double*)take(n * 8);
  w.g = (double*)take(n * 8);
  w.tvec = (double*)take(n * 8);
  w.piv = (double*)take((1 + (size_t)kmax) * 8);
  w.dot = (double*)take((size_t)kmax * 8);
  w.dpart = (double*)take((size_t)kmax * nb * 8);
  w.fval = (double*)take(nch * 8);
  w.fidx = (long long*)take(nch * 8);
  w.selmask = (unsigned char*)take(n);
  w.symv = take(pass_bytes);
  w.bytes = off;
  return w;
}

static CritWS crit_layout(void* base, int64_t n, int kmax) {
  return crit_layout(base, n, kmax, symv_layout(nullptr, n).bytes);
}

// Block-wide (value, index) arg-max for blockDim == 1024; the result is valid in all threads.
__device__ __forceinline__ void crit_block_keymax(double& v, long long& i) {
  __shared__ double sv[16];
  __shared__ long long si[16];
  wave_keymax(v, i);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) {
    sv[w] = v;
    si[w] = i;
  }
  __syncthreads();
  v = (l < 16) ? sv[l] : -DBL_MAX;
  i = (l < 16) ? si[l] : -1;
  wave_keymax(v, i);
}

// Block-wide sum for blockDim == CR_B, waves added in a fixed order; valid in all threads.
__device__ __forceinline__ double crit_block_sum(double v) {
  __shared__ double sw[CR_B / 64];
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sw[0] + sw[1]) + (sw[2] + sw[3]);
}
static_assert(CR_B == 256, "crit_block_sum adds four waves");

__global__ void crit_init_kernel(const double* S, int64_t n, int64_t lda, const double* diag,
                                 int criterion, double thr, const unsigned char* targets,
                                 const unsigned char* allowed, CritWS w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    w.nom[i] = diag ? diag[i] : S[i * lda + i];
    w.tvec[i] = (!targets || targets[i]) ? 1.0 : 0.0;
    w.selmask[i] = (allowed && !allowed[i]) ? 1 : 0;
    w.delta[i] = 0.0;
    if (criterion != VGPOSP_CRIT_VARIANCE) w.s[i] = 0.0;
  }
  if (i == 0) {
    w.prm[0] = thr;
    w.prm[1] = criterion == VGPOSP_CRIT_VARIANCE ? 0.0 : 1.0;
  }
}

// delta for every location, and the best key of the workgroup over the free candidates.
__global__ __launch_bounds__(CR_CH) void crit_score_kernel(int64_t n, CritWS w) {
  const int64_t i = (int64_t)blockIdx.x * CR_CH + threadIdx.x;
  const double thr = w.prm[0];
  const bool entropy = w.prm[1] != 0.0;
  double bv = -DBL_MAX;
  long long bi = -1;
  if (i < n) {
    const double nom = w.nom[i];
    const double d = nom < thr ? 0.0 : (entropy ? nom : w.s[i] / nom);
    w.delta[i] = d;
    if (!w.selmask[i]) {
      bv = d;
      bi = i;
    }
  }
  crit_block_keymax(bv, bi);
  if (threadIdx.x == 0) {
    w.fval[blockIdx.x] = bv;
    w.fidx[blockIdx.x] = bi;
  }
}

// One workgroup: the arg-max over the chunk keys, or forced[j]; then the pivot data of the pick.
// No candidate left: selected[round] = -1, and the update kernels of the round do nothing.
__global__ __launch_bounds__(CR_CH) void crit_select_kernel(int64_t n, int round,
                                                            const int64_t* forced, int64_t j,
                                                            int64_t* selected, double* sel_delta,
                                                            CritWS w) {
  const int64_t nch = (n + CR_CH - 1) / CR_CH;
  double v = -DBL_MAX;
  long long y = -1;
  if (forced) {
    y = min(max(forced[j], (int64_t)0), n - 1);  // validated by the host; never outside
  } else {
    for (int64_t e = threadIdx.x; e < nch; e += blockDim.x) {
      if (w.fidx[e] >= 0 && key_gt(w.fval[e], w.fidx[e], v, y)) {
        v = w.fval[e];
        y = w.fidx[e];
      }
    }
    crit_block_keymax(v, y);
  }
  if (threadIdx.x == 0) {
    selected[round] = y;
    if (sel_delta) sel_delta[round] = y >= 0 ? w.delta[y] : 0.0;
    if (y >= 0) {
      w.selmask[y] = 1;
      w.piv[0] = w.nom[y];
    }
  }
  if (y >= 0)
    for (int t = threadIdx.x; t < round; t += blockDim.x) w.piv[1 + t] = w.W[(int64_t)t * n + y];
}

// Step 1 and 4: the new row w of W, w.t, and nom -= w^2.  Sigma_ay comes from the upper triangle
// (column a above row a, row a beyond it).  A pick whose conditional variance is below the
// threshold adds nothing: w = 0.
__global__ __launch_bounds__(CR_B) void crit_row_kernel(const double* S, int64_t n, int64_t lda,
                                                        const double* diag,
                                                        const int64_t* selected, int round,
                                                        CritWS w) {
  const int64_t i = (int64_t)blockIdx.x * CR_B + threadIdx.x;
  const int64_t a = selected[round];
  if (i >= n || a < 0) return;
  double s = i < a ? S[i * lda + a] : (i > a ? S[a * lda + i] : (diag ? diag[a] : S[a * lda + a]));
  for (int t = 0; t < round; ++t) s -= w.piv[1 + t] * w.W[(int64_t)t * n + i];
  const double noma = w.piv[0];
  const double wy = noma >= w.prm[0] && noma > 0.0 ? s / sqrt(noma) : 0.0;
  w.W[(int64_t)round * n + i] = wy;
  w.wt[i] = wy * w.tvec[i];
  w.nom[i] -= wy * wy;
}

// dpart[u][chunk] = sum over the chunk of W_u[i] (w.t)_i, u = blockIdx.y <= round.
__global__ __launch_bounds__(CR_B) void crit_dots_kernel(int64_t n, const int64_t* selected,
                                                         int round, CritWS w) {
  if (w.prm[1] != 0.0 || selected[round] < 0) return;
  const int64_t i = (int64_t)blockIdx.x * CR_B + threadIdx.x;
  const int u = blockIdx.y;
  double v = i < n ? w.W[(int64_t)u * n + i] * w.wt[i] : 0.0;
  v = crit_block_sum(v);
  if (threadIdx.x == 0) w.dpart[(int64_t)u * gridDim.x + blockIdx.x] = v;
}

// dot[u] = the chunks of dpart[u] in a fixed order: strided per thread, then the block sum.
__global__ __launch_bounds__(CR_B) void crit_fold_kernel(int64_t nb, const int64_t* selected,
                                                         int round, CritWS w) {
  if (w.prm[1] != 0.0 || selected[round] < 0) return;
  const int u = blockIdx.x;
  double v = 0.0;
  for (int64_t e = threadIdx.x; e < nb; e += CR_B) v += w.dpart[(int64_t)u * nb + e];
  v = crit_block_sum(v);
  if (threadIdx.x == 0) w.dot[u] = v;
}

// Step 2 (second half) and 3: g = Sigma (w.t) - W^T dot, s -= 2 w g - w^2 |w.t|^2.
__global__ __launch_bounds__(CR_B) void crit_update_kernel(int64_t n, const int64_t* selected,
                                                           int round, CritWS w) {
  if (w.prm[1] != 0.0 || selected[round] < 0) return;
  const int64_t i = (int64_t)blockIdx.x * CR_B + threadIdx.x;
  if (i >= n) return;
  double g = w.g[i];
  for (int t = 0; t < round; ++t) g -= w.dot[t] * w.W[(int64_t)t * n + i];
  w.g[i] = g;
  const double wy = w.W[(int64_t)round * n + i];
  w.s[i] -= 2.0 * wy * g - wy * wy * w.dot[round];
}

// ---- targets outside V: the variance rule on a rectangular cross-covariance ----
// R = cross_cov (P x n, row-major, pitch ldr >= n, only read): the covariance between the P targets
// and the n locations; omega [P] >= 0 the targets' weights.  With D = R - R_{:,A} Sigma_AA^-1
// Sigma_{A,:} the rule is delta_y = sum_v omega_v D_vy^2 / C_yy.  The state gains the target-side
// rows U [kmax][P] (D = R - U^T W); with a the pick, a round does
//   1. w_y as above
//   2. u_v   = (R_va - sum_t U_t[v] W_t[a]) / sqrt(nom_a)          (0 when nom_a < threshold)
//   3. g     = R^T (omega.u) - W^T (U (omega.u))                   the one pass over R
//   4. s_y  -= 2 w_y g_y - w_y^2 sum_v omega_v u_v^2
//   5. nom_y -= w_y^2
// from s_y = sum_v omega_v R_vy^2, nom = diag Sigma.  sum_r U_r[v]^2 is the variance removed at v.
// The location side is the CritWS of the in-V rule with t = 1, so scoring, selection, the w-row
// and the update are its kernels; the dots U_t . (omega.u) are crit_dots / crit_fold on a view of
// the workspace whose W / wt / dpart are the target side's U / omega.u / partials (n -> P).
constexpr int64_t CRX_PMAX = (int64_t)1 << 24;  // 32,768 row tiles: within a grid's y extent

static size_t gemv_t_bytes(int64_t P, int64_t n) {
  return cr_align((size_t)ceil_div(P, SY_T) * n * 8);
}

// One 512 x 512 tile of y = R^T x (SQ: of the squared entries): symv_tile without its row-direction
// half.  part[blockIdx.y][c] = sum over the tile's rows of e(r, c) x[r]; a thread owns the column
// pair (c, c + 1), one 16-byte non-temporal load per row (VEC) or two 8-byte ones, four rows in
// flight, x[r] workgroup-uniform, the two column sums in registers.  Nothing is shared between
// threads, so there is no LDS and no barrier.
template <bool SQ, bool VEC>
__global__ __launch_bounds__(SY_TH) void gemv_t_kernel(const double* __restrict__ R, int64_t P,
                                                       int64_t n, int64_t ldr,
                                                       const double* __restrict__ x,
                                                       double* __restrict__ part,
                                                       const double* __restrict__ gate) {
  typedef double d2v __attribute__((ext_vector_type(2)));
  if (gate && *gate != 0.0) return;
  const int64_t r0 = (int64_t)blockIdx.y * SY_T, r1 = min(r0 + SY_T, P);
  const int64_t c = (int64_t)blockIdx.x * SY_T + 2 * threadIdx.x;
  if (c >= n) return;
  const bool in1 = c + 1 < n;
  auto load = [&](int64_t r) -> d2v {
    const double* p = R + r * ldr + c;
    if (VEC && in1) return __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p));
    d2v m = {__builtin_nontemporal_load(p), 0.0};
    if (in1) m.y = __builtin_nontemporal_load(p + 1);
    return m;
  };
  auto row = [&](d2v m, int64_t r, double& a, double& b) {
    if (SQ) m = m * m;
    const double xr = x[r];
    a = fma(m.x, xr, a);
    b = fma(m.y, xr, b);
  };
  double s0 = 0.0, s1 = 0.0, u0 = 0.0, u1 = 0.0;  // column c: s0 + s1, column c + 1: u0 + u1
  int64_t r = r0;
  for (; r + 3 < r1; r += 4) {
    const d2v m0 = load(r), m1 = load(r + 1), m2 = load(r + 2), m3 = load(r + 3);
    row(m0, r, s0, u0);
    row(m1, r + 1, s1, u1);
    row(m2, r + 2, s0, u0);
    row(m3, r + 3, s1, u1);
  }
  for (; r < r1; ++r) row(load(r), r, s0, u0);
  double* out = part + (int64_t)blockIdx.y * n;
  out[c] = s0 + s1;
  if (in1) out[c + 1] = u0 + u1;
}

// y_j = the partials of the row tiles 0 .. nt - 1, ascending; with `scale` (the matrix-free pass)
// times scale_j, or scale_j^2 when sq.
__global__ __launch_bounds__(CR_B) void gemv_t_reduce_kernel(int64_t nt, int64_t n,
                                                             const double* __restrict__ part,
                                                             double* __restrict__ y,
                                                             const double* __restrict__ gate,
                                                             const double* scale = nullptr,
                                                             int sq = 0) {
  if (gate && *gate != 0.0) return;
  const int64_t j = (int64_t)blockIdx.x * CR_B + threadIdx.x;
  if (j >= n) return;
  double s = 0.0;
#pragma unroll 8
  for (int64_t b = 0; b < nt; ++b) s += part[b * n + j];
  if (scale) s *= sq ? scale[j] * scale[j] : scale[j];
  y[j] = s;
}

template <bool SQ>
static void gemv_t_launch(const double* R, int64_t P, int64_t n, int64_t ldr, const double* x,
                          double* y, double* part, const double* gate, hipStream_t s) {
  const unsigned ntr = (unsigned)ceil_div(P, SY_T), ntc = (unsigned)ceil_div(n, SY_T);
  {
    const double pn = (double)P * (double)n;
    ProfScope ps(SQ ? "criteria_gemv_t_sq" : "criteria_gemv_t", s, (SQ ? 3.0 : 2.0) * pn,
                 8.0 * pn);
    if (symv_vec(R, ldr))
      hipLaunchKernelGGL((gemv_t_kernel<SQ, true>), dim3(ntc, ntr), dim3(SY_TH), 0, s, R, P, n,
                         ldr, x, part, gate);
    else
      hipLaunchKernelGGL((gemv_t_kernel<SQ, false>), dim3(ntc, ntr), dim3(SY_TH), 0, s, R, P, n,
                         ldr, x, part, gate);
  }
  hipLaunchKernelGGL(gemv_t_reduce_kernel, dim3((unsigned)ceil_div(n, CR_B)), dim3(CR_B), 0, s,
                     (int64_t)ntr, n, part, y, gate);
}

// c: the location side (its tvec all ones, its dot shared with the target side).  wu = omega.u;
// dpart [kmax][ceil(P / CR_B)]: the partials of the dots over P; gemv: the partials of the pass.
struct CritXWS {
  CritWS c;
  double *U, *wu, *omega, *dpart, *gemv;
  size_t bytes;
};

// part_bytes: the partials of the pass (gemv_t_bytes for a stored R, kgemv_t_bytes for a generated
// one).  sigma_bytes: crit_layout's pass_bytes; a stored Sigma keeps the area of its in-V rule.
static CritXWS critx_layout(void* base, int64_t n, int64_t P, int kmax, size_t part_bytes,
                            size_t sigma_bytes) {
  CritXWS w{};
  w.c = crit_layout(base, n, kmax, sigma_bytes);
  char* p = static_cast<char*>(base);
  size_t off = w.c.bytes;
  auto take = [&](size_t bytes) {
    char* r = p ? p + off : nullptr;
    off += cr_align(bytes);
    return (double*)r;
  };
  w.U = take((size_t)kmax * P * 8);
  w.wu = take((size_t)P * 8);
  w.omega = take((size_t)P * 8);
  w.dpart = take((size_t)kmax * ceil_div(P, CR_B) * 8);
  w.gemv = take(part_bytes);
  w.bytes = off;
  return w;
}

static CritXWS critx_layout(void* base, int64_t n, int64_t P, int kmax, size_t part_bytes) {
  return critx_layout(base, n, P, kmax, part_bytes, symv_layout(nullptr, n).bytes);
}

// The workspace as crit_dots / crit_fold see the target side: rows U, vector omega.u, length P.
static CritWS critx_target_view(const CritXWS& w) {
  CritWS t = w.c;
  t.W = w.U;
  t.wt = w.wu;
  t.dpart = w.dpart;
  return t;
}

__global__ void critx_init_kernel(int64_t P, const double* weights, CritXWS w) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < P) w.omega[v] = weights ? weights[v] : 1.0;
}

// Step 2: the new row u of U and omega.u; R_va is a strided read of column a.  As crit_row_kernel:
// a pick below the threshold adds nothing.
__global__ __launch_bounds__(CR_B) void critx_urow_kernel(const double* R, int64_t P, int64_t ldr,
                                                          const int64_t* selected, int round,
                                                          CritXWS w) {
  const int64_t v = (int64_t)blockIdx.x * CR_B + threadIdx.x;
  const int64_t a = selected[round];
  if (v >= P || a < 0) return;
  double s = R[v * ldr + a];
  for (int t = 0; t < round; ++t) s -= w.c.piv[1 + t] * w.U[(int64_t)t * P + v];
  const double noma = w.c.piv[0];
  const double u = noma >= w.c.prm[0] && noma > 0.0 ? s / sqrt(noma) : 0.0;
  w.U[(int64_t)round * P + v] = u;
  w.wu[v] = w.omega[v] * u;
}

// ---- a cross-covariance generated from the points: R = diag(a_t) K(Xt, X) diag(a_s) ----
// Xt [P][d], X [n][d] row-major, one stationary kernel (kind, amp, ls: device [1]) under a per-point
// amplitude field (a_t [P], a_s [n]; NULL: ones).  R is never stored: every entry is kentry<> of
// psd.h on 2 d coordinates, in the pass, in its squared form and in the u-row of a round alike.
struct KGen {
  int kind, d;
  const double *Xt, *X, *amp, *ls, *at, *as;
};

constexpr int KG_ROWS = VGPOSP_KGEMV_ROWS;  // targets per row chunk
static_assert(KG_ROWS == SY_T, "the partials and their reduction are those of gemv_t");

static size_t kgemv_t_bytes(int64_t P, int64_t n) {
  return cr_align((size_t)ceil_div(P, KG_ROWS) * n * 8);
}

// One (512-column tile, KG_ROWS-target chunk) of y = R^T x (SQ: of the squared entries), the shape
// of gemv_t_kernel with the load of R replaced by its evaluation:
//   part[blockIdx.y][c] = sum over the chunk's targets v of k(Xt_v, X_c)^p x_v a_t[v]^p,  p = 1 + SQ
// (a_s is applied once per column by the reduction).  A thread keeps the coordinates of its column
// pair (c, c + 1) in registers; the chunk's target coordinates and x_v a_t[v]^p are staged in LDS
// once, a row of D + 1 doubles per target, and read back as wave-uniform broadcasts.  D == 0: the
// dimension at run time (4 .. 8), rows of 9 doubles.
template <int KIND, int D, bool SQ>
__global__ __launch_bounds__(SY_TH) void kgemv_t_kernel(KGen g, int64_t P, int64_t n,
                                                        const double* __restrict__ x,
                                                        double* __restrict__ part,
                                                        const double* __restrict__ gate) {
  constexpr int DW = (D > 0 ? D : 8) + 1;
  __shared__ double rows[KG_ROWS * DW];
  if (gate && *gate != 0.0) return;  // workgroup-uniform: no barrier is left waiting
  const int dd = D > 0 ? D : g.d;
  const int64_t r0 = (int64_t)blockIdx.y * KG_ROWS;
  const int nrow = (int)min((int64_t)KG_ROWS, P - r0);
  for (int e = threadIdx.x; e < nrow * dd; e += SY_TH) {
    const int i = e / dd;
    rows[i * DW + (e - i * dd)] = g.Xt[r0 * dd + e];
  }
  for (int i = threadIdx.x; i < nrow; i += SY_TH) {
    const double a = g.at ? g.at[r0 + i] : 1.0;
    rows[i * DW + DW - 1] = x[r0 + i] * (SQ ? a * a : a);
  }
  const int64_t c = (int64_t)blockIdx.x * SY_T + 2 * threadIdx.x;
  const bool in0 = c < n, in1 = c + 1 < n;
  double xa[8], xb[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    xa[k] = (k < dd && in0) ? g.X[c * dd + k] : 0.0;
    xb[k] = (k < dd && in1) ? g.X[(c + 1) * dd + k] : 0.0;
  }
  const double tla = 2.0 * log(g.amp[0]), inv_l = 1.0 / g.ls[0], inv_l2 = inv_l * inv_l;
  __syncthreads();
  if (!in0) return;
  double s0 = 0.0, s1 = 0.0, u0 = 0.0, u1 = 0.0;  // column c: s0 + s1, column c + 1: u0 + u1
  auto row = [&](int i, double& a, double& b) {
    const double* t = rows + i * DW;
    double ka = kentry<KIND, D>(t, xa, dd, tla, inv_l, inv_l2);
    double kb = kentry<KIND, D>(t, xb, dd, tla, inv_l, inv_l2);
    if (SQ) {
      ka *= ka;
      kb *= kb;
    }
    const double xw = t[DW - 1];
    a = fma(ka, xw, a);
    b = fma(kb, xw, b);
  };
  int i = 0;
  for (; i + 1 < nrow; i += 2) {
    row(i, s0, u0);
    row(i + 1, s1, u1);
  }
  if (i < nrow) row(i, s0, u0);
  double* out = part + (int64_t)blockIdx.y * n;
  out[c] = s0 + s1;
  if (in1) out[c + 1] = u0 + u1;
}

// f(kind) with the kernel kind as a compile-time constant: every generated entry is a kentry<KIND>.
template <class F>
static void with_kind(int kind, F&& f) {
  switch (kind) {
    case VGPOSP_KERNEL_EQ: f(std::integral_constant<int, VGPOSP_KERNEL_EQ>{}); break;
    case VGPOSP_KERNEL_MATERN12: f(std::integral_constant<int, VGPOSP_KERNEL_MATERN12>{}); break;
    case VGPOSP_KERNEL_MATERN32: f(std::integral_constant<int, VGPOSP_KERNEL_MATERN32>{}); break;
    default: f(std::integral_constant<int, VGPOSP_KERNEL_MATERN52>{}); break;
  }
}

// f(D) for the passes' dimension: 1, 2, 3 unrolled, 0 for the run-time loop over 4 .. 8.
template <class F>
static void with_dim(int d, F&& f) {
  switch (d) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 0>{}); break;
  }
}

// y_j = a_s[j]^p sum_v x_v a_t[v]^p k(Xt_v, X_j)^p: the pass, then gemv_t's reduction of the
// partials in ascending chunk order with the site scale.  gate as in gemv_t_launch.
template <bool SQ>
static void kgemv_t_launch(const KGen& g, int64_t P, int64_t n, const double* x, double* y,
                           double* part, const double* gate, hipStream_t s) {
  {
    const double pn = (double)P * (double)n;
    ProfScope ps(SQ ? "criteria_kgemv_t_sq" : "criteria_kgemv_t", s, (3.0 * g.d + 32.0) * pn,
                 8.0 * (double)(P + n) * (g.d + 1));
    const dim3 grid((unsigned)ceil_div(n, SY_T), (unsigned)ceil_div(P, KG_ROWS));
    with_kind(g.kind, [&](auto kind) {
      with_dim(g.d, [&](auto dim) {
        hipLaunchKernelGGL((kgemv_t_kernel<decltype(kind)::value, decltype(dim)::value, SQ>), grid,
                           dim3(SY_TH), 0, s, g, P, n, x, part, gate);
      });
    });
  }
  hipLaunchKernelGGL(gemv_t_reduce_kernel, dim3((unsigned)ceil_div(n, CR_B)), dim3(CR_B), 0, s,
                     ceil_div(P, KG_ROWS), n, part, y, gate, g.as, SQ ? 1 : 0);
}

// critx_urow_kernel with R_va generated: a_t[v] k(Xt_v, X_a) a_s[a], the entry the pass sums.
template <int KIND>
__global__ __launch_bounds__(CR_B) void critk_urow_kernel(KGen g, int64_t P,
                                                          const int64_t* selected, int round,
                                                          CritXWS w) {
  const int64_t v = (int64_t)blockIdx.x * CR_B + threadIdx.x;
  const int64_t a = selected[round];
  if (v >= P || a < 0) return;
  double xt[8], xa[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    xt[k] = k < g.d ? g.Xt[v * g.d + k] : 0.0;
    xa[k] = k < g.d ? g.X[a * g.d + k] : 0.0;
  }
  const double tla = 2.0 * log(g.amp[0]), inv_l = 1.0 / g.ls[0], inv_l2 = inv_l * inv_l;
  double s = kentry<KIND, 0>(xt, xa, g.d, tla, inv_l, inv_l2);
  if (g.at) s *= g.at[v];
  if (g.as) s *= g.as[a];
  for (int t = 0; t < round; ++t) s -= w.c.piv[1 + t] * w.U[(int64_t)t * P + v];
  const double noma = w.c.piv[0];
  const double u = noma >= w.c.prm[0] && noma > 0.0 ? s / sqrt(noma) : 0.0;
  w.U[(int64_t)round * P + v] = u;
  w.wu[v] = w.omega[v] * u;
}

static void critk_urow_launch(const KGen& g, int64_t P, const int64_t* selected, int round,
                              const CritXWS& w, hipStream_t s) {
  with_kind(g.kind, [&](auto kind) {
    hipLaunchKernelGGL(critk_urow_kernel<decltype(kind)::value>, dim3((unsigned)ceil_div(P, CR_B)),
                       dim3(CR_B), 0, s, g, P, selected, round, w);
  });
}

// ---- Sigma generated from the points: Sigma = diag(a) K(X, X) diag(a) off the diagonal ----
// X [n][d] row-major, kind / amp / ls as for KGen, a [n] the sites' amplitude field (NULL: ones).
// The diagonal is a vector: diag [n] when given (noise, jitter), else a_i^2 amp^2.  Every
// off-diagonal entry is a_i a_j kentry<>(X_i, X_j), in the pass, its squared form and the column a
// round reads alike; Sigma is never stored.
struct SGen {
  int kind, d;
  const double *X, *amp, *ls, *a, *diag;
};

__device__ __forceinline__ double sgen_diag(const SGen& g, int64_t i) {
  if (g.diag) return g.diag[i];
  const double a = g.a ? g.a[i] : 1.0, amp = g.amp[0];
  return (a * a) * (amp * amp);
}

// A workgroup owns a block of G x G 512-tiles on or above the diagonal, so the partials are one per
// (row group, column) and one per (column group, row): 16 n ng bytes for ng groups.  G grows with
// n so that there are at most KS_NG groups up to n = 512 KS_NG KS_GMAX (262,144) and enough
// workgroups below it; beyond, G = KS_GMAX.  The allocation is the larger of the two regimes'
// bounds, which makes it monotone in n where ng itself is not.
constexpr int KS_CPL = 8;             // columns per lane: one wave spans a 512-column tile
constexpr int KS_RW = SY_T / (SY_TH / 64);  // rows of a tile per wave
constexpr int KS_RC = 8;              // row partials per transpose-reduce
constexpr int KS_GMAX = 8, KS_NG = 64;
static_assert(64 * KS_CPL == SY_T && KS_RW % KS_RC == 0, "a wave per 512 columns, whole chunks");
// Waves per SIMD the registers are budgeted for: a lane holds KS_CPL columns' coordinates (16 D
// VGPRs; 128 for the run-time dimension), 48 for xa, cs and the row partials, and the entries in
// flight.  The bound is the largest at which nothing spills.
constexpr int KS_WAVES(int D) { return D == 0 ? 1 : D == 3 ? 2 : 3; }

struct KSymvWS {
  double *cpart, *rpart;  // [ng][n] each: column sums per row group, row sums per column group
  int G;
  int64_t ng;
  size_t bytes;
};

static KSymvWS ksymv_layout(void* base, int64_t n) {
  KSymvWS w{};
  const int64_t nt = ceil_div(n, SY_T);
  w.G = (int)std::min<int64_t>(KS_GMAX, std::max<int64_t>(1, ceil_div(nt, KS_NG)));
  w.ng = ceil_div(nt, w.G);
  const int64_t cap = std::max(std::min<int64_t>(nt, KS_NG), ceil_div(nt, KS_GMAX));
  const size_t slab = cr_align((size_t)cap * n * 8);
  char* p = static_cast<char*>(base);
  w.cpart = (double*)p;
  w.rpart = (double*)(p ? p + slab : nullptr);
  w.bytes = 2 * slab;
  return w;
}

// Lanes whose bit O is clear: a summed over the lane pair (l, l ^ O); lanes whose bit O is set: b
// summed likewise.  One v_permlane{32,16}_swap per dword and one add: the halving exchange of a
// transpose-reduce (O = 32: the wave's halves, O = 16: the rows of 16 lanes).
template <int O>
__device__ __forceinline__ double fold_pair(double a, double b) {
  static_assert(O == 32 || O == 16, "the exchanges with a swap instruction");
  const unsigned long long ua = __builtin_bit_cast(unsigned long long, a);
  const unsigned long long ub = __builtin_bit_cast(unsigned long long, b);
  unsigned p0, p1, q0, q1;
  if constexpr (O == 32) {
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)ua, (unsigned)ub, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(ua >> 32), (unsigned)(ub >> 32),
                                                     false, false);
    p0 = lo[0], q0 = lo[1], p1 = hi[0], q1 = hi[1];
  } else {
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)ua, (unsigned)ub, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(ua >> 32), (unsigned)(ub >> 32),
                                                     false, false);
    p0 = lo[0], q0 = lo[1], p1 = hi[0], q1 = hi[1];
  }
  const double p = __builtin_bit_cast(double, (unsigned long long)p0 | ((unsigned long long)p1 << 32));
  const double q = __builtin_bit_cast(double, (unsigned long long)q0 | ((unsigned long long)q1 << 32));
  return p + q;
}

// The wave's share (KS_RW rows) of one 512 x 512 tile.  A lane owns the columns c0 + lane + 64 q,
// q < KS_CPL: coordinates xc, x_c a_c^p in xa, column sums cs, all in registers.  The tile's rows
// are staged in LDS as rows of DW doubles (coordinates, then x_r a_r^p last) and read back as
// wave-uniform broadcasts.  Off the diagonal an entry serves both directions: the lane's KS_CPL
// products of a row are one partial, KS_RC rows' partials are reduced over the wave together (two
// halving exchanges, then four butterfly steps on the two values left, each of which ends with one
// row's sum per 16 lanes) and added to racc, the row sums this wave owns.  DT,
// the diagonal tile: the full square in the column direction only, the entry r == c left out (the
// reduction adds diag); one row at a time, it is 1 / nt of the work.
template <int KIND, int D, bool SQ, bool DT>
__device__ __forceinline__ void ksymv_tile(const double* __restrict__ rows, int nrow, int64_t r0,
                                           int64_t c0, const double (&xc)[KS_CPL][D > 0 ? D : 8],
                                           const double (&xa)[KS_CPL], double (&cs)[KS_CPL],
                                           double* __restrict__ racc, int dd, double tla,
                                           double inv_l, double inv_l2) {
  constexpr int DW = (D > 0 ? D : 8) + 1;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i1 = min(nrow, (wv + 1) * KS_RW);
  if constexpr (DT) {
#pragma unroll 1
    for (int i = wv * KS_RW; i < i1; ++i) {
      const double* t = rows + i * DW;
      const double xw = t[DW - 1];
      const int64_t off = r0 + i - c0 - lane;
#pragma unroll
      for (int q = 0; q < KS_CPL; ++q) {
        double k = kentry<KIND, D>(t, xc[q], dd, tla, inv_l, inv_l2);
        if (SQ) k *= k;
        if (off == 64 * q) k = 0.0;
        cs[q] = fma(k, xw, cs[q]);
      }
    }
    return;
  }
  const auto add = [](double a, double b) { return a + b; };
  // one row's entries at a time: a rolled loop over row pairs keeps the basic block, and with it
  // the registers the scheduler spends on entries in flight, small
  const auto partial = [&](int i) {
    const double* t = rows + i * DW;
    const double xw = t[DW - 1];
    double rp = 0.0;
#pragma unroll
    for (int q = 0; q < KS_CPL; ++q) {
      double k = kentry<KIND, D>(t, xc[q], dd, tla, inv_l, inv_l2);
      if (SQ) k *= k;
      cs[q] = fma(k, xw, cs[q]);
      rp = fma(k, xa[q], rp);
    }
    return rp;
  };
  for (int i0 = wv * KS_RW; i0 < i1; i0 += KS_RC) {  // (rows past nrow are staged as zeros)
    double w0 = 0.0, w1 = 0.0, w2 = 0.0, w3 = 0.0;
#pragma unroll 1
    for (int m = 0; m < KS_RC; m += 2) {
      const double ra = partial(i0 + m), rb = partial(i0 + m + 1);
      w0 = w1, w1 = w2, w2 = w3;
      w3 = fold_pair<32>(ra, rb);  // lower half: row m, upper half: row m + 1
    }
    double z0 = fold_pair<16>(w0, w1), z1 = fold_pair<16>(w2, w3);
    z0 = wave_step<8>(z0, add);
    z1 = wave_step<8>(z1, add);
    z0 = wave_step<4>(z0, add);
    z1 = wave_step<4>(z1, add);
    z0 = wave_step<2>(z0, add);
    z1 = wave_step<2>(z1, add);
    z0 = wave_step<1>(z0, add);
    z1 = wave_step<1>(z1, add);
    if ((lane & 15) == 0) {  // lanes 0, 16, 32, 48 hold the rows 0, 2, 1, 3 of z0, 4 + those of z1
      const int q = lane >> 4;
      double* o = racc + i0 + 2 * (q & 1) + (q >> 1);
      o[0] += z0;
      o[4] += z1;
    }
  }
}
static_assert(KS_RC == 8, "ksymv_tile folds eight row partials");

// The block (gi, gj), gj >= gi, of G x G tiles.  Column tiles outermost: the lane's column sums
// live in registers over the block's row tiles, the four waves (same columns, a quarter of every
// row tile each) are added in a fixed order through LDS, and cpart[gi][c] is written once.  The
// row sums of the G row tiles stay in LDS (racc, dynamic: G x 512 doubles) over the column tiles;
// rpart[gj][r] is written at the end.  In a diagonal block only the tiles tj >= ti exist.
template <int KIND, int D, bool SQ>
__global__ __launch_bounds__(SY_TH, KS_WAVES(D)) void ksymv_kernel(SGen g, int64_t n,
                                                      const double* __restrict__ x, KSymvWS w,
                                                      const double* __restrict__ gate) {
  constexpr int DX = D > 0 ? D : 8, DW = DX + 1;
  constexpr int NST = DW > SY_TH / 64 ? SY_T * DW : SY_T * (SY_TH / 64);
  __shared__ double stage[NST];  // a row tile; between column tiles the waves' column sums
  extern __shared__ double racc[];
  const int64_t gi = blockIdx.y, gj = blockIdx.x;
  if (gj < gi) return;               // below the diagonal
  if (gate && *gate != 0.0) return;  // workgroup-uniform: no barrier is left waiting
  const int dd = D > 0 ? D : g.d, G = w.G;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t nt = (n + SY_T - 1) / SY_T;
  const double tla = 2.0 * log(g.amp[0]), inv_l = 1.0 / g.ls[0], inv_l2 = inv_l * inv_l;
  for (int i = threadIdx.x; i < G * SY_T; i += SY_TH) racc[i] = 0.0;
  for (int cj = 0; cj < G; ++cj) {
    const int64_t tj = gj * G + cj;
    if (tj >= nt) break;
    const int64_t c0 = tj * SY_T;
    double xc[KS_CPL][DX], xa[KS_CPL], cs[KS_CPL];
#pragma unroll
    for (int q = 0; q < KS_CPL; ++q) {
      const int64_t c = c0 + lane + 64 * q;
      const bool in = c < n;
#pragma unroll
      for (int k = 0; k < DX; ++k) xc[q][k] = (k < dd && in) ? g.X[c * dd + k] : 0.0;
      const double a = g.a && in ? g.a[c] : 1.0;
      xa[q] = in ? x[c] * (SQ ? a * a : a) : 0.0;
      cs[q] = 0.0;
    }
    const int nri = gi == gj ? cj + 1 : G;
    for (int ri = 0; ri < nri; ++ri) {
      const int64_t ti = gi * G + ri;
      if (ti >= nt) break;
      const int64_t r0 = ti * SY_T;
      const int nrow = (int)min((int64_t)SY_T, n - r0);
      __syncthreads();  // the readers of the previous tile (or of the column sums) are done
      for (int e = threadIdx.x; e < SY_T * DW; e += SY_TH) {
        const int i = e / DW, k = e - i * DW;
        double v = 0.0;
        if (i < nrow) {
          if (k < dd) {
            v = g.X[(r0 + i) * dd + k];
          } else if (k == DW - 1) {
            const double a = g.a ? g.a[r0 + i] : 1.0;
            v = x[r0 + i] * (SQ ? a * a : a);
          }
        }
        stage[e] = v;
      }
      __syncthreads();
      if (ti == tj)
        ksymv_tile<KIND, D, SQ, true>(stage, nrow, r0, c0, xc, xa, cs, racc + ri * SY_T, dd, tla,
                                      inv_l, inv_l2);
      else
        ksymv_tile<KIND, D, SQ, false>(stage, nrow, r0, c0, xc, xa, cs, racc + ri * SY_T, dd, tla,
                                       inv_l, inv_l2);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < KS_CPL; ++q) stage[wv * SY_T + lane + 64 * q] = cs[q];
    __syncthreads();
    for (int i = threadIdx.x; i < SY_T; i += SY_TH)
      if (c0 + i < n)
        w.cpart[gi * n + c0 + i] = (stage[i] + stage[SY_T + i]) +
                                   (stage[2 * SY_T + i] + stage[3 * SY_T + i]);
  }
  __syncthreads();
  const int64_t rb = gi * G * SY_T;
  for (int i = threadIdx.x; i < G * SY_T; i += SY_TH)
    if (rb + i < n) w.rpart[gj * n + rb + i] = racc[i];
}
static_assert(SY_TH == 256, "ksymv_kernel adds four waves");

// y_i = a_i^p ((the column sums of the row groups 0 .. gi, ascending) + (the row sums of the
//       column groups gi .. ng - 1, ascending)) + Sigma_ii^p x_i,   gi the group of i, p = 1 + sq
__global__ __launch_bounds__(CR_B) void ksymv_reduce_kernel(SGen g, int64_t n,
                                                            const double* __restrict__ x,
                                                            KSymvWS w, double* __restrict__ y,
                                                            int sq,
                                                            const double* __restrict__ gate) {
  if (gate && *gate != 0.0) return;
  const int64_t i = (int64_t)blockIdx.x * CR_B + threadIdx.x;
  if (i >= n) return;
  const int64_t gi = i / ((int64_t)w.G * SY_T);
  double cs = 0.0, rs = 0.0;
  for (int64_t b = 0; b <= gi; ++b) cs += w.cpart[b * n + i];
  for (int64_t b = gi; b < w.ng; ++b) rs += w.rpart[b * n + i];
  const double a = g.a ? g.a[i] : 1.0, dg = sgen_diag(g, i);
  const double s = (cs + rs) * (sq ? a * a : a);
  y[i] = fma(sq ? dg * dg : dg, x[i], s);
}

// y = Sigma x (SQ: of the squared entries) for the generated Sigma.  gate as in gemv_t_launch.
template <bool SQ>
static void ksymv_launch(const SGen& g, int64_t n, const double* x, double* y, const KSymvWS& w,
                         const double* gate, hipStream_t s) {
  {
    const double tri = 0.5 * (double)n * (double)n;
    ProfScope ps(SQ ? "criteria_ksymv_sq" : "criteria_ksymv", s, (3.0 * g.d + 34.0) * tri,
                 8.0 * (double)n * (g.d + 2) * (double)w.ng);
    const dim3 grid((unsigned)w.ng, (unsigned)w.ng);
    const size_t lds = (size_t)w.G * SY_T * 8;
    with_kind(g.kind, [&](auto kind) {
      with_dim(g.d, [&](auto dim) {
        hipLaunchKernelGGL((ksymv_kernel<decltype(kind)::value, decltype(dim)::value, SQ>), grid,
                           dim3(SY_TH), lds, s, g, n, x, w, gate);
      });
    });
  }
  hipLaunchKernelGGL(ksymv_reduce_kernel, dim3((unsigned)ceil_div(n, CR_B)), dim3(CR_B), 0, s, g, n,
                     x, w, y, SQ ? 1 : 0, gate);
}

// crit_init_kernel with nom = the generated diagonal.
__global__ void critg_init_kernel(SGen g, int64_t n, int criterion, double thr,
                                  const unsigned char* targets, const unsigned char* allowed,
                                  CritWS w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    w.nom[i] = sgen_diag(g, i);
    w.tvec[i] = (!targets || targets[i]) ? 1.0 : 0.0;
    w.selmask[i] = (allowed && !allowed[i]) ? 1 : 0;
    w.delta[i] = 0.0;
    if (criterion != VGPOSP_CRIT_VARIANCE) w.s[i] = 0.0;
  }
  if (i == 0) {
    w.prm[0] = thr;
    w.prm[1] = criterion == VGPOSP_CRIT_VARIANCE ? 0.0 : 1.0;
  }
}

// crit_row_kernel with Sigma_ay generated: a_a a_y k(X_y, X_a), the entry the pass sums, and the
// diagonal vector at y = a.
template <int KIND>
__global__ __launch_bounds__(CR_B) void critg_row_kernel(SGen g, int64_t n,
                                                         const int64_t* selected, int round,
                                                         CritWS w) {
  const int64_t i = (int64_t)blockIdx.x * CR_B + threadIdx.x;
  const int64_t a = selected[round];
  if (i >= n || a < 0) return;
  double s;
  if (i == a) {
    s = sgen_diag(g, a);
  } else {
    double xi[8], xa[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      xi[k] = k < g.d ? g.X[i * g.d + k] : 0.0;
      xa[k] = k < g.d ? g.X[a * g.d + k] : 0.0;
    }
    const double tla = 2.0 * log(g.amp[0]), inv_l = 1.0 / g.ls[0], inv_l2 = inv_l * inv_l;
    s = kentry<KIND, 0>(xi, xa, g.d, tla, inv_l, inv_l2);
    if (g.a) s *= g.a[i] * g.a[a];
  }
  for (int t = 0; t < round; ++t) s -= w.piv[1 + t] * w.W[(int64_t)t * n + i];
  const double noma = w.piv[0];
  const double wy = noma >= w.prm[0] && noma > 0.0 ? s / sqrt(noma) : 0.0;
  w.W[(int64_t)round * n + i] = wy;
  w.wt[i] = wy * w.tvec[i];
  w.nom[i] -= wy * wy;
}

// ---- Sigma generated from a factor: Sigma = F F^T off the diagonal ----
// F [n][S] row-major, pitch ldf >= S, only read (the centred samples of an empirical covariance
// over sqrt(S), a PCA-truncated field, a Nystroem factor); noise [n] >= 0 or NULL.
//   Sigma_ij = f_i . f_j  (i != j),   Sigma_ii = dg_i = f_i . f_i + noise_i
// dg is computed once (row_sumsq of gp.hip, then the noise) and kept in the workspace.  The three
// things the rounds need have closed forms on F:
//   column a:   f_y . f_a                                       (factor_row with z = f_a)
//   y = Sigma x:   z = F^T x, y_i = f_i . z + noise_i x_i       (factor_tv, then factor_row)
//   y_j = sum_i x_i Sigma_ij^2:   M = F^T diag(x) F (S x S),
//                  y_j = f_j^T M f_j - x_j (f_j . f_j)^2 + x_j dg_j^2
// the last in row chunks through the fp64 MFMA GEMM: O(n S^2), never n^2.
struct SFactor {
  const double* F;
  int64_t S, ldf;
  const double* noise;
};

constexpr int64_t FC_NMAX = (int64_t)1 << 22;  // the passes; the rounds keep CR_NMAX
constexpr int64_t FC_SMAX = 4096;
constexpr int FC_TH = 256;        // four waves; a wave of factor_row owns 64 rows
constexpr int FC_NBLK = 1024;     // at most this many row blocks (partials of z)
constexpr int64_t FC_ROWS = 16384;  // rows of a chunk of the squared pass, split partials included
static_assert(FC_TH == CR_B, "factor_row's column form does crit_row_kernel's 256 rows");

// dg [n], z [S], M [S][S], and one area that is the partials of z ([nblk][S]) in the plain pass
// and, in the squared pass, the chunk temporary ([rc][S]) followed by the GEMM's split-K partials.
struct FacWS {
  double *dg, *z, *M, *zpart, *tmp, *part;
  int64_t rb, nblk, rc;  // rows per block of factor_tv, blocks, rows per chunk
  int nsplit;
  size_t bytes;
};

static FacWS fac_layout(void* base, int64_t n, int64_t S) {
  FacWS w{};
  w.rb = std::max<int64_t>(64, ceil_div(ceil_div(n, FC_NBLK), 64) * 64);
  w.nblk = ceil_div(n, w.rb);
  // an S x S result is a few output tiles: enough K ranges to fill the device with them
  w.nsplit = (int)std::min<int64_t>(64, std::max<int64_t>(1, 8192 / S));
  // what is set aside for the split partials bounds nsplit S^2 and grows with S
  const int64_t pcap = std::min<int64_t>(64 * S * S, 8192 * S);
  w.rc = std::min<int64_t>(FC_ROWS - pcap / S, n + (n & 1));  // even: chunks start 16-byte aligned
  const int64_t area = std::max(std::min<int64_t>(FC_NBLK, ceil_div(n, 64)) * S, w.rc * S + pcap);
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = p ? p + off : nullptr;
    off += cr_align(bytes);
    return (double*)r;
  };
  w.dg = take((size_t)n * 8);
  w.z = take((size_t)S * 8);
  w.M = take((size_t)S * S * 8);
  w.zpart = w.tmp = take((size_t)area * 8);
  w.part = w.tmp ? w.tmp + w.rc * S : nullptr;
  w.bytes = off;
  return w;
}

typedef double fc_d2 __attribute__((ext_vector_type(2)));

// The column pair (c, c + 1) of the row at p (p already points at column c), zero past S.  One
// 16-byte load where the pair is whole and VEC (even pitch, 16-byte aligned base), else 8-byte
// loads; the last odd column is never read as a pair (it may be the buffer's last element).
template <bool VEC>
__device__ __forceinline__ fc_d2 fc_pair(const double* __restrict__ p, int64_t c, int64_t S) {
  fc_d2 m = {0.0, 0.0};
  if (c >= S) return m;
  if (c + 1 < S) {
    if (VEC) return *reinterpret_cast<const fc_d2*>(p);
    m.x = p[0];
    m.y = p[1];
    return m;
  }
  m.x = p[0];
  return m;
}

// factor_tv: zpart[blockIdx.x][c] = sum over the block's rows r of F[r][c] x[r].  A workgroup owns
// rb rows; wave wv takes the rows r0 + wv, r0 + wv + 4, ... in ascending order, a lane the column
// pairs 2 lane + 128 q (q < NQ) of a chunk of 128 NQ columns, with 8 / NQ rows in flight so that a
// short row still keeps eight loads per lane in the air.  The four waves' sums are added through
// LDS in a fixed order.
template <bool VEC, int NQ>
__global__ __launch_bounds__(FC_TH) void factor_tv_kernel(const double* __restrict__ F, int64_t n,
                                                         int64_t S, int64_t ldf,
                                                         const double* __restrict__ x, int64_t rb,
                                                         double* __restrict__ zpart,
                                                         const double* __restrict__ gate) {
  constexpr int RU = 8 / NQ, CW = 128 * NQ;
  __shared__ double acc[FC_TH / 64][CW];
  if (gate && *gate != 0.0) return;  // workgroup-uniform: no barrier is left waiting
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t r0 = (int64_t)blockIdx.x * rb, r1 = min(r0 + rb, n);
  for (int64_t cc = 0; cc < S; cc += CW) {
    fc_d2 a[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) a[q] = fc_d2{0.0, 0.0};
    const int64_t c0 = cc + 2 * lane;
    int64_t r = r0 + wv;
    for (; r + 4 * (RU - 1) < r1; r += 4 * RU) {
      fc_d2 m[RU][NQ];
#pragma unroll
      for (int u = 0; u < RU; ++u)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          m[u][q] = fc_pair<VEC>(F + (r + 4 * u) * ldf + c0 + 128 * q, c0 + 128 * q, S);
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        const double xr = x[r + 4 * u];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          a[q].x = fma(m[u][q].x, xr, a[q].x);
          a[q].y = fma(m[u][q].y, xr, a[q].y);
        }
      }
    }
    for (; r < r1; r += 4) {
      const double xr = x[r];
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const fc_d2 m = fc_pair<VEC>(F + r * ldf + c0 + 128 * q, c0 + 128 * q, S);
        a[q].x = fma(m.x, xr, a[q].x);
        a[q].y = fma(m.y, xr, a[q].y);
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      acc[wv][2 * lane + 128 * q] = a[q].x;
      acc[wv][2 * lane + 128 * q + 1] = a[q].y;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CW; i += FC_TH)
      if (cc + i < S)
        zpart[(int64_t)blockIdx.x * S + cc + i] = (acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i]);
    __syncthreads();
  }
}
static_assert(FC_TH == 256, "factor_tv_kernel adds four waves");

// z[c] = the partials of the blocks in ascending order: sixteen waves take sixteen consecutive
// ranges of blocks, each in ascending order, and the ranges are added in ascending order.
__global__ __launch_bounds__(1024) void factor_tv_reduce_kernel(int64_t S, int64_t nblk,
                                                                const double* __restrict__ zpart,
                                                                double* __restrict__ z,
                                                                const double* __restrict__ gate) {
  __shared__ double sw[16][64];
  if (gate && *gate != 0.0) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  const int64_t per = (nblk + 15) / 16, b0 = wv * per, b1 = min(b0 + per, nblk);
  double s = 0.0;
  if (c < S) {
#pragma unroll 8
    for (int64_t b = b0; b < b1; ++b) s += zpart[b * S + c];
  }
  sw[wv][lane] = s;
  __syncthreads();
  if (wv == 0 && c < S) {
    double t = sw[0][lane];
    for (int k = 1; k < 16; ++k) t += sw[k][lane];
    z[c] = t;
  }
}

// factor_row: one dot product of length S per row, a wave per row so that any S is coalesced: lane
// l holds the column pairs 2 l + 128 q in ascending q (the fixed order over S), then the wave's
// butterfly.  A wave owns 64 consecutive rows, four in flight; the sum of row base + l is kept by
// lane l, so that what follows the dot runs one lane per row on coalesced vectors.
//   FR_PLAIN  y_i = f_i . z + noise_i x_i                z [S] broadcast through LDS
//   FR_COL    the column of a round: z = f_a, the entry dg_a at i = a, then crit_row_kernel's
//             arithmetic (the W row, w.t, the nom downdate)
//   FR_SQ     y_i = f_i . h_i - x_i (f_i . f_i)^2 + x_i dg_i^2,  h_i = row i of H = F M ([n][S])
enum { FR_PLAIN = 0, FR_COL = 1, FR_SQ = 2 };

template <bool VEC, int MODE>
__global__ __launch_bounds__(FC_TH) void factor_row_kernel(
    const double* __restrict__ F, int64_t n, int64_t S, int64_t ldf, const double* __restrict__ z,
    const double* __restrict__ noise, const double* __restrict__ dg, const double* __restrict__ x,
    double* __restrict__ y, const int64_t* __restrict__ selected, int round, CritWS w,
    const double* __restrict__ gate) {
  extern __shared__ double zs[];  // S doubles (FR_PLAIN, FR_COL)
  if (gate && *gate != 0.0) return;  // workgroup-uniform, as the next one
  int64_t a = -1;
  if (MODE == FR_COL) {
    a = selected[round];
    if (a < 0) return;
    z = F + a * ldf;
  }
  if (MODE != FR_SQ) {
    for (int64_t i = threadIdx.x; i < S; i += FC_TH) zs[i] = z[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t base = (int64_t)blockIdx.x * FC_TH + 64 * wv;
  if (base >= n) return;
  const bool hvec = (S & 1) == 0;  // H has pitch S and a 256-byte aligned base
  double mine = 0.0, mff = 0.0;
  for (int k = 0; k < 64 && base + k < n; k += 4) {
    double s[4] = {0.0, 0.0, 0.0, 0.0}, ff[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t row[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) row[u] = min(base + k + u, n - 1);  // clamped: loaded, not kept
    for (int64_t cq = 0; cq < S; cq += 128) {
      const int64_t c = cq + 2 * lane;
      fc_d2 m[4], h[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) m[u] = fc_pair<VEC>(F + row[u] * ldf + c, c, S);
      if (MODE == FR_SQ) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          h[u] = hvec ? fc_pair<true>(z + row[u] * S + c, c, S)
                      : fc_pair<false>(z + row[u] * S + c, c, S);
      } else {
        const fc_d2 zz = {c < S ? zs[c] : 0.0, c + 1 < S ? zs[c + 1] : 0.0};
#pragma unroll
        for (int u = 0; u < 4; ++u) h[u] = zz;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        s[u] = fma(m[u].x, h[u].x, s[u]);
        s[u] = fma(m[u].y, h[u].y, s[u]);
        if (MODE == FR_SQ) {
          ff[u] = fma(m[u].x, m[u].x, ff[u]);
          ff[u] = fma(m[u].y, m[u].y, ff[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double v = wave_sum(s[u]);
      if (lane == k + u) mine = v;
      if (MODE == FR_SQ) {
        const double f2 = wave_sum(ff[u]);
        if (lane == k + u) mff = f2;
      }
    }
  }
  const int64_t i = base + lane;
  if (i >= n) return;
  if (MODE == FR_PLAIN) y[i] = noise ? fma(noise[i], x[i], mine) : mine;
  if (MODE == FR_SQ) {
    const double xi = x[i], d = dg[i];
    y[i] = (mine - xi * (mff * mff)) + xi * (d * d);
  }
  if (MODE == FR_COL) {
    double s = i == a ? dg[a] : mine;
    for (int t = 0; t < round; ++t) s -= w.piv[1 + t] * w.W[(int64_t)t * n + i];
    const double noma = w.piv[0];
    const double wy = noma >= w.prm[0] && noma > 0.0 ? s / sqrt(noma) : 0.0;
    w.W[(int64_t)round * n + i] = wy;
    w.wt[i] = wy * w.tvec[i];
    w.nom[i] -= wy * wy;
  }
}

template <int MODE>
static void factor_row_launch(const SFactor& f, int64_t n, const double* z, const double* dg,
                              const double* x, double* y, const int64_t* selected, int round,
                              const CritWS& w, const double* gate, hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(n, FC_TH));
  const size_t lds = MODE == FR_SQ ? 0 : (size_t)f.S * 8;
  if (symv_vec(f.F, f.ldf))
    hipLaunchKernelGGL((factor_row_kernel<true, MODE>), grid, dim3(FC_TH), lds, s, f.F, n, f.S,
                       f.ldf, z, f.noise, dg, x, y, selected, round, w, gate);
  else
    hipLaunchKernelGGL((factor_row_kernel<false, MODE>), grid, dim3(FC_TH), lds, s, f.F, n, f.S,
                       f.ldf, z, f.noise, dg, x, y, selected, round, w, gate);
}

// dg_i = f_i . f_i (+ noise_i)
__global__ void factor_noise_kernel(int64_t n, const double* __restrict__ noise,
                                    double* __restrict__ dg) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dg[i] += noise[i];
}

static int factor_diag_launch(const SFactor& f, int64_t n, double* dg, hipStream_t s) {
  if (int rc = vgposp_row_sumsq(f.F, n, f.S, f.ldf, 1.0, 0.0, dg, s)) return rc;
  if (f.noise) {
    hipLaunchKernelGGL(factor_noise_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, n,
                       f.noise, dg);
    VG_LAUNCH_CHECK();
  }
  return 0;
}

// y = Sigma x: factor_tv, its reduction, factor_row.  F is read twice.
static int factor_symv_launch(const SFactor& f, int64_t n, const double* x, double* y,
                              const FacWS& w, const double* gate, hipStream_t s) {
  const double ns = (double)n * (double)f.S;
  ProfScope ps("criteria_fsymv", s, 4.0 * ns, 16.0 * ns);
  const dim3 grid((unsigned)w.nblk);
  const bool vec = symv_vec(f.F, f.ldf);
#define FC_TV(NQ)                                                                                 \
  if (vec)                                                                                        \
    hipLaunchKernelGGL((factor_tv_kernel<true, NQ>), grid, dim3(FC_TH), 0, s, f.F, n, f.S, f.ldf, \
                       x, w.rb, w.zpart, gate);                                                   \
  else                                                                                            \
    hipLaunchKernelGGL((factor_tv_kernel<false, NQ>), grid, dim3(FC_TH), 0, s, f.F, n, f.S,       \
                       f.ldf, x, w.rb, w.zpart, gate);
  if (f.S <= 128) {
    FC_TV(1)
  } else if (f.S <= 256) {
    FC_TV(2)
  } else {
    FC_TV(4)
  }
#undef FC_TV
  hipLaunchKernelGGL(factor_tv_reduce_kernel, dim3((unsigned)ceil_div(f.S, 64)), dim3(1024), 0, s,
                     f.S, w.nblk, w.zpart, w.z, gate);
  factor_row_launch<FR_PLAIN>(f, n, w.z, nullptr, x, y, nullptr, 0, CritWS{}, gate, s);
  VG_LAUNCH_CHECK();
  return 0;
}

// tmp[i][j] = x[i] F[i][j] for the rows of a chunk (pitch S)
__global__ __launch_bounds__(256) void factor_scale_kernel(const double* __restrict__ F,
                                                           int64_t rows, int64_t S, int64_t ldf,
                                                           const double* __restrict__ x,
                                                           double* __restrict__ tmp) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * S) return;
  const int64_t i = e / S, j = e - i * S;
  tmp[e] = x[i] * F[i * ldf + j];
}

// w.M = F^T diag(x) F (S x S, full) in row chunks of w.rc rows through the fp64 MFMA GEMM (split-K
// for the S x S result of a long chunk).
static int factor_moment_launch(const SFactor& f, int64_t n, const double* x, const FacWS& w,
                                hipStream_t s) {
  const int64_t S = f.S;
  for (int64_t c0 = 0; c0 < n; c0 += w.rc) {
    const int64_t rc = std::min(w.rc, n - c0);
    const double* Fc = f.F + c0 * f.ldf;
    hipLaunchKernelGGL(factor_scale_kernel, dim3((unsigned)ceil_div(rc * S, 256)), dim3(256), 0, s,
                       Fc, rc, S, f.ldf, x + c0, w.tmp);
    VG_LAUNCH_CHECK();
    if (int rc2 = gemm_launch_split(1, 0, S, S, rc, 1.0, Fc, f.ldf, w.tmp, S, c0 ? 1.0 : 0.0, w.M,
                                    S, VGPOSP_FULL, 0, 0, w.nsplit, w.nsplit > 1 ? w.part : nullptr,
                                    s))
      return rc2;
  }
  return 0;
}

// y_j = sum_i x_i Sigma_ij^2 through the moment matrix M = F^T diag(x) F and the rows of F M, both
// in chunks through the GEMM.  dg must hold the diagonal.
static int factor_symv_sq_launch(const SFactor& f, int64_t n, const double* x, double* y,
                                 const FacWS& w, hipStream_t s) {
  const int64_t S = f.S;
  const double ns = (double)n * (double)S;
  ProfScope ps("criteria_fsymv_sq", s, 4.0 * ns * (double)S, 8.0 * 5.0 * ns);
  if (int rc2 = factor_moment_launch(f, n, x, w, s)) return rc2;
  for (int64_t c0 = 0; c0 < n; c0 += w.rc) {
    const int64_t rc = std::min(w.rc, n - c0);
    const SFactor fc{f.F + c0 * f.ldf, S, f.ldf, nullptr};
    if (int rc2 = gemm_launch(0, 0, rc, S, S, 1.0, fc.F, f.ldf, w.M, S, 0.0, w.tmp, S, VGPOSP_FULL,
                              0, 0, s))
      return rc2;
    factor_row_launch<FR_SQ>(fc, rc, w.tmp, w.dg + c0, x + c0, y + c0, nullptr, 0, CritWS{},
                             nullptr, s);
    VG_LAUNCH_CHECK();
  }
  return 0;
}

// ---- where Sigma comes from: what the host sequences of the rounds are written against ----
// A source of Sigma is SigmaStored, SGen or SFactor with the overloads sigma_init (nom, the masks
// and prm), sigma_row (step 1) and sigma_pass<SQ> (y = Sigma x on the workspace's pass area).
struct SigmaStored {
  const double* S;
  int64_t lda;
  const double* diag;
};

static void sigma_init(const SigmaStored& sg, int64_t n, int criterion, double thr,
                       const unsigned char* targets, const unsigned char* allowed, const CritWS& w,
                       hipStream_t s) {
  hipLaunchKernelGGL(crit_init_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, sg.S, n,
                     sg.lda, sg.diag, criterion, thr, targets, allowed, w);
}
static void sigma_init(const SGen& sg, int64_t n, int criterion, double thr,
                       const unsigned char* targets, const unsigned char* allowed, const CritWS& w,
                       hipStream_t s) {
  hipLaunchKernelGGL(critg_init_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, sg, n,
                     criterion, thr, targets, allowed, w);
}
// the diagonal into the pass area, where every later use reads it; then crit_init_kernel on it
static void sigma_init(const SFactor& sg, int64_t n, int criterion, double thr,
                       const unsigned char* targets, const unsigned char* allowed, const CritWS& w,
                       hipStream_t s) {
  const FacWS fw = fac_layout(w.symv, n, sg.S);
  if (factor_diag_launch(sg, n, fw.dg, s)) return;  // the launch check that follows reports it
  hipLaunchKernelGGL(crit_init_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, nullptr,
                     n, (int64_t)0, fw.dg, criterion, thr, targets, allowed, w);
}

static void sigma_row(const SigmaStored& sg, int64_t n, const int64_t* selected, int round,
                      const CritWS& w, hipStream_t s) {
  hipLaunchKernelGGL(crit_row_kernel, dim3((unsigned)ceil_div(n, CR_B)), dim3(CR_B), 0, s, sg.S, n,
                     sg.lda, sg.diag, selected, round, w);
}
static void sigma_row(const SGen& sg, int64_t n, const int64_t* selected, int round,
                      const CritWS& w, hipStream_t s) {
  with_kind(sg.kind, [&](auto kind) {
    hipLaunchKernelGGL(critg_row_kernel<decltype(kind)::value>, dim3((unsigned)ceil_div(n, CR_B)),
                       dim3(CR_B), 0, s, sg, n, selected, round, w);
  });
}
static void sigma_row(const SFactor& sg, int64_t n, const int64_t* selected, int round,
                      const CritWS& w, hipStream_t s) {
  factor_row_launch<FR_COL>(sg, n, nullptr, fac_layout(w.symv, n, sg.S).dg, nullptr, nullptr,
                            selected, round, w, nullptr, s);
}

// The pass over Sigma on the partials area of the workspace.
template <bool SQ>
static int sigma_pass(const SigmaStored& sg, int64_t n, const double* x, double* y, void* area,
                      const double* gate, hipStream_t s) {
  symv_launch<SQ>(sg.S, n, sg.lda, sg.diag, x, y, symv_layout(area, n), gate, s);
  return 0;
}
template <bool SQ>
static int sigma_pass(const SGen& sg, int64_t n, const double* x, double* y, void* area,
                      const double* gate, hipStream_t s) {
  ksymv_launch<SQ>(sg, n, x, y, ksymv_layout(area, n), gate, s);
  return 0;
}
// (the squared pass runs at init alone and is never gated)
template <bool SQ>
static int sigma_pass(const SFactor& sg, int64_t n, const double* x, double* y, void* area,
                      const double* gate, hipStream_t s) {
  const FacWS fw = fac_layout(area, n, sg.S);
  if (SQ) return factor_symv_sq_launch(sg, n, x, y, fw, s);
  return factor_symv_launch(sg, n, x, y, fw, gate, s);
}

// ---- where the targets are: the other thing the sequences are written against ----
// InV: the targets are locations (the 0/1 mask t), the workspace is a CritWS, the dots run over n
// on it and the pass of a round is sigma_pass.  Otherwise the targets lie outside V, the workspace
// is a CritXWS, and a source of R, CrossStored or KGen, has the overloads cross_pass<SQ>
// (y = R^T x on w.gemv), cross_urow (step 2) and cross_row_doubles (what the u-row reads and
// writes per target beside the rows of U, for criteria_row's byte model).
struct InV {};
struct CrossStored {
  const double* R;
  int64_t ldr;
};

template <bool SQ>
static void cross_pass(const CrossStored& c, int64_t P, int64_t n, const double* x, double* y,
                       const CritXWS& w, const double* gate, hipStream_t s) {
  gemv_t_launch<SQ>(c.R, P, n, c.ldr, x, y, w.gemv, gate, s);
}
template <bool SQ>
static void cross_pass(const KGen& g, int64_t P, int64_t n, const double* x, double* y,
                       const CritXWS& w, const double* gate, hipStream_t s) {
  kgemv_t_launch<SQ>(g, P, n, x, y, w.gemv, gate, s);
}

static void cross_urow(const CrossStored& c, int64_t P, const int64_t* selected, int round,
                       const CritXWS& w, hipStream_t s) {
  hipLaunchKernelGGL(critx_urow_kernel, dim3((unsigned)ceil_div(P, CR_B)), dim3(CR_B), 0, s, c.R,
                     P, c.ldr, selected, round, w);
}
static void cross_urow(const KGen& g, int64_t P, const int64_t* selected, int round,
                       const CritXWS& w, hipStream_t s) {
  critk_urow_launch(g, P, selected, round, w, s);
}

static int cross_row_doubles(const CrossStored&) { return 4; }
static int cross_row_doubles(const KGen& g) { return 4 + g.d; }

static const CritWS& location_side(const CritWS& w) { return w; }
static const CritWS& location_side(const CritXWS& w) { return w.c; }

// The rule's start, after the entry has checked its arguments and laid out w (a CritWS for InV, a
// CritXWS otherwise; P, weights: the target side's, unused for InV; the cross families run the
// variance rule without a mask).
template <class Sigma, class Cross, class WS>
static int crit_init_run(const Sigma& sg, const Cross& cr, int64_t n, int64_t P, int criterion,
                         double threshold, const unsigned char* targets, const double* weights,
                         const unsigned char* allowed, const WS& w, hipStream_t s) {
  const CritWS& c = location_side(w);
  sigma_init(sg, n, criterion, threshold, targets, allowed, c, s);
  if constexpr (std::is_same<Cross, InV>::value) {
    VG_LAUNCH_CHECK();
    if (criterion == VGPOSP_CRIT_VARIANCE) {  // s_y = sum_v t_v Sigma_vy^2
      if (int rc = sigma_pass<true>(sg, n, c.tvec, c.s, c.symv, nullptr, s)) return rc;
      VG_LAUNCH_CHECK();
    }
  } else {
    hipLaunchKernelGGL(critx_init_kernel, dim3((unsigned)ceil_div(P, 256)), dim3(256), 0, s, P,
                       weights, w);
    VG_LAUNCH_CHECK();
    // s_y = sum_v omega_v R_vy^2
    cross_pass<true>(cr, P, n, w.omega, c.s, w, nullptr, s);
    VG_LAUNCH_CHECK();
  }
  return 0;
}

// One round.  The three places where the families differ: where the column of R comes from
// (cross_urow; none for InV, whose w-row is its u-row), over which side the dots run, and which
// pass fills g.
template <class Sigma, class Cross, class WS>
static int crit_step_run(const Sigma& sg, const Cross& cr, int64_t n, int64_t P, int round,
                         const int64_t* forced, int64_t j, int64_t* selected, double* sel_delta,
                         const WS& w, hipStream_t s) {
  constexpr bool in_v = std::is_same<Cross, InV>::value;
  const CritWS& c = location_side(w);
  const unsigned nb = (unsigned)ceil_div(n, CR_B);
  {
    ProfScope ps("criteria_select", s, 0.0, 8.0 * 3.0 * n);
    hipLaunchKernelGGL(crit_score_kernel, dim3((unsigned)ceil_div(n, CR_CH)), dim3(CR_CH), 0, s, n,
                       c);
    hipLaunchKernelGGL(crit_select_kernel, dim3(1), dim3(CR_CH), 0, s, n, round, forced, j,
                       selected, sel_delta, c);
    VG_LAUNCH_CHECK();
  }
  double row_doubles = (double)n * (5 + round);
  if constexpr (!in_v) row_doubles += (double)P * (cross_row_doubles(cr) + round);
  {
    ProfScope ps("criteria_row", s, 0.0, 8.0 * row_doubles);
    sigma_row(sg, n, selected, round, c, s);
    if constexpr (!in_v) cross_urow(cr, P, selected, round, w, s);
    VG_LAUNCH_CHECK();
  }
  // The variance rule's part: every kernel below returns at once under the entropy rule (the
  // criterion lives in the workspace, so the launch sequence does not depend on it).
  // dot[t] = W_t . (w.t) over n, or U_t . (omega.u) over P on the target side's view, for
  // t <= round (t = round: |w.t|^2, or sum_v omega_v u_v^2)
  const double* gate = c.prm + 1;
  CritWS tv = c;
  int64_t nt = n;
  if constexpr (!in_v) {
    tv = critx_target_view(w);
    nt = P;
  }
  const unsigned nbt = (unsigned)ceil_div(nt, CR_B);
  hipLaunchKernelGGL(crit_dots_kernel, dim3(nbt, (unsigned)round + 1), dim3(CR_B), 0, s, nt,
                     selected, round, tv);
  hipLaunchKernelGGL(crit_fold_kernel, dim3((unsigned)round + 1), dim3(CR_B), 0, s, (int64_t)nbt,
                     selected, round, tv);
  VG_LAUNCH_CHECK();
  if constexpr (in_v) {
    if (int rc = sigma_pass<false>(sg, n, c.wt, c.g, c.symv, gate, s)) return rc;
  } else {
    cross_pass<false>(cr, P, n, w.wu, c.g, w, gate, s);
  }
  VG_LAUNCH_CHECK();
  {
    ProfScope ps("criteria_update", s, 0.0, 8.0 * (double)n * (4 + round));
    hipLaunchKernelGGL(crit_update_kernel, dim3(nb), dim3(CR_B), 0, s, n, selected, round, c);
    VG_LAUNCH_CHECK();
  }
  return 0;
}

// ---- the entries' argument checks, one per group of arguments ----
// VG_ARG: `fn` is the entry's name, `at` the position of the group's first argument in that entry.

// (Sigma, n, lda, diag)
static int check_sigma(const char* fn, int at, const SigmaStored& sg, int64_t n) {
  VG_ARG(sg.S != nullptr, at);
  VG_ARG(n >= 1 && n <= CR_NMAX, at + 1);
  VG_ARG(sg.lda >= n, at + 2);
  return 0;
}
// (kind, X, n, d, amp, ls, site_scale, diag)
static int check_sigma(const char* fn, int at, const SGen& g, int64_t n) {
  VG_ARG(g.kind >= VGPOSP_KERNEL_EQ && g.kind <= VGPOSP_KERNEL_MATERN52, at);
  VG_ARG(g.X != nullptr, at + 1);
  VG_ARG(n >= 1 && n <= CR_NMAX, at + 2);
  VG_ARG(g.d >= 1 && g.d <= 8, at + 3);
  VG_ARG(g.amp != nullptr, at + 4);
  VG_ARG(g.ls != nullptr, at + 5);
  return 0;
}
// (F, n, s, ldf, noise); nmax: the passes alone go beyond the rounds' CR_NMAX
static int check_sigma(const char* fn, int at, const SFactor& f, int64_t n,
                       int64_t nmax = CR_NMAX) {
  VG_ARG(f.F != nullptr, at);
  VG_ARG(n >= 1 && n <= nmax, at + 1);
  VG_ARG(f.S >= 1 && f.S <= FC_SMAX, at + 2);
  VG_ARG(f.ldf >= f.S, at + 3);
  return 0;
}

// (R, P, ldr), and (kind, Xt, P, X, d, amp, ls, target_scale, site_scale).  with_n: the pass
// entries have no Sigma group and carry n inside this one, after P (stored) or after X (generated).
static int check_cross(const char* fn, int at, const CrossStored& c, int64_t P, int64_t n,
                       bool with_n = false) {
  VG_ARG(c.R != nullptr, at);
  VG_ARG(P >= 1 && P <= CRX_PMAX, at + 1);
  if (with_n) {
    VG_ARG(n >= 1 && n <= CR_NMAX, at + 2);
    ++at;
  }
  VG_ARG(c.ldr >= n, at + 2);
  return 0;
}
static int check_cross(const char* fn, int at, const KGen& g, int64_t P, int64_t n,
                       bool with_n = false) {
  VG_ARG(g.kind >= VGPOSP_KERNEL_EQ && g.kind <= VGPOSP_KERNEL_MATERN52, at);
  VG_ARG(g.Xt != nullptr, at + 1);
  VG_ARG(P >= 1 && P <= CRX_PMAX, at + 2);
  VG_ARG(g.X != nullptr, at + 3);
  if (with_n) {
    VG_ARG(n >= 1 && n <= CR_NMAX, at + 4);
    ++at;
  }
  VG_ARG(g.d >= 1 && g.d <= 8, at + 4);
  VG_ARG(g.amp != nullptr, at + 5);
  VG_ARG(g.ls != nullptr, at + 6);
  return 0;
}

// (kmax, criterion, threshold) of an in-V init; the cross inits have (kmax, threshold):
// criterion == nullptr
static int check_rule(const char* fn, int at, int kmax, int64_t n, const int* criterion,
                      double threshold) {
  VG_ARG(kmax >= 1 && kmax <= n, at);
  if (criterion) {
    VG_ARG(*criterion == VGPOSP_CRIT_VARIANCE || *criterion == VGPOSP_CRIT_ENTROPY, at + 1);
    ++at;
  }
  VG_ARG(threshold >= 0.0, at + 1);
  return 0;
}

// (kmax, round, forced, j, selected, sel_delta) of a step
static int check_round(const char* fn, int at, int kmax, int64_t n, int round,
                       const int64_t* forced, int64_t j, const int64_t* selected) {
  VG_ARG(kmax >= 1 && kmax <= n, at);
  VG_ARG(round >= 0 && round < kmax, at + 1);
  VG_ARG(forced == nullptr || j >= 0, at + 3);
  VG_ARG(selected != nullptr, at + 4);
  return 0;
}

// (ws, n[, mid], kmax) of a _buffers entry; mid: P or s where the entry has one
static int check_buffers(const char* fn, const void* ws, int64_t n, const int64_t* mid, int kmax) {
  VG_ARG(ws != nullptr, 1);
  VG_ARG(n >= 1, 2);
  if (mid) VG_ARG(*mid >= 1, 3);
  VG_ARG(kmax >= 1, mid ? 4 : 3);
  return 0;
}

// (x, y, ws, ws_bytes) of a pass entry, x at `at`: a missing workspace is VGPOSP_E_WS there
static int check_pass(const char* fn, int at, const double* x, const double* y, const void* ws,
                      size_t ws_bytes, size_t need) {
  VG_ARG(x != nullptr, at);
  VG_ARG(y != nullptr, at + 1);
  if (ws == nullptr) {
    set_error("%s: workspace is null", fn);
    return VGPOSP_E_WS;
  }
  if (ws_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
    return VGPOSP_E_WS;
  }
  return 0;
}

// The outputs of a _buffers entry, each optional.
static void crit_outputs(const CritWS& w, double** nom, double** score, double** delta,
                         double** W) {
  if (nom) *nom = w.nom;
  if (score) *score = w.s;
  if (delta) *delta = w.delta;
  if (W) *W = w.W;
}
static void critx_outputs(const CritXWS& w, double** nom, double** score, double** delta,
                          double** W, double** U) {
  crit_outputs(w.c, nom, score, delta, W);
  if (U) *U = w.U;
}

// ---- mutual information on a factor: Sigma = F F^T + D, D = diag(noise) > 0 (Woodbury) ----
// The rounds of greedy.hip need Q = Sigma^-1, which at n S doubles cannot be stored either:
//   Q = D^-1 - D^-1 F C^-1 F^T D^-1,   C = I_S + F^T D^-1 F   (S x S, SPD, lambda_min >= 1)
// With C = L L^T and M = L^-1 (potrf_one, invert = 1) everything the rounds read is a closed form
// on F, d = noise and dg_i = f_i . f_i + d_i:
//   Q_yy          = 1 / d_y - |M f_y|^2 / d_y^2                         once, O(n S^2)
//   Sigma e_a     : s_i = f_i . f_a, dg_a at i = a
//   Q e_a         : q_i = [i = a] / d_a - (f_i . u_a) / d_i,   u_a = C^-1 f_a / d_a   (an S-vector)
// The rest is greedy_update_kernel's arithmetic with jitter 0: s and q downdated by the earlier
// rows of W and V through the pick's pivots, w = s / sqrt(nom_a), v = q / sqrt(prec_a), nom -= w^2,
// prec -= v^2, delta = delta_of(nom, prec, 0, thr).  A round scores and selects first, then updates
// for its pick (crit_step_run's order); the arg-max runs over the fresh delta of every free
// candidate, ties to the lower index: the full greedy.  Every delta is fresh after the one stream
// over F a round needs anyway, so there is no lazy cache to save evaluations.  Masked locations
// stay in every denominator.  Four launches a round, F read once, no float atomics.
// piv: [0] nom_a, [1] prec_a, [2 + t] W_t[a], [2 + kmax + t] V_t[a].
struct FmiWS {
  double *prm, *nom, *prec, *delta, *W, *V, *piv, *u, *Cinv, *fval;
  long long* fidx;
  unsigned char* selmask;
  void *fac, *potrf;  // fac_layout's area: dg kept; M, the chunk and its partials at init only
  bool compact;       // the layout of the factorization's workspace
  size_t bytes;
};

static FmiWS fmi_layout(void* base, int64_t n, int64_t S, int kmax) {
  FmiWS w{};
  const int64_t nch = ceil_div(n, CR_CH);
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = p ? p + off : nullptr;
    off += cr_align(bytes);
    return r;
  };
  w.prm = (double*)take(8 * 8);
  w.nom = (double*)take(n * 8);
  w.prec = (double*)take(n * 8);
  w.delta = (double*)take(n * 8);
  w.W = (double*)take((size_t)kmax * n * 8);
  w.V = (double*)take((size_t)kmax * n * 8);
  w.piv = (double*)take((2 + 2 * (size_t)kmax) * 8);
  w.u = (double*)take((size_t)S * 8);
  w.Cinv = (double*)take((size_t)S * S * 8);
  w.fval = (double*)take(nch * 8);
  w.fidx = (long long*)take(nch * 8);
  w.selmask = (unsigned char*)take(n);
  w.fac = take(fac_layout(nullptr, n, S).bytes);
  w.compact = potrf_ws_bytes_compact(S) < potrf_ws_bytes(S);
  w.potrf = take(potrf_ws_bytes_compact(S));
  w.bytes = off;
  return w;
}

__global__ void fmi_recip_kernel(int64_t n, const double* __restrict__ noise,
                                 double* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = 1.0 / noise[i];
}

// C = M + I on the diagonal (before the factorization); after it, zeros above the diagonal of
// M = L^-1, which the factorization never writes.
__global__ void fmi_square_kernel(int64_t S, double* __restrict__ M, int after) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= S * S) return;
  const int64_t i = e / S, j = e - i * S;
  if (!after && i == j) M[e] += 1.0;
  if (after && j > i) M[e] = 0.0;
}

// nom = dg, prec = Q_yy from tsq_y = |M f_y|^2 (held in prec), the masks and prm.
__global__ void fmi_init_kernel(int64_t n, const double* __restrict__ dg,
                                const double* __restrict__ noise, double thr,
                                const unsigned char* allowed, FmiWS w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const double d = noise[i];
    w.nom[i] = dg[i];
    w.prec[i] = 1.0 / d - w.prec[i] / (d * d);
    w.delta[i] = 0.0;
    w.selmask[i] = (allowed && !allowed[i]) ? 1 : 0;
  }
  if (i == 0) w.prm[0] = thr;
}

// delta for every location, and the best key of the workgroup over the free candidates.
__global__ __launch_bounds__(CR_CH) void fmi_score_kernel(int64_t n, FmiWS w) {
  const int64_t i = (int64_t)blockIdx.x * CR_CH + threadIdx.x;
  const double thr = w.prm[0];
  double bv = -DBL_MAX;
  long long bi = -1;
  if (i < n) {
    const double d = delta_of(w.nom[i], w.prec[i], 0.0, thr);
    w.delta[i] = d;
    if (!w.selmask[i]) {
      bv = d;
      bi = i;
    }
  }
  crit_block_keymax(bv, bi);
  if (threadIdx.x == 0) {
    w.fval[blockIdx.x] = bv;
    w.fidx[blockIdx.x] = bi;
  }
}

// crit_select_kernel with the pivots of both sides.  No candidate left: selected[round] = -1, and
// the rest of the round does nothing.
__global__ __launch_bounds__(CR_CH) void fmi_select_kernel(int64_t n, int kmax, int round,
                                                           const int64_t* forced, int64_t j,
                                                           int64_t* selected, double* sel_delta,
                                                           FmiWS w) {
  const int64_t nch = (n + CR_CH - 1) / CR_CH;
  double v = -DBL_MAX;
  long long y = -1;
  if (forced) {
    y = min(max(forced[j], (int64_t)0), n - 1);  // validated by the host; never outside
  } else {
    for (int64_t e = threadIdx.x; e < nch; e += blockDim.x) {
      if (w.fidx[e] >= 0 && key_gt(w.fval[e], w.fidx[e], v, y)) {
        v = w.fval[e];
        y = w.fidx[e];
      }
    }
    crit_block_keymax(v, y);
  }
  if (threadIdx.x == 0) {
    selected[round] = y;
    if (sel_delta) sel_delta[round] = y >= 0 ? w.delta[y] : 0.0;
    if (y >= 0) {
      w.selmask[y] = 1;
      w.piv[0] = w.nom[y];
      w.piv[1] = w.prec[y];
    }
  }
  if (y >= 0)
    for (int t = threadIdx.x; t < round; t += blockDim.x) {
      w.piv[2 + t] = w.W[(int64_t)t * n + y];
      w.piv[2 + kmax + t] = w.V[(int64_t)t * n + y];
    }
}

// u_a = C^-1 f_a / d_a: a wave per row of C^-1, lane l the columns l + 64 q in ascending q, then
// the wave's butterfly.
__global__ __launch_bounds__(FC_TH) void fmi_u_kernel(const double* __restrict__ F, int64_t S,
                                                      int64_t ldf,
                                                      const double* __restrict__ noise,
                                                      const int64_t* __restrict__ selected,
                                                      int round, FmiWS w) {
  const int64_t a = selected[round];
  if (a < 0) return;
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (FC_TH / 64) + (threadIdx.x >> 6);
  if (r >= S) return;  // whole waves
  const double* fa = F + a * ldf;
  const double* c = w.Cinv + r * S;
  double s = 0.0;
  for (int64_t k = lane; k < S; k += 64) s = fma(c[k], fa[k], s);
  s = wave_sum(s);
  if (lane == 0) w.u[r] = s / noise[a];
}

// factor_row_kernel's stream with two right-hand sides: f_i . f_a and f_i . u_a from one read of
// the row, f_a staged in LDS and u_a beside it (ULDS) or read through L2 where 2 S doubles are
// more LDS than a workgroup is given by default.  Then one lane per row: the columns of Sigma and
// of Q, their downdates, the two new rows and the nom and prec downdates.  w = 0 unless
// nom_a >= thr and > 0 (crit_row_kernel), v = 0 unless prec_a > 0 (greedy_update_kernel).
constexpr int64_t FMI_ULDS_SMAX = 2048;  // 2 S doubles = 32 KiB

template <bool VEC, bool ULDS>
__global__ __launch_bounds__(FC_TH) void fmi_row_kernel(
    const double* __restrict__ F, int64_t n, int64_t S, int64_t ldf,
    const double* __restrict__ noise, const double* __restrict__ dg,
    const int64_t* __restrict__ selected, int kmax, int round, FmiWS w) {
  extern __shared__ double zs[];  // f_a [S], then u_a [S] (ULDS)
  const int64_t a = selected[round];
  if (a < 0) return;  // workgroup-uniform
  const double* __restrict__ ug = w.u;
  for (int64_t i = threadIdx.x; i < S; i += FC_TH) {
    zs[i] = F[a * ldf + i];
    if (ULDS) zs[S + i] = ug[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t base = (int64_t)blockIdx.x * FC_TH + 64 * wv;
  if (base >= n) return;
  double mine = 0.0, mineu = 0.0;
  for (int k = 0; k < 64 && base + k < n; k += 4) {
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t row[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) row[u] = min(base + k + u, n - 1);  // clamped: loaded, not kept
    for (int64_t cq = 0; cq < S; cq += 128) {
      const int64_t c = cq + 2 * lane;
      fc_d2 m[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) m[u] = fc_pair<VEC>(F + row[u] * ldf + c, c, S);
      const fc_d2 zz = {c < S ? zs[c] : 0.0, c + 1 < S ? zs[c + 1] : 0.0};
      const fc_d2 uu = {c < S ? (ULDS ? zs[S + c] : ug[c]) : 0.0,
                        c + 1 < S ? (ULDS ? zs[S + c + 1] : ug[c + 1]) : 0.0};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        s[u] = fma(m[u].x, zz.x, s[u]);
        s[u] = fma(m[u].y, zz.y, s[u]);
        q[u] = fma(m[u].x, uu.x, q[u]);
        q[u] = fma(m[u].y, uu.y, q[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double vs = wave_sum(s[u]), vq = wave_sum(q[u]);
      if (lane == k + u) {
        mine = vs;
        mineu = vq;
      }
    }
  }
  const int64_t i = base + lane;
  if (i >= n) return;
  double sc = i == a ? dg[a] : mine;
  double qc = (i == a ? 1.0 / noise[a] : 0.0) - mineu / noise[i];
  for (int t = 0; t < round; ++t) {
    sc -= w.piv[2 + t] * w.W[(int64_t)t * n + i];
    qc -= w.piv[2 + kmax + t] * w.V[(int64_t)t * n + i];
  }
  const double noma = w.piv[0], preca = w.piv[1];
  const double wy = noma >= w.prm[0] && noma > 0.0 ? sc / sqrt(noma) : 0.0;
  const double vy = preca > 0.0 ? qc / sqrt(preca) : 0.0;
  w.W[(int64_t)round * n + i] = wy;
  w.V[(int64_t)round * n + i] = vy;
  w.nom[i] -= wy * wy;
  w.prec[i] -= vy * vy;
}

static void fmi_row_launch(const SFactor& f, int64_t n, const double* dg, const int64_t* selected,
                           int kmax, int round, const FmiWS& w, hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(n, FC_TH));
  const bool ulds = f.S <= FMI_ULDS_SMAX;
  const size_t lds = (size_t)f.S * 8 * (ulds ? 2 : 1);
#define FMI_ROW(VEC, ULDS)                                                                      \
  hipLaunchKernelGGL((fmi_row_kernel<VEC, ULDS>), grid, dim3(FC_TH), lds, s, f.F, n, f.S, f.ldf, \
                     f.noise, dg, selected, kmax, round, w)
  if (symv_vec(f.F, f.ldf)) {
    if (ulds) FMI_ROW(true, true); else FMI_ROW(true, false);
  } else {
    if (ulds) FMI_ROW(false, true); else FMI_ROW(false, false);
  }
#undef FMI_ROW
}

// The start: dg, C = I + F^T D^-1 F (factor_symv_sq's moment loop with x = 1 / d), M = L^-1,
// C^-1 = M^T M, and per chunk T = F_c M^T with its row sums of squares.  info: the
// factorization's status (device int32).
static int fmi_init_run(const SFactor& f, int64_t n, int kmax, double threshold,
                        const unsigned char* allowed, int* info, const FmiWS& w, hipStream_t s) {
  const int64_t S = f.S;
  const FacWS fw = fac_layout(w.fac, n, S);
  const double ns = (double)n * (double)S;
  ProfScope ps("criteria_fmi_init", s, 4.0 * ns * (double)S, 8.0 * 4.0 * ns);
  VG_TRY(factor_diag_launch(f, n, fw.dg, s));
  const unsigned nb = (unsigned)ceil_div(n, 256), sb = (unsigned)ceil_div(S * S, 256);
  hipLaunchKernelGGL(fmi_recip_kernel, dim3(nb), dim3(256), 0, s, n, f.noise, w.delta);
  VG_LAUNCH_CHECK();
  VG_TRY(factor_moment_launch(f, n, w.delta, fw, s));
  hipLaunchKernelGGL(fmi_square_kernel, dim3(sb), dim3(256), 0, s, S, fw.M, 0);
  VG_LAUNCH_CHECK();
  VG_HIP(vg_memset(info, 0, sizeof(int), s));
  VG_TRY(potrf_one(fw.M, S, S, 1, nullptr, info, w.potrf, s, false, true, w.compact));
  hipLaunchKernelGGL(fmi_square_kernel, dim3(sb), dim3(256), 0, s, S, fw.M, 1);
  VG_LAUNCH_CHECK();
  VG_TRY(gemm_launch(1, 0, S, S, S, 1.0, fw.M, S, fw.M, S, 0.0, w.Cinv, S, VGPOSP_FULL, 0, 0, s));
  for (int64_t c0 = 0; c0 < n; c0 += fw.rc) {
    const int64_t rc = std::min(fw.rc, n - c0);
    VG_TRY(gemm_launch(0, 1, rc, S, S, 1.0, f.F + c0 * f.ldf, f.ldf, fw.M, S, 0.0, fw.tmp, S,
                       VGPOSP_FULL, 0, 0, s));
    VG_TRY(vgposp_row_sumsq(fw.tmp, rc, S, S, 1.0, 0.0, w.prec + c0, s));
  }
  hipLaunchKernelGGL(fmi_init_kernel, dim3(nb), dim3(256), 0, s, n, fw.dg, f.noise, threshold,
                     allowed, w);
  VG_LAUNCH_CHECK();
  return 0;
}

static int fmi_step_run(const SFactor& f, int64_t n, int kmax, int round, const int64_t* forced,
                        int64_t j, int64_t* selected, double* sel_delta, const FmiWS& w,
                        hipStream_t s) {
  const double* dg = fac_layout(w.fac, n, f.S).dg;
  {
    ProfScope ps("criteria_fmi_select", s, 0.0, 8.0 * 4.0 * n);
    hipLaunchKernelGGL(fmi_score_kernel, dim3((unsigned)ceil_div(n, CR_CH)), dim3(CR_CH), 0, s, n,
                       w);
    hipLaunchKernelGGL(fmi_select_kernel, dim3(1), dim3(CR_CH), 0, s, n, kmax, round, forced, j,
                       selected, sel_delta, w);
    VG_LAUNCH_CHECK();
  }
  {
    ProfScope ps("criteria_fmi_u", s, 2.0 * (double)f.S * f.S, 8.0 * (double)f.S * (f.S + 2));
    hipLaunchKernelGGL(fmi_u_kernel, dim3((unsigned)ceil_div(f.S, FC_TH / 64)), dim3(FC_TH), 0, s,
                       f.F, f.S, f.ldf, f.noise, selected, round, w);
    VG_LAUNCH_CHECK();
  }
  {
    const double ns = (double)n * (double)f.S;
    ProfScope ps("criteria_fmi_row", s, 4.0 * ns, 8.0 * ns + 8.0 * (double)n * (2 * round + 6));
    fmi_row_launch(f, n, dg, selected, kmax, round, w, s);
    VG_LAUNCH_CHECK();
  }
  return 0;
}

// ---- field reconstruction from placed sensors on a factor: the posterior mean and variance ----
// A: k distinct sensors, sigma2 = obs_noise on the sensors' own covariance only:
//   G = F_A F_A^T + diag(d_A + sigma2) = L L^T,  M = L^-1,  c_i = F_A f_i + [i in A] d_i e_pos(i)
//   var_i = dg_i - |M c_i|^2,   mean_i,b = mu_i + c_i . alpha_b,   alpha = G^-1 (Y - mu_A)
// With W = M F_A (k x S) and Z = F_A^T alpha (S x B) a site outside A needs the row
// f_i . [W^T | Z] alone: var_i = dg_i - the sum of squares of its first k numbers, mean_i,b = mu_i +
// number k + b.  P = [W^T | Z] is kept as its two column blocks, Wt [S][kp] (written once by
// init) and Z [S][bp] (written by every apply, bp from that call's nrhs), kp and bp the next
// multiples of 16 with zero columns between: a zero column adds nothing to a sum of squares.
// fpost_stream_kernel is the tall-skinny product F . P on the fp64 matrix cores whose n x (k + B)
// result is never stored; fpost_sensor_kernel rewrites the k sensor rows with the term in d_a.
constexpr int FP_KMAX = 1024;  // sensors
constexpr int FP_BMAX = 1024;  // right-hand sides of one apply
constexpr int FP_KT = 32;      // columns of F, rows of P, per K-tile
constexpr int FP_LDP = 72;     // pitch of a staged row of P (doubles): rows 2 g and 2 g + 1 of the
                               // four lane groups g fall into disjoint banks
constexpr int FP_ROWS = 128;   // rows of F per workgroup: four waves of two 16-row blocks
constexpr int FP_NF = 4;       // 16-column fragments of a panel

// What the small kernels read of the workspace, and the rest of its layout for the host.
struct FpostDev {
  double *dA, *FA, *M, *Wt, *R, *alpha, *Z;
  int64_t* sens;
  int* status;  // the factorization's status, kept for every apply
  int kp, bp;   // k and nrhs padded to whole 16-column fragments
};
struct FpostWS : FpostDev {
  double *dg, *T;
  void* potrf;
  bool compact;
  size_t bytes;
};

static FpostWS fpost_layout(void* base, int64_t n, int64_t S, int k, int nrhs) {
  FpostWS w{};
  w.kp = (int)ceil_div(k, 16) * 16;
  w.bp = (int)ceil_div(nrhs, 16) * 16;
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = p ? p + off : nullptr;
    off += cr_align(bytes);
    return r;
  };
  w.dg = (double*)take((size_t)n * 8);
  w.sens = (int64_t*)take((size_t)k * 8);
  w.status = (int*)take(sizeof(int));
  w.dA = (double*)take((size_t)k * 8);
  w.FA = (double*)take((size_t)k * S * 8);
  w.M = (double*)take((size_t)k * k * 8);
  w.compact = potrf_ws_bytes_compact(k) < potrf_ws_bytes(k);
  w.potrf = take(potrf_ws_bytes_compact(k));
  w.Wt = (double*)take((size_t)S * w.kp * 8);
  w.R = (double*)take((size_t)k * w.bp * 8);
  w.T = (double*)take((size_t)k * w.bp * 8);
  w.alpha = (double*)take((size_t)k * w.bp * 8);
  w.Z = (double*)take((size_t)S * w.bp * 8);
  w.bytes = off;
  return w;
}

typedef double fp_d4 __attribute__((ext_vector_type(4)));

// One pass over F for a panel of NF 16-column fragments of P: the first nvf from Wt (variance),
// the rest from Z (mean).  A wave owns 32 rows as two 16-row blocks and accumulates 32 x 16 NF
// outputs.  Lane l (fr = l & 15, fk = l >> 4) loads the column pairs 8 q + 2 fk (q < 4) of row fr
// of each block straight from global memory, 16 bytes where VEC; a pair feeds two MFMAs, whose K
// index is then the even (odd) columns 8 q + 2 g (+ 1) over the lane groups g, and the B fragments
// follow that permutation: P[8 q + 2 fk (+ 1)][16 j + fr] from the K-tile of P staged in LDS, two
// buffers, one barrier a tile; the next tile of both operands is in registers while one is
// multiplied.  Rows past n are clamped for loading and dropped for storing; columns past S read
// zeros on both sides, and the last column of an odd S is never read as a pair (fc_pair).
// The epilogue runs from the accumulators (C/D map: col = fr, row = fk + 4 reg): the 16 lanes of a
// group hold the 16 columns of a row, so the squares of the variance fragments are summed in the
// lane over ascending j and across the group by the xor butterfly 8, 4, 2, 1, and
// var_i = (first ? dg_i : var_i) - that sum; a mean fragment is written to out[i][b0 + ...], 16
// consecutive lanes 128 contiguous bytes.  No atomics; gate != 0 (the factorization's status)
// makes the launch a workgroup-uniform no-op before any barrier.
template <bool VEC, int NF>
__global__ __launch_bounds__(FC_TH) void fpost_stream_kernel(
    const double* __restrict__ F, int64_t n, int64_t S, int64_t ldf,
    const double* __restrict__ Pv, int64_t ldv, int nvf, const double* __restrict__ Pz,
    int64_t ldz, int first, const double* __restrict__ dg, double* __restrict__ var,
    const double* __restrict__ mu, double* __restrict__ out, int64_t ldo, int b0, int nrhs,
    const int* __restrict__ gate) {
  __shared__ double ps[2][FP_KT * FP_LDP];
  if (gate && *gate != 0) return;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fk = lane >> 4;
  const int64_t base = (int64_t)blockIdx.x * FP_ROWS + 32 * wv;
  const double* frow[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) frow[rb] = F + min(base + 16 * rb + fr, n - 1) * ldf;

  // this thread's NF pairs of a K-tile of P: pair e = tid + 256 u is row e / (8 NF), pair e % (8 NF)
  constexpr int PR = 8 * NF;
  const double* psrc[NF];
  int prow[NF], pdst[NF];
  int64_t pld[NF];
#pragma unroll
  for (int u = 0; u < NF; ++u) {
    const int e = threadIdx.x + FC_TH * u, row = e / PR, pc = e % PR, j = pc >> 3;
    prow[u] = row;
    pdst[u] = row * FP_LDP + 2 * pc;
    pld[u] = j < nvf ? ldv : ldz;
    psrc[u] = (j < nvf ? Pv + 16 * j : Pz + 16 * (j - nvf)) + 2 * (pc & 7) + row * pld[u];
  }

  fp_d4 acc[2][NF];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[rb][j] = fp_d4{0.0, 0.0, 0.0, 0.0};

  fc_d2 a[2][4], an[2][4], pp[NF];
  auto load_a = [&](int64_t k0, fc_d2 (&dst)[2][4]) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t c = k0 + 8 * q + 2 * fk;
        dst[rb][q] = fc_pair<VEC>(frow[rb] + c, c, S);
      }
  };
  auto load_p = [&](int64_t k0) {
#pragma unroll
    for (int u = 0; u < NF; ++u)
      pp[u] = k0 + prow[u] < S ? *reinterpret_cast<const fc_d2*>(psrc[u] + k0 * pld[u])
                               : fc_d2{0.0, 0.0};
  };
  auto store_p = [&](int buf) {
#pragma unroll
    for (int u = 0; u < NF; ++u) *reinterpret_cast<fc_d2*>(&ps[buf][pdst[u]]) = pp[u];
  };

  load_a(0, a);
  load_p(0);
  store_p(0);
  __syncthreads();
  int buf = 0;
  for (int64_t k0 = 0; k0 < S; k0 += FP_KT) {
    const bool more = k0 + FP_KT < S;  // workgroup-uniform
    if (more) {
      load_a(k0 + FP_KT, an);
      load_p(k0 + FP_KT);
    }
    const double* pb = ps[buf] + 2 * fk * FP_LDP + fr;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double be[NF], bo[NF];
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        be[j] = pb[8 * q * FP_LDP + 16 * j];
        bo[j] = pb[(8 * q + 1) * FP_LDP + 16 * j];
      }
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int j = 0; j < NF; ++j) {
          acc[rb][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rb][q].x, be[j], acc[rb][j], 0, 0, 0);
          acc[rb][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rb][q].y, bo[j], acc[rb][j], 0, 0, 0);
        }
    }
    if (more) {
      store_p(buf ^ 1);
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int q = 0; q < 4; ++q) a[rb][q] = an[rb][q];
    }
    __syncthreads();
    buf ^= 1;
  }

  const auto add = [](double x, double y) { return x + y; };
  if (nvf > 0) {
    double keep = 0.0;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double ss = 0.0;
#pragma unroll
        for (int j = 0; j < NF; ++j)
          if (j < nvf) ss = fma(acc[rb][j][r], acc[rb][j][r], ss);
        ss = wave_step<8>(ss, add);
        ss = wave_step<4>(ss, add);
        ss = wave_step<2>(ss, add);
        ss = wave_step<1>(ss, add);
        if (fr == 4 * rb + r) keep = ss;
      }
    const int64_t row = base + 16 * (fr >> 2) + fk + 4 * (fr & 3);
    if (fr < 8 && row < n) var[row] = (first ? dg[row] : var[row]) - keep;
  }
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int b = b0 + 16 * (j - nvf) + fr;
    if (j >= nvf && b < nrhs) {
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t row = base + 16 * rb + fk + 4 * r;
          if (row < n) out[row * ldo + b] = (mu ? mu[row] : 0.0) + acc[rb][j][r];
        }
    }
  }
}

// One workgroup per sensor a = sens[p]: its row of var and of the mean with the term the stream
// leaves out, t_a = W f_a + d_a M[:, p] and mean_a,b = mu_a + f_a . Z[:, b] + d_a alpha[p][b].
// Thread j sums over S in ascending order; the squares are added over the threads in a fixed order.
__global__ __launch_bounds__(CR_B) void fpost_sensor_kernel(
    const double* __restrict__ F, int64_t S, int64_t ldf, const double* __restrict__ noise, int k,
    FpostDev w, const double* __restrict__ dg, double* __restrict__ var,
    const double* __restrict__ mu, double* __restrict__ out, int64_t ldo, int nrhs,
    const int* __restrict__ gate) {
  if (gate && *gate != 0) return;
  const int p = blockIdx.x;
  const int64_t a = w.sens[p];
  const double* __restrict__ fa = F + a * ldf;
  const double d = noise ? noise[a] : 0.0;
  if (var) {
    double ss = 0.0;
    for (int j = threadIdx.x; j < k; j += CR_B) {
      double t = 0.0;
      for (int64_t s = 0; s < S; ++s) t = fma(w.Wt[s * w.kp + j], fa[s], t);
      t = fma(d, w.M[(int64_t)j * k + p], t);
      ss = fma(t, t, ss);
    }
    ss = crit_block_sum(ss);
    if (threadIdx.x == 0) var[a] = dg[a] - ss;
  }
  if (out) {
    for (int b = threadIdx.x; b < nrhs; b += CR_B) {
      double t = 0.0;
      for (int64_t s = 0; s < S; ++s) t = fma(w.Z[s * w.bp + b], fa[s], t);
      out[a * ldo + b] = ((mu ? mu[a] : 0.0) + t) + d * w.alpha[(int64_t)p * w.bp + b];
    }
  }
}

// F_A [k][S], d_A + sigma2, and the sensors kept for every apply
__global__ __launch_bounds__(CR_B) void fpost_gather_kernel(const double* __restrict__ F, int64_t S,
                                                            int64_t ldf,
                                                            const double* __restrict__ noise,
                                                            const int64_t* __restrict__ sensors,
                                                            double sigma2, FpostDev w) {
  const int p = blockIdx.x;
  const int64_t a = sensors[p];
  for (int64_t s = threadIdx.x; s < S; s += CR_B) w.FA[p * S + s] = F[a * ldf + s];
  if (threadIdx.x == 0) {
    w.sens[p] = a;
    w.dA[p] = (noise ? noise[a] : 0.0) + sigma2;
  }
}

// before the factorization: G += diag(d_A + sigma2); after it: zeros above the diagonal of M, and
// the status where apply finds it
__global__ void fpost_square_kernel(int k, FpostDev w, int after, const int* __restrict__ info) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (after && e == 0) *w.status = *info;
  if (e >= (int64_t)k * k) return;
  const int64_t i = e / k, j = e - i * k;
  if (!after && i == j) w.M[e] += w.dA[i];
  if (after && j > i) w.M[e] = 0.0;
}

// R [k][bp] = Y - mu_A, zero in the columns past nrhs (so are T, alpha and Z then)
__global__ void fpost_rhs_kernel(int k, int nrhs, const double* __restrict__ Y, int64_t ldy,
                                 const double* __restrict__ mu, FpostDev w) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)k * w.bp) return;
  const int64_t p = e / w.bp, b = e - p * w.bp;
  w.R[e] = b < nrhs ? Y[p * ldy + b] - (mu ? mu[w.sens[p]] : 0.0) : 0.0;
}

static int fpost_init_run(const SFactor& f, int64_t n, const int64_t* sensors, int k,
                          double sigma2, int* info, const FpostWS& w, hipStream_t s) {
  const int64_t S = f.S;
  ProfScope ps("criteria_fpost_init", s, 2.0 * (double)k * k * (S + S + k / 3.0),
               8.0 * ((double)n * S + 3.0 * k * S));
  VG_TRY(factor_diag_launch(f, n, w.dg, s));
  hipLaunchKernelGGL(fpost_gather_kernel, dim3((unsigned)k), dim3(CR_B), 0, s, f.F, S, f.ldf,
                     f.noise, sensors, sigma2, w);
  VG_LAUNCH_CHECK();
  VG_TRY(gemm_launch(0, 1, k, k, S, 1.0, w.FA, S, w.FA, S, 0.0, w.M, k, VGPOSP_FULL, 0, 0, s));
  const unsigned kb = (unsigned)ceil_div((int64_t)k * k, 256);
  hipLaunchKernelGGL(fpost_square_kernel, dim3(kb), dim3(256), 0, s, k, w, 0, info);
  VG_LAUNCH_CHECK();
  VG_HIP(vg_memset(info, 0, sizeof(int), s));
  VG_TRY(potrf_one(w.M, k, k, 1, nullptr, info, w.potrf, s, false, true, w.compact));
  hipLaunchKernelGGL(fpost_square_kernel, dim3(kb), dim3(256), 0, s, k, w, 1, info);
  VG_LAUNCH_CHECK();
  // Wt = (M F_A)^T = F_A^T M^T, the columns k .. kp zero
  VG_HIP(vg_memset(w.Wt, 0, (size_t)S * w.kp * 8, s));
  VG_TRY(gemm_launch(1, 1, S, k, k, 1.0, w.FA, S, w.M, k, 0.0, w.Wt, w.kp, VGPOSP_FULL, 0, 0, s));
  return 0;
}

static void fpost_stream_launch(const SFactor& f, int64_t n, int nf, const double* Pv, int64_t ldv,
                                int nvf, const double* Pz, int64_t ldz, int first,
                                const double* dg, double* var, const double* mu, double* out,
                                int64_t ldo, int b0, int nrhs, const int* gate, hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(n, FP_ROWS));
  const bool vec = symv_vec(f.F, f.ldf);
#define FP_STREAM(VEC, NF)                                                                      \
  hipLaunchKernelGGL((fpost_stream_kernel<VEC, NF>), grid, dim3(FC_TH), 0, s, f.F, n, f.S,      \
                     f.ldf, Pv, ldv, nvf, Pz, ldz, first, dg, var, mu, out, ldo, b0, nrhs, gate)
#define FP_STREAM_NF(NF) \
  if (vec) FP_STREAM(true, NF); else FP_STREAM(false, NF)
  switch (nf) {
    case 1: FP_STREAM_NF(1); break;
    case 2: FP_STREAM_NF(2); break;
    case 3: FP_STREAM_NF(3); break;
    default: FP_STREAM_NF(4); break;
  }
#undef FP_STREAM_NF
#undef FP_STREAM
}

static int fpost_apply_run(const SFactor& f, int64_t n, int k, double* var, const double* Y,
                           int64_t ldy, int nrhs, const double* mu, double* out, int64_t ldo,
                           const FpostWS& w, hipStream_t s) {
  const int64_t S = f.S;
  const int* info = w.status;
  const bool mean = Y != nullptr && nrhs > 0;
  if (mean) {
    ProfScope ps("criteria_fpost_rhs", s, 2.0 * w.bp * k * (2.0 * k + S),
                 8.0 * ((double)k * k + (double)k * S + 2.0 * S * w.bp));
    hipLaunchKernelGGL(fpost_rhs_kernel, dim3((unsigned)ceil_div((int64_t)k * w.bp, 256)),
                       dim3(256), 0, s, k, nrhs, Y, ldy, mu, w);
    VG_LAUNCH_CHECK();
    VG_TRY(gemm_launch(0, 0, k, w.bp, k, 1.0, w.M, k, w.R, w.bp, 0.0, w.T, w.bp, VGPOSP_FULL, 0, 0,
                       s));
    VG_TRY(gemm_launch(1, 0, k, w.bp, k, 1.0, w.M, k, w.T, w.bp, 0.0, w.alpha, w.bp, VGPOSP_FULL,
                       0, 0, s));
    VG_TRY(gemm_launch(1, 0, S, w.bp, k, 1.0, w.FA, S, w.alpha, w.bp, 0.0, w.Z, w.bp, VGPOSP_FULL,
                       0, 0, s));
  }
  // the fragments asked for: the variance's first, then the mean's, four to a panel
  const int nv = var ? w.kp / 16 : 0, nm = mean ? w.bp / 16 : 0;
  for (int f0 = 0; f0 < nv + nm; f0 += FP_NF) {
    const int nf = std::min(FP_NF, nv + nm - f0);
    const int nvf = std::max(0, std::min(nv - f0, nf)), m0 = std::max(0, f0 - nv);
    const double ns = (double)n * (double)S;
    ProfScope ps("criteria_fpost_stream", s, 2.0 * ns * 16.0 * nf,
                 8.0 * ns + 8.0 * (double)n * ((nvf ? 1 : 0) + std::min(16 * (nf - nvf), nrhs)));
    fpost_stream_launch(f, n, nf, w.Wt + 16 * f0, w.kp, nvf, w.Z + 16 * m0, w.bp, f0 == 0, w.dg,
                        var, mu, out, ldo, 16 * m0, nrhs, info, s);
    VG_LAUNCH_CHECK();
  }
  if (var || mean) {
    hipLaunchKernelGGL(fpost_sensor_kernel, dim3((unsigned)k), dim3(CR_B), 0, s, f.F, S, f.ldf,
                       f.noise, k, w, w.dg, var, mu, mean ? out : nullptr, ldo, nrhs, info);
    VG_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace vgposp

using namespace vgposp;

extern "C" size_t vgposp_symv_upper_workspace_bytes(int64_t n) {
  if (n <= 0) return 0;
  return symv_layout(nullptr, n).bytes;
}

template <bool SQ>
static int symv_entry(const char* fn, const double* A, int64_t n, int64_t lda, const double* diag,
                      const double* x, double* y, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (n == 0) return 0;
  VG_TRY(check_sigma(fn, 1, SigmaStored{A, lda, diag}, n));
  const SymvWS w = symv_layout(ws, n);
  VG_TRY(check_pass(fn, 5, x, y, ws, ws_bytes, w.bytes));
  symv_launch<SQ>(A, n, lda, diag, x, y, w, nullptr, as_stream(stream));
  VG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vgposp_symv_upper(const double* A, int64_t n, int64_t lda, const double* diag,
                                 const double* x, double* y, void* ws, size_t ws_bytes,
                                 void* stream) {
  return symv_entry<false>(__func__, A, n, lda, diag, x, y, ws, ws_bytes, stream);
}

extern "C" int vgposp_symv_upper_sq(const double* A, int64_t n, int64_t lda, const double* diag,
                                    const double* x, double* y, void* ws, size_t ws_bytes,
                                    void* stream) {
  return symv_entry<true>(__func__, A, n, lda, diag, x, y, ws, ws_bytes, stream);
}

extern "C" size_t vgposp_crit_workspace_bytes(int64_t n, int kmax) {
  if (n <= 0 || kmax <= 0) return 0;
  return crit_layout(nullptr, n, kmax).bytes;
}

extern "C" int vgposp_crit_init(const double* Sigma, int64_t n, int64_t lda, const double* diag,
                                int kmax, int criterion, double threshold,
                                const unsigned char* targets, const unsigned char* allowed,
                                void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const SigmaStored sg{Sigma, lda, diag};
  VG_TRY(check_sigma(__func__, 1, sg, n));
  VG_TRY(check_rule(__func__, 5, kmax, n, &criterion, threshold));
  VG_CHECK_ARG(ws != nullptr, 10);
  const CritWS w = crit_layout(ws, n, kmax);
  VG_CHECK_WS(ws_bytes, w.bytes);
  return crit_init_run(sg, InV{}, n, 0, criterion, threshold, targets, nullptr, allowed, w,
                       as_stream(stream));
}

extern "C" int vgposp_crit_step(const double* Sigma, int64_t n, int64_t lda, const double* diag,
                                int kmax, int round, const int64_t* forced, int64_t j,
                                int64_t* selected, double* sel_delta, void* ws, size_t ws_bytes,
                                void* stream) {
  clear_error();
  const SigmaStored sg{Sigma, lda, diag};
  VG_TRY(check_sigma(__func__, 1, sg, n));
  VG_TRY(check_round(__func__, 5, kmax, n, round, forced, j, selected));
  VG_CHECK_ARG(ws != nullptr, 11);
  const CritWS w = crit_layout(ws, n, kmax);
  VG_CHECK_WS(ws_bytes, w.bytes);
  return crit_step_run(sg, InV{}, n, 0, round, forced, j, selected, sel_delta, w,
                       as_stream(stream));
}

extern "C" int vgposp_crit_buffers(void* ws, int64_t n, int kmax, double** nom, double** score,
                                   double** delta, double** W) {
  clear_error();
  VG_TRY(check_buffers(__func__, ws, n, nullptr, kmax));
  crit_outputs(crit_layout(ws, n, kmax), nom, score, delta, W);
  return 0;
}

extern "C" size_t vgposp_gemv_t_workspace_bytes(int64_t P, int64_t n) {
  if (P <= 0 || n <= 0) return 0;
  return gemv_t_bytes(P, n);
}

template <bool SQ>
static int gemv_t_entry(const char* fn, const double* R, int64_t P, int64_t n, int64_t ldr,
                        const double* x, double* y, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (P == 0 || n == 0) return 0;
  VG_TRY(check_cross(fn, 1, CrossStored{R, ldr}, P, n, true));
  VG_TRY(check_pass(fn, 5, x, y, ws, ws_bytes, gemv_t_bytes(P, n)));
  gemv_t_launch<SQ>(R, P, n, ldr, x, y, static_cast<double*>(ws), nullptr, as_stream(stream));
  VG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vgposp_gemv_t(const double* R, int64_t P, int64_t n, int64_t ldr, const double* x,
                             double* y, void* ws, size_t ws_bytes, void* stream) {
  return gemv_t_entry<false>(__func__, R, P, n, ldr, x, y, ws, ws_bytes, stream);
}

extern "C" int vgposp_gemv_t_sq(const double* R, int64_t P, int64_t n, int64_t ldr,
                                const double* x, double* y, void* ws, size_t ws_bytes,
                                void* stream) {
  return gemv_t_entry<true>(__func__, R, P, n, ldr, x, y, ws, ws_bytes, stream);
}

extern "C" size_t vgposp_critx_workspace_bytes(int64_t n, int64_t P, int kmax) {
  if (n <= 0 || P <= 0 || kmax <= 0) return 0;
  return critx_layout(nullptr, n, P, kmax, gemv_t_bytes(P, n)).bytes;
}

extern "C" int vgposp_critx_init(const double* Sigma, int64_t n, int64_t lda, const double* diag,
                                 const double* R, int64_t P, int64_t ldr, const double* weights,
                                 int kmax, double threshold, const unsigned char* allowed,
                                 void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const SigmaStored sg{Sigma, lda, diag};
  const CrossStored cr{R, ldr};
  VG_TRY(check_sigma(__func__, 1, sg, n));
  VG_TRY(check_cross(__func__, 5, cr, P, n));
  VG_TRY(check_rule(__func__, 9, kmax, n, nullptr, threshold));
  VG_CHECK_ARG(ws != nullptr, 12);
  const CritXWS w = critx_layout(ws, n, P, kmax, gemv_t_bytes(P, n));
  VG_CHECK_WS(ws_bytes, w.bytes);
  return crit_init_run(sg, cr, n, P, VGPOSP_CRIT_VARIANCE, threshold, nullptr, weights, allowed, w,
                       as_stream(stream));
}

extern "C" int vgposp_critx_step(const double* Sigma, int64_t n, int64_t lda, const double* diag,
                                 const double* R, int64_t P, int64_t ldr, int kmax, int round,
                                 const int64_t* forced, int64_t j, int64_t* selected,
                                 double* sel_delta, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const SigmaStored sg{Sigma, lda, diag};
  const CrossStored cr{R, ldr};
  VG_TRY(check_sigma(__func__, 1, sg, n));
  VG_TRY(check_cross(__func__, 5, cr, P, n));
  VG_TRY(check_round(__func__, 8, kmax, n, round, forced, j, selected));
  VG_CHECK_ARG(ws != nullptr, 14);
  const CritXWS w = critx_layout(ws, n, P, kmax, gemv_t_bytes(P, n));
  VG_CHECK_WS(ws_bytes, w.bytes);
  return crit_step_run(sg, cr, n, P, round, forced, j, selected, sel_delta, w, as_stream(stream));
}

extern "C" int vgposp_critx_buffers(void* ws, int64_t n, int64_t P, int kmax, double** nom,
                                    double** score, double** delta, double** W, double** U) {
  clear_error();
  VG_TRY(check_buffers(__func__, ws, n, &P, kmax));
  critx_outputs(critx_layout(ws, n, P, kmax, gemv_t_bytes(P, n)), nom, score, delta, W, U);
  return 0;
}

// ---- the matrix-free pass and the rounds on a generated R ----
extern "C" size_t vgposp_kernel_gemv_t_workspace_bytes(int64_t P, int64_t n) {
  if (P <= 0 || n <= 0) return 0;
  return kgemv_t_bytes(P, n);
}

template <bool SQ>
static int kgemv_t_entry(const char* fn, const KGen& g, int64_t P, int64_t n, const double* x,
                         double* y, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (P == 0 || n == 0) return 0;
  VG_TRY(check_cross(fn, 1, g, P, n, true));
  VG_TRY(check_pass(fn, 11, x, y, ws, ws_bytes, kgemv_t_bytes(P, n)));
  kgemv_t_launch<SQ>(g, P, n, x, y, static_cast<double*>(ws), nullptr, as_stream(stream));
  VG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vgposp_kernel_gemv_t(int kind, const double* Xt, int64_t P, const double* X,
                                    int64_t n, int d, const double* amp, const double* ls,
                                    const double* target_scale, const double* site_scale,
                                    const double* x, double* y, void* ws, size_t ws_bytes,
                                    void* stream) {
  return kgemv_t_entry<false>(__func__, KGen{kind, d, Xt, X, amp, ls, target_scale, site_scale}, P,
                              n, x, y, ws, ws_bytes, stream);
}

extern "C" int vgposp_kernel_gemv_t_sq(int kind, const double* Xt, int64_t P, const double* X,
                                       int64_t n, int d, const double* amp, const double* ls,
                                       const double* target_scale, const double* site_scale,
                                       const double* x, double* y, void* ws, size_t ws_bytes,
                                       void* stream) {
  return kgemv_t_entry<true>(__func__, KGen{kind, d, Xt, X, amp, ls, target_scale, site_scale}, P,
                             n, x, y, ws, ws_bytes, stream);
}

extern "C" size_t vgposp_critk_workspace_bytes(int64_t n, int64_t P, int kmax) {
  if (n <= 0 || P <= 0 || kmax <= 0) return 0;
  return critx_layout(nullptr, n, P, kmax, kgemv_t_bytes(P, n)).bytes;
}

extern "C" int vgposp_critk_init(const double* Sigma, int64_t n, int64_t lda, const double* diag,
                                 int kind, const double* Xt, int64_t P, const double* X, int d,
                                 const double* amp, const double* ls, const double* target_scale,
                                 const double* site_scale, const double* weights, int kmax,
                                 double threshold, const unsigned char* allowed, void* ws,
                                 size_t ws_bytes, void* stream) {
  clear_error();
  const SigmaStored sg{Sigma, lda, diag};
  const KGen g{kind, d, Xt, X, amp, ls, target_scale, site_scale};
  VG_TRY(check_sigma(__func__, 1, sg, n));
  VG_TRY(check_cross(__func__, 5, g, P, n));
  VG_TRY(check_rule(__func__, 15, kmax, n, nullptr, threshold));
  VG_CHECK_ARG(ws != nullptr, 18);
  const CritXWS w = critx_layout(ws, n, P, kmax, kgemv_t_bytes(P, n));
  VG_CHECK_WS(ws_bytes, w.bytes);
  return crit_init_run(sg, g, n, P, VGPOSP_CRIT_VARIANCE, threshold, nullptr, weights, allowed, w,
                       as_stream(stream));
}

extern "C" int vgposp_critk_step(const double* Sigma, int64_t n, int64_t lda, const double* diag,
                                 int kind, const double* Xt, int64_t P, const double* X, int d,
                                 const double* amp, const double* ls, const double* target_scale,
                                 const double* site_scale, int kmax, int round,
                                 const int64_t* forced, int64_t j, int64_t* selected,
                                 double* sel_delta, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const SigmaStored sg{Sigma, lda, diag};
  const KGen g{kind, d, Xt, X, amp, ls, target_scale, site_scale};
  VG_TRY(check_sigma(__func__, 1, sg, n));
  VG_TRY(check_cross(__func__, 5, g, P, n));
  VG_TRY(check_round(__func__, 14, kmax, n, round, forced, j, selected));
  VG_CHECK_ARG(ws != nullptr, 20);
  const CritXWS w = critx_layout(ws, n, P, kmax, kgemv_t_bytes(P, n));
  VG_CHECK_WS(ws_bytes, w.bytes);
  return crit_step_run(sg, g, n, P, round, forced, j, selected, sel_delta, w, as_stream(stream));
}

extern "C" int vgposp_critk_buffers(void* ws, int64_t n, int64_t P, int kmax, double** nom,
                                    double** score, double** delta, double** W, double** U) {
  clear_error();
  VG_TRY(check_buffers(__func__, ws, n, &P, kmax));
  critx_outputs(critx_layout(ws, n, P, kmax, kgemv_t_bytes(P, n)), nom, score, delta, W, U);
  return 0;
}

// ---- Sigma generated from the points: the pass and the rounds ----
extern "C" size_t vgposp_kernel_symv_workspace_bytes(int64_t n) {
  if (n <= 0) return 0;
  return ksymv_layout(nullptr, n).bytes;
}

template <bool SQ>
static int ksymv_entry(const char* fn, const SGen& g, int64_t n, const double* x, double* y,
                       void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (n == 0) return 0;
  VG_TRY(check_sigma(fn, 1, g, n));
  const KSymvWS w = ksymv_layout(ws, n);
  VG_TRY(check_pass(fn, 9, x, y, ws, ws_bytes, w.bytes));
  ksymv_launch<SQ>(g, n, x, y, w, nullptr, as_stream(stream));
  VG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vgposp_kernel_symv(int kind, const double* X, int64_t n, int d, const double* amp,
                                  const double* ls, const double* site_scale, const double* diag,
                                  const double* x, double* y, void* ws, size_t ws_bytes,
                                  void* stream) {
  return ksymv_entry<false>(__func__, SGen{kind, d, X, amp, ls, site_scale, diag}, n, x, y, ws,
                            ws_bytes, stream);
}

extern "C" int vgposp_kernel_symv_sq(int kind, const double* X, int64_t n, int d,
                                     const double* amp, const double* ls,
                                     const double* site_scale, const double* diag, const double* x,
                                     double* y, void* ws, size_t ws_bytes, void* stream) {
  return ksymv_entry<true>(__func__, SGen{kind, d, X, amp, ls, site_scale, diag}, n, x, y, ws,
                           ws_bytes, stream);
}

static CritWS critg_layout(void* base, int64_t n, int kmax) {
  return crit_layout(base, n, kmax, ksymv_layout(nullptr, n).bytes);
}

extern "C" size_t vgposp_critg_workspace_bytes(int64_t n, int kmax) {
  if (n <= 0 || kmax <= 0) return 0;
  return critg_layout(nullptr, n, kmax).bytes;
}

extern "C" int vgposp_critg_init(int kind, const double* X, int64_t n, int d, const double* amp,
                                 const double* ls, const double* site_scale, const double* diag,
                                 int kmax, int criterion, double threshold,
                                 const unsigned char* targets, const unsigned char* allowed,
                                 void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const SGen sg{kind, d, X, amp, ls, site_scale, diag};
  VG_TRY(check_sigma(__func__, 1, sg, n));
  VG_TRY(check_rule(__func__, 9, kmax, n, &criterion, threshold));
  VG_CHECK_ARG(ws != nullptr, 14);
  const CritWS w = critg_layout(ws, n, kmax);
  VG_CHECK_WS(ws_bytes, w.bytes);
  return crit_init_run(sg, InV{}, n, 0, criterion, threshold, targets, nullptr, allowed, w,
                       as_stream(stream));
}

extern "C" int vgposp_critg_step(int kind, const double* X, int64_t n, int d, const double* amp,
                                 const double* ls, const double* site_scale, const double* diag,
                                 int kmax, int round, const int64_t* forced, int64_t j,
                                 int64_t* selected, double* sel_delta, void* ws, size_t ws_bytes,
                                 void* stream) {
  clear_error();
  const SGen sg{kind, d, X, amp, ls, site_scale, diag};
  VG_TRY(check_sigma(__func__, 1, sg, n));
  VG_TRY(check_round(__func__, 9, kmax, n, round, forced, j, selected));
  VG_CHECK_ARG(ws != nullptr, 15);
  const CritWS w = critg_layout(ws, n, kmax);
  VG_CHECK_WS(ws_bytes, w.bytes);
  return crit_step_run(sg, InV{}, n, 0, round, forced, j, selected, sel_delta, w,
                       as_stream(stream));
}

extern "C" int vgposp_critg_buffers(void* ws, int64_t n, int kmax, double** nom, double** score,
                                    double** delta, double** W) {
  clear_error();
  VG_TRY(check_buffers(__func__, ws, n, nullptr, kmax));
  crit_outputs(critg_layout(ws, n, kmax), nom, score, delta, W);
  return 0;
}

// Both sides generated: the rounds never pass over Sigma, so the location side has no partials.
static CritXWS critgk_layout(void* base, int64_t n, int64_t P, int kmax) {
  return critx_layout(base, n, P, kmax, kgemv_t_bytes(P, n), 0);
}

extern "C" size_t vgposp_critgk_workspace_bytes(int64_t n, int64_t P, int kmax) {
  if (n <= 0 || P <= 0 || kmax <= 0) return 0;
  return critgk_layout(nullptr, n, P, kmax).bytes;
}

// (n, diag) stand for Sigma: its points, kernel and site scale are those of the generated R
extern "C" int vgposp_critgk_init(int64_t n, const double* diag, int kind, const double* Xt,
                                  int64_t P, const double* X, int d, const double* amp,
                                  const double* ls, const double* target_scale,
                                  const double* site_scale, const double* weights, int kmax,
                                  double threshold, const unsigned char* allowed, void* ws,
                                  size_t ws_bytes, void* stream) {
  clear_error();
  const KGen g{kind, d, Xt, X, amp, ls, target_scale, site_scale};
  VG_CHECK_ARG(n >= 1 && n <= CR_NMAX, 1);
  VG_TRY(check_cross(__func__, 3, g, P, n));
  VG_TRY(check_rule(__func__, 13, kmax, n, nullptr, threshold));
  VG_CHECK_ARG(ws != nullptr, 16);
  const CritXWS w = critgk_layout(ws, n, P, kmax);
  VG_CHECK_WS(ws_bytes, w.bytes);
  return crit_init_run(SGen{kind, d, X, amp, ls, site_scale, diag}, g, n, P, VGPOSP_CRIT_VARIANCE,
                       threshold, nullptr, weights, allowed, w, as_stream(stream));
}

extern "C" int vgposp_critgk_step(int64_t n, const double* diag, int kind, const double* Xt,
                                  int64_t P, const double* X, int d, const double* amp,
                                  const double* ls, const double* target_scale,
                                  const double* site_scale, int kmax, int round,
                                  const int64_t* forced, int64_t j, int64_t* selected,
                                  double* sel_delta, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const KGen g{kind, d, Xt, X, amp, ls, target_scale, site_scale};
  VG_CHECK_ARG(n >= 1 && n <= CR_NMAX, 1);
  VG_TRY(check_cross(__func__, 3, g, P, n));
  VG_TRY(check_round(__func__, 12, kmax, n, round, forced, j, selected));
  VG_CHECK_ARG(ws != nullptr, 18);
  const CritXWS w = critgk_layout(ws, n, P, kmax);
  VG_CHECK_WS(ws_bytes, w.bytes);
  return crit_step_run(SGen{kind, d, X, amp, ls, site_scale, diag}, g, n, P, round, forced, j,
                       selected, sel_delta, w, as_stream(stream));
}

extern "C" int vgposp_critgk_buffers(void* ws, int64_t n, int64_t P, int kmax, double** nom,
                                     double** score, double** delta, double** W, double** U) {
  clear_error();
  VG_TRY(check_buffers(__func__, ws, n, &P, kmax));
  critx_outputs(critgk_layout(ws, n, P, kmax), nom, score, delta, W, U);
  return 0;
}

// ---- Sigma generated from a factor: the passes and the rounds ----
extern "C" size_t vgposp_factor_symv_workspace_bytes(int64_t n, int64_t s) {
  if (n <= 0 || s <= 0) return 0;
  return fac_layout(nullptr, n, s).bytes;
}

template <bool SQ>
static int fsymv_entry(const char* fn, const SFactor& f, int64_t n, const double* x, double* y,
                       void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  if (n == 0) return 0;
  VG_TRY(check_sigma(fn, 1, f, n, FC_NMAX));
  const FacWS w = fac_layout(ws, n, f.S);
  VG_TRY(check_pass(fn, 6, x, y, ws, ws_bytes, w.bytes));
  hipStream_t s = as_stream(stream);
  if (SQ) {
    VG_TRY(factor_diag_launch(f, n, w.dg, s));
    return factor_symv_sq_launch(f, n, x, y, w, s);
  }
  return factor_symv_launch(f, n, x, y, w, nullptr, s);
}

extern "C" int vgposp_factor_symv(const double* F, int64_t n, int64_t s, int64_t ldf,
                                  const double* noise, const double* x, double* y, void* ws,
                                  size_t ws_bytes, void* stream) {
  return fsymv_entry<false>(__func__, SFactor{F, s, ldf, noise}, n, x, y, ws, ws_bytes, stream);
}

extern "C" int vgposp_factor_symv_sq(const double* F, int64_t n, int64_t s, int64_t ldf,
                                     const double* noise, const double* x, double* y, void* ws,
                                     size_t ws_bytes, void* stream) {
  return fsymv_entry<true>(__func__, SFactor{F, s, ldf, noise}, n, x, y, ws, ws_bytes, stream);
}

static CritWS critf_layout(void* base, int64_t n, int64_t S, int kmax) {
  return crit_layout(base, n, kmax, fac_layout(nullptr, n, S).bytes);
}

extern "C" size_t vgposp_critf_workspace_bytes(int64_t n, int64_t s, int kmax) {
  if (n <= 0 || s <= 0 || kmax <= 0) return 0;
  return critf_layout(nullptr, n, s, kmax).bytes;
}

extern "C" int vgposp_critf_init(const double* F, int64_t n, int64_t s, int64_t ldf,
                                 const double* noise, int kmax, int criterion, double threshold,
                                 const unsigned char* targets, const unsigned char* allowed,
                                 void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const SFactor sg{F, s, ldf, noise};
  VG_TRY(check_sigma(__func__, 1, sg, n));
  VG_TRY(check_rule(__func__, 6, kmax, n, &criterion, threshold));
  VG_CHECK_ARG(ws != nullptr, 11);
  const CritWS w = critf_layout(ws, n, s, kmax);
  VG_CHECK_WS(ws_bytes, w.bytes);
  return crit_init_run(sg, InV{}, n, 0, criterion, threshold, targets, nullptr, allowed, w,
                       as_stream(stream));
}

extern "C" int vgposp_critf_step(const double* F, int64_t n, int64_t s, int64_t ldf,
                                 const double* noise, int kmax, int round, const int64_t* forced,
                                 int64_t j, int64_t* selected, double* sel_delta, void* ws,
                                 size_t ws_bytes, void* stream) {
  clear_error();
  const SFactor sg{F, s, ldf, noise};
  VG_TRY(check_sigma(__func__, 1, sg, n));
  VG_TRY(check_round(__func__, 6, kmax, n, round, forced, j, selected));
  VG_CHECK_ARG(ws != nullptr, 12);
  const CritWS w = critf_layout(ws, n, s, kmax);
  VG_CHECK_WS(ws_bytes, w.bytes);
  return crit_step_run(sg, InV{}, n, 0, round, forced, j, selected, sel_delta, w,
                       as_stream(stream));
}

extern "C" int vgposp_critf_buffers(void* ws, int64_t n, int64_t s, int kmax, double** nom,
                                    double** score, double** delta, double** W) {
  clear_error();
  VG_TRY(check_buffers(__func__, ws, n, &s, kmax));
  crit_outputs(critf_layout(ws, n, s, kmax), nom, score, delta, W);
  return 0;
}

// ---- mutual information on a factor (Woodbury): the full greedy of placement_algorithm2.py:128-145
// with the deltas of :371-413, on main.py:190-199's covariance ----
static int check_noise(const char* fn, const SFactor& f) {
  VG_ARG(f.noise != nullptr, 5);
  return 0;
}

extern "C" size_t vgposp_fmi_workspace_bytes(int64_t n, int64_t s, int kmax) {
  if (n <= 0 || s <= 0 || kmax <= 0) return 0;
  if (s > FC_SMAX) s = FC_SMAX;  // the entries refuse it; the query stays finite
  return fmi_layout(nullptr, n, s, kmax).bytes;
}

extern "C" int vgposp_fmi_init(const double* F, int64_t n, int64_t s, int64_t ldf,
                               const double* noise, int kmax, double threshold,
                               const unsigned char* allowed, int* info, void* ws, size_t ws_bytes,
                               void* stream) {
  clear_error();
  const SFactor sg{F, s, ldf, noise};
  VG_TRY(check_sigma(__func__, 1, sg, n));
  VG_TRY(check_noise(__func__, sg));
  VG_TRY(check_rule(__func__, 6, kmax, n, nullptr, threshold));
  VG_CHECK_ARG(info != nullptr, 9);
  VG_CHECK_ARG(ws != nullptr, 10);
  const FmiWS w = fmi_layout(ws, n, s, kmax);
  VG_CHECK_WS(ws_bytes, w.bytes);
  return fmi_init_run(sg, n, kmax, threshold, allowed, info, w, as_stream(stream));
}

extern "C" int vgposp_fmi_step(const double* F, int64_t n, int64_t s, int64_t ldf,
                               const double* noise, int kmax, int round, const int64_t* forced,
                               int64_t j, int64_t* selected, double* sel_delta, void* ws,
                               size_t ws_bytes, void* stream) {
  clear_error();
  const SFactor sg{F, s, ldf, noise};
  VG_TRY(check_sigma(__func__, 1, sg, n));
  VG_TRY(check_noise(__func__, sg));
  VG_TRY(check_round(__func__, 6, kmax, n, round, forced, j, selected));
  VG_CHECK_ARG(ws != nullptr, 12);
  const FmiWS w = fmi_layout(ws, n, s, kmax);
  VG_CHECK_WS(ws_bytes, w.bytes);
  return fmi_step_run(sg, n, kmax, round, forced, j, selected, sel_delta, w, as_stream(stream));
}

extern "C" int vgposp_fmi_buffers(void* ws, int64_t n, int64_t s, int kmax, double** nom,
                                  double** prec, double** delta, double** W, double** V) {
  clear_error();
  VG_TRY(check_buffers(__func__, ws, n, &s, kmax));
  VG_CHECK_ARG(s <= FC_SMAX, 3);
  const FmiWS w = fmi_layout(ws, n, s, kmax);
  if (nom) *nom = w.nom;
  if (prec) *prec = w.prec;
  if (delta) *delta = w.delta;
  if (W) *W = w.W;
  if (V) *V = w.V;
  return 0;
}

// ---- field reconstruction on a factor: main.py:190-199's covariance, conditioned on the picks ----
// (F, n, s, ldf, noise) at 1, k at `at`
static int check_fpost(const char* fn, const SFactor& f, int64_t n, int k, int at) {
  VG_TRY(check_sigma(fn, 1, f, n, FC_NMAX));
  VG_ARG(k >= 1 && k <= FP_KMAX && k <= n, at);
  return 0;
}

extern "C" size_t vgposp_fpost_workspace_bytes(int64_t n, int64_t s, int k, int nrhs_max) {
  if (n <= 0 || s <= 0 || k <= 0) return 0;
  if (s > FC_SMAX) s = FC_SMAX;  // the entries refuse these; the query stays finite
  if (k > FP_KMAX) k = FP_KMAX;
  nrhs_max = std::max(0, std::min(nrhs_max, FP_BMAX));
  return fpost_layout(nullptr, n, s, k, nrhs_max).bytes;
}

extern "C" int vgposp_fpost_init(const double* F, int64_t n, int64_t s, int64_t ldf,
                                 const double* noise, const int64_t* sensors, int k,
                                 double obs_noise, int* info, void* ws, size_t ws_bytes,
                                 void* stream) {
  clear_error();
  const SFactor sg{F, s, ldf, noise};
  VG_TRY(check_fpost(__func__, sg, n, k, 7));
  VG_CHECK_ARG(sensors != nullptr, 6);
  VG_CHECK_ARG(obs_noise >= 0.0 && obs_noise <= DBL_MAX, 8);
  VG_CHECK_ARG(info != nullptr, 9);
  VG_CHECK_ARG(ws != nullptr, 10);
  const FpostWS w = fpost_layout(ws, n, s, k, 0);
  VG_CHECK_WS(ws_bytes, w.bytes);
  return fpost_init_run(sg, n, sensors, k, obs_noise, info, w, as_stream(stream));
}

extern "C" int vgposp_fpost_apply(const double* F, int64_t n, int64_t s, int64_t ldf,
                                  const double* noise, int k, double* var, const double* Y,
                                  int64_t ldy, int nrhs, const double* mu, double* out,
                                  int64_t ldo, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  const SFactor sg{F, s, ldf, noise};
  VG_TRY(check_fpost(__func__, sg, n, k, 6));
  VG_CHECK_ARG(Y == nullptr || nrhs <= 0 || ldy >= nrhs, 9);
  VG_CHECK_ARG(nrhs >= 0 && nrhs <= FP_BMAX, 10);
  if (Y == nullptr) nrhs = 0;
  VG_CHECK_ARG(nrhs == 0 || out != nullptr, 12);
  VG_CHECK_ARG(nrhs == 0 || ldo >= nrhs, 13);
  VG_CHECK_ARG(ws != nullptr, 14);
  const FpostWS w = fpost_layout(ws, n, s, k, nrhs);
  VG_CHECK_WS(ws_bytes, w.bytes);
  return fpost_apply_run(sg, n, k, var, Y, ldy, nrhs, mu, out, ldo, w, as_stream(stream));
}
