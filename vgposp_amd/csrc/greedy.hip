// Greedy mutual-information sensor placement, dense-exact, all on device.
//
// The reference (placement_algorithm2.py:151-219) evaluates, per candidate y,
//   nom_y   = sigma_yy - Sigma_yA pinv(Sigma_AA) Sigma_Ay                 (:371-388)
//   denom_y = sigma_yy - Sigma_yAbar pinv(Sigma_AbarAbar) Sigma_Abary     (:408-413)
// with an SVD pinv of an (N-|A|-1)^2 matrix per evaluation.  Here both are maintained for ALL
// candidates incrementally:
//   * Sigma = L L^T is factored once and inverted in the same sweep (potrf.hip): M = L^-1 in the
//     lower triangle, Sigma kept in the strictly upper triangle, diag(Sigma) saved.
//   * nom: rank-1 Cholesky rows W (W[t] = L_AA^-1 Sigma_{A,:} row t): nom_y -= w_y^2.
//   * denom = 1 / P_yy with P = (Sigma_SS)^-1, S = V \ A.  P_yy starts at Q_yy = |M e_y|^2 and is
//     downdated per selection with q = Q e_a = M^T (M e_a) (one triangular mat-vec, the HBM-bound
//     step) through rows V (V[t] = L_{Q_AA}^-1 Q_{A,:}): P_yy -= v_y^2.
// The lazy cache policy is emulated exactly: fresh deltas are computed for every candidate, every
// stale entry whose key exceeds the best fresh key is refreshed in bulk (the reference would refresh
// all of them before it could stop), and the remaining re-score loop runs in one workgroup over
// per-chunk maxima.  Keys order by value, ties by LOWER index (argmax_cache_linear, :53-67).
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <type_traits>

#include "dense.h"

namespace vgposp {

constexpr int RC = 512;     // rows per chunk of the transposed mat-vec
constexpr int CT = 256;     // columns per mat-vec workgroup
constexpr int CH = 1024;    // candidates per chunk / per update workgroup
constexpr int MAXCH = 2048; // chunks held in LDS by the select kernel -> n <= 2^21
constexpr double DELTA_EPS = 1e-8;  // placement_algorithm2.py:198

// Speculative mat-vec of vgposp_greedy_step (vgposp_greedy_set_speculation): a pass over L^-1
// forms q_a for the pick and for up to width - 1 columns the next rounds will probably ask for;
// q_c = M^T (M e_c) depends on M and c alone, so a cached column serves any later round.
constexpr int SPEC_TMAX = 8;   // largest width; the workspace is sized for it
constexpr int SPEC_HDR = 32;   // int64 words ahead of the table
// header words (device memory, written by greedy_spec_plan_kernel only)
enum { H_COUNT = 0, H_PASSES = 1, H_HITS = 2, H_HIT = 3, H_SLOT = 4, H_NB = 5, H_COL = 6,
       H_CSLOT = H_COL + SPEC_TMAX };
static_assert(H_CSLOT + SPEC_TMAX <= SPEC_HDR, "header words");
static int64_t spec_slots(int kmax) { return 4 * (int64_t)kmax; }
static std::atomic<int> g_spec_width{8};

// Variant parameters, written by vgposp_greedy_init_ex into the workspace (device memory) so the
// per-round entry points keep their signatures:
//   prm[0] jitter  eps added to the diagonal of Sigma_AA and Sigma_AbarAbar (0 for
//                  placement_algorithm2.py; 1e-6 for snippets_a2.tf_nominator :161-163)
//   prm[1] thr     |nom| or |denom| below thr -> delta = 0 (1e-8 at :198; 1e-7 at snippets_a2 :480)
//   prm[2] cinit   initial lazy-cache value (+inf at :164; INF = 1e8 at snippets_a2 :690)
struct GreedyWS {
  double *prm, *sdiag, *nom, *prec, *delta, *cache, *W, *V, *part, *xcol, *piv, *fval, *cval;
  long long *fidx, *cidx, *cnt;
  unsigned char *fresh, *selmask;
  // speculation: partial slices of columns 1 .. SPEC_TMAX-1 of a pass (slice 0 is `part`), the
  // row-interleaved right-hand sides, the cached columns q_c (these three overlay the
  // factorization scratch), and header + table (cached index and fill round per slot) followed
  // by one "is cached" byte per candidate
  double *spart, *X, *qc;
  long long* spec;
  unsigned char* cmask;
  size_t fact_off, bytes;
};

static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

static GreedyWS greedy_layout(void* base, int64_t n, int kmax) {
  GreedyWS w{};
  const int64_t nrc = ceil_div(n, RC), nch = ceil_div(n, CH);
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = p ? p + off : nullptr;
    off += align_up(bytes);
    return r;
  };
  w.prm = (double*)take(8 * 8);
  w.sdiag = (double*)take(n * 8);
  w.nom = (double*)take(n * 8);
  w.prec = (double*)take(n * 8);
  w.delta = (double*)take(n * 8);
  w.cache = (double*)take(n * 8);
  w.W = (double*)take((size_t)kmax * n * 8);
  w.V = (double*)take((size_t)kmax * n * 8);
  w.part = (double*)take((size_t)nrc * n * 8);
  w.xcol = (double*)take(n * 8);
  w.piv = (double*)take((2 + 2 * (size_t)kmax) * 8);
  w.fval = (double*)take(nch * 8);
  w.fidx = (long long*)take(nch * 8);
  w.cval = (double*)take(nch * 8);
  w.cidx = (long long*)take(nch * 8);
  w.cnt = (long long*)take(8 * 8);
  w.fresh = (unsigned char*)take(n);
  w.selmask = (unsigned char*)take(n);
  const int64_t slots = spec_slots(kmax);
  w.spec = (long long*)take((size_t)(SPEC_HDR + 2 * slots) * 8 + n);
  w.cmask = (unsigned char*)(p ? (char*)(w.spec + SPEC_HDR + 2 * slots) : nullptr);
  // factorization scratch (last).  The rounds come after the factorization, so the large areas of
  // the speculation live in the same bytes: the workspace grows by the table alone.
  w.fact_off = off;
  w.spart = (double*)take((size_t)(SPEC_TMAX - 1) * nrc * n * 8);
  w.X = (double*)take((size_t)SPEC_TMAX * n * 8);
  w.qc = (double*)take((size_t)slots * n * 8);
  off = w.fact_off + std::max(off - w.fact_off, align_up(potrf_ws_bytes(n)));
  w.bytes = off;
  return w;
}

static void* greedy_fact_ws(void* base, const GreedyWS& w, int64_t) {
  return static_cast<char*>(base) + w.fact_off;
}

// Block-wide (value, index) arg-max for blockDim == 1024.  Result valid in all threads.
__device__ __forceinline__ void block_keymax(double& v, long long& i) {
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
  const int nw = blockDim.x >> 6;
  v = (l < nw) ? sv[l] : -DBL_MAX;
  i = (l < nw) ? si[l] : -1;
  wave_keymax(v, i);  // every wave reduces the same 16 entries
}

// Saves diag(Sigma), shifts the diagonal by the jitter (the factorization is of Sigma + eps I:
// the inverse of Sigma_SS + eps I is the Schur complement of the A block of (Sigma + eps I)^-1),
// and fills the cache with its initial value.
__global__ void greedy_init_kernel(double* S, int64_t n, int64_t lda, double jitter, double thr,
                                   double cinit, GreedyWS w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const double d = S[i * lda + i];
    w.sdiag[i] = d;
    if (jitter != 0.0) S[i * lda + i] = d + jitter;
    w.cache[i] = cinit;
    w.selmask[i] = 0;
    w.cmask[i] = 0;
  }
  if (i < SPEC_HDR) w.spec[i] = 0;  // no column of the previous M survives
  if (i < 8) w.cnt[i] = 0;
  if (i == 0) {
    w.prm[0] = jitter;
    w.prm[1] = thr;
    w.prm[2] = cinit;
  }
}

// x = M e_a restricted to rows >= a (the selected column of L^-1), a = selected[round-1].  With a
// partitioned inverse only the owner of column a holds it: the others write zeros (the caller
// sum-all-reduces xcol), i.e. the column is taken only when a is in [own0, own1).
__global__ void greedy_extract_kernel(const double* M, int64_t n, int64_t lda,
                                      const int64_t* selected, int round, double* xcol,
                                      int64_t own0, int64_t own1) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t a = selected[round - 1];
  const bool own = a >= own0 && a < own1;
  if (r < n) xcol[r] = (own && r >= a) ? M[r * lda + a] : 0.0;
}

// part[rc][c] = sum_{r in chunk rc, r >= max(c, a)} M[r][c] * f(r, c)
//   SQ: f = M[r][c]          (column norms: Q_cc = |M e_c|^2)
//   else f = xcol[r]          (q = M^T x)
// Each thread owns a column pair (one 16-byte load per row, non-temporal: L^-1 is streamed once
// per round), four rows in flight; the pair's diagonal row contributes to its first column only.
constexpr int TRMV_COLS = 2 * CT;  // columns per workgroup

// f for right-hand side j; the NR values of row r sit XS doubles apart from the next row's.
template <bool SQ, int XS>
__device__ __forceinline__ double trmv_f(double m, const double* x, int64_t r, int j) {
  return SQ ? m * m : m * x[r * XS + j];
}

// The row loop of the mat-vec kernels: rows [r, r1) of the column pair (c, c + 1) against NR
// right-hand sides, sc[j] / tc[j] = the sums of column c / c + 1.  Per right-hand side the order
// is fixed: the diagonal element alone into s0, then groups of four rows from the origin r
// (s0 += f(r) + f(r+2), s1 += f(r+1) + f(r+3)), the tail rows into s0, result s0 + s1.  Every
// kernel that must agree bit for bit on a column instantiates this one source.  UNI: the caller
// guarantees c + 1 < r (a tile below the diagonal) and a workgroup-uniform r, so the x values are
// scalar loads.
template <bool SQ, int NR, int XS, bool UNI>
__device__ __forceinline__ void trmv_rows(const double* M, int64_t n, int64_t lda, int64_t c,
                                          int64_t r, int64_t r1, const double* x, int vec,
                                          double (&sc)[NR], double (&tc)[NR]) {
  typedef double d2v __attribute__((ext_vector_type(2)));
  double s0[NR], s1[NR], t0[NR], t1[NR];  // column c: s, column c + 1: t
#pragma unroll
  for (int j = 0; j < NR; ++j) s0[j] = s1[j] = t0[j] = t1[j] = 0.0;
  if (!UNI && r == c && r < r1) {  // diagonal of column c; (c, c + 1) is above the diagonal
    const double m = M[r * lda + c];
#pragma unroll
    for (int j = 0; j < NR; ++j) s0[j] += trmv_f<SQ, XS>(m, x, r, j);
    ++r;
  }
  const double* p = M + r * lda + c;
  if (vec && c + 1 < n) {
    for (; r + 3 < r1; r += 4, p += 4 * lda) {
      const d2v m0 = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p));
      const d2v m1 = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p + lda));
      const d2v m2 = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p + 2 * lda));
      const d2v m3 = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p + 3 * lda));
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        s0[j] += trmv_f<SQ, XS>(m0.x, x, r, j) + trmv_f<SQ, XS>(m2.x, x, r + 2, j);
        s1[j] += trmv_f<SQ, XS>(m1.x, x, r + 1, j) + trmv_f<SQ, XS>(m3.x, x, r + 3, j);
        t0[j] += trmv_f<SQ, XS>(m0.y, x, r, j) + trmv_f<SQ, XS>(m2.y, x, r + 2, j);
        t1[j] += trmv_f<SQ, XS>(m1.y, x, r + 1, j) + trmv_f<SQ, XS>(m3.y, x, r + 3, j);
      }
    }
    for (; r < r1; ++r, p += lda) {
      const d2v m0 = *reinterpret_cast<const d2v*>(p);
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        s0[j] += trmv_f<SQ, XS>(m0.x, x, r, j);
        t0[j] += trmv_f<SQ, XS>(m0.y, x, r, j);
      }
    }
  } else {
    for (; r < r1; ++r, p += lda) {
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        s0[j] += trmv_f<SQ, XS>(p[0], x, r, j);
        if (c + 1 < n) t0[j] += trmv_f<SQ, XS>(p[1], x, r, j);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    sc[j] = s0[j] + s1[j];
    tc[j] = t0[j] + t1[j];
  }
}

template <bool SQ>
__global__ __launch_bounds__(CT) void greedy_trmv_kernel(const double* M, int64_t n, int64_t lda,
                                                         const int64_t* selected, int round,
                                                         const double* xcol, double* part,
                                                         int64_t cbeg, int64_t cend, int vec) {
  const int64_t cb = (cbeg & ~(int64_t)1) + (int64_t)blockIdx.x * TRMV_COLS;
  const int64_t r0 = (int64_t)blockIdx.y * RC;
  const int64_t r1 = min(r0 + RC, n);
  if (cb >= r1) return;  // tile strictly above the diagonal: never read by the reducer
  const int64_t a = SQ ? 0 : selected[round - 1];
  const int64_t c = cb + 2 * threadIdx.x;
  if (c >= cend) return;
  const bool two = c + 1 < cend;
  double s[1], t[1];
  trmv_rows<SQ, 1, 1, false>(M, n, lda, c, max(max(r0, a), c), r1, xcol, vec, s, t);
  if (c >= cbeg) part[blockIdx.y * n + c] = s[0];
  if (two) part[blockIdx.y * n + c + 1] = t[0];
}

// Indices that come from the caller arrive validated by the host (range, duplicates); the clamp
// only keeps a corrupt value from addressing outside the matrix.
__device__ __forceinline__ int64_t forced_index(const int64_t* forced, int64_t j, int64_t n) {
  return min(max(forced[j], (int64_t)0), n - 1);
}

// greedy_trmv_kernel<false> for the up to T columns of a speculative pass (header words H_COL:
// the pick first, n for an unused entry), right-hand sides row-interleaved in X.  Column j's
// partials are bit for bit what the classic kernel writes for a = col[j]: its origin in row chunk
// [r0, r1) is max(r0, col[j], c), which depends on col[j] only in the chunk that holds it.  Every
// chunk runs the T-wide loop once with the shared origin max(r0, c) (r0, uniform, with scalar x
// below the diagonal tile); that is the result of every column above the chunk (X is zero above
// col[j]; a column's chunks above its own are never read by the reducers and not written).  A
// column whose col[j] lies inside the chunk then runs the single-column loop with its own origin:
// one partial re-read of a 512-row band per column and pass.  Nothing runs on a hit.  Slice 0
// is `part0` (the classic partials), slice j > 0 is spart[j - 1].
template <int T>
__global__ __launch_bounds__(CT) void greedy_trmv_spec_kernel(
    const double* __restrict__ M, int64_t n, int64_t lda, const long long* __restrict__ h,
    const double* __restrict__ X, double* __restrict__ part0, double* __restrict__ spart,
    int vec) {
  const int64_t cb = (int64_t)blockIdx.x * TRMV_COLS;
  const int64_t r0 = (int64_t)blockIdx.y * RC;
  const int64_t r1 = min(r0 + RC, n);
  if (cb >= r1) return;  // tile strictly above the diagonal: never read by the reducers
  if (h[H_HIT]) return;
  int64_t col[T], amin = n;
  bool own = false;  // some col[j] lies in this row chunk
#pragma unroll
  for (int j = 0; j < T; ++j) {
    col[j] = h[H_COL + j];
    amin = min(amin, col[j]);
    own = own || (col[j] >= r0 && col[j] < r1);
  }
  if (amin >= r1) return;  // rows above every column: no reducer starts here
  const int64_t c = cb + 2 * threadIdx.x;
  if (c >= n) return;
  const bool two = c + 1 < n;
  const bool below = blockIdx.x < blockIdx.y;  // every column of the tile is left of row r0
  const int64_t slice = ((n + RC - 1) / RC) * n;
  auto out = [&](int j) {
    return (j == 0 ? part0 : spart + (int64_t)(j - 1) * slice) + blockIdx.y * n + c;
  };
  {
    double s[T], t[T];
    if (below)
      trmv_rows<false, T, T, true>(M, n, lda, c, r0, r1, X, vec, s, t);
    else
      trmv_rows<false, T, T, false>(M, n, lda, c, max(r0, c), r1, X, vec, s, t);
#pragma unroll
    for (int j = 0; j < T; ++j) {
      if (col[j] < r0) {
        double* o = out(j);
        o[0] = s[j];
        if (two) o[1] = t[j];
      }
    }
  }
  if (own) {
#pragma unroll 1
    for (int j = 0; j < T; ++j) {
      const int64_t aj = h[H_COL + j];
      if (aj < r0 || aj >= r1) continue;
      double s[1], t[1];
      if (below)
        trmv_rows<false, 1, T, true>(M, n, lda, c, aj, r1, X + j, vec, s, t);
      else
        trmv_rows<false, 1, T, false>(M, n, lda, c, max(aj, c), r1, X + j, vec, s, t);
      double* o = out(j);
      o[0] = s[0];
      if (two) o[1] = t[0];
    }
  }
}

// One workgroup decides a round of vgposp_greedy_step with speculation, on the device: a =
// selected[round - 1] is looked up among the cached columns.  Hit: the slot is recorded and every
// later kernel of the pass returns at once.  Miss: the pass list is a, then up to width - 1
// columns that are unselected, unmasked and not yet cached, the largest fresh deltas of the
// previous round first (exact top-(width-1): one strided scan of delta per column, n / 1024
// loads a thread, against a pass over the triangle of L^-1); each gets the next free slot, and a
// full table only ends the list — nothing is evicted, so nothing a round computes depends on the
// table's history.
__global__ __launch_bounds__(CH) void greedy_spec_plan_kernel(int64_t n, int round, int width,
                                                              int64_t slots,
                                                              const int64_t* selected,
                                                              GreedyWS w) {
  __shared__ long long hit_slot;
  long long* h = w.spec;
  long long* tcol = h + SPEC_HDR;
  long long* tround = tcol + slots;
  // (clamped: selected[] holds -1 once no candidate was left, and nothing here may index with it)
  const long long a = min(max(selected[round - 1], (int64_t)0), n - 1);
  long long cnt = h[H_COUNT];
  if (threadIdx.x == 0) hit_slot = -1;
  __syncthreads();
  if (w.cmask[a])
    for (long long e = threadIdx.x; e < cnt; e += blockDim.x)
      if (tcol[e] == a) hit_slot = e;
  __syncthreads();
  if (hit_slot >= 0) {
    if (threadIdx.x == 0) {
      h[H_HIT] = 1;
      h[H_SLOT] = hit_slot;
      h[H_NB] = 0;
      h[H_HITS] += 1;
    }
    return;
  }
  int nb = 1;
  for (int t = 1; t < width && cnt < slots; ++t) {
    double bv = -DBL_MAX;
    long long bi = -1;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
      if (w.selmask[i] || w.cmask[i]) continue;
      const double d = w.delta[i];
      if (key_gt(d, i, bv, bi)) {
        bv = d;
        bi = i;
      }
    }
    block_keymax(bv, bi);
    if (bi < 0) break;  // no candidate left (uniform)
    if (threadIdx.x == 0) {
      w.cmask[bi] = 1;
      tcol[cnt] = bi;
      tround[cnt] = round;
      h[H_COL + nb] = bi;
      h[H_CSLOT + nb] = cnt;
    }
    ++nb;
    ++cnt;
    __syncthreads();  // the next scan sees cmask[bi]
  }
  if (threadIdx.x == 0) {
    h[H_HIT] = 0;
    h[H_SLOT] = -1;
    h[H_NB] = nb;
    h[H_COL] = a;
    h[H_CSLOT] = -1;
    for (int j = nb; j < SPEC_TMAX; ++j) {
      h[H_COL + j] = n;  // unused: above every row
      h[H_CSLOT + j] = -1;
    }
    h[H_COUNT] = cnt;
    h[H_PASSES] += 1;
  }
}

// The right-hand sides of a multi-column pass, row-interleaved so that the mat-vec reads the T
// values of a row with one uniform load: X[r][j] = (M e_{col[j]})_r for r >= col[j], else 0.
// col[j] = cols[j] for j < nt and n (unused: all zero) beyond.  The speculation passes the header
// words H_COL, where greedy_spec_plan_kernel marks its own unused entries with n, and H_HIT as
// `skip` (nothing runs when it is set); the conditioning passes placed + j0 with clamp = 1.
template <int T>
__global__ void greedy_extract_cols_kernel(const double* M, int64_t n, int64_t lda,
                                           const long long* cols, int nt, int clamp,
                                           const long long* skip, double* X) {
  if (skip && *skip) return;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * T) return;
  const int64_t r = e / T;
  const int j = (int)(e % T);
  int64_t a = n;
  if (j < nt) a = clamp ? forced_index(reinterpret_cast<const int64_t*>(cols), j, n) : cols[j];
  X[e] = (a < n && r >= a) ? M[r * lda + a] : 0.0;
}

// q_c[i] of the speculated columns j >= 1 of a pass into their slots, in exactly the order of
// greedy_update_kernel: q = 0; for rc = max(i, c) / RC .. nrc-1: q += part[rc][i].
__global__ __launch_bounds__(CH) void greedy_spec_reduce_kernel(int64_t n, GreedyWS w) {
  const long long* h = w.spec;
  if (h[H_HIT]) return;
  const int j = (int)blockIdx.y + 1;
  if (j >= h[H_NB]) return;
  const int64_t i = (int64_t)blockIdx.x * CH + threadIdx.x;
  if (i >= n) return;
  const int64_t c = h[H_COL + j], slot = h[H_CSLOT + j];
  const int64_t nrc = (n + RC - 1) / RC;
  const double* sp = w.spart + (int64_t)(j - 1) * nrc * n;
  double q = 0.0;
  for (int64_t rc = max(i, c) / RC; rc < nrc; ++rc) q += sp[rc * n + i];
  w.qc[slot * n + i] = q;
}

// Round 0: nom = diag(Sigma), prec = Q_ii.  Round t>0: rank-1 updates with a = selected[t-1].
// spec: a round of vgposp_greedy_step with speculation, whose q comes from the cache on a hit.
// Then delta for every unselected candidate and per-workgroup best fresh key.
__global__ __launch_bounds__(CH) void greedy_update_kernel(const double* S, int64_t n, int64_t lda,
                                                           const int64_t* selected, int round,
                                                           GreedyWS w, int64_t cbeg, int64_t cend,
                                                           int spec) {
  const int64_t i = (cbeg / CH + (int64_t)blockIdx.x) * CH + threadIdx.x;
  const double eps = w.prm[0], thr = w.prm[1];
  if (i >= cbeg && i < cend) {
    const int64_t nrc = (n + RC - 1) / RC;
    double q = 0.0;
    if (round == 0) {
      for (int64_t rc = i / RC; rc < nrc; ++rc) q += w.part[rc * n + i];
      w.prec[i] = q;
      w.nom[i] = w.sdiag[i];
    } else {
      const int64_t a = selected[round - 1];
      const int t1 = round - 1;  // new row index in W / V
      if (spec && w.spec[H_HIT])  // q_a was formed by an earlier pass, in this same order
        q = w.qc[w.spec[H_SLOT] * n + i];
      else
        for (int64_t rc = max(i, a) / RC; rc < nrc; ++rc) q += w.part[rc * n + i];
      double s = (i < a) ? S[i * lda + a] : (i > a ? S[a * lda + i] : w.sdiag[a]);
      for (int t = 0; t < t1; ++t) {
        s -= w.piv[2 + t] * w.W[(int64_t)t * n + i];
        q -= w.piv[2 + t1 + t] * w.V[(int64_t)t * n + i];
      }
      // pivot of the Cholesky of Sigma_AA + eps I: nom_a + eps
      const double noma = w.piv[0] + eps, preca = w.piv[1];
      const double wy = noma > 0.0 ? s / sqrt(noma) : 0.0;
      const double vy = preca > 0.0 ? q / sqrt(preca) : 0.0;
      w.W[(int64_t)t1 * n + i] = wy;
      w.V[(int64_t)t1 * n + i] = vy;
      w.nom[i] -= wy * wy;
      w.prec[i] -= vy * vy;
    }
    if (!w.selmask[i]) w.delta[i] = delta_of(w.nom[i], w.prec[i], eps, thr);
  }
}

// Best fresh key F* per workgroup over all candidates (delta is complete on every rank here).
__global__ __launch_bounds__(CH) void greedy_fresh_max_kernel(int64_t n, GreedyWS w) {
  const int64_t i = (int64_t)blockIdx.x * CH + threadIdx.x;
  double bv = -DBL_MAX;
  long long bi = -1;
  if (i < n && !w.selmask[i]) {
    bv = w.delta[i];
    bi = i;
  }
  block_keymax(bv, bi);
  if (threadIdx.x == 0) {
    w.fval[blockIdx.x] = bv;
    w.fidx[blockIdx.x] = bi;
  }
}

// Reduce the nf per-workgroup keys in `val/idx` (all threads get the result).
__device__ __forceinline__ void reduce_keys(const double* val, const long long* idx, int64_t nf,
                                            double& v, long long& i) {
  v = -DBL_MAX;
  i = -1;
  for (int64_t e = threadIdx.x; e < nf; e += blockDim.x) {
    // idx < 0: a chunk with no candidate left (wave_keymax returns (0.0, -1) for it); it must not
    // enter the comparison, or its 0.0 would shut out a real candidate with a value <= 0
    if (idx[e] >= 0 && key_gt(val[e], idx[e], v, i)) {
      v = val[e];
      i = idx[e];
    }
  }
  block_keymax(v, i);
}

// Bulk refresh: stale entries with key > best fresh key F* are re-scored (guaranteed by the
// reference's loop before it can stop), then per-chunk maxima of the cache.
__global__ __launch_bounds__(CH) void greedy_refresh_kernel(int64_t n, GreedyWS w) {
  const int64_t nch = (n + CH - 1) / CH;
  double fv;
  long long fi;
  reduce_keys(w.fval, w.fidx, nch, fv, fi);
  const int64_t i = (int64_t)blockIdx.x * CH + threadIdx.x;
  double bv = -DBL_MAX;
  long long bi = -1;
  int refreshed = 0;
  if (i < n && !w.selmask[i]) {
    double c = w.cache[i];
    if (key_gt(c, i, fv, fi)) {
      c = w.delta[i];
      w.cache[i] = c;
      w.fresh[i] = 1;
      refreshed = 1;
    } else {
      w.fresh[i] = 0;
    }
    bv = c;
    bi = i;
  }
  // count refreshes (one atomic per wave)
  unsigned long long ball = __ballot(refreshed);
  if ((threadIdx.x & 63) == 0 && ball) atomicAdd((unsigned long long*)&w.cnt[0], (unsigned long long)__popcll(ball));
  block_keymax(bv, bi);
  if (threadIdx.x == 0) {
    w.cval[blockIdx.x] = bv;
    w.cidx[blockIdx.x] = bi;
  }
}

// ---- placement algorithm 3 (snippets_a3.py:43-330): the cache is refreshed only inside the
// index-space window around the last pick; entries outside keep their stale values. ----

// Round 0 (snippets_a3.py:67-119): every candidate is scored once, cache = delta.
__global__ __launch_bounds__(CH) void greedy_cache_all_kernel(int64_t n, GreedyWS w) {
  const int64_t i = (int64_t)blockIdx.x * CH + threadIdx.x;
  if (i < n) w.cache[i] = w.selmask[i] ? 0.0 : w.delta[i];
  if (i == 0) w.cnt[0] = n;
}

// Rounds >= 1 (:196-318): for (j0, j1, j2) in [i - cutoff, i + cutoff) clipped to the grid
// (upper bound exclusive, as the reference's while loops), cache[yj] = delta[yj] or 0 for yj in A;
// cache[y*] = 0.  cnt[0] = number of window entries (the reference's body_D calls).
__global__ __launch_bounds__(256) void greedy_window_kernel(const int64_t* selected, int round,
                                                            int64_t I0, int64_t I1, int64_t I2,
                                                            int cutoff, GreedyWS w) {
  const int64_t a = selected[round - 1];
  const int64_t s0 = I1 * I2;
  const int64_t i0 = a / s0, i1 = (a - i0 * s0) / I2, i2 = a - i0 * s0 - i1 * I2;
  const int64_t lo0 = max(i0 - cutoff, (int64_t)0), hi0 = min(i0 + cutoff, I0);
  const int64_t lo1 = max(i1 - cutoff, (int64_t)0), hi1 = min(i1 + cutoff, I1);
  const int64_t lo2 = max(i2 - cutoff, (int64_t)0), hi2 = min(i2 + cutoff, I2);
  const int64_t W0 = max(hi0 - lo0, (int64_t)0), W1 = max(hi1 - lo1, (int64_t)0),
                W2 = max(hi2 - lo2, (int64_t)0);
  const int64_t total = W0 * W1 * W2;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j0 = lo0 + t / (W1 * W2), r = t % (W1 * W2);
    const int64_t j1 = lo1 + r / W2, j2 = lo2 + r % W2;
    const int64_t yj = j0 * s0 + j1 * I2 + j2;
    w.cache[yj] = w.selmask[yj] ? 0.0 : w.delta[yj];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    w.cache[a] = 0.0;
    w.cnt[0] = total;
  }
}

// Per-chunk maxima of the cache over unselected candidates (sparse_argmax_cache_linear, :24-50).
__global__ __launch_bounds__(CH) void greedy_cache_max_kernel(int64_t n, GreedyWS w) {
  const int64_t i = (int64_t)blockIdx.x * CH + threadIdx.x;
  double bv = -DBL_MAX;
  long long bi = -1;
  if (i < n && !w.selmask[i]) {
    bv = w.cache[i];
    bi = i;
  }
  block_keymax(bv, bi);
  if (threadIdx.x == 0) {
    w.fval[blockIdx.x] = bv;
    w.fidx[blockIdx.x] = bi;
  }
}

// One workgroup: the remaining re-score loop of placement_algorithm2.py:183-208, then selection.
// mode: 0 = full greedy (placement_algorithm_1), 1 = lazy (placement_algorithm_2),
//       2 = window (placement algorithm 3: arg-max of the cache maxima in fval / fidx).
__global__ __launch_bounds__(CH) void greedy_select_kernel(int64_t n, int round, int mode,
                                                           int64_t* selected, double* sel_delta,
                                                           int64_t* evals, GreedyWS w,
                                                           int64_t cbeg, int64_t cend) {
  __shared__ double cv[MAXCH];
  __shared__ long long ci[MAXCH];
  __shared__ long long ychosen;
  const int64_t nch = (n + CH - 1) / CH;
  double v;
  long long y = -1;
  long long loop_evals = 0;
  const bool lazy = mode == 1;
  if (!lazy) {
    reduce_keys(w.fval, w.fidx, nch, v, y);
  } else {
    for (int64_t c = threadIdx.x; c < nch; c += blockDim.x) {
      cv[c] = w.cval[c];
      ci[c] = w.cidx[c];
    }
    __syncthreads();
    for (int64_t it = 0; it <= n; ++it) {
      reduce_keys(cv, ci, nch, v, y);
      if (y < 0) break;
      if (w.fresh[y]) break;  // arg-max is up to date -> select (:187-189)
      // re-score y (:193-208) and recompute its chunk maximum
      const double dy = w.delta[y];
      __syncthreads();
      if (threadIdx.x == 0) {
        w.cache[y] = dy;
        w.fresh[y] = 1;
      }
      ++loop_evals;
      __syncthreads();
      const int64_t c = y / CH;
      const int64_t j = c * CH + threadIdx.x;
      double bv = -DBL_MAX;
      long long bi = -1;
      if (j < n && !w.selmask[j]) {
        bv = (j == y) ? dy : w.cache[j];
        bi = j;
      }
      block_keymax(bv, bi);
      if (threadIdx.x == 0) {
        cv[c] = bv;
        ci[c] = bi;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) ychosen = y;
  __syncthreads();
  y = ychosen;
  if (y < 0) {
    if (threadIdx.x == 0) {
      selected[round] = -1;
      if (sel_delta) sel_delta[round] = 0.0;
    }
    return;
  }
  // pivot data for the next update: nom_y, P_yy, W[0..round)[y], V[0..round)[y].  Only the rank
  // owning y's candidate slab holds them; the others write zeros (summed across ranks).
  const bool own = y >= cbeg && y < cend;
  if (threadIdx.x == 0) {
    selected[round] = y;
    if (sel_delta) sel_delta[round] = mode == 2 ? w.cache[y] : w.delta[y];
    if (evals) evals[round] = mode != 0 ? w.cnt[0] + loop_evals : n - round;
    w.cnt[0] = 0;
    w.selmask[y] = 1;
    w.piv[0] = own ? w.nom[y] : 0.0;
    w.piv[1] = own ? w.prec[y] : 0.0;
  }
  for (int t = threadIdx.x; t < round; t += blockDim.x) {
    w.piv[2 + t] = own ? w.W[(int64_t)t * n + y] : 0.0;
    w.piv[2 + round + t] = own ? w.V[(int64_t)t * n + y] : 0.0;
  }
}

// The odd-order padding candidate (GreedyPlacement pad_odd) is never an arg-max.
__global__ void greedy_exclude_kernel(unsigned char* selmask, int64_t idx) { selmask[idx] = 1; }

// ---- candidate set S != V and pre-installed sensors A0 (Krause's S / U split, which
// placement_algorithm2.py:128-160 assumes away: "assume U is empty, assume V = S", A = []) ----

// selmask[i] |= !allowed[i]: a masked location is never an arg-max, but greedy_update_kernel keeps
// updating its nom / prec, so it stays in A_bar (denominator, :408-413) like every unselected one.
__global__ void greedy_mask_kernel(int64_t n, const unsigned char* allowed,
                                   unsigned char* selmask) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && !allowed[i]) selmask[i] = 1;
}

// The tail of greedy_select_kernel for a pick given by the caller: y = forced[j] instead of the
// arg-max (A.append(y), :211).  Cache, fresh flags and evaluation counts are not touched.
__global__ __launch_bounds__(256) void greedy_force_kernel(int64_t n, int round,
                                                           const int64_t* forced, int64_t j,
                                                           int64_t* selected, GreedyWS w) {
  const int64_t y = forced_index(forced, j, n);
  if (threadIdx.x == 0) {
    selected[round] = y;
    w.selmask[y] = 1;
    w.piv[0] = w.nom[y];
    w.piv[1] = w.prec[y];
  }
  for (int t = threadIdx.x; t < round; t += blockDim.x) {
    w.piv[2 + t] = w.W[(int64_t)t * n + y];
    w.piv[2 + round + t] = w.V[(int64_t)t * n + y];
  }
}

// greedy_trmv_kernel<false> for T right-hand sides in one pass over M = L^-1:
//   part[j][rc][c] = sum_{r in chunk rc, r >= max(c, a_j)} M[r][c] * X[r][j]
// Same tiling and the same 16-byte non-temporal column-pair loads; rows start at
// max(c, min_j a_j) (X[.][j] is zero above a_j).  The row index is uniform over the workgroup, so
// the T values of X for a row are wave-uniform operands; the diagonal tile (RC == TRMV_COLS, all
// columns) masks the entries above the diagonal, which hold Sigma.
// Its own row loop, not trmv_rows, and so equal to the classic kernel to rounding only: two
// accumulators per column and right-hand side where trmv_rows' fixed order needs four, and a
// uniform row index in the diagonal tile too.  Conditioning through greedy_trmv_spec_kernel's
// pass was measured and is slower (profiles/cond_unified_ab.json; batch 8, 256 sensors): by
// 18 % at N = 65,536 and 2.4 x at 16,384 with its own-origin loops, by 12 % and 42 % without.
static_assert(RC == TRMV_COLS, "the batched mat-vec takes tile (b, b) as the diagonal tile");

template <int T, bool VEC>
__global__ __launch_bounds__(CT) void greedy_trmv_batch_kernel(
    const double* __restrict__ M, int64_t n, int64_t lda, const int64_t* __restrict__ forced,
    int64_t j0, int nt, const double* __restrict__ X, double* __restrict__ part) {
  typedef double d2v __attribute__((ext_vector_type(2)));
  const int64_t cb = (int64_t)blockIdx.x * TRMV_COLS;
  const int64_t r0 = (int64_t)blockIdx.y * RC;
  const int64_t r1 = min(r0 + RC, n);
  if (cb >= r1) return;  // tile strictly above the diagonal: never read by the reducer
  int64_t amin = n;
  for (int j = 0; j < nt; ++j) amin = min(amin, forced_index(forced, j0 + j, n));
  if (amin >= r1) return;  // rows above every a_j: the reducer starts at chunk a_j / RC
  const bool diag = blockIdx.x == blockIdx.y;
  const int64_t c = cb + 2 * threadIdx.x;
  if (c >= n) return;
  const bool two = c + 1 < n;
  double acc0[T], acc1[T];  // column c, column c + 1
#pragma unroll
  for (int j = 0; j < T; ++j) acc0[j] = acc1[j] = 0.0;
  auto load = [&](const double* p) -> d2v {
    if (VEC && two) return __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p));
    d2v m;
    m.x = __builtin_nontemporal_load(p);
    m.y = two ? __builtin_nontemporal_load(p + 1) : 0.0;
    return m;
  };
  auto row = [&](d2v m, int64_t r) {
    if (diag) {  // lower triangle only: (r, c) needs r >= c, (r, c + 1) needs r > c
      m.x = r >= c ? m.x : 0.0;
      m.y = r > c ? m.y : 0.0;
    }
    const double* x = X + r * T;
#pragma unroll
    for (int j = 0; j < T; ++j) {
      acc0[j] = fma(m.x, x[j], acc0[j]);
      acc1[j] = fma(m.y, x[j], acc1[j]);
    }
  };
  int64_t r = max(max(r0, cb), amin);
  const double* p = M + r * lda + c;
  for (; r + 3 < r1; r += 4, p += 4 * lda) {
    const d2v m0 = load(p), m1 = load(p + lda), m2 = load(p + 2 * lda), m3 = load(p + 3 * lda);
    row(m0, r);
    row(m1, r + 1);
    row(m2, r + 2);
    row(m3, r + 3);
  }
  for (; r < r1; ++r, p += lda) row(load(p), r);
  const int64_t nrc = (n + RC - 1) / RC;
#pragma unroll
  for (int j = 0; j < T; ++j) {
    if (j < nt) {
      double* o = part + ((int64_t)j * nrc + blockIdx.y) * n + c;
      o[0] = acc0[j];
      if (two) o[1] = acc1[j];
    }
  }
}

// ---- host side: the argument checks.  A checker takes the entry's name `fn` and the position of
// its group in THAT entry: a message is always "<entry>: bad argument <the entry's own position>".
// The checker an entry starts with clears the last error. ----
// (n, kmax) at `at`, `at` + 1
static int check_sizes(const char* fn, int at, int64_t n, int kmax) {
  clear_error();
  VG_ARG(n >= 1 && n <= (int64_t)MAXCH * CH, at);
  VG_ARG(kmax >= 1 && kmax <= n, at + 1);
  return 0;
}
// (Sigma, n, lda, kmax): arguments 1 to 4 of every entry that has a matrix
static int check_matrix(const char* fn, const double* Sigma, int64_t n, int64_t lda, int kmax) {
  clear_error();
  VG_ARG(Sigma != nullptr, 1);
  VG_ARG(n >= 1 && n <= (int64_t)MAXCH * CH, 2);
  VG_ARG(lda >= n, 3);
  VG_ARG(kmax >= 1 && kmax <= n, 4);
  return 0;
}
// (c0, c1, tmp, tmp_bytes): a slab of the partitioned inverse, 128-aligned or ending at n
static int check_slab(const char* fn, int at, int64_t n, int64_t c0, int64_t c1, const double* tmp,
                      size_t tmp_bytes) {
  VG_ARG(c0 >= 0 && c0 <= c1 && c0 % 128 == 0, at);
  VG_ARG(c1 <= n && (c1 % 128 == 0 || c1 == n), at + 1);
  VG_ARG(c1 == c0 || (tmp != nullptr && tmp_bytes >= partial_inverse_tmp_bytes(n, c0, c1)),
         at + 2);
  return 0;
}
// (jitter, threshold, cache_init) at 5 to 7 everywhere; a null info by position or by name
static int check_init(const char* fn, double jitter, double threshold, double cache_init,
                      int at_info, const int* info, bool by_name) {
  VG_ARG(jitter >= 0.0 && jitter < 1e300, 5);
  VG_ARG(threshold >= 0.0, 6);
  VG_ARG(cache_init == cache_init, 7);
  if (!by_name) VG_ARG(info != nullptr, at_info);
  if (info == nullptr) set_error("%s: info is null", fn);
  return info == nullptr ? -at_info : 0;
}
// (ws, ws_bytes): a null ws is argument `at`, or with at = 0 "workspace is null" and VGPOSP_E_WS
static int check_ws(const char* fn, int at, const void* ws, size_t ws_bytes, size_t need) {
  if (at) VG_ARG(ws != nullptr, at);
  if (ws == nullptr) set_error("%s: workspace is null", fn);
  else if (ws_bytes < need) set_error("%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
  return ws != nullptr && ws_bytes >= need ? 0 : VGPOSP_E_WS;
}
// (ws, n, kmax) of the entries that only look into a workspace
static int check_view(const char* fn, const void* ws, int64_t n, int kmax) {
  clear_error();
  VG_ARG(ws != nullptr, 1);
  VG_ARG(n >= 1, 2);
  VG_ARG(kmax >= 1, 3);
  return 0;
}

// Grid of a mat-vec kernel over columns [c0, c1) (the tile origin is even: column pairs), and
// whether it may load a column pair with one 16-byte access.
static dim3 trmv_grid(int64_t n, int64_t c0, int64_t c1) {
  return dim3((unsigned)ceil_div(c1 - (c0 & ~(int64_t)1), TRMV_COLS), (unsigned)ceil_div(n, RC));
}
static int trmv_vec(const double* M, int64_t lda) {
  return (reinterpret_cast<uintptr_t>(M) % 16 == 0) && (lda % 2 == 0);
}

// `info` cleared and the init kernel (vgposp_greedy_prepare)
static int run_prepare(const char* fn, double* Sigma, int64_t n, int64_t lda, double jitter,
                       double threshold, double cache_init, int* info, const GreedyWS& w,
                       hipStream_t s) {
  VG_HIP_AS(fn, vg_memset(info, 0, sizeof(int), s));
  hipLaunchKernelGGL(greedy_init_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, Sigma,
                     n, lda, jitter, threshold, cache_init, w);
  VG_HIP_AS(fn, hipGetLastError());
  return 0;
}

// Q_ii = |M e_i|^2 for columns [c0, c1) -> part (reduced in the round-0 update)
static void launch_colsq(const double* M, int64_t n, int64_t lda, int64_t c0, int64_t c1,
                         const GreedyWS& w, hipStream_t s) {
  const bool whole = c0 == 0 && c1 == n;  // a slab reports no algorithmic figures
  const double tri = 0.5 * (double)n * (n + 1);
  ProfScope ps("greedy_colsq", s, whole ? 2.0 * tri : 0.0,
               whole ? 8.0 * (tri + (double)ceil_div(n, RC) * n) : 0.0);
  hipLaunchKernelGGL(greedy_trmv_kernel<true>, trmv_grid(n, c0, c1), dim3(CT), 0, s, M, n, lda,
                     nullptr, 0, nullptr, w.part, c0, c1, trmv_vec(M, lda));
}

// L^-1 in columns [c0, c1) of a factored Sigma and their column norms (vgposp_greedy_finish_slab)
static int run_finish_slab(const char* fn, double* Sigma, int64_t n, int64_t lda, int kmax,
                           int64_t c0, int64_t c1, double* tmp, void* ws, const GreedyWS& w,
                           hipStream_t s) {
  if (c1 == c0) return 0;
  // M changes here: no cached column survives (header, table and the "is cached" bytes)
  VG_HIP_AS(fn, vg_memset(w.spec, 0, (size_t)(SPEC_HDR + 2 * spec_slots(kmax)) * 8 + n, s));
  VG_TRY(partial_inverse(Sigma, n, lda, c0, c1, tmp, greedy_fact_ws(ws, w, n), s));
  launch_colsq(Sigma, n, lda, c0, c1, w, s);
  VG_HIP_AS(fn, hipGetLastError());
  return 0;
}

// xcol = the last pick's column of L^-1 where [own0, own1) holds it, zeros elsewhere
static void launch_extract(const double* Sigma, int64_t n, int64_t lda, const int64_t* selected,
                           int round, const GreedyWS& w, int64_t own0, int64_t own1,
                           hipStream_t s) {
  hipLaunchKernelGGL(greedy_extract_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s,
                     Sigma, n, lda, selected, round, w.xcol, own0, own1);
}

// q = M^T xcol in columns [c0, c1) -> part
static void launch_trmv(const double* Sigma, int64_t n, int64_t lda, const int64_t* selected,
                        int round, const GreedyWS& w, int64_t c0, int64_t c1, hipStream_t s) {
  // algorithmic: the lower triangle of L^-1 in rows >= a, columns [c0, c1) (a is device-side;
  // bench.py recomputes the exact bytes from the selections)
  ProfScope ps("greedy_trmv", s, 0.0, 8.0 * (0.5 * (double)n * (n + 1) + 2.0 * n));
  hipLaunchKernelGGL(greedy_trmv_kernel<false>, trmv_grid(n, c0, c1), dim3(CT), 0, s, Sigma, n,
                     lda, selected, round, w.xcol, w.part, c0, c1, trmv_vec(Sigma, lda));
}

// Rank-1 rows, nom, P_yy and fresh deltas of columns [c0, c1) from the partials `part` (spec: the
// plan says where the pick's column is); the CH-aligned blocks spanning [c0, c1), from c0 / CH on
static void launch_update(const double* Sigma, int64_t n, int64_t lda, const int64_t* selected,
                          int round, GreedyWS w, int64_t c0, int64_t c1, double* part, int spec,
                          hipStream_t s) {
  w.part = part;
  ProfScope ps("greedy_update", s, 0.0, 8.0 * (double)(c1 - c0) * (6 + 2.0 * round));
  hipLaunchKernelGGL(greedy_update_kernel, dim3((unsigned)(ceil_div(c1, CH) - c0 / CH)), dim3(CH),
                     0, s, Sigma, n, lda, selected, round, w, c0, c1, spec);
}

// The arg-max of a round.  mode 0: full greedy, 1: lazy (the stale entries above the best fresh
// key are refreshed first), 2: over the cache (algorithm 3).
static void launch_select(int64_t n, int round, int mode, int64_t* selected, double* sel_delta,
                          int64_t* evals, const GreedyWS& w, int64_t c0, int64_t c1,
                          hipStream_t s) {
  const unsigned nch = (unsigned)ceil_div(n, CH);
  hipLaunchKernelGGL(mode == 2 ? greedy_cache_max_kernel : greedy_fresh_max_kernel, dim3(nch),
                     dim3(CH), 0, s, n, w);
  if (mode == 1) {
    ProfScope psr("greedy_refresh", s, 0.0, 8.0 * 3.0 * n);
    hipLaunchKernelGGL(greedy_refresh_kernel, dim3(nch), dim3(CH), 0, s, n, w);
  }
  ProfScope pss("greedy_select", s, 0.0, 0.0);
  hipLaunchKernelGGL(greedy_select_kernel, dim3(1), dim3(CH), 0, s, n, round, mode, selected,
                     sel_delta, evals, w, c0, c1);
}

// f(T), T = width (2, 4 or 8) at compile time; LO: the smallest built (a dead 2 then names LO)
template <int LO, class F>
static void with_width(int width, F&& f) {
  if (LO <= 2 && width == 2) return f(std::integral_constant<int, std::max(LO, 2)>{});
  if (width == 4) return f(std::integral_constant<int, 4>{});
  f(std::integral_constant<int, 8>{});
}

// The mat-vec part of a speculative round: plan, the T right-hand sides, one pass (or none), the
// speculated columns into their slots.  A fixed launch sequence, hit or miss.
template <int T>
static void launch_spec_pass(const double* Sigma, int64_t n, int64_t lda, int kmax, int round,
                             const int64_t* selected, const GreedyWS& w, hipStream_t s) {
  hipLaunchKernelGGL(greedy_spec_plan_kernel, dim3(1), dim3(CH), 0, s, n, round, T,
                     spec_slots(kmax), selected, w);
  hipLaunchKernelGGL(greedy_extract_cols_kernel<T>, dim3((unsigned)ceil_div(n * T, 256)),
                     dim3(256), 0, s, Sigma, n, lda, w.spec + H_COL, T, 0, w.spec + H_HIT, w.X);
  {
    ProfScope ps("greedy_trmv_spec", s, 0.0, 8.0 * (0.5 * (double)n * (n + 1) + (double)T * n));
    hipLaunchKernelGGL(greedy_trmv_spec_kernel<T>, trmv_grid(n, 0, n), dim3(CT), 0, s, Sigma, n,
                       lda, w.spec, w.X, w.part, w.spart, trmv_vec(Sigma, lda));
  }
  hipLaunchKernelGGL(greedy_spec_reduce_kernel, dim3((unsigned)ceil_div(n, CH), T - 1), dim3(CH),
                     0, s, n, w);
}

struct CondScratch {
  double *X, *part;
  size_t bytes;
};

static CondScratch cond_layout(void* base, int64_t n, int batch) {
  CondScratch c{};
  char* p = static_cast<char*>(base);
  const size_t xb = align_up((size_t)n * batch * 8);
  c.X = (double*)p;
  c.part = (double*)(p ? p + xb : nullptr);
  c.bytes = xb + align_up((size_t)batch * ceil_div(n, RC) * n * 8);
  return c;
}
static bool cond_batch_ok(int batch) { return batch == 1 || batch == 4 || batch == 8; }
// The columns q of placed[j0 .. j0 + nt) in one pass over L^-1 -> c.part, a slice per column
template <int T>
static void launch_cond_batch(const double* Sigma, int64_t n, int64_t lda, const int64_t* forced,
                              int64_t j0, int nt, const CondScratch& c, hipStream_t s) {
  hipLaunchKernelGGL(greedy_extract_cols_kernel<T>, dim3((unsigned)ceil_div(n * T, 256)),
                     dim3(256), 0, s, Sigma, n, lda,
                     reinterpret_cast<const long long*>(forced + j0), nt, 1, nullptr, c.X);
  ProfScope ps("greedy_trmv_batch", s, 2.0 * T * 0.5 * (double)n * (n + 1),
               8.0 * (0.5 * (double)n * (n + 1) + (double)T * n));
  if (trmv_vec(Sigma, lda))
    hipLaunchKernelGGL((greedy_trmv_batch_kernel<T, true>), trmv_grid(n, 0, n), dim3(CT), 0, s,
                       Sigma, n, lda, forced, j0, nt, c.X, c.part);
  else
    hipLaunchKernelGGL((greedy_trmv_batch_kernel<T, false>), trmv_grid(n, 0, n), dim3(CT), 0, s,
                       Sigma, n, lda, forced, j0, nt, c.X, c.part);
}

// vgposp_greedy_init (info, ws at 5, 6; the variant parameters are constants) and _init_ex (8, 9)
static int init_entry(const char* fn, int at_info, double* Sigma, int64_t n, int64_t lda, int kmax,
                      double jitter, double threshold, double cache_init, int* info, void* ws,
                      size_t ws_bytes, void* stream) {
  VG_TRY(check_matrix(fn, Sigma, n, lda, kmax));
  VG_TRY(check_init(fn, jitter, threshold, cache_init, at_info, info, false));
  const GreedyWS w = greedy_layout(ws, n, kmax);
  VG_TRY(check_ws(fn, at_info + 1, ws, ws_bytes, w.bytes));
  hipStream_t s = as_stream(stream);
  VG_TRY(run_prepare(fn, Sigma, n, lda, jitter, threshold, cache_init, info, w, s));
  // early: after a failed pivot (a singular cov_vv) every later launch of the factorization and
  // inverse reads `info` on the device and exits, so the host's jitter retry does not pay for a
  // whole O(n^3) factorization + inverse first — and nothing here synchronises the host
  VG_TRY(potrf_one(Sigma, n, lda, /*invert=*/1, nullptr, info, greedy_fact_ws(ws, w, n), s,
                   /*early=*/true));
  launch_colsq(Sigma, n, lda, 0, n, w, s);
  VG_HIP_AS(fn, hipGetLastError());
  return 0;
}

// vgposp_greedy_update (extract = 1) and _update_ex: the same positions up to `selected`
static int update_entry(const char* fn, const double* Sigma, int64_t n, int64_t lda, int kmax,
                        int round, int64_t c0, int64_t c1, const int64_t* selected, int extract,
                        void* ws, size_t ws_bytes, void* stream) {
  VG_TRY(check_matrix(fn, Sigma, n, lda, kmax));
  VG_ARG(round >= 0 && round < kmax, 5);
  VG_ARG(c0 >= 0 && c0 <= c1 && c1 <= n, 6);
  VG_ARG(selected != nullptr || round == 0, 8);
  const GreedyWS w = greedy_layout(ws, n, kmax);
  VG_TRY(check_ws(fn, 0, ws, ws_bytes, w.bytes));
  hipStream_t s = as_stream(stream);
  if (c1 == c0) return 0;
  if (round > 0) {
    if (extract) launch_extract(Sigma, n, lda, selected, round, w, 0, n, s);
    launch_trmv(Sigma, n, lda, selected, round, w, c0, c1, s);
  }
  launch_update(Sigma, n, lda, selected, round, w, c0, c1, w.part, 0, s);
  VG_HIP_AS(fn, hipGetLastError());
  return 0;
}

}  // namespace vgposp

using namespace vgposp;

extern "C" size_t vgposp_greedy_workspace_bytes(int64_t n, int kmax) {
  if (n <= 0 || kmax <= 0) return 0;
  return greedy_layout(nullptr, n, kmax).bytes;
}

extern "C" int vgposp_greedy_init_ex(double* Sigma, int64_t n, int64_t lda, int kmax,
                                     double jitter, double threshold, double cache_init, int* info,
                                     void* ws, size_t ws_bytes, void* stream) {
  return init_entry(__func__, 8, Sigma, n, lda, kmax, jitter, threshold, cache_init, info, ws,
                    ws_bytes, stream);
}

extern "C" int vgposp_greedy_init(double* Sigma, int64_t n, int64_t lda, int kmax, int* info,
                                  void* ws, size_t ws_bytes, void* stream) {
  return init_entry(__func__, 5, Sigma, n, lda, kmax, 0.0, DELTA_EPS, __builtin_huge_val(), info,
                    ws, ws_bytes, stream);
}

extern "C" int vgposp_greedy_update_ex(const double* Sigma, int64_t n, int64_t lda, int kmax,
                                       int round, int64_t c0, int64_t c1, const int64_t* selected,
                                       int extract, void* ws, size_t ws_bytes, void* stream) {
  return update_entry(__func__, Sigma, n, lda, kmax, round, c0, c1, selected, extract, ws,
                      ws_bytes, stream);
}

extern "C" int vgposp_greedy_update(const double* Sigma, int64_t n, int64_t lda, int kmax,
                                    int round, int64_t c0, int64_t c1, const int64_t* selected,
                                    void* ws, size_t ws_bytes, void* stream) {
  return update_entry(__func__, Sigma, n, lda, kmax, round, c0, c1, selected, 1, ws, ws_bytes,
                      stream);
}

extern "C" int vgposp_greedy_extract(const double* Sigma, int64_t n, int64_t lda, int kmax,
                                     int round, int64_t own0, int64_t own1,
                                     const int64_t* selected, void* ws, size_t ws_bytes,
                                     void* stream) {
  VG_TRY(check_matrix(__func__, Sigma, n, lda, kmax));
  VG_CHECK_ARG(round >= 1 && round < kmax, 5);
  VG_CHECK_ARG(own0 >= 0 && own0 <= own1 && own1 <= n, 6);
  VG_CHECK_ARG(selected != nullptr, 8);
  const GreedyWS w = greedy_layout(ws, n, kmax);
  VG_TRY(check_ws(__func__, 0, ws, ws_bytes, w.bytes));
  launch_extract(Sigma, n, lda, selected, round, w, own0, own1, as_stream(stream));
  VG_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t vgposp_greedy_slab_tmp_bytes(int64_t n, int64_t c0, int64_t c1) {
  if (n <= 0 || c0 < 0 || c1 <= c0 || c1 > n) return 0;
  return partial_inverse_tmp_bytes(n, c0, c1);
}

extern "C" int vgposp_greedy_prepare(double* Sigma, int64_t n, int64_t lda, int kmax,
                                     double jitter, double threshold, double cache_init, int* info,
                                     void* ws, size_t ws_bytes, void* stream) {
  VG_TRY(check_matrix(__func__, Sigma, n, lda, kmax));
  VG_TRY(check_init(__func__, jitter, threshold, cache_init, 8, info, true));
  const GreedyWS w = greedy_layout(ws, n, kmax);
  VG_TRY(check_ws(__func__, 0, ws, ws_bytes, w.bytes));
  return run_prepare(__func__, Sigma, n, lda, jitter, threshold, cache_init, info, w,
                     as_stream(stream));
}

extern "C" int vgposp_greedy_fact_ws(void* ws, int64_t n, int kmax, void** fws,
                                     size_t* fws_bytes) {
  VG_TRY(check_view(__func__, ws, n, kmax));
  VG_CHECK_ARG(fws != nullptr && fws_bytes != nullptr, 4);
  *fws = greedy_fact_ws(ws, greedy_layout(ws, n, kmax), n);
  *fws_bytes = potrf_ws_bytes(n);
  return 0;
}

extern "C" int vgposp_greedy_finish_slab(double* Sigma, int64_t n, int64_t lda, int kmax,
                                         int64_t c0, int64_t c1, double* tmp, size_t tmp_bytes,
                                         void* ws, size_t ws_bytes, void* stream) {
  VG_TRY(check_matrix(__func__, Sigma, n, lda, kmax));
  VG_TRY(check_slab(__func__, 5, n, c0, c1, tmp, tmp_bytes));
  const GreedyWS w = greedy_layout(ws, n, kmax);
  VG_TRY(check_ws(__func__, 9, ws, ws_bytes, w.bytes));
  return run_finish_slab(__func__, Sigma, n, lda, kmax, c0, c1, tmp, ws, w, as_stream(stream));
}

extern "C" int vgposp_greedy_init_slab(double* Sigma, int64_t n, int64_t lda, int kmax,
                                       double jitter, double threshold, double cache_init,
                                       int64_t c0, int64_t c1, double* tmp, size_t tmp_bytes,
                                       int* info, void* ws, size_t ws_bytes, void* stream) {
  VG_TRY(check_matrix(__func__, Sigma, n, lda, kmax));
  VG_TRY(check_init(__func__, jitter, threshold, cache_init, 12, info, true));
  VG_TRY(check_slab(__func__, 8, n, c0, c1, tmp, tmp_bytes));
  const GreedyWS w = greedy_layout(ws, n, kmax);
  VG_TRY(check_ws(__func__, 0, ws, ws_bytes, w.bytes));
  hipStream_t s = as_stream(stream);
  VG_TRY(run_prepare(__func__, Sigma, n, lda, jitter, threshold, cache_init, info, w, s));
  // (the slab path stays classical, like the sharded factorization it stands in for)
  VG_TRY(potrf_one(Sigma, n, lda, /*invert=*/0, nullptr, info, greedy_fact_ws(ws, w, n), s,
                   /*early=*/false, /*strassen=*/false));
  return run_finish_slab(__func__, Sigma, n, lda, kmax, c0, c1, tmp, ws, w, s);
}

extern "C" int vgposp_greedy_xcol(void* ws, int64_t n, int kmax, double** xcol) {
  VG_TRY(check_view(__func__, ws, n, kmax));
  VG_CHECK_ARG(xcol != nullptr, 4);
  *xcol = greedy_layout(ws, n, kmax).xcol;
  return 0;
}

extern "C" int vgposp_greedy_select(int64_t n, int kmax, int round, int lazy, int64_t c0,
                                    int64_t c1, int64_t* selected, double* sel_delta,
                                    int64_t* evals, void* ws, size_t ws_bytes, void* stream) {
  VG_TRY(check_sizes(__func__, 1, n, kmax));
  VG_CHECK_ARG(round >= 0 && round < kmax, 3);
  VG_CHECK_ARG(c0 >= 0 && c0 <= c1 && c1 <= n, 5);
  VG_CHECK_ARG(selected != nullptr, 7);
  const GreedyWS w = greedy_layout(ws, n, kmax);
  VG_TRY(check_ws(__func__, 0, ws, ws_bytes, w.bytes));
  launch_select(n, round, lazy ? 1 : 0, selected, sel_delta, evals, w, c0, c1, as_stream(stream));
  VG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vgposp_greedy_select_window(int64_t n, int kmax, int round, int64_t I0, int64_t I1,
                                           int64_t I2, int cutoff, int64_t c0, int64_t c1,
                                           int64_t* selected, double* sel_delta, int64_t* evals,
                                           void* ws, size_t ws_bytes, void* stream) {
  VG_TRY(check_sizes(__func__, 1, n, kmax));
  VG_CHECK_ARG(round >= 0 && round < kmax, 3);
  VG_CHECK_ARG(I0 >= 1 && I1 >= 1 && I2 >= 1 && I0 * I1 * I2 == n, 4);
  VG_CHECK_ARG(cutoff >= 0, 7);
  VG_CHECK_ARG(c0 >= 0 && c0 <= c1 && c1 <= n, 8);
  VG_CHECK_ARG(selected != nullptr, 10);
  const GreedyWS w = greedy_layout(ws, n, kmax);
  VG_TRY(check_ws(__func__, 0, ws, ws_bytes, w.bytes));
  hipStream_t s = as_stream(stream);
  {
    ProfScope psw("greedy_window", s, 0.0, 0.0);
    if (round == 0) {
      hipLaunchKernelGGL(greedy_cache_all_kernel, dim3((unsigned)ceil_div(n, CH)), dim3(CH), 0, s,
                         n, w);
    } else {
      const int64_t span = 2 * (int64_t)cutoff;
      const int64_t total = span * span * span;
      const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(total, 256), 4096));
      hipLaunchKernelGGL(greedy_window_kernel, dim3(g), dim3(256), 0, s, selected, round, I0, I1,
                         I2, cutoff, w);
    }
  }
  launch_select(n, round, 2, selected, sel_delta, evals, w, c0, c1, s);
  VG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vgposp_greedy_step(const double* Sigma, int64_t n, int64_t lda, int kmax, int round,
                                  int lazy, int64_t* selected, double* sel_delta, int64_t* evals,
                                  void* ws, size_t ws_bytes, void* stream) {
  VG_TRY(check_matrix(__func__, Sigma, n, lda, kmax));
  VG_CHECK_ARG(round >= 0 && round < kmax, 5);
  VG_CHECK_ARG(selected != nullptr, 7);
  const GreedyWS w = greedy_layout(ws, n, kmax);
  VG_TRY(check_ws(__func__, 0, ws, ws_bytes, w.bytes));
  hipStream_t s = as_stream(stream);
  const int width = g_spec_width.load(std::memory_order_relaxed);
  const bool spec = width > 1 && round > 0;
  if (round > 0) launch_extract(Sigma, n, lda, selected, round, w, 0, n, s);
  if (spec)
    with_width<2>(width, [&](auto t) {
      launch_spec_pass<decltype(t)::value>(Sigma, n, lda, kmax, round, selected, w, s);
    });
  else if (round > 0)
    launch_trmv(Sigma, n, lda, selected, round, w, 0, n, s);
  launch_update(Sigma, n, lda, selected, round, w, 0, n, w.part, spec, s);
  launch_select(n, round, lazy ? 1 : 0, selected, sel_delta, evals, w, 0, n, s);
  VG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vgposp_greedy_set_speculation(int width) {
  clear_error();
  VG_CHECK_ARG(width == 1 || width == 2 || width == 4 || width == 8, 1);
  g_spec_width.store(width, std::memory_order_relaxed);
  return 0;
}

extern "C" int vgposp_greedy_speculation(void) { return g_spec_width.load(); }

extern "C" int vgposp_greedy_spec_stats(void* ws, int64_t n, int kmax, int64_t* passes,
                                        int64_t* hits, int64_t* cached) {
  VG_TRY(check_view(__func__, ws, n, kmax));
  long long h[3];
  VG_HIP(hipMemcpy(h, greedy_layout(ws, n, kmax).spec, sizeof(h), hipMemcpyDeviceToHost));
  if (cached) *cached = h[H_COUNT];
  if (passes) *passes = h[H_PASSES];
  if (hits) *hits = h[H_HITS];
  return 0;
}

extern "C" int vgposp_greedy_spec_table(void* ws, int64_t n, int kmax, int64_t** column,
                                        int64_t** fill_round, int64_t* slots) {
  VG_TRY(check_view(__func__, ws, n, kmax));
  const GreedyWS w = greedy_layout(ws, n, kmax);
  if (column) *column = (int64_t*)(w.spec + SPEC_HDR);
  if (fill_round) *fill_round = (int64_t*)(w.spec + SPEC_HDR + spec_slots(kmax));
  if (slots) *slots = spec_slots(kmax);
  return 0;
}

extern "C" int vgposp_greedy_buffers(void* ws, int64_t n, int kmax, double** delta, double** piv,
                                     int64_t* piv_len) {
  VG_TRY(check_view(__func__, ws, n, kmax));
  const GreedyWS w = greedy_layout(ws, n, kmax);
  if (delta) *delta = w.delta;
  if (piv) *piv = w.piv;
  if (piv_len) *piv_len = 2 + 2 * (int64_t)kmax;
  return 0;
}

extern "C" int vgposp_greedy_cache(void* ws, int64_t n, int kmax, double** cache) {
  VG_TRY(check_view(__func__, ws, n, kmax));
  VG_CHECK_ARG(cache != nullptr, 4);
  *cache = greedy_layout(ws, n, kmax).cache;
  return 0;
}

extern "C" int vgposp_greedy_exclude(void* ws, int64_t n, int kmax, int64_t idx, void* stream) {
  VG_TRY(check_view(__func__, ws, n, kmax));
  VG_CHECK_ARG(idx >= 0 && idx < n, 4);
  hipLaunchKernelGGL(greedy_exclude_kernel, dim3(1), dim3(1), 0, as_stream(stream),
                     greedy_layout(ws, n, kmax).selmask, idx);
  VG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vgposp_greedy_mask(void* ws, int64_t n, int kmax, const unsigned char* allowed,
                                  void* stream) {
  VG_CHECK_ARG(ws != nullptr, 1);
  VG_TRY(check_sizes(__func__, 2, n, kmax));
  VG_CHECK_ARG(allowed != nullptr, 4);
  hipLaunchKernelGGL(greedy_mask_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0,
                     as_stream(stream), n, allowed, greedy_layout(ws, n, kmax).selmask);
  VG_LAUNCH_CHECK();
  return 0;
}

extern "C" int vgposp_greedy_force(int64_t n, int kmax, int round, const int64_t* forced,
                                   int64_t j, int64_t* selected, void* ws, size_t ws_bytes,
                                   void* stream) {
  VG_TRY(check_sizes(__func__, 1, n, kmax));
  VG_CHECK_ARG(round >= 0 && round < kmax, 3);
  VG_CHECK_ARG(forced != nullptr, 4);
  VG_CHECK_ARG(j >= 0, 5);
  VG_CHECK_ARG(selected != nullptr, 6);
  const GreedyWS w = greedy_layout(ws, n, kmax);
  VG_TRY(check_ws(__func__, 0, ws, ws_bytes, w.bytes));
  hipLaunchKernelGGL(greedy_force_kernel, dim3(1), dim3(256), 0, as_stream(stream), n, round,
                     forced, j, selected, w);
  VG_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t vgposp_greedy_condition_workspace_bytes(int64_t n, int batch) {
  if (n <= 0 || !cond_batch_ok(batch)) return 0;
  return batch == 1 ? 256 : cond_layout(nullptr, n, batch).bytes;
}

extern "C" int vgposp_greedy_condition(const double* Sigma, int64_t n, int64_t lda, int kmax,
                                       int m, int k, int batch, const int64_t* placed,
                                       int64_t* selected, void* ws, size_t ws_bytes,
                                       void* scratch, size_t scratch_bytes, void* stream) {
  VG_TRY(check_matrix(__func__, Sigma, n, lda, kmax));
  VG_CHECK_ARG(m >= 1 && m <= kmax, 5);
  VG_CHECK_ARG(k >= 0 && (int64_t)m + k <= kmax, 6);
  VG_CHECK_ARG(batch >= 1 && cond_batch_ok(batch), 7);
  VG_CHECK_ARG(placed != nullptr, 8);
  VG_CHECK_ARG(selected != nullptr, 9);
  const GreedyWS w = greedy_layout(ws, n, kmax);
  VG_TRY(check_ws(__func__, 0, ws, ws_bytes, w.bytes));
  VG_CHECK_ARG(scratch != nullptr, 12);
  const size_t need = batch == 1 ? 256 : cond_layout(nullptr, n, batch).bytes;
  if (scratch_bytes < need) {
    set_error("%s: scratch %zu < %zu bytes", __func__, scratch_bytes, need);
    return VGPOSP_E_WS;
  }
  hipStream_t s = as_stream(stream);
  // round r conditions on a_{r-1} = placed[r - 1], then A <- A + [a_r]; round 0: nom =
  // diag(Sigma), prec = Q_ii from init's column norms.  a_{m-1}'s column is left to the next
  // vgposp_greedy_step (round m), whose own mat-vec reads selected[m - 1]
  auto place = [&](int r, double* part) {
    launch_update(Sigma, n, lda, selected, r, w, 0, n, part, 0, s);
    hipLaunchKernelGGL(greedy_force_kernel, dim3(1), dim3(256), 0, s, n, r, placed, r, selected, w);
  };
  place(0, w.part);
  if (batch == 1) {
    for (int r = 1; r < m; ++r) {
      launch_extract(Sigma, n, lda, selected, r, w, 0, n, s);
      launch_trmv(Sigma, n, lda, selected, r, w, 0, n, s);
      place(r, w.part);
    }
  } else {
    const CondScratch c = cond_layout(scratch, n, batch);
    const int64_t slice = ceil_div(n, RC) * n;
    for (int j0 = 0; j0 < m - 1; j0 += batch) {
      const int nt = std::min(batch, m - 1 - j0);
      with_width<4>(batch, [&](auto t) {
        launch_cond_batch<decltype(t)::value>(Sigma, n, lda, placed, j0, nt, c, s);
      });
      for (int j = 0; j < nt; ++j) place(j0 + j + 1, c.part + (int64_t)j * slice);
    }
  }
  VG_LAUNCH_CHECK();
  return 0;
}
