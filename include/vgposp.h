/*
 * vgposp.h — C-ABI of libvgposp.so, the MI355X (gfx950) hot path of DL-WG/VGPosp:
 * GP kernel assembly -> fp64 Cholesky (+ fused inverse) -> GP log-marginal-likelihood / gradient
 * -> greedy mutual-information sensor placement.
 *
 * The reference exposes this path as Python (TF1 graph + TFP + numpy).  Each entry point below
 * names the reference interface it replaces (file:line under the reference checkout).  Bindings:
 * vgposp_amd/_lib.py (ctypes); a maintainer-side ctypes stub for the reference is in
 * INTEGRATION.md.
 *
 * Conventions
 *   - Every array argument is a caller-owned DEVICE pointer (e.g. a torch tensor's data_ptr());
 *     the library never allocates device memory.  Scratch is passed in as `ws`/`ws_bytes`, sized
 *     by the matching *_workspace_bytes() query.
 *   - Matrices are row-major fp64 with an explicit leading dimension (elements).  Batched
 *     operands are `batch` matrices `stride` elements apart.
 *   - `stream` is a hipStream_t (may be NULL = default stream).  Calls only enqueue work: no host
 *     synchronisation happens inside the library, so device-side status (`info`) must be read by
 *     the caller after synchronising.
 *   - Return: 0 = enqueued; -i = argument i (1-based) invalid; VGPOSP_E_HIP = HIP runtime error;
 *     VGPOSP_E_WS = workspace too small.  vgposp_last_error() returns a thread-local message.
 *   - Device `info` (int32 per batch entry): 0 = success, k > 0 = the leading minor of order k
 *     is not positive definite (LAPACK potrf convention).  The Python layer maps k > 0 to the
 *     TF error "Cholesky decomposition was not successful".
 *   - Stateless and re-entrant; concurrent calls on different streams with disjoint buffers are
 *     safe.
 */
#ifndef VGPOSP_H_
#define VGPOSP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGPOSP_ABI_VERSION 2

#define VGPOSP_E_HIP (-100)
#define VGPOSP_E_WS (-101)
#define VGPOSP_E_UNSUPPORTED (-102) /* a run-time library or one of its kernels is missing */

/* PSD kernel families (tfp.positive_semidefinite_kernels). */
#define VGPOSP_KERNEL_EQ 0       /* ExponentiatedQuadratic: 3D_sin_wave.py:158-159, main_tests.py:617 */
#define VGPOSP_KERNEL_MATERN12 1 /* MaternOneHalf: gp_functions.py:160-163, main.py:94 */
#define VGPOSP_KERNEL_MATERN32 2 /* MaternThreeHalves */
#define VGPOSP_KERNEL_MATERN52 3 /* MaternFiveHalves: main_architecture_2_sampledistribution.py:211 */

/* Output triangle selectors. */
#define VGPOSP_FULL 0
#define VGPOSP_LOWER 1

int vgposp_abi_version(void);
const char* vgposp_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Kernel assembly.  Replaces `kernel.matrix(x1, x2)` of the TFP PSD kernels built by
 * gp_functions.create_cov_kernel (gp_functions.py:160-163) and consumed by tfd.GaussianProcess
 * (gp_functions.py:166-172), GPRM (:283-297) and the VGP (variational_Gaussian_process_example.py
 * :55-89):
 *     K[b][i][j] = exp(2*log(amp[b]) + log k(|X1_i - X2_j| / ls[b])) + (i==j ? diag_shift[b] : 0)
 * X1: n1 x d, X2: n2 x d (row-major, d <= 8).  amp, ls: [batch] device arrays.  diag_shift:
 * [batch] device array or NULL (added on i == j, used for noise + jitter of a symmetric K).
 * uplo = VGPOSP_LOWER writes only j <= i (the upper triangle is left untouched).
 * --------------------------------------------------------------------------------------------- */
int vgposp_kernel_matrix(int kind, const double* X1, int64_t n1, const double* X2, int64_t n2,
                         int d, const double* amp, const double* ls, const double* diag_shift,
                         int batch, int uplo, double* K, int64_t ldk, int64_t stride_k,
                         void* stream);

/* Kernel assembly fused with its product by a vector (the VGP's optimal posterior,
 * variational_Gaussian_process_example.py:68-74, needs Kzx and c = Kzx y over all N observations):
 * writes the full K (batch 1, no diagonal shift) and out[n1] = K v[n2] without re-reading K.
 * Deterministic (per-tile partials in ws, summed in a fixed order); ws is
 * vgposp_kernel_matrix_matvec_workspace_bytes(n1, n2) bytes. */
size_t vgposp_kernel_matrix_matvec_workspace_bytes(int64_t n1, int64_t n2);
int vgposp_kernel_matrix_matvec(int kind, const double* X1, int64_t n1, const double* X2,
                                int64_t n2, int d, const double* amp, const double* ls, double* K,
                                int64_t ldk, const double* v, double* out, void* ws,
                                size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * fp64 GEMM on MFMA (v_mfma_f64_16x16x4f64):  C = alpha * op(A) * op(B) + beta * C
 * op(A) = A (m x k, transa=0) or A^T (A stored k x m, transa=1);
 * op(B) = B (k x n, transb=0) or B^T (B stored n x k, transb=1).
 * uplo_c = VGPOSP_LOWER updates only the lower triangle of C (j <= i).  tri_a / tri_b = 1 treat
 * the STORED A / B as lower triangular (entries above their diagonal read as 0).
 * The building block of the Cholesky trailing update / TRMM / C^-1 formation below.
 * --------------------------------------------------------------------------------------------- */
int vgposp_gemm(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                const double* A, int64_t lda, const double* B, int64_t ldb, double beta,
                double* C, int64_t ldc, int uplo_c, int tri_a, int tri_b, void* stream);

/* Batched vgposp_gemm: element b (< batch) computes C + b sC from A + b sA and B + b sB, all in
 * one launch (e.g. the VGP's four M x M inverse factors' L^-T L^-1).  Split-K over the workspace
 * as vgposp_gemm_splitk when ws holds vgposp_gemm_batched_workspace_bytes, else unsplit. */
size_t vgposp_gemm_batched_workspace_bytes(int64_t m, int64_t n, int64_t k, int uplo_c, int batch);
int vgposp_gemm_batched(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                        const double* A, int64_t lda, int64_t sA, const double* B, int64_t ldb,
                        int64_t sB, double beta, double* C, int64_t ldc, int64_t sC, int uplo_c,
                        int tri_a, int tri_b, int batch, void* ws, size_t ws_bytes, void* stream);

/* Split-K form of vgposp_gemm for few output tiles and a long K (e.g. the VGP's
 * Kzx Kzx^T with M = 512 inducing points and K = N = 262,144 observations: 10 lower tiles).  Each
 * of `splits` K-ranges writes alpha * partial into ws ([splits][m][n]); a second kernel sums them
 * in a fixed order and adds beta * C, so results are deterministic.  splits <= 0 chooses a count
 * (about 512 workgroups, >= 512-deep ranges).  Falls back to vgposp_gemm's kernels (no split) for
 * operands the MFMA path does not take. */
size_t vgposp_gemm_splitk_workspace_bytes(int64_t m, int64_t n, int64_t k, int uplo_c, int splits);
/* Process-wide tuning of the automatic split-K: a short-K split (few output tiles, K < 4096) is at
 * least min_k deep (a multiple of 16 in [16, 4096]; default 16, measured: profiles/
 * r4_vgp_ab_splitk_*.jsonl).  Change it only while no work that was sized under the old value
 * is being enqueued: workspace queries (vgposp_*_workspace_bytes) and the launches that use the
 * workspace must see the same value.  Not read from the environment. */
int vgposp_gemm_set_split_depth(int min_k);
int vgposp_gemm_split_depth(void);
/* Process-wide choice of the fast GEMM kernels' K loop for products with transa = 0 (every
 * entry point that launches them, grouped launches excepted): 0 = the compiler-scheduled C++
 * loop, 1 = the hand-scheduled loop for the K-tiles that need no mask.  Both give bit-identical
 * results.  Read at launch; not read from the environment. */
int vgposp_gemm_set_kloop(int kloop);
int vgposp_gemm_kloop(void);
/* Process-wide choice of the fast GEMM kernels' epilogue (every entry point that launches them,
 * grouped launches included): 0 = the element-wise reference (one memory round trip per
 * accumulator element and destination), 1 = the batched one (16 loads, one wait, 16 stores per
 * group and destination; interior tiles without tests).  Both give bit-identical results.  Read
 * at launch; not read from the environment. */
int vgposp_gemm_set_epilogue(int epilogue);
int vgposp_gemm_epilogue(void);
int vgposp_gemm_splitk(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                       const double* A, int64_t lda, const double* B, int64_t ldb, double beta,
                       double* C, int64_t ldc, int uplo_c, int tri_a, int tri_b, int splits,
                       void* ws, size_t ws_bytes, void* stream);

/* Strassen form of vgposp_gemm for large plain products (full C, dense operands, C not
 * overlapping A or B): up to `levels` (0..2) levels of the classic seven-product recursion in
 * native fp64.  A level is taken while m, n and k are each a multiple of 256 and >= min_dim (the
 * process-wide value below) and the operands are 16-byte aligned with even leading dimensions;
 * every product is one launch that accumulates into all the quadrants of C it belongs to, the
 * operand sums go through ws (vgposp_gemm_strassen_workspace_bytes).  Anything not eligible, and
 * levels = 0, is vgposp_gemm's single launch, bit-identical.  Results are fp64-accurate in the
 * norm-wise sense (Higham, Accuracy and Stability of Numerical Algorithms, §23.2.2),
 * deterministic, and not bit-identical to vgposp_gemm.
 * vgposp_potrf_set_strassen(min_dim, levels): process-wide; min_dim a multiple of 256, levels
 * 0..2 (0 = off).  ON BY DEFAULT with min_dim 8192 and 2 levels (DESIGN.md §4 "Strassen": the
 * 65k step 6.7 % faster).  vgposp_potrf_lower (single matrix) and vgposp_greedy_init run the
 * plain products of the fused Cholesky + inverse with all dimensions >= min_dim this way, and
 * vgposp_potrf_workspace_bytes / vgposp_greedy_workspace_bytes grow by the operand temporaries
 * of the largest eligible product (none below n = 4 min_dim; 2.7 GB at n = 65,536).  Results
 * at n >= 32,768 are therefore fp64-accurate but not bit-identical to the classical recursion;
 * levels = 0 restores it exactly.  Same caveat as the split depth: change the setting only
 * between a workspace query and its use, consistently.  Batched, sharded and slab
 * factorizations stay classical. */
int vgposp_potrf_set_strassen(int64_t min_dim, int levels);
int vgposp_potrf_strassen(int64_t* min_dim, int* levels);
size_t vgposp_gemm_strassen_workspace_bytes(int64_t m, int64_t n, int64_t k, int levels);
int vgposp_gemm_strassen(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                         const double* A, int64_t lda, const double* B, int64_t ldb, double beta,
                         double* C, int64_t ldc, int levels, void* ws, size_t ws_bytes,
                         void* stream);

/* The same product with fp64 emulated on the int8 matrix cores (the integer modular scheme,
 * "Ozaki scheme II"; DESIGN.md §4 "fp64 products on the int8 matrix cores"): rows of op(A) and
 * columns of op(B) are scaled by powers of two and truncated to integers below 2^s, sixteen int8
 * residue planes per operand go through sixteen exact int8 -> int32 products of hipBLASLt, and
 * every element is rebuilt exactly (Garner, a 128-bit integer, one rounding).  The error is the
 * truncation alone: |dC_ij| <= 2 k 2^-s max_k|a_ik| max_k|b_kj| with s = floor((125.37 - 1 -
 * ceil(log2 k)) / 2), at most 57; integer-valued operands below 2^s give the exact product.  A row
 * of op(A) or column of op(B) with a non-finite entry makes its row or column of C NaN.
 * k <= 65,536.  hipBLASLt is bound at run time (dlopen of libhipblaslt.so.1, the process's own copy
 * first) and never linked: vgposp_gemm_emulation_available tells whether it resolved, and
 * vgposp_gemm_emulated returns VGPOSP_E_UNSUPPORTED without it.  ws holds
 * vgposp_gemm_emulated_workspace_bytes (the planes of both operands and the int32 results of one
 * output block, together at most 24 GiB + the planes' excess over it).  Deterministic; all four
 * layouts; C may overlap A or B.
 * The fused Cholesky + inverse takes its large plain products (every dimension a multiple of 256
 * and >= min_dim, the products Strassen takes at the same threshold) this way when the
 * process-wide setting below has moduli = 16 and the library resolves; moduli = 0 turns it off.
 * ON BY DEFAULT with min_dim 8192 (the 65k step 18.7 % faster), which leaves every
 * n < 32,768 as it was; where the library does not resolve, everything is as without it.  The
 * workspace queries of the factorization and of the greedy
 * placement grow by the emulation scratch of the largest such product, appended behind the
 * Strassen scratch, which keeps its size and place and serves when the library fails at run
 * time.  Change the setting only between a workspace query and its use, consistently.
 * Test hooks: set_unavailable(1) makes the library count as absent, set_block_cap(bytes) lowers
 * the 24 GiB cap (0 restores it), garner runs the reconstruction of one element on the host
 * (sixteen residues -> sixteen symmetric mixed-radix digits and their integer rounded to fp64),
 * vgposp_gemm_set_abort_flag sets the calling thread's device abort flag of every dense product
 * (a device int; non-zero = launches return without writing; NULL = none). */
int vgposp_gemm_emulation_available(void);
int vgposp_gemm_emulation_set_unavailable(int off);
int vgposp_gemm_emulation_set_block_cap(size_t bytes);
int vgposp_gemm_emulation_garner(const int32_t* residues, int32_t* digits, double* value);
int vgposp_gemm_set_abort_flag(const void* flag);
int vgposp_potrf_set_emulation(int64_t min_dim, int moduli);
int vgposp_potrf_emulation(int64_t* min_dim, int* moduli);
size_t vgposp_gemm_emulated_workspace_bytes(int64_t m, int64_t n, int64_t k);
int vgposp_gemm_emulated(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                         const double* A, int64_t lda, const double* B, int64_t ldb, double beta,
                         double* C, int64_t ldc, void* ws, size_t ws_bytes, void* stream);

/* The structured products of the factorization on the same int8 path, each as a staircase of
 * rectangular block products over planes that are split ONCE:
 *   VGPOSP_EMUL_SYRK_LOWER  C (n x n, lower triangle only) = alpha A A^T + beta C,  A n x k (m = n;
 *                           B is not read); the strict upper triangle of C is neither read nor
 *                           written;
 *   VGPOSP_EMUL_TRMM_B      C (m x n) = alpha A X + beta C,  A m x n, X = B n x n lower triangular
 *                           stored [k][j] (k = n);
 *   VGPOSP_EMUL_TRMM_A      C (m x n) = alpha X B + beta C,  X = A m x m lower triangular stored
 *                           [i][k], B m x n (k = m).
 * The strict upper triangle of X is never loaded.  Error bound and non-finite rule as above, with
 * the maxima taken over the entries that are read.  ws may be of any size: the planner cuts the
 * product into tiles whose planes and int32 block fit ws_bytes (and the block cap);
 * VGPOSP_E_UNSUPPORTED when not even one block fits or the library has no kernel.  C must not
 * overlap A or B.  vgposp_gemm_emulation_tri_plan is the planner alone (no GPU): the steps, 14
 * int64 each (tile, tile rows r0 r1, tile columns c0 c1, the depth ka kb its planes hold, the
 * step's rows i0 i1, columns j0 j1 and depth k0 k1, the tile's bytes), and the int8 flops
 * (2 * 16 * rows * columns * depth rounded up to 128, summed); it returns the number of steps or -1.
 * The fused Cholesky + inverse sends a structured product here exactly where it would otherwise
 * split it for the plain-product emulation (vgposp_potrf_set_emulation_structured(0) turns that
 * off; on by default).  Test hook: set_tri_block(width) sets the staircase's block width (a
 * multiple of 128; 0 restores the default, 2,048). */
#define VGPOSP_EMUL_SYRK_LOWER 0
#define VGPOSP_EMUL_TRMM_B 1
#define VGPOSP_EMUL_TRMM_A 2
#define VGPOSP_EMUL_TRI_STEP_FIELDS 14
int vgposp_gemm_emulation_set_tri_block(int64_t width);
int vgposp_potrf_set_emulation_structured(int on);
int vgposp_potrf_emulation_structured(void);
int64_t vgposp_gemm_emulation_tri_plan(int kind, int64_t m, int64_t n, int64_t k, size_t bytes,
                                       int64_t* steps, int64_t cap_steps, double* flops);
int vgposp_gemm_emulated_tri(int kind, int64_t m, int64_t n, int64_t k, double alpha,
                             const double* A, int64_t lda, const double* B, int64_t ldb,
                             double beta, double* C, int64_t ldc, void* ws, size_t ws_bytes,
                             void* stream);

/* Grouped vgposp_gemm: `count` independent products, problem g with flags[5g..5g+4] = (transa,
 * transb, uplo_c, tri_a, tri_b), dims[3g..3g+2] = (m, n, k), alpha[g], beta[g], A[g] (lda[g]),
 * B[g] (ldb[g]), C[g] (ldc[g]), all in ONE launch (problem on blockIdx.y) plus one grouped split-K
 * reduction; problems the MFMA tile kernel does not take (n == 1, odd or unaligned operands) run
 * one by one.  For the VGP step's latency-bound M x M products.  ws holds
 * vgposp_gemm_group_workspace_bytes(count, flags, dims) bytes of split-K partials. */
size_t vgposp_gemm_group_workspace_bytes(int count, const int* flags, const int64_t* dims);
int vgposp_gemm_group(int count, const int* flags, const int64_t* dims, const double* alpha,
                      const double* beta, const double* const* A, const int64_t* lda,
                      const double* const* B, const int64_t* ldb, double* const* C,
                      const int64_t* ldc, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * VGP training-step glue (vgposp_amd/vgp_training.py): the non-GEMM element-wise and reduction
 * parts of variational_loss and of the gradient TF autodiff takes through it
 * (variational_Gaussian_process_example.py:51-102, AdamOptimizer.minimize).  Row-major fp64; s
 * (the observation noise variance) and amp are device scalars, so the step has no host sync.
 *   vgposp_vgp_sinv:       P0 (lower, from the SYRK) -> symmetric in place;
 *                          F[0] = Sinv = Kzz + P0 / s + pj I  (n x n, ld n); nf = 4 also
 *                          writes F[1] = Kzz + jitter I, F[2] = Kzz + (s + 1e-6) I, F[3] = Kzz
 *                          (the step's four M x M factorizations, done as one batch)
 *   vgposp_sym_from_lower: A's strict upper triangle <- its lower triangle
 *   vgposp_lincomb:        out = sum_k coef[k] (s + shift)^spow[k] X[k], on i == j times
 *                          diag_scale plus diag_coef (s + shift)^diag_spow; k <= 4, all
 *                          rows x cols with ld
 *   vgposp_vgp_kzz_bar:    KzzS = Kbar + Kbar^T of Kzz and G = (2 / s) Sinv_bar, from
 *                          vecs = {u, v, qv, m_bar, t, c_bar} and mats = {HHt, P HHt, Kp^-1,
 *                          QA QA^T, Kzz^-1, Li^T Li, Sc, Li^T A_bar} (n x n, ld n)
 *   vgposp_dots:           out[p] = sum_i x_p[i incx_p] y_p[i incy_p] (y_p NULL: sum x) for
 *                          op 0, sum_i log x_p[i incx_p] for op 1; p < 16, deterministic
 *   vgposp_vgp_scalars:    out = (-E, -dE/damp, -dE/dls, -dE/dnoise) from the sums below, the
 *                          three kernel-VJP gradients g1 (Kzz, halved inside), g2 (Kzx), g3 (Kzb)
 * --------------------------------------------------------------------------------------------- */
enum {
  VGPOSP_S_RR = 0,       /* r . r, r = y_b - Kzb^T Kzj^-1 m            */
  VGPOSP_S_KZB_H = 1,    /* <Kzb, H>, H = Kzj^-1 Kzb                   */
  VGPOSP_S_Q_HHT = 2,    /* <Q, H H^T>                                 */
  VGPOSP_S_PA2 = 3,      /* <Lp^-1 A, Lp^-1 A>                         */
  VGPOSP_S_QM2 = 4,      /* |Lp^-1 m|^2                                */
  VGPOSP_S_LOGDET_S = 5, /* sum log diag chol(Sinv)                    */
  VGPOSP_S_LOGDET_P = 6, /* sum log diag chol(Kzz + (s + 1e-6) I)      */
  VGPOSP_S_LOGDET_K = 7, /* sum log diag chol(Kzz)                     */
  VGPOSP_S_TR_KPINV = 8, /* tr Kp^-1                                   */
  VGPOSP_S_QV2 = 9,      /* |Kp^-1 m|^2                                */
  VGPOSP_S_TR_QAQA = 10, /* tr (Kp^-1 A)(Kp^-1 A)^T                    */
  VGPOSP_S_MB_M = 11,    /* m_bar . m                                  */
  VGPOSP_S_G_P0 = 12,    /* <G, P0>                                    */
  VGPOSP_S_COUNT = 13
};
int vgposp_vgp_sinv(double* P0, int64_t n, int64_t ldp, const double* Kzz, const double* s,
                    double pj, double jitter, double* F, int nf, void* stream);
int vgposp_sym_from_lower(double* A, int64_t n, int64_t lda, void* stream);
int vgposp_lincomb(int64_t rows, int64_t cols, int64_t ld, int nterms, const double* const* X,
                   const double* coef, const int* spow, double diag_scale, double diag_coef,
                   int diag_spow, const double* s, double shift, double* out, void* stream);
int vgposp_vgp_kzz_bar(int64_t n, const double* const* vecs, const double* const* mats,
                       const double* s, double w, double* KzzS, double* G, void* stream);
size_t vgposp_dots_workspace_bytes(int ndots);
int vgposp_dots(int ndots, const double* const* x, const int64_t* incx, const double* const* y,
                const int64_t* incy, const int64_t* len, const int* op, double* out, void* ws,
                size_t ws_bytes, void* stream);
int vgposp_vgp_scalars(const double* sums, const double* s, const double* amp, const double* g1,
                       const double* g2, const double* g3, double nb, double m, double w,
                       double jitter, double* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Vector-Jacobian product of kernel assembly: the reverse pass TF autodiff runs through
 * kernel.matrix when the reference trains a VGP (variational_Gaussian_process_example.py:95-102,
 * AdamOptimizer.minimize over amplitude, length_scale, inducing_index_points).  For one kernel
 * (amp, ls: device [1]) and Kbar [n1 x n2] (ld ldk) plus an optional rank-1 term u w^T
 * (u: [n1], w: [n2], both NULL or both set):
 *     grad[0] = sum_ij Kbar_ij dK_ij/damp,   grad[1] = sum_ij Kbar_ij dK_ij/dls,
 *     X1bar[i][:] = sum_j Kbar_ij dK_ij/dX1[i][:]    (X1bar [n1 x d] or NULL)
 * K is recomputed on the fly (one HBM pass over Kbar).  Deterministic (fixed-order reduction).
 * For a symmetric use (K(Z, Z)) pass Kbar + Kbar^T and halve grad.
 * --------------------------------------------------------------------------------------------- */
size_t vgposp_kernel_vjp_workspace_bytes(int64_t n1, int64_t n2, int d);
int vgposp_kernel_vjp(int kind, const double* X1, int64_t n1, const double* X2, int64_t n2, int d,
                      const double* amp, const double* ls, const double* Kbar, int64_t ldk,
                      const double* u, const double* w, double* grad, double* X1bar, void* ws,
                      size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-feature length scales: tfkern.FeatureScaled(base, scale_diag),
 *     k(x1, x2) = base(x1 / scale_diag, x2 / scale_diag),   scale: device [d], 1 <= d <= 8.
 * vgposp_scale_points: out[i][k] = X[i][k] / scale[k] (a true division, as TFP; out may alias X;
 *   n == 0 returns 0 without device work; no host synchronisation).  Every assembly entry of this
 *   header applied to scaled points is the FeatureScaled kernel.
 * vgposp_kernel_vjp_scaled: vgposp_kernel_vjp on ALREADY-SCALED points Z1 = X1 / scale,
 *   Z2 = X2 / scale, with the scale gradient from the same single pass over Kbar:
 *     grad[0], grad[1] as vgposp_kernel_vjp,
 *     grad[2 + k] = sum_ij (Kbar + u w^T)_ij dK_ij/dscale_k,
 *                   dK_ij/dscale_k = -c_ij (z1_ik - z2_jk)^2 / scale_k,  dK/dz1 = c (z1 - z2),
 *     X1bar [n1 x d] or NULL: with respect to the UNSCALED X1 (the z-space adjoint / scale_k).
 *   grad: [2 + d].  Deterministic (fixed-order reduction, no atomics).
 * vgposp_lml_grad_scaled: vgposp_lml_grad for one FeatureScaled kernel (batch 1) on scaled points
 *   Z [n x d]: grad [3 + d] = (d/damp, d/dls, d/dnoise, d/dscale_0 ... d/dscale_{d-1}),
 *     grad[3 + k] = 0.5 sum_ij (alpha alpha^T - C^-1)_ij dC_ij/dscale_k.
 *   Reads the lower triangle of Cinv.  Deterministic.
 * --------------------------------------------------------------------------------------------- */
int vgposp_scale_points(const double* X, int64_t n, int d, const double* scale, double* out,
                        void* stream);
size_t vgposp_kernel_vjp_scaled_workspace_bytes(int64_t n1, int64_t n2, int d);
int vgposp_kernel_vjp_scaled(int kind, const double* Z1, int64_t n1, const double* Z2, int64_t n2,
                             int d, const double* amp, const double* ls, const double* scale,
                             const double* Kbar, int64_t ldk, const double* u, const double* w,
                             double* grad, double* X1bar, void* ws, size_t ws_bytes,
                             void* stream);
size_t vgposp_lml_grad_scaled_workspace_bytes(int64_t n);
int vgposp_lml_grad_scaled(int kind, const double* Z, int64_t n, int d, const double* amp,
                           const double* ls, const double* scale, const double* Cinv, int64_t ldc,
                           const double* alpha, double* grad, void* ws, size_t ws_bytes,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * Covariance builders (cov_vv on device).
 * vgposp_kernel_matvec: out[i] = sum_j K(X1_i, X2_j) v[j] + beta * out[i] for one kernel (amp, ls:
 *   device [1]), without materialising K: the VGP / GPRM predictive mean at many points, e.g. the
 *   tracer value at every (location, T/P sample) 5-D point that main_architecture_2_
 *   sampledistribution.py:432-458 evaluates one vgp.mean() at a time.
 * vgposp_center_rows: T[i][0:s] <- (T[i][:] - mean(T[i][:])) * scale.  A SYRK of the result
 *   (vgposp_gemm, alpha = 1/s) is tfp.stats.covariance(t_i, t_j, sample_axis=0) for every pair
 *   (main.py:190-199, main_architecture_2_sampledistribution.py:470-479).
 * vgposp_index_taper: C[i][j] *= g(|idx_i - idx_j|), g(d) = exp(-(beta d)^2 / (2 pi)), 0 where
 *   g < threshold, over an I0 x I1 x I2 C-order grid (the beta-decay local kernel filter,
 *   main_architecture_2_sampledistribution.py:361-421; threshold 0.01 there).  uplo as elsewhere.
 * --------------------------------------------------------------------------------------------- */
int vgposp_kernel_matvec(int kind, const double* X1, int64_t n1, const double* X2, int64_t n2,
                         int d, const double* amp, const double* ls, const double* v, double beta,
                         double* out, void* stream);
int vgposp_center_rows(double* T, int64_t n, int64_t s, int64_t ld, double scale, void* stream);
int vgposp_index_taper(double* C, int64_t n, int64_t ldc, int64_t I0, int64_t I1, int64_t I2,
                       double beta, double threshold, int uplo, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Recursive Cholesky, lower, in place (128x128 leaves in LDS, everything else fp64 MFMA GEMMs).
 * Replaces tf.linalg.cholesky inside tfd.GaussianProcess.log_prob / GPRM / VGP
 * (gp_functions.py:166-172, main.py:105, 3D_sin_wave.py:172) and is the O(N^3) core of the dense
 * greedy placement.
 *   invert = 0: lower triangle of A <- L with A = L L^T.
 *   invert = 1: lower triangle of A <- L^-1 (recursive triangular inverse after the factor).
 * The strictly upper triangle of A is never read or written (it keeps Sigma for the greedy
 * nominators).  diag_out ([batch][n], or NULL) receives diag(L) (log-det).  info: [batch] int32.
 * ws must hold vgposp_potrf_workspace_bytes(n), which includes a fixed 64 MiB of split-K
 * partials for every n > 128 (sized for the large factorizations).  A caller that factors a small
 * matrix and minds the memory (the chunked predictive variance) may pass
 * vgposp_potrf_compact_workspace_bytes(n) instead: the partials area is then min(64 MiB, 64 n^2
 * bytes), which holds every split an order-n factorization takes, so the results are bit-identical;
 * the two sizes are equal for n <= 128 and n >= 1024.  Any ws_bytes below the full size is laid
 * out compactly.
 * --------------------------------------------------------------------------------------------- */
size_t vgposp_potrf_compact_workspace_bytes(int64_t n);
/* Workspace for factoring a batch of n > 128 matrices in ONE recursion (every launch covers the
 * whole batch): pass at least this many bytes to vgposp_potrf_lower with batch > 1 (a smaller
 * workspace of vgposp_potrf_workspace_bytes(n) factors them one after another). */
size_t vgposp_potrf_batched_workspace_bytes(int64_t n, int batch);
size_t vgposp_potrf_workspace_bytes(int64_t n);
int vgposp_potrf_lower(double* A, int64_t n, int64_t lda, int64_t stride, int batch, int invert,
                       double* diag_out, int* info, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mixed-precision Cholesky (config C5, "fp32 mixed-prec Cholesky": the VGP's M x M factorizations,
 * tf.linalg.cholesky inside tfd.VariationalGaussianProcess, main_architecture_2_sampledistribution
 * .py:223-265): fp32 factor of A on the f32 matrix cores (v_mfma_f32_16x16x4_f32), then `iters`
 * fp64 refinement steps X <- (I - Phi(X A X^T - I)) X of X0 = L32^-1 (Phi: lower part, diagonal
 * halved), which converge quadratically to the fp64 inverse Cholesky factor.
 *   A: full symmetric n x n (lda), not modified.  Linv (ldl, != A) <- L^-1, zeros above the
 *   diagonal (what vgposp_potrf_lower(invert = 1) leaves in the lower triangle).  diag_out [n] (or
 *   NULL) <- diag(L) = 1 / diag(L^-1).  resid (device double or NULL) <- max|X A X^T - I| of the
 *   last step.  info: k > 0 = fp32 pivot k not positive; n + 1 = not converged (resid > 1e-6).
 * --------------------------------------------------------------------------------------------- */
size_t vgposp_potrf_mixed_workspace_bytes(int64_t n);
int vgposp_potrf_mixed(const double* A, int64_t n, int64_t lda, double* Linv, int64_t ldl,
                       double* diag_out, int iters, double* resid, int* info, void* ws,
                       size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The Cholesky of ONE matrix distributed over R ranks (one process per GPU) that each hold the
 * whole matrix: the O(N^3) factorization behind placement_algorithm2.py:151-219's pinv calls,
 * which the candidate-sharded placement would otherwise replicate on every rank.
 * The host (vgposp_amd/dist_cholesky.py) walks vgposp_potrf_lower's recursion: a node of size nsub
 * at column col0 splits at n1 = vgposp_potrf_split(nsub); nodes below a size threshold are factored
 * whole on every rank (vgposp_potrf_block); above it every rank computes a share of the node's
 * panel TRSM (vgposp_potrf_panel: rows [r0, r1) of L21 = A21 L11^-T, rows counted from col0 + n1)
 * and of its SYRK (vgposp_potrf_trailing: rows [b0, b1) of the lower triangle of A22 -= L21 L21^T),
 * and the ranks all-gather the shares (vgposp_pack_rows / unpack into contiguous buffers, RCCL
 * all-gather).  ws: a vgposp_potrf_workspace_bytes(n) workspace for the whole n (the leaf and
 * 512-block inverses are kept at their global columns, as vgposp_potrf_lower leaves them, e.g.
 * vgposp_greedy_fact_ws's).  col0 is a multiple of 128.
 * vgposp_pack_rows: rows [r0, r1) x columns [c0, c1) of A (lower = 0) or the lower trapezoid
 * (columns [c0, r] of row r; lower = 1 needs c0 <= r0, c1 >= r1) <-> buf, packed row after row
 * (unpack = 1 writes A); vgposp_pack_elems gives the element count.
 * --------------------------------------------------------------------------------------------- */
int64_t vgposp_potrf_split(int64_t n);
int vgposp_potrf_block(double* A, int64_t n, int64_t lda, int64_t col0, int64_t nb, int* info,
                       void* ws, size_t ws_bytes, void* stream);
int vgposp_potrf_panel(double* A, int64_t n, int64_t lda, int64_t col0, int64_t nsub, int64_t r0,
                       int64_t r1, void* ws, size_t ws_bytes, void* stream);
int vgposp_potrf_trailing(double* A, int64_t n, int64_t lda, int64_t col0, int64_t nsub,
                          int64_t b0, int64_t b1, void* ws, size_t ws_bytes, void* stream);
int64_t vgposp_pack_elems(int64_t r0, int64_t r1, int64_t c0, int64_t c1, int lower);
int vgposp_pack_rows(double* A, int64_t lda, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                     int lower, double* buf, int unpack, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Left-side triangular solve with a factor from vgposp_potrf_lower(invert = 0), in place on B:
 *   trans = 0:  B (n x nrhs, ldb) <- L^-1 B        trans = 1:  B <- L^-T B
 * Replaces tf.linalg.triangular_solve(L, ...) inside tfd.GaussianProcess.log_prob and the
 * GPRM posterior (gp_functions.py:166-172, 283-297; SURVEY §8(b) vgposp_trsm_lower).  The
 * strictly upper triangle of L is never read.  ws: vgposp_trsm_workspace_bytes(n, nrhs).
 * --------------------------------------------------------------------------------------------- */
size_t vgposp_trsm_workspace_bytes(int64_t n, int64_t nrhs);
int vgposp_trsm_lower(const double* L, int64_t n, int64_t ldl, int trans, double* B, int64_t nrhs,
                      int64_t ldb, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * GP log marginal likelihood from the inverted factor.  Replaces
 * tfd.GaussianProcess(...).log_prob(y) (gp_functions.py:166-172, main.py:105):
 *     z = Minv y,   out[b] = -0.5 |z|^2 - sum_i log Ldiag[b][i] - n/2 log(2 pi)
 * Minv: output of vgposp_potrf_lower(invert=1); Ldiag: its diag_out; y: [n] (shared over batch).
 * alpha ([batch][n] or NULL) <- C^-1 y = Minv^T z.  ws: vgposp_lml_workspace_bytes(n, batch).
 * --------------------------------------------------------------------------------------------- */
size_t vgposp_lml_workspace_bytes(int64_t n, int batch);
int vgposp_lml(const double* Minv, int64_t n, int64_t lda, int64_t stride, int batch,
               const double* Ldiag, const double* y, double* alpha, double* out, void* ws,
               size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gradient of the LML w.r.t. (amp[b], ls[b], noise) for the kernel family `kind`:
 *     dLML/dtheta = 0.5 * sum_ij (alpha alpha^T - C^-1)_ij dC_ij/dtheta
 * Cinv: the full C^-1 (lower triangle suffices; formed by vgposp_gemm(transa=1, tri) from Minv).
 * grad: [batch][3] = (d/damp, d/dls, d/dnoise).  Replaces TF autodiff of
 * tf_train_gp_adam's loss (gp_functions.py:179-182).
 * --------------------------------------------------------------------------------------------- */
size_t vgposp_lml_grad_workspace_bytes(int64_t n, int batch);
int vgposp_lml_grad(int kind, const double* X, int64_t n, int d, const double* amp,
                    const double* ls, const double* Cinv, int64_t ldc, int64_t stride_c,
                    const double* alpha, int batch, double* grad, void* ws, size_t ws_bytes,
                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * Row sums of squares of a row-major strip V (rows x cols, ldv >= cols):
 *     out[i] = alpha * sum_j V[i][j]^2 + (beta != 0 ? beta * out[i] : 0),   0 <= i < rows
 * The marginal predictive variance without the P x P covariance: with V = K_*x L^-T one row per
 * prediction point, alpha = -1 and beta = 1 onto out = k(x*, x*) give the reference's
 * s2 = np.diag(K_ss) - np.sum(Lk**2, axis=0) (plot_confidence_interval.py:51; the stddev() of
 * main_GP_fit.py:251 and main_tests.py:404).  out is not read when beta == 0.  rows == 0 returns
 * 0 without device work; cols == 0 writes beta * out.  No workspace, no host synchronisation,
 * no atomics: column j always goes to the same lane, so two runs are bit-identical.
 * --------------------------------------------------------------------------------------------- */
int vgposp_row_sumsq(const double* V, int64_t rows, int64_t cols, int64_t ldv, double alpha,
                     double beta, double* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Greedy mutual-information placement (Krause, Singh & Guestrin Alg. 2 as implemented by
 * placement_algorithm2.placement_algorithm_2, placement_algorithm2.py:151-219; lazy = 0 gives
 * placement_algorithm_1, :128-145).  Same selections: delta_y = nom/denom with
 *   nom   = sigma_yy - Sigma_yA Sigma_AA^-1 Sigma_Ay                    (nominator, :371-388)
 *   denom = conditional variance of y given V \ (A u {y})               (denominator, :408-413)
 * zeroed when |nom| < 1e-8 or |denom| < 1e-8 (:198); the lazy cache starts at +inf and every
 * round re-scores the stale arg-max until the arg-max is fresh (:173-208); ties -> lowest index.
 *
 * Sigma: n x n row-major covariance (cov_vv) on device, lda >= n.  vgposp_greedy_init factors it
 * IN PLACE (lower triangle <- L^-1, diagonal saved in ws; the strictly upper triangle must hold
 * Sigma and is kept).  vgposp_greedy_step performs one selection round (round = 0, 1, ...).
 * selected: int64 [kmax] device; sel_delta: f64 [kmax] device (delta of each pick) or NULL;
 * info: int32 device (Cholesky status of init).  evals: int64 [kmax] device or NULL (number of
 * delta evaluations the reference would have made in each round).
 * Every vgposp_greedy_* entry reports a bad argument as "<its own name>: bad argument <the
 * argument's position in its own prototype>" and returns minus that position.
 * --------------------------------------------------------------------------------------------- */
size_t vgposp_greedy_workspace_bytes(int64_t n, int kmax);
int vgposp_greedy_init(double* Sigma, int64_t n, int64_t lda, int kmax, int* info, void* ws,
                       size_t ws_bytes, void* stream);
int vgposp_greedy_step(const double* Sigma, int64_t n, int64_t lda, int kmax, int round, int lazy,
                       int64_t* selected, double* sel_delta, int64_t* evals, void* ws,
                       size_t ws_bytes, void* stream);

/* The TF-graph variant snippets_a2.sparse_placement_algorithm_2 (snippets_a2.py:679-822, with
 * tf_nominator :138-213 and placement_algorithm2.sparse_argmax_cache_linear :24-50) differs only in
 * three constants, which vgposp_greedy_init_ex stores in the workspace for the later rounds:
 *   jitter      eps added to the diagonal of Sigma_AA and of Sigma_AbarAbar (snippets_a2.py:161-163:
 *               1e-6; 0 for placement_algorithm_2).  The factorization is of Sigma + eps I and
 *               denom_y = 1 / [(Sigma_SS + eps I)^-1]_yy - eps.
 *   threshold   |nom| or |denom| < threshold -> delta = 0 (:480: 1e-7; 1e-8 for alg. 2)
 *   cache_init  initial lazy-cache value (:690: INF = 1e8; +inf for alg. 2)
 * vgposp_greedy_init(...) == vgposp_greedy_init_ex(..., 0, 1e-8, +inf, ...).
 * After a failed pivot every later launch of init's factorization and inverse reads `info` on
 * the device and exits: a singular Sigma costs the factorization up to the failed pivot, not a
 * whole factor + inverse, before the caller's jitter retry (placement_algorithm2.py:399-413's
 * pinv has no failure mode) — without any host synchronisation, so init can be captured into a
 * graph.  Sigma and the workspace are then undefined, as after any failed factorization.
 * vgposp_greedy_cache returns the device pointer of the lazy cache [n] (delta_cached): the
 * per-round snapshot delta_cached_iters[:, r] of the TF variant is a copy of it after round r. */
int vgposp_greedy_init_ex(double* Sigma, int64_t n, int64_t lda, int kmax, double jitter,
                          double threshold, double cache_init, int* info, void* ws,
                          size_t ws_bytes, void* stream);
int vgposp_greedy_cache(void* ws, int64_t n, int kmax, double** cache);
/* Mark candidate idx as never selectable (after init: it is never scored, never an arg-max,
 * never counted in evals).  placement_algorithm2 factors an odd-order cov_vv as
 * [Sigma 0; 0 s] at the even order n + 1 (the fast GEMM needs even leading dimensions; the leading
 * block's factor and inverse are unchanged and the padding couples to nothing) and excludes the
 * padding candidate with this. */
int vgposp_greedy_exclude(void* ws, int64_t n, int kmax, int64_t idx, void* stream);

/* A candidate set and pre-installed sensors: Krause's split of V into S (where a sensor may go) and
 * U (whose uncertainty counts, but where none can be put), and a greedy loop that starts from
 * sensors A0 already in place.  The reference assumes both away ("assume U is empty, assume
 * V = S", A = [], placement_algorithm2.py:128-160); here A starts as A0 (in the given order),
 * A_bar as V \ A0, and the arg-max loops (argmax_cache_linear :53-67, argmax_ :105-125) run over
 * candidates \ A.  nominator (:371-388) and denominator (:408-413) are unchanged, so A_bar keeps
 * every non-candidate location.
 *   vgposp_greedy_mask   after init: selmask[i] |= !allowed[i] for a device byte mask allowed[n]
 *                        (the set form of vgposp_greedy_exclude).
 *   vgposp_greedy_force  a selection round whose pick is given: y = forced[j] (device array, so
 *                        nothing synchronises the host) instead of the arg-max; writes
 *                        selected[round], the selection mask and the pivot data exactly as
 *                        vgposp_greedy_select does after choosing (A.append(y), :211) and leaves
 *                        the cache, the fresh flags and evals alone.  It counts towards kmax.
 *   vgposp_greedy_condition  right after init: rounds 0 .. m-1 as forced rounds on
 *                        placed[0 .. m), with the workspace sized for kmax >= m + k rounds; the k
 *                        free rounds then continue with vgposp_greedy_step(round = m, ...), which
 *                        conditions on placed[m-1] itself.  batch = 1 runs one vgposp_greedy_update
 *                        per sensor (one pass over L^-1 each); batch = 4 or 8 forms the columns
 *                        q_a = M^T (M e_a) of that many sensors in ONE pass over L^-1 (they do not
 *                        depend on each other; only the O(n t) Gram-Schmidt of the update is
 *                        sequential).  scratch: vgposp_greedy_condition_workspace_bytes(n, batch)
 *                        bytes (0 for an unsupported batch), separate from the greedy workspace.
 * Index range and duplicates in placed are the caller's to check before upload. */
int vgposp_greedy_mask(void* ws, int64_t n, int kmax, const unsigned char* allowed, void* stream);
int vgposp_greedy_force(int64_t n, int kmax, int round, const int64_t* forced, int64_t j,
                        int64_t* selected, void* ws, size_t ws_bytes, void* stream);
size_t vgposp_greedy_condition_workspace_bytes(int64_t n, int batch);
int vgposp_greedy_condition(const double* Sigma, int64_t n, int64_t lda, int kmax, int m, int k,
                            int batch, const int64_t* placed, int64_t* selected, void* ws,
                            size_t ws_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* Speculative mat-vec of vgposp_greedy_step.  q_a = M^T (M e_a) depends on M = L^-1 and a alone,
 * so a pass over L^-1 can carry, beside the pick's column, the columns the next rounds will
 * probably ask for, and a round whose pick is already cached reads nothing of L^-1.
 *   vgposp_greedy_set_speculation(width)  process-wide; width 1, 2, 4 or 8 columns per pass
 *        (anything else: -1).  Width 1 makes exactly the launches of a library without the
 *        feature.  vgposp_greedy_speculation() returns the current width.
 *   The guarantee: every output of every round (selected, sel_delta, evals, and the whole state
 *        in the workspace) is bit for bit the same at every width.  The multi-column kernel and
 *        the single-column one compile from one source of the row loop, a cached column is summed
 *        in the order the update would sum it, and the prediction (the largest fresh deltas of
 *        the previous round among the unselected, unmasked, not yet cached candidates) decides
 *        speed only.  Everything is decided on the device: a round is the same launch sequence
 *        on a hit and on a miss, with no synchronisation, so the rounds stay capturable.
 *   Only vgposp_greedy_step at rounds >= 1 speculates; vgposp_greedy_update(_ex), _extract, the
 *        slab entry points and vgposp_greedy_condition are as before.  vgposp_greedy_init(_ex),
 *        _prepare, _init_slab and _finish_slab clear the cache; vgposp_greedy_workspace_bytes is
 *        sized for width 8 whatever the current width.
 *   vgposp_greedy_spec_stats  reads the counters of the workspace's current run (synchronous copy;
 *        call it after the stream has been synchronised): passes over L^-1 made by speculating
 *        rounds, rounds served from the cache, columns cached.  Each pointer may be NULL.
 *   vgposp_greedy_spec_table  device pointers of the table: column[s] is the candidate whose q
 *        sits in slot s, fill_round[s] the round whose pass formed it (s < cached); *slots is
 *        the capacity (4 kmax; a full table ends the speculation, nothing is evicted). */
int vgposp_greedy_set_speculation(int width);
int vgposp_greedy_speculation(void);
int vgposp_greedy_spec_stats(void* ws, int64_t n, int kmax, int64_t* passes, int64_t* hits,
                             int64_t* cached);
int vgposp_greedy_spec_table(void* ws, int64_t n, int kmax, int64_t** column,
                             int64_t** fill_round, int64_t* slots);

/* Placement algorithm 3, the local-kernel greedy (snippets_a3.sparse_placement_algorithm_3,
 * snippets_a3.py:43-330; with vgposp_greedy_init_ex(..., 1e-6, 1e-7, 1e8, ...) as its tf_nominator
 * constants).  Per round, after vgposp_greedy_update(round): round 0 scores every candidate into
 * the cache; round r >= 1 refreshes the cache only for candidates in the index window
 * [i_d - cutoff, i_d + cutoff) (per grid axis d, clipped, upper bound exclusive) around the
 * previous pick y* = selected[r-1] of the I0 x I1 x I2 C-order grid (candidates in A -> 0,
 * cache[y*] = 0); entries outside the window keep their stale values.  Then selects the arg-max of
 * the cache over the unselected candidates (lowest index on ties).  sel_delta[r] = cache[y];
 * evals[r] = entries scored this round. */
int vgposp_greedy_select_window(int64_t n, int kmax, int round, int64_t I0, int64_t I1, int64_t I2,
                                int cutoff, int64_t c0, int64_t c1, int64_t* selected,
                                double* sel_delta, int64_t* evals, void* ws, size_t ws_bytes,
                                void* stream);

/* The two phases of vgposp_greedy_step, for candidate-sharded multi-GPU placement:
 * every rank holds the factored Sigma (replicated init) and owns the candidate slab [c0, c1).
 *   vgposp_greedy_update: rank-1 updates of nom / P_yy and fresh deltas for y in [c0, c1) only
 *                         (the triangular mat-vec reads only the slab's columns of L^-1).
 *   -> caller all-gathers the delta slabs into the full delta vector (vgposp_greedy_buffers)
 *   vgposp_greedy_select: lazy-cache emulation over ALL candidates (identical on every rank) and
 *                         the pivot row of the pick, written only by the rank whose slab owns it
 *                         (zeros elsewhere)
 *   -> caller sum-all-reduces the pivot buffer (2 + 2*kmax doubles) before the next update.
 * With c0 = 0, c1 = n and no collectives this is exactly vgposp_greedy_step. */
int vgposp_greedy_update(const double* Sigma, int64_t n, int64_t lda, int kmax, int round,
                         int64_t c0, int64_t c1, const int64_t* selected, void* ws,
                         size_t ws_bytes, void* stream);
int vgposp_greedy_select(int64_t n, int kmax, int round, int lazy, int64_t c0, int64_t c1,
                         int64_t* selected, double* sel_delta, int64_t* evals, void* ws,
                         size_t ws_bytes, void* stream);
/* Partitioned inverse for one problem sharded over R ranks (the O(N^3) factorization is replicated,
 * the inverse is not): vgposp_greedy_init_slab factors Sigma like vgposp_greedy_init_ex but forms
 * L^-1 only in columns [c0, c1) (the rank's candidate slab; c0 and c1 multiples of 128 or c1 = n),
 * about 1/R of the inverse's flops; tmp: vgposp_greedy_slab_tmp_bytes(n, c0, c1) bytes.  Per round
 * the owner of the last pick's column then provides it: vgposp_greedy_extract writes xcol = that
 * column of L^-1 if the pick is in [own0, own1) and zeros otherwise, the caller sum-all-reduces
 * xcol (vgposp_greedy_xcol gives its device address) and runs vgposp_greedy_update_ex with
 * extract = 0.  vgposp_greedy_update(...) == vgposp_greedy_update_ex(..., extract = 1, ...). */
size_t vgposp_greedy_slab_tmp_bytes(int64_t n, int64_t c0, int64_t c1);
int vgposp_greedy_init_slab(double* Sigma, int64_t n, int64_t lda, int kmax, double jitter,
                            double threshold, double cache_init, int64_t c0, int64_t c1,
                            double* tmp, size_t tmp_bytes, int* info, void* ws, size_t ws_bytes,
                            void* stream);
/* vgposp_greedy_init_slab in phases, for a factorization the caller runs itself (the distributed
 * Cholesky above): vgposp_greedy_prepare (saves diag(Sigma), jitter, cache init, info = 0), then the
 * lower factor of Sigma in place with the potrf workspace vgposp_greedy_fact_ws returns, then
 * vgposp_greedy_finish_slab (L^-1 in columns [c0, c1) and their column norms). */
int vgposp_greedy_prepare(double* Sigma, int64_t n, int64_t lda, int kmax, double jitter,
                          double threshold, double cache_init, int* info, void* ws,
                          size_t ws_bytes, void* stream);
int vgposp_greedy_fact_ws(void* ws, int64_t n, int kmax, void** fws, size_t* fws_bytes);
int vgposp_greedy_finish_slab(double* Sigma, int64_t n, int64_t lda, int kmax, int64_t c0,
                              int64_t c1, double* tmp, size_t tmp_bytes, void* ws,
                              size_t ws_bytes, void* stream);
int vgposp_greedy_extract(const double* Sigma, int64_t n, int64_t lda, int kmax, int round,
                          int64_t own0, int64_t own1, const int64_t* selected, void* ws,
                          size_t ws_bytes, void* stream);
int vgposp_greedy_update_ex(const double* Sigma, int64_t n, int64_t lda, int kmax, int round,
                            int64_t c0, int64_t c1, const int64_t* selected, int extract, void* ws,
                            size_t ws_bytes, void* stream);
int vgposp_greedy_xcol(void* ws, int64_t n, int kmax, double** xcol);
/* Device pointers into the workspace: the full delta vector [n] and the pivot buffer. */
int vgposp_greedy_buffers(void* ws, int64_t n, int kmax, double** delta, double** piv,
                          int64_t* piv_len);

/* ---------------------------------------------------------------------------------------------
 * Greedy placement by variance reduction (A-optimal) and by entropy: the two baselines Krause,
 * Singh & Guestrin judge the mutual-information placement against.  Sigma = cov_vv (n x n,
 * symmetric PSD), A the sensors chosen so far (pre-installed ones first),
 *   C = Sigma - Sigma_{:,A} Sigma_AA^-1 Sigma_{A,:}       the conditional covariance given A.
 *   VGPOSP_CRIT_VARIANCE  delta_y = sum_{v in T} C_vy^2 / C_yy, which is tr_T(C) - tr_T(C after
 *                         adding y): the deltas of a run sum to the total reduction of the
 *                         targets' posterior variance.  T: the targets (default: every location).
 *   VGPOSP_CRIT_ENTROPY   delta_y = C_yy (the largest conditional variance).
 * C_yy < threshold gives delta_y = 0 under both rules.  The arg-max runs over S \ A (S: the
 * candidates, default every location; T need not intersect S); ties go to the lowest index.
 * Every round scores every free candidate: no lazy cache, the variance rule is not submodular.
 * Nothing is factored, so a singular PSD Sigma needs no jitter.  The state is nom_y = C_yy,
 * score_y = sum_{v in T} C_vy^2 and the rows W of the pivoted Cholesky of Sigma given A
 * (C = Sigma - W^T W); with a the pick, t the 0/1 target mask and w.t the element-wise product a
 * round does
 *   w_y      = (Sigma_ay - sum_u W_u[a] W_u[y]) / sqrt(nom_a)        (0 when nom_a < threshold)
 *   g        = Sigma (w.t) - W^T (W (w.t))                           (the one pass over Sigma)
 *   score_y -= 2 w_y g_y - w_y^2 |w.t|^2,     nom_y -= w_y^2
 * from score_y = sum_{v in T} Sigma_vy^2, nom = diag Sigma; entropy keeps nom and W only and never
 * passes over Sigma.
 *
 * Only the entries j >= i of Sigma are read, Sigma is never written, and a non-NULL diag[n]
 * replaces its diagonal: exactly what a buffer factored in place by vgposp_greedy_init still holds
 * (Sigma strictly above the diagonal, L^-1 below it) plus the diagonal the caller saved, so both
 * rules run on the MI path's buffer without a second copy of Sigma.
 *
 *   vgposp_symv_upper     y = A x for a symmetric row-major A of which only the entries j >= i are
 *                         read (diag as above), lda >= n.  Every element of the triangle is loaded
 *                         once per launch and serves y_i and y_j; 16-byte non-temporal loads when
 *                         lda is even and A is 16-byte aligned, 8-byte loads otherwise.  No float
 *                         atomics: per-tile partial sums go to ws
 *                         (vgposp_symv_upper_workspace_bytes(n) bytes; 0 for n <= 0) and are
 *                         reduced in a fixed order, so two runs are bit-identical.  No host
 *                         synchronisation.  n == 0 returns 0 without device work.
 *   vgposp_symv_upper_sq  the same pass with every entry squared: y_j = sum_i x_i A_ij^2 (the
 *                         initial score for x = t).
 *   vgposp_crit_init      nom, score (variance rule: one vgposp_symv_upper_sq pass), the masks.
 *                         targets / allowed: device byte masks [n] or NULL (= all ones).
 *   vgposp_crit_step      one round: delta for every location, the arg-max over the free
 *                         candidates — or forced[j] (device array) when forced is non-NULL, as
 *                         vgposp_greedy_force —, selected[round] and sel_delta[round] (NULL: not
 *                         written) = delta of the pick, then the updates above.  Rounds run 0, 1,
 *                         ... < kmax; with no candidate left selected[round] = -1 and the state is
 *                         left alone.  The criterion lives in the workspace: a round is the same
 *                         launch sequence under both rules.
 *   vgposp_crit_buffers   device pointers into the workspace (each may be NULL): nom [n],
 *                         score [n], delta [n] (as scored by the last round, before its pick) and
 *                         W [kmax][n] (row r written by round r).
 * Argument errors return -(position) before any device work. */
#define VGPOSP_CRIT_VARIANCE 0
#define VGPOSP_CRIT_ENTROPY 1
size_t vgposp_symv_upper_workspace_bytes(int64_t n);
int vgposp_symv_upper(const double* A, int64_t n, int64_t lda, const double* diag,
                      const double* x, double* y, void* ws, size_t ws_bytes, void* stream);
int vgposp_symv_upper_sq(const double* A, int64_t n, int64_t lda, const double* diag,
                         const double* x, double* y, void* ws, size_t ws_bytes, void* stream);
size_t vgposp_crit_workspace_bytes(int64_t n, int kmax);
int vgposp_crit_init(const double* Sigma, int64_t n, int64_t lda, const double* diag, int kmax,
                     int criterion, double threshold, const unsigned char* targets,
                     const unsigned char* allowed, void* ws, size_t ws_bytes, void* stream);
int vgposp_crit_step(const double* Sigma, int64_t n, int64_t lda, const double* diag, int kmax,
                     int round, const int64_t* forced, int64_t j, int64_t* selected,
                     double* sel_delta, void* ws, size_t ws_bytes, void* stream);
int vgposp_crit_buffers(void* ws, int64_t n, int kmax, double** nom, double** score,
                        double** delta, double** W);

/* ---------------------------------------------------------------------------------------------
 * The variance rule for targets outside V: sensors go on the n locations of Sigma, the field is
 * judged at P targets that are no rows of Sigma (a finer mesh, the latent field without sensor
 * noise).  R = cross_cov (P x n, row-major fp64, row pitch ldr >= n, only read) is the covariance
 * between the targets and the locations, omega [P] >= 0 the targets' weights (NULL: all ones),
 *   D = R - R_{:,A} Sigma_AA^-1 Sigma_{A,:},     delta_y = sum_v omega_v D_vy^2 / C_yy:
 * the drop of the weighted total posterior variance of the targets when y is added.  Threshold,
 * candidate mask, forced rounds, ties and "no candidate left -> -1" are those of
 * vgposp_crit_step.  The state is nom, score, W as above and the target-side rows U [kmax][P]
 * (D = R - U^T W); with a the pick a round does
 *   w_y      as above
 *   u_v      = (R_va - sum_t U_t[v] W_t[a]) / sqrt(nom_a)            (0 when nom_a < threshold)
 *   g        = R^T (omega.u) - W^T (U (omega.u))                     (the one pass over R)
 *   score_y -= 2 w_y g_y - w_y^2 sum_v omega_v u_v^2,     nom_y -= w_y^2
 * from score_y = sum_v omega_v R_vy^2, nom = diag Sigma.  sum_r U_r[v]^2 is the variance removed
 * at target v.  Nothing is factored, so a singular joint covariance works.
 *
 *   vgposp_gemv_t         y_j = sum_v x_v R_vj for a P x n row-major R, ldr >= n: a pure stream of
 *                         8 P n bytes, 16-byte non-temporal loads when ldr is even and R is
 *                         16-byte aligned, 8-byte loads otherwise.  No float atomics: one partial
 *                         per (512-row tile, column) goes to ws
 *                         (vgposp_gemv_t_workspace_bytes(P, n) bytes; 0 when P <= 0 or n <= 0) and
 *                         the partials are added in ascending row-tile order, so two runs are
 *                         bit-identical.  No host synchronisation.  P == 0 or n == 0 returns 0
 *                         without device work.
 *   vgposp_gemv_t_sq      the same pass with every entry squared: y_j = sum_v x_v R_vj^2.
 *   vgposp_critx_init     nom, omega, score (one vgposp_gemv_t_sq pass), the candidate mask.
 *   vgposp_critx_step     one round, as vgposp_crit_step.
 *   vgposp_critx_buffers  device pointers into the workspace (each may be NULL): nom, score,
 *                         delta [n], W [kmax][n], U [kmax][P] (row r written by round r).
 * Argument errors return -(position) before any device work. */
size_t vgposp_gemv_t_workspace_bytes(int64_t P, int64_t n);
int vgposp_gemv_t(const double* R, int64_t P, int64_t n, int64_t ldr, const double* x, double* y,
                  void* ws, size_t ws_bytes, void* stream);
int vgposp_gemv_t_sq(const double* R, int64_t P, int64_t n, int64_t ldr, const double* x,
                     double* y, void* ws, size_t ws_bytes, void* stream);
size_t vgposp_critx_workspace_bytes(int64_t n, int64_t P, int kmax);
int vgposp_critx_init(const double* Sigma, int64_t n, int64_t lda, const double* diag,
                      const double* R, int64_t P, int64_t ldr, const double* weights, int kmax,
                      double threshold, const unsigned char* allowed, void* ws, size_t ws_bytes,
                      void* stream);
int vgposp_critx_step(const double* Sigma, int64_t n, int64_t lda, const double* diag,
                      const double* R, int64_t P, int64_t ldr, int kmax, int round,
                      const int64_t* forced, int64_t j, int64_t* selected, double* sel_delta,
                      void* ws, size_t ws_bytes, void* stream);
int vgposp_critx_buffers(void* ws, int64_t n, int64_t P, int kmax, double** nom, double** score,
                         double** delta, double** W, double** U);

/* ---------------------------------------------------------------------------------------------
 * The same rule on a cross-covariance that is never stored: R = diag(a_t) K(Xt, X) diag(a_s) is
 * generated from the points in every pass.  Xt [P][d] (targets) and X [n][d] (locations) are
 * row-major fp64, 1 <= d <= 8; kind, amp and ls (device [1]) as in vgposp_kernel_matvec;
 * target_scale a_t [P] and site_scale a_s [n] (NULL: ones) are a per-point amplitude field.  The
 * device holds (P + n) d doubles instead of P n.  Limits: P <= 2^24, n <= 2^21.
 *
 *   vgposp_kernel_gemv_t     y_j = a_s[j] sum_v x_v a_t[v] k(Xt_v, X_j): vgposp_gemv_t with the
 *                            load of R_vj replaced by its evaluation (it replaces
 *                            vgposp_kernel_matvec(X, Xt, x) for this shape: that one parallelises
 *                            over its n output rows alone).  A 2-D grid of (512-column tile,
 *                            VGPOSP_KGEMV_ROWS-target chunk) workgroups; one partial per (chunk,
 *                            column) goes to ws (vgposp_kernel_gemv_t_workspace_bytes(P, n) bytes;
 *                            0 when P <= 0 or n <= 0), the partials are added in ascending chunk
 *                            order.  No float atomics, two runs are bit-identical, no host
 *                            synchronisation.  P == 0 or n == 0 returns 0 without device work.
 *   vgposp_kernel_gemv_t_sq  every generated entry squared (replaces vgposp_gemv_t_sq):
 *                            y_j = a_s[j]^2 sum_v x_v a_t[v]^2 k(Xt_v, X_j)^2.
 *   vgposp_critk_workspace_bytes / _init / _step / _buffers
 *                            vgposp_critx_* with (R, P, ldr) replaced by (kind, Xt, P, X, d, amp,
 *                            ls, target_scale, site_scale): the same launch sequence, the column
 *                            R_{:,a} of a round and the pass generated by one device function.
 * Argument errors return -(position) before any device work. */
#define VGPOSP_KGEMV_ROWS 512
size_t vgposp_kernel_gemv_t_workspace_bytes(int64_t P, int64_t n);
int vgposp_kernel_gemv_t(int kind, const double* Xt, int64_t P, const double* X, int64_t n, int d,
                         const double* amp, const double* ls, const double* target_scale,
                         const double* site_scale, const double* x, double* y, void* ws,
                         size_t ws_bytes, void* stream);
int vgposp_kernel_gemv_t_sq(int kind, const double* Xt, int64_t P, const double* X, int64_t n,
                            int d, const double* amp, const double* ls, const double* target_scale,
                            const double* site_scale, const double* x, double* y, void* ws,
                            size_t ws_bytes, void* stream);
size_t vgposp_critk_workspace_bytes(int64_t n, int64_t P, int kmax);
int vgposp_critk_init(const double* Sigma, int64_t n, int64_t lda, const double* diag, int kind,
                      const double* Xt, int64_t P, const double* X, int d, const double* amp,
                      const double* ls, const double* target_scale, const double* site_scale,
                      const double* weights, int kmax, double threshold,
                      const unsigned char* allowed, void* ws, size_t ws_bytes, void* stream);
int vgposp_critk_step(const double* Sigma, int64_t n, int64_t lda, const double* diag, int kind,
                      const double* Xt, int64_t P, const double* X, int d, const double* amp,
                      const double* ls, const double* target_scale, const double* site_scale,
                      int kmax, int round, const int64_t* forced, int64_t j, int64_t* selected,
                      double* sel_delta, void* ws, size_t ws_bytes, void* stream);
int vgposp_critk_buffers(void* ws, int64_t n, int64_t P, int kmax, double** nom, double** score,
                         double** delta, double** W, double** U);

/* ---------------------------------------------------------------------------------------------
 * The rules on a covariance that is never stored: Sigma = diag(a) K(X, X) diag(a) + a diagonal,
 * generated from the points.  X [n][d] row-major fp64, 1 <= d <= 8; kind, amp, ls (device [1]) as
 * above; site_scale a [n] (NULL: ones).  Sigma_ij = a_i a_j k(X_i, X_j) for i != j; Sigma_ii =
 * diag[i] when diag [n] is given (noise, jitter), else a_i^2 amp^2.  The device holds n (d + 2)
 * doubles instead of n^2.  Limit: n <= 2^21.
 *
 *   vgposp_kernel_symv       y = Sigma x.  Every off-diagonal entry whose row and column lie in
 *                            different 512-tiles is evaluated once and serves y_i and y_j (the
 *                            diagonal tiles are evaluated as full squares: n 512 entries more).  A
 *                            workgroup owns a block of G x G tiles on or above the diagonal
 *                            (G = 1 .. 8 by n, 8 from n = 229,377 on); one partial per (row
 *                            group, column) and per (column group, row) goes to ws, added in
 *                            ascending group order.  vgposp_kernel_symv_workspace_bytes(n) (0 when
 *                            n <= 0) is at most 16 n max(ceil(n / 4096), min(ceil(n / 512), 64))
 *                            bytes plus alignment: 0.27 GB at n = 262,144.  No float atomics, two
 *                            launches are bit-identical, no host synchronisation.  n == 0 returns
 *                            0 without device work.
 *   vgposp_kernel_symv_sq    y_j = sum_i x_i Sigma_ij^2.
 *   vgposp_critg_workspace_bytes / _init / _step / _buffers
 *                            vgposp_crit_* with (Sigma, n, lda, diag) replaced by (kind, X, n, d,
 *                            amp, ls, site_scale, diag): the same launch sequence, the column
 *                            Sigma_{:,a} of a round and the pass generated by one device function.
 *                            Under the entropy rule nothing but that column is ever evaluated.
 *   vgposp_critgk_workspace_bytes / _init / _step / _buffers
 *                            vgposp_critk_* with (Sigma, n, lda, diag) replaced by (n, diag): the
 *                            off-diagonal entries of Sigma come from the kind, X, d, amp, ls and
 *                            site_scale that generate R, so nothing of size n^2 or P n is held.
 * Argument errors return -(position) before any device work. */
size_t vgposp_kernel_symv_workspace_bytes(int64_t n);
int vgposp_kernel_symv(int kind, const double* X, int64_t n, int d, const double* amp,
                       const double* ls, const double* site_scale, const double* diag,
                       const double* x, double* y, void* ws, size_t ws_bytes, void* stream);
int vgposp_kernel_symv_sq(int kind, const double* X, int64_t n, int d, const double* amp,
                          const double* ls, const double* site_scale, const double* diag,
                          const double* x, double* y, void* ws, size_t ws_bytes, void* stream);
size_t vgposp_critg_workspace_bytes(int64_t n, int kmax);
int vgposp_critg_init(int kind, const double* X, int64_t n, int d, const double* amp,
                      const double* ls, const double* site_scale, const double* diag, int kmax,
                      int criterion, double threshold, const unsigned char* targets,
                      const unsigned char* allowed, void* ws, size_t ws_bytes, void* stream);
int vgposp_critg_step(int kind, const double* X, int64_t n, int d, const double* amp,
                      const double* ls, const double* site_scale, const double* diag, int kmax,
                      int round, const int64_t* forced, int64_t j, int64_t* selected,
                      double* sel_delta, void* ws, size_t ws_bytes, void* stream);
int vgposp_critg_buffers(void* ws, int64_t n, int kmax, double** nom, double** score,
                         double** delta, double** W);
size_t vgposp_critgk_workspace_bytes(int64_t n, int64_t P, int kmax);
int vgposp_critgk_init(int64_t n, const double* diag, int kind, const double* Xt, int64_t P,
                       const double* X, int d, const double* amp, const double* ls,
                       const double* target_scale, const double* site_scale,
                       const double* weights, int kmax, double threshold,
                       const unsigned char* allowed, void* ws, size_t ws_bytes, void* stream);
int vgposp_critgk_step(int64_t n, const double* diag, int kind, const double* Xt, int64_t P,
                       const double* X, int d, const double* amp, const double* ls,
                       const double* target_scale, const double* site_scale, int kmax, int round,
                       const int64_t* forced, int64_t j, int64_t* selected, double* sel_delta,
                       void* ws, size_t ws_bytes, void* stream);
int vgposp_critgk_buffers(void* ws, int64_t n, int64_t P, int kmax, double** nom, double** score,
                          double** delta, double** W, double** U);

/* ---------------------------------------------------------------------------------------------
 * The rules on a covariance given by a factor: Sigma = F F^T + diag(noise).  This is the
 * reference's own placement covariance, the empirical covariance of S tracer samples per location
 * (tfp.stats.covariance(t_i, t_j, sample_axis=0) for every pair, main.py:190-199; the VGP-predicted
 * variant, main_architecture_2_sampledistribution.py:470-479), with F = the centred samples over
 * tr_stdev sqrt(S) (vgposp_center_rows); any low-rank-plus-diagonal covariance has the same form.
 * F [n][s] row-major fp64, row pitch ldf >= s, only read; noise [n] >= 0 or NULL (zeros).
 *   Sigma_ij = f_i . f_j (i != j),    Sigma_ii = dg_i = f_i . f_i + noise_i
 * dg is computed once (the kernel of vgposp_row_sumsq) and kept in the workspace.  The device holds
 * n s doubles instead of n^2.  Limits: 1 <= s <= 4,096; n <= 2^22 for the passes and n <= 2^21 for
 * the rounds, whose scoring and selection kernels are those of vgposp_crit_step.
 *
 *   vgposp_factor_symv     y = Sigma x as z = F^T x, y_i = f_i . z + noise_i x_i: two streams over
 *                          F, 16 n s bytes.  A workgroup of the first owns a block of rows, read
 *                          with 16-byte loads when ldf is even and F is 16-byte aligned (8-byte
 *                          loads otherwise), and writes one partial z to ws; the partials are added
 *                          in ascending block order.  In the second a wave takes whole rows, z is
 *                          broadcast through LDS and the order over s is fixed.  No float atomics,
 *                          two launches are bit-identical, no host synchronisation.  n == 0 returns
 *                          0 without device work.
 *   vgposp_factor_symv_sq  y_j = sum_i x_i Sigma_ij^2 through the s x s moment matrix
 *                          M = F^T diag(x) F:  y_j = f_j^T M f_j - x_j (f_j . f_j)^2 + x_j dg_j^2.
 *                          M and F M run in row chunks through vgposp_gemm's kernels: O(n s^2).
 *   vgposp_factor_symv_workspace_bytes(n, s): at most 8 (s^2 + 16,384 s) + 8 n bytes plus
 *                          alignment; 0 when n <= 0 or s <= 0.
 *   vgposp_critf_workspace_bytes / _init / _step / _buffers
 *                          vgposp_crit_* with (Sigma, n, lda, diag) replaced by (F, n, s, ldf,
 *                          noise): the same launch sequence; the column Sigma_{:,a} of a round is
 *                          f_y . f_a, with dg_a at y = a.  Threshold, candidate mask, forced rounds,
 *                          ties and "no candidate left -> -1" are those of vgposp_crit_step.  The
 *                          workspace query returns 0 when n <= 0, s <= 0 or kmax <= 0.
 * Argument errors return -(position) before any device work. */
size_t vgposp_factor_symv_workspace_bytes(int64_t n, int64_t s);
int vgposp_factor_symv(const double* F, int64_t n, int64_t s, int64_t ldf, const double* noise,
                       const double* x, double* y, void* ws, size_t ws_bytes, void* stream);
int vgposp_factor_symv_sq(const double* F, int64_t n, int64_t s, int64_t ldf, const double* noise,
                          const double* x, double* y, void* ws, size_t ws_bytes, void* stream);
size_t vgposp_critf_workspace_bytes(int64_t n, int64_t s, int kmax);
int vgposp_critf_init(const double* F, int64_t n, int64_t s, int64_t ldf, const double* noise,
                      int kmax, int criterion, double threshold, const unsigned char* targets,
                      const unsigned char* allowed, void* ws, size_t ws_bytes, void* stream);
int vgposp_critf_step(const double* F, int64_t n, int64_t s, int64_t ldf, const double* noise,
                      int kmax, int round, const int64_t* forced, int64_t j, int64_t* selected,
                      double* sel_delta, void* ws, size_t ws_bytes, void* stream);
int vgposp_critf_buffers(void* ws, int64_t n, int64_t s, int kmax, double** nom, double** score,
                         double** delta, double** W);

/* ---------------------------------------------------------------------------------------------
 * Mutual-information placement on a factored covariance Sigma = F F^T + D, D = diag(noise) with
 * noise_i > 0 at EVERY location (D must be invertible): the reference's own criterion, the full
 * greedy of placement_algorithm2.py:128-145 with the deltas of :371-413, on the reference's own
 * covariance (main.py:190-199), at site counts where neither Sigma nor its inverse can be stored.
 * Woodbury:
 *   Q = Sigma^-1 = D^-1 - D^-1 F C^-1 F^T D^-1,   C = I_s + F^T D^-1 F   (s x s, SPD, lambda_min >= 1)
 * With C = L L^T and M = L^-1 (vgposp_potrf_lower's recursion, invert = 1) the rounds of
 * vgposp_greedy_step read three closed forms on F:
 *   Q_yy = 1 / d_y - |M f_y|^2 / d_y^2                    once, O(n s^2) through vgposp_gemm's kernels
 *   column a of Sigma:  s_i = f_i . f_a, dg_a at i = a
 *   column a of Q:      q_i = [i = a] / d_a - (f_i . u_a) / d_i,   u_a = C^-1 f_a / d_a
 * and then do greedy_update_kernel's arithmetic with jitter 0: s and q downdated by the earlier
 * rows of W and V through the pick's pivots, w = s / sqrt(nom_a) (0 unless nom_a >= threshold and
 * > 0), v = q / sqrt(prec_a) (0 unless prec_a > 0), nom -= w^2, prec -= v^2, and
 * delta = nom / (1 / prec), 0 where |nom| or |1 / prec| is below the threshold.
 * Selection: the arg-max over the FRESH delta of every free candidate, ties to the lower index
 * (the full greedy, vgposp_greedy_step with lazy = 0).  The lazy cache of vgposp_greedy_step, its
 * default, exists to save evaluations; here every delta is fresh after the one stream over F a
 * round needs anyway, so it is not emulated and there is no `evals`.  Masked locations (`allowed`)
 * are never picked and stay in every denominator; forced rounds as in vgposp_crit_step; no
 * candidate left -> selected[round] = -1 and the round changes nothing.
 *   vgposp_fmi_init   dg, C (the moment-matrix loop of vgposp_factor_symv_sq with x = 1 / d),
 *                     M, C^-1 = M^T M, prec = Q_yy, nom = dg, the masks.  info (device int32):
 *                     the factorization's status, 0 whenever d > 0.
 *   vgposp_fmi_step   four launches: score, select (+ the pick's pivots), u_a (a wave per row of
 *                     C^-1, fixed order), and one stream over F that forms f_i . f_a and f_i . u_a
 *                     from a single read of each row (16-byte loads when ldf is even and F is
 *                     16-byte aligned, else 8-byte) and applies both downdates: 8 n s +
 *                     8 n (2 round + 6) bytes.  No float atomics, two runs are bit-identical, no
 *                     host synchronisation.
 *   vgposp_fmi_buffers  device pointers into ws, each output optional: nom [n], prec [n],
 *                     delta [n] (as scored by the last round, before its pick), W and V
 *                     [kmax][n].
 *   vgposp_fmi_workspace_bytes(n, s, kmax): 2 kmax n + O(n) + 2 s^2 doubles, the chunk area of
 *                     vgposp_factor_symv_workspace_bytes and the s x s factorization's
 *                     workspace; 0 when n <= 0, s <= 0 or kmax <= 0.
 * Limits and argument groups are those of vgposp_critf_*: 1 <= s <= 4,096, n <= 2^21, ldf >= s,
 * 1 <= kmax <= n; noise must not be NULL.  Argument errors return -(position) before any device
 * work, a short workspace VGPOSP_E_WS. */
size_t vgposp_fmi_workspace_bytes(int64_t n, int64_t s, int kmax);
int vgposp_fmi_init(const double* F, int64_t n, int64_t s, int64_t ldf, const double* noise,
                    int kmax, double threshold, const unsigned char* allowed, int* info,
                    void* ws, size_t ws_bytes, void* stream);
int vgposp_fmi_step(const double* F, int64_t n, int64_t s, int64_t ldf, const double* noise,
                    int kmax, int round, const int64_t* forced, int64_t j, int64_t* selected,
                    double* sel_delta, void* ws, size_t ws_bytes, void* stream);
int vgposp_fmi_buffers(void* ws, int64_t n, int64_t s, int kmax, double** nom, double** prec,
                       double** delta, double** W, double** V);

/* ---------------------------------------------------------------------------------------------
 * Field reconstruction from k placed sensors on a factored covariance Sigma = F F^T + D: the
 * posterior mean at all n sites from the sensors' readings and the variance that is left, on the
 * reference's own covariance (main.py:190-199) without Sigma, Sigma_VA or any n x k array.
 * A = `sensors` (k distinct sites, pos(a) the position of a in it), sigma2 = obs_noise >= 0 a scalar
 * measurement-error variance on the sensors' own covariance only, dg_i = f_i . f_i + d_i:
 *   G = F_A F_A^T + diag(d_A + sigma2) = L L^T   (k x k),   M = L^-1
 *   c_i = F_A f_i + [i in A] d_i e_pos(i)
 *   var_i = dg_i - |M c_i|^2,   mean_i,b = mu_i + c_i . alpha_b,   alpha = G^-1 (Y - mu_A)
 * With W = M F_A (k x s) and Z = F_A^T alpha (s x nrhs) a site outside A needs the row
 * f_i . [W^T | Z] alone; the k sensor rows take the term in d_a from a second, small launch.
 *   vgposp_fpost_init   (main.py:190-199 conditioned on the picks of placement_algorithm2.py:
 *                     128-145) dg, the gathered F_A and d_A, G through vgposp_gemm's kernels,
 *                     M by vgposp_potrf_lower's recursion (invert = 1), W^T.  info (device int32):
 *                     the factorization's status; > 0 when G is not positive definite (noise NULL,
 *                     sigma2 = 0 and F_A rank-deficient).  It is kept in ws: after a non-zero
 *                     status every launch of vgposp_fpost_apply that writes var or out is a
 *                     no-op.  Bytes: 8 n s (dg) + O(k s).
 *   vgposp_fpost_apply  (main.py:190-199, the prediction the reference stops short of) var [n]
 *                     (or NULL: not computed), and with Y [k][ldy] (or NULL) the nrhs columns of
 *                     readings: out [n][ldo] = the posterior means; mu [n] the prior mean (NULL:
 *                     zeros).  alpha = M^T (M (Y - mu_A)) and Z through vgposp_gemm's kernels, then
 *                     one stream over F per panel of 64 columns of [W^T | Z] (k and nrhs each
 *                     padded to a multiple of 16; only the columns asked for) on the fp64 matrix
 *                     cores, reduced per row as it leaves the accumulators, then the k sensor rows.
 *                     Byte model: 8 n s per panel + 8 n (1 + nrhs).  Any number of calls after
 *                     one init; F, noise, n, s, ldf, k as given to init.  That is NOT checked:
 *                     the status word and the layout live in ws, so an apply on a workspace no
 *                     init has run on, or with another n, s or k, reads an undefined status and
 *                     undefined factors.  No float atomics, two runs are bit-identical, no host
 *                     synchronisation.
 *   vgposp_fpost_workspace_bytes(n, s, k, nrhs_max)  (main.py:190-199) n + 2 k s + k^2 +
 *                     (3 k + s) nrhs_max doubles with k and nrhs_max padded to 16, and the k x k
 *                     factorization's workspace; 0 when n <= 0, s <= 0 or k <= 0.  apply needs
 *                     the bytes of its own nrhs only.
 * Limits: 1 <= s <= 4,096, n <= 2^22, ldf >= s, 1 <= k <= min(n, 1,024), 0 <= nrhs <= 1,024,
 * ldy >= nrhs, ldo >= nrhs; noise may be NULL.  Argument errors return -(position) before any
 * device work, a short workspace VGPOSP_E_WS. */
size_t vgposp_fpost_workspace_bytes(int64_t n, int64_t s, int k, int nrhs_max);
int vgposp_fpost_init(const double* F, int64_t n, int64_t s, int64_t ldf, const double* noise,
                      const int64_t* sensors, int k, double obs_noise, int* info, void* ws,
                      size_t ws_bytes, void* stream);
int vgposp_fpost_apply(const double* F, int64_t n, int64_t s, int64_t ldf, const double* noise,
                       int k, double* var, const double* Y, int64_t ldy, int nrhs,
                       const double* mu, double* out, int64_t ldo, void* ws, size_t ws_bytes,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * Exact algorithm 3 at grid sizes where cov_vv cannot be dense (config C4, 128^3): the beta-decay
 * tapered covariance (main_architecture_2_sampledistribution.py:355-421) is a sparse SPD stencil
 * matrix, and snippets_a3.sparse_placement_algorithm_3 (snippets_a3.py:43-364) with tf_nominator /
 * tf_denominator (snippets_a2.py:138-218) over the FULL sets A and V \ (A u {y}) needs
 *   round 0:  denom_y = 1 / Q_yy - eps,  Q = (Sigma + eps I)^-1   (every candidate)
 *   round t:  denom_y = 1 / (Q_yy - Q_yA Q_AA^-1 Q_Ay) - eps,
 *             nom_y   = s_yy - s_yA (Sigma_AA + eps I)^-1 s_Ay        (the window re-score)
 * diag(Q) comes from a nested-dissection multifrontal Cholesky and its selected inverse (the
 * symbolic plan is host-side, vgposp_amd/nested_dissection.py).  A front = pivots P + boundary U,
 * stored as row-major blocks PP [p][p] (lower), UP [u][p], UU [u][u]; a group of nf fronts of one
 * tree level is a strided batch (strides p*p, u*p, u*u).  p and u even (padded by the plan).
 *   vgposp_front_assemble:   original entries of the pivot columns into zeroed PP / UP:
 *       s(i, j) = tau[|i - j|^2] (K(x_i, x_j) + diag_shift [i == j]) + jitter [i == j]
 *     (the taper arguments as VGPOSP_LOCAL_ARGS); owner_ord / owner_pos [N]: post-order id of the
 *     front eliminating each node and its pivot position; piv [nf][p] (-1 = padding: identity);
 *     U [nf][u] ascending, ulen [nf]; order [nf]: the fronts' post-order ids.
 *   vgposp_front_extend_add: parent front += the lower triangle of each child's update UUc
 *     ([nfc][uc][uc]) at positions pmap [nfc][uc] (-1 = padding) of its parent front, which sits
 *     at element offsets par_off [nfc][3] of the parent level's PP / UP / UU buffers with padded
 *     sizes par_dim [nfc][2] = (p, u); only children with sibling[c] == sib (call once per
 *     sibling index: siblings share a parent).
 *   vgposp_front_factor:     per front, PP <- M = L^-1 (F_PP = L L^T), UU -= L_UP L_UP^T with
 *     L_UP = F_UP M^T, UP <- W = L_UP M.  info [nf] (potrf convention).  ws:
 *     vgposp_front_factor_workspace_bytes(p, u, nf).
 *   vgposp_front_gather:     child's full Q_UU [nfc][uc][uc] <- its parent's Q front (QPP lower,
 *     QUP, QUU full; the parent level's buffers, par_off / par_dim as above) at
 *     (pmap[a], pmap[b]); 0 on padding.
 *   vgposp_front_selinv:     QPP <- M^T M - W^T T (lower), QUP <- T = -QUU W (out of place).
 *   vgposp_front_diag:       out[piv[f][k]] <- QPP[f][k][k] for piv >= 0.
 * --------------------------------------------------------------------------------------------- */
size_t vgposp_front_factor_workspace_bytes(int64_t p, int64_t u, int nf);
int vgposp_front_assemble(int kind, const double* X, int64_t I0, int64_t I1, int64_t I2,
                          double amp, double ls, double diag_shift, double jitter,
                          const int* offsets, int m, const double* tau, int ntau,
                          const int* owner_ord, const int* owner_pos, const int* piv, int64_t p,
                          const int* U, int64_t u, const int* ulen, const int* order, int nf,
                          double* PP, double* UP, void* stream);
int vgposp_front_extend_add(const double* UUc, int64_t uc, int nfc, const int* pmap,
                            const int64_t* par_off, const int* par_dim, const int* sibling, int sib,
                            double* PP, double* UP, double* UU, void* stream);
int vgposp_front_factor(double* PP, double* UP, double* UU, int64_t p, int64_t u, int nf,
                        int* info, void* ws, size_t ws_bytes, void* stream);
int vgposp_front_gather(const double* QPP, const double* QUP, const double* QUU,
                        const int* pmap, const int64_t* par_off, const int* par_dim, int nfc,
                        int64_t uc, double* QUUc, void* stream);
int vgposp_front_selinv(const double* M, const double* W, const double* QUU, int64_t p, int64_t u,
                        int nf, double* QPP, double* QUP, void* stream);
int vgposp_front_diag(const double* QPP, int64_t p, int nf, const int* piv, double* out,
                      void* stream);

/* The rounds of exact algorithm 3 on the tapered covariance (taper arguments as above; kmax <= 128;
 * cutoff: the window [i_d - cutoff, i_d + cutoff) of snippets_a3.py:190-303; threshold: |nom| or
 * |denom| below -> delta 0, snippets_a2.py:480; radius: the stencil radius (largest offset
 * component); cg_iters: conjugate-gradient iterations per column).  qdiag [N]:
 * diag((Sigma + jitter I)^-1) from the front_* calls, or upper bounds of it from
 * vgposp_exact_bounds; cache [N] f64 (delta_cached), selected [N] uint8, both caller-owned.
 *
 * Selected-inverse form (qdiag exact):
 *   vgposp_exact_prepare(flags = 0): the stencil coefficients, round 0 (every candidate:
 *     nom = s_yy, denom = 1 / Q_yy - jitter) and the arg-max keys; clears `selected`.
 *   vgposp_exact_round:   pick `round` = the arg-max of the cache over V \ A (lowest index on ties),
 *     picks[round] / pick_delta[round]; unless `last`: q = Q e_pick by cg_iters CG iterations on
 *     Sigma + jitter I (stopping early once |r| <= cg_tol) on the box of half-width
 *     radius * cg_iters around the pick (the Krylov vectors are exactly zero beyond it), the next
 *     rows of chol(Q_AA) and chol(Sigma_AA + jitter I), and the window re-score
 *       nom = s_yy - |LS^-1 s_Ay|^2,  denom = 1 / (Q_yy - |LQ^-1 q_Ay|^2) - jitter.
 *
 * Bounded-lazy form (no selected inverse; same picks):
 *   vgposp_exact_coef:    the stencil coefficients and Gershgorin bounds [lambda_min, lambda_max]
 *     of Sigma + jitter I (device doubles, vgposp_exact_buffers' `gersh`).
 *   vgposp_exact_bounds:  qdiag[y] for y in [c0, c1) <- an upper bound of e_y^T (Sigma + jitter I)^-1
 *     e_y from K CG steps from x = 0: with mu = 0, hi_scale * g_K (g_K = the CG estimate, a
 *     lower bound; hi_scale = (1 + margin) / (1 - 4 rho^2K)); with 0 < mu <= lambda_min, the
 *     Gauss-Radau bound hi_scale * (g_K + gamma^mu_K |r_K|^2) (hi_scale = 1 + margin; the
 *     recurrence is in exact_greedy.hip).  tab_off int [T][3]: the offsets
 *     within K stencil steps, sorted by step count (offset 0 first); tab_cnt int [K + 1]: offsets
 *     within d steps; tab_nb int [T][m - 1]: row of (offset + offsets[o]) in the table or -1.
 *     T <= 1024, T (m - 1) <= 8192.
 *   vgposp_exact_prepare(flags = 1): round 0 from those bounds (cache = upper bounds); flags = 3:
 *     the same, the bounds being the first of two levels (vgposp_exact_tighten_pending).
 *   vgposp_exact_steps_reset: clears the rounds' control block (after prepare, before the rounds).
 *   vgposp_exact_steps:   rounds [round0, round1) of a run of k picks, decided on the device.
 *     Each round is two kernels: the first refreshes the arg-max keys of the previous round's
 *     window, takes the arg-max of the cache over V \ A (lowest index on ties) and either picks
 *     it (its Q_yy exact, its column in a slot: picks[round] / pick_delta[round], the pick's rows
 *     of chol(Q_AA) and chol(Sigma_AA + jitter I)) or STALLS: the control block records the round
 *     and the refinement
 *     batch: every later kernel of the issued rounds then does nothing.  The second re-scores the
 *     window of the pick (upper bounds where Q_yy is still only bounded).  After the rounds one
 *     kernel chooses the batch of a stalled round: of the `batch` <= 32 best entries without a
 *     column, those still on their first (K_lo-step) bound go to the TIGHTENING list, the others
 *     and the arg-max to the CG batch, each given a free column slot or the oldest unpinned one.
 *   vgposp_exact_tighten_pending: the tightening list's bounds again with the K_hi-step table
 *     (arguments as vgposp_exact_bounds; the smaller of the two bounds is kept), the candidates'
 *     cache entries re-scored; clears the stall when the CG batch is empty.  m = 7 only.
 *   vgposp_exact_pretighten: after prepare(flags = 3) and steps_reset, before the rounds: the
 *     M <= 32,768 candidates with the largest round-0 entries (a radix select of the M-th largest
 *     key; ties at the threshold included; if that lists more than 65,536, none) get the K_hi-step
 *     bounds at once
 *     (arguments as vgposp_exact_bounds), their entries re-scored and the arg-max keys rebuilt;
 *     the count is added to the control block's tightened total.  m = 7 only.
 *   vgposp_exact_refine_pending: Q e_c for the pending CG batch by one batched CG (columns into
 *     their slots); each Q_cc becomes exact and the candidate's cache entry the reference's value
 *     (scored with the A of its last re-score); clears the stall.  After the tightening when both
 *     are pending.
 *   vgposp_exact_ctl:     device address of the control block, int32 [8]: stalled round (-1:
 *     none), CG batch size, refined-not-picked count, refinement batches, candidates refined,
 *     refinement counter, tightening list size, candidates tightened.
 *   vgposp_exact_update:  after pick `round`: the factor rows and the window re-score (upper
 *     bounds where Q_yy is still only bounded), for a caller that issues the rounds itself;
 *     vgposp_exact_steps does not call it (it launches the same window kernel per round).
 *   The caller issues rounds, reads the control block, and on a stall refines the pending batch
 *   and re-issues the rounds from the stalled one: one host read per refinement batch (the B best
 *   entries are refined together, one batched CG, the launches of one column; the next rounds'
 *   picks are mostly among them).
 *
 *   vgposp_exact_buffers: device addresses of the column slots [2 kmax][b0 b1 b2] (box-local, C
 *     order, box dims b_d = min(2 radius cg_iters + 1, I_d)), their box origins int64
 *     [2 kmax][3], the CG state (int [2]: converged flag, iterations of the last solve), the
 *     column slot of every pick (int [kmax]), two int64 of unused scratch (`cand`, kept so that
 *     the signature and the workspace size stay) and the Gershgorin bounds (double [2]). */
#define VGPOSP_EXACT_ARGS                                                                         \
  int kind, const double *X, int64_t I0, int64_t I1, int64_t I2, double amp, double ls,          \
      double diag_shift, double jitter, double threshold, const int *offsets, int m,             \
      const double *tau, int ntau, int kmax, int cutoff, int radius, int cg_iters,               \
      const double *qdiag, double *cache, uint8_t *selected, void *ws, size_t ws_bytes
size_t vgposp_exact_workspace_bytes(int64_t I0, int64_t I1, int64_t I2, int m, int kmax, int radius,
                                    int cg_iters);
int vgposp_exact_prepare(VGPOSP_EXACT_ARGS, int flags, void* stream);
int vgposp_exact_round(VGPOSP_EXACT_ARGS, int round, int last, int64_t* picks, double* pick_delta,
                       double cg_tol, void* stream);
int vgposp_exact_coef(VGPOSP_EXACT_ARGS, void* stream);
int vgposp_exact_bounds(VGPOSP_EXACT_ARGS, const int* tab_off, const int* tab_nb,
                        const int* tab_cnt, int T, int K, double hi_scale, double mu, int64_t c0,
                        int64_t c1, void* stream);
int vgposp_exact_steps_reset(VGPOSP_EXACT_ARGS, void* stream);
int vgposp_exact_steps(VGPOSP_EXACT_ARGS, int round0, int round1, int k, int batch,
                       int64_t* picks, double* pick_delta, void* stream);
int vgposp_exact_refine_pending(VGPOSP_EXACT_ARGS, int batch, const int64_t* picks, double cg_tol,
                                void* stream);
int vgposp_exact_tighten_pending(VGPOSP_EXACT_ARGS, const int* tab_off, const int* tab_nb,
                                 const int* tab_cnt, int T, int K, double hi_scale, double mu,
                                 const int64_t* picks, void* stream);
int vgposp_exact_pretighten(VGPOSP_EXACT_ARGS, const int* tab_off, const int* tab_nb,
                            const int* tab_cnt, int T, int K, double hi_scale, double mu,
                            int64_t M, void* stream);
int vgposp_exact_ctl(void* ws, int64_t I0, int64_t I1, int64_t I2, int m, int kmax, int radius,
                     int cg_iters, int** ctl);
int vgposp_exact_update(VGPOSP_EXACT_ARGS, int round, const int64_t* picks, void* stream);
int vgposp_exact_buffers(void* ws, int64_t I0, int64_t I1, int64_t I2, int m, int kmax, int radius,
                         int cg_iters, double** qcols, int64_t** boxlo, int** cgstate,
                         int** slot_of_round, int64_t** cand, double** gersh);

/* ---------------------------------------------------------------------------------------------
 * TF1 AdamOptimizer step on a device parameter vector (tf.train.AdamOptimizer in
 * gp_functions.tf_train_gp_adam, gp_functions.py:179-182; variational_Gaussian_process_example.py
 * :101-102).  g = grad_scale * grad (grad_scale = -1 maximises);  t = *step + 1 (device int64,
 * incremented):  lr_t = lr sqrt(1 - b2^t) / (1 - b1^t);  m = b1 m + (1-b1) g;
 * v = b2 v + (1-b2) g^2;  theta -= lr_t m / (sqrt(v) + eps).
 * --------------------------------------------------------------------------------------------- */
int vgposp_adam_update(double* theta, const double* grad, double* m, double* v, int64_t n,
                       double lr, double beta1, double beta2, double eps, int64_t* step,
                       double grad_scale, void* stream);

/* Softplus-constrained parameters (the reference's `softplus(var)` / `1e-5 + softplus(var)`
 * kernel amplitude, length scale and noise, variational_Gaussian_process_example.py:47-61;
 * gp_functions.py:131-134) whose unconstrained vars live in theta:
 *   vgposp_softplus_values:       out[k] = offsets[k] + softplus(theta[slots[k]]), nparam <= 4;
 *   vgposp_adam_update_softplus:  vgposp_adam_update where the gradient of theta[slots[k]] is
 *                                 *gsrc[k] * sigmoid(theta[slots[k]]) (gsrc: nparam device
 *                                 pointers; the chain rule through the softplus; grad[slots[k]]
 *                                 is not read).
 * One launch each instead of a few elementwise launches per parameter. */
int vgposp_softplus_values(const double* theta, int64_t n, int nparam, const int* slots,
                           const double* offsets, double* out, void* stream);
int vgposp_adam_update_softplus(double* theta, const double* grad, double* m, double* v,
                                int64_t n, double lr, double beta1, double beta2, double eps,
                                int64_t* step, double grad_scale, int nparam, const int* slots,
                                const double* const* gsrc, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Optional per-launch timing (no reference counterpart; the reference times with wall clocks,
 * placement_algorithm2.py:416-430).  When enabled, every launch of the library's named kernels
 * ("gemm_f64", "potrf_diag", "kernel_matrix", "greedy_trmv", "greedy_update", "greedy_select",
 * ...) is bracketed by a hipEvent pair on its stream together with its algorithmic flops and
 * bytes.  vgposp_prof_query synchronises on the recorded events and sums them per kernel name.
 * Enabling (or re-enabling) clears the records.  Host-side state, guarded by a mutex.
 * --------------------------------------------------------------------------------------------- */
int vgposp_prof_enable(int on);
int vgposp_prof_query(const char* name, double* total_ms, int64_t* launches, double* flops,
                      double* bytes);
/* Text summary of all records: one "name<TAB>ms<TAB>launches<TAB>flops<TAB>bytes" line per
 * distinct kernel name.  Returns the size needed (with the NUL); buf may be NULL. */
int64_t vgposp_prof_dump(char* buf, size_t len);

#ifdef __cplusplus
}
#endif

#endif /* VGPOSP_H_ */
