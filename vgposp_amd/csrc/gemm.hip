// fp64 GEMM on CDNA4 matrix cores (v_mfma_f64_16x16x4f64), the dense contraction behind the
// Cholesky trailing update, the fused block Gauss-Jordan inverse and C^-1 = M^T M formation.
//
//   C = alpha * op(A) * op(B) + beta * C        (row-major, fp64)
//
// Two kernels share the 128x128x16 tile geometry (4 waves in a 2x2 grid, 64x64 = 4x4 MFMA
// fragments per wave):
//   gemm_glds_kernel (default)  LDS-DMA staging (global_load_lds), 2-stage ring, 2 WG per CU,
//                               XOR-swizzled lane-linear LDS images; described above the kernel.
//   gemm_ref_kernel (fallback)  odd sizes / unaligned operands: register staging into padded
//                               images, bank-conflict-free for the fragment reads (lane l reads
//                               row l&15, k = l>>4):
//     KC image [row][k] with a row pitch of 18 doubles   (operand stored k-contiguous)
//     MC image [k][row] with a row pitch of 144 doubles  (operand stored row-contiguous)
// No operand ever needs an explicit transpose in HBM.
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "dense.h"

namespace vgposp {

typedef double dbl4 __attribute__((ext_vector_type(4)));
typedef unsigned int v2u32_t __attribute__((ext_vector_type(2)));

constexpr int GBM = 128;
constexpr int GBN = 128;
constexpr int GBK = 16;
constexpr int KC_PITCH = GBK + 2;    // 18 doubles
constexpr int MC_PITCH = GBM + 16;   // 144 doubles
constexpr int TILE_ELEMS = GBM * KC_PITCH;  // == GBK * MC_PITCH == 2304 doubles
static_assert(GBM * KC_PITCH == GBK * MC_PITCH, "LDS images must be the same size");

struct GemmParams {
  int64_t m, n, k;
  double alpha, beta;
  const double* A;
  int64_t lda;
  const double* B;
  int64_t ldb;
  double* C;
  int64_t ldc;
  int uplo_c, tri_a, tri_b;
  // split-K: nsplit > 1 launches nblk * nsplit workgroups; split z covers K range
  // [z * kchunk, (z + 1) * kchunk) and writes alpha * partial to part + z * m * n (ld n)
  int nsplit, nblk;
  int64_t kchunk;
  double* part;
  // batch (grid.y of the fast kernel, grid.z of the reference kernel): element b reads
  // A + b sA, B + b sB and writes C + b sC (split-K partials at part + b sP)
  int64_t sA, sB, sC, sP;
  // device abort flag (a failed pivot of the enclosing factorization): non-zero -> the launch
  // does nothing (vgposp_greedy_init's early stop without a host synchronisation)
  const int* abort;
  // epilogue of the fast kernels (vgposp_gemm_set_epilogue): 0 = element-wise reference,
  // 1 = batched; filled by gemm_plan
  int epilogue;
};

// Further destinations of one product (gemm_glds_multi_kernel, the Strassen products): besides
// C = alpha acc + beta C the epilogue writes C[d] = alpha[d] acc + beta[d] C[d] for d < n.  A
// product of one Strassen level lands in two quadrants of C, of two levels in four (1 + 3).
// Kept out of GemmParams so that the kernels without extra destinations keep their arguments.
constexpr int GEMM_XDST = 3;
struct GemmExtra {
  int n;
  double* C[GEMM_XDST];
  int64_t ld[GEMM_XDST];
  double alpha[GEMM_XDST], beta[GEMM_XDST];
};

// Set by a factorization for the GEMMs it launches from this thread (gemm_abort_scope).
thread_local const int* tl_gemm_abort = nullptr;

// Stage one operand tile (128 rows of the M/N dimension x 16 of K) into registers.
//   KC: stored[row][k] (row = M/N index), MC: stored[k][row].
// tri: the stored matrix is lower triangular (entries with column > row read as 0).
template <bool KC>
__device__ __forceinline__ void load_tile(const double* __restrict__ base, int64_t ld, int64_t r0,
                                          int64_t k0, int64_t R, int64_t K, bool tri, bool vec,
                                          double2 (&reg)[4]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int e = t + 256 * it;
    int64_t gr, gk;
    if (KC) {
      gr = r0 + (e >> 3);
      gk = k0 + (e & 7) * 2;
    } else {
      gk = k0 + (e >> 6);
      gr = r0 + (e & 63) * 2;
    }
    double2 v = make_double2(0.0, 0.0);
    if (KC) {
      // elements (gr, gk) and (gr, gk+1) of stored[row][k]
      const double* p = base + gr * ld + gk;
      if (gr < R) {
        if (vec && gk + 1 < K) {
          v = *reinterpret_cast<const double2*>(p);
        } else {
          if (gk < K) v.x = p[0];
          if (gk + 1 < K) v.y = p[1];
        }
        if (tri) {
          if (gk > gr) v.x = 0.0;
          if (gk + 1 > gr) v.y = 0.0;
        }
      }
    } else {
      // elements (gk, gr) and (gk, gr+1) of stored[k][row]
      const double* p = base + gk * ld + gr;
      if (gk < K) {
        if (vec && gr + 1 < R) {
          v = *reinterpret_cast<const double2*>(p);
        } else {
          if (gr < R) v.x = p[0];
          if (gr + 1 < R) v.y = p[1];
        }
        if (tri) {
          if (gr > gk) v.x = 0.0;
          if (gr + 1 > gk) v.y = 0.0;
        }
      }
    }
    reg[it] = v;
  }
}

template <bool KC>
__device__ __forceinline__ void store_tile(double* lds, const double2 (&reg)[4]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int e = t + 256 * it;
    int off;
    if (KC) off = (e >> 3) * KC_PITCH + (e & 7) * 2;
    else off = (e >> 6) * MC_PITCH + (e & 63) * 2;
    *reinterpret_cast<double2*>(lds + off) = reg[it];
  }
}

// Fragment read: element (row, k) of the staged tile.
template <bool KC>
__device__ __forceinline__ double frag(const double* lds, int row, int k) {
  return KC ? lds[row * KC_PITCH + k] : lds[k * MC_PITCH + row];
}

// TA: A stored k x m (A^T used).  TB: B stored n x k (B^T used).
template <bool TA, bool TB>
__global__ __launch_bounds__(256) void gemm_ref_kernel(GemmParams p, int vec_a, int vec_b) {
  if (p.abort != nullptr && *p.abort != 0) return;
  constexpr bool A_KC = !TA;  // A[m][k] is k-contiguous
  constexpr bool B_KC = TB;   // B[n][k] is k-contiguous
  __shared__ double smem[2 * 2 * TILE_ELEMS];  // [buf][A|B][tile]

  const int64_t m0 = (int64_t)blockIdx.y * GBM;
  const int64_t n0 = (int64_t)blockIdx.x * GBN;
  if (p.uplo_c == VGPOSP_LOWER && n0 > m0 + GBM - 1) return;  // tile entirely above diagonal
  p.A += blockIdx.z * p.sA;
  p.B += blockIdx.z * p.sB;
  p.C += blockIdx.z * p.sC;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fk = lane >> 4;

  // K range that can contribute (triangular operands have zero blocks).
  int64_t kbeg = 0, kend = p.k;
  if (p.tri_a) {
    if (TA) kbeg = m0;               // stored A[k][i], zero for i > k  -> k >= i >= m0
    else kend = min(kend, m0 + GBM); // stored A[i][k], zero for k > i  -> k <= i < m0+GBM
  }
  if (p.tri_b) {
    if (TB) kend = min(kend, n0 + GBN);  // stored B[j][k], zero for k > j
    else kbeg = max(kbeg, n0);           // stored B[k][j], zero for j > k
  }
  kbeg = (kbeg / GBK) * GBK;

  dbl4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = dbl4{0.0, 0.0, 0.0, 0.0};

  const bool va = vec_a != 0, vb = vec_b != 0;
  double2 ra[4], rb[4];
  int buf = 0;
  if (kbeg < kend) {
    load_tile<A_KC>(p.A, p.lda, m0, kbeg, p.m, p.k, p.tri_a != 0, va, ra);
    load_tile<B_KC>(p.B, p.ldb, n0, kbeg, p.n, p.k, p.tri_b != 0, vb, rb);
    store_tile<A_KC>(smem, ra);
    store_tile<B_KC>(smem + TILE_ELEMS, rb);
  }
  __syncthreads();

  for (int64_t k0 = kbeg; k0 < kend; k0 += GBK) {
    const bool more = k0 + GBK < kend;
    if (more) {
      load_tile<A_KC>(p.A, p.lda, m0, k0 + GBK, p.m, p.k, p.tri_a != 0, va, ra);
      load_tile<B_KC>(p.B, p.ldb, n0, k0 + GBK, p.n, p.k, p.tri_b != 0, vb, rb);
    }
    const double* As = smem + buf * 2 * TILE_ELEMS;
    const double* Bs = As + TILE_ELEMS;
#pragma unroll
    for (int ks = 0; ks < GBK / 4; ++ks) {
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = frag<A_KC>(As, wm * 64 + i * 16 + fr, ks * 4 + fk);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = frag<B_KC>(Bs, wn * 64 + j * 16 + fr, ks * 4 + fk);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      double* Ad = smem + (buf ^ 1) * 2 * TILE_ELEMS;
      store_tile<A_KC>(Ad, ra);
      store_tile<B_KC>(Ad + TILE_ELEMS, rb);
    }
    __syncthreads();
    buf ^= 1;
  }

  // Epilogue.  f64 MFMA C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg.
  const bool lower = p.uplo_c == VGPOSP_LOWER;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t col = n0 + wn * 64 + j * 16 + fr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = m0 + wm * 64 + i * 16 + fk + 4 * r;
        if (row < p.m && col < p.n && (!lower || col <= row)) {
          double* c = p.C + row * p.ldc + col;
          double v = p.alpha * acc[i][j][r];
          if (p.beta != 0.0) v += p.beta * *c;
          *c = v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Fast path: operands streamed HBM -> LDS with global_load_lds_dwordx4 (no VGPR staging) through
// a two-stage ring, vmcnt waits and raw barriers, so the next K-tile is in flight while one is
// multiplied.  Two stages (64 KiB of LDS) let two workgroups share a CU, i.e. two
// waves per SIMD: one wave's barrier / LDS-latency bubbles are filled by the other's MFMAs.
// Measured on 8192^3 NT: 4 stages x 1 WG/CU 57 TF/s, 3 x 1 61, 2 x 1 62, 2 x 2 69 TF/s.  The LDS images are lane-linear (as glds requires) and the XOR swizzle
// is applied on the per-lane SOURCE address and on the fragment read (conflict-free reads):
//   KC image [128 rows][16 k]:  slot (r, pair p) holds pair p ^ ((r & 15) >> 1)
//   MC image [16 k][128 cols]:  slot (k, pair p) holds pair p ^ ((k & 1) << 3)
// Out-of-range rows / columns / k are CLAMPED to valid addresses (every load is in bounds); the
// duplicated data is discarded at the store (rows, columns) or masked at the fragment read (k,
// triangular operands).  Requires even m, n, k, ld and 16-byte aligned bases (else gemm_ref).
// Workgroups are remapped XCD-aware (contiguous tile ranges per XCD) and, for a lower-triangular
// C, only tiles on or below the diagonal are launched.
constexpr int STAGES = 2;      // LDS ring depth (3 and 4 stages at one workgroup per CU: slower)
constexpr int GEMM_GROUP = 4;  // row tiles per XCD band (1, 2, 8, 16 measured: DESIGN.md §4)
constexpr int GEMM_OCC = 2;    // workgroups per CU (the launch bound)
constexpr int GEMM_WAVES = 4;  // 2 x 2 waves of 64 x 64 (4 x 4 MFMA fragments each)
// LDS-DMA pieces per wave per stage: 4 of A, then 4 of B.  Every wave issues its share of both
// operands, with no branches (measured: splitting the waves into A-loaders and B-loaders cost
// 10% on 8192^3).
constexpr int WAVE_PIECES = 8;
// The next K-tile's pieces are spread over the first two k-slices, each slice's share after its
// fragment reads: the reads do not wait behind the piece issue after the barrier (measured
// against all eight issued right after the barrier: 65k step 16.10 -> 16.23 placements/s over
// three interleaved repeats).
constexpr int SPREAD_SLICES = 2;
constexpr int OPND_ELEMS = GBM * GBK;        // 2048 doubles = 16 KiB per operand per stage
// LDS of one workgroup (doubles): the ring of stages, each [A tile | B tile]
constexpr int GLDS_SMEM_ELEMS = STAGES * 2 * OPND_ELEMS;
static_assert(STAGES == 2, "the K loop loads one tile ahead and waits for all of it: 2-stage ring");

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// One 1-KiB wave-instruction ("piece" i = 0..15) of a 128-row x 16-k operand tile.
template <bool KC>
__device__ __forceinline__ void glds_piece(const double* base, int64_t ld, int64_t r0, int64_t k0,
                                           int64_t R, int64_t K, double* dst, int i, int lane) {
  {
    const double* src;
    if (KC) {
      const int row = 8 * i + (lane >> 3);
      const int kp = (lane & 7) ^ ((row & 15) >> 1);
      const int64_t gr = min(r0 + row, R - 1);
      const int64_t gk = min(k0 + 2 * kp, K - 2);
      src = base + gr * ld + gk;
    } else {
      const int p = lane ^ ((i & 1) << 3);
      const int64_t gk = min(k0 + i, K - 1);
      const int64_t gc = min(r0 + 2 * p, R - 2);
      src = base + gk * ld + gc;
    }
    __builtin_amdgcn_global_load_lds((const void*)src, (lds_ptr_t)(dst + i * 128), 16, 0, 0);
  }
}

template <bool KC>
__device__ __forceinline__ int frag_off(int row, int k) {
  if (KC) return row * 16 + 2 * ((k >> 1) ^ ((row & 15) >> 1)) + (k & 1);
  return k * 128 + 2 * ((row >> 1) ^ ((k & 1) << 3)) + (row & 1);
}

__device__ __forceinline__ int tri_root(int64_t id) {
  int64_t t = (int64_t)((sqrt(8.0 * (double)id + 1.0) - 1.0) * 0.5);
  while ((t + 1) * (t + 2) / 2 <= id) ++t;
  while (t * (t + 1) / 2 > id) --t;
  return (int)t;
}

// (The 256x128 tile configurations and the register-staged kernel measured against this one
// live in tools/variants.)

// ---------------------------------------------------------------------------------------------
// Hand-scheduled interior K-tiles (vgposp_gemm_set_kloop(1); TA = false, 2-stage ring).  One asm
// statement (kloop_pair) takes two K-tiles, the first in ring stage 0 and the second in stage 1,
// so that both stages are immediates.  Each K-tile t, out of stage S, leaves tile t + 1 ready:
//   reads(1) wait MFMA(0) [A pieces] reads(2) wait MFMA(1) [B pieces] reads(3) wait MFMA(2)
//   vmcnt(0) lgkmcnt(0) s_barrier reads(0 of t + 1) MFMA(3)
// reads(s) = the slice's fragment reads, issued one slice ahead into the other of two fragment
// buffers and retired by counted lgkmcnt waits; MFMA(s) = the 16 MFMAs of slice s, in the C++
// loop's (i, j) order, so every accumulator sees the same products in the same k order and the
// result is bit-identical to the C++ loop.  The one barrier sits before the last slice's MFMAs:
// that slice's fragments are in registers by then, so behind it stage S is free (for tile t + 2)
// and stage S^1 holds tile t + 1.
// The statement's registers are fixed, because it names sub-registers of vector operands:
//   v[208:215] per-lane source offsets of this wave's 8 pieces (A 0..3, B 0..3), constant
//   v[216:223] per-lane LDS fragment bases: A k-slice 0..3, then B k-slice 0..3 (stored n x k)
//              or B fragments {0, 2} / {1, 3} (stored k x n, where the k-slice is an immediate)
//   v[224:239] fragment buffer 0 (a0..a3, b0..b3): slice 0 on entry, slice 0 of tile t + 1 on exit
//   v[240:255] fragment buffer 1 (clobbered)
// The A and B source bases of the tile to load are scalar operands, advanced by a uniform stride
// per K-tile in the C++ around the statement (scalar adds); the pieces need no clamp selects
// (interior tiles have no k clamp, the row clamp is folded into the constant offsets).
// Stage, fragment and row group are immediate offset fields; M0 is saved and restored.
// The next LDS-DMA pieces, for tile t + 1, go four behind slice 0's MFMAs and four behind slice
// 1's.  Two other placements, all eight for tile t + 2 directly behind the barrier or behind
// tile t + 1's slice-0 reads, were slower on every layout (DESIGN.md §4 "Hand-scheduled K loop";
// they were build switches of commit cb6bc49, which git history keeps).
// VGPOSP_KLOOP_DEFAULT is the setting a process starts with.
// ---------------------------------------------------------------------------------------------
#ifndef VGPOSP_KLOOP_DEFAULT
#define VGPOSP_KLOOP_DEFAULT 1
#endif

typedef double dbl8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x8 __attribute__((ext_vector_type(8)));

#define KL_M(A, B, C) "v_mfma_f64_16x16x4_f64 %[" #C "], v[" A "], v[" B "], %[" #C "]\n\t"
#define KL_M4(A, I, B0, B1, B2, B3) \
  KL_M(A, B0, c##I##0) KL_M(A, B1, c##I##1) KL_M(A, B2, c##I##2) KL_M(A, B3, c##I##3)
#define KL_MFMA_F0                                               \
  KL_M4("224:225", 0, "232:233", "234:235", "236:237", "238:239") \
  KL_M4("226:227", 1, "232:233", "234:235", "236:237", "238:239") \
  KL_M4("228:229", 2, "232:233", "234:235", "236:237", "238:239") \
  KL_M4("230:231", 3, "232:233", "234:235", "236:237", "238:239")
#define KL_MFMA_F1                                               \
  KL_M4("240:241", 0, "248:249", "250:251", "252:253", "254:255") \
  KL_M4("242:243", 1, "248:249", "250:251", "252:253", "254:255") \
  KL_M4("244:245", 2, "248:249", "250:251", "252:253", "254:255") \
  KL_M4("246:247", 3, "248:249", "250:251", "252:253", "254:255")
// four fragments of a k-contiguous image: rows 16 apart are 4 x 512 bytes apart (U: the stage's
// and the operand's offset in 512-byte units)
#define KL_RKC(D0, D1, BASE, U)                                                   \
  "ds_read2st64_b64 v[" D0 "], v" BASE " offset0:" U "+0 offset1:" U "+4\n\t" \
  "ds_read2st64_b64 v[" D1 "], v" BASE " offset0:" U "+8 offset1:" U "+12\n\t"
// four fragments of B stored k x n: fragments {0, 2} and {1, 3} are 256 bytes apart from their
// bases (the swizzle exchanges 0/1 and 2/3 on odd k), a k-slice 4096 bytes (SB: stage bytes)
#define KL_RMC(D0, D1, D2, D3, KS, SB)                                        \
  "ds_read_b64 v[" D0 "], v220 offset:" SB "+16384+" #KS "*4096\n\t"      \
  "ds_read_b64 v[" D1 "], v221 offset:" SB "+16384+" #KS "*4096\n\t"      \
  "ds_read_b64 v[" D2 "], v220 offset:" SB "+16384+" #KS "*4096+256\n\t"  \
  "ds_read_b64 v[" D3 "], v221 offset:" SB "+16384+" #KS "*4096+256\n\t"
// slice KS of the tile at stage symbol SR (512-byte units) / SB (bytes) into buffer 0 or 1
#define KL_RD0_NT(KS, SR, SB) \
  KL_RKC("224:227", "228:231", KL_LA##KS, SR) KL_RKC("232:235", "236:239", KL_LB##KS, SR "+32")
#define KL_RD1_NT(KS, SR, SB) \
  KL_RKC("240:243", "244:247", KL_LA##KS, SR) KL_RKC("248:251", "252:255", KL_LB##KS, SR "+32")
#define KL_RD0_NN(KS, SR, SB)                  \
  KL_RKC("224:227", "228:231", KL_LA##KS, SR) \
  KL_RMC("232:233", "234:235", "236:237", "238:239", KS, SB)
#define KL_RD1_NN(KS, SR, SB)                  \
  KL_RKC("240:243", "244:247", KL_LA##KS, SR) \
  KL_RMC("248:249", "250:251", "252:253", "254:255", KS, SB)
#define KL_LA0 "216"
#define KL_LA1 "217"
#define KL_LA2 "218"
#define KL_LA3 "219"
#define KL_LB0 "220"
#define KL_LB1 "221"
#define KL_LB2 "222"
#define KL_LB3 "223"
// piece Q of operand O into the stage at PD bytes: M0 = the wave's LDS destination, source =
// base SG + this lane's offset
#define KL_PIECE(O, Q, V, PD, SG)                                          \
  "s_add_u32 m0, %[lds], " PD "+" #O "*16384+" #Q "*1024\n\ts_nop 0\n\t" \
  "global_load_lds_dwordx4 v" V ", " SG "\n\t"
#define KL_PIECES_A(PD, GA)                                    \
  KL_PIECE(0, 0, "208", PD, GA) KL_PIECE(0, 1, "209", PD, GA) \
  KL_PIECE(0, 2, "210", PD, GA) KL_PIECE(0, 3, "211", PD, GA)
#define KL_PIECES_B(PD, GB)                                    \
  KL_PIECE(1, 0, "212", PD, GB) KL_PIECE(1, 1, "213", PD, GB) \
  KL_PIECE(1, 2, "214", PD, GB) KL_PIECE(1, 3, "215", PD, GB)
// L = NT | NN, NRD = fragment-read instructions per slice (a wait for slice s leaves slice s + 1's
// NRD reads in flight), GA / GB = the source bases of the next tile's pieces, PD = the bytes of
// the stage they go to, SR / SB = the tile's stage in 512-byte units / bytes, NR / NB = the next
// tile's
#define KL_TILE(L, NRD, PD, GA, GB, SR, SB, NR, NB)                                        \
  KL_RD1_##L(1, SR, SB) "s_waitcnt lgkmcnt(" #NRD ")\n\t" KL_MFMA_F0 KL_PIECES_A(PD, GA) \
  KL_RD0_##L(2, SR, SB) "s_waitcnt lgkmcnt(" #NRD ")\n\t" KL_MFMA_F1 KL_PIECES_B(PD, GB) \
  KL_RD1_##L(3, SR, SB) "s_waitcnt lgkmcnt(" #NRD ")\n\t" KL_MFMA_F0                     \
  "s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier\n\t"                                     \
  KL_RD0_##L(0, NR, NB) KL_MFMA_F1
// a tile's pieces go to the other stage
#define KL_T0(L, NRD) KL_TILE(L, NRD, "32768", "%[ga0]", "%[gb0]", "0", "0", "64", "32768")
#define KL_T1(L, NRD) KL_TILE(L, NRD, "0", "%[ga1]", "%[gb1]", "64", "32768", "0", "0")

// K-tiles t (even: ring stage 0) and t + 1 (stage 1) in one statement, so that both stages are
// immediates.  ga0 / gb0 and ga1 / gb1 are the source bases of the tiles that the first and the
// second tile load.
template <bool TB>
__device__ __forceinline__ void kloop_pair(dbl4 (&acc)[4][4], u32x8& vo, u32x8& lb, dbl8& f0,
                                           uint64_t ga0, uint64_t gb0, uint64_t ga1, uint64_t gb1,
                                           unsigned lds) {
  unsigned keep;
#define KL_OPERANDS                                                                              \
  : [c00] "+v"(acc[0][0]), [c01] "+v"(acc[0][1]), [c02] "+v"(acc[0][2]), [c03] "+v"(acc[0][3]),  \
    [c10] "+v"(acc[1][0]), [c11] "+v"(acc[1][1]), [c12] "+v"(acc[1][2]), [c13] "+v"(acc[1][3]),  \
    [c20] "+v"(acc[2][0]), [c21] "+v"(acc[2][1]), [c22] "+v"(acc[2][2]), [c23] "+v"(acc[2][3]),  \
    [c30] "+v"(acc[3][0]), [c31] "+v"(acc[3][1]), [c32] "+v"(acc[3][2]), [c33] "+v"(acc[3][3]),  \
    "+{v[208:215]}"(vo), "+{v[216:223]}"(lb), "+{v[224:239]}"(f0), [keep] "=&s"(keep)            \
  : [ga0] "s"(ga0), [gb0] "s"(gb0), [ga1] "s"(ga1), [gb1] "s"(gb1), [lds] "s"(lds)               \
  : "memory", "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", "v248",            \
    "v249", "v250", "v251", "v252", "v253", "v254", "v255"
#define KL_SAVE "s_mov_b32 %[keep], m0\n\t"
#define KL_RESTORE "s_mov_b32 m0, %[keep]\n\t"
#define KL_PAIR(L, NRD) asm volatile(KL_SAVE KL_T0(L, NRD) KL_T1(L, NRD) KL_RESTORE KL_OPERANDS)
  if constexpr (TB) KL_PAIR(NT, 4);
  else KL_PAIR(NN, 6);
#undef KL_PAIR
#undef KL_OPERANDS
}

// One group of the batched epilogue: fragment row i of a wave, that is this lane's 16 elements
// a[j][r] of the four accumulators acc[i][0..3] (rows lr + 4 r, columns lc + 16 j of the tile),
// into one destination whose tile origin is org (wave-uniform) with leading dimension ld.
//   the 16 loads of C (only with beta != 0: C may hold anything otherwise), one wait,
//   t = alpha a and fma(beta, c, t) exactly as the element-wise epilogue computes them,
//   the 16 stores
// INNER (interior tile): no tests; an element is at a uniform base plus one per-lane offset.
// Otherwise (edge tiles: rows x cols of C lie behind org; diag: diagonal tile of a lower C, only
// columns <= row are written): the loads go to an address clamped into the part of C that the
// tile writes, the stores are under the lane's own mask.
// Offsets are 32-bit: the caller checks 128 ld * 8 < 2^32.
template <bool INNER>
__device__ __forceinline__ void epi_group(const dbl4 (&a)[4], double* org, int64_t ld, double alpha,
                                          double beta, int lr, int lc, int64_t rows, int64_t cols,
                                          bool diag) {
  char* at[4][4];
  unsigned off[4][4];
  bool ok[4][4];
  const unsigned ldb = (unsigned)ld * 8u;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (INNER) {
        at[r][j] = reinterpret_cast<char*>(org + 4 * r * ld + 16 * j);
        off[r][j] = (unsigned)lr * ldb + (unsigned)lc * 8u;
        ok[r][j] = true;
      } else {
        const int row = lr + 4 * r, col = lc + 16 * j;
        ok[r][j] = row < rows && col < cols && (!diag || col <= row);
        const int rc = (int)min((int64_t)row, rows - 1);
        int cc = (int)min((int64_t)col, cols - 1);
        if (diag) cc = min(cc, rc);
        at[r][j] = reinterpret_cast<char*>(org);
        off[r][j] = (unsigned)rc * ldb + (unsigned)cc * 8u;
      }
    }
  }
  if (beta != 0.0) {
    double c[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) c[r][j] = *reinterpret_cast<const double*>(at[r][j] + off[r][j]);
    if (!INNER) {
      // all 16 values are wanted here: the compiler otherwise sinks each use into its masked
      // store's block and waits there again, which drains the store before it
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(c[r][j]));
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) c[r][j] = __builtin_fma(beta, c[r][j], alpha * a[j][r]);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (INNER || ok[r][j]) *reinterpret_cast<double*>(at[r][j] + off[r][j]) = c[r][j];
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (INNER || ok[r][j]) *reinterpret_cast<double*>(at[r][j] + off[r][j]) = alpha * a[j][r];
  }
}

// One workgroup of the fast kernel: workgroup `bid` of the launch's `nwg` for this problem, batch
// element bz, LDS ring at smem (the kernel's own __shared__ array).
// MULTI: the epilogue also writes the extra destinations *x (plain products only: no triangular
// operand, full C, no split-K); the K loop is the same code.
// KL: the first run of K-tiles that need no mask and have a successor goes through kloop_pair;
// every other K-tile, the prologue and the epilogue are the C++ below.
template <bool TA, bool TB, bool TRIA, bool TRIB, bool MULTI = false, bool KL = false>
__device__ __forceinline__ void gemm_glds_body(const GemmParams& p, int tiles_m, int tiles_n,
                                               const int bid, const int nwg, const int64_t bz,
                                               double* smem, const GemmExtra* xd = nullptr) {
  static_assert(!MULTI || (!TRIA && !TRIB), "extra destinations: plain products only");
  static_assert(!KL || !TA, "hand-scheduled K loop: TA = false");
  if (p.abort != nullptr && *p.abort != 0) return;
  constexpr bool A_KC = !TA;
  constexpr bool B_KC = TB;

  // Tile order.  Uniform-K launches: XCD-aware bijective remap (each XCD walks a contiguous range
  // of tiles, so neighbours share A rows / B columns in its L2).  A lower-triangular A (K range
  // grows with the row tile) must NOT hand contiguous ranges to XCDs — one XCD would get every
  // long tile — so it keeps the round-robin dispatch and walks row groups longest first.
  int wg = bid;
  if (!TRIA) {
    const int xcd = bid & 7, q = nwg >> 3, rr = nwg & 7;
    wg = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (bid >> 3);
  }
  int zsplit = 0;
  if (p.nsplit > 1) {
    zsplit = wg / p.nblk;
    wg -= zsplit * p.nblk;
  }
  int ti, tj;
  if (p.uplo_c == VGPOSP_LOWER) {
    ti = tri_root(wg);
    tj = wg - ti * (ti + 1) / 2;
  } else {
    constexpr int GROUP = GEMM_GROUP;  // row tiles per group: neighbours share A rows and B columns
    const int per_group = GROUP * tiles_n;
    const int g = wg / per_group, first = g * GROUP;
    const int gsize = min(GROUP, tiles_m - first);
    const int local = wg - g * per_group;
    ti = first + local % gsize;
    tj = local / gsize;
    if (TRIA && !TA) ti = tiles_m - 1 - ti;  // longest K ranges first
  }
  const int64_t m0 = (int64_t)ti * GBM, n0 = (int64_t)tj * GBN;
  const double* const gA = p.A + bz * p.sA;
  const double* const gB = p.B + bz * p.sB;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fk = lane >> 4;

  // K range that can contribute when an operand is stored lower triangular.
  int64_t kbeg = 0, kend = p.k;
  if (TRIA) {
    if (TA) kbeg = max(kbeg, m0);        // stored A[k][i], zero for i > k
    else kend = min(kend, m0 + GBM);     // stored A[i][k], zero for k > i
  }
  if (TRIB) {
    if (TB) kend = min(kend, n0 + GBN);  // stored B[j][k], zero for k > j
    else kbeg = max(kbeg, n0);           // stored B[k][j], zero for j > k
  }
  if (p.nsplit > 1) {
    kbeg = max(kbeg, (int64_t)zsplit * p.kchunk);
    kend = min(kend, (int64_t)(zsplit + 1) * p.kchunk);
  }
  kbeg = (kbeg / GBK) * GBK;
  if (kend < kbeg) kend = kbeg;
  const int T = (int)((kend - kbeg + GBK - 1) / GBK);
  const bool partial_last = ((kend - kbeg) % GBK) != 0;

  dbl4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = dbl4{0.0, 0.0, 0.0, 0.0};

  // stage layout: [A tile | B tile].  Piece q (0 .. WAVE_PIECES - 1) of this wave for K-tile t:
  // the first half are pieces of A, the second half of B.
  int ln = lane;  // the lane as the K loop sees it
  auto issue_piece = [&](int t, int q) {
    double* st = smem + (t % STAGES) * 2 * OPND_ELEMS;
    const int64_t k0 = kbeg + (int64_t)t * GBK;
    const int j = wave * (WAVE_PIECES / 2) + q % (WAVE_PIECES / 2);  // piece of the operand tile
    if (q < WAVE_PIECES / 2)
      glds_piece<A_KC>(gA, p.lda, m0, k0, p.m, p.k, st, j, KL ? ln : lane);
    else
      glds_piece<B_KC>(gB, p.ldb, n0, k0, p.n, p.k, st + OPND_ELEMS, j, KL ? ln : lane);
  };

  if (T > 0) {
#pragma unroll
    for (int q = 0; q < WAVE_PIECES; ++q) issue_piece(0, q);
  }

  // [f0, f1): the first run of unmasked K-tiles, each with a successor (KL)
  int f0 = 0, f1 = 0;
  if constexpr (KL) {
    // the C++ tile's `mask` below, which it must agree with (see there why it is written twice)
    auto masked = [&](int t) {
      const int64_t k0 = kbeg + (int64_t)t * GBK;
      return (partial_last && t == T - 1) || (TRIA && k0 < m0 + GBM && k0 + GBK > m0) ||
             (TRIB && k0 < n0 + GBN && k0 + GBK > n0);
    };
    // 32-bit per-lane source offsets: 128 rows of a leading dimension below 2^21
    if (p.lda < (1 << 21) && p.ldb < (1 << 21)) {
      while (f0 < T - 1 && masked(f0)) ++f0;
      f0 += f0 & 1;  // pairs of K-tiles: the run starts at ring stage 0 and has an even length
      f1 = f0;
      while (f1 + 2 <= T - 1 && !masked(f1) && !masked(f1 + 1)) f1 += 2;
      // the run loads tile f1 without a k clamp: not the partial last tile
      if (partial_last && f1 == T - 1 && f1 > f0) f1 -= 2;
    }
  }

  for (int t = 0; t < T; ++t) {
    if constexpr (KL) {
      if (t == f0 && f0 < f1) {
        // tile t has landed and every wave is done with the other stage
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const unsigned lds0 = (unsigned)(uintptr_t)(lds_ptr_t)smem;
        const unsigned ldsw = __builtin_amdgcn_readfirstlane(lds0 + wave * (WAVE_PIECES / 2 * 1024));
        u32x8 vo, lb;
        dbl8 fr0;
        const double* As = smem + (t % STAGES) * 2 * OPND_ELEMS;
        const double* Bs = As + OPND_ELEMS;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = wave * (WAVE_PIECES / 2) + q;  // piece of the operand tile: glds_piece's addresses
          const int row = 8 * j + (lane >> 3);
          const int kp = (lane & 7) ^ ((row & 15) >> 1);
          vo[q] = (unsigned)((min(m0 + row, p.m - 1) - m0) * p.lda * 8 + kp * 16);
          if (TB) {
            vo[4 + q] = (unsigned)((min(n0 + row, p.n - 1) - n0) * p.ldb * 8 + kp * 16);
          } else {
            const int pp = lane ^ ((j & 1) << 3);
            vo[4 + q] = (unsigned)(j * p.ldb * 8 + (min(n0 + 2 * pp, p.n - 2) - n0) * 8);
          }
          lb[q] = lds0 + 8 * frag_off<true>(wm * 64 + fr, q * 4 + fk);
          if (TB) lb[4 + q] = lds0 + 8 * frag_off<true>(wn * 64 + fr, q * 4 + fk);
          else lb[4 + q] = q < 2 ? lds0 + 8 * frag_off<false>(wn * 64 + q * 16 + fr, fk) : 0u;
          fr0[q] = As[frag_off<true>(wm * 64 + q * 16 + fr, fk)];
          fr0[4 + q] = Bs[frag_off<B_KC>(wn * 64 + q * 16 + fr, fk)];
        }
        const int64_t kn = kbeg + (int64_t)(t + 1) * GBK;  // the run's first tile loads tile t + 1
        uint64_t ga = (uint64_t)(uintptr_t)(gA + m0 * p.lda + kn);
        uint64_t gb = (uint64_t)(uintptr_t)(TB ? gB + n0 * p.ldb + kn : gB + kn * p.ldb + n0);
        const uint64_t stride_b = TB ? GBK * 8u : (uint64_t)(GBK * 8 * p.ldb);
        int u = t;
        for (; u + 2 < f1; u += 2) {
          kloop_pair<TB>(acc, vo, lb, fr0, ga, gb, ga + GBK * 8, gb + stride_b, ldsw);
          ga += 2 * GBK * 8;
          gb += 2 * stride_b;
        }
        kloop_pair<TB>(acc, vo, lb, fr0, ga, gb, ga + GBK * 8, gb + stride_b, ldsw);
        // the last MFMAs' results, before anything but an accumulating MFMA touches them
        asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");
        t = f1;  // < T: the C++ tile below redoes tile f1's wait and barrier, which is harmless
      }
    }
    // KL: the lane is opaque per C++ tile, so that what the tile derives from it (fragment
    // offsets, piece addresses) is recomputed here and not kept in registers across kloop_pair
    if constexpr (KL) asm volatile("" : "+v"(ln));
    const int tfr = KL ? ln & 15 : fr, tfk = KL ? ln >> 4 : fk;
    // Tile t has landed: it is the only one in flight, so the wait is always vmcnt(0) and the
    // other branch is never taken.  The test stays, and `mask` below stays written out instead of
    // sharing the run finder's lambda, because only with both does the compiler peel the last
    // K-tile off this loop, which leaves the loop proper without the `more` and partial-tile
    // branches.  With either one simplified it keeps a single copy of the body and the kernels
    // that run this loop end to end lose 2% (16384^3 TN 66.5 -> 65.2, TT 67.4 -> 66.3 TF/s).
    if (min(T - 1 - t, STAGES - 2) == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const bool more = t + 1 < T;  // its pieces go between the MFMAs below (SPREAD_SLICES)

    const double* As = smem + (t % STAGES) * 2 * OPND_ELEMS;
    const double* Bs = As + OPND_ELEMS;
    const int64_t k0 = kbeg + (int64_t)t * GBK;
    // masks only where needed: the last partial K-tile, and K-tiles that straddle the diagonal
    // of a triangular operand (k0 within 128 of the tile's first row / column)
    const bool mask = (partial_last && t == T - 1) || (TRIA && k0 < m0 + GBM && k0 + GBK > m0) ||
                      (TRIB && k0 < n0 + GBN && k0 + GBK > n0);
#pragma unroll
    for (int ks = 0; ks < GBK / 4; ++ks) {
      const int k = ks * 4 + tfk;
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = wm * 64 + i * 16 + tfr;
        a[i] = As[frag_off<A_KC>(r, k)];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = wn * 64 + j * 16 + tfr;
        b[j] = Bs[frag_off<B_KC>(c, k)];
      }
      if (mask) {
        const int64_t gk = k0 + k;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int64_t gm = m0 + wm * 64 + i * 16 + tfr;
          if (gk >= kend || (TRIA && (TA ? gm > gk : gk > gm))) a[i] = 0.0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t gn = n0 + wn * 64 + j * 16 + tfr;
          if (gk >= kend || (TRIB && (TB ? gk > gn : gn > gk))) b[j] = 0.0;
        }
      }
      if (more && ks < SPREAD_SLICES) {
#pragma unroll
        for (int q = 0; q < WAVE_PIECES / SPREAD_SLICES; ++q)
          issue_piece(t + 1, ks * (WAVE_PIECES / SPREAD_SLICES) + q);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }

  // KL: the epilogue derives its lane and wave indices afresh, so that they do not occupy
  // registers across kloop_pair
  int et = threadIdx.x;
  if constexpr (KL) asm volatile("" : "+v"(et));
  const int efr = KL ? et & 15 : fr, efk = KL ? (et & 63) >> 4 : fk;
  const int ewm = KL ? et >> 7 : wm, ewn = KL ? (et >> 6) & 1 : wn;
  const bool lower = p.uplo_c == VGPOSP_LOWER;
  // 32-bit per-lane offsets in the batched epilogue: 128 rows of a leading dimension below 2^21
  bool batched = p.epilogue != 0 && (p.nsplit > 1 ? p.n : p.ldc) < (1 << 21);
  // whole inside C and, for a lower C, strictly below the diagonal
  const bool inner = m0 + GBM <= p.m && n0 + GBN <= p.n && !(lower && ti == tj);
  if (MULTI) {
    // (the Strassen products have no edge tiles: m and n are multiples of 128)
    if (!inner) batched = false;
#pragma unroll
    for (int d = 0; d < GEMM_XDST; ++d)
      if (d < xd->n && xd->ld[d] >= (1 << 21)) batched = false;
  }
  if (!batched) {
    // the element-wise reference: every test and the memory round trip once per element
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t col = n0 + ewn * 64 + j * 16 + efr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t row = m0 + ewm * 64 + i * 16 + efk + 4 * r;
          if (row < p.m && col < p.n && (!lower || col <= row)) {
            if (p.nsplit > 1) {
              p.part[bz * p.sP + (int64_t)zsplit * p.m * p.n + row * p.n + col] = p.alpha * acc[i][j][r];
              continue;
            }
            double* c = p.C + bz * p.sC + row * p.ldc + col;
            double v = p.alpha * acc[i][j][r];
            if (p.beta != 0.0) v += p.beta * *c;
            *c = v;
            if (MULTI) {
#pragma unroll
              for (int d = 0; d < GEMM_XDST; ++d) {
                if (d < xd->n) {
                  double* c2 = xd->C[d] + row * xd->ld[d] + col;
                  double v2 = xd->alpha[d] * acc[i][j][r];
                  if (xd->beta[d] != 0.0) v2 += xd->beta[d] * *c2;
                  *c2 = v2;
                }
              }
            }
          }
        }
      }
    }
    return;
  }

  // The batched epilogue (epi_group above).  Everything wave-uniform is decided here, once per
  // tile: partial or C, the destinations and their beta, and whether the tile is interior.
  const int lr = ewm * 64 + efk, lc = ewn * 64 + efr;
  const int64_t rows = p.m - m0, cols = p.n - n0;
  const bool diag = lower && ti == tj;
  if (p.nsplit > 1) {  // the split's partial: alpha acc, row stride n
    double* const org = p.part + bz * p.sP + (int64_t)zsplit * p.m * p.n + m0 * p.n + n0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (inner) epi_group<true>(acc[i], org, p.n, p.alpha, 0.0, lr + 16 * i, lc, rows, cols, diag);
      else epi_group<false>(acc[i], org, p.n, p.alpha, 0.0, lr + 16 * i, lc, rows, cols, diag);
    }
    return;
  }
  double* const org = p.C + bz * p.sC + m0 * p.ldc + n0;
  if (inner) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      epi_group<true>(acc[i], org, p.ldc, p.alpha, p.beta, lr + 16 * i, lc, rows, cols, diag);
      if (MULTI) {
#pragma unroll
        for (int d = 0; d < GEMM_XDST; ++d)
          if (d < xd->n)
            epi_group<true>(acc[i], xd->C[d] + m0 * xd->ld[d] + n0, xd->ld[d], xd->alpha[d],
                            xd->beta[d], lr + 16 * i, lc, rows, cols, diag);
      }
    }
  } else if (!MULTI) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      epi_group<false>(acc[i], org, p.ldc, p.alpha, p.beta, lr + 16 * i, lc, rows, cols, diag);
  }
}

template <bool TA, bool TB, bool TRIA, bool TRIB, bool KL = false>
__global__ __launch_bounds__(64 * GEMM_WAVES, GEMM_OCC) void gemm_glds_kernel(
    GemmParams p, int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(16))) double smem[GLDS_SMEM_ELEMS];
  gemm_glds_body<TA, TB, TRIA, TRIB, false, KL>(p, tiles_m, tiles_n, blockIdx.x, gridDim.x,
                                                blockIdx.y, smem);
}

// The plain product with extra destinations (gemm_strassen): same tiles, ring and K loop.
template <bool TA, bool TB, bool KL = false>
__global__ __launch_bounds__(64 * GEMM_WAVES, GEMM_OCC) void gemm_glds_multi_kernel(
    GemmParams p, GemmExtra x, int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(16))) double smem[GLDS_SMEM_ELEMS];
  gemm_glds_body<TA, TB, false, false, true, KL>(p, tiles_m, tiles_n, blockIdx.x, gridDim.x, 0,
                                                 smem, &x);
}

// Grouped launch: up to GROUP_MAX independent problems (each its own shape, operands, flags and
// split-K) in ONE launch, problem g on blockIdx.y.  For the latency-bound M x M products of the
// VGP step, which each fill a few dozen CUs: one launch instead of one per product.
constexpr int GROUP_MAX = 8;
struct GemmGroup {
  GemmParams p[GROUP_MAX];
  int tiles_m[GROUP_MAX], tiles_n[GROUP_MAX], nwg[GROUP_MAX];
  int flags[GROUP_MAX];  // bit 0 transa, 1 transb, 2 tri_a, 3 tri_b
};

__global__ __launch_bounds__(64 * GEMM_WAVES, GEMM_OCC) void gemm_group_kernel(GemmGroup gg) {
  __shared__ __attribute__((aligned(16))) double smem[GLDS_SMEM_ELEMS];
  const int g = blockIdx.y;
  const int bid = blockIdx.x, nwg = gg.nwg[g];
  if (bid >= nwg) return;
  // a copy, read once: the sixteen bodies then use scalars of their own and gg itself has few
  // enough uses to stay in the kernel-argument segment (the compiler otherwise copies all of it
  // to scratch to index it by g)
  const GemmParams p = gg.p[g];
  const int tm = gg.tiles_m[g], tn = gg.tiles_n[g];
#define VG_GROUP_CASE(F)                                                                      \
  case F:                                                                                   \
    gemm_glds_body<(F & 1) != 0, (F & 2) != 0, (F & 4) != 0, (F & 8) != 0>(p, tm, tn, bid,   \
                                                                          nwg, 0, smem);    \
    break;
  switch (gg.flags[g]) {
    VG_GROUP_CASE(0) VG_GROUP_CASE(1) VG_GROUP_CASE(2) VG_GROUP_CASE(3)
    VG_GROUP_CASE(4) VG_GROUP_CASE(5) VG_GROUP_CASE(6) VG_GROUP_CASE(7)
    VG_GROUP_CASE(8) VG_GROUP_CASE(9) VG_GROUP_CASE(10) VG_GROUP_CASE(11)
    VG_GROUP_CASE(12) VG_GROUP_CASE(13) VG_GROUP_CASE(14) VG_GROUP_CASE(15)
  }
#undef VG_GROUP_CASE
}

// K loop of the TA = false fast kernels (vgposp_gemm_set_kloop): 0 = the C++ loop, 1 = the
// hand-scheduled interior K-tiles (kloop_pair).  Process-wide, read at launch.  Bit-identical
// results either way.  Default from the 65k step's A/B (DESIGN.md §4 "Hand-scheduled K loop").
static std::atomic<int> g_kloop{VGPOSP_KLOOP_DEFAULT};

// Epilogue of the fast kernels (vgposp_gemm_set_epilogue): 0 = the element-wise reference, 1 = the
// batched one (gemm_glds_body).  Process-wide, read at launch into GemmParams, so one branch per
// tile and no further kernels.  Bit-identical results either way.  Default from the 65k step's
// A/B (DESIGN.md §4 "Batched epilogue").
#ifndef VGPOSP_EPILOGUE_DEFAULT
#define VGPOSP_EPILOGUE_DEFAULT 1
#endif
static std::atomic<int> g_epilogue{VGPOSP_EPILOGUE_DEFAULT};

// The kernel of a launch: every (transa, transb, tri_a, tri_b) combination has its C++-loop
// kernel (the K-range and mask logic is generic in the four flags); the TA = false ones also
// have a hand-scheduled one, taken when g_kloop is set.
static void launch_glds(dim3 g1, hipStream_t stream, const GemmParams& p, int tm, int tn,
                        int transa, int transb, int tri_a, int tri_b) {
  using Kernel = void (*)(GemmParams, int, int);
#define VG_TRI(TA, TB, KL)                                                                \
  gemm_glds_kernel<TA, TB, false, false, KL>, gemm_glds_kernel<TA, TB, true, false, KL>, \
      gemm_glds_kernel<TA, TB, false, true, KL>, gemm_glds_kernel<TA, TB, true, true, KL>
  static const Kernel cxx[16] = {VG_TRI(false, false, false), VG_TRI(false, true, false),
                                 VG_TRI(true, false, false), VG_TRI(true, true, false)};
  static const Kernel kl[8] = {VG_TRI(false, false, true), VG_TRI(false, true, true)};
#undef VG_TRI
  const int f = (transa ? 8 : 0) + (transb ? 4 : 0) + (tri_b ? 2 : 0) + (tri_a ? 1 : 0);
  const bool hand = !transa && g_kloop.load(std::memory_order_relaxed) != 0;
  hipLaunchKernelGGL(hand ? kl[f] : cxx[f], g1, dim3(64 * GEMM_WAVES), 0, stream, p, tm, tn);
}

// C = sum_z part[z] + beta * C over the (lower) output, fixed summation order.
__global__ __launch_bounds__(256) void gemm_splitk_reduce_kernel(int64_t m, int64_t n, int nsplit,
                                                                 const double* part, double beta,
                                                                 double* C, int64_t ldc,
                                                                 int lower, int64_t sP = 0,
                                                                 int64_t sC = 0) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= m * n) return;
  part += blockIdx.y * sP;
  C += blockIdx.y * sC;
  const int64_t row = e / n, col = e - row * n;
  if (lower && col > row) return;
  double v = 0.0;
  for (int z = 0; z < nsplit; ++z) v += part[(int64_t)z * m * n + e];
  double* c = C + row * ldc + col;
  if (beta != 0.0) v += beta * *c;
  *c = v;
}

// The split-K reduction of a grouped launch: problem g on blockIdx.y (no-op where unsplit).
struct ReduceGroup {
  int64_t m[GROUP_MAX], n[GROUP_MAX], ldc[GROUP_MAX];
  const double* part[GROUP_MAX];
  double* C[GROUP_MAX];
  double beta[GROUP_MAX];
  int nsplit[GROUP_MAX], lower[GROUP_MAX];
};

__global__ __launch_bounds__(256) void gemm_splitk_reduce_group_kernel(ReduceGroup r) {
  const int g = blockIdx.y;
  if (r.nsplit[g] <= 1) return;
  const int64_t m = r.m[g], n = r.n[g];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= m * n) return;
  const int64_t row = e / n, col = e - row * n;
  if (r.lower[g] && col > row) return;
  double v = 0.0;
  for (int z = 0; z < r.nsplit[g]; ++z) v += r.part[g][(int64_t)z * m * n + e];
  double* c = r.C[g] + row * r.ldc[g] + col;
  if (r.beta[g] != 0.0) v += r.beta[g] * *c;
  *c = v;
}

// y = alpha * A x + beta * y for a single output column (C = A B with n == 1): one wave per row,
// HBM-bound (reads A once).  x is B's only column (stride ldb_x elements).
__global__ __launch_bounds__(256) void gemv_rows_kernel(int64_t m, int64_t k, double alpha,
                                                        const double* A, int64_t lda,
                                                        const double* x, int64_t incx, double beta,
                                                        double* y, int64_t incy, int tri) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= m) return;
  if (tri) k = min(k, r + 1);  // stored lower triangular: A[r][c] = 0 for c > r
  const double* row = A + r * lda;
  double s0 = 0.0, s1 = 0.0;
  int64_t c = lane;
  for (; c + 64 < k; c += 128) {
    s0 += row[c] * x[c * incx];
    s1 += row[c + 64] * x[(c + 64) * incx];
  }
  if (c < k) s0 += row[c] * x[c * incx];
  const double s = wave_sum(s0 + s1);
  if (lane == 0) {
    double v = alpha * s;
    if (beta != 0.0) v += beta * y[r * incy];
    y[r * incy] = v;
  }
}

// Split-K GEMV: wave (row r, split z) writes part[z][r]; then gemv_reduce.  For a few rows and a
// long K (c = Kzx y of the VGP: 512 rows x 262,144) one wave per row leaves most CUs idle.
__global__ __launch_bounds__(256) void gemv_rows_split_kernel(int64_t m, int64_t k, int64_t kchunk,
                                                              const double* A, int64_t lda,
                                                              const double* x, int64_t incx,
                                                              double* part, int tri) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= m) return;
  const int64_t k0 = (int64_t)blockIdx.y * kchunk, k1 = min(tri ? min(k, r + 1) : k, k0 + kchunk);
  const double* row = A + r * lda;
  double s0 = 0.0, s1 = 0.0;
  int64_t c = k0 + lane;
  for (; c + 64 < k1; c += 128) {
    s0 += row[c] * x[c * incx];
    s1 += row[c + 64] * x[(c + 64) * incx];
  }
  if (c < k1) s0 += row[c] * x[c * incx];
  const double s = wave_sum(s0 + s1);
  if (lane == 0) part[(int64_t)blockIdx.y * m + r] = s;
}

// y = alpha A^T x (+ beta y) with A stored k x m (row-major): thread j owns output j, the k rows
// it walks are read coalesced across the workgroup.  Split over k when part != null.
__global__ __launch_bounds__(256) void gemv_t_kernel(int64_t m, int64_t k, int64_t kchunk,
                                                     double alpha, const double* A, int64_t lda,
                                                     const double* x, int64_t incx, double beta,
                                                     double* y, int64_t incy, double* part,
                                                     int tri) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  // tri: A stored k x m lower triangular, A[c][j] = 0 for j > c, so only c >= j contribute
  const int64_t k0 = max((int64_t)blockIdx.y * kchunk, tri ? j : (int64_t)0);
  const int64_t k1 = min(k, (int64_t)blockIdx.y * kchunk + kchunk);
  double s0 = 0.0, s1 = 0.0;
  int64_t c = k0;
  for (; c + 1 < k1; c += 2) {
    s0 += A[c * lda + j] * x[c * incx];
    s1 += A[(c + 1) * lda + j] * x[(c + 1) * incx];
  }
  if (c < k1) s0 += A[c * lda + j] * x[c * incx];
  if (part) {
    part[(int64_t)blockIdx.y * m + j] = s0 + s1;
  } else {
    double v = alpha * (s0 + s1);
    if (beta != 0.0) v += beta * y[j * incy];
    y[j * incy] = v;
  }
}

__global__ __launch_bounds__(256) void gemv_reduce_kernel(int64_t m, int nsplit, const double* part,
                                                          double alpha, double beta, double* y,
                                                          int64_t incy) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= m) return;
  double s = 0.0;
  for (int z = 0; z < nsplit; ++z) s += part[(int64_t)z * m + r];
  double v = alpha * s;
  if (beta != 0.0) v += beta * y[r * incy];
  y[r * incy] = v;
}

// splits for the n == 1 paths: about 8192 (rows) / 4096 (transposed) waves in flight, >= 1024
// (rows) / 32 (transposed) K elements per split.  Short per-thread chains matter more than the
// partials: the VGP step's M x M triangular L^-T x (m = 512, k <= 512) ran 41 us on 2 workgroups
// of 256-long serial sums, its Kzb^T v (32,768 x 512) at 2.1 TB/s.
static int gemv_splits(int64_t m, int64_t k, int transa) {
  int64_t s = transa ? ceil_div(4096 * 64, std::max<int64_t>(m, 1)) : ceil_div(8192, m);
  s = std::min<int64_t>(s, transa ? k / 32 : k / 1024);
  return (int)std::max<int64_t>(std::min<int64_t>(s, 4096), 1);
}

static bool aligned16(const void* ptr, int64_t ld) {
  return (reinterpret_cast<uintptr_t>(ptr) % 16 == 0) && (ld % 2 == 0);
}

// "gemm_f64[nt|nn|tn|tt][,triA][,triB][,narrow]": narrow = fewer than 512 workgroups (less than
// two per CU: the recursion's small levels, latency-bound)
static const char* gemm_class_name(int ta, int tb, int tra, int trb, bool wide) {
  static const char* names[32] = {
#define VG_CLS(L, T) "gemm_f64[" L T "]", "gemm_f64[" L T ",narrow]"
      VG_CLS("nn", ""), VG_CLS("nn", ",triA"), VG_CLS("nn", ",triB"), VG_CLS("nn", ",triA,triB"),
      VG_CLS("nt", ""), VG_CLS("nt", ",triA"), VG_CLS("nt", ",triB"), VG_CLS("nt", ",triA,triB"),
      VG_CLS("tn", ""), VG_CLS("tn", ",triA"), VG_CLS("tn", ",triB"), VG_CLS("tn", ",triA,triB"),
      VG_CLS("tt", ""), VG_CLS("tt", ",triA"), VG_CLS("tt", ",triB"), VG_CLS("tt", ",triA,triB"),
#undef VG_CLS
  };
  const int lay = (ta ? 2 : 0) + (tb ? 1 : 0);
  const int tri = (tra ? 1 : 0) + (trb ? 2 : 0);
  return names[(lay * 4 + tri) * 2 + (wide ? 0 : 1)];
}

// The launch plan of one problem (a batch of `batch` at p's strides): which kernel takes it, the
// fast kernel's tile grid, and the algorithmic flops / bytes recorded for it.
struct GemmPlan {
  int va, vb;           // A / B readable with 16-byte loads (aligned, even ld and batch stride)
  bool fast;            // the fast kernel takes it: both of those, and m, n, k even with k > 0
  int tm, tn;           // output tiles per column / row
  int64_t nblk;         // output tiles in all (lower: of the triangle)
  double outs;          // output elements per matrix
  double flops, bytes;  // a triangular operand halves the useful products
};

// Also fills p's split-K fields when the fast kernel takes p split (nsplit > 1, partials at part),
// and its epilogue setting.
static GemmPlan gemm_plan(GemmParams& p, int batch, int nsplit, double* part) {
  GemmPlan pl{};
  p.epilogue = g_epilogue.load(std::memory_order_relaxed);
  pl.va = aligned16(p.A, p.lda) && (batch == 1 || p.sA % 2 == 0);
  pl.vb = aligned16(p.B, p.ldb) && (batch == 1 || p.sB % 2 == 0);
  pl.fast = pl.va && pl.vb && (p.m % 2 == 0) && (p.n % 2 == 0) && (p.k % 2 == 0) && p.k > 0;
  const bool lower = p.uplo_c == VGPOSP_LOWER;
  const double m = (double)p.m, n = (double)p.n, k = (double)p.k;
  pl.tm = (int)ceil_div(p.m, GBM);
  pl.tn = (int)ceil_div(p.n, GBN);
  pl.nblk = lower ? (int64_t)pl.tm * (pl.tm + 1) / 2 : (int64_t)pl.tm * pl.tn;
  pl.outs = lower ? 0.5 * m * (double)(p.m + 1) : m * n;
  pl.flops = 2.0 * batch * k * pl.outs *
             ((p.tri_a && p.tri_b) ? (1.0 / 3.0) : (p.tri_a || p.tri_b) ? 0.5 : 1.0);
  pl.bytes = 8.0 * batch * (m * k + k * n + (p.beta != 0.0 ? 2.0 : 1.0) * pl.outs);
  if (pl.fast && nsplit > 1 && part != nullptr) {
    p.nblk = (int)pl.nblk;
    p.kchunk = ceil_div(ceil_div(p.k, nsplit), GBK) * GBK;
    p.nsplit = (int)ceil_div(p.k, p.kchunk);
    p.part = part;
  }
  return pl;
}

int gemm_launch_batched(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                        const double* A, int64_t lda, int64_t sA, const double* B, int64_t ldb,
                        int64_t sB, double beta, double* C, int64_t ldc, int64_t sC, int uplo_c,
                        int tri_a, int tri_b, int nsplit, double* part, int64_t sP, int batch,
                        hipStream_t stream) {
  if (m <= 0 || n <= 0 || batch <= 0) return 0;
  if (n == 1 && !tri_b && uplo_c == VGPOSP_FULL && k > 0 && batch > 1) {
    for (int b = 0; b < batch; ++b) {
      int rc = gemm_launch_batched(transa, transb, m, n, k, alpha, A + b * sA, lda, 0, B + b * sB,
                                   ldb, 0, beta, C + b * sC, ldc, 0, uplo_c, tri_a, tri_b, nsplit,
                                   part ? part + b * sP : nullptr, 0, 1, stream);
      if (rc) return rc;
    }
    return 0;
  }
  if (n == 1 && !tri_b && uplo_c == VGPOSP_FULL && k > 0) {
    ProfScope ps("gemv_f64", stream, 2.0 * (double)m * k, 8.0 * ((double)m * k + k + 2.0 * m));
    const int64_t incx = transb ? 1 : ldb;
    const int S = (nsplit > 1 && part != nullptr) ? nsplit : 1;
    const int64_t kchunk = ceil_div(k, S);
    if (!transa) {
      if (S == 1) {
        hipLaunchKernelGGL(gemv_rows_kernel, dim3((unsigned)ceil_div(m, 4)), dim3(256), 0, stream, m,
                           k, alpha, A, lda, B, incx, beta, C, ldc, tri_a);
      } else {
        hipLaunchKernelGGL(gemv_rows_split_kernel, dim3((unsigned)ceil_div(m, 4), (unsigned)S),
                           dim3(256), 0, stream, m, k, kchunk, A, lda, B, incx, part, tri_a);
      }
    } else {
      hipLaunchKernelGGL(gemv_t_kernel, dim3((unsigned)ceil_div(m, 256), (unsigned)S), dim3(256), 0,
                         stream, m, k, kchunk, alpha, A, lda, B, incx, beta, C, ldc,
                         S > 1 ? part : nullptr, tri_a);
    }
    VG_LAUNCH_CHECK();
    if (S > 1) {
      hipLaunchKernelGGL(gemv_reduce_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, stream,
                         m, S, part, alpha, beta, C, ldc);
      VG_LAUNCH_CHECK();
    }
    return 0;
  }
  GemmParams p{m, n, k, alpha, beta, A, lda, B, ldb, C, ldc, uplo_c, tri_a, tri_b, 1, 0, 0, nullptr,
               sA, sB, sC, sP, tl_gemm_abort};
  const GemmPlan pl = gemm_plan(p, batch, nsplit, part);
  if (pl.fast) {
    // recorded under its layout class; vgposp_prof_query("gemm_f64") sums the classes
    ProfScope ps(gemm_class_name(transa, transb, tri_a, tri_b, pl.nblk * p.nsplit * batch >= 512),
                 stream, pl.flops, pl.bytes);
    dim3 g1((unsigned)(pl.nblk * p.nsplit), (unsigned)batch);
    launch_glds(g1, stream, p, pl.tm, pl.tn, transa, transb, tri_a, tri_b);
    VG_LAUNCH_CHECK();
    if (p.nsplit > 1) {
      hipLaunchKernelGGL(gemm_splitk_reduce_kernel, dim3((unsigned)ceil_div(m * n, 256), (unsigned)batch),
                         dim3(256), 0, stream, m, n, p.nsplit, part, beta, C, ldc,
                         uplo_c == VGPOSP_LOWER, sP, sC);
      VG_LAUNCH_CHECK();
    }
    return 0;
  }
  dim3 grid((unsigned)pl.tn, (unsigned)pl.tm, (unsigned)batch);
  ProfScope ps("gemm_f64", stream, 2.0 * batch * (double)k * pl.outs, pl.bytes);
  using Kernel = void (*)(GemmParams, int, int);
  static const Kernel ref[4] = {gemm_ref_kernel<false, false>, gemm_ref_kernel<false, true>,
                                gemm_ref_kernel<true, false>, gemm_ref_kernel<true, true>};
  hipLaunchKernelGGL(ref[2 * !!transa + !!transb], grid, dim3(256), 0, stream, p, pl.va, pl.vb);
  VG_LAUNCH_CHECK();
  return 0;
}

int gemm_launch_split(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                      const double* A, int64_t lda, const double* B, int64_t ldb, double beta,
                      double* C, int64_t ldc, int uplo_c, int tri_a, int tri_b, int nsplit,
                      double* part, hipStream_t stream) {
  return gemm_launch_batched(transa, transb, m, n, k, alpha, A, lda, 0, B, ldb, 0, beta, C, ldc, 0,
                             uplo_c, tri_a, tri_b, nsplit, part, 0, 1, stream);
}

int gemm_launch(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                const double* A, int64_t lda, const double* B, int64_t ldb, double beta,
                double* C, int64_t ldc, int uplo_c, int tri_a, int tri_b, hipStream_t stream) {
  return gemm_launch_split(transa, transb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, uplo_c,
                           tri_a, tri_b, 1, nullptr, stream);
}

// Minimum depth of a short-K split (vgposp_gemm_set_split_depth).  Set explicitly by the caller,
// never from the environment: every workspace query and the launch that uses the workspace read
// the same value as long as the caller does not change it in between (round 3 read it from
// the environment on every launch, while tools/vgp_ab.py rewrote it between variants).
static std::atomic<int> g_split_min_k{16};

// Split count for a launch with few output tiles and a long K: enough workgroups for 256 CUs
// (about two per CU), each split at least 512 deep.
int gemm_auto_splits(int64_t m, int64_t n, int64_t k, int uplo_c, int transa) {
  if (n == 1 && uplo_c == VGPOSP_FULL) return gemv_splits(m, k, transa);
  const int64_t tm = ceil_div(m, GBM), tn = ceil_div(n, GBN);
  const int64_t nblk = uplo_c == VGPOSP_LOWER ? tm * (tm + 1) / 2 : tm * tn;
  // one full round of workgroup slots (256 CUs x 2 workgroups): the splits all run the same K
  // length, so a round that overflows by a few workgroups costs a whole second round (measured:
  // 10 lower tiles x 52 splits = 520 > 512 ran as slowly as the 16-tile full product)
  int64_t s = 512 / nblk;
  // long K: splits at least 512 deep.  Short K (few output tiles, e.g. the M x M products of the
  // VGP step, 16 tiles of a 512^3 product on 16 CUs, and the Cholesky recursion's 128..1024
  // levels): up to 8 splits, at least 16 deep (one K-tile).  Measured against 64 deep (the
  // VGPOSP_SPLIT_MIN_K override, profiles/r3_vgp_ab_streams_splitk_*.jsonl): C3 6.30 -> 6.19 ms,
  // C5 7.32 -> 7.26 ms, the 65k step unchanged (16.27 vs 16.30 placements/s): a split's partial
  // costs less than the serial K-steps it removes from a latency-bound chain.
  const int64_t deep = k / 512;
  const int64_t min_k = g_split_min_k.load(std::memory_order_relaxed);
  s = std::min<int64_t>(s, deep >= 8 ? deep : std::min<int64_t>(8, k / min_k));
  return (int)std::max<int64_t>(s, 1);
}

// Partial elements problem g of a group needs (0 when it runs unsplit or off the fast kernel).
static int64_t group_part_elems(int transa, int64_t m, int64_t n, int64_t k, int uplo_c) {
  if (m <= 0 || n <= 0 || k <= 0 || n == 1) return 0;
  const int sp = gemm_auto_splits(m, n, k, uplo_c, transa);
  return sp > 1 ? (int64_t)sp * m * n : 0;
}

// `count` independent GEMMs (flags[5 g ..]: transa, transb, uplo_c, tri_a, tri_b; dims[3 g ..]:
// m, n, k): every problem the fast kernel takes runs in ONE grouped launch (+ one grouped split-K
// reduction), the others (GEMV shapes, unaligned or odd operands) one by one.
int gemm_launch_group(int count, const int* flags, const int64_t* dims, const double* alpha,
                      const double* beta, const double* const* A, const int64_t* lda,
                      const double* const* B, const int64_t* ldb, double* const* C,
                      const int64_t* ldc, double* part, hipStream_t s) {
  GemmGroup gg{};
  ReduceGroup rg{};
  int ng = 0, maxwg = 0;
  int64_t poff = 0, maxel = 0;
  double fl = 0.0, by = 0.0;
  for (int g = 0; g < count; ++g) {
    const int ta = flags[5 * g], tb = flags[5 * g + 1], up = flags[5 * g + 2];
    const int tra = flags[5 * g + 3], trb = flags[5 * g + 4];
    const int64_t m = dims[3 * g], n = dims[3 * g + 1], k = dims[3 * g + 2];
    if (m <= 0 || n <= 0) continue;
    const int64_t pe = group_part_elems(ta, m, n, k, up);
    GemmParams p{m, n, k, alpha[g], beta[g], A[g], lda[g], B[g], ldb[g], C[g], ldc[g], up, tra, trb,
                 1, 0, 0, nullptr, 0, 0, 0, 0, tl_gemm_abort};
    const int sp = pe > 0 ? (int)(pe / (m * n)) : 1;
    const GemmPlan pl = gemm_plan(p, 1, sp, part + poff);
    if (!pl.fast || ng == GROUP_MAX) {
      if (int rc = gemm_launch_split(ta, tb, m, n, k, alpha[g], A[g], lda[g], B[g], ldb[g], beta[g],
                                     C[g], ldc[g], up, tra, trb, sp,
                                     pe > 0 ? part + poff : nullptr, s))
        return rc;
      poff += pe;
      continue;
    }
    poff += pe;
    fl += pl.flops;
    by += pl.bytes;
    gg.p[ng] = p;
    gg.tiles_m[ng] = pl.tm;
    gg.tiles_n[ng] = pl.tn;
    gg.nwg[ng] = (int)(pl.nblk * p.nsplit);
    gg.flags[ng] = (ta ? 1 : 0) | (tb ? 2 : 0) | (tra ? 4 : 0) | (trb ? 8 : 0);
    maxwg = std::max(maxwg, gg.nwg[ng]);
    rg.m[ng] = m;
    rg.n[ng] = n;
    rg.ldc[ng] = ldc[g];
    rg.part[ng] = p.part;
    rg.C[ng] = C[g];
    rg.beta[ng] = beta[g];
    rg.nsplit[ng] = p.nsplit;
    rg.lower[ng] = up == VGPOSP_LOWER;
    if (p.nsplit > 1) maxel = std::max(maxel, m * n);
    ++ng;
  }
  if (ng == 0) return 0;
  {
    ProfScope ps("gemm_f64", s, fl, by);
    hipLaunchKernelGGL(gemm_group_kernel, dim3((unsigned)maxwg, (unsigned)ng), dim3(256), 0, s, gg);
    VG_LAUNCH_CHECK();
  }
  if (maxel > 0) {
    hipLaunchKernelGGL(gemm_splitk_reduce_group_kernel, dim3((unsigned)ceil_div(maxel, 256), (unsigned)ng),
                       dim3(256), 0, s, rg);
    VG_LAUNCH_CHECK();
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Strassen for large plain products: one or two levels of the classic seven-product form on
// op(A) op(B), in native fp64.  With the quadrants X11 X12 / X21 X22:
//   M1 = (A11 + A22)(B11 + B22)  -> C11 + , C22 +      M5 = (A11 + A12) B22  -> C11 - , C12 +
//   M2 = (A21 + A22) B11         -> C21 + , C22 -      M6 = (A21 - A11)(B11 + B12)  -> C22 +
//   M3 = A11 (B12 - B22)         -> C12 + , C22 +      M7 = (A12 - A22)(B21 + B22)  -> C11 +
//   M4 = A22 (B21 - B11)         -> C11 + , C21 +
// Each product is ONE launch whose epilogue accumulates into every quadrant it belongs to
// (gemm_glds_multi_kernel), so there are no C-side temporaries or sums: the first product that
// touches a quadrant carries the caller's beta, later ones beta = 1.  The ten operand sums of a
// level go through one A-side and one B-side temporary (strassen_add_kernel).  A second level
// splits each of the seven products again; its products then land in up to four places.
// Everything is enqueued on one stream in a fixed order: results are deterministic.
// Eligible: m, n, k multiples of 256 and >= min_dim, 16-byte aligned operands with even leading
// dimensions.  Anything else is the single classical launch, bit-identical to gemm_launch.
// ---------------------------------------------------------------------------------------------
struct GemmDst {
  double* C;
  int64_t ld;
  double alpha, beta;
};

// D = X + sgn Y on rows x cols (cols a multiple of 128), 16-byte accesses: a wave covers 1 KiB of
// one row, a thread four rows (its loads issued together).
__global__ __launch_bounds__(256) void strassen_add_kernel(int64_t rows, const double* X, int64_t ldx,
                                                          const double* Y, int64_t ldy, double sgn,
                                                          double* D, int64_t ldd, const int* abort) {
  if (abort != nullptr && *abort != 0) return;
  const int64_t c = ((int64_t)blockIdx.x * 64 + threadIdx.x) * 2;
  const int64_t r0 = (int64_t)blockIdx.y * 16 + threadIdx.y;
  double2 xv[4], yv[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t r = min(r0 + 4 * u, rows - 1);
    xv[u] = *reinterpret_cast<const double2*>(X + r * ldx + c);
    yv[u] = *reinterpret_cast<const double2*>(Y + r * ldy + c);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t r = r0 + 4 * u;
    if (r < rows)
      *reinterpret_cast<double2*>(D + r * ldd + c) =
          make_double2(xv[u].x + sgn * yv[u].x, xv[u].y + sgn * yv[u].y);
  }
}

static int strassen_add(int64_t rows, int64_t cols, const double* X, int64_t ldx, const double* Y,
                        int64_t ldy, double sgn, double* D, int64_t ldd, hipStream_t s) {
  ProfScope ps("strassen_add", s, (double)rows * cols, 24.0 * (double)rows * cols);
  hipLaunchKernelGGL(strassen_add_kernel, dim3((unsigned)(cols / 128), (unsigned)ceil_div(rows, 16)),
                     dim3(64, 4), 0, s, rows, X, ldx, Y, ldy, sgn, D, ldd, tl_gemm_abort);
  VG_LAUNCH_CHECK();
  return 0;
}

// Process-wide Strassen setting of the fused Cholesky + inverse (vgposp_potrf_set_strassen) and
// the size threshold of vgposp_gemm_strassen.  Like the split depth above: set explicitly, never
// from the environment, and only between a workspace query and its use, consistently.
// Defaults from the 65k step's A/B (DESIGN.md §4 "Strassen", profiles/strassen_ab.json): 8192 / 2
// levels 2,862 ms, 8192 / 1 2,902, 16384 / 1 or 2 2,951, classical 3,067.
static std::atomic<int64_t> g_strassen_min_dim{8192};
static std::atomic<int> g_strassen_levels{2};

static bool strassen_dims_ok(int64_t m, int64_t n, int64_t k, int64_t min_dim) {
  return m % 256 == 0 && n % 256 == 0 && k % 256 == 0 && m >= min_dim && n >= min_dim &&
         k >= min_dim && std::max({m, n, k}) / 32 <= 65535;  // (the add kernel's grid.y)
}

// Doubles of operand temporaries: one A-side and one B-side per level actually taken.
int64_t gemm_strassen_ws_elems(int64_t m, int64_t n, int64_t k, int levels, int64_t min_dim) {
  int64_t e = 0;
  for (; levels > 0 && strassen_dims_ok(m, n, k, min_dim); --levels) {
    m /= 2, n /= 2, k /= 2;
    e += m * k + k * n;
  }
  return e;
}

// One classical launch of op(A) op(B) into nd destinations.
static int gemm_launch_multi(int transa, int transb, int64_t m, int64_t n, int64_t k,
                             const double* A, int64_t lda, const double* B, int64_t ldb,
                             const GemmDst* d, int nd, hipStream_t stream) {
  if (nd == 1)
    return gemm_launch(transa, transb, m, n, k, d[0].alpha, A, lda, B, ldb, d[0].beta, d[0].C,
                       d[0].ld, VGPOSP_FULL, 0, 0, stream);
  GemmParams p{m, n, k, d[0].alpha, d[0].beta, A, lda, B, ldb, d[0].C, d[0].ld, VGPOSP_FULL, 0, 0,
               1, 0, 0, nullptr, 0, 0, 0, 0, tl_gemm_abort};
  GemmExtra x{};
  x.n = nd - 1;
  double outs = d[0].beta != 0.0 ? 2.0 : 1.0;
  for (int i = 1; i < nd; ++i) {
    x.C[i - 1] = d[i].C;
    x.ld[i - 1] = d[i].ld;
    x.alpha[i - 1] = d[i].alpha;
    x.beta[i - 1] = d[i].beta;
    outs += d[i].beta != 0.0 ? 2.0 : 1.0;
  }
  const GemmPlan pl = gemm_plan(p, 1, 1, nullptr);
  const int tm = pl.tm, tn = pl.tn;
  const int64_t nblk = pl.nblk;
  // the flops of the launch actually made (a Strassen product is a smaller classical product)
  ProfScope ps(gemm_class_name(transa, transb, 0, 0, nblk >= 512), stream,
               2.0 * (double)m * (double)n * (double)k,
               8.0 * ((double)m * k + (double)k * n + outs * (double)m * n));
  using Kernel = void (*)(GemmParams, GemmExtra, int, int);
  static const Kernel cxx[4] = {gemm_glds_multi_kernel<false, false>, gemm_glds_multi_kernel<false, true>,
                                gemm_glds_multi_kernel<true, false>, gemm_glds_multi_kernel<true, true>};
  static const Kernel kl[2] = {gemm_glds_multi_kernel<false, false, true>,
                               gemm_glds_multi_kernel<false, true, true>};
  const int f = (transa ? 2 : 0) + (transb ? 1 : 0);
  const bool hand = !transa && g_kloop.load(std::memory_order_relaxed) != 0;
  hipLaunchKernelGGL(hand ? kl[f] : cxx[f], dim3((unsigned)nblk), dim3(64 * GEMM_WAVES), 0, stream,
                     p, x, tm, tn);
  VG_LAUNCH_CHECK();
  return 0;
}

// An operand of a Strassen product: quadrant x, or quadrant x + sgn * quadrant y (y >= 0).
struct StrassenOpnd {
  int x, y;
  double sgn;
};
struct StrassenProd {
  StrassenOpnd a, b;
  int nq;        // quadrants of C the product lands in
  int q[2];      // 2 i + j
  double s[2];   // its sign there
};
static const StrassenProd STRASSEN[7] = {
    {{0, 3, 1.0}, {0, 3, 1.0}, 2, {0, 3}, {1.0, 1.0}},    // M1
    {{2, 3, 1.0}, {0, -1, 0.0}, 2, {2, 3}, {1.0, -1.0}},  // M2
    {{0, -1, 0.0}, {1, 3, -1.0}, 2, {1, 3}, {1.0, 1.0}},  // M3
    {{3, -1, 0.0}, {2, 0, -1.0}, 2, {0, 2}, {1.0, 1.0}},  // M4
    {{0, 1, 1.0}, {3, -1, 0.0}, 2, {0, 1}, {-1.0, 1.0}},  // M5
    {{2, 0, -1.0}, {0, 1, 1.0}, 1, {3, 3}, {1.0, 0.0}},   // M6
    {{1, 3, -1.0}, {2, 3, 1.0}, 1, {0, 0}, {1.0, 0.0}},   // M7
};

static int strassen_rec(int transa, int transb, int64_t m, int64_t n, int64_t k, const double* A,
                        int64_t lda, const double* B, int64_t ldb, const GemmDst* dst, int nd,
                        int levels, int64_t min_dim, double* ws, hipStream_t s) {
  if (levels <= 0 || 2 * nd > 1 + GEMM_XDST || !strassen_dims_ok(m, n, k, min_dim))
    return gemm_launch_multi(transa, transb, m, n, k, A, lda, B, ldb, dst, nd, s);
  const int64_t m2 = m / 2, n2 = n / 2, k2 = k / 2;
  // stored shapes of the operand quadrants (and of the temporaries, packed)
  const int64_t ar = transa ? k2 : m2, ac = transa ? m2 : k2;
  const int64_t br = transb ? n2 : k2, bc = transb ? k2 : n2;
  double* const TA = ws;
  double* const TB = TA + m2 * k2;
  double* const next = TB + k2 * n2;
  // quadrant (i, j) of op(X) sits at block (j, i) of a transposed store
  auto Aq = [&](int q) {
    const int i = q >> 1, j = q & 1;
    return transa ? A + j * ar * lda + i * ac : A + i * ar * lda + j * ac;
  };
  auto Bq = [&](int q) {
    const int i = q >> 1, j = q & 1;
    return transb ? B + j * br * ldb + i * bc : B + i * br * ldb + j * bc;
  };
  bool touched[4] = {false, false, false, false};
  for (const StrassenProd& pr : STRASSEN) {
    int rc;
    const double* a = Aq(pr.a.x);
    int64_t la = lda;
    if (pr.a.y >= 0) {
      if ((rc = strassen_add(ar, ac, a, lda, Aq(pr.a.y), lda, pr.a.sgn, TA, ac, s))) return rc;
      a = TA, la = ac;
    }
    const double* b = Bq(pr.b.x);
    int64_t lb = ldb;
    if (pr.b.y >= 0) {
      if ((rc = strassen_add(br, bc, b, ldb, Bq(pr.b.y), ldb, pr.b.sgn, TB, bc, s))) return rc;
      b = TB, lb = bc;
    }
    GemmDst sub[1 + GEMM_XDST];
    int ns = 0;
    for (int d = 0; d < nd; ++d)
      for (int t = 0; t < pr.nq; ++t) {
        const int q = pr.q[t];
        sub[ns++] = GemmDst{dst[d].C + (q >> 1) * m2 * dst[d].ld + (q & 1) * n2, dst[d].ld,
                            pr.s[t] * dst[d].alpha, touched[q] ? 1.0 : dst[d].beta};
      }
    for (int t = 0; t < pr.nq; ++t) touched[pr.q[t]] = true;
    if ((rc = strassen_rec(transa, transb, m2, n2, k2, a, la, b, lb, sub, ns, levels - 1, min_dim,
                           next, s)))
      return rc;
  }
  return 0;
}

// C = alpha op(A) op(B) + beta C (full C, dense operands) with up to `levels` Strassen levels on
// the products whose m, n and k are all >= min_dim; ws holds gemm_strassen_ws_elems doubles (a
// smaller one means fewer levels).  C must not overlap A or B.
int gemm_strassen(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                  const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C,
                  int64_t ldc, int levels, int64_t min_dim, double* ws, int64_t ws_elems,
                  hipStream_t stream) {
  levels = std::min(levels, 2);
  while (levels > 0 && (ws == nullptr || gemm_strassen_ws_elems(m, n, k, levels, min_dim) > ws_elems))
    --levels;
  const bool ok = levels > 0 && strassen_dims_ok(m, n, k, min_dim) && aligned16(A, lda) &&
                  aligned16(B, ldb) && aligned16(C, ldc) && aligned16(ws, 2);
  if (!ok)
    return gemm_launch(transa, transb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, VGPOSP_FULL, 0,
                       0, stream);
  const GemmDst d{C, ldc, alpha, beta};
  return strassen_rec(transa, transb, m, n, k, A, lda, B, ldb, &d, 1, levels, min_dim, ws, stream);
}

void gemm_strassen_config(int64_t* min_dim, int* levels) {
  *min_dim = g_strassen_min_dim.load(std::memory_order_relaxed);
  *levels = g_strassen_levels.load(std::memory_order_relaxed);
}

void gemm_set_abort(const int* flag) { tl_gemm_abort = flag; }
const int* gemm_abort_flag() { return tl_gemm_abort; }

}  // namespace vgposp

extern "C" int vgposp_gemm_set_abort_flag(const void* flag) {
  vgposp::clear_error();
  vgposp::gemm_set_abort(static_cast<const int*>(flag));
  return 0;
}

extern "C" int vgposp_gemm_set_split_depth(int min_k) {
  using namespace vgposp;
  clear_error();
  VG_CHECK_ARG(min_k >= 16 && min_k <= 4096 && min_k % 16 == 0, 1);
  g_split_min_k.store(min_k, std::memory_order_relaxed);
  return 0;
}

extern "C" int vgposp_gemm_split_depth(void) { return vgposp::g_split_min_k.load(); }

extern "C" int vgposp_gemm_set_kloop(int kloop) {
  using namespace vgposp;
  clear_error();
  VG_CHECK_ARG(kloop == 0 || kloop == 1, 1);
  g_kloop.store(kloop, std::memory_order_relaxed);
  return 0;
}

extern "C" int vgposp_gemm_kloop(void) { return vgposp::g_kloop.load(); }

extern "C" int vgposp_gemm_set_epilogue(int epilogue) {
  using namespace vgposp;
  clear_error();
  VG_CHECK_ARG(epilogue == 0 || epilogue == 1, 1);
  g_epilogue.store(epilogue, std::memory_order_relaxed);
  return 0;
}

extern "C" int vgposp_gemm_epilogue(void) { return vgposp::g_epilogue.load(); }

// The operand checks vgposp_gemm, vgposp_gemm_splitk and vgposp_gemm_strassen share: the same
// arguments at the same positions (vgposp_gemm_batched has its strides in between).
#define VGPOSP_GEMM_CHECK_OPERANDS()                                     \
  VG_CHECK_ARG(m >= 0, 3);                                               \
  VG_CHECK_ARG(n >= 0, 4);                                               \
  VG_CHECK_ARG(k >= 0, 5);                                               \
  VG_CHECK_ARG(A != nullptr || m == 0 || k == 0, 7);                     \
  VG_CHECK_ARG(lda >= (transa ? (m > 0 ? m : 1) : (k > 0 ? k : 1)), 8);  \
  VG_CHECK_ARG(B != nullptr || n == 0 || k == 0, 9);                     \
  VG_CHECK_ARG(ldb >= (transb ? (k > 0 ? k : 1) : (n > 0 ? n : 1)), 10); \
  VG_CHECK_ARG(C != nullptr || m == 0 || n == 0, 12);                    \
  VG_CHECK_ARG(ldc >= (n > 0 ? n : 1), 13)

extern "C" size_t vgposp_gemm_splitk_workspace_bytes(int64_t m, int64_t n, int64_t k, int uplo_c,
                                                     int splits) {
  using namespace vgposp;
  if (m <= 0 || n <= 0 || k <= 0) return 0;
  // the GEMV paths pick their split count by transa, which this query does not take: size for
  // the larger of the two
  if (splits <= 0)
    splits = std::max(gemm_auto_splits(m, n, k, uplo_c, 0), gemm_auto_splits(m, n, k, uplo_c, 1));
  return splits > 1 ? 8 * (size_t)splits * m * n : 0;
}

extern "C" int vgposp_gemm_splitk(int transa, int transb, int64_t m, int64_t n, int64_t k,
                                  double alpha, const double* A, int64_t lda, const double* B,
                                  int64_t ldb, double beta, double* C, int64_t ldc, int uplo_c,
                                  int tri_a, int tri_b, int splits, void* ws, size_t ws_bytes,
                                  void* stream) {
  using namespace vgposp;
  clear_error();
  VGPOSP_GEMM_CHECK_OPERANDS();
  VG_CHECK_ARG(uplo_c == VGPOSP_FULL || (uplo_c == VGPOSP_LOWER && m == n), 14);
  if (m == 0 || n == 0) return 0;
  if (splits <= 0) splits = k > 0 ? gemm_auto_splits(m, n, k, uplo_c, transa) : 1;
  if (splits > 1) {
    const size_t need = 8 * (size_t)splits * m * n;
    if (ws == nullptr || ws_bytes < need) {
      set_error("vgposp_gemm_splitk: workspace %zu < %zu bytes", ws_bytes, need);
      return VGPOSP_E_WS;
    }
  }
  return gemm_launch_split(transa, transb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, uplo_c,
                           tri_a, tri_b, splits, static_cast<double*>(ws), as_stream(stream));
}

extern "C" int vgposp_gemm(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                           const double* A, int64_t lda, const double* B, int64_t ldb,
                           double beta, double* C, int64_t ldc, int uplo_c, int tri_a, int tri_b,
                           void* stream) {
  using namespace vgposp;
  clear_error();
  VGPOSP_GEMM_CHECK_OPERANDS();
  VG_CHECK_ARG(uplo_c == VGPOSP_FULL || (uplo_c == VGPOSP_LOWER && m == n), 14);
  return gemm_launch(transa, transb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, uplo_c, tri_a,
                     tri_b, as_stream(stream));
}

extern "C" int vgposp_potrf_set_strassen(int64_t min_dim, int levels) {
  using namespace vgposp;
  clear_error();
  VG_CHECK_ARG(min_dim >= 256 && min_dim % 256 == 0, 1);
  VG_CHECK_ARG(levels >= 0 && levels <= 2, 2);
  g_strassen_min_dim.store(min_dim, std::memory_order_relaxed);
  g_strassen_levels.store(levels, std::memory_order_relaxed);
  return 0;
}

extern "C" int vgposp_potrf_strassen(int64_t* min_dim, int* levels) {
  using namespace vgposp;
  clear_error();
  VG_CHECK_ARG(min_dim != nullptr, 1);
  VG_CHECK_ARG(levels != nullptr, 2);
  gemm_strassen_config(min_dim, levels);
  return 0;
}

extern "C" size_t vgposp_gemm_strassen_workspace_bytes(int64_t m, int64_t n, int64_t k,
                                                       int levels) {
  using namespace vgposp;
  if (m <= 0 || n <= 0 || k <= 0 || levels <= 0) return 0;
  return 8 * (size_t)gemm_strassen_ws_elems(m, n, k, std::min(levels, 2),
                                            g_strassen_min_dim.load(std::memory_order_relaxed));
}

extern "C" int vgposp_gemm_strassen(int transa, int transb, int64_t m, int64_t n, int64_t k,
                                    double alpha, const double* A, int64_t lda, const double* B,
                                    int64_t ldb, double beta, double* C, int64_t ldc, int levels,
                                    void* ws, size_t ws_bytes, void* stream) {
  using namespace vgposp;
  clear_error();
  VGPOSP_GEMM_CHECK_OPERANDS();
  VG_CHECK_ARG(levels >= 0 && levels <= 2, 14);
  const size_t need = vgposp_gemm_strassen_workspace_bytes(m, n, k, levels);
  if (need > 0 && (ws == nullptr || ws_bytes < need)) {
    set_error("vgposp_gemm_strassen: workspace %zu < %zu bytes", ws_bytes, need);
    return VGPOSP_E_WS;
  }
  return gemm_strassen(transa, transb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, levels,
                       g_strassen_min_dim.load(std::memory_order_relaxed),
                       static_cast<double*>(ws), (int64_t)(ws_bytes / 8), as_stream(stream));
}

extern "C" size_t vgposp_gemm_batched_workspace_bytes(int64_t m, int64_t n, int64_t k, int uplo_c,
                                                      int batch) {
  using namespace vgposp;
  if (m <= 0 || n <= 0 || k <= 0 || batch <= 0 || n == 1) return 0;
  const int sp = gemm_auto_splits(m, n, k, uplo_c, 0);
  return sp > 1 ? 8 * (size_t)sp * m * n * batch : 0;
}

extern "C" int vgposp_gemm_batched(int transa, int transb, int64_t m, int64_t n, int64_t k,
                                   double alpha, const double* A, int64_t lda, int64_t sA,
                                   const double* B, int64_t ldb, int64_t sB, double beta, double* C,
                                   int64_t ldc, int64_t sC, int uplo_c, int tri_a, int tri_b,
                                   int batch, void* ws, size_t ws_bytes, void* stream) {
  using namespace vgposp;
  clear_error();
  VG_CHECK_ARG(m >= 0, 3);
  VG_CHECK_ARG(n >= 0, 4);
  VG_CHECK_ARG(k >= 0, 5);
  VG_CHECK_ARG(A != nullptr || m == 0 || k == 0, 7);
  VG_CHECK_ARG(lda >= (transa ? (m > 0 ? m : 1) : (k > 0 ? k : 1)), 8);
  VG_CHECK_ARG(B != nullptr || n == 0 || k == 0, 10);
  VG_CHECK_ARG(ldb >= (transb ? (k > 0 ? k : 1) : (n > 0 ? n : 1)), 11);
  VG_CHECK_ARG(C != nullptr || m == 0 || n == 0, 14);
  VG_CHECK_ARG(ldc >= (n > 0 ? n : 1), 15);
  VG_CHECK_ARG(uplo_c == VGPOSP_FULL || (uplo_c == VGPOSP_LOWER && m == n), 17);
  VG_CHECK_ARG(batch >= 1 && batch <= 65535, 20);
  if (m == 0 || n == 0) return 0;
  int sp = (k > 0 && n > 1) ? gemm_auto_splits(m, n, k, uplo_c, transa) : 1;
  if (sp > 1 && (ws == nullptr || ws_bytes < 8 * (size_t)sp * m * n * batch)) sp = 1;
  return gemm_launch_batched(transa, transb, m, n, k, alpha, A, lda, sA, B, ldb, sB, beta, C, ldc,
                             sC, uplo_c, tri_a, tri_b, sp, sp > 1 ? static_cast<double*>(ws) : nullptr,
                             (int64_t)sp * m * n, batch, as_stream(stream));
}

extern "C" size_t vgposp_gemm_group_workspace_bytes(int count, const int* flags,
                                                    const int64_t* dims) {
  using namespace vgposp;
  if (count <= 0 || flags == nullptr || dims == nullptr) return 0;
  int64_t el = 0;
  for (int g = 0; g < count; ++g)
    el += group_part_elems(flags[5 * g], dims[3 * g], dims[3 * g + 1], dims[3 * g + 2],
                           flags[5 * g + 2]);
  return 8 * (size_t)el;
}

extern "C" int vgposp_gemm_group(int count, const int* flags, const int64_t* dims,
                                 const double* alpha, const double* beta, const double* const* A,
                                 const int64_t* lda, const double* const* B, const int64_t* ldb,
                                 double* const* C, const int64_t* ldc, void* ws, size_t ws_bytes,
                                 void* stream) {
  using namespace vgposp;
  clear_error();
  VG_CHECK_ARG(count >= 0, 1);
  if (count == 0) return 0;
  VG_CHECK_ARG(flags != nullptr, 2);
  VG_CHECK_ARG(dims != nullptr, 3);
  VG_CHECK_ARG(alpha != nullptr && beta != nullptr, 4);
  VG_CHECK_ARG(A != nullptr && lda != nullptr && B != nullptr && ldb != nullptr, 6);
  VG_CHECK_ARG(C != nullptr && ldc != nullptr, 10);
  for (int g = 0; g < count; ++g) {
    const int ta = flags[5 * g], tb = flags[5 * g + 1], up = flags[5 * g + 2];
    const int64_t m = dims[3 * g], n = dims[3 * g + 1], k = dims[3 * g + 2];
    VG_CHECK_ARG(m >= 0 && n >= 0 && k >= 0, 3);
    VG_CHECK_ARG(up == VGPOSP_FULL || (up == VGPOSP_LOWER && m == n), 2);
    VG_CHECK_ARG(A[g] != nullptr || m == 0 || k == 0, 6);
    VG_CHECK_ARG(lda[g] >= (ta ? (m > 0 ? m : 1) : (k > 0 ? k : 1)), 7);
    VG_CHECK_ARG(B[g] != nullptr || n == 0 || k == 0, 8);
    VG_CHECK_ARG(ldb[g] >= (tb ? (k > 0 ? k : 1) : (n > 0 ? n : 1)), 9);
    VG_CHECK_ARG(C[g] != nullptr || m == 0 || n == 0, 10);
    VG_CHECK_ARG(ldc[g] >= (n > 0 ? n : 1), 11);
  }
  const size_t need = vgposp_gemm_group_workspace_bytes(count, flags, dims);
  if (need > 0 && (ws == nullptr || ws_bytes < need)) {
    set_error("vgposp_gemm_group: workspace %zu < %zu bytes", ws_bytes, need);
    return VGPOSP_E_WS;
  }
  return gemm_launch_group(count, flags, dims, alpha, beta, A, lda, B, ldb, C, ldc,
                           static_cast<double*>(ws), as_stream(stream));
}
