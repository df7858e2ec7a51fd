// fp64 products on the int8 matrix cores (the integer modular scheme, "Ozaki scheme II").
//
//   C = alpha op(A) op(B) + beta C,  op(A) m x k, op(B) k x n, row-major fp64.
//
// 1. Per row of op(A) and per column of op(B) a power of two scales the vector so that every entry
//    is below 2^s in magnitude; the scaled entries are truncated toward zero to integers a', b'.
//    s = floor((log2 P - 1 - ceil(log2 k)) / 2) (at most 57), P the product of the moduli, so that
//    2 sum_k |a'||b'| < P.
// 2. Sixteen int8 planes a' mod p_t, b' mod p_t (symmetric residues), written K-contiguous whatever
//    the fp64 layout was.
// 3. Sixteen exact int8 x int8 -> int32 products through hipBLASLt (bound at run time with dlopen:
//    the library is not linked), in output blocks that keep planes + int32 results under a cap.
// 4. Per element: residues of the int32 results, Garner's mixed-radix digits (symmetric), the
//    128-bit integer C' = v_1 + p_1 (v_2 + p_2 (...)) exactly, ONE rounding to fp64, then
//    C = alpha 2^(-mu_i - nu_j) C' + beta C.
// The integer part is exact; the error is the truncation of step 1 ("fp64 products
// on the int8 matrix cores").
#include <dlfcn.h>
#include <hipblaslt/hipblaslt.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "dense.h"

namespace vgposp {

constexpr int EMUL_NMOD = 16;
constexpr int EMUL_SMAX = 57;  // q = a' / p stays far below 2^53 in emul_residue
// Planes of both operands + the int32 results of one output block stay under this many bytes
// (vgposp_gemm_emulation_set_block_cap lowers it for tests).  24 GiB: the planes of the 65k
// step's largest product (16384 x 16384 x 32768) are 16 GiB by themselves, and the blocks that
// are left, 16384 x 8192, run at the library's full int8 rate (profiles/gemm_emul_int8_rates.json).
constexpr size_t EMUL_CAP_DEFAULT = (size_t)24 << 30;
constexpr size_t EMUL_LT_WS_BYTES = (size_t)64 << 20;  // the library's own workspace

__host__ __device__ constexpr int emul_mod(int t) {
  constexpr int p[EMUL_NMOD] = {256, 255, 253, 251, 247, 241, 239, 233,
                                229, 227, 223, 217, 211, 199, 197, 193};
  return p[t];
}

// p_j^-1 mod p_t for j < t, symmetric representatives (Garner's 120 constants).
__host__ __device__ constexpr int emul_inv(int t, int j) {
  constexpr signed char inv[EMUL_NMOD][EMUL_NMOD] = {
      {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
      {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
      {-84, -126, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
      {-50, 63, -125, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
      {55, 31, -41, 62, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
      {-16, -86, -20, -24, -40, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
      {-14, 15, -17, 20, 30, -119, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
      {-81, 53, 35, 13, 50, -29, 39, 0, 0, 0, 0, 0, 0, 0, 0, 0},
      {17, -44, 105, -52, -89, -19, 23, -57, 0, 0, 0, 0, 0, 0, 0, 0},
      {47, 73, -96, -104, -34, -81, 19, 38, -113, 0, 0, 0, 0, 0, 0, 0},
      {-27, 7, -52, 8, -65, 62, 14, 67, -37, 56, 0, 0, 0, 0, 0, 0},
      {-89, 40, -6, 83, -94, -9, -69, 95, -18, -65, -36, 0, 0, 0, 0, 0},
      {-75, 24, -5, -58, -41, -7, 98, 48, -82, 66, 88, -35, 0, 0, 0, 0},
      {7, 32, -70, -88, -29, -90, 5, 41, 73, 64, -58, -11, 83, 0, 0, 0},
      {-10, 17, 95, -62, 67, -94, 61, -93, -80, 46, -53, 69, -14, -98, 0, 0},
      {-49, -28, 74, 10, -25, -4, 21, -82, 59, -17, -45, -8, -75, -32, -48, 0},
  };
  return inv[t][j];
}

// x mod p into the symmetric range: [-(p-1)/2, (p-1)/2] for odd p, [-128, 127] for 256.  x is an
// integer held in fp64 with |x| < 2^57: q is within 1 of x / p, the fma is exact, one correction
// by p is enough.
template <int T>
__host__ __device__ inline int emul_residue(double x) {
  constexpr int p = emul_mod(T), h = (p - 1) / 2;
  const double q = rint(x * (1.0 / p));
  int r = (int)fma(-(double)p, q, x);
  r = r > h ? r - p : r;
  r = r < h - (p - 1) ? r + p : r;  // (lower end -h for odd p, -128 for 256)
  return r;
}

// The same for a small integer held in fp32 (|x| < 2^23), without the correction: the result is
// congruent to x and within (p + 1) / 2 of zero.
__host__ __device__ inline float emul_fold(float x, int p) {
  return fmaf(-(float)p, rintf(x * (1.0f / (float)p)), x);
}

// Sixteen residues r_t (any representatives with |r_t| <= 2^30) -> Garner's mixed-radix digits
// v_t, strictly symmetric, so that the integer v_0 + p_0 (v_1 + p_1 (...)) is THE representative
// of the residue class in [-P/2, P/2).  Every intermediate is an integer below 2^17 in magnitude,
// exact in fp32.
__host__ __device__ inline void emul_garner(const int (&c)[EMUL_NMOD], int (&v)[EMUL_NMOD]) {
  float r[EMUL_NMOD], d[EMUL_NMOD];
#define VG_EMUL_R(T) r[T] = (float)emul_residue<T>((double)c[T]);
  VG_EMUL_R(0) VG_EMUL_R(1) VG_EMUL_R(2) VG_EMUL_R(3) VG_EMUL_R(4) VG_EMUL_R(5) VG_EMUL_R(6)
  VG_EMUL_R(7) VG_EMUL_R(8) VG_EMUL_R(9) VG_EMUL_R(10) VG_EMUL_R(11) VG_EMUL_R(12) VG_EMUL_R(13)
  VG_EMUL_R(14) VG_EMUL_R(15)
#undef VG_EMUL_R
  d[0] = r[0];
#pragma unroll
  for (int t = 1; t < EMUL_NMOD; ++t) {
    const int p = emul_mod(t), h = (p - 1) / 2;
    float x = r[t];
#pragma unroll
    for (int j = 0; j < t; ++j) x = emul_fold((x - d[j]) * (float)emul_inv(t, j), p);
    x = x > (float)h ? x - (float)p : x;
    x = x < -(float)h ? x + (float)p : x;
    d[t] = x;
  }
#pragma unroll
  for (int t = 0; t < EMUL_NMOD; ++t) v[t] = (int)d[t];
}

// The digits' integer, rounded once (to nearest even) to fp64.
__host__ __device__ inline double emul_value(const int (&v)[EMUL_NMOD]) {
  __int128 acc = v[EMUL_NMOD - 1];
#pragma unroll
  for (int t = EMUL_NMOD - 2; t >= 0; --t) acc = acc * emul_mod(t) + v[t];
  const bool neg = acc < 0;
  const unsigned __int128 u = neg ? -(unsigned __int128)acc : (unsigned __int128)acc;
  const unsigned long long hi = (unsigned long long)(u >> 64), lo = (unsigned long long)u;
  double mag;
  if (hi == 0) {
    mag = (double)lo;
  } else {
    const int sh = 64 - __builtin_clzll(hi);  // 1 .. 64 bits move out at the low end
    unsigned long long top = sh == 64 ? hi : (hi << (64 - sh)) | (lo >> sh);
    const unsigned long long lost = sh == 64 ? lo : lo << (64 - sh);
    top |= lost != 0 ? 1ull : 0ull;  // sticky: bit 0 lies below the rounding position (bit 10)
    mag = ldexp((double)top, sh);
  }
  return neg ? -mag : mag;
}

// Bits of the largest |x| of a vector -> its scale exponent mu (|2^mu x| < 2^s).  A vector with a
// non-finite entry gets INT_MIN (its row or column of C becomes NaN), a zero vector 0.
constexpr int EMUL_NONFINITE = INT_MIN;
__host__ __device__ inline int emul_mu(unsigned long long maxbits, int s) {
  if (maxbits >= 0x7FF0000000000000ull) return EMUL_NONFINITE;
  if (maxbits == 0) return 0;
  int e;
  (void)frexp(__builtin_bit_cast(double, maxbits), &e);  // max = f 2^e, 0.5 <= f < 1
  return s - e;
}

// ---- split: row maxima, then the planes ------------------------------------------------------
// An operand is nv vectors (rows of op(A) / columns of op(B)) of k entries; entry (v, kk) is at
// X[v * sv + kk * sk] with one of the two strides 1.  Tiles of 32 vectors x 128 entries.
constexpr int EM_TV = 32, EM_TK = 128;

template <bool KCONTIG>
__device__ __forceinline__ void emul_tile_coord(int i, int tid, int& v, int& kk) {
  if constexpr (KCONTIG) {
    v = i * 2 + (tid >> 7);
    kk = tid & 127;
  } else {
    kk = i * 8 + (tid >> 5);
    v = tid & 31;
  }
}

// Triangle modes of a split (the structured drivers).  The operand is the window of a lower
// triangular X whose first vector is global row / column vg0 and whose first entry is global
// index kg0: EMUL_TRI_A zeroes the entries with global k > v (X stored [i][k], rows are the
// vectors), EMUL_TRI_B those with k < v (X stored [k][j], columns are the vectors).  A zeroed
// entry is NEVER LOADED.  bw is the staircase's block width: a 32 x 128 tile that no staircase step
// reads (beyond the vectors' own block in EMUL_TRI_A, before it in EMUL_TRI_B) is skipped whole,
// its planes left as they are.
constexpr int EMUL_TRI_NONE = 0, EMUL_TRI_A = 1, EMUL_TRI_B = 2;

struct EmulTri {
  int64_t vg0, kg0, bw;
};

template <int TRI>
__device__ __forceinline__ bool emul_tile_unread(const EmulTri& t, int64_t v0, int64_t k0) {
  if constexpr (TRI == EMUL_TRI_A) return t.kg0 + k0 >= ((t.vg0 + v0) / t.bw + 1) * t.bw;
  if constexpr (TRI == EMUL_TRI_B) return t.kg0 + k0 + EM_TK <= (t.vg0 + v0) / t.bw * t.bw;
  return false;
}

template <int TRI>
__device__ __forceinline__ bool emul_masked(const EmulTri& t, int64_t v, int64_t kk) {
  if constexpr (TRI == EMUL_TRI_A) return t.kg0 + kk > t.vg0 + v;
  if constexpr (TRI == EMUL_TRI_B) return t.kg0 + kk < t.vg0 + v;
  return false;
}

template <bool KCONTIG, int TRI>
__global__ __launch_bounds__(256) void emul_max_kernel(const double* __restrict__ X, int64_t ld,
                                                       int64_t nv, int64_t k,
                                                       unsigned long long* __restrict__ maxbits,
                                                       const int* abort, EmulTri tri) {
  if (abort != nullptr && *abort != 0) return;
  __shared__ unsigned long long smax[EM_TV];
  const int tid = threadIdx.x;
  const int64_t v0 = (int64_t)blockIdx.y * EM_TV, k0 = (int64_t)blockIdx.x * EM_TK;
  if (emul_tile_unread<TRI>(tri, v0, k0)) return;
  if (tid < EM_TV) smax[tid] = 0;
  __syncthreads();
  unsigned long long own = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    int v, kk;
    emul_tile_coord<KCONTIG>(i, tid, v, kk);
    unsigned long long b = 0;
    if (v0 + v < nv && k0 + kk < k && !emul_masked<TRI>(tri, v0 + v, k0 + kk)) {
      const double x = KCONTIG ? X[(v0 + v) * ld + k0 + kk] : X[(k0 + kk) * ld + v0 + v];
      b = __builtin_bit_cast(unsigned long long, x) & 0x7FFFFFFFFFFFFFFFull;
    }
    if constexpr (KCONTIG) {
      // the wave's 64 lanes hold one vector's entries: reduce, one LDS atomic per wave
      const double r = wave_reduce(__builtin_bit_cast(double, b), [](double a, double c) {
        const unsigned long long ua = __builtin_bit_cast(unsigned long long, a);
        const unsigned long long uc = __builtin_bit_cast(unsigned long long, c);
        return __builtin_bit_cast(double, ua > uc ? ua : uc);
      });
      if ((tid & 63) == 0) atomicMax(&smax[v], __builtin_bit_cast(unsigned long long, r));
    } else {
      own = b > own ? b : own;  // (every i is the same vector)
    }
  }
  if constexpr (!KCONTIG) atomicMax(&smax[tid & 31], own);
  __syncthreads();
  if (tid < EM_TV && v0 + tid < nv && smax[tid] != 0) atomicMax(&maxbits[v0 + tid], smax[tid]);
}

constexpr int EM_LDS_ROW = EM_TK + EM_TK / 16 + 1;  // 16-entry groups land in different banks

template <bool KCONTIG, int TRI>
__global__ __launch_bounds__(256) void emul_split_kernel(const double* __restrict__ X, int64_t ld,
                                                         int64_t nv, int64_t k, int64_t kp, int s,
                                                         const unsigned long long* __restrict__ maxbits,
                                                         signed char* __restrict__ planes,
                                                         const int* abort, EmulTri tri) {
  if (abort != nullptr && *abort != 0) return;
  __shared__ double tile[EM_TV * EM_LDS_ROW];
  const int tid = threadIdx.x;
  const int64_t v0 = (int64_t)blockIdx.y * EM_TV, k0 = (int64_t)blockIdx.x * EM_TK;
  if (emul_tile_unread<TRI>(tri, v0, k0)) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    int v, kk;
    emul_tile_coord<KCONTIG>(i, tid, v, kk);
    double x = 0.0;
    if (v0 + v < nv && k0 + kk < k && !emul_masked<TRI>(tri, v0 + v, k0 + kk)) {
      x = KCONTIG ? X[(v0 + v) * ld + k0 + kk] : X[(k0 + kk) * ld + v0 + v];
      const int mu = emul_mu(maxbits[v0 + v], s);
      x = mu == EMUL_NONFINITE ? 0.0 : trunc(ldexp(x, mu));
    }
    tile[v * EM_LDS_ROW + kk + (kk >> 4)] = x;
  }
  __syncthreads();
  const int v = tid >> 3, g = tid & 7;
  if (v0 + v >= nv) return;
  double a[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) a[j] = tile[v * EM_LDS_ROW + g * 17 + j];
  signed char* out = planes + (v0 + v) * kp + k0 + g * 16;
  const int64_t pstride = nv * kp;
#define VG_EMUL_PLANE(T)                                                          \
  {                                                                               \
    unsigned w[4];                                                                \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                               \
      w[q] = 0;                                                                   \
      _Pragma("unroll") for (int b = 0; b < 4; ++b)                               \
          w[q] |= ((unsigned)emul_residue<T>(a[4 * q + b]) & 0xFFu) << (8 * b);   \
    }                                                                             \
    *reinterpret_cast<uint4*>(out + (T) * pstride) = make_uint4(w[0], w[1], w[2], w[3]); \
  }
  VG_EMUL_PLANE(0) VG_EMUL_PLANE(1) VG_EMUL_PLANE(2) VG_EMUL_PLANE(3) VG_EMUL_PLANE(4)
  VG_EMUL_PLANE(5) VG_EMUL_PLANE(6) VG_EMUL_PLANE(7) VG_EMUL_PLANE(8) VG_EMUL_PLANE(9)
  VG_EMUL_PLANE(10) VG_EMUL_PLANE(11) VG_EMUL_PLANE(12) VG_EMUL_PLANE(13) VG_EMUL_PLANE(14)
  VG_EMUL_PLANE(15)
#undef VG_EMUL_PLANE
}

// ---- reconstruction --------------------------------------------------------------------------
// One thread per element of a cm x cn output block: its sixteen int32 values are loaded together,
// then Garner, the exact integer, one rounding, the scales, alpha and beta.  Only the elements
// with j <= i + low are touched (a SYRK block on the diagonal: low = its first row - its first
// column); every other element of C is neither read nor written.  EMUL_LOW_ALL = all of them.
constexpr int64_t EMUL_LOW_ALL = INT64_MAX / 2;
__global__ __launch_bounds__(256) void emul_crt_kernel(const int* __restrict__ planes, int64_t cm,
                                                       int64_t cn, int s,
                                                       const unsigned long long* __restrict__ maxA,
                                                       const unsigned long long* __restrict__ maxB,
                                                       double alpha, double beta, double* C,
                                                       int64_t ldc, const int* abort, int64_t low) {
  if (abort != nullptr && *abort != 0) return;
  const int64_t nbx = (cn + 255) / 256;
  const int64_t i = blockIdx.x / nbx, j = (blockIdx.x % nbx) * 256 + threadIdx.x;
  if (j >= cn || j > i + low) return;
  int c[EMUL_NMOD];
  const int* src = planes + i * cn + j;
#pragma unroll
  for (int t = 0; t < EMUL_NMOD; ++t) c[t] = src[(int64_t)t * cm * cn];
  const int mu = emul_mu(maxA[i], s), nu = emul_mu(maxB[j], s);
  double* dst = C + i * ldc + j;
  if (mu == EMUL_NONFINITE || nu == EMUL_NONFINITE) {
    *dst = __builtin_nan("");
    return;
  }
  int v[EMUL_NMOD];
  emul_garner(c, v);
  const double val = ldexp(emul_value(v), -mu - nu);
  *dst = beta == 0.0 ? alpha * val : fma(alpha, val, beta * *dst);
}

// ---- hipBLASLt, bound at run time --------------------------------------------------------------
struct LtApi {
  decltype(&hipblasLtCreate) Create;
  decltype(&hipblasLtMatmulDescCreate) DescCreate;
  decltype(&hipblasLtMatmulDescSetAttribute) DescSet;
  decltype(&hipblasLtMatrixLayoutCreate) LayoutCreate;
  decltype(&hipblasLtMatrixLayoutSetAttribute) LayoutSet;
  decltype(&hipblasLtMatmulPreferenceCreate) PrefCreate;
  decltype(&hipblasLtMatmulPreferenceSetAttribute) PrefSet;
  decltype(&hipblasLtMatmulPreferenceDestroy) PrefDestroy;
  decltype(&hipblasLtMatmulAlgoGetHeuristic) Heuristic;
  decltype(&hipblasLtMatmul) Matmul;
};

static std::mutex g_lt_mutex;
static std::atomic<int> g_forced_unavailable{0};  // the tests' hook
static std::atomic<size_t> g_block_cap{EMUL_CAP_DEFAULT};
// Process-wide setting of the fused Cholesky + inverse (vgposp_potrf_set_emulation), like the
// Strassen one: set explicitly, never from the environment.  On by default at 8192 from the 65k
// step's A/B (profiles/gemm_emul_ab.json): parent 2,504 ms, on at 8192 2,035 ms, on
// at 4096 2,010 ms; 8192 because it leaves every n < 32,768 as it was, workspace included.
static std::atomic<int64_t> g_emul_min_dim{8192};
static std::atomic<int> g_emul_moduli{EMUL_NMOD};

// The library's entry points, resolved once (no GPU work); null when it cannot be found.
static const LtApi* lt_api() {
  static LtApi api;
  static int state = 0;  // 0 not tried, 1 resolved, -1 absent
  std::lock_guard<std::mutex> lock(g_lt_mutex);
  if (state == 0) {
    state = -1;
    void* h = dlopen("libhipblaslt.so.1", RTLD_NOW | RTLD_NOLOAD);  // the process's own copy
    if (h == nullptr) h = dlopen("libhipblaslt.so.1", RTLD_NOW | RTLD_LOCAL);
    if (h == nullptr) h = dlopen("/opt/rocm/lib/libhipblaslt.so.1", RTLD_NOW | RTLD_LOCAL);
    if (h != nullptr) {
      bool ok = true;
#define VG_LT_SYM(field, name)                                         \
  api.field = reinterpret_cast<decltype(api.field)>(dlsym(h, name));   \
  ok = ok && api.field != nullptr
      VG_LT_SYM(Create, "hipblasLtCreate");
      VG_LT_SYM(DescCreate, "hipblasLtMatmulDescCreate");
      VG_LT_SYM(DescSet, "hipblasLtMatmulDescSetAttribute");
      VG_LT_SYM(LayoutCreate, "hipblasLtMatrixLayoutCreate");
      VG_LT_SYM(LayoutSet, "hipblasLtMatrixLayoutSetAttribute");
      VG_LT_SYM(PrefCreate, "hipblasLtMatmulPreferenceCreate");
      VG_LT_SYM(PrefSet, "hipblasLtMatmulPreferenceSetAttribute");
      VG_LT_SYM(PrefDestroy, "hipblasLtMatmulPreferenceDestroy");
      VG_LT_SYM(Heuristic, "hipblasLtMatmulAlgoGetHeuristic");
      VG_LT_SYM(Matmul, "hipblasLtMatmul");
#undef VG_LT_SYM
      if (ok) state = 1;
    }
  }
  return state == 1 ? &api : nullptr;
}

bool gemm_emul_available() {
  return g_forced_unavailable.load(std::memory_order_relaxed) == 0 && lt_api() != nullptr;
}

// One int8 product shape: rows x cols int32 results over a depth of K-contiguous planes whose
// vectors are ld apart, `batch` of them.
struct LtPlan {
  bool ok = false;
  int batch = 0;  // planes per call (EMUL_NMOD, or 1 when the library has no batched kernel)
  hipblasLtMatmulDesc_t desc = nullptr;
  hipblasLtMatrixLayout_t la = nullptr, lb = nullptr, lc = nullptr;
  hipblasLtMatmulAlgo_t algo;
  size_t ws = 0;
};

struct LtState {
  hipblasLtHandle_t handle = nullptr;
  void* ws = nullptr;
  bool failed = false;
  std::map<std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>, LtPlan> plans;
};
static LtState g_lt;

// Handle, workspace and the plan of (cm, cn, depth, ld, sa, sb), each created once.  Null when
// the library refuses (the caller then takes another path).
static const LtPlan* lt_plan(const LtApi& lt, int64_t cm, int64_t cn, int64_t depth, int64_t ld,
                             int64_t sa, int64_t sb) {
  std::lock_guard<std::mutex> lock(g_lt_mutex);
  if (g_lt.failed) return nullptr;
  if (g_lt.handle == nullptr) {
    if (lt.Create(&g_lt.handle) != HIPBLAS_STATUS_SUCCESS ||
        hipMalloc(&g_lt.ws, EMUL_LT_WS_BYTES) != hipSuccess) {
      g_lt.failed = true;
      return nullptr;
    }
  }
  const auto key = std::make_tuple(cm, cn, depth, ld, sa, sb);
  auto it = g_lt.plans.find(key);
  if (it != g_lt.plans.end()) return it->second.ok ? &it->second : nullptr;
  LtPlan& p = g_lt.plans[key];
  // row-major C (cm x cn) = A' B'^T is, column-major, C^T (cn x cm) = op_T(B' planes) A' planes
  const int32_t opt = HIPBLAS_OP_T, opn = HIPBLAS_OP_N;
  hipblasLtMatmulPreference_t pref = nullptr;
  const uint64_t maxws = EMUL_LT_WS_BYTES;
  bool made = lt.DescCreate(&p.desc, HIPBLAS_COMPUTE_32I, HIP_R_32I) == HIPBLAS_STATUS_SUCCESS &&
              lt.DescSet(p.desc, HIPBLASLT_MATMUL_DESC_TRANSA, &opt, sizeof opt) == HIPBLAS_STATUS_SUCCESS &&
              lt.DescSet(p.desc, HIPBLASLT_MATMUL_DESC_TRANSB, &opn, sizeof opn) == HIPBLAS_STATUS_SUCCESS &&
              lt.LayoutCreate(&p.la, HIP_R_8I, depth, cn, ld) == HIPBLAS_STATUS_SUCCESS &&
              lt.LayoutCreate(&p.lb, HIP_R_8I, depth, cm, ld) == HIPBLAS_STATUS_SUCCESS &&
              lt.LayoutCreate(&p.lc, HIP_R_32I, cn, cm, cn) == HIPBLAS_STATUS_SUCCESS &&
              lt.PrefCreate(&pref) == HIPBLAS_STATUS_SUCCESS &&
              lt.PrefSet(pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &maxws, sizeof maxws) ==
                  HIPBLAS_STATUS_SUCCESS;
  for (int batch : {EMUL_NMOD, 1}) {
    if (!made || p.ok) break;
    const int32_t bc = batch;
    const int64_t stb = sb, sta = sa, stc = cm * cn;
    bool set = lt.LayoutSet(p.la, HIPBLASLT_MATRIX_LAYOUT_BATCH_COUNT, &bc, sizeof bc) == HIPBLAS_STATUS_SUCCESS &&
               lt.LayoutSet(p.lb, HIPBLASLT_MATRIX_LAYOUT_BATCH_COUNT, &bc, sizeof bc) == HIPBLAS_STATUS_SUCCESS &&
               lt.LayoutSet(p.lc, HIPBLASLT_MATRIX_LAYOUT_BATCH_COUNT, &bc, sizeof bc) == HIPBLAS_STATUS_SUCCESS &&
               lt.LayoutSet(p.la, HIPBLASLT_MATRIX_LAYOUT_STRIDED_BATCH_OFFSET, &stb, sizeof stb) == HIPBLAS_STATUS_SUCCESS &&
               lt.LayoutSet(p.lb, HIPBLASLT_MATRIX_LAYOUT_STRIDED_BATCH_OFFSET, &sta, sizeof sta) == HIPBLAS_STATUS_SUCCESS &&
               lt.LayoutSet(p.lc, HIPBLASLT_MATRIX_LAYOUT_STRIDED_BATCH_OFFSET, &stc, sizeof stc) == HIPBLAS_STATUS_SUCCESS;
    hipblasLtMatmulHeuristicResult_t res;
    int found = 0;
    if (set &&
        lt.Heuristic(g_lt.handle, p.desc, p.la, p.lb, p.lc, p.lc, pref, 1, &res, &found) ==
            HIPBLAS_STATUS_SUCCESS &&
        found > 0 && res.state == HIPBLAS_STATUS_SUCCESS && res.workspaceSize <= EMUL_LT_WS_BYTES) {
      p.algo = res.algo;
      p.ws = res.workspaceSize;
      p.batch = batch;
      p.ok = true;
    }
  }
  if (pref != nullptr) lt.PrefDestroy(pref);
  return p.ok ? &p : nullptr;
}

// ---- the product ---------------------------------------------------------------------------
static int64_t round_up(int64_t x, int64_t to) { return (x + to - 1) / to * to; }

int gemm_emul_scale_bits(int64_t k) {
  long double l2p = 0.0L;
  for (int t = 0; t < EMUL_NMOD; ++t) l2p += log2l((long double)emul_mod(t));
  int cl = 0;
  while (((int64_t)1 << cl) < k) ++cl;
  const int s = (int)floorl((l2p - 1.0L - cl) / 2.0L);
  return std::min(s, EMUL_SMAX);
}

static bool emul_dims_ok(int64_t m, int64_t n, int64_t k) {
  return m > 0 && n > 0 && k > 0 && k <= 65536 && m <= ((int64_t)1 << 30) && n <= ((int64_t)1 << 30);
}

struct EmulLayout {
  int64_t kp, cm, cn;  // padded depth, output block
  size_t maxA, maxB, pa, pb, pc, bytes;
};

static EmulLayout emul_layout(int64_t m, int64_t n, int64_t k) {
  EmulLayout l{};
  l.kp = round_up(k, EM_TK);
  l.cm = m;
  l.cn = n;
  const size_t cap = g_block_cap.load(std::memory_order_relaxed);
  const size_t fixed = (size_t)EMUL_NMOD * (m + n) * l.kp;
  while (fixed + (size_t)EMUL_NMOD * 4 * l.cm * l.cn > cap && (l.cm > 128 || l.cn > 128)) {
    if (l.cm >= l.cn)
      l.cm = round_up((l.cm + 1) / 2, 128);
    else
      l.cn = round_up((l.cn + 1) / 2, 128);
  }
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  size_t off = 0;
  l.maxA = off, off += al(8 * (size_t)m);
  l.maxB = off, off += al(8 * (size_t)n);
  l.pa = off, off += al((size_t)EMUL_NMOD * m * l.kp);
  l.pb = off, off += al((size_t)EMUL_NMOD * n * l.kp);
  l.pc = off, off += al((size_t)EMUL_NMOD * 4 * l.cm * l.cn);
  l.bytes = off;
  return l;
}

size_t gemm_emul_ws_bytes(int64_t m, int64_t n, int64_t k) {
  return emul_dims_ok(m, n, k) ? emul_layout(m, n, k).bytes : 0;
}

void gemm_emul_config(int64_t* min_dim, int* moduli) {
  *min_dim = g_emul_min_dim.load(std::memory_order_relaxed);
  *moduli = g_emul_moduli.load(std::memory_order_relaxed);
}

// ---- the three pieces: split, block product, reconstruction ------------------------------------
// Split: nv vectors of k entries at X (the window's first entry) -> their maxima and the sixteen
// planes (nv x kp each, K-contiguous) at the caller's places.  tri_mode / tri: see EmulTri; the
// triangle modes exist for the layouts the factorization has (EMUL_TRI_A K-contiguous, EMUL_TRI_B
// not).
static int emul_split(const double* X, int64_t ld, bool kcontig, int64_t nv, int64_t k, int64_t kp,
                      int s, unsigned long long* maxbits, signed char* planes, const int* abort,
                      hipStream_t st, int tri_mode = EMUL_TRI_NONE, EmulTri tri = EmulTri{0, 0, 1}) {
  // entries actually read and converted (a triangle mode loads only its side of the diagonal)
  double live = (double)nv * k;
  if (tri_mode != EMUL_TRI_NONE) {
    live = 0.0;
    for (int64_t v = 0; v < nv; ++v) {
      const int64_t d = tri.vg0 + v - tri.kg0;  // the diagonal's place in this vector
      live += tri_mode == EMUL_TRI_A ? (double)std::clamp<int64_t>(d + 1, 0, k)
                                     : (double)std::clamp<int64_t>(k - d, 0, k);
    }
  }
  ProfScope ps("gemm_emul_split", st, (double)EMUL_NMOD * 6.0 * live, live * (16.0 + EMUL_NMOD));
  VG_HIP(vg_memset(maxbits, 0, 8 * (size_t)nv, st));
  const dim3 grid((unsigned)(kp / EM_TK), (unsigned)ceil_div(nv, EM_TV));
#define VG_EMUL_SPLIT(KC, TR)                                                                     \
  hipLaunchKernelGGL((emul_max_kernel<KC, TR>), grid, dim3(256), 0, st, X, ld, nv, k, maxbits,    \
                     abort, tri);                                                                 \
  hipLaunchKernelGGL((emul_split_kernel<KC, TR>), grid, dim3(256), 0, st, X, ld, nv, k, kp, s,    \
                     maxbits, planes, abort, tri)
  if (tri_mode == EMUL_TRI_A && kcontig) {
    VG_EMUL_SPLIT(true, EMUL_TRI_A);
  } else if (tri_mode == EMUL_TRI_B && !kcontig) {
    VG_EMUL_SPLIT(false, EMUL_TRI_B);
  } else if (tri_mode != EMUL_TRI_NONE) {
    set_error("emul_split: triangle mode %d in an unsupported layout", tri_mode);
    return VGPOSP_E_UNSUPPORTED;
  } else if (kcontig) {
    VG_EMUL_SPLIT(true, EMUL_TRI_NONE);
  } else {
    VG_EMUL_SPLIT(false, EMUL_TRI_NONE);
  }
#undef VG_EMUL_SPLIT
  VG_LAUNCH_CHECK();
  return 0;
}

// Block product: cm vectors of A-planes at pa times cn vectors of B-planes at pb over `depth`
// entries (a multiple of 128; a K sub-range is an offset already in pa / pb), vectors ld apart,
// plane t at t * sa / t * sb; the int32 results (cm x cn per plane) at pc.
static int emul_block_product(const LtApi& lt, const LtPlan* p, const char* scope,
                              const signed char* pa, const signed char* pb, int64_t cm, int64_t cn,
                              int64_t depth, int64_t sa, int64_t sb, int* pc, hipStream_t st) {
  const int32_t one = 1, zero = 0;
  ProfScope ps(scope, st, 2.0 * EMUL_NMOD * (double)cm * cn * depth,
               (double)EMUL_NMOD * ((double)(cm + cn) * depth + 4.0 * cm * cn));
  for (int t = 0; t < EMUL_NMOD; t += p->batch) {
    const hipblasStatus_t rc =
        lt.Matmul(g_lt.handle, p->desc, &one, pb + t * sb, p->la, pa + t * sa, p->lb, &zero,
                  pc + t * cm * cn, p->lc, pc + t * cm * cn, p->lc, &p->algo, g_lt.ws,
                  EMUL_LT_WS_BYTES, st);
    if (rc != HIPBLAS_STATUS_SUCCESS) {
      set_error("gemm_emulated: hipblasLtMatmul failed with status %d", (int)rc);
      return VGPOSP_E_HIP;
    }
  }
  return 0;
}

// Reconstruction: the int32 block at pc -> C = alpha 2^(-mu - nu) C' + beta C.  low: see
// emul_crt_kernel.
static int emul_reconstruct(const int* pc, int64_t cm, int64_t cn, int s,
                            const unsigned long long* maxA, const unsigned long long* maxB,
                            double alpha, double beta, double* C, int64_t ldc, const int* abort,
                            hipStream_t st, int64_t low = EMUL_LOW_ALL) {
  const double outs = low == EMUL_LOW_ALL ? (double)cm * cn : 0.5 * cm * (double)(cm + 1) + (double)cm * (cn - cm);
  ProfScope ps("gemm_emul_crt", st, 1000.0 * outs,
               outs * (4.0 * EMUL_NMOD + (beta != 0.0 ? 16.0 : 8.0)));
  const int64_t nblk = cm * ceil_div(cn, 256);
  hipLaunchKernelGGL(emul_crt_kernel, dim3((unsigned)nblk), dim3(256), 0, st, pc, cm, cn, s, maxA,
                     maxB, alpha, beta, C, ldc, abort, low);
  VG_LAUNCH_CHECK();
  return 0;
}

// C = alpha op(A) op(B) + beta C through the int8 products.  ws holds gemm_emul_ws_bytes(m, n, k).
// Returns 1, with nothing launched, when the library is absent or has no kernel for a block
// shape; the caller then takes its fp64 path.
int gemm_emulated(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                  const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C,
                  int64_t ldc, void* ws, hipStream_t st) {
  if (!gemm_emul_available() || !emul_dims_ok(m, n, k) ||
      ceil_div(std::max(m, n), EM_TV) > 65535)  // (the split kernels' grid.y)
    return 1;
  const LtApi& lt = *lt_api();
  const EmulLayout l = emul_layout(m, n, k);
  // every block shape must have a kernel before anything is launched
  for (int64_t i0 = 0; i0 < m; i0 += l.cm)
    for (int64_t j0 = 0; j0 < n; j0 += l.cn)
      if (lt_plan(lt, std::min(l.cm, m - i0), std::min(l.cn, n - j0), l.kp, l.kp, m * l.kp,
                  n * l.kp) == nullptr)
        return 1;
  char* base = static_cast<char*>(ws);
  auto* maxA = reinterpret_cast<unsigned long long*>(base + l.maxA);
  auto* maxB = reinterpret_cast<unsigned long long*>(base + l.maxB);
  auto* pa = reinterpret_cast<signed char*>(base + l.pa);
  auto* pb = reinterpret_cast<signed char*>(base + l.pb);
  int* pc = reinterpret_cast<int*>(base + l.pc);
  const int* abort = gemm_abort_flag();
  const int s = gemm_emul_scale_bits(k);
  // rows of op(A): stored m x k (k contiguous) or k x m; columns of op(B): stored k x n or n x k
  VG_TRY(emul_split(A, lda, !transa, m, k, l.kp, s, maxA, pa, abort, st));
  VG_TRY(emul_split(B, ldb, transb != 0, n, k, l.kp, s, maxB, pb, abort, st));
  for (int64_t i0 = 0; i0 < m; i0 += l.cm)
    for (int64_t j0 = 0; j0 < n; j0 += l.cn) {
      const int64_t cm = std::min(l.cm, m - i0), cn = std::min(l.cn, n - j0);
      const LtPlan* p = lt_plan(lt, cm, cn, l.kp, l.kp, m * l.kp, n * l.kp);
      VG_TRY(emul_block_product(lt, p, "gemm_i8", pa + i0 * l.kp, pb + j0 * l.kp, cm, cn, l.kp,
                                m * l.kp, n * l.kp, pc, st));
      VG_TRY(emul_reconstruct(pc, cm, cn, s, maxA + i0, maxB + j0, alpha, beta, C + i0 * ldc + j0,
                              ldc, abort, st));
    }
  return 0;
}

// ---- the structured products: a staircase of block products ------------------------------------
// kind: VGPOSP_EMUL_SYRK_LOWER  C (n x n, lower) = alpha A A^T + beta C,  A n x k
//       VGPOSP_EMUL_TRMM_B      C (m x n) = alpha A X + beta C,  X n x n lower stored [k][j]
//       VGPOSP_EMUL_TRMM_A      C (m x n) = alpha X B + beta C,  X m x m lower stored [i][k]
// A triangular product is a staircase of rectangular ones over K-contiguous planes:
//   SYRK    block row i of C needs the columns [0, end of block i) over the full depth;
//   TRMM_B  column block j needs only the depth suffix [start of block j, n);
//   TRMM_A  row block i needs only the depth prefix [0, end of block i).
// The planner cuts the product into tiles (a row panel x a column panel whose planes and one
// step's int32 results fit the bytes given; ONE tile where everything fits) and each tile into
// steps of the block width.  It is pure: the driver, its plan check and the tests all call it.
constexpr int64_t EMUL_TRI_BLOCK[3] = {2048, 2048, 2048};  // SYRK, TRMM_B, TRMM_A
static std::atomic<int64_t> g_tri_block{0};  // the tests' hook; 0 = the default per kind
static std::atomic<int> g_tri_on{1};

// Block widths from the staircase rates on one MI355X (profiles/gemm_emul_tri_rates.json) and
// the 65k step's A/B (profiles/gemm_emul_tri_ab.json): parent 2,077.5 ms, drivers
// on at 2,048 1,808.3 ms, at 4,096 1,858.8 ms.
static int64_t tri_block_width(int kind) {
  const int64_t b = g_tri_block.load(std::memory_order_relaxed);
  if (b > 0) return b;
  return EMUL_TRI_BLOCK[kind];
}

bool gemm_emul_tri_enabled() { return g_tri_on.load(std::memory_order_relaxed) != 0; }

struct TriStep {
  int64_t tile;                    // steps of one tile are consecutive
  int64_t r0, r1, c0, c1, ka, kb;  // the tile: rows and columns of C, the depth its planes hold
  int64_t i0, i1, j0, j1, k0, k1;  // the step: its block of C and its depth range
  int64_t tile_bytes;              // maxima + planes + the largest int32 block of the tile
  bool diag;                       // SYRK tile on the diagonal: one operand, lower steps
};

static size_t tri_al(size_t x) { return (x + 255) & ~(size_t)255; }

// Bytes of a tile: rows nr, columns nc (0 = the planes are shared), depth kd, largest step cm x cn.
static size_t tri_tile_bytes(int64_t nr, int64_t nc, int64_t kd, int64_t cm, int64_t cn) {
  const int64_t kp = round_up(kd, EM_TK);
  return tri_al(8 * (size_t)nr) + tri_al(8 * (size_t)nc) + tri_al((size_t)EMUL_NMOD * nr * kp) +
         tri_al((size_t)EMUL_NMOD * nc * kp) + tri_al((size_t)EMUL_NMOD * 4 * cm * cn);
}

// The steps of (kind, m, n, k) within `bytes`, block width b (a multiple of 128).  False when not
// even one block per panel fits.  C is m x n; SYRK has m == n, TRMM_B k == n, TRMM_A k == m.
static bool tri_plan(int kind, int64_t m, int64_t n, int64_t k, size_t bytes, int64_t b,
                     std::vector<TriStep>& steps) {
  steps.clear();
  int64_t pr = round_up(m, b), pc = round_up(n, b);  // panel heights and widths
  for (;;) {
    // the largest tile of this panelling: the longest depth, the widest step
    const int64_t nr = std::min(pr, m), nc = std::min(pc, n);
    size_t worst;
    if (kind == VGPOSP_EMUL_SYRK_LOWER)
      worst = pr >= m ? tri_tile_bytes(nr, 0, k, std::min(b, m), nr)
                      : tri_tile_bytes(nr, nc, k, std::min(b, m), nc);
    else if (kind == VGPOSP_EMUL_TRMM_B)
      worst = tri_tile_bytes(nr, nc, k, nr, std::min(b, n));
    else
      worst = tri_tile_bytes(nr, nc, k, std::min(b, m), nc);
    if (worst <= bytes) break;
    if (pr <= b && pc <= b) return false;
    // halve the taller side (SYRK: both, its panels are square)
    if (kind == VGPOSP_EMUL_SYRK_LOWER)
      pr = pc = round_up((pr + 1) / 2, b);
    else if (pr >= pc)
      pr = round_up((pr + 1) / 2, b);
    else
      pc = round_up((pc + 1) / 2, b);
  }
  int64_t tile = 0;
  for (int64_t r0 = 0; r0 < m; r0 += pr)
    for (int64_t c0 = 0; c0 < n; c0 += pc) {
      const int64_t r1 = std::min(r0 + pr, m), c1 = std::min(c0 + pc, n);
      if (kind == VGPOSP_EMUL_SYRK_LOWER && c0 > r0) continue;
      TriStep t{};
      t.tile = tile++;
      t.r0 = r0, t.r1 = r1, t.c0 = c0, t.c1 = c1;
      t.diag = kind == VGPOSP_EMUL_SYRK_LOWER && c0 == r0;
      t.ka = kind == VGPOSP_EMUL_TRMM_B ? c0 : 0;
      t.kb = kind == VGPOSP_EMUL_TRMM_A ? r1 : k;
      const size_t first = steps.size();
      int64_t wm = 0, wn = 0;
      if (kind == VGPOSP_EMUL_TRMM_B) {
        for (int64_t j0 = c0; j0 < c1; j0 += b) {
          t.i0 = r0, t.i1 = r1, t.j0 = j0, t.j1 = std::min(j0 + b, c1), t.k0 = j0, t.k1 = k;
          steps.push_back(t);
        }
      } else {
        for (int64_t i0 = r0; i0 < r1; i0 += b) {
          t.i0 = i0, t.i1 = std::min(i0 + b, r1);
          t.j0 = c0, t.j1 = t.diag ? t.i1 : c1;
          t.k0 = 0, t.k1 = kind == VGPOSP_EMUL_TRMM_A ? t.i1 : k;
          steps.push_back(t);
        }
      }
      for (size_t q = first; q < steps.size(); ++q)
        if ((steps[q].i1 - steps[q].i0) * (steps[q].j1 - steps[q].j0) > wm * wn)
          wm = steps[q].i1 - steps[q].i0, wn = steps[q].j1 - steps[q].j0;
      const size_t tb = tri_tile_bytes(r1 - r0, t.diag ? 0 : c1 - c0, t.kb - t.ka, wm, wn);
      for (size_t q = first; q < steps.size(); ++q) steps[q].tile_bytes = (int64_t)tb;
    }
  return true;
}

static int64_t tri_step_depth(const TriStep& t) { return round_up(t.k1 - t.k0, EM_TK); }

static bool tri_dims_ok(int kind, int64_t m, int64_t n, int64_t k) {
  if (!emul_dims_ok(m, n, k) || ceil_div(std::max(m, n), EM_TV) > 65535) return false;
  if (kind == VGPOSP_EMUL_SYRK_LOWER) return m == n;
  if (kind == VGPOSP_EMUL_TRMM_B) return k == n;
  return kind == VGPOSP_EMUL_TRMM_A && k == m;
}

// The structured product through the staircase, within ws_bytes of scratch (and the block cap).
// Returns 1, with nothing launched, when the library is absent, has no kernel for a step's shape,
// or not even the smallest tile fits; the caller then takes its other path.  C must not overlap
// A or B.
int gemm_emulated_tri(int kind, int64_t m, int64_t n, int64_t k, double alpha, const double* A,
                      int64_t lda, const double* B, int64_t ldb, double beta, double* C,
                      int64_t ldc, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!gemm_emul_available() || !tri_dims_ok(kind, m, n, k)) return 1;
  const LtApi& lt = *lt_api();
  const int64_t b = tri_block_width(kind);
  std::vector<TriStep> steps;
  if (!tri_plan(kind, m, n, k, std::min(ws_bytes, g_block_cap.load(std::memory_order_relaxed)), b,
                steps))
    return 1;
  auto strides = [](const TriStep& t, int64_t& kpt, int64_t& sa, int64_t& sb) {
    kpt = round_up(t.kb - t.ka, EM_TK);
    sa = (t.r1 - t.r0) * kpt;
    sb = t.diag ? sa : (t.c1 - t.c0) * kpt;
  };
  // every step's shape must have a kernel before anything is launched
  for (const TriStep& t : steps) {
    int64_t kpt, sa, sb;
    strides(t, kpt, sa, sb);
    if (lt_plan(lt, t.i1 - t.i0, t.j1 - t.j0, tri_step_depth(t), kpt, sa, sb) == nullptr) return 1;
  }
  static const char* scopes[3] = {"gemm_i8[syrk]", "gemm_i8[trmm_b]", "gemm_i8[trmm_a]"};
  const int* abort = gemm_abort_flag();
  const int s = gemm_emul_scale_bits(k);
  char* base = static_cast<char*>(ws);
  unsigned long long *maxA = nullptr, *maxB = nullptr;
  signed char *pa = nullptr, *pb = nullptr;
  int* pc = nullptr;
  int64_t tile = -1;
  for (const TriStep& t : steps) {
    int64_t kpt, sa, sb;
    strides(t, kpt, sa, sb);
    const int64_t nr = t.r1 - t.r0, nc = t.c1 - t.c0, kd = t.kb - t.ka;
    if (t.tile != tile) {  // a new tile: its places in the scratch, its splits
      tile = t.tile;
      size_t off = 0;
      maxA = reinterpret_cast<unsigned long long*>(base + off), off += tri_al(8 * (size_t)nr);
      maxB = maxA;
      if (!t.diag) maxB = reinterpret_cast<unsigned long long*>(base + off), off += tri_al(8 * (size_t)nc);
      pa = reinterpret_cast<signed char*>(base + off), off += tri_al((size_t)EMUL_NMOD * nr * kpt);
      pb = pa;
      if (!t.diag) pb = reinterpret_cast<signed char*>(base + off), off += tri_al((size_t)EMUL_NMOD * nc * kpt);
      pc = reinterpret_cast<int*>(base + off);
      const EmulTri tri{kind == VGPOSP_EMUL_TRMM_A ? t.r0 : t.c0, t.ka, b};
      if (kind == VGPOSP_EMUL_SYRK_LOWER) {
        VG_TRY(emul_split(A + t.r0 * lda, lda, true, nr, kd, kpt, s, maxA, pa, abort, st));
        if (!t.diag)
          VG_TRY(emul_split(A + t.c0 * lda, lda, true, nc, kd, kpt, s, maxB, pb, abort, st));
      } else if (kind == VGPOSP_EMUL_TRMM_B) {
        VG_TRY(emul_split(A + t.r0 * lda + t.ka, lda, true, nr, kd, kpt, s, maxA, pa, abort, st));
        VG_TRY(emul_split(B + t.ka * ldb + t.c0, ldb, false, nc, kd, kpt, s, maxB, pb, abort, st,
                          EMUL_TRI_B, tri));
      } else {
        VG_TRY(emul_split(A + t.r0 * lda + t.ka, lda, true, nr, kd, kpt, s, maxA, pa, abort, st,
                          EMUL_TRI_A, tri));
        VG_TRY(emul_split(B + t.ka * ldb + t.c0, ldb, false, nc, kd, kpt, s, maxB, pb, abort, st));
      }
    }
    const int64_t cm = t.i1 - t.i0, cn = t.j1 - t.j0, depth = tri_step_depth(t);
    const LtPlan* p = lt_plan(lt, cm, cn, depth, kpt, sa, sb);
    VG_TRY(emul_block_product(lt, p, scopes[kind], pa + (t.i0 - t.r0) * kpt + (t.k0 - t.ka),
                              pb + (t.j0 - t.c0) * kpt + (t.k0 - t.ka), cm, cn, depth, sa, sb, pc,
                              st));
    VG_TRY(emul_reconstruct(pc, cm, cn, s, maxA + (t.i0 - t.r0), maxB + (t.j0 - t.c0), alpha, beta,
                            C + t.i0 * ldc + t.j0, ldc, abort, st,
                            t.diag ? t.i0 - t.j0 : EMUL_LOW_ALL));
  }
  return 0;
}

}  // namespace vgposp

extern "C" int vgposp_gemm_emulation_available(void) { return vgposp::gemm_emul_available() ? 1 : 0; }

extern "C" int vgposp_gemm_emulation_set_unavailable(int off) {
  using namespace vgposp;
  clear_error();
  VG_CHECK_ARG(off == 0 || off == 1, 1);
  g_forced_unavailable.store(off, std::memory_order_relaxed);
  return 0;
}

extern "C" int vgposp_gemm_emulation_set_block_cap(size_t bytes) {
  using namespace vgposp;
  clear_error();
  g_block_cap.store(bytes == 0 ? EMUL_CAP_DEFAULT : bytes, std::memory_order_relaxed);
  return 0;
}

extern "C" int vgposp_gemm_emulation_set_tri_block(int64_t width) {
  using namespace vgposp;
  clear_error();
  VG_CHECK_ARG(width >= 0 && width % 128 == 0, 1);
  g_tri_block.store(width, std::memory_order_relaxed);
  return 0;
}

extern "C" int vgposp_potrf_set_emulation_structured(int on) {
  using namespace vgposp;
  clear_error();
  VG_CHECK_ARG(on == 0 || on == 1, 1);
  g_tri_on.store(on, std::memory_order_relaxed);
  return 0;
}

extern "C" int vgposp_potrf_emulation_structured(void) {
  return vgposp::gemm_emul_tri_enabled() ? 1 : 0;
}

// The planner of the structured drivers (pure: no GPU, no library): the steps of (kind, m, n, k)
// within `bytes` at the current block width, VGPOSP_EMUL_TRI_STEP_FIELDS int64 per step written
// to steps[0 .. cap_steps) (tile, r0, r1, c0, c1, ka, kb, i0, i1, j0, j1, k0, k1, tile_bytes),
// the int8 flops of all of them to *flops.  Returns the number of steps, -1 when the shape is not
// a structured product or nothing fits.
extern "C" int64_t vgposp_gemm_emulation_tri_plan(int kind, int64_t m, int64_t n, int64_t k,
                                                  size_t bytes, int64_t* steps, int64_t cap_steps,
                                                  double* flops) {
  using namespace vgposp;
  clear_error();
  if (kind < 0 || kind > 2 || !tri_dims_ok(kind, m, n, k)) return -1;
  std::vector<TriStep> plan;
  if (!tri_plan(kind, m, n, k, bytes, tri_block_width(kind), plan)) return -1;
  double fl = 0.0;
  for (size_t q = 0; q < plan.size(); ++q) {
    const TriStep& t = plan[q];
    fl += 2.0 * EMUL_NMOD * (double)(t.i1 - t.i0) * (t.j1 - t.j0) * tri_step_depth(t);
    if (steps != nullptr && (int64_t)q < cap_steps) {
      const int64_t f[VGPOSP_EMUL_TRI_STEP_FIELDS] = {t.tile, t.r0, t.r1, t.c0, t.c1, t.ka, t.kb,
                                                      t.i0,   t.i1, t.j0, t.j1, t.k0, t.k1,
                                                      t.tile_bytes};
      std::copy(f, f + VGPOSP_EMUL_TRI_STEP_FIELDS, steps + q * VGPOSP_EMUL_TRI_STEP_FIELDS);
    }
  }
  if (flops != nullptr) *flops = fl;
  return (int64_t)plan.size();
}

extern "C" int vgposp_gemm_emulated_tri(int kind, int64_t m, int64_t n, int64_t k, double alpha,
                                        const double* A, int64_t lda, const double* B, int64_t ldb,
                                        double beta, double* C, int64_t ldc, void* ws,
                                        size_t ws_bytes, void* stream) {
  using namespace vgposp;
  clear_error();
  VG_CHECK_ARG(kind >= 0 && kind <= 2, 1);
  VG_CHECK_ARG(m > 0, 2);
  VG_CHECK_ARG(n > 0, 3);
  VG_CHECK_ARG(tri_dims_ok(kind, m, n, k), 4);
  VG_CHECK_ARG(A != nullptr, 6);
  VG_CHECK_ARG(lda >= k, 7);
  VG_CHECK_ARG(kind == VGPOSP_EMUL_SYRK_LOWER || (B != nullptr && ldb >= n), 8);
  VG_CHECK_ARG(C != nullptr && ldc >= n, 11);
  VG_CHECK_ARG(ws != nullptr, 13);
  if (!gemm_emul_available()) {
    set_error("vgposp_gemm_emulated_tri: libhipblaslt.so.1 not found");
    return VGPOSP_E_UNSUPPORTED;
  }
  const int rc = gemm_emulated_tri(kind, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, ws, ws_bytes,
                                   as_stream(stream));
  if (rc == 1) {
    set_error("vgposp_gemm_emulated_tri: no int8 kernel, or %zu bytes hold no tile, for kind %d "
              "%lld x %lld x %lld", ws_bytes, kind, (long long)m, (long long)n, (long long)k);
    return VGPOSP_E_UNSUPPORTED;
  }
  return rc;
}

extern "C" int vgposp_potrf_set_emulation(int64_t min_dim, int moduli) {
  using namespace vgposp;
  clear_error();
  VG_CHECK_ARG(min_dim >= 256 && min_dim % 256 == 0, 1);
  VG_CHECK_ARG(moduli == 0 || moduli == EMUL_NMOD, 2);
  g_emul_min_dim.store(min_dim, std::memory_order_relaxed);
  g_emul_moduli.store(moduli, std::memory_order_relaxed);
  return 0;
}

extern "C" int vgposp_potrf_emulation(int64_t* min_dim, int* moduli) {
  using namespace vgposp;
  clear_error();
  VG_CHECK_ARG(min_dim != nullptr, 1);
  VG_CHECK_ARG(moduli != nullptr, 2);
  gemm_emul_config(min_dim, moduli);
  return 0;
}

extern "C" size_t vgposp_gemm_emulated_workspace_bytes(int64_t m, int64_t n, int64_t k) {
  return vgposp::gemm_emul_ws_bytes(m, n, k);
}

extern "C" int vgposp_gemm_emulated(int transa, int transb, int64_t m, int64_t n, int64_t k,
                                    double alpha, const double* A, int64_t lda, const double* B,
                                    int64_t ldb, double beta, double* C, int64_t ldc, void* ws,
                                    size_t ws_bytes, void* stream) {
  using namespace vgposp;
  clear_error();
  VG_CHECK_ARG(m >= 0, 3);
  VG_CHECK_ARG(n >= 0, 4);
  VG_CHECK_ARG(k >= 0 && k <= 65536, 5);
  VG_CHECK_ARG(A != nullptr || m == 0 || k == 0, 7);
  VG_CHECK_ARG(lda >= (transa ? (m > 0 ? m : 1) : (k > 0 ? k : 1)), 8);
  VG_CHECK_ARG(B != nullptr || n == 0 || k == 0, 9);
  VG_CHECK_ARG(ldb >= (transb ? (k > 0 ? k : 1) : (n > 0 ? n : 1)), 10);
  VG_CHECK_ARG(C != nullptr || m == 0 || n == 0, 12);
  VG_CHECK_ARG(ldc >= (n > 0 ? n : 1), 13);
  if (m == 0 || n == 0) return 0;
  if (k == 0)  // an empty sum: the fp64 kernel's beta pass
    return gemm_launch(transa, transb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, VGPOSP_FULL, 0,
                       0, as_stream(stream));
  if (!gemm_emul_available()) {
    set_error("vgposp_gemm_emulated: libhipblaslt.so.1 not found");
    return VGPOSP_E_UNSUPPORTED;
  }
  const size_t need = gemm_emul_ws_bytes(m, n, k);
  if (ws == nullptr || ws_bytes < need) {
    set_error("vgposp_gemm_emulated: workspace %zu < %zu bytes", ws_bytes, need);
    return VGPOSP_E_WS;
  }
  const int rc = gemm_emulated(transa, transb, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, ws,
                               as_stream(stream));
  if (rc == 1) {
    set_error("vgposp_gemm_emulated: no int8 kernel for %lld x %lld x %lld", (long long)m,
              (long long)n, (long long)k);
    return VGPOSP_E_UNSUPPORTED;
  }
  return rc;
}

// The host side of the reconstruction, as the kernel runs it: sixteen residues (any
// representatives) -> the symmetric mixed-radix digits and their integer rounded to fp64.
extern "C" int vgposp_gemm_emulation_garner(const int32_t* residues, int32_t* digits, double* value) {
  using namespace vgposp;
  clear_error();
  VG_CHECK_ARG(residues != nullptr, 1);
  VG_CHECK_ARG(digits != nullptr, 2);
  int c[EMUL_NMOD], v[EMUL_NMOD];
  for (int t = 0; t < EMUL_NMOD; ++t) c[t] = residues[t];
  emul_garner(c, v);
  for (int t = 0; t < EMUL_NMOD; ++t) digits[t] = v[t];
  if (value != nullptr) *value = emul_value(v);
  return 0;
}
