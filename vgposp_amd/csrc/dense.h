// The dense fp64 layer's internal interface: the only declaration of every function that one .hip
// file defines and another calls.  The defining files include it too, so a changed signature is a
// compile error.  Default arguments live here and nowhere else.
#pragma once

#include "common.h"

namespace vgposp {

// ---- gemm.hip -------------------------------------------------------------------------------
int gemm_launch(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                const double* A, int64_t lda, const double* B, int64_t ldb, double beta,
                double* C, int64_t ldc, int uplo_c, int tri_a, int tri_b, hipStream_t stream);
int gemm_launch_split(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                      const double* A, int64_t lda, const double* B, int64_t ldb, double beta,
                      double* C, int64_t ldc, int uplo_c, int tri_a, int tri_b, int nsplit,
                      double* part, hipStream_t stream);
int gemm_launch_batched(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                        const double* A, int64_t lda, int64_t sA, const double* B, int64_t ldb,
                        int64_t sB, double beta, double* C, int64_t ldc, int64_t sC, int uplo_c,
                        int tri_a, int tri_b, int nsplit, double* part, int64_t sP, int batch,
                        hipStream_t stream);
int gemm_auto_splits(int64_t m, int64_t n, int64_t k, int uplo_c, int transa);
void gemm_set_abort(const int* flag);
const int* gemm_abort_flag();
int gemm_strassen(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                  const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C,
                  int64_t ldc, int levels, int64_t min_dim, double* ws, int64_t ws_elems,
                  hipStream_t stream);
int64_t gemm_strassen_ws_elems(int64_t m, int64_t n, int64_t k, int levels, int64_t min_dim);
void gemm_strassen_config(int64_t* min_dim, int* levels);

// ---- gemm_emul.hip --------------------------------------------------------------------------
// fp64 products on the int8 matrix cores.  gemm_emulated returns 1, with nothing written, when
// the int8 library is absent or has no kernel for a block shape: the caller takes its fp64 path.
bool gemm_emul_available();
size_t gemm_emul_ws_bytes(int64_t m, int64_t n, int64_t k);
void gemm_emul_config(int64_t* min_dim, int* moduli);
int gemm_emul_scale_bits(int64_t k);
int gemm_emulated(int transa, int transb, int64_t m, int64_t n, int64_t k, double alpha,
                  const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C,
                  int64_t ldc, void* ws, hipStream_t stream);
// The structured products (kind: VGPOSP_EMUL_SYRK_LOWER / _TRMM_B / _TRMM_A) as a staircase of
// int8 block products within ws_bytes; 1 with nothing written like gemm_emulated.
bool gemm_emul_tri_enabled();
int gemm_emulated_tri(int kind, int64_t m, int64_t n, int64_t k, double alpha, const double* A,
                      int64_t lda, const double* B, int64_t ldb, double beta, double* C,
                      int64_t ldc, void* ws, size_t ws_bytes, hipStream_t stream);

// ---- potrf.hip ------------------------------------------------------------------------------
int potrf_one(double* A, int64_t n, int64_t lda, int invert, double* diag_out, int* info,
              void* ws, hipStream_t stream, bool early = false, bool strassen = true,
              bool compact = false);  // compact: ws is potrf_ws_bytes_compact(n)
int potrf_batched(double* A, int64_t n, int64_t lda, int64_t sA, int batch, int invert,
                  double* diag_out, int* info, void* ws, hipStream_t stream, bool use_part);
size_t potrf_ws_bytes(int64_t n);
size_t potrf_ws_bytes_compact(int64_t n);
size_t potrf_ws_bytes_opt(int64_t n, bool use_part);
int partial_inverse(double* A, int64_t n, int64_t lda, int64_t c0, int64_t c1, double* tmp,
                    void* ws, hipStream_t s);
size_t partial_inverse_tmp_bytes(int64_t n, int64_t c0, int64_t c1);
int trsm_left(const double* L, int64_t n, int64_t ldl, int trans, double* B, int64_t m,
              int64_t ldb, void* ws, hipStream_t s);
size_t trsm_ws_bytes(int64_t n, int64_t m);

}  // namespace vgposp
