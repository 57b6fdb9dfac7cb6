// Host side of the bf16 GEMM launchers (gemm.hip, gemm_w6.hip): the operands of one call as one struct, built
// once per exported entry from its parameter list and passed by reference below that (as ConvArgs is for the
// convs, but never a kernel argument: the kernels keep their positional parameters).
#pragma once
#include "common.h"
#include "mfma_core.h"

// Kernel choice of cgs_gemm_bf16_v / _lnfold_v / _rowstats_v / _splitk. The numbers are ABI: the op layer passes
// them (ops/core.py, the names of data/tune_mi355x.json map to them).
enum GemmVariant {
  kVariantProcess = -2,    // cgs_gemm_bf16_v only: the process-wide choice of cgs_gemm_set_variant
  kVariantAuto = -1,
  kVariantV1 = 1,          // 128 x 128, register-staged
  kVariantV2 = 2,          // 256 x 128 / 256, LDS-DMA ring
  kVariantV3 = 3,          // mc::tile 256 x BN, 4 waves
  kVariantV4 = 4,          // mc::tile 256 x BN, 8 waves
  kVariantV5 = 5,          // 256 x 256 ping-pong
  kVariantV6 = 6,          // 256 x 160 ping-pong
  kVariantV7 = 7,          // persistent 256 x 256 ping-pong
  kVariantV8 = 8,          // mc::tile 128 x 128 (the small tiles: 8, 10..14)
  kVariantSkinny = 9,      // M <= 128
  kVariantT64x128 = 10,
  kVariantT128x64 = 11,
  kVariantT64x128s6 = 12,  // 6-stage ring
  kVariantT128x64s6 = 13,
  kVariantT128s5 = 14,     // 128 x 128, 5 stages
  kVariantW6 = 16,         // gemm_w6.hip, 256 x 256
  kVariantW6n160 = 17,     // gemm_w6.hip, 256 x 160
  kVariantV6m128 = 19,     // v6 on 128 x 160 tiles
  kVariantV6w4 = 20,       // v6 on 128 x 80 tiles, one wave group
};
inline bool small_tile_variant(int v) { return v == kVariantV8 || (v >= kVariantT64x128 && v <= kVariantT128s5); }

CGS_EXPORT int cgs_gemm_w6_ok(int M, int N, int K, long long lda, long long ldw, long long ldc, long long ldr, int epi,
                              int bn);

struct GemmArgs {
  const void* A;           // [M][lda] bf16
  const void* W;           // [N][ldw] bf16
  void* C;                 // [M][ldc] bf16 (fp32 with MC_EPI_F32OUT)
  const void* bias;        // [N] bf16 or null
  const void* R;           // [M][ldr] bf16 residual or null
  const float* rs;         // MC_EPI_LNFOLD: [M][2] (mean, rstd) rows
  const float* cs;         //                [N] column sums of W' = W * gamma
  int M, N, K;
  long long lda, ldw, ldc, ldr;
  int epi;                 // MC_EPI_* flags (+ activation code bits, CGS_EPI_ACT_MASK)
  float alpha;
  hipStream_t stream;
  void* ws = nullptr;      // split-K workspace (v7 tail, skinny, cgs_gemm_bf16_splitk) or null
  long long ws_bytes = 0;
  float* part = nullptr;   // per-row LayerNorm statistics partials out (pq::run RSO) or null

  // 16-B aligned rows and operands for the LDS-DMA kernels (mc::tile, the ping-pong loops)
  bool v3_ok() const {
    const int nout = (epi & MC_EPI_GEGLU) ? N / 2 : N;
    return (K % 32 == 0) && (lda % 8 == 0) && (ldw % 8 == 0) && (nout % 8 == 0) && (ldc % 8 == 0) &&
           (!(epi & MC_EPI_RESIDUAL) || ldr % 8 == 0) &&
           ((((uintptr_t)A | (uintptr_t)W | (uintptr_t)C | (uintptr_t)R)) % 16 == 0);
  }
  // v2 needs K % 64 == 0 and 16-B aligned rows; it pays off once there are >= ~256 big tiles' worth of work
  // (otherwise the 128x128 kernel keeps more CUs busy)
  bool v2_ok() const {
    return (K % 64 == 0) && (lda % 8 == 0) && (ldw % 8 == 0) && M >= 256 && N >= 128 &&
           (((uintptr_t)A | (uintptr_t)W) % 16 == 0);
  }
  // w6's shape / stride domain and pointer alignment (gemm_w6 returns hipErrorInvalidValue otherwise)
  bool w6_ok(int bn) const {
    return cgs_gemm_w6_ok(M, N, K, lda, ldw, ldc, ldr, epi, bn) &&
           ((uintptr_t)A | (uintptr_t)W | (uintptr_t)C) % 16 == 0 &&
           (!(epi & MC_EPI_RESIDUAL) || (uintptr_t)R % 16 == 0) && (!(epi & MC_EPI_BIAS) || (uintptr_t)bias % 16 == 0);
  }
  // what every LayerNorm-folded entry needs (rs / cs, K % 64, K >= 128, aligned rows, no residual, < 4 GiB operands)
  bool lnfold_ok() const {
    const int nout = (epi & MC_EPI_GEGLU) ? N / 2 : N;
    return !(!rs || !cs || K % 64 || K < 128 || lda % 8 || ldw % 8 || ldc % 8 || nout % 8 || (epi & MC_EPI_RESIDUAL) ||
             ((uintptr_t)A | (uintptr_t)W | (uintptr_t)C) % 16 || ((uintptr_t)bias % 8) || ((uintptr_t)cs % 16) ||
             ((uintptr_t)rs % 8) || (long long)M * lda * 2 >= (1ll << 32) || (long long)N * ldw * 2 >= (1ll << 32));
  }
};

// gemm_w6.hip: the w6 kernel on a (dbg: ablation probes; group_m <= 0: 4; grid_cap 0: one workgroup per CU; bn:
// tile width 256 or 160)
int gemm_w6(const GemmArgs& a, int dbg, int group_m, int grid_cap, int bn);

// Launch a kernel whose parameters begin (A, W, C, bias, R, M, N, K, lda, ldw, ldc, ldr, epi, alpha): the struct
// expands into that prefix, tail follows it. Dynamic LDS is raised to lds_bytes first (max_dynamic_lds_once).
template <auto Kern, typename... Tail>
inline void launch_gemm(dim3 grid, dim3 block, int lds_bytes, const GemmArgs& a, Tail... tail) {
  if (lds_bytes > 0) max_dynamic_lds_once<Kern>(lds_bytes);
  Kern<<<grid, block, lds_bytes, a.stream>>>((const u16*)a.A, (const u16*)a.W, (u16*)a.C, (const u16*)a.bias,
                                             (const u16*)a.R, a.M, a.N, a.K, a.lda, a.ldw, a.ldc, a.ldr, a.epi,
                                             a.alpha, tail...);
}
