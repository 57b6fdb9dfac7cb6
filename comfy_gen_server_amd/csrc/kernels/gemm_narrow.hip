// Narrow-K linear with an optional fused LayerNorm for the dim-180 / dim-60 Swin-family upscalers on gfx950, and
// the row LayerNorm for C % 8 != 0 that goes with it.
//
//   y = act(LN?(x) W^T + bias) (+ residual)        bf16 in / out, fp32 accumulate, 4 <= K <= 384, K % 4 == 0
//
// K = 180 (SwinIR-M, Swin2SR, HAT, DAT), K = 60 (the lightweight variants) and their fc2 at K = 360 / 120 fail the
// K % 8 / K % 32 rules of the tiled GEMMs (16-byte, K-tiled loaders). The work is memory-bound -- 13 GFLOP against
// 94 MB for qkv at 65536 tokens -- so the kernel is built around how often a byte moves, not around MFMA rate: the
// whole K of a row tile is resident, there is no K loop over global memory, and LN(x) never exists in HBM.
//
// Work split. One workgroup (4 waves) owns a tile of TM = 128 rows (64 where KP > 256) and ALL N columns of it;
// KP = K padded to the kernel's instance (32, 64, 128, 192, 256, 384). x is read from HBM exactly once, y written
// once; W (N x K, at most 1080 x 384) comes from L2 once per workgroup.
//
// Data movement. The row tile is read in 8-byte units (K % 4 == 0 is all that dim 180 / 60 rows are aligned to) into
// LDS rows of LDX = KP + 8 elements (an odd number of 16-byte slots, so the 16 rows of a fragment read spread over
// the banks); the pad [K, KP) is zeroed in LDS once and never touched again. With LN a row's mean and variance are
// taken in fp32, two-pass, by 4 lanes a row (each sums its 8-byte units as (a + b) + (c + d), one after another, then a
// 2-step butterfly), and the row is normalised IN PLACE, ((v - mean) rstd) gamma + beta rounded to bf16: the value the
// row LayerNorm kernel stores, so no derived weights and no statistics tensor are needed. Each wave then pulls the
// MFMA fragments of its TM / 4 rows into registers ONCE (RB * KS bf16x8: 48 VGPRs at KP = 192) and keeps them for every
// column chunk. After a barrier the staging area is dead and is reused as the double buffer of W chunks of NC = TM / 2
// output columns: the same pitch LDX, so the zeroed pad columns serve W as well. The next chunk's global loads are in
// flight (registers) while this one computes; one barrier a chunk.
//
// Compute. v_mfma_f32_16x16x32_bf16 with W as the A operand (16 output channels on the rows) and x as B (16 tile rows
// on the columns), as dense.hip does: lane (fr = lane & 15, fq = lane >> 4) ends up with the 4 consecutive output
// channels 16 cb + 4 fq .. + 3 of row fr. Bias is one 8-byte read, the residual one 8-byte load, the store one packed
// 8-byte bf16 store; a partial last chunk and a partial last row tile are masked per lane (N % 4 == 0: a lane's four
// channels are all inside or all outside), nothing outside [M, N] is written and pitch padding is never touched.
//
// Budget. LDS = TM * LDX * 2 bytes: 51200 at KP = 192, 67584 at KP = 256, 50176 at KP = 384. Registers as compiled:
// 162 VGPRs + 40 AGPRs at KP = 192, 194 + 40 at KP = 256, 132 + 12 at KP = 384: two workgroups a CU (three at
// KP = 384), so one workgroup's loads and stores overlap the other's MFMAs. No scratch (the build fails on any), no
// workspace, no host synchronisation: capturable.
#include "common.h"

namespace {

struct NarrowArgs {
  const u16* x;
  const u16* w;
  const u16* bias;
  const u16* gamma;
  const u16* beta;
  const u16* res;
  u16* y;
  long long lda, ldr, ldc, M;
  int N, K, act;
  float eps;
};

template <int KS>
struct NarrowCfg {
  static constexpr int KP = 32 * KS;
  static constexpr int TM = KP > 256 ? 64 : 128;   // rows of a tile
  static constexpr int RB = TM / 64;               // 16-row blocks a wave
  static constexpr int NC = TM / 2;                // output columns of a W chunk (two chunks fill the staging area)
  static constexpr int NCB = NC / 16;
  static constexpr int LDX = KP + 8;               // LDS row (elements)
  static constexpr int NU = NC * KS / 32;          // 8-byte units of a W chunk per thread (K = KP)
  static constexpr int LDS = TM * LDX * 2;
};

// sum of the four values of an 8-byte unit as a tree: two dependent additions
__device__ __forceinline__ float sum4(float4 v) { return (v.x + v.y) + (v.z + v.w); }

template <int KS, bool LN>
__global__ __launch_bounds__(256) void gemm_narrow_kernel(const NarrowArgs a) {
  using Cf = NarrowCfg<KS>;
  constexpr int KP = Cf::KP, TM = Cf::TM, RB = Cf::RB, NC = Cf::NC, NCB = Cf::NCB, LDX = Cf::LDX, NU = Cf::NU;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u16* S = reinterpret_cast<u16*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const long long row0 = (long long)blockIdx.x * TM;
  const int rows = (int)min((long long)TM, a.M - row0);
  const int K = a.K, N = a.N, ku = K >> 2;        // ku: 8-byte units of a row
  const int nchunks = (N + NC - 1) / NC;

  // ---- W chunk c: rows [c NC, c NC + NC) of the contiguous W are one run of 8-byte units. Unit tid + 256 i goes to
  // LDS offset woff[i] (the same for every chunk); rows past N are staged as zeros.
  int woff[NU];
  {
    int r = tid / ku, u = tid - r * ku;
    const int dr = 256 / ku, du = 256 - dr * ku;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      woff[i] = tid + 256 * i < NC * ku ? r * LDX + 4 * u : -1;
      r += dr;
      u += du;
      if (u >= ku) { u -= ku; ++r; }
    }
  }
  uint2 wr[NU];
  auto load = [&](int c) {
    const int nun = min(NC, N - c * NC) * ku;
    const uint2* src = reinterpret_cast<const uint2*>(a.w + (size_t)c * NC * K);
#pragma unroll
    for (int i = 0; i < NU; ++i) wr[i] = tid + 256 * i < nun ? src[tid + 256 * i] : uint2{0u, 0u};
  };
  auto put = [&](int buf) {
    u16* B = S + buf * NC * LDX;
#pragma unroll
    for (int i = 0; i < NU; ++i)
      if (woff[i] >= 0) *reinterpret_cast<uint2*>(&B[woff[i]]) = wr[i];
  };
  load(0);

  // ---- the row tile: HBM -> LDS in 8-byte units, the K pad zeroed; rows past M staged as zeros
  if (K < KP) {
    const int pu = (KP - K) >> 2;
    for (int idx = tid; idx < TM * pu; idx += 256) {
      const int r = idx / pu, u = idx - r * pu;
      *reinterpret_cast<uint2*>(&S[r * LDX + K + 4 * u]) = uint2{0u, 0u};
    }
  }
  {
    int r = tid / ku, u = tid - r * ku;
    const int dr = 256 / ku, du = 256 - dr * ku;
    const u16* xt = a.x + (size_t)row0 * a.lda;
#pragma unroll 4
    for (int idx = tid; idx < TM * ku; idx += 256) {
      uint2 v = uint2{0u, 0u};
      if (r < rows) v = *reinterpret_cast<const uint2*>(xt + (size_t)r * a.lda + 4 * u);
      *reinterpret_cast<uint2*>(&S[r * LDX + 4 * u]) = v;
      r += dr;
      u += du;
      if (u >= ku) { u -= ku; ++r; }
    }
  }
  __syncthreads();

  // ---- LayerNorm of the staged rows, in place: 4 lanes a row, fp32 two-pass statistics
  if constexpr (LN) {
    const int l4 = tid & 3;
    const float fK = (float)K;
#pragma unroll
    for (int r = tid >> 2; r < TM; r += 64) {
      u16* xr = S + r * LDX;
      float s = 0.f;
      for (int u = l4; u < ku; u += 4) s += sum4(unpack4_bf16(*reinterpret_cast<const uint2*>(xr + 4 * u)));
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      const float mean = s / fK;
      float q = 0.f;
      for (int u = l4; u < ku; u += 4) {
        const float4 v = unpack4_bf16(*reinterpret_cast<const uint2*>(xr + 4 * u));
        const float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
        q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
      }
      q += __shfl_xor(q, 1, 64);
      q += __shfl_xor(q, 2, 64);
      const float rstd = rsqrtf(q / fK + a.eps);
      for (int u = l4; u < ku; u += 4) {
        const float4 v = unpack4_bf16(*reinterpret_cast<const uint2*>(xr + 4 * u));
        float4 g = float4{1.f, 1.f, 1.f, 1.f}, b = float4{0.f, 0.f, 0.f, 0.f};
        if (a.gamma) g = unpack4_bf16(*reinterpret_cast<const uint2*>(a.gamma + 4 * u));
        if (a.beta) b = unpack4_bf16(*reinterpret_cast<const uint2*>(a.beta + 4 * u));
        *reinterpret_cast<uint2*>(xr + 4 * u) =
            pack4_bf16((v.x - mean) * rstd * g.x + b.x, (v.y - mean) * rstd * g.y + b.y,
                       (v.z - mean) * rstd * g.z + b.z, (v.w - mean) * rstd * g.w + b.w);
      }
    }
    __syncthreads();
  }

  // ---- this wave's rows as MFMA B fragments, held for every column chunk
  bf16x8 xf[RB][KS];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int kb = 0; kb < KS; ++kb)
      xf[rb][kb] = *reinterpret_cast<const bf16x8*>(&S[((wave * RB + rb) * 16 + fr) * LDX + 32 * kb + 8 * fq]);
  __syncthreads();        // the staging area is dead: it becomes the W double buffer
  put(0);
  __syncthreads();

  int buf = 0;
  for (int c = 0; c < nchunks; ++c) {
    const bool more = c + 1 < nchunks;
    if (more) load(c + 1);
    f32x4 acc[RB][NCB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const u16* B = S + buf * NC * LDX;
#pragma unroll
    for (int kb = 0; kb < KS; ++kb)
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const bf16x8 wf = *reinterpret_cast<const bf16x8*>(&B[(cb * 16 + fr) * LDX + 32 * kb + 8 * fq]);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
          acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf[rb][kb], acc[rb][cb], 0, 0, 0);
      }
    if (more) put(buf ^ 1);
    __syncthreads();
    buf ^= 1;
    // acc[rb][cb][q] = (channel c NC + 16 cb + 4 fq + q, tile row (wave RB + rb) 16 + fr)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const int col = c * NC + 16 * cb + 4 * fq;
      if (col >= N) continue;
      float4 bv = float4{0.f, 0.f, 0.f, 0.f};
      if (a.bias) bv = unpack4_bf16(*reinterpret_cast<const uint2*>(a.bias + col));
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const int r = (wave * RB + rb) * 16 + fr;
        if (r >= rows) continue;
        float v0 = acc[rb][cb][0] + bv.x, v1 = acc[rb][cb][1] + bv.y, v2 = acc[rb][cb][2] + bv.z,
              v3 = acc[rb][cb][3] + bv.w;
        if (a.act) {
          v0 = act_apply(a.act, v0, 0.f);
          v1 = act_apply(a.act, v1, 0.f);
          v2 = act_apply(a.act, v2, 0.f);
          v3 = act_apply(a.act, v3, 0.f);
        }
        if (a.res) {
          const float4 rv = unpack4_bf16(*reinterpret_cast<const uint2*>(a.res + (size_t)(row0 + r) * a.ldr + col));
          v0 += rv.x;
          v1 += rv.y;
          v2 += rv.z;
          v3 += rv.w;
        }
        *reinterpret_cast<uint2*>(a.y + (size_t)(row0 + r) * a.ldc + col) = pack4_bf16(v0, v1, v2, v3);
      }
    }
  }
}

template <int KS>
int gemm_narrow_launch(const NarrowArgs& a, bool ln, hipStream_t stream) {
  using Cf = NarrowCfg<KS>;
  const long long nwg = (a.M + Cf::TM - 1) / Cf::TM;
  if (nwg > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (ln) {
    max_dynamic_lds_once<gemm_narrow_kernel<KS, true>>(Cf::LDS);
    gemm_narrow_kernel<KS, true><<<dim3((unsigned)nwg), 256, Cf::LDS, stream>>>(a);
  } else {
    max_dynamic_lds_once<gemm_narrow_kernel<KS, false>>(Cf::LDS);
    gemm_narrow_kernel<KS, false><<<dim3((unsigned)nwg), 256, Cf::LDS, stream>>>(a);
  }
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Row LayerNorm for C % 4 == 0, C <= 1024 (the rows the 16-byte kernel of norm.hip cannot take): 16 lanes a row, the
// row in registers as up to MAXU 8-byte units a lane, fp32 two-pass statistics (a lane adds its units one after
// another, each as (a + b) + (c + d); then a 4-step butterfly), y = ((x - mean) rstd) w + b (+ residual), the
// residual added in fp32 before the one rounding.
// ------------------------------------------------------------------------------------------------
template <int MAXU>
__global__ __launch_bounds__(256) void layernorm_rows4_kernel(const u16* __restrict__ x, u16* __restrict__ y,
                                                             const u16* __restrict__ w, const u16* __restrict__ b,
                                                             const u16* __restrict__ res, long long rows, int C,
                                                             float eps) {
  const int l = threadIdx.x & 15;
  const long long row = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = row < rows;       // dead rows still join the shuffles
  const int nu = C >> 2;
  const size_t ro = (size_t)(live ? row : 0) * C;
  float4 v[MAXU];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MAXU; ++k) {
    const int u = l + 16 * k;
    if (live && u < nu) {
      v[k] = unpack4_bf16(reinterpret_cast<const uint2*>(x + ro)[u]);
      s += sum4(v[k]);
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float mean = s / C;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < MAXU; ++k) {
    const int u = l + 16 * k;
    if (live && u < nu) {
      const float d0 = v[k].x - mean, d1 = v[k].y - mean, d2 = v[k].z - mean, d3 = v[k].w - mean;
      q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  const float rstd = rsqrtf(q / C + eps);
  if (!live) return;
#pragma unroll
  for (int k = 0; k < MAXU; ++k) {
    const int u = l + 16 * k;
    if (u < nu) {
      float4 g = float4{1.f, 1.f, 1.f, 1.f}, bb = float4{0.f, 0.f, 0.f, 0.f};
      if (w) g = unpack4_bf16(reinterpret_cast<const uint2*>(w)[u]);
      if (b) bb = unpack4_bf16(reinterpret_cast<const uint2*>(b)[u]);
      float f0 = (v[k].x - mean) * rstd * g.x + bb.x, f1 = (v[k].y - mean) * rstd * g.y + bb.y,
            f2 = (v[k].z - mean) * rstd * g.z + bb.z, f3 = (v[k].w - mean) * rstd * g.w + bb.w;
      if (res) {
        const float4 rv = unpack4_bf16(reinterpret_cast<const uint2*>(res + ro)[u]);
        f0 += rv.x;
        f1 += rv.y;
        f2 += rv.z;
        f3 += rv.w;
      }
      reinterpret_cast<uint2*>(y + ro)[u] = pack4_bf16(f0, f1, f2, f3);
    }
  }
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace

// y[M, N] = act(LN?(x[M, K]) w[N, K]^T + bias) (+ res), bf16. x rows at pitch lda, res at ldr, y at ldc (elements);
// w contiguous; bias [N], gamma / beta [K] nullable; ln != 0: LayerNorm over K with eps first (gamma / beta are
// ignored without it); act a CgsAct code up to CGS_ACT_RELU, applied before the residual. Domain: 4 <= K <= 384,
// K % 4 == 0, N % 4 == 0, pitches >= the row and multiples of 4, every pointer 8-byte aligned, ceil(M / tile) within
// int; anything else is hipErrorInvalidValue and nothing is launched.
CGS_EXPORT int cgs_gemm_narrow(const void* x, long long lda, const void* w, const void* bias, const void* gamma,
                               const void* beta, float eps, int ln, const void* res, long long ldr, void* y,
                               long long ldc, long long M, int N, int K, int act, hipStream_t stream) {
  const int E = (int)hipErrorInvalidValue;
  if (!x || !w || !y || M <= 0 || N <= 0 || (N & 3) || K < 4 || K > 384 || (K & 3)) return E;
  if (lda < K || (lda & 3) || ldc < N || (ldc & 3) || (res && (ldr < N || (ldr & 3)))) return E;
  if (!aligned8(x) || !aligned8(w) || !aligned8(y) || !aligned8(bias) || !aligned8(res)) return E;
  if (ln && (!aligned8(gamma) || !aligned8(beta))) return E;
  if (act < CGS_ACT_NONE || act > CGS_ACT_RELU) return E;
  const NarrowArgs a{(const u16*)x, (const u16*)w, (const u16*)bias, ln ? (const u16*)gamma : nullptr,
                     ln ? (const u16*)beta : nullptr, (const u16*)res, (u16*)y, lda, res ? ldr : 0, ldc, M, N, K, act,
                     eps};
  const int ks = (K + 31) / 32;
  if (ks <= 1) return gemm_narrow_launch<1>(a, ln != 0, stream);
  if (ks <= 2) return gemm_narrow_launch<2>(a, ln != 0, stream);
  if (ks <= 4) return gemm_narrow_launch<4>(a, ln != 0, stream);
  if (ks <= 6) return gemm_narrow_launch<6>(a, ln != 0, stream);
  if (ks <= 8) return gemm_narrow_launch<8>(a, ln != 0, stream);
  return gemm_narrow_launch<12>(a, ln != 0, stream);
}

// y = LN(x) w + b (+ res) over rows of C bf16 values; x, y, res contiguous [rows, C], w / b [C], each of w, b, res
// nullable. Domain: 4 <= C <= 1024, C % 4 == 0, every pointer 8-byte aligned, rows / 16 within int; anything else is
// hipErrorInvalidValue and nothing is launched.
CGS_EXPORT int cgs_layernorm_rows4(const void* x, void* y, const void* w, const void* b, const void* res,
                                   long long rows, int C, float eps, hipStream_t stream) {
  const int E = (int)hipErrorInvalidValue;
  if (!x || !y || rows <= 0 || C < 4 || C > 1024 || (C & 3)) return E;
  if (!aligned8(x) || !aligned8(y) || !aligned8(w) || !aligned8(b) || !aligned8(res)) return E;
  const long long nwg = (rows + 15) / 16;
  if (nwg > 0x7fffffffLL) return E;
  if (C <= 256)
    layernorm_rows4_kernel<4><<<dim3((unsigned)nwg), 256, 0, stream>>>((const u16*)x, (u16*)y, (const u16*)w,
                                                                      (const u16*)b, (const u16*)res, rows, C, eps);
  else
    layernorm_rows4_kernel<16><<<dim3((unsigned)nwg), 256, 0, stream>>>((const u16*)x, (u16*)y, (const u16*)w,
                                                                       (const u16*)b, (const u16*)res, rows, C, eps);
  return (int)hipGetLastError();
}
