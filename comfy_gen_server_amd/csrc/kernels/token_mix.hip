// Token-layout depthwise 3 x 3 conv and the adaptive interaction module (AIM) of DAT on gfx950.
//
// DAT mixes every attention with a depthwise-conv branch on v through two small gates, and gates its feed-forward
// with another depthwise conv (SGFN). All operands are token-major rows [B, H W, C] with C = 180 / 60 -- often channel
// slices of wider rows (the v third of the packed qkv, a half of the SGFN's hidden rows) -- so nothing here wants an
// NCHW or a contiguous NHWC copy. bf16 in and out, fp32 arithmetic, no atomics, every sum in a fixed order.
//
// 1. tok_dwconv3_kernel<EPI>: grid (16 x 16 patches, B), 256 threads.
//      y[b, p, c] = epi(bias[c] + sum_taps w[c, tap] x[b, p + tap, c])          stride 1, zero padding
//    x is (base, pixel pitch in elements); y is contiguous. The channels are walked in chunks of 64: the 18 x 18 halo of
//    a chunk is staged in LDS as 8-byte units (pixel-major, 128 bytes a pixel, 41472 bytes), zero outside the image
//    and in the pad channels; the next chunk's 21 units a thread are loaded into registers right after the current
//    image is complete, so they are in flight while it computes. Thread (cg = tid & 15, col = tid >> 4) owns 4
//    consecutive channels and one column of the patch: it walks the 18 halo rows once, reads 3 units a row and feeds
//    three rolling accumulators (the output rows r, r - 1, r - 2), so an LDS value is read three times, not nine; the
//    taps of an output are added ky-major after the bias. A wave's reads of a row are 512 consecutive bytes.
//      EPI_NONE     y = conv + b
//      EPI_BN_GELU  y = gelu(s (conv + b - mean) + beta), s = gamma rsqrt(var + eps) formed here from the four
//                   BatchNorm vectors; gelu is gelu_sig (common.h)
//      EPI_MUL      y = m (conv + b), m a second strided operand
//    With EPI_BN_GELU and a workspace it also writes fp32 per-patch, per-channel sums ws[b, patch, c] of the in-image
//    pixels of its own fp32 output (before rounding), or of the same patch of pool_src [B, N, C]: a thread adds its 16
//    rows in sequence, two shuffles join the 4 columns of a wave, the 4 waves are added in wave order.
// 2. aim_cmap_kernel: grid B. Adds the patch partials in patch order, divides by N, then
//      gate[c] = sigmoid(W2 gelu(bn(W1 mean + b1)) + b2)        hidden width hc <= 32, fp32 [B, C]
//    (a wave a hidden unit: a lane adds every 64th channel, wave_sum; a thread an output channel, hc fmas in sequence).
// 3. aim_mix_kernel<KP>: grid (64-token tiles, B), 4 waves, KP = C padded to 64 / 128 / 192 / 256. Both att and conv
//    rows of the tile are read once in 8-byte units and stay in registers for the mix; the SOURCE rows of the spatial
//    gate (att in a spatial block, conv in a channel block) also go to LDS rows of KP + 8 elements, zero in [C, KP) and
//    past the last token, beside W1 padded to 16 x KP. A wave owns 16 tokens: KP / 32 MFMAs 16x16x32 bf16 with W1 as the
//    A operand and the tokens as B leave lane (fr, fq) with hidden units 4 fq .. + 3 of token fr (hs <= 16; units past
//    hs have zero weights and zero BatchNorm scale, gelu(0) w2 = 0). BatchNorm + GELU on the accumulators, the dot
//    with w2 in sequence over the lane's four and two shuffles over fq, + b2, sigmoid: the token gate, through LDS.
//      y = att ga + conv gb        spatial: ga = channel gate, gb = token gate; channel: ga = token gate, gb = channel
//    and the bf16 rows leave in 8-byte stores.
//
// LDS: 41472 + 1024 B (conv), (64 + 16)(KP + 8) 2 + 256 B (mix: 42496 at KP = 256). No scratch (the build fails on any).
#include "common.h"

namespace {

constexpr int TD_P = 16;                 // patch edge
constexpr int TD_HP = TD_P + 2;          // halo edge
constexpr int TD_CH = 64;                // channels a chunk
constexpr int TD_NT = 256;
constexpr int TD_UNITS = TD_HP * TD_HP * (TD_CH / 4);
constexpr int TD_NU = (TD_UNITS + TD_NT - 1) / TD_NT;
constexpr int AIM_TM = 64;               // tokens a mix workgroup
constexpr int AIM_NP = 22;               // parameter pointers of cgs_aim_fwd
constexpr float LOG2E = 1.4426950408889634f;

enum { EPI_NONE = 0, EPI_BN_GELU = 1, EPI_MUL = 2 };
enum { AIM_SPATIAL = 0, AIM_CHANNEL = 1 };
// the parameter table of cgs_aim_fwd: the depthwise conv and its BatchNorm, the channel gate, the spatial gate
enum { P_DW_W, P_DW_B, P_DBN_W, P_DBN_B, P_DBN_M, P_DBN_V, P_C_W1, P_C_B1, P_CBN_W, P_CBN_B, P_CBN_M, P_CBN_V, P_C_W2,
       P_C_B2, P_S_W1, P_S_B1, P_SBN_W, P_SBN_B, P_SBN_M, P_SBN_V, P_S_W2, P_S_B2 };

struct TokConvArgs {
  const u16* x;
  const u16* w;           // [C, 9]
  const u16* bias;        // [C] or null
  const u16* bn_w;        // EPI_BN_GELU: gamma, beta, mean, var [C]
  const u16* bn_b;
  const u16* bn_m;
  const u16* bn_v;
  const u16* m;           // EPI_MUL
  const u16* pool_src;    // [B, N, C] or null
  u16* y;
  float* ws;              // [B, px py, C] or null
  long long xpitch, mpitch;
  float eps;
  int B, H, W, C, px, py;
};

struct AimArgs {
  const u16* p[AIM_NP];
  const u16* att;
  const u16* conv;
  u16* y;
  const float* part;      // [B, np, C]
  float* cgate;           // [B, C]
  float eps_c, eps_s;
  int B, N, C, hc, hs, np, kind;
};

__device__ __forceinline__ float sigmoid_f(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-x * LOG2E));
}

// gelu(s (pre - mean) + beta) with s = gamma rsqrt(var + eps)
__device__ __forceinline__ float bn_gelu(float pre, float gamma, float beta, float mean, float var, float eps) {
  const float s = gamma * rsqrtf(var + eps);
  return gelu_sig(__builtin_fmaf(s, pre - mean, beta));
}

template <int EPI>
__global__ __launch_bounds__(TD_NT) void tok_dwconv3_kernel(const TokConvArgs a) {
  __shared__ __attribute__((aligned(16))) uint2 halo[TD_UNITS];
  __shared__ float red[4][TD_CH];
  const int tid = threadIdx.x, cg = tid & 15, col = tid >> 4, lane = tid & 63, wave = tid >> 6;
  const int patch = blockIdx.x, b = blockIdx.y;
  const int pyi = patch / a.px, pxi = patch - pyi * a.px;
  const int y0 = pyi * TD_P, x0 = pxi * TD_P;
  const int H = a.H, W = a.W, C = a.C;
  const size_t img = (size_t)b * H * W;          // first token of the image
  const u16* xb = a.x + img * a.xpitch;
  const int nch = (C + TD_CH - 1) / TD_CH;

  uint2 r[TD_NU];
  auto load = [&](int ch) {
    const int c = ch * TD_CH + 4 * cg;           // u & 15 == cg for every unit of this thread
#pragma unroll
    for (int i = 0; i < TD_NU; ++i) {
      const int u = tid + i * TD_NT, hp = u >> 4, hy = hp / TD_HP, hx = hp - hy * TD_HP;
      const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
      r[i] = uint2{0u, 0u};
      if (u < TD_UNITS && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W && c < C)
        r[i] = *reinterpret_cast<const uint2*>(xb + ((size_t)gy * W + gx) * a.xpitch + c);
    }
  };
  load(0);

#pragma unroll 1
  for (int ch = 0; ch < nch; ++ch) {
    if (ch) __syncthreads();                     // every thread done with the previous image
#pragma unroll
    for (int i = 0; i < TD_NU; ++i) {
      const int u = tid + i * TD_NT;
      if (u < TD_UNITS) halo[u] = r[i];
    }
    __syncthreads();
    if (ch + 1 < nch) load(ch + 1);              // in flight during the taps below

    const int c = ch * TD_CH + 4 * cg;
    const bool live = c < C;
    float wt[4][9], bs[4], g[4], be[4], mu[4], va[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int t = 0; t < 9; ++t) wt[k][t] = live ? bf2f(a.w[(c + k) * 9 + t]) : 0.f;
      bs[k] = live && a.bias ? bf2f(a.bias[c + k]) : 0.f;
      g[k] = be[k] = mu[k] = 0.f;
      va[k] = 1.f;
      if (EPI == EPI_BN_GELU && live) {
        g[k] = bf2f(a.bn_w[c + k]);
        be[k] = bf2f(a.bn_b[c + k]);
        mu[k] = bf2f(a.bn_m[c + k]);
        va[k] = bf2f(a.bn_v[c + k]);
      }
    }
    const int gx = x0 + col;
    float acc[3][4], ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int hr = 0; hr < TD_HP; ++hr) {
      float h[3][4];
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const float4 v = unpack4_bf16(halo[(hr * TD_HP + col + dx) * 16 + cg]);
        h[dx][0] = v.x;
        h[dx][1] = v.y;
        h[dx][2] = v.z;
        h[dx][3] = v.w;
      }
      // halo row hr is tap row 0 of output row hr, tap row 1 of hr - 1 and tap row 2 of hr - 2, which it completes
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int orow = hr - ky;
        if (orow < 0 || orow >= TD_P) continue;
        float* ac = acc[orow % 3];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float s = ky == 0 ? bs[k] : ac[k];
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) s = __builtin_fmaf(wt[k][3 * ky + dx], h[dx][k], s);
          ac[k] = s;
        }
      }
      const int orow = hr - 2;
      if (orow < 0) continue;
      const int gy = y0 + orow;
      const bool in = live && gy < H && gx < W;
      const size_t tok = img + (size_t)(in ? gy : 0) * W + (in ? gx : 0);
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = acc[orow % 3][k];
      if (EPI == EPI_BN_GELU) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = bn_gelu(v[k], g[k], be[k], mu[k], va[k], a.eps);
        if (a.ws && in) {
          float4 q = float4{v[0], v[1], v[2], v[3]};
          if (a.pool_src) q = unpack4_bf16(*reinterpret_cast<const uint2*>(a.pool_src + tok * C + c));
          ps[0] += q.x;
          ps[1] += q.y;
          ps[2] += q.z;
          ps[3] += q.w;
        }
      }
      if (EPI == EPI_MUL && in) {
        const float4 q = unpack4_bf16(*reinterpret_cast<const uint2*>(a.m + tok * a.mpitch + c));
        v[0] *= q.x;
        v[1] *= q.y;
        v[2] *= q.z;
        v[3] *= q.w;
      }
      if (in) *reinterpret_cast<uint2*>(a.y + tok * C + c) = pack4_bf16(v[0], v[1], v[2], v[3]);
    }
    if (EPI == EPI_BN_GELU && a.ws) {            // workgroup-uniform
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ps[k] += __shfl_xor(ps[k], 16, 64);
        ps[k] += __shfl_xor(ps[k], 32, 64);
        if (lane < 16) red[wave][4 * cg + k] = ps[k];
      }
      __syncthreads();
      if (tid < 16 && live) {
        float4 s;
        s.x = ((red[0][4 * cg] + red[1][4 * cg]) + red[2][4 * cg]) + red[3][4 * cg];
        s.y = ((red[0][4 * cg + 1] + red[1][4 * cg + 1]) + red[2][4 * cg + 1]) + red[3][4 * cg + 1];
        s.z = ((red[0][4 * cg + 2] + red[1][4 * cg + 2]) + red[2][4 * cg + 2]) + red[3][4 * cg + 2];
        s.w = ((red[0][4 * cg + 3] + red[1][4 * cg + 3]) + red[2][4 * cg + 3]) + red[3][4 * cg + 3];
        *reinterpret_cast<float4*>(a.ws + ((size_t)b * a.px * a.py + patch) * C + c) = s;
      }
    }
  }
}

__global__ __launch_bounds__(256) void aim_cmap_kernel(const AimArgs a) {
  __shared__ float mean[256], hid[32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, C = a.C, hc = a.hc;
  if (tid < C) {
    const float* p = a.part + (size_t)b * a.np * C + tid;
    float s = 0.f;
    for (int i = 0; i < a.np; ++i) s += p[(size_t)i * C];
    mean[tid] = s / (float)a.N;
  }
  __syncthreads();
  for (int j = wave; j < hc; j += 4) {
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = __builtin_fmaf(bf2f(a.p[P_C_W1][j * C + c]), mean[c], s);
    s = wave_sum(s);
    if (lane == 0)
      hid[j] = bn_gelu(s + bf2f(a.p[P_C_B1][j]), bf2f(a.p[P_CBN_W][j]), bf2f(a.p[P_CBN_B][j]), bf2f(a.p[P_CBN_M][j]),
                       bf2f(a.p[P_CBN_V][j]), a.eps_c);
  }
  __syncthreads();
  if (tid < C) {
    float s = 0.f;
    for (int j = 0; j < hc; ++j) s = __builtin_fmaf(bf2f(a.p[P_C_W2][tid * hc + j]), hid[j], s);
    a.cgate[(size_t)b * C + tid] = sigmoid_f(s + bf2f(a.p[P_C_B2][tid]));
  }
}

template <int KP>
__global__ __launch_bounds__(256) void aim_mix_kernel(const AimArgs a) {
  constexpr int TM = AIM_TM, LD = KP + 8, UPR = KP / 4, NU = TM * UPR / 256;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u16* S = reinterpret_cast<u16*>(smem);                 // [TM][LD] source rows
  u16* Ws = S + TM * LD;                                 // [16][LD] W1
  float* tg = reinterpret_cast<float*>(Ws + 16 * LD);    // [TM] token gates
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int b = blockIdx.y, C = a.C, hs = a.hs;
  const int row0 = blockIdx.x * TM, rows = min(TM, a.N - row0);
  const size_t base = ((size_t)b * a.N + row0) * C;
  const bool chan = a.kind == AIM_CHANNEL;

  uint2 ra[NU], rc[NU];
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    const int u = tid + i * 256, rr = u / UPR, cu = u - rr * UPR;
    ra[i] = rc[i] = uint2{0u, 0u};
    if (rr < rows && 4 * cu < C) {
      ra[i] = *reinterpret_cast<const uint2*>(a.att + base + (size_t)rr * C + 4 * cu);
      rc[i] = *reinterpret_cast<const uint2*>(a.conv + base + (size_t)rr * C + 4 * cu);
    }
  }
  for (int u = tid; u < 16 * UPR; u += 256) {
    const int j = u / UPR, cu = u - j * UPR;
    uint2 v = uint2{0u, 0u};
    if (j < hs && 4 * cu < C) v = *reinterpret_cast<const uint2*>(a.p[P_S_W1] + j * C + 4 * cu);
    *reinterpret_cast<uint2*>(Ws + j * LD + 4 * cu) = v;
  }
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    const int u = tid + i * 256, rr = u / UPR, cu = u - rr * UPR;
    *reinterpret_cast<uint2*>(S + rr * LD + 4 * cu) = chan ? rc[i] : ra[i];
  }
  // the lane's four hidden units: BatchNorm scale and shift, b1, w2 (zeros past hs)
  float sc[4], mb[4], be[4], w2[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = 4 * fq + q;
    sc[q] = mb[q] = be[q] = w2[q] = 0.f;
    if (j < hs) {
      sc[q] = bf2f(a.p[P_SBN_W][j]) * rsqrtf(bf2f(a.p[P_SBN_V][j]) + a.eps_s);
      mb[q] = bf2f(a.p[P_SBN_M][j]);
      be[q] = bf2f(a.p[P_SBN_B][j]);
      w2[q] = bf2f(a.p[P_S_W2][j]);
    }
  }
  const float b1[4] = {4 * fq < hs ? bf2f(a.p[P_S_B1][4 * fq]) : 0.f, 4 * fq + 1 < hs ? bf2f(a.p[P_S_B1][4 * fq + 1]) : 0.f,
                       4 * fq + 2 < hs ? bf2f(a.p[P_S_B1][4 * fq + 2]) : 0.f,
                       4 * fq + 3 < hs ? bf2f(a.p[P_S_B1][4 * fq + 3]) : 0.f};
  const float b2 = bf2f(a.p[P_S_B2][0]);
  __syncthreads();

  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < KP / 32; ++kb) {
    const bf16x8 wf = *reinterpret_cast<const bf16x8*>(Ws + fr * LD + 32 * kb + 8 * fq);
    const bf16x8 xf = *reinterpret_cast<const bf16x8*>(S + (16 * wave + fr) * LD + 32 * kb + 8 * fq);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc, 0, 0, 0);
  }
  // acc[q] = hidden unit 4 fq + q of token 16 wave + fr
  float t = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    t = __builtin_fmaf(gelu_sig(__builtin_fmaf(sc[q], (acc[q] + b1[q]) - mb[q], be[q])), w2[q], t);
  t += __shfl_xor(t, 16, 64);
  t += __shfl_xor(t, 32, 64);
  if (fq == 0) tg[16 * wave + fr] = sigmoid_f(t + b2);
  __syncthreads();

  const float* cgp = a.cgate + (size_t)b * C;
#pragma unroll
  for (int i = 0; i < NU; ++i) {
    const int u = tid + i * 256, rr = u / UPR, cu = u - rr * UPR;
    if (rr >= rows || 4 * cu >= C) continue;
    const float4 cgv = *reinterpret_cast<const float4*>(cgp + 4 * cu);
    const float tv = tg[rr];
    const float4 ga = chan ? float4{tv, tv, tv, tv} : cgv, gb = chan ? cgv : float4{tv, tv, tv, tv};
    const float4 x = unpack4_bf16(ra[i]), v = unpack4_bf16(rc[i]);
    *reinterpret_cast<uint2*>(a.y + base + (size_t)rr * C + 4 * cu) =
        pack4_bf16(__builtin_fmaf(x.x, ga.x, v.x * gb.x), __builtin_fmaf(x.y, ga.y, v.y * gb.y),
                   __builtin_fmaf(x.z, ga.z, v.z * gb.z), __builtin_fmaf(x.w, ga.w, v.w * gb.w));
  }
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// Shape rules shared by the conv and the AIM: positive sizes, C % 4 == 0, patches and images within a grid axis, and
// every element index of the widest operand (pitch elements a token) below 2^31.
bool tok_shape_ok(int B, int H, int W, int C, long long pitch) {
  if (B < 1 || H < 1 || W < 1 || C < 4 || (C & 3) || B > 65535 || pitch < C || (pitch & 3)) return false;
  const long long N = (long long)H * W;
  return N <= 0x7fffffffLL && (long long)B * N <= 0x7fffffffLL / pitch;
}

inline int patches(int n) { return (n + TD_P - 1) / TD_P; }

int tok_conv_launch(const TokConvArgs& a, int epi, hipStream_t stream) {
  const dim3 grid(a.px * a.py, a.B);
  if (epi == EPI_NONE) tok_dwconv3_kernel<EPI_NONE><<<grid, TD_NT, 0, stream>>>(a);
  else if (epi == EPI_BN_GELU) tok_dwconv3_kernel<EPI_BN_GELU><<<grid, TD_NT, 0, stream>>>(a);
  else tok_dwconv3_kernel<EPI_MUL><<<grid, TD_NT, 0, stream>>>(a);
  return (int)hipGetLastError();
}

template <int KP>
int aim_mix_launch(const AimArgs& a, hipStream_t stream) {
  constexpr int lds = (AIM_TM + 16) * (KP + 8) * 2 + AIM_TM * 4;
  max_dynamic_lds_once<aim_mix_kernel<KP>>(lds);
  aim_mix_kernel<KP><<<dim3((a.N + AIM_TM - 1) / AIM_TM, a.B), 256, lds, stream>>>(a);
  return (int)hipGetLastError();
}

struct AimPlan {
  long long part_bytes, gate_bytes, ws_bytes;
};

bool aim_plan(int B, int H, int W, int C, AimPlan& p) {
  if (!tok_shape_ok(B, H, W, C, 3LL * C) || C < 16 || C > 256) return false;
  const auto up16 = [](long long v) { return (v + 15) / 16 * 16; };
  p.part_bytes = up16((long long)B * patches(H) * patches(W) * C * 4);
  p.gate_bytes = up16((long long)B * C * 4);
  p.ws_bytes = p.part_bytes + p.gate_bytes + up16((long long)B * H * W * C * 2);
  return true;
}

}  // namespace

// Depthwise 3 x 3 conv on token-major rows. x bf16 (base, xpitch elements a token, images xpitch H W apart), w bf16
// [C, 9], bias bf16 [C] or null, y bf16 [B, H W, C] contiguous. epi 0: plain; 1: BatchNorm + GELU from the four bf16
// vectors bn_w, bn_b, bn_mean, bn_var and eps, and with ws (fp32 [B, patches, C], ws_bytes at least that, 16-byte
// aligned) the per-patch sums of its fp32 output or of pool_src bf16 [B, H W, C]; 2: y = m (conv + b), m bf16 (base,
// mpitch). Domain: C % 4 == 0, B, H, W >= 1, pitches % 4 == 0 and >= C, x, m, y, pool_src 8-byte aligned, every
// element index below 2^31; anything else is hipErrorInvalidValue and nothing is launched.
CGS_EXPORT int cgs_token_dwconv3(const void* x, long long xpitch, const void* w, const void* bias, const void* bn_w,
                                 const void* bn_b, const void* bn_mean, const void* bn_var, float eps, const void* m,
                                 long long mpitch, void* y, void* ws, long long ws_bytes, const void* pool_src, int B,
                                 int H, int W, int C, int epi, hipStream_t stream) {
  if (!x || !w || !y || epi < EPI_NONE || epi > EPI_MUL || !tok_shape_ok(B, H, W, C, xpitch))
    return (int)hipErrorInvalidValue;
  if (!aligned8(x) || !aligned8(y)) return (int)hipErrorInvalidValue;
  if (epi == EPI_BN_GELU && (!bn_w || !bn_b || !bn_mean || !bn_var)) return (int)hipErrorInvalidValue;
  if (epi == EPI_MUL && (!m || !aligned8(m) || !tok_shape_ok(B, H, W, C, mpitch))) return (int)hipErrorInvalidValue;
  if (epi != EPI_BN_GELU && (ws || pool_src)) return (int)hipErrorInvalidValue;
  if (pool_src && (!ws || !aligned8(pool_src))) return (int)hipErrorInvalidValue;
  const int px = patches(W), py = patches(H);
  if (ws && ((reinterpret_cast<uintptr_t>(ws) & 15) || ws_bytes < (long long)B * px * py * C * 4))
    return (int)hipErrorInvalidValue;
  const TokConvArgs a{(const u16*)x, (const u16*)w, (const u16*)bias, (const u16*)bn_w, (const u16*)bn_b,
                      (const u16*)bn_mean, (const u16*)bn_var, (const u16*)m, (const u16*)pool_src, (u16*)y,
                      (float*)ws, xpitch, mpitch, eps, B, H, W, C, px, py};
  return tok_conv_launch(a, epi, stream);
}

// Bytes of workspace cgs_aim_fwd needs for this shape (0 outside the domain): pool partials, channel gates, conv rows.
CGS_EXPORT long long cgs_aim_ws_bytes(int B, int H, int W, int C) {
  AimPlan p;
  return aim_plan(B, H, W, C, p) ? p.ws_bytes : 0;
}

// The adaptive interaction module of DAT after the attention: conv = gelu(bn(dwconv3(v))) from the v third of qkv bf16
// [B, H W, 3C], the channel gate from the pooled conv (kind 0, spatial block) or att (kind 1, channel block), the token
// gate from att (kind 0) or conv (kind 1), y = att ga + conv gb; three launches. params: 22 bf16 device pointers in
// the order of the P_ table above (dw weight [C, 9], bias, BatchNorm gamma / beta / mean / var; channel gate W1
// [hc, C], b1, BatchNorm x 4 [hc], W2 [C, hc], b2 [C]; spatial gate W1 [hs, C], b1, BatchNorm x 4 [hs], w2 [hs], b2
// [1]); eps of the three BatchNorms. Domain: C % 4 == 0 in [16, 256], 1 <= hc <= 32, 1 <= hs <= 16, B, H, W >= 1,
// qkv, att, y and the spatial W1 8-byte aligned, ws 16-byte aligned with at least cgs_aim_ws_bytes bytes, 3 B H W C
// below 2^31; anything else is hipErrorInvalidValue and nothing is launched.
CGS_EXPORT int cgs_aim_fwd(const void* qkv, const void* att, void* y, const void* const* params, float eps_dw,
                           float eps_c, float eps_s, void* ws, long long ws_bytes, int B, int H, int W, int C, int hc,
                           int hs, int kind, hipStream_t stream) {
  AimPlan p;
  if (!qkv || !att || !y || !params || !ws || !aim_plan(B, H, W, C, p)) return (int)hipErrorInvalidValue;
  if (hc < 1 || hc > 32 || hs < 1 || hs > 16 || (kind != AIM_SPATIAL && kind != AIM_CHANNEL))
    return (int)hipErrorInvalidValue;
  if (ws_bytes < p.ws_bytes || (reinterpret_cast<uintptr_t>(ws) & 15)) return (int)hipErrorInvalidValue;
  if (!aligned8(qkv) || !aligned8(att) || !aligned8(y) || !aligned8(params[P_S_W1])) return (int)hipErrorInvalidValue;
  for (int i = 0; i < AIM_NP; ++i)
    if (!params[i]) return (int)hipErrorInvalidValue;
  float* part = (float*)ws;
  float* cgate = reinterpret_cast<float*>((char*)ws + p.part_bytes);
  u16* conv = reinterpret_cast<u16*>((char*)ws + p.part_bytes + p.gate_bytes);
  const int N = H * W, px = patches(W), py = patches(H);
  const TokConvArgs ca{(const u16*)qkv + 2 * C, (const u16*)params[P_DW_W], (const u16*)params[P_DW_B],
                       (const u16*)params[P_DBN_W], (const u16*)params[P_DBN_B], (const u16*)params[P_DBN_M],
                       (const u16*)params[P_DBN_V], nullptr, kind == AIM_CHANNEL ? (const u16*)att : nullptr, conv, part,
                       3LL * C, 0, eps_dw, B, H, W, C, px, py};
  int err = tok_conv_launch(ca, EPI_BN_GELU, stream);
  if (err) return err;
  AimArgs a;
  for (int i = 0; i < AIM_NP; ++i) a.p[i] = (const u16*)params[i];
  a.att = (const u16*)att;
  a.conv = conv;
  a.y = (u16*)y;
  a.part = part;
  a.cgate = cgate;
  a.eps_c = eps_c;
  a.eps_s = eps_s;
  a.B = B, a.N = N, a.C = C, a.hc = hc, a.hs = hs, a.np = px * py, a.kind = kind;
  aim_cmap_kernel<<<B, 256, 0, stream>>>(a);
  if ((err = (int)hipGetLastError())) return err;
  return C <= 64 ? aim_mix_launch<64>(a, stream) : C <= 128 ? aim_mix_launch<128>(a, stream)
       : C <= 192 ? aim_mix_launch<192>(a, stream) : aim_mix_launch<256>(a, stream);
}
