// Channel (transposed) attention forward of DAT's channel blocks on gfx950.
//
//   G[i, j] = sum_n q[n, i] k[n, j]        nq[i] = sqrt(sum_n q[n, i]^2), nk[j] likewise        (per image and head)
//   s[i, j] = G[i, j] / (max(nq[i], 1e-12) max(nk[j], 1e-12))                                    (F.normalize's eps)
//   P[i, :] = softmax_j(temperature[h] s[i, j])  in fp32, rounded to bf16
//   o[n, i] = sum_j P[i, j] v[n, j]
//
// The attention matrix is D x D per head and the reduction axis of its scores is the TOKEN axis. The kernels read the
// packed qkv [B, N, 3C] (channel order [3][heads][D]) where it lies and write o [B, N, C] in token order: no fp32 copy,
// no [B, h, d, N] permute, no normalised q or k and no permute back exist in memory. Three launches on one stream, no
// host synchronisation and no float atomics: every sum has a fixed order, so two calls give the same bits. The head
// width is padded to DP = 16 (D <= 16) or 32; every pad is an exact zero.
//
// 1. chan_gram_kernel<DP>: grid (chunks, head groups, B), 256 threads. The token axis is cut into chunks of L tokens
//    (chan_plan: about two workgroups a CU at batch 1, L a multiple of the 128-token stage and at least 512); a
//    workgroup owns one chunk and one group of at most HG = 4 heads (64 accumulator registers at DP = 32; the groups
//    are evened out, 6 heads = 3 + 3). Per stage of 128 tokens it loads the group's q and k segments of the token
//    rows in 4-byte units, lane-consecutive dwords of a row, each lane the same dword of FOUR consecutive tokens;
//    two byte permutes a channel turn the four dwords into the 8-byte words (channel c, tokens t..t+3) and (channel
//    c + 1, tokens t..t+3), which go to the transposed LDS image Xt[q | k][head][DP channels][128 + 8 tokens] as
//    8-byte writes. Tokens past the chunk's end take no load and are written as zeros; the channel rows D..DP and the
//    heads past the group's end are zeroed once. A stage's loads are issued into registers right after the previous
//    stage's image is complete, so they are in flight while the MFMAs of that stage run; the image itself is single.
//    Wave w owns tokens [32 w, 32 w + 32) of every stage, for all heads of the group: per head it reads NB = DP / 16
//    q^T fragments (A: channel fr, tokens 8 fq..8 fq + 7) and NB k^T fragments (B, the same shape) as 16-byte LDS
//    reads and runs NB x NB MFMAs 16x16x32 bf16 with tokens as the K axis. The squared norms are summed in fp32 from
//    the same fragments (8 fma a fragment; a bf16 square is exact in fp32): a lane keeps the partial of its channel
//    over its tokens. At the chunk's end the fq lanes are combined by two shuffles, the four waves through LDS in wave
//    order, and the workgroup writes fp32 partials [DP * DP + 2 DP] a head to the workspace.
// 2. chan_softmax_kernel<DP>: grid (heads, B). Adds the chunk partials in chunk order, forms r = 1 / max(sqrt(n2),
//    1e-12) for the 2 DP norms, then one thread a row: x = fl(fl(fl(G rq) rk) t), p = exp2(fl(fl(x - max) L)),
//    P = bf16(p (1 / sum)). Rows and columns at or beyond D are written as zeros. P is bf16 [B, heads, DP, DP].
// 3. chan_apply_kernel<DP>: grid (128-token tiles, B), 4 waves, a wave 2 blocks of 16 tokens, all heads. P is the A
//    operand (row i = 16 ib + fr, 8 consecutive j a lane, 16 bytes straight from the workspace, once a head), v^T the B
//    operand: a lane's 8 values are channels 8 fq..8 fq + 7 of token fr's v segment, four guarded dwords from the
//    packed row -- a dword at j >= D or of a token >= N is not loaded and is zero, so neither the next head's
//    values nor memory past the tensor enter. acc[r] = o[token fr][16 ib + 4 fq + r]: 4 consecutive channels, one
//    8-byte store where the address allows it, 4-byte stores otherwise (D = 30: every other head).
//
// LDS: gram 69632 B at DP = 32 (two workgroups a CU), 34816 B at DP = 16; the cross-wave reduction reuses it.
#include <algorithm>

#include "common.h"

namespace {

constexpr int CA_HG = 4;            // heads a gram workgroup, at most
constexpr int CA_TS = 128;          // tokens a stage
constexpr int CA_LDT = CA_TS + 8;   // token pitch of Xt (elements): 272 bytes, 16 fragment rows hit 16 x 4 distinct banks
constexpr int CA_NT = 256;
constexpr int CA_MIN_CHUNK = 512;   // tokens: at least four stages a workgroup where N allows it
constexpr int CA_TILE = 128;        // tokens an apply workgroup
constexpr int CA_NQ = CA_TS / 4;    // token quads a stage

struct ChanArgs {
  const u16* qkv;
  u16* o;
  const float* temp;
  float* part;      // [B, heads, nchunks, DP * DP + 2 DP]
  u16* P;           // [B, heads, DP, DP]
  int B, N, heads, D;
  int G, ngroups, L, nchunks;
};

template <int DP>
struct ChanCfg {
  static constexpr int NB = DP / 16;
  static constexpr int PS = DP * DP + 2 * DP;                      // floats of a head's partial
  static constexpr int ROWS = CA_HG * DP;                          // channel rows of q (and of k) in Xt
  static constexpr int NU = 2 * CA_NQ * (ROWS / 2) / CA_NT;        // loader units a thread, at most
  static constexpr int XT_BYTES = 2 * ROWS * CA_LDT * 2;
  static constexpr int RED_BYTES = 4 * CA_HG * PS * 4;
  static constexpr int LDS = XT_BYTES > RED_BYTES ? XT_BYTES : RED_BYTES;
  static_assert(NU * CA_NT == 2 * CA_NQ * (ROWS / 2) && XT_BYTES % 16 == 0, "loader geometry");
};

__device__ __forceinline__ float sumsq8(bf16x8 f, float s) {
  const uint4 w = __builtin_bit_cast(uint4, f);
  const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float lo = __uint_as_float(d[i] << 16), hi = __uint_as_float(d[i] & 0xffff0000u);
    s = __builtin_fmaf(lo, lo, s);
    s = __builtin_fmaf(hi, hi, s);
  }
  return s;
}

template <int DP>
__global__ __launch_bounds__(CA_NT, 2) void chan_gram_kernel(const ChanArgs a) {
  using Cf = ChanCfg<DP>;
  constexpr int NB = Cf::NB, PS = Cf::PS, ROWS = Cf::ROWS, NU = Cf::NU, LDT = CA_LDT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u16* Xt = reinterpret_cast<u16*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int chunk = blockIdx.x, grp = blockIdx.y, b = blockIdx.z;
  const int D = a.D, C = a.heads * D;
  const int h0 = grp * a.G;
  const int GH = min(a.G, a.heads - h0);         // heads of this group (the last one may be short)
  const int segdw = GH * D / 2;                  // dwords of the group's q (or k) segment of a token row
  const int tok0 = chunk * a.L, tokend = min(a.N, tok0 + a.L);
  const int nst = (tokend - tok0 + CA_TS - 1) / CA_TS;
  const u16* base = a.qkv + ((size_t)b * a.N + tok0) * 3 * C + h0 * D;

  // ---- loader units: (q | k, token quad, dword of the segment), dword fastest. goff: elements from the stage's
  // first row; meta: LDS element offset of (channel, first token of the quad) | 4 tq << 16; -1: no unit
  int goff[NU], meta[NU];
  {
    int e = tid % segdw, rq = tid / segdw;
    const int de = CA_NT % segdw, dq = CA_NT / segdw;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      goff[i] = 0;
      meta[i] = -1;
      if (rq < 2 * CA_NQ) {
        const int w = rq / CA_NQ, tq4 = 4 * (rq - w * CA_NQ);
        const int hl = 2 * e / D, d = 2 * e - hl * D;
        goff[i] = tq4 * 3 * C + w * C + 2 * e;
        meta[i] = ((w * ROWS + hl * DP + d) * LDT + tq4) | (tq4 << 16);
      }
      e += de;
      rq += dq;
      if (e >= segdw) { e -= segdw; ++rq; }
    }
  }

  uint32_t r[NU][4];
  auto load = [&](int s) {
    const u16* sb = base + (size_t)s * CA_TS * 3 * C;
    const int rem = tokend - tok0 - s * CA_TS;   // live tokens of the stage (>= 1)
    unsigned rs = 3 * C;                         // row pitch, opaque to the optimiser: the 4 NU offsets below are
    asm volatile("" : "+s"(rs));                 // one add each per stage, not 4 NU registers live across the loop
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      int m = meta[i];
      asm volatile("" : "+v"(m));                // likewise: the predicates are formed per stage
      const int lim = m < 0 ? 0 : rem - (m >> 16);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[i][j] = 0u;
        if (j < lim) r[i][j] = *reinterpret_cast<const uint32_t*>(sb + ((unsigned)goff[i] + j * rs));
      }
    }
  };
  auto put = [&]() {
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      int m = meta[i];
      asm volatile("" : "+v"(m));
      if (m >= 0) {
        u16* dst = Xt + (m & 0xffff);
        *reinterpret_cast<uint2*>(dst) = uint2{__builtin_amdgcn_perm(r[i][1], r[i][0], 0x05040100u),
                                               __builtin_amdgcn_perm(r[i][3], r[i][2], 0x05040100u)};
        *reinterpret_cast<uint2*>(dst + LDT) = uint2{__builtin_amdgcn_perm(r[i][1], r[i][0], 0x07060302u),
                                                     __builtin_amdgcn_perm(r[i][3], r[i][2], 0x07060302u)};
      }
    }
  };
  load(0);

  // ---- once: the whole image zeroed (channel rows D..DP, heads past GH, row pads)
  for (int idx = tid; idx < Cf::XT_BYTES / 16; idx += CA_NT) reinterpret_cast<uint4*>(smem)[idx] = uint4{0u, 0u, 0u, 0u};

  f32x4 acc[CA_HG][NB][NB];
  float nq[CA_HG][NB], nk[CA_HG][NB];
#pragma unroll
  for (int hl = 0; hl < CA_HG; ++hl)
#pragma unroll
    for (int ib = 0; ib < NB; ++ib) {
      nq[hl][ib] = nk[hl][ib] = 0.f;
#pragma unroll
      for (int jb = 0; jb < NB; ++jb) acc[hl][ib][jb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

#pragma unroll 1
  for (int s = 0; s < nst; ++s) {
    __syncthreads();        // the zeroing (stage 0); every wave done with the previous stage
    put();
    __syncthreads();
    if (s + 1 < nst) load(s + 1);     // in flight during the MFMAs below
    const u16* xw = Xt + 32 * wave + 8 * fq;
#pragma unroll
    for (int hl = 0; hl < CA_HG; ++hl) {
      if (hl >= GH) continue;         // workgroup-uniform
      bf16x8 af[NB], kf[NB];
#pragma unroll
      for (int ib = 0; ib < NB; ++ib) {
        af[ib] = *reinterpret_cast<const bf16x8*>(xw + (hl * DP + 16 * ib + fr) * LDT);
        kf[ib] = *reinterpret_cast<const bf16x8*>(xw + (ROWS + hl * DP + 16 * ib + fr) * LDT);
        nq[hl][ib] = sumsq8(af[ib], nq[hl][ib]);
        nk[hl][ib] = sumsq8(kf[ib], nk[hl][ib]);
      }
#pragma unroll
      for (int ib = 0; ib < NB; ++ib)
#pragma unroll
        for (int jb = 0; jb < NB; ++jb)
          acc[hl][ib][jb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ib], kf[jb], acc[hl][ib][jb], 0, 0, 0);
    }
  }
  __syncthreads();          // the image is free: the waves' partials are staged over it

  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int hl = 0; hl < CA_HG; ++hl) {
    if (hl >= GH) continue;
    float* rw = red + (wave * CA_HG + hl) * PS;
#pragma unroll
    for (int ib = 0; ib < NB; ++ib) {
#pragma unroll
      for (int jb = 0; jb < NB; ++jb)
#pragma unroll
        for (int q = 0; q < 4; ++q) rw[(16 * ib + 4 * fq + q) * DP + 16 * jb + fr] = acc[hl][ib][jb][q];
      float x = nq[hl][ib], y = nk[hl][ib];
      x += __shfl_xor(x, 16, 64);
      y += __shfl_xor(y, 16, 64);
      x += __shfl_xor(x, 32, 64);
      y += __shfl_xor(y, 32, 64);
      if (fq == 0) {
        rw[DP * DP + 16 * ib + fr] = x;
        rw[DP * DP + DP + 16 * ib + fr] = y;
      }
    }
  }
  __syncthreads();
  for (int idx = tid; idx < GH * PS; idx += CA_NT) {
    const int hl = idx / PS, e = idx - hl * PS;
    const float* p = red + hl * PS + e;
    const float v = ((p[0] + p[CA_HG * PS]) + p[2 * CA_HG * PS]) + p[3 * CA_HG * PS];
    a.part[(((size_t)b * a.heads + h0 + hl) * a.nchunks + chunk) * PS + e] = v;
  }
}

template <int DP>
__global__ __launch_bounds__(CA_NT) void chan_softmax_kernel(const ChanArgs a) {
  constexpr int PS = ChanCfg<DP>::PS;
  constexpr float LOG2E = 1.4426950408889634f;
  __shared__ float S[PS];
  const int tid = threadIdx.x, h = blockIdx.x, b = blockIdx.y, D = a.D;
  const float* part = a.part + ((size_t)b * a.heads + h) * a.nchunks * PS;
  for (int e = tid; e < PS; e += CA_NT) {
    float s = 0.f;
    for (int c = 0; c < a.nchunks; ++c) s += part[(size_t)c * PS + e];
    S[e] = s;
  }
  __syncthreads();
  if (tid < 2 * DP) S[DP * DP + tid] = 1.0f / fmaxf(sqrtf(S[DP * DP + tid]), 1e-12f);
  __syncthreads();
  if (tid >= DP) return;
  const int i = tid;
  u16* out = a.P + (((size_t)b * a.heads + h) * DP + i) * DP;
  float x[DP];
  float mx = -INFINITY;
  const float t = a.temp[h], rq = S[DP * DP + i];
#pragma unroll
  for (int j = 0; j < DP; ++j) {
    x[j] = (S[i * DP + j] * rq) * S[DP * DP + DP + j] * t;
    if (j < D) mx = fmaxf(mx, x[j]);
  }
  float l = 0.f;
#pragma unroll
  for (int j = 0; j < DP; ++j) {
    x[j] = j < D ? __builtin_amdgcn_exp2f((x[j] - mx) * LOG2E) : 0.f;
    l += x[j];
  }
  const float inv = i < D ? 1.0f / l : 0.f;      // a row at or beyond D is written as zeros
#pragma unroll
  for (int j = 0; j < DP; j += 4)
    *reinterpret_cast<uint2*>(out + j) = pack4_bf16(x[j] * inv, x[j + 1] * inv, x[j + 2] * inv, x[j + 3] * inv);
}

template <int DP>
__global__ __launch_bounds__(CA_NT) void chan_apply_kernel(const ChanArgs a) {
  constexpr int NB = DP / 16, TB = CA_TILE / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int b = blockIdx.y, D = a.D, C = a.heads * D;
  const int tile0 = blockIdx.x * CA_TILE;
  for (int h = 0; h < a.heads; ++h) {
    const u16* Ph = a.P + ((size_t)b * a.heads + h) * DP * DP;
    bf16x8 pf[NB];
#pragma unroll
    for (int ib = 0; ib < NB; ++ib) {
      uint4 w = uint4{0u, 0u, 0u, 0u};
      if (8 * fq < DP) w = *reinterpret_cast<const uint4*>(Ph + (16 * ib + fr) * DP + 8 * fq);
      pf[ib] = __builtin_bit_cast(bf16x8, w);
    }
#pragma unroll
    for (int tb = 0; tb < TB; ++tb) {
      const int n = tile0 + (tb * 4 + wave) * 16 + fr;
      const bool live = n < a.N;
      const size_t row = (size_t)b * a.N + (live ? n : 0);
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      const u16* src = a.qkv + row * 3 * C + 2 * C + h * D + 8 * fq;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (live && 8 * fq + 2 * i < D) w[i] = *reinterpret_cast<const uint32_t*>(src + 2 * i);
      const uint4 w4 = {w[0], w[1], w[2], w[3]};
      const bf16x8 vf = __builtin_bit_cast(bf16x8, w4);
#pragma unroll
      for (int ib = 0; ib < NB; ++ib) {
        const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[ib], vf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        const int c0 = 16 * ib + 4 * fq;
        if (!live || c0 >= D) continue;
        u16* dst = a.o + row * C + h * D + c0;
        const uint2 v = pack4_bf16(acc[0], acc[1], acc[2], acc[3]);
        if (c0 + 4 <= D && (reinterpret_cast<uintptr_t>(dst) & 7) == 0) {
          *reinterpret_cast<uint2*>(dst) = v;
        } else {
          *reinterpret_cast<uint32_t*>(dst) = v.x;
          if (c0 + 2 < D) *reinterpret_cast<uint32_t*>(dst + 2) = v.y;
        }
      }
    }
  }
}

struct ChanPlan {
  int DP, G, ngroups, L, nchunks;
  long long part_bytes, ws_bytes;
};

// The split of one call, a fixed function of the shape and the CU count. False outside the domain.
bool chan_plan(int B, int N, int heads, int D, ChanPlan& p) {
  if (B < 1 || N < 1 || heads < 1 || D < 2 || D > 32 || (D & 1)) return false;
  p.DP = D <= 16 ? 16 : 32;
  p.ngroups = (heads + CA_HG - 1) / CA_HG;
  p.G = (heads + p.ngroups - 1) / p.ngroups;
  if (B > 65535 || p.ngroups > 65535 || 6LL * heads * D * CA_TS > 0x7fffffffLL) return false;
  const long long maxchunks = std::max(1LL, 2LL * num_cus() / ((long long)B * p.ngroups));
  long long L = ((N + maxchunks - 1) / maxchunks + CA_TS - 1) / CA_TS * CA_TS;
  if (L < CA_MIN_CHUNK) L = CA_MIN_CHUNK;
  p.L = (int)std::min(L, 0x7fffff80LL);
  p.nchunks = (int)((N + (long long)p.L - 1) / p.L);
  const long long ps = p.DP * p.DP + 2 * p.DP;
  p.part_bytes = (long long)B * heads * p.nchunks * ps * 4;
  p.ws_bytes = p.part_bytes + (long long)B * heads * p.DP * p.DP * 2;
  return true;
}

template <int DP>
int chan_launch(const ChanArgs& a, hipStream_t stream) {
  using Cf = ChanCfg<DP>;
  max_dynamic_lds_once<chan_gram_kernel<DP>>(Cf::LDS);
  chan_gram_kernel<DP><<<dim3(a.nchunks, a.ngroups, a.B), CA_NT, Cf::LDS, stream>>>(a);
  int err = (int)hipGetLastError();
  if (err) return err;
  chan_softmax_kernel<DP><<<dim3(a.heads, a.B), CA_NT, 0, stream>>>(a);
  if ((err = (int)hipGetLastError())) return err;
  chan_apply_kernel<DP><<<dim3((a.N + CA_TILE - 1) / CA_TILE, a.B), CA_NT, 0, stream>>>(a);
  return (int)hipGetLastError();
}

}  // namespace

// Bytes of workspace cgs_channel_attn_fwd needs for this shape (0 outside the domain), and the gram kernel's chunk
// length in tokens (0 outside the domain): the fp32 summation depth of a score, for the tests' bound.
CGS_EXPORT long long cgs_channel_attn_ws_bytes(int B, int N, int heads, int D) {
  ChanPlan p;
  return chan_plan(B, N, heads, D, p) ? p.ws_bytes : 0;
}

CGS_EXPORT int cgs_channel_attn_chunk(int B, int N, int heads, int D) {
  ChanPlan p;
  return chan_plan(B, N, heads, D, p) ? p.L : 0;
}

// qkv bf16 [B, N, 3 heads D] contiguous, o bf16 [B, N, heads D], temperature fp32 [heads], ws at least
// cgs_channel_attn_ws_bytes(B, N, heads, D) bytes. Domain: D even in [2, 32], heads, N, B >= 1 (B and heads / 4 within
// a grid axis), qkv and o 4-byte aligned, ws 16-byte aligned; anything else is hipErrorInvalidValue and nothing is
// launched.
CGS_EXPORT int cgs_channel_attn_fwd(const void* qkv, void* o, const float* temperature, void* ws, long long ws_bytes,
                                    int B, int N, int heads, int D, hipStream_t stream) {
  ChanPlan p;
  if (!qkv || !o || !temperature || !ws || !chan_plan(B, N, heads, D, p)) return (int)hipErrorInvalidValue;
  if (ws_bytes < p.ws_bytes || (reinterpret_cast<uintptr_t>(ws) & 15)) return (int)hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(o)) & 3) return (int)hipErrorInvalidValue;
  const ChanArgs a{(const u16*)qkv, (u16*)o, temperature, (float*)ws,
                   reinterpret_cast<u16*>((char*)ws + p.part_bytes), B, N, heads, D, p.G, p.ngroups, p.L, p.nchunks};
  return p.DP == 16 ? chan_launch<16>(a, stream) : chan_launch<32>(a, stream);
}
