// Shifted-window attention forward for the Swin-family upscalers (SwinIR, Swin2SR, HAT) on gfx950.
//
//   o = softmax(scale * hs[h] * s + table[r(q, k), h] + m(q, k)) v      per ws x ws window and head, fp32 scores
//
// The kernel knows the window geometry, so nothing around the attention is materialised: it reads the packed qkv
// tensor [B, H*W, 3*C] of the un-rolled, un-partitioned tokens where it lies (channel order [3][heads][D]) and
// writes o [B, H*W, C] at the un-shifted pixel of every query. With y = roll(x, (-shift, -shift)) the token at
// rolled position (i, j) is source pixel ((i + shift) % H, (j + shift) % W): the cyclic shift and the window
// partition are load / store address arithmetic. table is the [(2ws-1)^2, heads] relative-position table, indexed
// r = (yq - yk + ws-1) * (2ws-1) + (xq - xk + ws-1); m = -100 (finite) where the region labels of the two tokens
// differ (per axis: rolled index < n - ws: 0, < n - shift: 1, else 2; shift > 0 only). No [heads, N, N] bias and no
// [nW, N, N] mask exists anywhere. cosine (SwinV2): s = (q . k) rq rk with rq = 1 / max(||q||, 1e-12) taken in fp32
// from the bf16 rows and applied to the fp32 scores -- no normalised bf16 copy of q or k is rounded.
//
// Work split. One workgroup owns one window and one group of G heads: the segment [h0 D, (h0 + G) D) of every token
// row of q, k and v, so every byte of qkv comes from HBM once. G is chosen by the host (window_groups): at least
// enough heads for a 128-byte segment of a token row (never a lone 60-byte head slice, unless LDS leaves no choice),
// more while the workgroup stays under 52 KB of LDS (three workgroups a CU); the groups of a window are adjacent
// block indices, so the cache lines two groups share are still in L2. An 8 x 8 window of C = 180 runs as 2 groups
// of 3 heads (48 KB each), a 16 x 16 window head group by head group (D = 30: 2 heads, 126 KB; D = 64: 1 head, 112 KB).
//
// Data movement. The loader works in 4-byte units (D is even; head slices start at 60-byte offsets at D = 30 and
// rows are 1080 bytes at C = 180, so nothing wider is aligned): lane-consecutive dwords of a token's segment,
// written to LDS as Q[h][token][DP + 8], K likewise and V transposed, Vt[h][d][N + 8]; DP = D padded to 32 or 64,
// the pad zeroed in LDS once, never in memory. The group's table columns (225 or 961 floats a head), the source
// pixel and the region label of each window token are staged in LDS once per workgroup.
//
// Compute, per (head, 16-query block), one wave each (MFMA 16x16x32 bf16, wave64; fr = lane & 15, fq = lane >> 4):
//   S^T = K Q^T      A = K rows (16 keys), B = Q rows (16 queries): acc[j][q] = score of key 16 j + 4 fq + q for
//                    query fr. A lane holds N / 4 scores of ONE query: all 64 or 256 keys of the window sit in
//                    accumulators at once, the softmax is single pass (no online rescale); row max and row sum are
//                    lane-local plus two cross-lane steps over fq (lane ^ 16, lane ^ 32).
//   O^T = V^T P^T    the exponentiated accumulators, rounded to bf16, ARE the B operand: MFMA k index 8 fq + t is
//                    key 32 m + 4 fq + t (t < 4) or 32 m + 16 + 4 fq + t - 4, and the A operand reads Vt in the same
//                    order (two 8-byte LDS reads). acc[db][q] = O[query fr][16 db + 4 fq + q].
//   O / rowsum is rounded to bf16 into the block's own Q rows (no other wave reads them), and after a barrier the
//   workgroup copies the group's segment of every token row to o in lane-consecutive dwords: whole token rows where
//   one group holds all heads, whole group segments otherwise, never per-head scatters.
//
// Budget. 256 threads (ws 8: 4 query blocks a head) or 512 threads (ws 16: 16 blocks a head). Registers as compiled:
// ws 8 64 - 76 VGPRs + 16 AGPRs, ws 16 166 VGPRs (N / 4 = 64 of them score accumulators), no scratch (the build
// fails on any). LDS decides the occupancy: ws 8 runs 3 workgroups (12 waves) a CU at D <= 32 and 2 - 5 at D <= 64,
// ws 16 one workgroup (8 waves, 2 a SIMD, 256 VGPRs each allowed) a CU. No workspace, no host synchronisation:
// capturable.
#include "common.h"

namespace {

constexpr int WA_LDS_SOFT = 52 * 1024;    // three workgroups a CU
constexpr int WA_LDS_HARD = 160 * 1024;   // the CU's LDS

struct WinArgs {
  const u16* qkv;
  u16* o;
  const float* table;
  const float* hscale;
  float scale;
  int cosine;
  int B, H, W, heads, D, shift;
  int G, ngroups;
};

template <int WS, int DP>
struct WinCfg {
  static constexpr int N = WS * WS;             // tokens of a window
  static constexpr int NQB = N / 16;            // 16-query blocks a head
  static constexpr int NW = WS == 8 ? 4 : 8;    // waves
  static constexpr int NT = 64 * NW;
  static constexpr int LDQ = DP + 8;            // Q / K row (elements): 80 / 144 bytes, 16-byte multiples
  static constexpr int LDV = N + 8;             // Vt row (elements): 144 / 528 bytes, 8-byte multiples
  static constexpr int R = (2 * WS - 1) * (2 * WS - 1);
  // LDS of a workgroup with G heads: Q, K, Vt, rq, rk per head, then tok, the table columns, the labels
  static constexpr int PER_HEAD = 2 * N * LDQ * 2 + DP * LDV * 2 + 2 * N * 4 + R * 4;
  static constexpr int FIXED = N * 4 + N;
  static int lds(int G) { return G * PER_HEAD + FIXED; }
};

// Heads per workgroup (see the header): at least a 128-byte segment, more under WA_LDS_SOFT, never over WA_LDS_HARD;
// then evened out over the groups. 0: one head does not fit.
template <class Cf>
int window_groups(int heads, int D) {
  int G = (64 + D - 1) / D;
  if (G > heads) G = heads;
  while (G < heads && Cf::lds(G + 1) <= WA_LDS_SOFT) ++G;
  while (G > 1 && Cf::lds(G) > WA_LDS_HARD) --G;
  if (Cf::lds(G) > WA_LDS_HARD) return 0;
  const int ng = (heads + G - 1) / G;
  return (heads + ng - 1) / ng;
}

template <int WS, int DP>
__global__ __launch_bounds__(WS == 8 ? 256 : 512) void window_attn_kernel(const WinArgs a) {
  using Cf = WinCfg<WS, DP>;
  constexpr int N = Cf::N, NQB = Cf::NQB, NW = Cf::NW, NT = Cf::NT, LDQ = Cf::LDQ, LDV = Cf::LDV, R = Cf::R;
  constexpr int NKB = N / 16;     // 16-key blocks
  constexpr int KS = DP / 32;     // k-steps of the QK product
  constexpr int NDB = DP / 16;    // 16-wide d blocks of the output
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int G = a.G;
  u16* Qs = reinterpret_cast<u16*>(smem);
  u16* Ks = Qs + G * N * LDQ;
  u16* Vt = Ks + G * N * LDQ;
  float* rq = reinterpret_cast<float*>(Vt + G * DP * LDV);
  float* rk = rq + G * N;
  int* tok = reinterpret_cast<int*>(rk + G * N);
  float* tab = reinterpret_cast<float*>(tok + N);
  unsigned char* lab = reinterpret_cast<unsigned char*>(tab + G * R);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int nwx = a.W / WS, nwin = (a.H / WS) * nwx;
  int bid = blockIdx.x;
  const int grp = bid % a.ngroups;
  bid /= a.ngroups;
  const int win = bid % nwin, b = bid / nwin;
  const int wy = win / nwx, wx = win - wy * nwx;
  const int D = a.D, C = a.heads * D;
  const int h0 = grp * G;
  const int GH = min(G, a.heads - h0);      // heads of this group (the last one may be short)
  const int segdw = GH * D / 2;             // dwords of the group's segment of a token row
  const size_t img = (size_t)b * a.H * a.W;

  // ---- window geometry: source pixel and region label of every window token
  if (tid < N) {
    const int ry = wy * WS + tid / WS, rx = wx * WS + tid % WS;      // rolled coordinates
    int sy = ry + a.shift, sx = rx + a.shift;
    if (sy >= a.H) sy -= a.H;
    if (sx >= a.W) sx -= a.W;
    tok[tid] = sy * a.W + sx;
    const int ly = ry < a.H - WS ? 0 : (ry < a.H - a.shift ? 1 : 2);
    const int lx = rx < a.W - WS ? 0 : (rx < a.W - a.shift ? 1 : 2);
    lab[tid] = (unsigned char)(a.shift ? 3 * ly + lx : 0);
  }
  for (int idx = tid; idx < GH * R; idx += NT) {
    const int hl = idx / R, r = idx - hl * R;
    tab[idx] = a.table[(size_t)r * a.heads + h0 + hl];
  }
  if (D < DP) {     // the pad of the head dim: zero in LDS, once
    const int pd = DP - D;
    for (int idx = tid; idx < GH * N * pd; idx += NT) {
      const int row = idx / pd, d = D + idx - row * pd;     // row = hl * N + token
      const int hl = row / N, t = row - hl * N;
      Qs[row * LDQ + d] = 0;
      Ks[row * LDQ + d] = 0;
      Vt[(hl * DP + d) * LDV + t] = 0;
    }
  }
  __syncthreads();

  // ---- q, k, v segments of the window's tokens: HBM -> LDS in 4-byte units, V transposed
  for (int idx = tid; idx < N * segdw; idx += NT) {
    const int t = idx / segdw, e = 2 * (idx - t * segdw);
    const int hl = e / D, d = e - hl * D;
    const u16* src = a.qkv + (img + tok[t]) * 3 * C + h0 * D + e;
    const uint32_t q = *reinterpret_cast<const uint32_t*>(src);
    const uint32_t k = *reinterpret_cast<const uint32_t*>(src + C);
    const uint32_t v = *reinterpret_cast<const uint32_t*>(src + 2 * C);
    *reinterpret_cast<uint32_t*>(&Qs[(hl * N + t) * LDQ + d]) = q;
    *reinterpret_cast<uint32_t*>(&Ks[(hl * N + t) * LDQ + d]) = k;
    Vt[(hl * DP + d) * LDV + t] = (u16)(v & 0xffffu);
    Vt[(hl * DP + d + 1) * LDV + t] = (u16)(v >> 16);
  }
  __syncthreads();

  // ---- SwinV2: reciprocal norms of the bf16 rows, fp32
  if (a.cosine) {
    for (int idx = tid; idx < 2 * GH * N; idx += NT) {
      const int which = idx / (GH * N), row = idx - which * GH * N;
      const u16* p = (which ? Ks : Qs) + row * LDQ;
      float ss = 0.f;
#pragma unroll
      for (int d = 0; d < DP; d += 2) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p + d);
        const float x = __uint_as_float(w << 16), y = __uint_as_float(w & 0xffff0000u);
        ss = __builtin_fmaf(x, x, ss);
        ss = __builtin_fmaf(y, y, ss);
      }
      (which ? rk : rq)[row] = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    }
    __syncthreads();
  }

  // ---- one (head, 16-query block) per wave and turn
  for (int w = wave; w < GH * NQB; w += NW) {
    const int hl = w / NQB, qb = w - hl * NQB;
    const int tq = 16 * qb + fr;                 // this lane's query (window token)
    const int qrow = hl * N + tq;
    bf16x8 qf[KS];
#pragma unroll
    for (int kb = 0; kb < KS; ++kb) qf[kb] = *reinterpret_cast<const bf16x8*>(&Qs[qrow * LDQ + 32 * kb + 8 * fq]);
    f32x4 s[NKB];
#pragma unroll
    for (int j = 0; j < NKB; ++j) {
      s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < KS; ++kb) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&Ks[(hl * N + 16 * j + fr) * LDQ + 32 * kb + 8 * fq]);
        s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kb], s[j], 0, 0, 0);
      }
    }
    // score terms: x = s qs (rk) + (table + mask)
    float qs = a.hscale ? a.scale * a.hscale[h0 + hl] : a.scale;
    if (a.cosine) qs *= rq[qrow];
    const int iq = tq / WS, jq = tq % WS;
    const uint32_t labq = lab[tq];
    const float* tb = tab + hl * R;
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < NKB; ++j) {
      const int k0 = 16 * j + 4 * fq;            // four keys of one window row
      const int r0 = (iq - k0 / WS + WS - 1) * (2 * WS - 1) + (jq - k0 % WS + WS - 1);
      const uint32_t lk = *reinterpret_cast<const uint32_t*>(&lab[k0]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float t = s[j][q] * qs;
        if (a.cosine) t *= rk[hl * N + k0 + q];
        float add = tb[r0 - q];
        if (((lk >> (8 * q)) & 0xffu) != labq) add += -100.0f;
        const float x = t + add;
        s[j][q] = x;
        mx = fmaxf(mx, x);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < NKB; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float p = __builtin_amdgcn_exp2f((s[j][q] - mx) * 1.4426950408889634f);
        s[j][q] = p;
        l += p;
      }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    f32x4 oacc[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) oacc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < NKB / 2; ++m) {
      const bf16x8 pf = {(__bf16)s[2 * m][0],     (__bf16)s[2 * m][1],     (__bf16)s[2 * m][2],
                         (__bf16)s[2 * m][3],     (__bf16)s[2 * m + 1][0], (__bf16)s[2 * m + 1][1],
                         (__bf16)s[2 * m + 1][2], (__bf16)s[2 * m + 1][3]};
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const u16* vr = &Vt[(hl * DP + 16 * db + fr) * LDV + 32 * m + 4 * fq];
        const s16x4 lo = *reinterpret_cast<const s16x4*>(vr);
        const s16x4 hi = *reinterpret_cast<const s16x4*>(vr + 16);
        const s16x8 vv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        oacc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vv), pf, oacc[db], 0, 0, 0);
      }
    }
    const float inv = 1.0f / l;
#pragma unroll
    for (int db = 0; db < NDB; ++db)       // over the block's own Q rows: no other wave reads them
      *reinterpret_cast<uint2*>(&Qs[qrow * LDQ + 16 * db + 4 * fq]) =
          pack4_bf16(oacc[db][0] * inv, oacc[db][1] * inv, oacc[db][2] * inv, oacc[db][3] * inv);
  }
  __syncthreads();

  // ---- the group's segment of every token row, at the query's source pixel
  for (int idx = tid; idx < N * segdw; idx += NT) {
    const int t = idx / segdw, e = 2 * (idx - t * segdw);
    const int hl = e / D, d = e - hl * D;
    *reinterpret_cast<uint32_t*>(a.o + (img + tok[t]) * C + h0 * D + e) =
        *reinterpret_cast<const uint32_t*>(&Qs[(hl * N + t) * LDQ + d]);
  }
}

template <int WS, int DP>
int window_attn_launch(WinArgs a, hipStream_t stream) {
  using Cf = WinCfg<WS, DP>;
  a.G = window_groups<Cf>(a.heads, a.D);
  if (a.G <= 0) return (int)hipErrorInvalidValue;
  a.ngroups = (a.heads + a.G - 1) / a.G;
  const long long nwg = (long long)a.B * (a.H / WS) * (a.W / WS) * a.ngroups;
  if (nwg <= 0 || nwg > 0x7fffffffLL || (long long)a.H * a.W > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  max_dynamic_lds_once<window_attn_kernel<WS, DP>>(WA_LDS_HARD);
  window_attn_kernel<WS, DP><<<dim3((unsigned)nwg), Cf::NT, Cf::lds(a.G), stream>>>(a);
  return (int)hipGetLastError();
}

}  // namespace

// qkv bf16 [B, H*W, 3*C] contiguous, o bf16 [B, H*W, C], table fp32 [(2ws-1)^2, heads], hscale fp32 [heads] or null.
// Domain: ws 8 or 16, H % ws == W % ws == 0, 0 <= shift < ws, D even in [2, 64], qkv and o 4-byte aligned; anything
// else is hipErrorInvalidValue and nothing is launched.
CGS_EXPORT int cgs_window_attn_fwd(const void* qkv, void* o, const float* table, float scale, int cosine,
                                   const float* hscale, int B, int H, int W, int heads, int D, int ws, int shift,
                                   hipStream_t stream) {
  if (!qkv || !o || !table || B <= 0 || H <= 0 || W <= 0 || heads <= 0) return (int)hipErrorInvalidValue;
  if ((ws != 8 && ws != 16) || H % ws || W % ws || shift < 0 || shift >= ws) return (int)hipErrorInvalidValue;
  if (D < 2 || D > 64 || (D & 1)) return (int)hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(o)) & 3) return (int)hipErrorInvalidValue;
  const WinArgs a{(const u16*)qkv, (u16*)o, table, hscale, scale, cosine ? 1 : 0, B, H, W, heads, D, shift, 0, 0};
  if (ws == 8) return D <= 32 ? window_attn_launch<8, 32>(a, stream) : window_attn_launch<8, 64>(a, stream);
  return D <= 32 ? window_attn_launch<16, 32>(a, stream) : window_attn_launch<16, 64>(a, stream);
}
