// Overlapping cross-attention forward (HAT's OCAB) on gfx950.
//
//   o[q] = sum_k softmax_k(scale * (q . k) + table[r(q, k), h]) v[k]      per ws x ws window and head, fp32 scores
//
// Queries are the ws*ws tokens of window (wy, wx) of the un-rolled image; keys and values are the ows*ows positions
// (wy ws - pad + ky, wx ws - pad + kx), pad = (ows - ws) / 2, in row-major (ky, kx) order. A position outside the
// image has k = v = 0 and is NOT masked: its logit is table[r, h] and it counts in the denominator (what
// nn.Unfold(padding = pad) gives). r = a (ws + ows - 1) + b with a = ky - qy + (ws - ows + 1), b likewise in x; r is
// negative for many pairs and the table [(ws + ows - 1)^2, heads] is indexed from the end then (r + T^2). The range of
// r is exactly T^2 consecutive integers starting at RMIN = (2 - ows)(T + 1), so the wrap is done once, while the
// group's table columns are staged: LDS slot r - RMIN holds table[r < 0 ? r + T^2 : r]. The kernel reads the packed
// qkv [B, H*W, 3*C] (channel order [3][heads][D]) where it lies and writes o [B, H*W, C] at the query pixels:
// no slice, unfold, partition, bias tensor, head-dim pad or un-partition exists in memory.
//
// Work split. One workgroup owns one window and one group of G heads (overlap_groups on the host): enough heads for
// a 128-byte segment of a token row where that stays under 80 KB of LDS (two workgroups a CU), at most 4 (ws 8) or 2
// (ws 16), evened out over the groups; the last group may be short. Block index = ((image, window row, window
// column), group): the groups of a window, then its horizontal neighbours, are adjacent, so the 2.25x re-read of k
// and v by neighbouring windows and the cache lines two groups share come from L2.
//
// Key bands (ws 16). The 24 key rows are taken in NB = 3 bands of 8 rows (192 keys: 12 MFMA key blocks, 48 score
// registers a lane) with an online-softmax rescale between bands; all 576 keys at once would need 144 score
// registers and 81 KB of K and Vt a head. ws 8 is single pass: one band of 12 rows, 144 keys = 9 key blocks (36
// score registers); the P V step eats blocks in pairs, so the key axis of Vt is padded to 160 with zeros and the
// tenth block's P is an exact 0 that never enters the row sum (unlike the out-of-image keys, which do).
//
// Data movement. Per band the workgroup gathers the k and v segments of the band's tokens from qkv in 4-byte units
// (D is even; head slices start at 60-byte offsets at D = 30), lane-consecutive dwords of a token's segment, into
// K[h][key][DP + 8] and, transposed, Vt[h][d][keys + 8]; DP = 32, the head-dim pad and the key pad are zeroed in LDS
// once. A position outside the image takes no load and stores zeros: one predicate per dword in the loader, none in
// the MFMA loops. The Q fragments of a wave's 16 queries are needed once and go from global memory to registers
// (four guarded dwords a lane), never through LDS.
//
// Compute, per (head, 16-query block), MAXT = 4 such turns a wave, their state (Q fragment, running max, lane-partial
// row sum, 2 output accumulators) in registers across the bands (MFMA 16x16x32 bf16; fr = lane & 15, fq = lane >> 4):
//   S^T = K Q^T     A = 16 key rows, B = 16 query rows: acc[j][q] = score of band key 16 j + 4 fq + q for query fr.
//                   ows % 4 == 0: a lane's four keys lie in one key row and read four consecutive table slots.
//   x = fl(fl(s scale) + table);  m' = max(m, band max) (lane-local, then lane ^ 16, lane ^ 32);
//   al = exp2((m - m') L), l = l al, O = O al (NB > 1 only);  p = exp2((x - m') L), l += p (lane-partial: the
//   four lanes of a query hold the same al, the partials are added once after the last band)
//   O^T += V^T P^T  the bf16-rounded p ARE the B operand; the A operand reads Vt in the same key order.
//   After the last band O / l is rounded to bf16 into LDS (over the K and Vt region, behind a barrier) and the
//   workgroup copies the group's segment of every query's token row to o in lane-consecutive dwords.
//
// LDS budget, bytes a head (K + Vt + table):
//   ws 8   144 x 40 x 2 = 11520 + 32 x 168 x 2 = 10752 + 361 x 4 = 1444:   23716; G = 3 (D = 30): 71148, two fit the LDS of a CU
//   ws 16  192 x 40 x 2 = 15360 + 32 x 200 x 2 = 12800 + 1521 x 4 = 6084:  34244; G = 2 (D = 30): 68488, two fit the LDS of a CU
// Threads: 256 (ws 8) or 512 (ws 16). As compiled for gfx950 (kernel_resources.json; a compile, not a run): ws 8
// 96 VGPRs + 44 AGPRs, ws 16 160 VGPRs, no scratch (the build fails on any). Occupancy: ws 8 two workgroups (8 waves)
// a CU by LDS; ws 16 one workgroup (8 waves, 2 a SIMD) a CU by registers -- two would fit in LDS at 128 VGPRs or
// fewer. No workspace, no host synchronisation: capturable.
#include "common.h"

namespace {

constexpr int OA_LDS_SOFT = 80 * 1024;    // two workgroups a CU
constexpr int OA_LDS_HARD = 160 * 1024;   // the CU's LDS

struct OvArgs {
  const u16* qkv;
  u16* o;
  const float* table;
  float scale;
  int B, H, W, heads, D;
  int G, ngroups;
};

template <int WS>
struct OvCfg {
  static constexpr int OWS = WS * 3 / 2;           // key window side
  static constexpr int PAD = (OWS - WS) / 2;
  static constexpr int NQ = WS * WS;               // queries of a window
  static constexpr int NQB = NQ / 16;              // 16-query blocks a head
  static constexpr int NW = WS == 8 ? 4 : 8;       // waves
  static constexpr int NT = 64 * NW;
  static constexpr int BR = WS == 8 ? 12 : 8;      // key rows a band
  static constexpr int NB = OWS / BR;              // bands
  static constexpr int KB = BR * OWS;              // keys a band
  static constexpr int NKB = KB / 16;              // 16-key blocks a band
  static constexpr int NKBP = (NKB + 1) & ~1;      // ... padded to pairs for the P V step
  static constexpr int DP = 32;
  static constexpr int LDQ = DP + 8;               // K / staged-o row (elements): 80 bytes
  static constexpr int LDV = 16 * NKBP + 8;        // Vt row (elements): 336 / 400 bytes, 8-byte multiples
  static constexpr int T = WS + OWS - 1;
  static constexpr int TT = T * T;                 // table rows
  static constexpr int RMIN = (2 - OWS) * (T + 1); // smallest r; the largest is RMIN + TT - 1
  static constexpr int MAXG = WS == 8 ? 4 : 2;     // heads a workgroup, at most
  static constexpr int MAXT = MAXG * NQB / NW;     // (head, query block) turns a wave, at most
  static constexpr int KV_HEAD = (KB * LDQ + DP * LDV) * 2;
  static constexpr int PER_HEAD = KV_HEAD + TT * 4;
  static int lds(int G) { return G * PER_HEAD; }
  static_assert(KB % 16 == 0 && OWS % 4 == 0 && OWS % BR == 0 && KV_HEAD % 16 == 0, "band geometry");
  static_assert(NQ * LDQ * 2 <= KV_HEAD, "o is staged over K and Vt");
  static_assert(MAXT * NW == MAXG * NQB, "turns");
};

// Heads per workgroup (see the header): a 128-byte segment where OA_LDS_SOFT allows it, at most MAXG, evened out.
template <class Cf>
int overlap_groups(int heads, int D) {
  int G = (64 + D - 1) / D;
  if (G > heads) G = heads;
  if (G > Cf::MAXG) G = Cf::MAXG;
  while (G > 1 && Cf::lds(G) > OA_LDS_SOFT) --G;
  const int ng = (heads + G - 1) / G;
  return (heads + ng - 1) / ng;
}

template <int WS>
__global__ __launch_bounds__(OvCfg<WS>::NT) void overlap_attn_kernel(const OvArgs a) {
  using Cf = OvCfg<WS>;
  constexpr int OWS = Cf::OWS, PAD = Cf::PAD, NQ = Cf::NQ, NQB = Cf::NQB, NW = Cf::NW, NT = Cf::NT, BR = Cf::BR;
  constexpr int NB = Cf::NB, KB = Cf::KB, NKB = Cf::NKB, NKBP = Cf::NKBP, DP = Cf::DP, LDQ = Cf::LDQ, LDV = Cf::LDV;
  constexpr int T = Cf::T, TT = Cf::TT, RMIN = Cf::RMIN, MAXT = Cf::MAXT;
  constexpr float LOG2E = 1.4426950408889634f;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int G = a.G;
  u16* Ks = reinterpret_cast<u16*>(smem);
  u16* Vt = Ks + G * KB * LDQ;
  float* tab = reinterpret_cast<float*>(Vt + G * DP * LDV);
  u16* Os = Ks;                                  // after the last band

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int nwx = a.W / WS, nwin = (a.H / WS) * nwx;
  int bid = blockIdx.x;
  const int grp = bid % a.ngroups;
  bid /= a.ngroups;
  const int win = bid % nwin, b = bid / nwin;
  const int wy = win / nwx, wx = win - wy * nwx;
  const int D = a.D, C = a.heads * D;
  const int h0 = grp * G;
  const int GH = min(G, a.heads - h0);           // heads of this group (the last one may be short)
  const int segdw = GH * D / 2;                  // dwords of the group's segment of a token row
  const size_t img = (size_t)b * a.H * a.W;
  const int y0 = wy * WS - PAD, x0 = wx * WS - PAD;   // image position of key (0, 0); may be negative

  // ---- once: K and Vt zeroed (head-dim pad, key pad, row pads), the group's table columns with the wrap undone
  for (int idx = tid; idx < G * Cf::KV_HEAD / 16; idx += NT) reinterpret_cast<uint4*>(smem)[idx] = uint4{0u, 0u, 0u, 0u};
  for (int idx = tid; idx < GH * TT; idx += NT) {
    const int hl = idx / TT;
    int r = idx - hl * TT + RMIN;
    if (r < 0) r += TT;
    tab[idx] = a.table[(size_t)r * a.heads + h0 + hl];
  }

  // ---- the turns of this wave: Q fragment from global memory (d >= D: zero), softmax state
  bf16x8 qf[MAXT];
  f32x4 oacc[MAXT][2];
  float m_run[MAXT], l_run[MAXT];
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const int bi = t * NW + wave;
    m_run[t] = -INFINITY;
    l_run[t] = 0.f;
    oacc[t][0] = oacc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (bi < GH * NQB) {
      const int hl = bi / NQB, tq = 16 * (bi - hl * NQB) + fr;
      const size_t pix = (size_t)(wy * WS + tq / WS) * a.W + wx * WS + tq % WS;
      const u16* src = a.qkv + (img + pix) * 3 * C + (h0 + hl) * D + 8 * fq;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (8 * fq + 2 * i < D) w[i] = *reinterpret_cast<const uint32_t*>(src + 2 * i);
    }
    const uint4 w4 = {w[0], w[1], w[2], w[3]};
    qf[t] = __builtin_bit_cast(bf16x8, w4);
  }

#pragma unroll 1
  for (int band = 0; band < NB; ++band) {
    __syncthreads();      // the zeroing (band 0); every wave done with the previous band
    // ---- k, v segments of the band's positions: HBM / L2 -> LDS in 4-byte units, V transposed; outside: zeros
    for (int idx = tid; idx < KB * segdw; idx += NT) {
      const int t = idx / segdw, e = 2 * (idx - t * segdw);
      const int hl = e / D, d = e - hl * D;
      const int kyl = t / OWS, kx = t - kyl * OWS;
      const int y = y0 + band * BR + kyl, x = x0 + kx;
      uint32_t k = 0u, v = 0u;
      if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W) {
        const u16* src = a.qkv + (img + (size_t)y * a.W + x) * 3 * C + C + h0 * D + e;
        k = *reinterpret_cast<const uint32_t*>(src);
        v = *reinterpret_cast<const uint32_t*>(src + C);
      }
      *reinterpret_cast<uint32_t*>(&Ks[(hl * KB + t) * LDQ + d]) = k;
      Vt[(hl * DP + d) * LDV + t] = (u16)(v & 0xffffu);
      Vt[(hl * DP + d + 1) * LDV + t] = (u16)(v >> 16);
    }
    __syncthreads();

#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      const int bi = t * NW + wave;
      if (bi >= GH * NQB) continue;              // wave-uniform
      const int hl = bi / NQB, tq = 16 * (bi - hl * NQB) + fr;
      const int qy = tq / WS, qx = tq % WS;
      f32x4 s[NKB];
#pragma unroll
      for (int j = 0; j < NKB; ++j) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&Ks[(hl * KB + 16 * j + fr) * LDQ + 8 * fq]);
        s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[t], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      }
      // x = s scale + table[r]: slot r - RMIN of the staged column
      const float* tb = tab + hl * TT - RMIN + (band * BR - qy + WS - OWS + 1) * T + (WS - OWS + 1 - qx);
      float mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < NKB; ++j) {
        const int k0 = 16 * j + 4 * fq;          // four keys of one key row
        const int kyl = k0 / OWS, kx0 = k0 - kyl * OWS;
        const float* tr = tb + kyl * T + kx0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float sc = s[j][q] * a.scale;
          const float x = sc + tr[q];
          s[j][q] = x;
          mx = fmaxf(mx, x);
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      float l = l_run[t];
      if (NB > 1) {                              // online rescale: exact 0 on the first band (m = -inf)
        const float mn = fmaxf(m_run[t], mx);
        const float al = __builtin_amdgcn_exp2f((m_run[t] - mn) * LOG2E);
        l *= al;
        oacc[t][0] *= al;
        oacc[t][1] *= al;
        m_run[t] = mx = mn;
      }
#pragma unroll
      for (int j = 0; j < NKB; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float p = __builtin_amdgcn_exp2f((s[j][q] - mx) * LOG2E);
          s[j][q] = p;
          l += p;
        }
      l_run[t] = l;
#pragma unroll
      for (int m = 0; m < NKBP / 2; ++m) {
        bf16x8 pf = {(__bf16)s[2 * m][0], (__bf16)s[2 * m][1], (__bf16)s[2 * m][2], (__bf16)s[2 * m][3],
                     (__bf16)0.f,         (__bf16)0.f,         (__bf16)0.f,         (__bf16)0.f};
        if (2 * m + 1 < NKB) {                   // compile time: the pad block of ws 8 has P = 0
          pf[4] = (__bf16)s[(2 * m + 1) % NKB][0];
          pf[5] = (__bf16)s[(2 * m + 1) % NKB][1];
          pf[6] = (__bf16)s[(2 * m + 1) % NKB][2];
          pf[7] = (__bf16)s[(2 * m + 1) % NKB][3];
        }
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const u16* vr = &Vt[(hl * DP + 16 * db + fr) * LDV + 32 * m + 4 * fq];
          const s16x4 lo = *reinterpret_cast<const s16x4*>(vr);
          const s16x4 hi = *reinterpret_cast<const s16x4*>(vr + 16);
          const s16x8 vv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          oacc[t][db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vv), pf, oacc[t][db], 0, 0, 0);
        }
      }
    }
  }
  __syncthreads();        // K and Vt are free: o is staged over them

#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const int bi = t * NW + wave;
    if (bi >= GH * NQB) continue;
    const int hl = bi / NQB, tq = 16 * (bi - hl * NQB) + fr;
    float l = l_run[t];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
#pragma unroll
    for (int db = 0; db < 2; ++db)
      *reinterpret_cast<uint2*>(&Os[(hl * NQ + tq) * LDQ + 16 * db + 4 * fq]) =
          pack4_bf16(oacc[t][db][0] * inv, oacc[t][db][1] * inv, oacc[t][db][2] * inv, oacc[t][db][3] * inv);
  }
  __syncthreads();

  // ---- the group's segment of every query's token row
  for (int idx = tid; idx < NQ * segdw; idx += NT) {
    const int t = idx / segdw, e = 2 * (idx - t * segdw);
    const int hl = e / D, d = e - hl * D;
    const size_t pix = (size_t)(wy * WS + t / WS) * a.W + wx * WS + t % WS;
    *reinterpret_cast<uint32_t*>(a.o + (img + pix) * C + h0 * D + e) =
        *reinterpret_cast<const uint32_t*>(&Os[(hl * NQ + t) * LDQ + d]);
  }
}

template <int WS>
int overlap_attn_launch(OvArgs a, hipStream_t stream) {
  using Cf = OvCfg<WS>;
  a.G = overlap_groups<Cf>(a.heads, a.D);
  a.ngroups = (a.heads + a.G - 1) / a.G;
  const long long nwg = (long long)a.B * (a.H / WS) * (a.W / WS) * a.ngroups;
  if (nwg <= 0 || nwg > 0x7fffffffLL || (long long)a.H * a.W > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  max_dynamic_lds_once<overlap_attn_kernel<WS>>(OA_LDS_HARD);
  overlap_attn_kernel<WS><<<dim3((unsigned)nwg), Cf::NT, Cf::lds(a.G), stream>>>(a);
  return (int)hipGetLastError();
}

}  // namespace

// qkv bf16 [B, H*W, 3*C] contiguous, o bf16 [B, H*W, C], table fp32 [(ws+ows-1)^2, heads].
// Domain: (ws, ows) (8, 12) or (16, 24), H % ws == W % ws == 0, D even in [2, 32], qkv and o 4-byte aligned; anything
// else is hipErrorInvalidValue and nothing is launched.
CGS_EXPORT int cgs_overlap_attn_fwd(const void* qkv, void* o, const float* table, float scale, int B, int H, int W,
                                    int heads, int D, int ws, int ows, hipStream_t stream) {
  if (!qkv || !o || !table || B <= 0 || H <= 0 || W <= 0 || heads <= 0) return (int)hipErrorInvalidValue;
  if ((ws != 8 && ws != 16) || 2 * ows != 3 * ws || H % ws || W % ws) return (int)hipErrorInvalidValue;
  if (D < 2 || D > 32 || (D & 1)) return (int)hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(o)) & 3) return (int)hipErrorInvalidValue;
  const OvArgs a{(const u16*)qkv, (u16*)o, table, scale, B, H, W, heads, D, 0, 0};
  return ws == 8 ? overlap_attn_launch<8>(a, stream) : overlap_attn_launch<16>(a, stream);
}
