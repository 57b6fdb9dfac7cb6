// Rectangular-window attention forward for DAT's spatial blocks on gfx950.
//
//   o = softmax(scale * q.k + table[r(q, k), h] + m(q, k)) v      per wh x ww window and head, fp32 scores
//
// A spatial block splits the channels in two branches. Branch i owns channels [i C/2, (i+1) C/2) of each of q, k and
// v (heads / 2 heads), attends in wh x ww = (s0, s1) (branch 0) or (s1, s0) (branch 1) windows shifted by
// (wh / 2, ww / 2) when `shifted`, and has its own fp32 table [(2wh-1)(2ww-1), heads / 2], indexed
// r = (yq - yk + wh-1)(2ww-1) + (xq - xk + ww-1). The image is padded to Hp x Wp, multiples of max(s0, s1): rolled
// position (i, j) of the padded grid is source pixel ((i + sh) % Hp, (j + sw) % Wp), and a source pixel with y >= H
// or x >= W is a zero q / k / v row. As a key it is NOT masked (its score is table + m, it counts in the row sum); as
// a query it is never written. m = -100 (finite) where the region labels of the two tokens differ (per axis, on the
// padded rolled grid: index < n - w: 0, < n - s: 1, else 2; `shifted` only). The kernel reads the packed qkv
// [B, H*W, 3*C] (channel order [3][heads][D]) where it lies and writes both branches' halves of o [B, H*W, C] at the
// un-shifted, un-padded pixels: no pad, channel slice, roll, partition, [h, N, N] bias, [nW, N, N] mask,
// un-partition, crop or concat exists in memory.
//
// Work split. One launch, grid (image x window, branch). One workgroup owns one window of one branch and all
// heads / 2 heads of it, so every byte of the branch's half-row segments (180 B at dim 180) comes from HBM once. The
// heads are staged G at a time (rect_chunk on the host: at most 3, evened out; heads / 2 <= 3 is one chunk). A
// workgroup none of whose queries lies in the image (whole windows of the padding) returns before its first load.
//
// Data movement, per chunk. The loader works in 4-byte units (D is even; head slices start at 60-byte offsets at
// D = 30): lane-consecutive dwords of a token's k and v segments go to LDS as K[h][token][DP + 8] and, transposed,
// Vt[h][d][N + 8], DP = 32; the head-dim pad is zeroed in LDS, never in memory; an out-of-image token takes no load
// and stores zeros (one predicate per dword in the loader, none in the MFMA loops). The chunk's table columns, and
// once per workgroup the source pixel (-1: outside) and the region label of every window token, are LDS tables. Q
// never goes through LDS: the fragment of a wave's 16 queries is four guarded dwords a lane from global memory, the
// next head's fetched while the current head computes.
//
// Compute. The heads of a chunk run one after the other; a head is N / 16 query blocks over N / 32 waves: two turns
// a wave (MFMA 16x16x32 bf16, wave64; fr = lane & 15, fq = lane >> 4):
//   S^T = K Q^T      A = 16 key rows, B = 16 query rows: acc[j][q] = score of key 16 j + 4 fq + q for query fr. A lane
//                    holds N / 4 scores of ONE query: all 128 or 256 keys sit in accumulators at once, the softmax is
//                    single pass (no online rescale). ww % 4 == 0: a lane's four keys lie in one window row and read
//                    four consecutive table slots and one dword of labels.
//   x = fl(fl(s scale) + add), add = table (+ -100);  mx: lane-local, then lane ^ 16, lane ^ 32;
//   p = exp2(fl(fl(x - mx) L)), row sum likewise
//   O^T = V^T P^T    the bf16-rounded p ARE the B operand; the A operand reads Vt in the same key order (two 8-byte
//                    LDS reads). acc[db][q] = O[query fr][16 db + 4 fq + q].
//   A barrier ends the head: K_h's rows are dead then and take O / rowsum rounded to bf16 (no staging area of its
//   own). After the chunk's last head the workgroup copies the chunk's segment of every in-image query's token row to
//   o in lane-consecutive dwords, never per-head scatters.
//
// LDS, bytes a head: K N x 40 x 2 + Vt 32 x (N + 8) x 2 + table (2wh-1)(2ww-1) x 4, plus 5 N for pixels and labels:
//   N = 256 (8 x 32)  20480 + 16896 + 3780 = 41156;  3 heads: 124748, one 512-thread workgroup a CU
//   N = 128 (8 x 16)  10240 +  8704 + 1860 = 20804;  3 heads:  63052, two 256-thread workgroups a CU
// As compiled for gfx950 (kernel_resources.json; a compile, not a run): N = 256 164 VGPRs, N = 128 148 VGPRs + 8
// AGPRs, no scratch (the build fails on any); LDS decides the occupancy, 8 waves (2 a SIMD) a CU either way. No
// workspace, no host synchronisation: capturable.
#include "common.h"

namespace {

constexpr int RA_LDS_HARD = 160 * 1024;   // the CU's LDS
constexpr int RA_MAXG = 3;                // heads staged at a time

struct RectArgs {
  const u16* qkv;
  u16* o;
  const float* table0;
  const float* table1;
  float scale;
  int B, H, W, Hp, Wp, heads, D, s0, s1, shifted;
  int G;
};

template <int N>
struct RectCfg {
  static constexpr int NKB = N / 16;            // 16-key blocks = 16-query blocks a head
  static constexpr int NW = N / 32;             // waves: two turns each a head
  static constexpr int NT = 64 * NW;
  static constexpr int DP = 32;
  static constexpr int LDQ = DP + 8;            // K / staged-o row (elements): 80 bytes
  static constexpr int LDV = N + 8;             // Vt row (elements): 272 / 528 bytes, 8-byte multiples
  static constexpr int KV_HEAD = (N * LDQ + DP * LDV) * 2;
  static int lds(int G, int R) { return G * (KV_HEAD + R * 4) + N * 4 + N; }
  static_assert(KV_HEAD % 16 == 0 && NKB == 2 * NW, "geometry");
};

// Heads staged at a time: at most RA_MAXG, evened out over the chunks.
inline int rect_chunk(int hb) {
  const int nch = (hb + RA_MAXG - 1) / RA_MAXG;
  return (hb + nch - 1) / nch;
}

template <int N>
__global__ __launch_bounds__(RectCfg<N>::NT) void rect_attn_kernel(const RectArgs a) {
  using Cf = RectCfg<N>;
  constexpr int NKB = Cf::NKB, NW = Cf::NW, NT = Cf::NT, DP = Cf::DP, LDQ = Cf::LDQ, LDV = Cf::LDV;
  constexpr float LOG2E = 1.4426950408889634f;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int G = a.G;
  u16* Ks = reinterpret_cast<u16*>(smem);
  u16* Vt = Ks + G * N * LDQ;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int br = blockIdx.y;
  const int wh = br ? a.s1 : a.s0, ww = br ? a.s0 : a.s1;     // powers of two, wh ww = N
  const int lw = __builtin_ctz(ww);
  const int sh = a.shifted ? wh >> 1 : 0, sw = a.shifted ? ww >> 1 : 0;
  const int T = 2 * ww - 1, R = (2 * wh - 1) * T;
  float* tab = reinterpret_cast<float*>(Vt + G * DP * LDV);
  int* tok = reinterpret_cast<int*>(tab + G * R);
  unsigned char* lab = reinterpret_cast<unsigned char*>(tok + N);

  const int nwx = a.Wp >> lw, nwin = (a.Hp / wh) * nwx;
  const int win = blockIdx.x % nwin, b = blockIdx.x / nwin;
  const int wy = win / nwx, wx = win - wy * nwx;
  const int D = a.D, C = a.heads * D, HB = a.heads >> 1;
  const size_t img = (size_t)b * a.H * a.W;
  const u16* qkv = a.qkv + br * HB * D;          // the branch's half of a q row; k at + C, v at + 2 C
  u16* o = a.o + br * HB * D;
  const float* table = br ? a.table1 : a.table0;

  // ---- no query of this window in the image: its source rows (columns) are wh (ww) consecutive ones from y0 (x0),
  // cyclic in Hp (Wp); one of them is below H iff the run starts below H or wraps to 0
  int y0 = wy * wh + sh, x0 = (wx << lw) + sw;
  if (y0 >= a.Hp) y0 -= a.Hp;
  if (x0 >= a.Wp) x0 -= a.Wp;
  if (!((y0 < a.H || y0 + wh > a.Hp) && (x0 < a.W || x0 + ww > a.Wp))) return;

  // ---- window geometry: source pixel (-1: outside the image) and region label of every window token
  if (tid < N) {
    const int ry = wy * wh + (tid >> lw), rx = (wx << lw) + (tid & (ww - 1));     // rolled coordinates
    int sy = ry + sh, sx = rx + sw;
    if (sy >= a.Hp) sy -= a.Hp;
    if (sx >= a.Wp) sx -= a.Wp;
    tok[tid] = sy < a.H && sx < a.W ? sy * a.W + sx : -1;
    const int ly = ry < a.Hp - wh ? 0 : (ry < a.Hp - sh ? 1 : 2);
    const int lx = rx < a.Wp - ww ? 0 : (rx < a.Wp - sw ? 1 : 2);
    lab[tid] = (unsigned char)(a.shifted ? 3 * ly + lx : 0);
  }

#pragma unroll 1
  for (int h0 = 0; h0 < HB; h0 += G) {
    const int GH = min(G, HB - h0);             // heads of this chunk (the last one may be short)
    const int segdw = GH * D / 2;               // dwords of the chunk's segment of a token row
    __syncthreads();      // tok and lab (first chunk); the previous chunk's copy to o is done with K

    // Q fragment of turn t (query block t NW + wave) of head hl: global memory -> registers, d >= D and
    // out-of-image queries zero
    auto load_q = [&](int hl, int t) -> bf16x8 {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      const int tk = tok[16 * (t * NW + wave) + fr];
      if (tk >= 0 && hl < GH) {
        const u16* src = qkv + (img + tk) * 3 * C + (h0 + hl) * D + 8 * fq;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (8 * fq + 2 * i < D) w[i] = *reinterpret_cast<const uint32_t*>(src + 2 * i);
      }
      const uint4 w4 = {w[0], w[1], w[2], w[3]};
      return __builtin_bit_cast(bf16x8, w4);
    };
    bf16x8 qf[2] = {load_q(0, 0), load_q(0, 1)};

    // ---- the chunk's table columns; the pad of the head dim, zero in LDS
    for (int idx = tid; idx < GH * R; idx += NT) {
      const int hl = idx / R, r = idx - hl * R;
      tab[idx] = table[(size_t)r * HB + h0 + hl];
    }
    if (D < DP) {
      const int pd = (DP - D) >> 1;             // dwords of pad a row
      for (int idx = tid; idx < GH * N * pd; idx += NT) {
        const int row = idx / pd, d = D + 2 * (idx - row * pd);     // row = hl * N + token
        const int hl = row / N, t = row - hl * N;
        *reinterpret_cast<uint32_t*>(&Ks[row * LDQ + d]) = 0u;
        Vt[(hl * DP + d) * LDV + t] = 0;
        Vt[(hl * DP + d + 1) * LDV + t] = 0;
      }
    }
    // ---- k, v segments of the window's tokens: HBM -> LDS in 4-byte units, V transposed; outside: zeros
    for (int idx = tid; idx < N * segdw; idx += NT) {
      const int t = idx / segdw, e = 2 * (idx - t * segdw);
      const int hl = e / D, d = e - hl * D;
      const int tk = tok[t];
      uint32_t k = 0u, v = 0u;
      if (tk >= 0) {
        const u16* src = qkv + (img + tk) * 3 * C + C + h0 * D + e;
        k = *reinterpret_cast<const uint32_t*>(src);
        v = *reinterpret_cast<const uint32_t*>(src + C);
      }
      *reinterpret_cast<uint32_t*>(&Ks[(hl * N + t) * LDQ + d]) = k;
      Vt[(hl * DP + d) * LDV + t] = (u16)(v & 0xffffu);
      Vt[(hl * DP + d + 1) * LDV + t] = (u16)(v >> 16);
    }
    __syncthreads();

#pragma unroll 1
    for (int hl = 0; hl < GH; ++hl) {
      const float* tb = tab + hl * R;
      uint2 ob[2][2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int tq = 16 * (t * NW + wave) + fr;      // this lane's query (window token)
        f32x4 s[NKB];
#pragma unroll
        for (int j = 0; j < NKB; ++j) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&Ks[(hl * N + 16 * j + fr) * LDQ + 8 * fq]);
          s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[t], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        }
        // x = s scale + (table + mask)
        const int iq = tq >> lw, jq = tq & (ww - 1);
        const uint32_t labq = lab[tq] * 0x01010101u;
        const int rq = (iq + wh - 1) * T + jq + ww - 1;
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < NKB; ++j) {
          const int k0 = 16 * j + 4 * fq;              // four keys of one window row
          const float* tr = tb + rq - (k0 >> lw) * T - (k0 & (ww - 1));
          const uint32_t diff = *reinterpret_cast<const uint32_t*>(&lab[k0]) ^ labq;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float sc = s[j][q] * a.scale;
            float add = tr[-q];
            if ((diff >> (8 * q)) & 0xffu) add += -100.0f;
            const float x = sc + add;
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
            const float p = __builtin_amdgcn_exp2f((s[j][q] - mx) * LOG2E);
            s[j][q] = p;
            l += p;
          }
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        f32x4 oacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int m = 0; m < NKB / 2; ++m) {
          const bf16x8 pf = {(__bf16)s[2 * m][0],     (__bf16)s[2 * m][1],     (__bf16)s[2 * m][2],
                             (__bf16)s[2 * m][3],     (__bf16)s[2 * m + 1][0], (__bf16)s[2 * m + 1][1],
                             (__bf16)s[2 * m + 1][2], (__bf16)s[2 * m + 1][3]};
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            const u16* vr = &Vt[(hl * DP + 16 * db + fr) * LDV + 32 * m + 4 * fq];
            const s16x4 lo = *reinterpret_cast<const s16x4*>(vr);
            const s16x4 hi = *reinterpret_cast<const s16x4*>(vr + 16);
            const s16x8 vv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            oacc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vv), pf, oacc[db], 0, 0, 0);
          }
        }
        const float inv = 1.0f / l;
#pragma unroll
        for (int db = 0; db < 2; ++db)
          ob[t][db] = pack4_bf16(oacc[db][0] * inv, oacc[db][1] * inv, oacc[db][2] * inv, oacc[db][3] * inv);
        qf[t] = load_q(hl + 1, t);                     // the next head's fragment (zeros after the last)
      }
      __syncthreads();    // every wave is done with K_h: its rows take o_h
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int db = 0; db < 2; ++db)
          *reinterpret_cast<uint2*>(&Ks[(hl * N + 16 * (t * NW + wave) + fr) * LDQ + 16 * db + 4 * fq]) = ob[t][db];
    }
    __syncthreads();

    // ---- the chunk's segment of every in-image query's token row, at its source pixel
    for (int idx = tid; idx < N * segdw; idx += NT) {
      const int t = idx / segdw, e = 2 * (idx - t * segdw);
      const int hl = e / D, d = e - hl * D;
      const int tk = tok[t];
      if (tk >= 0)
        *reinterpret_cast<uint32_t*>(o + (img + tk) * C + h0 * D + e) =
            *reinterpret_cast<const uint32_t*>(&Ks[(hl * N + t) * LDQ + d]);
    }
  }
}

template <int N>
int rect_attn_launch(RectArgs a, hipStream_t stream) {
  using Cf = RectCfg<N>;
  const int R = (2 * a.s0 - 1) * (2 * a.s1 - 1);
  a.G = rect_chunk(a.heads / 2);
  const int lds = Cf::lds(a.G, R);
  const long long nwg = (long long)a.B * ((long long)a.Hp * a.Wp / N);
  if (lds > RA_LDS_HARD || nwg <= 0 || nwg > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  max_dynamic_lds_once<rect_attn_kernel<N>>(RA_LDS_HARD);
  rect_attn_kernel<N><<<dim3((unsigned)nwg, 2u), Cf::NT, lds, stream>>>(a);
  return (int)hipGetLastError();
}

}  // namespace

// qkv bf16 [B, H*W, 3*C] contiguous, o bf16 [B, H*W, C], table0 / table1 fp32 [(2 s0 - 1)(2 s1 - 1), heads / 2] of
// branch 0 (s0 x s1 windows, channels [0, C/2)) and branch 1 (s1 x s0 windows, channels [C/2, C)).
// Domain: (s0, s1) in {(8, 16), (16, 8), (8, 32), (32, 8)}, heads even, D even in [2, 32], any H, W, B >= 1, qkv and o
// 4-byte aligned, the padded grid and the workgroup count within int; anything else is hipErrorInvalidValue and
// nothing is launched.
CGS_EXPORT int cgs_rect_attn_fwd(const void* qkv, void* o, const float* table0, const float* table1, float scale,
                                 int B, int H, int W, int heads, int D, int s0, int s1, int shifted,
                                 hipStream_t stream) {
  if (!qkv || !o || !table0 || !table1 || B <= 0 || H <= 0 || W <= 0) return (int)hipErrorInvalidValue;
  if (heads < 2 || (heads & 1) || D < 2 || D > 32 || (D & 1)) return (int)hipErrorInvalidValue;
  const int lo = s0 < s1 ? s0 : s1, m = s0 < s1 ? s1 : s0;
  if (lo != 8 || (m != 16 && m != 32)) return (int)hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(o)) & 3) return (int)hipErrorInvalidValue;
  const long long Hp = ((long long)H + m - 1) / m * m, Wp = ((long long)W + m - 1) / m * m;
  if (Hp * Wp > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  const RectArgs a{(const u16*)qkv, (u16*)o, table0, table1, scale, B, H, W, (int)Hp, (int)Wp, heads, D, s0, s1,
                   shifted ? 1 : 0, 0};
  return m == 16 ? rect_attn_launch<128>(a, stream) : rect_attn_launch<256>(a, stream);
}
