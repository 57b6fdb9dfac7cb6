// K12 (tap form): nearest-2x upsample + 3x3 conv (stride 1, pad 1) with every tap product formed ONCE, at
// low resolution. conv.hip's CONV_UP2X runs the 9-tap implicit GEMM at the upsampled resolution, where each
// product x[p, ci] * W[co, ci, dy, dx] is formed four times (every upsampled pixel is one of four copies).
//
//   T[dy,dx][n, i, j, co] = sum_ci x[n, i, j, ci] * W[co, ci, dy, dx]            fp32, low resolution
//   out[n, 2i+a, 2j+b, co] = bias[co] + sum_{dy,dx} T[dy,dx][n, (2i+a+dy-1) >> 1, (2j+b+dx-1) >> 1, co]
//
// A tap whose upsampled coordinate lies outside the image has its source pixel outside the low-resolution
// image too ((-1) >> 1 = -1, (2H) >> 1 = H), so it is enough that out-of-image rows of the GEMM are zeros.
// Every product stays exact (bf16 x bf16 in fp32); against CONV_UP2X only the order of the fp32 additions
// changes, and the one rounding to bf16 is at the store.
//
// One workgroup (8 waves) takes a pw x ph low-resolution patch, one-pixel halo included, as its 256 GEMM rows
// (16 x 16, or 18 x 14 / 14 x 18 / 34 x 7 where that covers the image in fewer patches) and NG = 2 groups of 16
// output channels x 9 taps as its 288 columns (weights pre-ordered [Cout / 16][tap][16][Cin],
// ops.upconv_tap_weights). Main loop: 256 x 288 x 64 tiles, LDS-DMA double buffer with the 8-row x 128-B swizzled
// pieces of conv v2, a plain row loader (no im2col); wave w owns rows 32 w .. 32 w + 31 and all 18 column tiles
// (36 accumulators, 20 ds_read_b128 per 36 MFMAs). Measured slower, profiles/r07: one group per workgroup (half
// the MFMAs per byte fetched from L2: 1.3-1.7x instead of 1.6-2.1x over CONV_UP2X), 4 waves with 64 rows each,
// a 3-stage ring. The fp32 tap tile T[256][144] (144 KiB) of one group at a time is then written over the
// staging buffers and the four output pixels of every interior source pixel are combined from it: 25 float4
// reads (centre 9 taps, edge neighbours 3 each, corners 1 each) and 36 additions for 4 pixels x 4 channels.
// Pixels whose source lies in the halo belong to the neighbouring patch and are not written.
//
// LDS behaviour of the epilogue. T's row pitch is 144 floats = 16 mod 64 banks.
//   store (ds_write_b32, two groups of 32 lanes, bank = dword mod 32): a group holds 16 consecutive columns of
//     rows 4 apart (4 * 144 = 0 mod 32): 2-way, which costs a ds_write_b32 nothing (the address / data transfer
//     sets its cycles).
//   combine (ds_read_b128, four fixed groups of 16 lanes, bank = dword mod 64): lane = 4 * pixel + channel quad,
//     and the lanes of a group are four pixels whose GEMM rows differ mod 4 ({0, 3, 5, 6} and {1, 2, 4, 7}), each
//     reading 64 contiguous bytes: windows 16 banks apart, conflict-free for every (neighbour, tap) since those
//     only add a constant.
#include "common.h"
#include <stdlib.h>

typedef __attribute__((address_space(3))) void lds_void;

__device__ __attribute__((aligned(16))) unsigned char g_upconv_zero_page[256];

struct UpconvArgs {
  const u16* in;     // [N, H, W, Cin]
  const u16* wt;     // [groups][9][16][Cin]
  const u16* bias;   // [Cout] or null
  u16* out;          // [N, 2H, 2W, Cout]
  int N, H, W, Cin, Cout;
  int pw, ph;        // patch extent with halo, pw * ph <= 256
  int tiles_x, tiles_y;
  int groups16;      // ceil(Cout / 16): 16-channel groups in wt
  int groups;        // column tiles of the grid: ceil(groups16 / NG)
  int group_m;
};

namespace uc {
constexpr int BM = 256, BK = 64, NT = 9, CG = 16, BN = NT * CG;
constexpr int A_BYTES = BM * BK * 2;
constexpr int T_PITCH = BN;   // floats
constexpr int T_BYTES = BM * T_PITCH * 4;
constexpr int NG = 2;                               // 16-channel groups per workgroup
constexpr int BROWS = NG * BN;                      // weight rows per stage
constexpr int NJ = NG * NT;                         // 16-column MFMA tiles per wave
constexpr int STAGE = A_BYTES + BROWS * BK * 2;
constexpr int LDS = T_BYTES > 2 * STAGE ? T_BYTES : 2 * STAGE;
constexpr int NW = 8;                               // waves: two per SIMD, 32 rows each
constexpr int A_PIECES = BM / 8 / NW;               // 8-row pieces per wave
constexpr int B_PIECES = (BROWS / 8 + NW - 1) / NW; // 36 pieces dealt round-robin: waves 0-3 take 5, the rest 4
// source offset of tap d for output parity a: ((2 i + a + d - 1) >> 1) - i
__device__ __forceinline__ constexpr int nb(int a, int d) { return a == 0 ? (d == 0 ? -1 : 0) : (d == 2 ? 1 : 0); }
}   // namespace uc

__global__ __launch_bounds__(64 * uc::NW) void upconv_taps_kernel(UpconvArgs a) {
  using namespace uc;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int prow = lane >> 3, pchunk = lane & 7;

  const int patches = a.N * a.tiles_y * a.tiles_x;
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  int tp, grp;
  grouped_tile(logical, patches, a.groups, a.group_m, tp, grp);
  const int n = tp / (a.tiles_y * a.tiles_x);
  const int trem = tp - n * a.tiles_y * a.tiles_x;
  const int ty = trem / a.tiles_x, tx = trem - ty * a.tiles_x;
  const int y0 = ty * (a.ph - 2) - 1, x0 = tx * (a.pw - 2) - 1;   // image coordinates of patch row 0

  // loader slots: per-lane source of each A / B piece (chunk swizzle folded in), null = zeros
  const u16* asrc[A_PIECES];
  int achk[A_PIECES];
#pragma unroll
  for (int i = 0; i < A_PIECES; ++i) {
    const int r = (wave * A_PIECES + i) * 8 + prow;
    const int py = r / a.pw, px = r - py * a.pw;
    const int y = y0 + py, x = x0 + px;
    const bool ok = py < a.ph && y >= 0 && y < a.H && x >= 0 && x < a.W;
    achk[i] = 8 * (pchunk ^ ((r >> 1) & 7));
    asrc[i] = ok ? a.in + (((long long)n * a.H + y) * a.W + x) * a.Cin + achk[i] : nullptr;
  }
  const u16* bsrc[B_PIECES];
  int bchk[B_PIECES];
#pragma unroll
  for (int i = 0; i < B_PIECES; ++i) {
    const int g = wave + NW * i;
    const int r = (g < BROWS / 8 ? g : 0) * 8 + prow;
    const long long wr = (long long)grp * BROWS + r;      // the NG groups' rows are consecutive in wt
    bchk[i] = 8 * (pchunk ^ ((r >> 1) & 7));
    bsrc[i] = wr < (long long)a.groups16 * BN ? a.wt + wr * a.Cin + bchk[i] : nullptr;   // past the last group: zeros
  }
  const void* zero = (const void*)(g_upconv_zero_page + 16 * (lane & 15));
  auto issue = [&](int kt, int stage) {
    unsigned char* base = smem + stage * STAGE;
    const int k0 = kt * BK;
#pragma unroll
    for (int i = 0; i < A_PIECES; ++i) {
      const bool ok = asrc[i] != nullptr && k0 + achk[i] < a.Cin;   // Cin % 64 == 32: the last tile's upper half
      const void* src = ok ? (const void*)(asrc[i] + k0) : zero;
      __builtin_amdgcn_global_load_lds(src, (lds_void*)(base + ((wave * A_PIECES + i) * 8) * 128), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < B_PIECES; ++i) {
      const int g = wave + NW * i;
      if (g < BROWS / 8) {   // wave-uniform
        const void* src = bsrc[i] != nullptr && k0 + bchk[i] < a.Cin ? (const void*)(bsrc[i] + k0) : zero;
        __builtin_amdgcn_global_load_lds(src, (lds_void*)(base + A_BYTES + (g * 8) * 128), 16, 0, 0);
      }
    }
  };

  constexpr int NI = BM / NW / 16;
  f32x4 acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (a.Cin + BK - 1) / BK;
  const int fr = lane & 15, fq = lane >> 4;
  const int wm = wave * (16 * NI);
  issue(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const int st = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) issue(kt + 1, st ^ 1);   // the stage tile kt - 1 was read from: every wave has left it
    const unsigned char* As = smem + st * STAGE;
    const unsigned char* Bs = As + A_BYTES;
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      bf16x8 af[NI];
      const int c = kk * 4 + fq;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int r = wm + i * 16 + fr;
        af[i] = *reinterpret_cast<const bf16x8*>(As + r * 128 + 16 * (c ^ ((r >> 1) & 7)));
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int r = j * 16 + fr;
        const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(Bs + r * 128 + 16 * (c ^ ((r >> 1) & 7)));
#pragma unroll
        for (int i = 0; i < NI; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr, acc[i][j], 0, 0, 0);
      }
    }
  }

  float* T = reinterpret_cast<float*>(smem);
  const float4* T4 = reinterpret_cast<const float4*>(smem);
  const int cq = lane & 3;
  const int Ho = 2 * a.H, Wo = 2 * a.W;
#pragma unroll
  for (int h = 0; h < NG; ++h) {
    // tap tile of group h -> LDS (over the staging buffers, then over the previous group's tile):
    // acc[i][9 h + j][q] = (row wm + 16 i + 4 fq + q, tap j, channel fr)
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) T[(wm + i * 16 + fq * 4 + q) * T_PITCH + j * CG + fr] = acc[i][h * NT + j][q];
    __syncthreads();

    // combine: item = (patch row r, channel quad cq); 1024 items over 512 threads
    const int co = (grp * NG + h) * CG + cq * 4;
    float4 bv = float4{0.f, 0.f, 0.f, 0.f};
    if (a.bias && co < a.Cout)
      bv = float4{bf2f(a.bias[co]), bf2f(a.bias[co + 1]), bf2f(a.bias[co + 2]), bf2f(a.bias[co + 3])};
#pragma unroll 1
    for (int it = 0; it < BM / (16 * NW); ++it) {
      const int r = it * (16 * NW) + wave * 16 + (lane >> 2);
      const int py = r / a.pw, px = r - py * a.pw;
      const int y = y0 + py, x = x0 + px;
      const bool ok = py >= 1 && py <= a.ph - 2 && px >= 1 && px <= a.pw - 2 && y < a.H && x < a.W && co < a.Cout;
      if (!ok) continue;
      float4 o[2][2] = {{bv, bv}, {bv, bv}};
#pragma unroll
      for (int ny = -1; ny <= 1; ++ny)
#pragma unroll
        for (int nx = -1; nx <= 1; ++nx)
#pragma unroll
          for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
              const bool used = (nb(0, dy) == ny || nb(1, dy) == ny) && (nb(0, dx) == nx || nb(1, dx) == nx);
              if (!used) continue;
              const float4 v = T4[(r + ny * a.pw + nx) * (T_PITCH / 4) + (dy * 3 + dx) * (CG / 4) + cq];
#pragma unroll
              for (int oa = 0; oa < 2; ++oa)
#pragma unroll
                for (int ob = 0; ob < 2; ++ob)
                  if (nb(oa, dy) == ny && nb(ob, dx) == nx) {
                    o[oa][ob].x += v.x;
                    o[oa][ob].y += v.y;
                    o[oa][ob].z += v.z;
                    o[oa][ob].w += v.w;
                  }
            }
#pragma unroll
      for (int oa = 0; oa < 2; ++oa)
#pragma unroll
        for (int ob = 0; ob < 2; ++ob) {
          u16* dst = a.out + (((long long)n * Ho + 2 * y + oa) * Wo + 2 * x + ob) * a.Cout + co;
          *reinterpret_cast<uint2*>(dst) = pack4_bf16(o[oa][ob].x, o[oa][ob].y, o[oa][ob].z, o[oa][ob].w);
        }
    }
  }
}

// CGS_UPCONV_GROUP at load / cgs_upconv_set_tile_group: patches walked together by grouped_tile (A/B)
static int g_upconv_group = getenv("CGS_UPCONV_GROUP") ? atoi(getenv("CGS_UPCONV_GROUP")) : 16;
CGS_EXPORT void cgs_upconv_set_tile_group(int g) { g_upconv_group = g < 1 ? 1 : g; }

// x [N, H, W, Cin] NHWC bf16, wt [ceil(Cout / 16) * 144, Cin] tap-ordered weights (rows of channels past Cout are
// zeros), bias [Cout] | null, out [N, 2H, 2W, Cout]. Cin % 32 == 0, Cout % 8 == 0.
CGS_EXPORT int cgs_upconv_taps_nhwc(const void* x, const void* wt, const void* bias, void* out, int N, int H, int W,
                                    int Cin, int Cout, hipStream_t stream) {
  if (N < 1 || H < 1 || W < 1 || Cin < 32 || Cin % 32 || Cout < 8 || Cout % 8 || ((uintptr_t)out % 8) ||
      ((uintptr_t)x % 16) || ((uintptr_t)wt % 16))
    return (int)hipErrorInvalidValue;
  static const int shapes[4][2] = {{16, 16}, {18, 14}, {14, 18}, {34, 7}};
  UpconvArgs a{(const u16*)x, (const u16*)wt, (const u16*)bias, (u16*)out, N, H, W, Cin, Cout};
  long long best = -1;
  for (const auto& s : shapes) {
    const int txs = (W + s[0] - 3) / (s[0] - 2), tys = (H + s[1] - 3) / (s[1] - 2);
    const long long t = (long long)txs * tys;
    if (best < 0 || t < best) {
      best = t;
      a.pw = s[0];
      a.ph = s[1];
      a.tiles_x = txs;
      a.tiles_y = tys;
    }
  }
  a.groups16 = (Cout + uc::CG - 1) / uc::CG;
  a.groups = (a.groups16 + uc::NG - 1) / uc::NG;
  a.group_m = g_upconv_group < 1 ? 1 : g_upconv_group;
  const long long nwg = (long long)N * best * a.groups;
  if (nwg > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)upconv_taps_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, uc::LDS);
    attr = true;
  }
  upconv_taps_kernel<<<(unsigned)nwg, 64 * uc::NW, uc::LDS, stream>>>(a);
  return (int)hipGetLastError();
}
