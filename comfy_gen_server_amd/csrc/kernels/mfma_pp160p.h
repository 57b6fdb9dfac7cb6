// Patch form of the 256 x 160 ping-pong main loop ("v6p") for the 3 x 3 / stride 1 / pad 1 conv.
//
// The v6 conv (mfma_pp160.h with ConvGatherKD) orders K as (tap, channel) and DMAs the 256 source rows of its
// tile again for every tap: each input pixel of a tile crosses L2 -> LDS nine times, shifted by one pixel.
// Here the 256 tile rows are one 16 x 16 output patch of one image, K is ordered (64-channel slab, tap), and
// the 18 x 18 input patch of a slab (324 pixels x 128 B) is staged once; the nine taps read it at shifted LDS
// addresses. Per tile and slab: 41 A pieces of 1 KiB instead of 9 x 32, the B pieces (9 x 20) unchanged.
//
// Geometry, accumulators, MFMA order and the B staging are v6's (pq::Geo<5>): 8 waves, wave (wm, grp) owns 64
// rows x 80 columns, group 1 one barrier behind group 0. MFMA row block i of wave wm is patch row 4 wm + i,
// x = 0..15 (lane & 15).
//
// LDS (159,744 B): two patch buffers of 48 KiB and a ring of three 20 KiB B stages, one per (slab, tap) step.
//   A patch pixel p = py * 18 + px sits at p * 128, its 16-B chunk c at position c ^ (p & 7) (applied on the
//   DMA source chunk). Tap (ky, kx), row block i reads pixels p = (4 wm + i + ky) * 18 + kx + fr, fr = 0..15:
//   a run of 16 consecutive pixels from any start. ds_read_b128 serves 8 lanes per pass over the 64 banks, so 8
//   consecutive pixels must land in 8 distinct 16-B columns: with p & 7 they do for every start offset and both
//   K halves (8 consecutive p have 8 distinct p & 7, and x ^ const is a bijection); v6's (row >> 1) & 7 gives
//   only 4-5 distinct values over 8 consecutive pixels once kx shifts the run, i.e. 2-way conflicts.
//   Each buffer is 48 pieces, not 41: all 8 waves issue 6 pieces per slab, so the counted vmcnt waits are the
//   same in every wave; pieces past pixel 323 carry out-of-range offsets (zeros, no L2 traffic).
//   Pixels outside the image get offset bit 31 (past the per-image descriptor's range): the DMA writes zeros.
//
// Schedule per step (slab s, tap t), two phases (k 0..31, 32..63) like a v6 K-tile:
//   phase 0: fragment reads; DMA B piece 0 of step + 2 and, for t = 1..6, A piece t - 1 of the next slab's patch
//   phase 1: fragment reads; DMA B pieces 1, 2 of step + 2; counted wait: only this step's DMAs stay in flight.
// The stream runs across units: the last slab of a unit stages the next unit's first patch and its last two
// steps the next unit's first two B stages; the register epilogue runs with those in flight.
#pragma once
#include "mfma_pp160.h"

namespace pq {

constexpr int PATCH = 16, PATCH_W = PATCH + 2, PATCH_PIX = PATCH_W * PATCH_W;   // 18 x 18 = 324 input pixels
constexpr int PA_ROUNDS = 6;                           // A pieces per wave and slab (48 >= 40.5)
constexpr int PA_BYTES = PA_ROUNDS * 8 * 1024;         // one patch buffer
constexpr int PB_BYTES = Geo<5>::B_BYTES;
constexpr int P_LDS = 2 * PA_BYTES + 3 * PB_BYTES;

struct PatchUnit {
  int n, y0, x0, n0, pi;   // image, patch origin, first column, patch index in the image
};

// X [NB][H][Wd][Cin] bf16, Wt [N][3][3][Cin]; Cin % 64 == 0, N % 8 == 0, H * Wd * Cin * 2 < 2 GiB.
// GNS: GroupNorm partials (mean, M2) of the stored outputs per (image, block patch * 4 + wm, column): 64 pixels
// per block, every block written once (host: H % 16 == 0, Wd % 16 == 0).
template <bool GNS>
__device__ __forceinline__ void run_patch(const u16* __restrict__ X, int NB, int H, int Wd, int Cin,
                                          const u16* __restrict__ Wt, int N, const mc::Epi& e, unsigned char* smem,
                                          int tiles_n) {
  using Gm = Geo<5>;
  constexpr int NI = 4, NJ = 5, GW = Gm::GW, BN = Gm::BN;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2;
  const int wm = wave & 3;
  const int nslab = Cin / 64;
  const long long ldw = 9ll * Cin;
  const int tiles_x = (Wd + PATCH - 1) / PATCH, tiles_y = (H + PATCH - 1) / PATCH;
  const int ppi = tiles_x * tiles_y;
  const int T = NB * ppi * tiles_n;
  const int G = gridDim.x;
  const int base_l = xcd_remap(blockIdx.x, G);
  if (base_l >= T) return;

  auto decode = [&](int l) {
    PatchUnit u;
    const int pg = l / tiles_n;
    u.n0 = (l - pg * tiles_n) * BN;
    u.n = pg / ppi;
    u.pi = pg - u.n * ppi;
    const int ty = u.pi / tiles_x;
    u.y0 = ty * PATCH;
    u.x0 = (u.pi - ty * tiles_x) * PATCH;
    return u;
  };

  unsigned char* const SA = smem;
  unsigned char* const SB = smem + 2 * PA_BYTES;

  // ---- A: the lane's six patch DMAs (pixel p = d >> 3, LDS chunk position d & 7, d = piece * 64 + lane)
  uint32_t voff[PA_ROUNDS];
  __amdgpu_buffer_rsrc_t ra;
  auto a_setup = [&](const PatchUnit& u) {
    ra = __builtin_amdgcn_make_buffer_rsrc((void*)(X + (long long)u.n * H * Wd * Cin), 0, H * Wd * Cin * 2, 0x00020000);
#pragma unroll
    for (int r = 0; r < PA_ROUNDS; ++r) {
      const int d = (r * 8 + wave) * 64 + lane;
      const int p = d >> 3, c = d & 7;
      const int py = p / PATCH_W, px = p - py * PATCH_W;
      const int iy = u.y0 - 1 + py, ix = u.x0 - 1 + px;
      const bool ok = p < PATCH_PIX && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)Wd;
      voff[r] = ok ? (uint32_t)(((iy * Wd + ix) * Cin + 8 * (c ^ (p & 7))) * 2) : 0x80000000u;
    }
  };
  auto dma_a = [&](int r, int slab, int buf) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (mc_lds_void*)(SA + buf * PA_BYTES + (r * 8 + wave) * 1024), 16,
                                             voff[r], slab * 128, 0, 0);
  };

  // ---- B: v6's staging (b_col160 rows, chunk c at c ^ ((row >> 1) & 7)); piece 2 by waves 0..3 only
  const int lrow = tid >> 3, lch = tid & 7;
  const u16* bsrc[3];
  auto b_setup = [&](int n0) {
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const int r = g * 64 + lrow;
      int n = n0 + b_col160<5>(r < BN ? r : BN - 1);
      n = n < N ? n : N - 1;
      bsrc[g] = Wt + (long long)n * ldw + 8 * (lch ^ ((r >> 1) & 7));
    }
  };
  auto dma_b = [&](int g, int tap, int slab, int slot) {
    if (g == 2 && wave >= 4) return;
    mc::lds_dma16((const void*)(bsrc[g] + tap * Cin + slab * 64), SB + slot * PB_BYTES + wave * 1024 + g * 8192);
  };
  // all but the DMAs of the current step retired: its B pieces (3 in waves 0..3, 2 in 4..7) + A of them
  auto wait_step = [&](auto ac) {
    constexpr int A = decltype(ac)::value;
    if (wave < 4) mc::wait_vmcnt<3 + A>();
    else mc::wait_vmcnt<2 + A>();
  };

  f32x4 acc[NI][NJ];
  const int fr = lane & 15, fq = lane >> 4;
  bf16x8 af[NI], bfr[NJ];
  // Fragment addresses. A: pixel p = pbase + c with c = i * 18 + ky * 18 + kx a constant of the unrolled step;
  // p & 7 depends on c & 7 only, so 8 x 2 (K half) lane offsets serve every (tap, i): offset abase[c & 7][kk] +
  // (c >> 3) * 1024 (the constant part rides in the ds_read offset field). B: (r >> 1) & 7 = (fr >> 1) for every
  // column tile and group (16 j and 80 grp are multiples of 16), so two lane offsets and constants.
  const int pbase = 4 * wm * PATCH_W + fr;
  int abase[8][2], bbase[2];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) abase[m][kk] = (pbase + m) * 128 + 16 * ((4 * kk + fq) ^ ((pbase + m) & 7));
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
    bbase[kk] = 2 * PA_BYTES + (grp * GW + fr) * 128 + 16 * ((4 * kk + fq) ^ (fr >> 1));
  auto read_frags = [&](int aoff, auto tapc, auto slotc, auto kkc) {   // aoff: byte offset of the patch buffer
    constexpr int tapoff = decltype(tapc)::value, slot = decltype(slotc)::value, kk = decltype(kkc)::value;
    mc::static_for<0, NI>([&](auto ic) {
      constexpr int i = decltype(ic)::value, c = i * PATCH_W + tapoff;
      af[i] = *reinterpret_cast<const bf16x8*>(smem + (aoff + abase[c & 7][kk]) + (c >> 3) * 1024);
    });
    mc::static_for<0, NJ>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      bfr[j] = *reinterpret_cast<const bf16x8*>(smem + bbase[kk] + (slot * PB_BYTES + j * 2048));
    });
  };
  auto mma = [&]() {   // C^T tiles as in pq::run: lane (fr, fq) accumulates C[16i + fr][16j + 4fq + 0..3]
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };

  // ---- epilogue: pq::run's register epilogue (bias / residual / GroupNorm partials) with tile row 16 ib + fr of
  // wave wm -> pixel (y0 + 4 wm + ib, x0 + fr); rows outside the image are idle
  auto colj = [&](int j) { return j < 4 ? 32 * (j >> 1) + 8 * fq + 4 * (j & 1) : 64 + 4 * fq; };
  auto epilogue_t = [&](const PatchUnit& u, auto has_bias_c, auto has_res_c) {
    constexpr bool HB = decltype(has_bias_c)::value, HR = decltype(has_res_c)::value;
    const int n_w = u.n0 + grp * GW;
    const int x = u.x0 + fr, yw = u.y0 + 4 * wm;
    const long long img_row = (long long)u.n * H * Wd;
    auto row_of = [&](int ib, long long& row) {
      const int y = yw + ib;
      row = img_row + (long long)y * Wd + x;
      return y < H && x < Wd;
    };
    float4 bv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      int col = n_w + colj(j);
      col = col < N ? col : N - 4;
      bv[j] = HB ? unpack4_bf16(*reinterpret_cast<const uint2*>(e.bias + col)) : float4{0.f, 0.f, 0.f, 0.f};
    }
    uint2 rw[NI][NJ];   // residual words
    if (HR) {
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        long long row;
        if (!row_of(i, row)) row = img_row;
        const u16* rrow = e.R + row * e.ldr;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          int col = n_w + 32 * p + 8 * fq;
          col = col < N ? col : N - 8;
          const uint4 w4 = *reinterpret_cast<const uint4*>(rrow + col);
          rw[i][2 * p] = uint2{w4.x, w4.y};
          rw[i][2 * p + 1] = uint2{w4.z, w4.w};
        }
        int col = n_w + 64 + 4 * fq;
        col = col < N ? col : N - 4;
        rw[i][4] = *reinterpret_cast<const uint2*>(rrow + col);
      }
    }
    uint2 pk[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        float v0 = acc[i][j][0] * e.alpha + bv[j].x, v1 = acc[i][j][1] * e.alpha + bv[j].y;
        float v2 = acc[i][j][2] * e.alpha + bv[j].z, v3 = acc[i][j][3] * e.alpha + bv[j].w;
        if (HR) {
          const float4 rv = unpack4_bf16(rw[i][j]);
          v0 += rv.x; v1 += rv.y; v2 += rv.z; v3 += rv.w;
        }
        pk[i][j] = pack4_bf16(v0, v1, v2, v3);
      }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      long long row;
      const bool ok = row_of(i, row);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int col = n_w + 32 * p + 8 * fq;
        if (ok && col < N)
          *reinterpret_cast<uint4*>(e.C + row * e.ldc + col) =
              uint4{pk[i][2 * p].x, pk[i][2 * p].y, pk[i][2 * p + 1].x, pk[i][2 * p + 1].y};
      }
    }
    // column tile 4: row blocks i / i + 1 paired with v_permlane16_swap -> 16-B stores (pq::run store_t4)
#pragma unroll
    for (int i = 0; i < NI; i += 2) {
      const auto rx = __builtin_amdgcn_permlane16_swap(pk[i][4].x, pk[i + 1][4].x, false, false);
      const auto ry = __builtin_amdgcn_permlane16_swap(pk[i][4].y, pk[i + 1][4].y, false, false);
      long long row;
      const bool ok = row_of(i + (fq & 1), row);
      const int col = n_w + 64 + 8 * (fq >> 1);
      if (ok && col < N) *reinterpret_cast<uint4*>(e.C + row * e.ldc + col) = uint4{rx[0], ry[0], rx[1], ry[1]};
    }
    if constexpr (GNS) {
      const int nbk = (H * Wd) >> 6;
      float* dst = e.gnp + (size_t)(u.n * nbk + u.pi * 4 + wm) * N * 2;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        float4 v[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) v[i] = unpack4_bf16(pk[i][j]);
        float4 mu = v[0];
#pragma unroll
        for (int i = 1; i < NI; ++i) { mu.x += v[i].x; mu.y += v[i].y; mu.z += v[i].z; mu.w += v[i].w; }
        constexpr float inv = 1.f / 64.f;
        mu = float4{row16_sum(mu.x) * inv, row16_sum(mu.y) * inv, row16_sum(mu.z) * inv, row16_sum(mu.w) * inv};
        float4 q = float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const float dx = v[i].x - mu.x, dy = v[i].y - mu.y, dz = v[i].z - mu.z, dw = v[i].w - mu.w;
          q.x += dx * dx; q.y += dy * dy; q.z += dz * dz; q.w += dw * dw;
        }
        q = float4{row16_sum(q.x), row16_sum(q.y), row16_sum(q.z), row16_sum(q.w)};
        const int col = n_w + colj(j);
        if (fr == 0 && col < N) {
          float4* d4 = reinterpret_cast<float4*>(dst + (size_t)col * 2);
          d4[0] = float4{mu.x, q.x, mu.y, q.y};
          d4[1] = float4{mu.z, q.z, mu.w, q.w};
        }
      }
    }
  };
  using T0 = std::false_type;
  using T1 = std::true_type;
  const bool hb = (e.flags & MC_EPI_BIAS) != 0, hr = (e.flags & MC_EPI_RESIDUAL) != 0;
  auto epilogue = [&](const PatchUnit& u) {
    if (hr) {
      if (hb) epilogue_t(u, T1{}, T1{});
      else epilogue_t(u, T0{}, T1{});
    } else {
      if (hb) epilogue_t(u, T1{}, T0{});
      else epilogue_t(u, T0{}, T0{});
    }
  };

  int l = base_l;
  PatchUnit u = decode(l);
  a_setup(u);
  b_setup(u.n0);
#pragma unroll
  for (int r = 0; r < PA_ROUNDS; ++r) dma_a(r, 0, 0);
#pragma unroll
  for (int g = 0; g < 3; ++g) dma_b(g, 0, 0, 0);
#pragma unroll
  for (int g = 0; g < 3; ++g) dma_b(g, 1, 0, 1);
  wait_step(std::integral_constant<int, 0>{});   // the patch and step 0 landed; step 1 in flight
  pp::barrier();
  if (grp == 1) pp::barrier();   // stagger: group 1 runs one segment behind group 0

  int abuf = 0;                  // patch buffer of the slab being consumed
  while (true) {
    const int ln = l + G;
    const bool has_next = ln < T;
    const PatchUnit nu = has_next ? decode(ln) : u;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < nslab; ++s) {
      const bool last = s == nslab - 1;
      // the unit's patches are all staged: its last slab stages the next unit's first (past the last unit: this
      // unit's first again, into the dead buffer -- keeps the vmcnt pattern)
      if (last && has_next) a_setup(nu);
      const int sn = last ? 0 : s + 1;
      const int aoff = abuf * PA_BYTES;
      mc::static_for<0, 9>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        constexpr int tapoff = (t / 3) * PATCH_W + t % 3;
        constexpr int t2 = (t + 2) % 9, slot2 = (t + 2) % 3;
        constexpr bool AR = t >= 1 && t <= PA_ROUNDS;
        const int s2 = t + 2 < 9 ? s : sn;
        if constexpr (t == 7) {
          if (last && has_next) b_setup(nu.n0);   // steps 7, 8 stage the next unit's steps 0, 1
        }
        using Tap = std::integral_constant<int, tapoff>;
        using Slot = std::integral_constant<int, t % 3>;
        // phase 0 (not drained before the barrier: the MFMAs wait for their fragments one by one)
        read_frags(aoff, Tap{}, Slot{}, std::integral_constant<int, 0>{});
        dma_b(0, t2, s2, slot2);
        if constexpr (AR) dma_a(t - 1, sn, abuf ^ 1);
        pp::barrier();
        mma();
        pp::barrier();
        // phase 1
        read_frags(aoff, Tap{}, Slot{}, std::integral_constant<int, 1>{});
        dma_b(1, t2, s2, slot2);
        dma_b(2, t2, s2, slot2);
        wait_step(std::integral_constant<int, AR ? 1 : 0>{});
        pp::wait_lgkm0();
        pp::barrier();
        mma();
        pp::barrier();
      });
      abuf ^= 1;
    }
    epilogue(u);
    if (!has_next) break;
    l = ln;
    u = nu;
  }
  if (grp == 0) pp::barrier();   // balance the stagger
  mc::wait_vmcnt<0>();           // the trailing dummy DMAs must land before the LDS is released
}

}  // namespace pq
