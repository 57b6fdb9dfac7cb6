// Shared MFMA main loop for the v3 GEMM and implicit-GEMM conv kernels (gfx950 / CDNA4).
//
// Block tile 256 x BN x 32 (BN = 256 or 128), 4 waves in a 2x2 grid, each wave owns a
// 128 x BN/2 accumulator tile computed with v_mfma_f32_32x32x16_bf16 (4 x BN/64 MFMA tiles,
// 256 / 128 accumulator registers -> one wave per SIMD, up to 512 VGPRs).
//
// Operands stream global -> LDS with buffer-less LDS DMA (global_load_lds_dwordx4, 16 B / lane,
// 1 KiB = 16 rows x 64 B per wave-instruction) through a 4-stage ring (stage = 256x32 A + BNx32 B
// = 32 / 24 KiB): three k-steps are in flight while one is consumed, which covers HBM latency at
// one wave per SIMD. Rows are 64 B (4 x 16 B chunks); chunk c of row r is stored at chunk
// c ^ ((r >> 2) & 3), which makes every ds_read_b128 fragment read conflict-free for the CDNA4
// lane groups {0-3,12-15,20-27} / {4-11,16-19,28-31} (MI355X_MICROARCH.md, LDS table). The swizzle
// is applied on the global source address, because LDS DMA writes lane-linear.
//
// The A operand comes from a loader policy (dense rows for GEMM, NHWC pixel gather for conv);
// B is always K-contiguous rows (nn.Linear weight / [Cout][kh][kw][Cin] conv weight).
#pragma once
#include "common.h"
#include <type_traits>

typedef __attribute__((address_space(3))) void mc_lds_void;

#define MC_EPI_BIAS 1
#define MC_EPI_RESIDUAL 2
#define MC_EPI_GEGLU 4
#define MC_EPI_LNFOLD 8   // y = rstd_r * (acc - mean_r * cs[c]) + bias[c]  (LayerNorm folded into the GEMM)
#define MC_EPI_F32OUT 16  // v7 only: C is fp32 (ldc in floats), no GEGLU / residual (attention scores, K22)
#define MC_EPI_GELU 32    // GELU(acc * alpha + bias) before the residual (mc::tile, pq::run ACT, skinny; no GEGLU)
#define MC_EPI_F32RAW 64  // mc::tile only: the raw fp32 accumulators to (float*)C (ldc in floats), no other epilogue
                          // (split-K partial products, reduced + epilogued by cgs_gemm_bf16_splitk's second pass)

namespace mc {

// Compile-time loop: f(std::integral_constant<int, I>) for I in [0, N). Used where the body is
// too large for the unroller but the index must stay constant (register-resident accumulators).
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

constexpr int BM = 256;
constexpr int BK = 32;
constexpr int STAGES = 4;

// NW = waves per block: 4 (2x2 grid, one wave per SIMD, BMV/2 x BN/2 per wave) or 8 (2x4 grid, two
// waves per SIMD, BMV/2 x BN/4 per wave: the partner wave hides LDS latency, barriers and VMEM issue).
// BMV = tile rows: 256, or 128 for the small-M "v8" form (128 x 128 tiles, 64 KiB of LDS -> two
// workgroups per CU: 4x the tiles of a 256 x 256 grid where M or N is short -- SDXL at batch 1,
// Cascade's 24^2 / 32^2 token grids -- and one workgroup's epilogue overlaps the other's main loop).
// NS: LDS ring depth (stages); NS - 2 k-steps are in flight while one is consumed. The small-tile
// GEMMs use 5-6 (two workgroups per CU still fit) to cover L2 latency with few waves per CU.
template <int BN, int NW = 4, int BMV = BM, int NS = STAGES>
struct Cfg {
  static constexpr int THREADS = 64 * NW;
  static constexpr int WCOLS = NW / 2;                  // wave grid is 2 x WCOLS
  static constexpr int TM = BMV;                        // tile rows
  static constexpr int WROWS = BMV / 2;                 // wave tile rows
  static constexpr int A_BYTES = BMV * BK * 2;          // 16 KiB at 256 rows
  static constexpr int B_BYTES = BN * BK * 2;
  static constexpr int STAGE = A_BYTES + B_BYTES;
  static constexpr int LDS = NS * STAGE;
  static constexpr int A_PIECES = BMV / 16 / NW;        // LDS-DMA pieces (16 rows) per wave
  static constexpr int B_PIECES = BN / 16 / NW;
  static constexpr int PER_STAGE = A_PIECES + B_PIECES; // LDS-DMA instructions per wave per stage
  static constexpr int WN = BN / WCOLS;                 // wave tile cols
  static constexpr int NI = WROWS / 32;                 // 32-row MFMA tiles per wave
  static constexpr int NJ = WN / 32;                    // 32-col MFMA tiles per wave
  static_assert(A_PIECES >= 1 && B_PIECES >= 1 && NJ >= 1 && NI >= 1, "tile too narrow for this wave count");
  static_assert(NW * WROWS * WN * 2 <= LDS, "epilogue regions must fit the stage ring");
};

struct Epi {
  u16* C;
  const u16* bias;
  const u16* R;
  long long ldc, ldr;
  int flags;
  float alpha;
  const float* rs = nullptr;   // MC_EPI_LNFOLD: per-row (mean, rstd) pairs of the GEMM's A rows
  const float* cs = nullptr;   // MC_EPI_LNFOLD: per-column sums of the gamma-scaled weight rows
  float* gnp = nullptr;        // GroupNorm statistics out (pq::run GNS): per-(image, 64-row block, column)
  int hw = 0;                  //   (mean, M2) partials in the gn_partial layout; hw = rows per image
  int act = 0;                 // MC_EPI_GELU: the CgsAct code applied instead of the erf GELU (0 / CGS_ACT_GELU: erf)
  float act_param = 0.f;       //   its parameter (the leaky_relu slope)
};

// s_waitcnt with only vmcnt constrained (gfx9 encoding: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt_hi[15:14])
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 0xF) | (0x7 << 4) | (0xF << 8) | ((N >> 4) << 14));
}

// A loader that issues its own LDS DMA (``static constexpr bool kOwnDMA``; ``tile(m0)`` at each output tile,
// ``dma(slot, k0, dst)`` per K-tile -- conv.hip ConvGatherKD's buffer_load ... lds) instead of handing the
// main loop a global source address (``src(slot, k0)``).
template <class T, class = void>
struct own_dma : std::false_type {};
template <class T>
struct own_dma<T, std::void_t<decltype(T::kOwnDMA)>> : std::true_type {};

__device__ __forceinline__ void lds_dma16(const void* src, unsigned char* dst) {
  __builtin_amdgcn_global_load_lds(src, (mc_lds_void*)dst, 16, 0, 0);
}

// Lane -> (row in 16-row piece, source chunk) for the loaders.
__device__ __forceinline__ int piece_row(int lane) { return lane >> 2; }
__device__ __forceinline__ int src_chunk(int lane) { return (lane & 3) ^ ((lane >> 4) & 3); }

// Main loop + epilogue for one 256 x BN output tile.
//   AL: loader with  __device__ void setup(int p, int row)  (p = this wave's A piece 0..3, row =
//       global output row, may be >= M) and  __device__ const void* src(int p, int k0) const.
template <int BN, int NW, class AL, int BMV = BM, int NS = STAGES>
__device__ __forceinline__ void tile(AL& al, const u16* __restrict__ W, long long ldw, int M, int N, int K, int m0,
                                     int n0, const Epi& e, unsigned char* smem) {
  using C = Cfg<BN, NW, BMV, NS>;
  static_assert(NS >= 4, "ring depth");
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = (wave / C::WCOLS) * C::WROWS;
  const int wn = (wave % C::WCOLS) * C::WN;
  const int prow = piece_row(lane);
  const int sch = src_chunk(lane);

#pragma unroll
  for (int p = 0; p < C::A_PIECES; ++p) al.setup(p, m0 + (wave * C::A_PIECES + p) * 16 + prow);
  const u16* bsrc[C::B_PIECES];
#pragma unroll
  for (int p = 0; p < C::B_PIECES; ++p) {
    int r = n0 + (wave * C::B_PIECES + p) * 16 + prow;
    r = r < N ? r : N - 1;
    bsrc[p] = W + (long long)r * ldw + 8 * sch;
  }

  const int nk = K / BK;
  auto issue = [&](int kt, int slot) {
    unsigned char* base = smem + slot * C::STAGE;
    const int k0 = (kt < nk ? kt : nk - 1) * BK;   // past the end: harmless reload into a dead slot
#pragma unroll
    for (int p = 0; p < C::A_PIECES; ++p) lds_dma16(al.src(p, k0), base + (wave * C::A_PIECES + p) * 1024);
#pragma unroll
    for (int p = 0; p < C::B_PIECES; ++p)
      lds_dma16((const void*)(bsrc[p] + k0), base + C::A_BYTES + (wave * C::B_PIECES + p) * 1024);
  };

  f32x16 acc[C::NI][C::NJ];
#pragma unroll
  for (int i = 0; i < C::NI; ++i)
#pragma unroll
    for (int j = 0; j < C::NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment addressing: row r = base + (lane & 31), logical chunk c = 2*kk + (lane >> 5)
  const int frow = lane & 31;
  const int fswz = (lane >> 2) & 3;       // ((r >> 2) & 3) for r = 32*i + frow
  const int fhalf = lane >> 5;

  auto read_frags = [&](int slot, int kk, bf16x8 (&a)[C::NI], bf16x8 (&b)[C::NJ]) {
    const unsigned char* As = smem + slot * C::STAGE;
    const unsigned char* Bs = As + C::A_BYTES;
    const int c = (2 * kk + fhalf) ^ fswz;
#pragma unroll
    for (int i = 0; i < C::NI; ++i) a[i] = *reinterpret_cast<const bf16x8*>(As + (wm + 32 * i + frow) * 64 + 16 * c);
#pragma unroll
    for (int j = 0; j < C::NJ; ++j) b[j] = *reinterpret_cast<const bf16x8*>(Bs + (wn + 32 * j + frow) * 64 + 16 * c);
  };
  auto mma = [&](const bf16x8 (&a)[C::NI], const bf16x8 (&b)[C::NJ]) {
#pragma unroll
    for (int i = 0; i < C::NI; ++i)
#pragma unroll
      for (int j = 0; j < C::NJ; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
  };
  // Pin the interleave (the scheduler otherwise sinks every ds_read to its use and stalls on each
  // one): after MFMA q of a phase, issue its share of the R fragment reads and V LDS-DMA loads.
  auto pin_schedule = [&](auto vmem_c) {
    constexpr int V = decltype(vmem_c)::value;
    constexpr int R = C::NI + C::NJ, Q = C::NI * C::NJ;
    static_for<0, Q>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      constexpr int nds = ((q + 1) * R) / Q - (q * R) / Q;
      constexpr int nvm = ((q + 1) * V) / Q - (q * V) / Q;
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);              // MFMA
      if constexpr (nds > 0) __builtin_amdgcn_sched_group_barrier(0x100, nds, 0);  // DS read
      if constexpr (nvm > 0) __builtin_amdgcn_sched_group_barrier(0x010, nvm, 0);  // VMEM (LDS DMA)
    });
  };

  // Pipeline (4-slot ring, stage s DMA'd during iteration s-3): iteration kt computes k-slice 0 of
  // stage kt while reading slice 1; then waits for its own DMAs of stage kt+1 (vmcnt: exactly one
  // younger stage may stay in flight) and the block barrier (everyone's DMAs landed, everyone done
  // with slot kt-1); then computes slice 1 while DMA-ing stage kt+3 into slot kt-1 and reading
  // slice 0 of stage kt+1. No fence, so younger stages stay in flight across the barrier; every
  // iteration issues one stage (clamped past the end) so the body is one basic block and the vmcnt
  // count is a constant.
  bf16x8 a0[C::NI], b0[C::NJ], a1[C::NI], b1[C::NJ];
#pragma unroll
  for (int st = 0; st < NS - 1; ++st) issue(st, st);
  wait_vmcnt<(NS - 2) * C::PER_STAGE>();
  __builtin_amdgcn_s_barrier();
  read_frags(0, 0, a0, b0);

  // slots: cur = kt % NS (consumed), nxt = (kt + 1) % NS, iss = (kt + NS - 1) % NS (= slot of kt - 1)
  int cur = 0, nxt = 1 % NS, iss = NS - 1;
  for (int kt = 0; kt < nk; ++kt) {
    mma(a0, b0);
    read_frags(cur, 1, a1, b1);
    pin_schedule(std::integral_constant<int, 0>{});
    wait_vmcnt<(NS - 3) * C::PER_STAGE>();
    __builtin_amdgcn_s_barrier();
    mma(a1, b1);
    issue(kt + NS - 1, iss);
    read_frags(nxt, 0, a0, b0);
    pin_schedule(std::integral_constant<int, C::PER_STAGE>{});
    cur = nxt;
    nxt = nxt + 1 == NS ? 0 : nxt + 1;
    iss = iss + 1 == NS ? 0 : iss + 1;
  }

  // ---- epilogue, staged through LDS so global traffic is 16-B vectors.
  // 32x32 C layout: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).
  // Each wave owns a WROWS x OW bf16 region (OW = WN, or WN/2 for GEGLU); 16-B chunk ch of row r is
  // stored at ch ^ (r & (CPR - 1)) so the column-wise fragment writes and row-wise reads are
  // conflict-free without padding (the 4 regions fill exactly the 4-stage ring).
  wait_vmcnt<0>();   // the clamped tail DMAs target slots the epilogue reuses
  if (e.flags & MC_EPI_F32RAW) {   // split-K partials: straight from the registers, 32 lanes = 128-B runs
    float* Cf = reinterpret_cast<float*>(e.C);
    const int erow0 = 4 * (lane >> 5);
#pragma unroll
    for (int j = 0; j < C::NJ; ++j) {
      const int col = n0 + wn + 32 * j + (lane & 31);
#pragma unroll
      for (int i = 0; i < C::NI; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + erow0;
          if (row < M && col < N) Cf[(long long)row * e.ldc + col] = acc[i][j][r];
        }
    }
    return;
  }
  __syncthreads();   // other waves may still be reading the last stage
  const bool geglu = (e.flags & MC_EPI_GEGLU) != 0;
  const int OW = geglu ? C::WN / 2 : C::WN;
  const int CPR = OW / 8;               // 16-B chunks per row
  const int pitch = OW * 2;
  unsigned char* region = smem + wave * (C::WROWS * C::WN * 2);
  const int ecol = lane & 31;
  const int erow = 4 * fhalf;
  // MC_EPI_LNFOLD (LayerNorm folded in, alpha = 1): v = rstd_row * (acc - mean_row * cs[col]); the
  // (mean, rstd) pair of each output row comes from e.rs (rows clamped to M - 1)
  const bool lnf = (e.flags & MC_EPI_LNFOLD) != 0;
  auto ln_row = [&](int lrow) {
    int grow = m0 + wm + lrow;
    grow = grow < M ? grow : M - 1;
    return *reinterpret_cast<const float2*>(e.rs + 2 * (long long)grow);
  };
  if (geglu) {
    // weight rows interleaved in 16-row groups [a0..a15, g0..g15, ...]: within a 32-col MFMA tile,
    // lanes 0-15 hold 'a' and lanes 16-31 the matching 'g'; out col = tile col0 / 2 + (lane & 15).
    static_for<0, C::NJ>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      const int col0 = n0 + wn + 32 * j;
      const int ca = col0 + (ecol & 15);
      float ba = 0.f, bg = 0.f;
      if ((e.flags & MC_EPI_BIAS) && col0 < N) { ba = bf2f(e.bias[ca]); bg = bf2f(e.bias[ca + 16]); }
      const float csl = (lnf && col0 < N) ? e.cs[col0 + ecol] : 0.f;   // this lane's own column (a or g)
      const int oc = 16 * j + (ecol & 15);   // col within the wave's output region
      static_for<0, C::NI>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const f32x16 t = acc[i][j];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = t[r] * e.alpha;
          if (lnf) {
            const float2 st = ln_row(32 * i + (r & 3) + 8 * (r >> 2) + erow);
            v = st.y * (t[r] - st.x * csl);
          }
          float other = __shfl_xor(v, 16, 64);
          int row = 32 * i + (r & 3) + 8 * (r >> 2) + erow;
          if ((ecol & 16) == 0) {
            float gl = other + bg;
            *reinterpret_cast<u16*>(region + row * pitch + 16 * ((oc >> 3) ^ (row & (CPR - 1))) + 2 * (oc & 7)) =
                f2bf((v + ba) * gelu_sig(gl));
          }
        }
      });
    });
  } else {
    // plain / GELU (MC_EPI_GELU) / other activation (MC_EPI_GELU + e.act) forms as straight-line paths: the
    // flag and the code are wave-uniform
    const ActFam af = act_family(e.act, e.act_param);   // (e.act 0 / CGS_ACT_GELU: the erf path below)
    auto plain = [&](auto act_c) {
      constexpr int ACT = decltype(act_c)::value;
#pragma unroll
      for (int j = 0; j < C::NJ; ++j) {
        const int oc = 32 * j + ecol;
        const int col = n0 + wn + oc;
        const float bv = ((e.flags & MC_EPI_BIAS) && col < N) ? bf2f(e.bias[col]) : 0.f;
        const float csl = (lnf && col < N) ? e.cs[col] : 0.f;
#pragma unroll
        for (int i = 0; i < C::NI; ++i) {
          const f32x16 t = acc[i][j];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            int row = 32 * i + (r & 3) + 8 * (r >> 2) + erow;
            float v = t[r] * e.alpha;
            if (lnf) {
              const float2 st = ln_row(row);
              v = st.y * (t[r] - st.x * csl);
            }
            v += bv;
            if constexpr (ACT == ACT_FAM_ERF) v = gelu_sig(v);
            else if constexpr (ACT != ACT_FAM_NONE) v = act_fam<ACT>(v, af.a, af.b);
            *reinterpret_cast<u16*>(region + row * pitch + 16 * ((oc >> 3) ^ (row & (CPR - 1))) + 2 * (oc & 7)) =
                f2bf(v);
          }
        }
      }
    };
    if (!(e.flags & MC_EPI_GELU)) plain(std::integral_constant<int, ACT_FAM_NONE>{});
    else if (af.fam == ACT_FAM_SIG) plain(std::integral_constant<int, ACT_FAM_SIG>{});
    else if (af.fam == ACT_FAM_LIN) plain(std::integral_constant<int, ACT_FAM_LIN>{});
    else plain(std::integral_constant<int, ACT_FAM_ERF>{});
  }
  // wave-local region: only this wave's LDS writes must land before its reads (lgkmcnt wait is
  // inserted by the compiler); then 16-B row-wise reads -> (+ residual) -> 16-B global stores.
  const int rows_per_it = 64 / CPR;
  const int gcol0 = geglu ? (n0 + wn) / 2 : n0 + wn;
  const int Nout = geglu ? N / 2 : N;
  const int ch = lane % CPR;
  for (int rr = lane / CPR; rr < C::WROWS; rr += rows_per_it) {
    const int grow = m0 + wm + rr;
    const int gcol = gcol0 + 8 * ch;
    s16x8 v = *reinterpret_cast<const s16x8*>(region + rr * pitch + 16 * (ch ^ (rr & (CPR - 1))));
    if (grow < M && gcol < Nout) {
      if (e.flags & MC_EPI_RESIDUAL) {
        s16x8 rv = *reinterpret_cast<const s16x8*>(e.R + (long long)grow * e.ldr + gcol);
#pragma unroll
        for (int t = 0; t < 8; ++t) v[t] = (short)f2bf(bf2f((u16)v[t]) + bf2f((u16)rv[t]));
      }
      *reinterpret_cast<s16x8*>(e.C + (long long)grow * e.ldc + gcol) = v;
    }
  }
}

// Pick BN for an M x N problem: fewest (rounds of 256 CUs) x (tile width) -- i.e. least tail
// waste; ties go to the wider tile (less operand traffic per flop).
inline int pick_bn(int M, int N) {
  long long tm = (M + BM - 1) / BM;
  long long t256 = tm * ((N + 255) / 256), t128 = tm * ((N + 127) / 128);
  long long c256 = ((t256 + 255) / 256) * 256, c128 = ((t128 + 255) / 256) * 128;
  return c128 < c256 ? 128 : 256;
}

}  // namespace mc
