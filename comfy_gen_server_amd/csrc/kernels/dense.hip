// K09/K10 (slice form): 3 x 3 / stride 1 / pad 1 bf16 conv whose input is the first Cin channels of each pixel of a
// wider NHWC buffer and whose output is Cout = 16 .. 64 channels of each pixel of the same or of another buffer.
// A dense block (ESRGAN's ResidualDenseBlock5C) keeps one [N, H, W, nf + 4 gc] feature buffer: conv i reads the
// prefix [0, nf + (i - 1) gc) and writes its gc outputs right behind it, so nothing is concatenated, and the
// block's / the RRDB's scale-and-add is the epilogue of conv5:
//
//   out = alpha * act(conv(x) + bias) + beta * res + res2          fp32, one rounding to bf16 at the store
//
// Every operand carries its own base pointer (the channel offset folded in), pixel pitch and image stride, in
// elements; all offsets are 64-bit.
//
// Geometry of conv_nhwc_smalln_lds_kernel (conv.hip): a workgroup of 4 waves owns a 16 x 16 output patch of one
// image, wave w its pixel rows 4 w .. 4 w + 3; each 32-channel chunk of the 18 x 18 input halo is staged through
// LDS once (register-staged, double-buffered: the next chunk's global loads are in flight while this one
// computes; taps outside the image are staged as zeros). New here: NB = Cout / 16 MFMAs per fragment read from
// LDS, and the MFMA's operands swapped -- the weights are A (16 output channels on the rows), the 16 pixels of a
// row are B (on the columns) -- so a lane's four accumulator registers are four CHANNELS of one pixel. MFMA row
// 4 fq + q of block nb is given output channel 4 NB fq + 4 nb + q, so that a lane ends up with the 4 NB
// consecutive channels 4 NB fq .. 4 NB fq + 4 NB - 1 of its pixel: residual loads and output stores are 8-byte
// (NB odd) or 16-byte (NB even) vectors. The weight fragments come from global / L1 (every workgroup reads the
// same 18 NB KiB per chunk).
//
// LDS image: 80 B per staged pixel (32 channels + 16 B pad), as in conv.hip. A ds_read_b128 is served in four
// fixed groups of 16 lanes that mix two fq values (lanes 0-3, 12-15, 20-27, ...), and with one pixel per lane no
// pixel stride makes all 16 slots of such a group distinct (the fq = 1 lanes would have to sit a multiple of 16
// slots from the fq = 0 ones); 80 B leaves three 2-way conflicts per group. docs/OPEN_ITEMS.md has what is left.
#include "common.h"
#include <stdint.h>

#define DS_PX 40   // u16 per staged pixel: 32 channels + 8 pad

struct SliceArgs {
  const u16* x;
  const u16* w;      // [Cout, 3, 3, Cin]
  const u16* bias;   // [Cout] | null
  const u16* res;    // | null
  const u16* res2;   // | null
  u16* out;
  long long xs, os, rs, r2s;   // image strides
  int xp, op, rp, r2p;         // pixel pitches
  int N, H, W, Cin, act;
  float act_param, alpha, beta;
};

template <int NB>
__global__ __launch_bounds__(256) void conv3x3_slice_kernel(SliceArgs a) {
  __shared__ __attribute__((aligned(16))) u16 halo[2][18 * 18 * DS_PX];
  constexpr int NV = 18 * 18 * 4, NS = (NV + 255) / 256, NC = 4 * NB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_x = (a.W + 15) >> 4, tiles_y = (a.H + 15) >> 4;
  const int bid = blockIdx.x;
  const int n = bid / (tiles_x * tiles_y);
  const int trem = bid - n * tiles_x * tiles_y;
  const int ty = trem / tiles_x, tx = trem - ty * tiles_x;
  const int fr = lane & 15, fq = lane >> 4;
  const int y0 = ty * 16 - 1, x0 = tx * 16 - 1;
  const u16* img = a.x + (long long)n * a.xs;
  // staging slots of this thread: vector v = tid + 256 s -> (halo pixel v >> 2, 16-B chunk v & 3)
  long long soff[NS];
  bool sok[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int v = tid + 256 * s, p = v >> 2, ch = v & 3;
    const int py = p / 18, px = p - py * 18, iy = y0 + py, ix = x0 + px;
    sok[s] = v < NV && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
    soff[s] = sok[s] ? ((long long)iy * a.W + ix) * a.xp + 8 * ch : 0;
  }
  const s16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  s16x8 r[NS];
  auto load = [&](int c) {
#pragma unroll
    for (int s = 0; s < NS; ++s) r[s] = sok[s] ? *reinterpret_cast<const s16x8*>(img + soff[s] + c) : zero8;
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int v = tid + 256 * s;
      if (v < NV) *reinterpret_cast<s16x8*>(&halo[buf][(v >> 2) * DS_PX + 8 * (v & 3)]) = r[s];
    }
  };
  // A operand: MFMA row fr of block nb is output channel NC (fr >> 2) + 4 nb + (fr & 3); k = 8 fq .. 8 fq + 7
  const u16* wrow[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
    wrow[nb] = a.w + (long long)(NC * (fr >> 2) + 4 * nb + (fr & 3)) * 9 * a.Cin + 8 * fq;
  f32x4 acc[4][NB];
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[b][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  load(0);
  put(0);
  __syncthreads();
  int buf = 0;
  for (int c = 0; c < a.Cin; c += 32) {
    const bool more = c + 32 < a.Cin;
    if (more) load(c + 32);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        bf16x8 wf[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
          wf[nb] = *reinterpret_cast<const bf16x8*>(wrow[nb] + (ky * 3 + kx) * a.Cin + c);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int p = (wave * 4 + b + ky) * 18 + fr + kx;
          const bf16x8 xf = *reinterpret_cast<const bf16x8*>(&halo[buf][p * DS_PX + 8 * fq]);
#pragma unroll
          for (int nb = 0; nb < NB; ++nb)
            acc[b][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nb], xf, acc[b][nb], 0, 0, 0);
        }
      }
    if (more) put(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  // C/D layout: acc[b][nb][q] = (MFMA row 4 fq + q = channel NC fq + 4 nb + q, MFMA column fr = pixel tx * 16 + fr)
  // of image row ty * 16 + 4 wave + b.
  const int ox = tx * 16 + fr;
  if (ox >= a.W) return;
  const int cb = NC * fq;
  float bv[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) bv[j] = a.bias ? bf2f(a.bias[cb + j]) : 0.f;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int oy = ty * 16 + wave * 4 + b;
    if (oy >= a.H) continue;
    const long long pix = (long long)oy * a.W + ox;
    float v[NC];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float t = acc[b][nb][q] + bv[4 * nb + q];
        v[4 * nb + q] = a.alpha * (a.act ? act_apply(a.act, t, a.act_param) : t);
      }
    if (a.res) {
      const u16* rp = a.res + (long long)n * a.rs + pix * a.rp + cb;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const s16x4 t = *reinterpret_cast<const s16x4*>(rp + 4 * nb);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[4 * nb + q] += a.beta * bf2f((u16)t[q]);
      }
    }
    if (a.res2) {
      const u16* rp = a.res2 + (long long)n * a.r2s + pix * a.r2p + cb;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const s16x4 t = *reinterpret_cast<const s16x4*>(rp + 4 * nb);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[4 * nb + q] += bf2f((u16)t[q]);
      }
    }
    u16* op = a.out + (long long)n * a.os + pix * a.op + cb;
    if constexpr (NB % 2 == 0) {
#pragma unroll
      for (int h = 0; h < NB / 2; ++h) {
        s16x8 t;
#pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = (short)f2bf(v[8 * h + q]);
        *reinterpret_cast<s16x8*>(op + 8 * h) = t;
      }
    } else {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        s16x4 t;
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = (short)f2bf(v[4 * nb + q]);
        *reinterpret_cast<s16x4*>(op + 4 * nb) = t;
      }
    }
  }
}

// One operand as the host sees it: C channels of every pixel, from base, at a pixel pitch and an image stride.
struct SliceView {
  uintptr_t base;
  long long pitch, istride;
  int C;
};

static bool slice_ok(const SliceView& s, int N, long long HW) {
  if (!s.base || s.base % 16 || s.pitch % 8 || s.pitch < s.C || s.pitch > (1 << 20)) return false;
  if (N == 1) return true;
  return s.istride % 8 == 0 && s.istride >= (HW - 1) * s.pitch + s.C && s.istride <= (1ll << 60) / N;
}

// elements from the first to one past the last of a view (HW * pitch < 2^51, N * istride <= 2^60: slice_ok)
static long long slice_span(const SliceView& s, int N, long long HW) {
  return (N > 1 ? (N - 1) * s.istride : 0) + (HW - 1) * s.pitch + s.C;
}

static bool ranges_disjoint(uintptr_t a, long long na, uintptr_t b, long long nb) {   // na, nb: bf16 elements
  return a + 2 * (uintptr_t)na <= b || b + 2 * (uintptr_t)nb <= a;
}

static bool slice_same(const SliceView& a, const SliceView& b, int N) {
  return a.base == b.base && a.pitch == b.pitch && a.C == b.C && (N == 1 || a.istride == b.istride);
}

// No element of b is an element of a: their address ranges are apart, or they are channel slices of one pixel
// lattice (same pitch, same image stride, a multiple of the pitch) and b's channels lie behind a's in the pixel.
static bool slice_disjoint(const SliceView& a, const SliceView& b, int N, long long HW) {
  if (ranges_disjoint(a.base, slice_span(a, N, HW), b.base, slice_span(b, N, HW))) return true;
  if (a.pitch != b.pitch || (N > 1 && (a.istride != b.istride || a.istride % a.pitch))) return false;
  const long long d = ((long long)b.base - (long long)a.base) / 2;
  const long long r = ((d % a.pitch) + a.pitch) % a.pitch;
  return r >= a.C && r + b.C <= a.pitch;
}

// x: channels [0, Cin) of each pixel at pitch xp / image stride xs (elements); w [Cout, 3, 3, Cin]; bias [Cout] | null;
// res, res2: Cout channels per pixel at their own pitch / stride, | null; out likewise. Everything is validated
// before the launch and a call that breaks a rule returns hipErrorInvalidValue without one:
//   domain     N, H, W >= 1, H * W < 2^31, Cin % 32 == 0, Cout in {16, 32, 48, 64}, act a CgsAct code
//   layout     bases 16-byte aligned (bias: 2), pitches multiples of 8 and >= the channels used, the images of an
//              operand apart (stride >= (H W - 1) pitch + C)
//   aliasing   out shares no element with x, w or bias; res / res2 are out itself (the thread that writes an
//              element is the one that reads it) or share no element with it
CGS_EXPORT int cgs_conv3x3_slice(const void* x, int xp, long long xs, const void* w, const void* bias, const void* res,
                                 int rp, long long rs, const void* res2, int r2p, long long r2s, void* out, int op,
                                 long long os, int N, int H, int W, int Cin, int Cout, int act, float act_param,
                                 float alpha, float beta, hipStream_t stream) {
  const int E = (int)hipErrorInvalidValue;
  if (N < 1 || H < 1 || W < 1 || (long long)H * W >= (1ll << 31) || Cin < 32 || Cin % 32 || Cin > (1 << 20) ||
      Cout < 16 || Cout > 64 || Cout % 16 || act < CGS_ACT_NONE || act > CGS_ACT_LEAKY_RELU)
    return E;
  const long long HW = (long long)H * W;
  const long long nwg = (long long)N * ((H + 15) / 16) * ((W + 15) / 16);
  if (nwg > 0x7fffffffLL || nwg < 1) return E;
  const SliceView vx{(uintptr_t)x, xp, xs, Cin}, vo{(uintptr_t)out, op, os, Cout};
  const SliceView vr{(uintptr_t)res, rp, rs, Cout}, vr2{(uintptr_t)res2, r2p, r2s, Cout};
  if (!slice_ok(vx, N, HW) || !slice_ok(vo, N, HW) || !w || (uintptr_t)w % 16 || (uintptr_t)bias % 2) return E;
  if ((res && !slice_ok(vr, N, HW)) || (res2 && !slice_ok(vr2, N, HW))) return E;
  const long long ospan = slice_span(vo, N, HW);
  if (!slice_disjoint(vx, vo, N, HW) || !ranges_disjoint((uintptr_t)w, 9ll * Cin * Cout, vo.base, ospan) ||
      (bias && !ranges_disjoint((uintptr_t)bias, Cout, vo.base, ospan)))
    return E;
  if (res && !slice_same(vr, vo, N) && !slice_disjoint(vo, vr, N, HW) && !slice_disjoint(vr, vo, N, HW)) return E;
  if (res2 && !slice_same(vr2, vo, N) && !slice_disjoint(vo, vr2, N, HW) && !slice_disjoint(vr2, vo, N, HW)) return E;
  SliceArgs a{(const u16*)x, (const u16*)w, (const u16*)bias, (const u16*)res, (const u16*)res2, (u16*)out,
              N > 1 ? xs : 0, N > 1 ? os : 0, N > 1 ? rs : 0, N > 1 ? r2s : 0, xp, op, rp, r2p,
              N, H, W, Cin, act, act_param, alpha, beta};
  switch (Cout / 16) {
    case 1: conv3x3_slice_kernel<1><<<(unsigned)nwg, 256, 0, stream>>>(a); break;
    case 2: conv3x3_slice_kernel<2><<<(unsigned)nwg, 256, 0, stream>>>(a); break;
    case 3: conv3x3_slice_kernel<3><<<(unsigned)nwg, 256, 0, stream>>>(a); break;
    default: conv3x3_slice_kernel<4><<<(unsigned)nwg, 256, 0, stream>>>(a); break;
  }
  return (int)hipGetLastError();
}
