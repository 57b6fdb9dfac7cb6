// Image-space filters (K25 / K28 family): separable correlation with a fused epilogue (gaussian blur,
// unsharp mask, SAG's latent blur), k x k box maximum / minimum (grey morphology), and the two device
// stages of Canny (Sobel + non-maximum suppression + thresholds, then hysteresis sweeps).
// All are bandwidth-bound and use no MFMA: fp32 accumulation, fp32 / bf16 / fp16 storage selected at run
// time, inputs read in place through element strides (n, c, h, w) so an IMAGE [B, H, W, C], its movedim
// view, a channels-last latent and a plain NCHW tensor need no contiguous() copy.
//
// "Interleave" CI: when the channel stride is 1 and C <= 4, a workgroup owns a strip of W * C
// interleaved columns j = w * C + c of one image (neighbours along w are CI columns apart), so NHWC
// reads and writes coalesce; otherwise CI = 1 and a workgroup works on one (n, c) plane.
#include "common.h"

namespace {

template <int DT>
__device__ __forceinline__ float ldv(const void* p, long long i) {
  if constexpr (DT == CGS_F32) return reinterpret_cast<const float*>(p)[i];
  else return cvt_in<DT>(reinterpret_cast<const u16*>(p)[i]);
}

template <int DT>
__device__ __forceinline__ void stv(void* p, long long i, float v) {
  if constexpr (DT == CGS_F32) reinterpret_cast<float*>(p)[i] = v;
  else reinterpret_cast<u16*>(p)[i] = cvt_out<DT>(v);
}

#define CGS_DISPATCH_DT(dtype, KERNEL, ...)                                        \
  do {                                                                             \
    if ((dtype) == CGS_F32) KERNEL<CGS_F32> __VA_ARGS__;                           \
    else if ((dtype) == CGS_BF16) KERNEL<CGS_BF16> __VA_ARGS__;                    \
    else if ((dtype) == CGS_F16) KERNEL<CGS_F16> __VA_ARGS__;                      \
    else return (int)hipErrorInvalidValue;                                         \
  } while (0)

enum { BORDER_REFLECT = 0, BORDER_REPLICATE = 1, BORDER_ZERO = 2 };

// Source index of tap position i on an axis of n samples, -1 for a zero tap. Reflect is F.pad's (no edge
// repeat, one reflection: the caller guarantees r < n); the final clamp keeps every index in range whatever
// the caller passed.
__device__ __forceinline__ int border_index(int i, int n, int mode) {
  if (i >= 0 && i < n) return i;
  if (mode == BORDER_ZERO) return -1;
  if (mode == BORDER_REFLECT) i = i < 0 ? -i : 2 * (n - 1) - i;
  return min(max(i, 0), n - 1);
}

struct Strides4 {
  long long n, c, h, w;
};

// q / CI for q >= 0 and the interleaves the launchers admit (1..4): no runtime division
__device__ __forceinline__ int div_ci(int q, int CI) {
  switch (CI) {
    case 1: return q;
    case 2: return q >> 1;
    case 3: return q / 3;
    default: return q >> 2;
  }
}

// ---------------------------------------------------------------------------------------------
// cgs_filter_sep: y = clamp(ax * x + ay * ((t_h (x) t_w) * x), lo, hi), correlation, one launch.
// A workgroup owns a 32 x 64 tile (rows x interleaved columns). Horizontal pass: 16 input row segments at a
// time (4 per wave; tile + halo, border resolved in the index) are staged in LDS lines and every lane sums its
// column's kw taps from them into the 32 + 2 r_h rows of hbuf; vertical pass out of hbuf, 8 consecutive rows
// per thread so that each hbuf value is read once for its 8 outputs (the taps slide through registers).
// LDS is sized by the launch: at r = 31 hbuf is 94 x 64 fp32 = 23.5 KiB and the lines up to 19.5 KiB.
// Sums are explicit fmaf chains in tap order, so the result does not depend on the layout of x.
// ---------------------------------------------------------------------------------------------
constexpr int FS_TH = 32, FS_TW = 64, FS_MAXT = 63, FS_MAXCI = 4;
constexpr int FS_RPW = 4;               // lines staged per wave and step
constexpr int FS_VR = FS_TH / 4;        // output rows per thread of the vertical pass

constexpr int FS_MAXSEG = (FS_TW + (FS_MAXT - 1) * FS_MAXCI + 63) / 64;   // 64-lane pieces of the longest line

template <int DTI, int DTO>
__global__ void __launch_bounds__(256) filter_sep_kernel(const void* __restrict__ x, const void* __restrict__ xe,
                                                         void* __restrict__ y, const float* __restrict__ tw,
                                                         const float* __restrict__ th, int kw, int kh, int C, int H,
                                                         int W, int CI, Strides4 si, Strides4 se, Strides4 so,
                                                         int border, float ax, float ay, float lo, float hi,
                                                         int planes) {
#pragma clang fp contract(off)
  extern __shared__ float fs_smem[];
  __shared__ float taps_w[FS_MAXT + 1], taps_h[FS_MAXT + 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid < kw) taps_w[tid] = tw ? tw[tid] : 1.f;                              // null taps: the one tap 1
  if (tid >= 64 && tid - 64 < kh) taps_h[tid - 64] = th ? th[tid - 64] : 1.f;
  const int rw = kw >> 1, rh = kh >> 1;
  const int j0 = blockIdx.x * FS_TW, h0 = blockIdx.y * FS_TH;
  const int WJ = W * CI, cgroups = C / CI;
  const int rows = FS_TH + 2 * rh;
  const int L = FS_TW + 2 * rw * CI;
  float* hbuf = fs_smem;                                         // [rows][FS_TW]
  float* lines = fs_smem + rows * FS_TW + wave * FS_RPW * L;     // this wave's [FS_RPW][L]
  // the column part of the source offset of this lane's line elements (the same for every row): -1 = zero tap
  long long coff[FS_MAXSEG];
#pragma unroll
  for (int m = 0; m < FS_MAXSEG; ++m) {
    const int q = j0 + lane + 64 * m;   // line element l is column j0 - rw * CI + l: same channel as j0 + l
    const int wq = div_ci(q, CI);
    const int ws = border_index(wq - rw, W, border);
    coff[m] = ws >= 0 ? (q - wq * CI) * si.c + ws * si.w : -1;
  }
  for (int p = blockIdx.z; p < planes; p += gridDim.z) {
    const int n = p / cgroups, c0 = (p - n * cgroups) * CI;
    const long long xb = n * si.n + c0 * si.c;
    __syncthreads();   // the taps are in LDS; the previous plane's reads of hbuf are done
    for (int rb = 0; rb < rows; rb += 4 * FS_RPW) {
      const int r0 = rb + wave * FS_RPW;
#pragma unroll
      for (int k = 0; k < FS_RPW; ++k) {
        const int r = r0 + k;
        const int hs = r < rows ? border_index(h0 - rh + r, H, border) : -1;
#pragma unroll
        for (int m = 0; m < FS_MAXSEG; ++m) {
          const int l = lane + 64 * m;
          if (l < L) lines[k * L + l] = (hs >= 0 && coff[m] >= 0) ? ldv<DTI>(x, xb + hs * si.h + coff[m]) : 0.f;
        }
      }
      __syncthreads();
      float acc[FS_RPW];
#pragma unroll
      for (int k = 0; k < FS_RPW; ++k) acc[k] = 0.f;
      for (int t = 0; t < kw; ++t) {
        const float wt = taps_w[t];
#pragma unroll
        for (int k = 0; k < FS_RPW; ++k) acc[k] = fmaf(wt, lines[k * L + lane + t * CI], acc[k]);
      }
#pragma unroll
      for (int k = 0; k < FS_RPW; ++k)
        if (r0 + k < rows) hbuf[(r0 + k) * FS_TW + lane] = acc[k];
      __syncthreads();
    }
    const int j = j0 + lane;
    if (j < WJ) {
      const int w = div_ci(j, CI), c = c0 + (j - w * CI);
      const int ib = wave * FS_VR;
      float acc[FS_VR], tp[FS_VR];     // tp[i] = tap s - i of step s (0 outside the taps: never used)
#pragma unroll
      for (int i = 0; i < FS_VR; ++i) acc[i] = tp[i] = 0.f;
      for (int s = 0; s < FS_VR + kh - 1; ++s) {
#pragma unroll
        for (int i = FS_VR - 1; i > 0; --i) tp[i] = tp[i - 1];
        tp[0] = s < kh ? taps_h[s] : 0.f;
        const float v = hbuf[(ib + s) * FS_TW + lane];
#pragma unroll
        for (int i = 0; i < FS_VR; ++i)
          if (s - i >= 0 && s - i < kh) acc[i] = fmaf(tp[i], v, acc[i]);   // output row ib + i, tap s - i: tap order
      }
#pragma unroll
      for (int i = 0; i < FS_VR; ++i) {
        const int h = h0 + ib + i;
        if (h < H) {
          float v = ay * acc[i];
          if (ax != 0.f) v = fmaf(ax, ldv<DTO>(xe, n * se.n + c * se.c + h * se.h + w * se.w), v);
          v = fminf(fmaxf(v, lo), hi);
          stv<DTO>(y, n * so.n + c * so.c + h * so.h + w * so.w, v);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// cgs_morph_box: one axis of the k x k box maximum / minimum. The window of output i on an axis of L
// samples is [i - p, i + q] clamped to the image (= max_pool2d after replicate padding (p, q)). A workgroup
// loads its outputs plus the p + q halo into LDS (indices clamped) and builds window maxima by doubling:
// M_2s[e] = op(M_s[e], M_s[e + s]), log2(p + q + 1) ping-pong steps, then out = op(M_P[e], M_P[e + len - P])
// with P the largest power of two <= len. O(log k) per element whatever k is; exact in every dtype.
// axis 0 (along w): the workgroup owns SEG interleaved columns of one row, window step CI elements.
// axis 1 (along h): it owns SEG rows of LW adjacent interleaved columns, window step LW elements.
// ---------------------------------------------------------------------------------------------
constexpr int MB_EXT = 8192;   // floats per ping-pong buffer: 2 x 32 KiB
constexpr int MB_MAXLEN = 1023;

template <bool MAXOP>
__device__ __forceinline__ float morph_op(float a, float b) {   // NaN wins, as in max_pool2d
  if constexpr (MAXOP) return (b > a || b != b) ? b : a;
  else return (b < a || b != b) ? b : a;
}

template <int DT, bool MAXOP>
__global__ void __launch_bounds__(256) morph_pass_kernel(const void* __restrict__ x, void* __restrict__ y, int C,
                                                         int H, int W, int CI, Strides4 si, Strides4 so, int axis,
                                                         int p, int q, int LW, int SEG, int planes) {
  extern __shared__ float mb_smem[];
  const int tid = threadIdx.x;
  const int len = p + q + 1;
  const int WJ = W * CI, cgroups = C / CI;
  const int S = axis == 0 ? CI : LW;
  const int lw_shift = 31 - __clz(LW);   // LW is a power of two
  const int n_out = axis == 0 ? SEG : SEG * LW;
  const int n_ext = n_out + (len - 1) * S;
  for (int pl = blockIdx.z; pl < planes; pl += gridDim.z) {
    const int n = pl / cgroups, c0 = (pl - n * cgroups) * CI;
    __syncthreads();   // the previous plane's reads of the buffers are done
    for (int e = tid; e < n_ext; e += 256) {
      int h, w, c;
      if (axis == 0) {
        const int qq = blockIdx.x * SEG + e;   // element e is column blockIdx.x * SEG - p * CI + e
        const int wq = div_ci(qq, CI);
        c = qq - wq * CI;
        w = min(max(wq - p, 0), W - 1);
        h = blockIdx.y;
      } else {
        const int r = e >> lw_shift, col = e - r * LW;
        const int j = min((int)blockIdx.x * LW + col, WJ - 1);
        w = div_ci(j, CI);
        c = j - w * CI;
        h = min(max((int)blockIdx.y * SEG + r - p, 0), H - 1);
      }
      mb_smem[e] = ldv<DT>(x, n * si.n + (c0 + c) * si.c + h * si.h + w * si.w);
    }
    __syncthreads();
    float *cur = mb_smem, *nxt = mb_smem + n_ext;
    int pw = 1;
    while (2 * pw <= len) {   // uniform: len is a kernel argument
      const int off = pw * S;
      for (int e = tid; e < n_ext; e += 256) {
        float a = cur[e];
        if (e + off < n_ext) a = morph_op<MAXOP>(a, cur[e + off]);
        nxt[e] = a;
      }
      __syncthreads();
      float* t = cur;
      cur = nxt;
      nxt = t;
      pw *= 2;
    }
    const int off = (len - pw) * S;   // f + off <= n_out - 1 + (len - 1) * S < n_ext
    for (int f = tid; f < n_out; f += 256) {
      int h, j;
      if (axis == 0) {
        j = blockIdx.x * SEG + f;
        h = blockIdx.y;
      } else {
        const int r = f >> lw_shift;
        j = blockIdx.x * LW + (f - r * LW);
        h = blockIdx.y * SEG + r;
      }
      if (j >= WJ || h >= H) continue;
      const int w = div_ci(j, CI), c = c0 + (j - w * CI);
      stv<DT>(y, n * so.n + c * so.c + h * so.h + w * so.w, morph_op<MAXOP>(cur[f], cur[f + off]));
    }
  }
}

// ---------------------------------------------------------------------------------------------
// cgs_canny_nms: blurred gray plane [B, H, W] fp32 -> magnitude (fp32) and class map (uint8: 2 strong,
// 1 weak, 0 none). A workgroup stages its 16 x 64 tile of the blur plus a 2-pixel replicate halo, forms
// mag = sqrt(gx^2 + gy^2 + 1e-6) on the tile plus a 1-pixel ring (0 outside the image, as the zero-padded
// mag of the reference), then suppresses against the two neighbours along the quantised direction.
// The direction sector needs no atan2: with a = |gx|, b = |gy|, b < tan(22.5 deg) a is 0 deg,
// b >= tan(67.5 deg) a is 90 deg, and between them the signs tell 45 from 135.
// ---------------------------------------------------------------------------------------------
constexpr int CN_TH = 16, CN_TW = 64;

__device__ __forceinline__ void sobel_at(const float (*bl)[CN_TW + 4], int r, int c, float& gx, float& gy) {
  const float a = bl[r - 1][c - 1], b = bl[r - 1][c], d = bl[r - 1][c + 1];
  const float e = bl[r][c - 1], f = bl[r][c + 1];
  const float g = bl[r + 1][c - 1], h = bl[r + 1][c], k = bl[r + 1][c + 1];
  gx = ((d - a) + (k - g)) + 2.f * (f - e);
  gy = ((g - a) + (k - d)) + 2.f * (h - b);
}

__global__ void __launch_bounds__(256) canny_nms_kernel(const float* __restrict__ blur, float* __restrict__ mag,
                                                        uint8_t* __restrict__ cls, int H, int W, float low,
                                                        float high) {
#pragma clang fp contract(off)
  __shared__ float bl[CN_TH + 4][CN_TW + 4];
  __shared__ float mg[CN_TH + 2][CN_TW + 2];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * CN_TW, y0 = blockIdx.y * CN_TH;
  const long long base = (long long)blockIdx.z * H * W;
  for (int e = tid; e < (CN_TH + 4) * (CN_TW + 4); e += 256) {
    const int r = e / (CN_TW + 4), c = e - r * (CN_TW + 4);
    const int yy = min(max(y0 - 2 + r, 0), H - 1), xx = min(max(x0 - 2 + c, 0), W - 1);
    bl[r][c] = blur[base + (long long)yy * W + xx];
  }
  __syncthreads();
  for (int e = tid; e < (CN_TH + 2) * (CN_TW + 2); e += 256) {
    const int r = e / (CN_TW + 2), c = e - r * (CN_TW + 2);
    const int yy = y0 - 1 + r, xx = x0 - 1 + c;
    float m = 0.f;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
      float gx, gy;
      sobel_at(bl, r + 1, c + 1, gx, gy);
      m = sqrtf(gx * gx + gy * gy + 1e-6f);
    }
    mg[r][c] = m;
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  const int xx = x0 + lane;
  if (xx >= W) return;   // no barrier below
  for (int i = wave; i < CN_TH; i += 4) {
    const int yy = y0 + i;
    if (yy >= H) break;
    float gx, gy;
    sobel_at(bl, i + 2, lane + 2, gx, gy);
    const float a = fabsf(gx), b = fabsf(gy);
    int dy, dx;
    if (b < 0.41421356237309503f * a || (a == 0.f && b == 0.f)) { dy = 0; dx = 1; }       // 0 deg
    else if (b >= 2.414213562373095f * a) { dy = 1; dx = 0; }                               // 90 deg
    else if ((gx > 0.f) == (gy > 0.f)) { dy = 1; dx = 1; }                                  // 45 deg
    else { dy = 1; dx = -1; }                                                               // 135 deg
    const float m = mg[i + 1][lane + 1];
    const float n1 = mg[i + 1 + dy][lane + 1 + dx], n2 = mg[i + 1 - dy][lane + 1 - dx];
    const float nms = (m >= n1 && m >= n2) ? m : 0.f;
    const long long o = base + (long long)yy * W + xx;
    mag[o] = m;
    cls[o] = nms > high ? 2 : (nms > low ? 1 : 0);
  }
}

// ---------------------------------------------------------------------------------------------
// cgs_hysteresis_sweep: one sweep of "grow class 2 through 8-connected class 1" over a class map
// [B, H, W] uint8, in place. A workgroup loads its 32 x 64 tile plus a 1-pixel ring (0 outside the image),
// promotes weak pixels that touch a strong one until its tile stops changing (the loop condition is a
// __syncthreads_or, so every lane leaves together; at most one iteration per tile pixel), writes the
// promoted pixels back and adds 1 to *counter if there were any. Promotion is monotone (1 -> 2 only), so a
// ring read while a neighbouring workgroup writes it is either value of a pixel that ends as 2 anyway; the
// host relaunches until a sweep leaves the counter at 0, which is the fixed point whatever the order was.
// No workgroup waits for another.
// ---------------------------------------------------------------------------------------------
constexpr int HY_TH = 32, HY_TW = 64, HY_ROWS = HY_TH / 4;

__global__ void __launch_bounds__(256) hysteresis_sweep_kernel(uint8_t* cls, int H, int W, int* counter) {
  __shared__ uint8_t t[HY_TH + 2][HY_TW + 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = blockIdx.x * HY_TW, y0 = blockIdx.y * HY_TH;
  uint8_t* img = cls + (long long)blockIdx.z * H * W;
  for (int e = tid; e < (HY_TH + 2) * (HY_TW + 2); e += 256) {
    const int r = e / (HY_TW + 2), c = e - r * (HY_TW + 2);
    const int yy = y0 - 1 + r, xx = x0 - 1 + c;
    t[r][c] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? img[(long long)yy * W + xx] : (uint8_t)0;
  }
  __syncthreads();
  unsigned mine = 0;   // bit k: this thread promoted its k-th pixel
  const int c = lane + 1;
  for (int iter = 0; iter < HY_TH * HY_TW; ++iter) {
    unsigned promote = 0;
#pragma unroll
    for (int k = 0; k < HY_ROWS; ++k) {
      const int r = wave * HY_ROWS + k + 1;
      if (t[r][c] == 1) {
        const bool s = t[r - 1][c - 1] == 2 || t[r - 1][c] == 2 || t[r - 1][c + 1] == 2 || t[r][c - 1] == 2 ||
                       t[r][c + 1] == 2 || t[r + 1][c - 1] == 2 || t[r + 1][c] == 2 || t[r + 1][c + 1] == 2;
        if (s) promote |= 1u << k;
      }
    }
    __syncthreads();   // every read of this round is done before any write
#pragma unroll
    for (int k = 0; k < HY_ROWS; ++k)
      if (promote & (1u << k)) t[wave * HY_ROWS + k + 1][c] = 2;
    mine |= promote;
    if (!__syncthreads_or(promote != 0)) break;
  }
  const int changed = __syncthreads_or(mine != 0);
  if (!changed) return;
#pragma unroll
  for (int k = 0; k < HY_ROWS; ++k)
    if (mine & (1u << k)) img[(long long)(y0 + wave * HY_ROWS + k) * W + x0 + lane] = 2;   // was 1: inside the image
  if (tid == 0) atomicAdd(counter, 1);
}

inline unsigned plane_grid(long long planes) { return (unsigned)(planes < 65535 ? planes : 65535); }

}  // namespace

// x by element strides (n, c, h, w); y by element strides too (contiguous in the caller's layout).
// tw / th: fp32 device arrays of kw / kh taps (odd, 1..63). CI: channel interleave (1, or C when C <= 4).
// border 0 reflect (needs r < extent), 1 replicate, 2 zero. y = clamp(ax * x + ay * filtered, lo, hi).
// tmp: null for the one-launch form; else an fp32 buffer with y's strides, and the same kernel runs twice:
// the horizontal taps into tmp, then the vertical taps and the epilogue out of it. The horizontal sums are
// stored exactly as the fused form holds them in LDS and the passes' unit taps multiply by 1, so both forms
// give the same bits.
CGS_EXPORT int cgs_filter_sep(const void* x, void* y, void* tmp, const float* tw, const float* th, int kw, int kh,
                              int N, int C, int H, int W, int CI, long long sn, long long sc, long long sh,
                              long long sw, long long on, long long oc, long long oh, long long ow, int border,
                              float ax, float ay, float lo, float hi, int dtype, hipStream_t stream) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  if (kw < 1 || kh < 1 || kw > FS_MAXT || kh > FS_MAXT || !(kw & 1) || !(kh & 1) || border < 0 || border > 2 ||
      CI < 1 || CI > FS_MAXCI || C % CI || !tw || !th || dtype < CGS_F32 || dtype > CGS_F16)
    return (int)hipErrorInvalidValue;
  if (border == BORDER_REFLECT && (kw / 2 >= W || kh / 2 >= H)) return (int)hipErrorInvalidValue;
  const long long gx = ((long long)W * CI + FS_TW - 1) / FS_TW, gy = (H + FS_TH - 1) / FS_TH;
  if (gx > 0x7fffffffLL || gy > 65535) return (int)hipErrorInvalidValue;
  const long long planes = (long long)N * (C / CI);
  if (planes > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)gx, (unsigned)gy, plane_grid(planes));
  const Strides4 si{sn, sc, sh, sw}, so{on, oc, oh, ow};
  const float inf = __builtin_inff();
  auto lds = [&](int w_taps, int h_taps) {
    return ((size_t)(FS_TH + h_taps - 1) * FS_TW + 4 * FS_RPW * (size_t)(FS_TW + (w_taps - 1) * CI)) * sizeof(float);
  };
#define CGS_FS(TI, TO, SRC, SI, DST, TW, TH, KW, KH, AX, AY, LO, HI)                                                  \
  filter_sep_kernel<TI, TO><<<grid, 256, lds(KW, KH), stream>>>(SRC, x, DST, TW, TH, KW, KH, C, H, W, CI, SI, si, so, \
                                                                border, AX, AY, LO, HI, (int)planes)
  if (!tmp) {
    if (dtype == CGS_F32) CGS_FS(CGS_F32, CGS_F32, x, si, y, tw, th, kw, kh, ax, ay, lo, hi);
    else if (dtype == CGS_BF16) CGS_FS(CGS_BF16, CGS_BF16, x, si, y, tw, th, kw, kh, ax, ay, lo, hi);
    else CGS_FS(CGS_F16, CGS_F16, x, si, y, tw, th, kw, kh, ax, ay, lo, hi);
  } else {
    if (dtype == CGS_F32) CGS_FS(CGS_F32, CGS_F32, x, si, tmp, tw, nullptr, kw, 1, 0.f, 1.f, -inf, inf);
    else if (dtype == CGS_BF16) CGS_FS(CGS_BF16, CGS_F32, x, si, tmp, tw, nullptr, kw, 1, 0.f, 1.f, -inf, inf);
    else CGS_FS(CGS_F16, CGS_F32, x, si, tmp, tw, nullptr, kw, 1, 0.f, 1.f, -inf, inf);
    if (dtype == CGS_F32) CGS_FS(CGS_F32, CGS_F32, tmp, so, y, nullptr, th, 1, kh, ax, ay, lo, hi);
    else if (dtype == CGS_BF16) CGS_FS(CGS_F32, CGS_BF16, tmp, so, y, nullptr, th, 1, kh, ax, ay, lo, hi);
    else CGS_FS(CGS_F32, CGS_F16, tmp, so, y, nullptr, th, 1, kh, ax, ay, lo, hi);
  }
#undef CGS_FS
  return (int)hipGetLastError();
}

// k x k box maximum (op 0) / minimum (op 1): rows into tmp, then columns into y. tmp and y share the element
// strides (on, oc, oh, ow) and x's dtype. Window [i - k/2, i + k - 1 - k/2] clamped to the image; on an axis of L
// samples only min(., L - 1) of either side matters, and that clamped window must be at most 1023 long.
CGS_EXPORT int cgs_morph_box(const void* x, void* tmp, void* y, int N, int C, int H, int W, int CI, long long sn,
                             long long sc, long long sh, long long sw, long long on, long long oc, long long oh,
                             long long ow, int k, int op, int dtype, hipStream_t stream) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  if (k < 1 || CI < 1 || CI > FS_MAXCI || C % CI || (op != 0 && op != 1) || H > 65535) return (int)hipErrorInvalidValue;
  const int p = k / 2, q = k - 1 - p;
  const int pw = p < W - 1 ? p : W - 1, qw = q < W - 1 ? q : W - 1;
  const int ph = p < H - 1 ? p : H - 1, qh = q < H - 1 ? q : H - 1;
  if (pw + qw + 1 > MB_MAXLEN || ph + qh + 1 > MB_MAXLEN) return (int)hipErrorInvalidValue;
  const long long planes = (long long)N * (C / CI);
  if (planes > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  const long long WJ = (long long)W * CI;
  const Strides4 si{sn, sc, sh, sw}, so{on, oc, oh, ow};
  // rows: SEG interleaved columns of one row per workgroup, the row split evenly; LDS = the two ping-pong buffers
  int seg = MB_EXT - (pw + qw) * CI;
  if (seg > 2048) seg = 2048;
  const long long nseg = (WJ + seg - 1) / seg;
  seg = (int)(((WJ + nseg - 1) / nseg + 63) / 64 * 64);
  const dim3 g0((unsigned)((WJ + seg - 1) / seg), (unsigned)H, plane_grid(planes));
  const size_t lds0 = 2 * (size_t)(seg + (pw + qw) * CI) * sizeof(float);
  // columns: the widest strip that leaves room for a row segment of at least half the halo (8 rows at the least);
  // the segment is twice the halo where that fits (small windows: more workgroups per CU), 30 rows at the least
  const int halo = ph + qh;
  int lw = 64, segh = MB_EXT / 64 - halo;
  while (lw > 4 && segh < (halo / 2 > 8 ? halo / 2 : 8)) {
    lw >>= 1;
    segh = MB_EXT / lw - halo;
  }
  const int want = 2 * halo > 30 ? 2 * halo : 30;
  if (segh > want) segh = want;
  if (segh > (H + 7) / 8 * 8) segh = (H + 7) / 8 * 8;
  const long long g1x = (WJ + lw - 1) / lw, g1y = (H + segh - 1) / segh;
  if (g1x > 0x7fffffffLL || g1y > 65535) return (int)hipErrorInvalidValue;
  const dim3 g1((unsigned)g1x, (unsigned)g1y, plane_grid(planes));
  const size_t lds1 = 2 * (size_t)(segh + halo) * lw * sizeof(float);
#define CGS_MORPH(DT)                                                                                              \
  do {                                                                                                             \
    if (op == 0) {                                                                                                 \
      morph_pass_kernel<DT, true><<<g0, 256, lds0, stream>>>(x, tmp, C, H, W, CI, si, so, 0, pw, qw, 1, seg, (int)planes); \
      morph_pass_kernel<DT, true><<<g1, 256, lds1, stream>>>(tmp, y, C, H, W, CI, so, so, 1, ph, qh, lw, segh, (int)planes); \
    } else {                                                                                                       \
      morph_pass_kernel<DT, false><<<g0, 256, lds0, stream>>>(x, tmp, C, H, W, CI, si, so, 0, pw, qw, 1, seg, (int)planes); \
      morph_pass_kernel<DT, false><<<g1, 256, lds1, stream>>>(tmp, y, C, H, W, CI, so, so, 1, ph, qh, lw, segh, (int)planes); \
    }                                                                                                              \
  } while (0)
  if (dtype == CGS_F32) CGS_MORPH(CGS_F32);
  else if (dtype == CGS_BF16) CGS_MORPH(CGS_BF16);
  else if (dtype == CGS_F16) CGS_MORPH(CGS_F16);
  else return (int)hipErrorInvalidValue;
#undef CGS_MORPH
  return (int)hipGetLastError();
}

// blur [B, H, W] fp32 contiguous -> mag [B, H, W] fp32, cls [B, H, W] uint8
CGS_EXPORT int cgs_canny_nms(const float* blur, float* mag, void* cls, int B, int H, int W, float low, float high,
                             hipStream_t stream) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  const int gy = (H + CN_TH - 1) / CN_TH;
  if (B > 65535 || gy > 65535) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((W + CN_TW - 1) / CN_TW), (unsigned)gy, (unsigned)B);
  canny_nms_kernel<<<grid, 256, 0, stream>>>(blur, mag, (uint8_t*)cls, H, W, low, high);
  return (int)hipGetLastError();
}

// one sweep over cls [B, H, W] uint8 in place; *counter (int32, device) += number of tiles that promoted a pixel
CGS_EXPORT int cgs_hysteresis_sweep(void* cls, int B, int H, int W, int* counter, hipStream_t stream) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  const int gy = (H + HY_TH - 1) / HY_TH;
  if (B > 65535 || gy > 65535 || !counter) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((W + HY_TW - 1) / HY_TW), (unsigned)gy, (unsigned)B);
  hysteresis_sweep_kernel<<<grid, 256, 0, stream>>>((uint8_t*)cls, H, W, counter);
  return (int)hipGetLastError();
}
