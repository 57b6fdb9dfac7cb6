"""Per-element worst-case error bounds of the bf16 GEMM, conv and attention kernels (test_kernel_bounds_*.py) and
of the bf16 / fp16 GroupNorm, LayerNorm, depthwise-conv and softmax2 kernels (test_norm_bounds_gpu.py), of the GRN
family and of the planar image-space kernels (test_image_bounds_gpu.py), of the fp32 GEMM, conv, norm and
attention kernels (test_f32_bounds_gpu.py), and of the small kernels of the sampler loop: CFG combine, Euler step,
counter-based noise, the device-parameterised step, timestep embedding and SiLU (test_sampling_bounds_gpu.py).

Every ``*_bound`` function takes the operands the kernel is given (CPU or GPU tensors of any float type), builds
the result in fp64 and returns ``(ref, tol)``: two fp64 tensors of the output's shape. ``assert_within`` then
requires ``|y - ref| <= tol`` in every element: the bounds are worst-case, so the permitted share of outliers
is zero. They are derived from the number formats, not measured:

    u = 2^-8    bf16 unit roundoff (round to nearest, 8 significand bits)
    e = 2^-24   fp32 unit roundoff
    C_ACC = 2   factor on Higham's gamma_K = K e for the unknown summation order inside and across MFMAs

GEMM / conv:  tol = u |ref| (1 + 2u)  +  [residual given] u |pre|  +  C_ACC K e mag
  1. the final bf16 store of a value within delta of ref: u |ref + delta| <= u |ref| + u delta; (1 + 2u) and
     the third term absorb u delta;
  2. the second rounding of the kernels whose epilogue rounds the tile to bf16 and then adds the residual in
     bf16 (pre = alpha a w^T + bias is rounded, pre + res is rounded again);
  3. fp32 accumulation of K products in any order: |fl(sum) - sum| <= gamma_K sum |a_i w_i|; mag is that sum of
     magnitudes plus |bias| and |res| (the fp32 epilogue additions).

Attention:  tol = u |ref| (1 + 2u) + (2 + extra_roundings) u A + 1e-6,  A = p |v|
  one u for the bf16 rounding of P before the PV MFMA (relative: P <= 2^8 under the deferred rescale), one u
  of margin for the normaliser summed from rounded or unrounded P; the score error is negligible (fp32 scale
  after the dot product). The key-split forms keep per-slice partial outputs in bf16: extra_roundings = 1.

The norm, depthwise and softmax2 kernels (test_norm_bounds_gpu.py) run in bf16 and fp16: u = u(dtype) below, 2^-8
or 2^-11, taken from the dtype of x. Every store term also carries tiny(dtype): half the fp16 subnormal spacing
(2^-25), or the smallest normal 2^-126 where bf16 / fp32 results may be flushed to zero.

GroupNorm statistics of the n = HW C/G values v = x + pre_add of a group. Every intermediate mean lies in the
data's range, so R = max |v| + 3 (max v - min v) bounds one step's error / e: Lb = the dependent fp32 additions of
one block sum, L = those of the whole reduction (gn_depth; a reduction of unknown structure: Lb = L = n):
  dmean = L e R                                 a block mean sh + s1 / cnt, then merges mean += d f: one rounding
                                                of the new mean (<= max |v|) and three on the increment d f (d, f,
                                                the product; |d f| <= max v - min v) on each of the L steps
  dvar  = 2 Lb e E2 + 8 L e var + 4 sqrt(var) dmean + dmean^2
    E2 = mean (v - shift)^2 with shift = the block's first pixel (known blocks; else <= 2 var + 2 max (v-mean)^2):
         s2 - s1^2 / cnt cancels at the magnitude of s2, both summed with gamma_Lb;
    8 L e var: the merges add the positive terms qb + d^2 na f, eight roundings a step;
    4 sqrt(var) dmean: Chan's merge of perturbed means m_b + delta_b is the exact weighted variance of those means,
         off by 2 sum c_b (m_b - mean)(delta_b - delta) <= 2 n sqrt(var) 2 dmean to first order (Jensen).
LayerNorm statistics of a row of C values, two-pass, L = ln_depth(C) the depth of the kernels' summation tree:
  dmean = C_ACC L e mean|v| + e |mean|          fp32 sum over a tree of depth L (gamma_L sum|v|), then the division
  dvar  = C_ACC (L + 4) e var + dmean^2         sum (v - m)^2 = C var + C (m - mean)^2, every term relative to
                                                var; no cancellation term
  drstd / rstd = dvar / (2 (var + eps)) + RSQRT_REL
GroupNorm output: the kernel folds a = rstd gamma, b = (pre - mean) a + beta and stores round(act(x a + b)):
  d = |a| dmean + |z gamma| drstd / rstd + 6 e (|x||a| + (|mean| + |pre|)|a| + |beta|)
  the last term is the cancellation of x a against b: four roundings on each path (a, the product, pre - mean,
  the sums), 6 for the second order;  through SiLU d -> SILU_SLOPE d + silu_rel |ref|;
  tol = u |ref| (1 + 2u) + tiny + d (1 + u).  groupnorm_apply_bound: (mean, rstd) given, dmean = drstd = 0.
LayerNorm output, round(((x - m) r) w + b):  d = |w| rstd dmean + |z w| drstd / rstd + 6 e (|z w| + |b|).
Partials (P (mean, M2) pairs of 80 columns, P Chan merges in sequence), dev = max_p |m_p - mean|:
  dmean = C_ACC P e (|mean| + 4 dev) + e |mean|   each merge: mean += d f, three roundings on d f (|d| <= 2 dev), one
                                                  on the sum (<= |mean| + dev)
  dM2   = C_ACC (P + 6) e M2 + 320 P dev dmean     d^2 n f with d off by the running mean's error, n f <= 80
Depthwise conv: the GEMM bound with K = k k products (+ 1 for the bias): tol = store + C_ACC (K + 1) e mag.
softmax2, p = 2^(x - max) / sum:  tol = u p (1 + 2u) + tiny + (C_ACC cols e + 2 EXP2_REL + 14 e + |x - max| e ln 2) p
  the normaliser is an fp32 sum of cols terms, each with the relative error EXP2_REL + |x_j - max| e ln 2 of its own
  (the subtraction is rounded once); weighted by p_j / sum these average to at most EXP2_REL + ln(cols) e <= EXP2_REL
  + 10 e; 4 e for the reciprocal and the product. A -inf input gets ref = tol = 0.
The GRN family and the image-space kernels (csrc/kernels/image.hip; test_image_bounds_gpu.py). build_native.py
compiles with -O3 and without -ffast-math or any other relaxed-math flag: sqrtf and / are correctly rounded, one e
each; fused multiply-adds only remove roundings. The kernels store bf16, fp16 or fp32: u(float32) = e.

GRN statistics, gx[n, c] = sqrt(sum_HW a^2), a = x or gelu(x). Only positive terms, so the error of the sum is
relative, C_ACC (L + 1) e: L dependent additions and the rounding of a^2. grn_depth restates L from the code:
  v2   a lane adds every fourth row of its slice (ceil(rows_per / 4), rows_per = ceil(HW / S), S = grn_slices), the
       LDS merge of the four row groups (2), the finalize loop over S / 4 float4s, each summed as a tree (+ 2);
  gns  nbk = HW / 64 given partials in four chains (nbk / 4, the tail on the first), then the merge (2);
  v1   32-row block sums added by atomics in unknown order: L = HW.
  dgx = gx (C_ACC (L + 1) e / 2 + e) + tiny: the square root halves the relative error and adds a rounding. With the
  fused GELU, | ||a + d|| - ||a|| | <= ||d|| <= sqrt(HW) GELU_ABS is added as an absolute term -- not a relative one,
  a channel of large negative x has gx below the approximation error. A channel of zeros is exact (tol = 0):
  gelu_sig2(0) = 0 * rcp(2) = 0.
Channel mean, positive terms again: wave_sum (6) and the 4-wave merge (2) give the sum of a block of 256 channels,
the apply kernel adds ceil(nblk / 64) of those per lane and runs another wave_sum (6): Lm. v1: ceil(C / 256) per
thread and an 8-level LDS tree.
  dmean = mean_C dgx + C_ACC Lm e mean;  inv = 1 / (mean + 1e-6):  dinv = inv (dmean / (mean + 1e-6) + 4 e)
  (the division by C, the addition, the fp32 value of 1e-6f, the reciprocal).
GRN output y = beta + a (1 + gamma nx), nx = gx inv, dnx = dgx inv + gx dinv + dgx dinv:
  d = |a gamma| dnx + k e (|beta| + |a| (1 + |gamma nx|)) + [GELU] GELU_ABS |1 + gamma nx|;  tol = _store_dt(ref, d)
  k = 5 roundings in every form: nx = gx inv, gamma nx, 1 + ., a (.), beta + .. The row-tiled form does the first
  three once per thread (a_j = 1 + gamma (nx iv)), the grid-stride form and v1 per element: the same count.
grn_apply_bound: gx and the block sums given, dnx = nx (C_ACC (ceil(nblk / 64) + 6) e + 4 e) only.
grn_scale_weight_bound, Wn[n] = W (1 + (gamma gx) inv) in bf16: four roundings, d = |W gamma| dnx + 4 e |W| (1 +
  |gamma nx|) with the dnx of grn_apply_bound.
resize (bilinear, bicubic, area) is separable: ref = Wy x Wx^T with the weights in fp64 from the exact scale.
  tol = store + k e sum |w_i x_i| + dw sum |x_taps|
  The fp32 source coordinate (o + 0.5) scale - 0.5 carries three roundings of values <= max(H, Ho): 3 e max(H, Ho),
  times the largest slope of the weight in the coordinate: 1 for bilinear, 1.35 for the cubic convolution with A =
  -0.75 (|cubic1'| at t = 0.6); the cubic's Horner forms add 64 e (six roundings of intermediates <= 8 |A| = 6 at t
  <= 2). dw is the sum over both axes (the weights of the other axis are <= 1). Both interpolants are continuous
  across integer source coordinates, so a floor that differs between fp32 and fp64 moves the taps but changes the
  value by no more than the same coordinate error: it stays inside dw. k = 6 (bilinear: 1 - l, two products and
  a sum per axis), 10 (bicubic: four products and sums per axis, the weights' last rounding), window size + 1 (area,
  dw = 0). nearest and nearest-exact move bits: the reference is F.interpolate on the CPU in the same dtype, tol = 0.
upfirdn2d: an fp64 reference of its own (zero-insert, pad or crop, true convolution, decimate);
  tol = store + C_ACC kh kw e mag.
fused_bias_act, leaky(x + b[c]) * scale with slope and scale as the fp32 values the kernel is given: three relative
  roundings, tol = store + 3 e |ref|.
softmax_rows, p = __expf(x scale - max) / sum in fp32: the product and the subtraction are rounded once each, the
  exponent is off by (|x scale| + |t|) e, t = x scale - max; __expf multiplies by the rounded constant log2 e: 2 |t|
  e more; relative after the exponential, plus EXP2_REL. The normaliser carries the p-weighted mean of the same and
  C_ACC cols e; 2 e for the reciprocal and the product; the fp32 store e p.
tome_match, s = (a_i . b_j) inv_a inv_b with inv = rsqrtf(sum of squares):
  ds = C_ACC (C + 2) e sum |a_i| |b_j| inv_a inv_b + 2 RSQRT_REL |s|
  the dot product runs over k in sequence, two more products; the second term is the two reciprocal roots (the
  relative error of their sums of squares, (ceil(C / 64) + 7) e each, is not itemised: for C >= 32 the second half
  of C_ACC (C + 2) e mag, unused by a sequential sum, majorises it). A row of zeros has inv = 0 and s = 0.

The fused epilogues (test_epilogue_bounds_gpu.py). Activation epilogues of the GEMMs and convs, out = round(act(pre))
(+ res), pre = alpha a w^T + bias (or the LayerNorm-folded or conv pre-activation), d_pre = C_ACC K e mag as above:
  tol = u |ref| (1 + 2u) + ([res] u |act(pre)| + slope_act d_pre + act_err) (1 + u)
  [res] u |act(pre)|: the mc::tile kernels round the activated tile to bf16 and add the residual to that (mfma_core.h,
    the row-wise read-back loop); v6, skinny and the split-K reduce add it in fp32 and round once, inside the same term.
  slope_act = max |act'|: GELU_SLOPE (erf and tanh GELU), SILU_SLOPE (SiLU; quick-GELU is the same curve in 1.702 x,
    with 1.702 x as the argument the slope in x is the same number), 1 (ReLU), max(1, |p|) (leaky ReLU).
  act_err: erf path GELU_ABS (gelu_sig against the exact function). SIG family, x rcp(1 + exp2(t)), t = x fma(x x, b,
    a) (act_fam / act_fam2, common.h): the fp32 constants a, b are within e of -c0 log2 e, -c1 log2 e; x x, the fma and
    the product x q round once each: |dt| <= 4 e |t| (a and b have one sign, so |t| = |x| (|a| + |b| x^2)); z = t ln 2 is
    the sigmoid's argument, so exp2 is off by 4 e |z| relative, then EXP2_REL, the addition of 1 (e), RCP_REL, the final
    product (e); the error of the denominator is at most that of its exp term:
      act_err = (4 |z| e + EXP2_REL + RCP_REL + 2 e) |act(pre)| + 1e-36   (1e-36: exp2 overflows to rcp(inf) = 0)
    LIN family: one rounding of a x, e |act(pre)| (x >= 0 and relu are exact).
  (1 + u): the last store rounds a value within those terms of ref (as _store_dt).
Row-statistics partials (pq::run RSO, mfma_pp160.h), (mean, M2) of every 80-column chunk of a stored row. Lane fq of
the four that hold a row's chunk has 20 values: columns 8 fq .. + 7, 32 + 8 fq .. + 7, 64 + 4 fq .. + 3 (colj); it sums
d = v - sh, sh = its first value, as five trees of four (depth 2) added in sequence (5): Lb = 7 dependent additions.
  lane:  s1 off by (Lb + 1) e S, S = sum |d| (the rounding of d);  s2 by (Lb + 2) e s2
         dmean = (Lb + 3) e S / 20 + e |mean|       the product by fl(1 / 20) (2 e) and the addition of sh
         dM2   = (3 Lb + 7) e s2                    m2 = s2 - s1^2 / 20 cancels at the magnitude of s2: s1^2 / 20 <= s2
                                                    (Cauchy-Schwarz), 2 (Lb + 1) e s2 from s1, 2 e s2 from its two
                                                    products, e s2 from the subtraction, (Lb + 2) e s2 from s2
  merge of two halves of n values (lanes l ^ 16, then l ^ 32): mean = (ma + mb) / 2, m2 = qa + qb + d^2 n / 2, d = mb - ma,
         delta = dma + dmb:  dmean = delta / 2 + e |mean|
         dM2 = dqa + dqb + n |d| delta + n delta^2 / 2 + 4 e d^2 n / 2 + 2 e m2     d, d d and the product by n / 2
                                                    (two roundings on d^2), then two additions of positive terms
  |y| is known, so every term is evaluated on the data. The sum of a representable x and an increment is off by at
  most the increment, so the two e |mean| are min(e |mean|, S / 20) in the lane (sh + s1 / 20) and min(e |mean|,
  (|d| + delta) / 2) in a merge (ma + mb = 2 ma + d): a chunk of identical values has d = S = s2 = 0 in every lane
  and every merge, and tol(M2) = tiny(fp32) alone.
  partials_merge_tol: partials each within (dm_p, dq_p) of exact ones move the row's mean = mean_p m_p by mean_p dm_p
  =: dmean and its M2 = sum q_p + 80 sum (m_p - mean)^2 by sum dq_p + 80 sum (2 |m_p - mean| dd_p + dd_p^2), dd_p =
  dm_p + dmean; rstd by rstd dM2 / (2 n (var + eps)). Added to layernorm_stats_bound of the stored rows and to the
  merge's own rs_from_partials_bound it bounds cgs_ln_rs_from_partials of a producer's partials against the rows.
Sum-of-squares partials (pq::run GNS == 2), [M / 64, N] over the 64 rows of a wave: NI = 4 additions in sequence, then
row16_sum (4): L = 8; positive terms only, tol = C_ACC (L + 1) e ref (+ 1: the square) + 64 tiny(fp32) (each of the
64 squares may be flushed below 2^-126). A block of zeros is exact.
GroupNorm partials (pq::run GNS == 1), [N, HW / 64, C, 2], two passes over the wave's registers: the sum of 4 values in
sequence (3) and row16_sum (4), L = 7, the product by 1 / 64 is exact; the structure is _ln_stats's:
  dmean = C_ACC L e mean |v| + e |mean|;  dM2 = C_ACC (L + 4) e M2 + 64 dmean^2    (v - m, its square, 8 additions)

The fp32 kernels (csrc/kernels/f32.hip, ops/f32.py; test_f32_bounds_*.py): u(float32) = e everywhere, _store_dt for
the norms. Nothing is rounded to a storage type, so every term is a rounding of the code.
GEMM / conv (f32_gemm_kernel, ``dtype=torch.float32`` on gemm_bound, gemm_act_bound, conv_bound, conv_act_bound; the
default dtype leaves every bf16 caller's (ref, tol) as it was, bit for bit). The epilogue is
  v = fmaf(acc, alpha, bias)  one rounding;  v = act(v);  v += R  one rounding;  the store does not round.
  tol = e |ref| (1 + 2e) + [R] e |pre| + C_ACC K e mag: the first term is the last rounding (the fma, or the addition
  of R), the second the fma when R follows it, the third the MFMA accumulation (exact fp32 products, one rounding
  a k step, in the permuted k order of the 16-deep slices). alpha is the fp32 value the kernel is passed.
  With an activation d_pre = C_ACC K e mag + e |pre| (the fma before it) and
  tol = e |ref| (1 + 2e) + ([R] e |act(pre)| + slope_act d_pre + act_err) (1 + e).
  A bare GELU, or code CGS_ACT_GELU, is gelu_f here, 0.5f x (1.0f + erff(x 0.70710678f)), not gelu_sig (GELU_ABS does
  not apply): t = fl(x c) with c within e of 1 / sqrt 2 is off by 2 e |t|, times erf' = 2 / sqrt(pi) exp(-t^2); erff
  adds ERFF_REL |erf t|; 1 + erf rounds once, e (1 + erf t); 0.5 x is exact and the last product rounds once more.
  The error of 1 + erf is absolute, not relative to the result -- it cancels for x << 0 -- so
    act_err = 0.5 |x| (4 / sqrt(pi) e |t| exp(-t^2) + ERFF_REL |erf t| + e (1 + erf t)) + 2 e |gelu(x)|.
  gelu_tanh, quick_gelu, silu and relu go through act_apply: the SIG / LIN terms above.
GroupNorm (cgs_groupnorm_f32): gn_f32_form restates S = gn_slices(N, HW) and the P pixel lanes of a channel chunk,
  gn_f32_depth the (Lb, L) of the three kernels; the statistics formulas are those of the bf16 kernels with E2 taken
  over the real slices [HW s // S, HW (s + 1) // S), shift = the slice's first pixel with its pre-add. New here:
  v = fl(x + pre_add) is rounded before use (gn_ld: one more step of R in L; e |v| |a| in the output, inside 6 e mag);
  a = fl(gamma rstd) and b = fl(beta - fl(mean a)) are stored and the output is fmaf(v, a, b): five roundings, each
  relative to a term of mag, inside the same 6 e mag; SiLU is o / (1.0f + expf(-o)) with a true division (_silu_div).
LayerNorm (cgs_layernorm_f32): one wave a row, two passes, L = ln_f32_depth(C) = ceil(C / 256) + 2 + 6 through the
  ``depth=`` of layernorm_bound; ((x - m) r) w + b is four roundings, inside 6 e (|z w| + |b|).
Attention (ops.f32.attention; attention_f32_bound), three launches a chunk of query rows:
  scores  s = fmaf(q . k, fl32(1 / sqrt D), 0):  ds = C_ACC D e mag + e |s|, + e |s + mask| for the host's sc.add_(mask)
  softmax cgs_softmax_rows over ld = ceil4(Sk) columns, the pad columns at -inf: its own relative term (softmax_rows
          at scale 1, cols = ld), and dp / p <= exp(2 max_row ds) - 1 for the scores' error (every t_j = s_j - max
          moves by at most 2 max ds, and so does the log of the normaliser)
  output  tol = store + C_ACC (Sk + 1) e (p |v|) + dp |v|     (K = Sk products of the stored p, alpha = 1)
  A row whose keys are all blocked is NaN on this path: ref = tol = nan, left out of assert_within and checked apart.

The kernels of the sampling loop (csrc/kernels/rng.hip and the fp32 / 16-bit kernels at the head of elementwise.hip;
test_sampling_bounds_cpu.py, test_sampling_bounds_gpu.py). Everything is fp32 arithmetic on fp32 data unless said
otherwise; every scalar is the fp32 value the kernel is passed (_f32). No sum is longer than two terms, so C_ACC
does not appear: every term is one counted rounding. Factors (1 + k e) absorb the second-order products. The device
libm figures are supposed, like EXPF_REL and ERFF_REL: LOGF_REL = 2 ulp for logf, SINCOSF_REL = 2 ulp for sinf and
cosf (1 ulp = 2 e); EXP2_REL for the v_exp_f32 inside __expf is the supposed figure of the softmax bounds.
cfg_combine_bound, ref = u + (c - u) s: the difference, the product and the sum round once each; a contraction of
  the last two into an fma only removes one.   tol = (2 e |c - u| |s| + e |ref|) (1 + 2e)
euler_step_bound, D = (x - den) / sigma, dt = sigma_down - sigma, x1 = x + D dt, ref = x1 + noise sigma_up:
  the host's 1.0f / sigma and sigma_down - sigma (a true division and a subtraction: e each), x - den and its product
  with the reciprocal (e each): d dt is within 4 e |D dt| of D dt; fmaf(d, dt, x) rounds once, e |x1|;
  fmaf(noise, sigma_up, x1) once more, e |ref|. The torch form of the same update (the fallback of ops.euler_step)
  rounds the two products on their own: e |D dt| and e |noise sigma_up| more, which the bound grants to both.
    tol = (5 e |D dt| + e |x1| + [noise] (e |noise sigma_up| + e |ref|)) (1 + 8e)
  noise is ignored, as the kernel ignores it, unless sigma_up > 0.
normal_bound, the N(0, 1) values of (seed, image, stream): element 4 g + j of an image is normal j of Philox group g.
  The Philox4x32-10 words w come from the integer code of the CPU mirror (sampling/rng.py, pinned to the published
  known-answer vectors in test_rng_cpu.py), the uniforms from the mirror's own fp32 _u01 and only then widened: the
  fp32 rounding of (k + 0.5) 2^-24 for k >= 2^23 is part of the definition of the generator (u = 1.0 for k = 2^24 - 1),
  a reference from the exact u is off by 2e-5 near u = 1. From there fp64 Box-Muller with the fp32 literal 6.2831853f:
    r = sqrt(-2 ln u0), t = 2pi_f u1, z = r cos t, r sin t       (u0, u1 = words 0, 1 and 2, 3)
  logf is off by LOGF_REL relative, the product by -2 is exact, sqrtf halves the relative error and rounds (e);
  t = fl(2pi_f u1) <= 2 pi is off by e t <= 2 pi e, which moves cos and sin by as much; cosf and sinf add SINCOSF_REL
  of a result <= 1; the product r cos t rounds once:
    tol = e (A r + B |z|) (1 + 8e),  A = 2 pi + SINCOSF_REL / e,  B = 2 + LOGF_REL / (2 e)
  u0 = 1.0 gives r = 0 and tol = 0: the value is an exact zero. bf16 output: _store_dt of that, u |ref| (1 + 2u) more.
  Measured on the MI355X (test_sampling_bounds_gpu.py): max |y - ref| / tol = 0.40 over the 180 fp32 cases of
  test_philox_randn_bound and 0.43 over the 17 x 2^20 values of test_philox_randn_block_cap (bf16: 0.99, the store
  alone). The CPU mirror (glibc through torch) reaches 0.63 of e (7.3 r + |z|) over 4 images of 2^21 values.
sampler_step_bound, cgs_sampler_step_dev: den = cfg_combine_bound (u given; else den = c, exact), then
  euler_step_bound from the row's (sigma, sigma_down) with noise = normal_bound at stream = step scaled by
  sup = fl(row[2] row[3]), rounded once as the kernel does; the errors of den and of the normals pass through their
  slopes:  tol = (tol_euler + |dt / sigma| tol_den + sup tol_z) (1 + 8e). Returns (ref, tol) of x and of den_out.
timestep_embedding_bound, cos / sin(a), a = t f, f = exp(-x), x = ln P k / half with ln P the fp32 value of logf(P):
  -ln P k and the division by half round once each, __expf multiplies by the fp32 value of log2 e (its rounding and
  that of the product): 4 e x in the exponent, relative after the exponential; v_exp_f32 adds EXP2_REL; t f rounds
  once:  da = |t| f (EXP2_REL + 4 e (1 + x));  tol = da + SINCOSF_REL (|ref| + da);  t = 0: cos 0 = 1 and sin 0 = 0
  are exact, tol = 0. Measured on the MI355X (test_timestep_embedding_bound, all 64 cases): max |y - ref| / tol = 0.35.
silu_bound (cgs_silu, bf16 / fp16): x rcp(1 + __expf(-x)) is the SIG family's x rcp(1 + exp2(x a)) with the product
  by log2 e inside __expf: act_err of the fused epilogues with d_pre = 0, one store in the dtype's u, and tiny(dtype)
  for a result below the dtype's normal range.
upsample_nearest2x moves bits: torch.equal against F.interpolate, no bound.
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -8
E = 2.0 ** -24
C_ACC = 2
GELU_SLOPE = 1.13        # max |gelu'(x)| (1.129 at x = sqrt(2))
GELU_ABS = 2.6e-5        # absolute error bound of gelu_sig (csrc/kernels/common.h)
SILU_SLOPE = 1.1         # max |silu'(x)| (1.0998 at x = 2.4)
# Hardware approximations. None of them is measured here: the figures are the 1 ulp (= 2 e) the CDNA ISA guide
# gives for v_exp_f32, v_rcp_f32 and v_rsq_f32, taken as supposed.
EXP2_REL = 2 * E         # v_exp_f32 (softmax2; __expf in silu_f after one multiply by log2 e)
RCP_REL = 2 * E          # v_rcp_f32 (silu_f)
RSQRT_REL = 4 * E        # rsqrtf (2 e) of var + eps formed by one division and one addition (e each)
# The library functions of the fp32 kernels (f32.hip). No copy of ROCm's HIP math accuracy table is installed beside
# the compiler, so these are supposed as well: 4 ulp for erff, 2 ulp for expf (1 ulp = 2 e).
ERFF_REL = 8 * E         # erff (gelu_f)
EXPF_REL = 4 * E         # expf (the SiLU of gn_f32_apply_kernel)
# rng.hip and timestep_emb_kernel: supposed in the same way, 2 ulp each for logf and for sinf / cosf
LOGF_REL = 4 * E         # logf (normal4)
SINCOSF_REL = 4 * E      # sinf, cosf (normal4, timestep_emb_kernel), relative to a result <= 1
TINY = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -126}


def u(dtype):
    """Unit roundoff of a storage type."""
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}[dtype]


def f64(t):
    return None if t is None else t.detach().to(torch.float64)


def _store(ref, dtype=torch.bfloat16):
    ud = u(dtype)
    return ud * ref.abs() * (1 + 2 * ud)


def rel(a, b):
    """The Frobenius-norm relative error the older kernel tests assert on."""
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-12)).item()


def assert_within(y, ref, tol, what):
    """Print ``what``, max |y - ref| / tol and the share of elements over tol; assert that none is over."""
    y = f64(y)
    assert tuple(y.shape) == tuple(ref.shape) == tuple(tol.shape), (what, y.shape, ref.shape, tol.shape)
    assert bool(torch.isfinite(y).all()), f"{what}: non-finite output"
    diff = (y - ref).abs()
    ratio = diff / tol
    if bool((tol == 0).any()):          # tol = 0: the value must be exact
        ratio = torch.where(tol == 0, torch.where(diff == 0, 0.0, math.inf).to(ratio.dtype), ratio)
    worst = ratio.max().item() if ratio.numel() else 0.0
    over = (ratio > 1).double().mean().item() if ratio.numel() else 0.0
    print(f"BOUND {what}: max |y-ref|/tol {worst:.3f}, share over tol {over:.2e}")
    if over > 0:
        i = int(ratio.reshape(-1).argmax())
        idx = tuple(int(j) for j in torch.unravel_index(torch.tensor(i), ratio.shape))
        raise AssertionError(f"{what}: {over:.3e} of the elements over tol, worst {worst:.3f} x tol at {idx}: "
                             f"y {y[idx].item():.6g} ref {ref[idx].item():.6g} tol {tol[idx].item():.3g}")
    return worst


# ------------------------------------------------------------------------------------------------ GEMM
def _pre_mag(a, w, bias, alpha):
    a, w, bias = f64(a), f64(w), f64(bias)
    pre = alpha * (a @ w.t())
    mag = abs(alpha) * (a.abs() @ w.abs().t())
    if bias is not None:
        pre = pre + bias
        mag = mag + bias.abs()
    return pre, mag


def _alpha(alpha, dtype):
    """float32: alpha as the fp32 value cgs_gemm_f32 is passed."""
    return _f32(alpha) if dtype == torch.float32 else alpha


def gemm_bound(a, w, bias=None, res=None, alpha=1.0, K=None, dtype=torch.bfloat16):
    """out = alpha a w^T + bias + res. a [M, K], w [N, K] (fp8 weights: pass them decoded, the decode is exact).
    dtype: the type the kernel stores (float32: the fp32 kernels of f32.hip, module docstring)."""
    K = a.shape[-1] if K is None else K
    pre, mag = _pre_mag(a, w, bias, _alpha(alpha, dtype))
    ref, tol = pre, 0.0
    if res is not None:
        res = f64(res)
        ref = pre + res
        mag = mag + res.abs()
        tol = u(dtype) * pre.abs()
    return ref, _store(ref, dtype) + tol + C_ACC * K * E * mag


def _geglu_tol(x1, g, d1, dg):
    ref = x1 * F.gelu(g)
    dgelu = GELU_SLOPE * dg + GELU_ABS
    return ref, _store(ref) + F.gelu(g).abs() * d1 + x1.abs() * dgelu + d1 * dgelu


def geglu_bound(a, w, bias=None, K=None):
    """out = x1 * gelu(g) with [x1, g] = a w^T + bias; w [2 No, K] in the plain (not interleaved) row order."""
    K = a.shape[-1] if K is None else K
    h, mag = _pre_mag(a, w, bias, 1.0)
    (x1, g), (m1, mg) = h.chunk(2, dim=-1), mag.chunk(2, dim=-1)
    return _geglu_tol(x1, g, C_ACC * K * E * m1, C_ACC * K * E * mg)


def _lnfold_pre_mag(a, w2, b2, rs, cs):
    """(pre, mag) of rstd (a w2^T - mean cs) + b2 (lnfold_bound); mag also takes |rstd mean cs|."""
    a, w2, b2, rs, cs = f64(a), f64(w2), f64(b2), f64(rs), f64(cs)
    mu, rstd = rs[:, :1], rs[:, 1:2]
    pre = rstd * (a @ w2.t() - mu * cs[None, :])
    mag = rstd.abs() * (a.abs() @ w2.abs().t()) + (rstd * mu * cs[None, :]).abs()
    if b2 is not None:
        pre = pre + b2
        mag = mag + b2.abs()
    return pre, mag


# the sigmoid's argument z of the SIG family, act = x sigmoid(z(x))
_SIG_ARG = {"gelu_tanh": lambda x: 2 * math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3), "quick_gelu": lambda x: 1.702 * x,
            "silu": lambda x: x}


def act_ref(pre, act, param=0.0):
    """The activation set of the fused epilogues (CgsAct, csrc/kernels/common.h) in fp64; ``act`` None: the identity;
    ``param``: the leaky_relu slope, taken as the fp32 value the kernel is passed."""
    pre = f64(pre)
    if act is None:
        return pre
    if act == "gelu":
        return F.gelu(pre)
    if act in _SIG_ARG:
        return pre * torch.sigmoid(_SIG_ARG[act](pre))
    if act == "relu":
        return pre.clamp_min(0.0)
    assert act == "leaky_relu", act
    return torch.where(pre >= 0, pre, pre * _f32(param))


def _gelu_f_err(pre, y):
    """gelu_f (common.h), 0.5f x (1 + erff(x fl(1 / sqrt 2))), against the exact function (module docstring)."""
    t = pre / math.sqrt(2.0)
    d_erf = 2 / math.sqrt(math.pi) * torch.exp(-t * t) * t.abs() * 2 * E + ERFF_REL * torch.erf(t).abs()
    return 0.5 * pre.abs() * (d_erf + E * torch.erfc(-t)) + 2 * E * y.abs()


def _act_tol(pre, d_pre, res, act, param, dtype=torch.bfloat16):
    """(ref, tol) of round(act(pre)) (+ res) for a pre-activation within d_pre of pre (module docstring)."""
    y = act_ref(pre, act, param)
    if dtype == torch.float32 and act is not None:
        d_pre = d_pre + E * pre.abs()            # f32.hip: fmaf(acc, alpha, bias) rounds once before the activation
    if act is None:
        slope, err = 1.0, 0.0
    elif act == "gelu" and dtype == torch.float32:
        slope, err = GELU_SLOPE, _gelu_f_err(pre, y)
    elif act == "gelu":
        slope, err = GELU_SLOPE, GELU_ABS
    elif act in _SIG_ARG:
        slope = GELU_SLOPE if act == "gelu_tanh" else SILU_SLOPE
        err = (4 * _SIG_ARG[act](pre).abs() * E + EXP2_REL + RCP_REL + 2 * E) * y.abs() + 1e-36
    else:
        slope = 1.0 if act == "relu" else max(1.0, abs(_f32(param)))
        err = E * y.abs() if act == "leaky_relu" else 0.0
    ref, d = y, slope * d_pre + err
    if res is not None:
        ref = y + f64(res)
        d = d + u(dtype) * y.abs()
    return ref, _store(ref, dtype) + d * (1 + u(dtype))


def gemm_act_bound(a, w, bias, res, act, param=0.0, alpha=1.0, K=None, rs=None, cs=None, dtype=torch.bfloat16):
    """out = round(act(alpha a w^T + bias)) (+ res); with rs / cs the pre-activation is lnfold_bound's (w = w2, bias =
    b2, alpha ignored). The fp32 addition of the residual is part of mag, as in gemm_bound. dtype: as gemm_bound."""
    K = a.shape[-1] if K is None else K
    pre, mag = _pre_mag(a, w, bias, _alpha(alpha, dtype)) if rs is None else _lnfold_pre_mag(a, w, bias, rs, cs)
    if res is not None:
        mag = mag + f64(res).abs()
    return _act_tol(pre, C_ACC * K * E * mag, res, act, param, dtype)


def lnfold_bound(a, w2, b2, rs, cs, geglu=False):
    """The LayerNorm-folded GEMM from the operands the kernel is given: out = rstd (a w2^T - mean cs) + b2, with
    rs [M, 2] = (mean, rstd) per row, w2 = W gamma (bf16), cs = rowsum(w2) (fp32), b2 (bf16). Judges the kernel's
    arithmetic only; mag also takes |rstd mean cs|. geglu: w2 / cs / b2 in the plain row order."""
    K = a.shape[-1]
    ref, mag = _lnfold_pre_mag(a, w2, b2, rs, cs)
    if geglu:
        (x1, g), (m1, mg) = ref.chunk(2, dim=-1), mag.chunk(2, dim=-1)
        return _geglu_tol(x1, g, C_ACC * K * E * m1, C_ACC * K * E * mg)
    return ref, _store(ref) + C_ACC * K * E * mag


# ------------------------------------------------------------------------------------------------ conv
def _conv_pre_mag(x, w, bias, stride, pad, upsample2x, x2):
    """(pre, mag, K) of conv2d(x (cat x2) (nearest 2x), w) + bias in NCHW; K = Cin kh kw."""
    x, w, bias = f64(x), f64(w), f64(bias)
    if x2 is not None:
        x = torch.cat([x, f64(x2)], 1)
    if upsample2x:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    K = w.shape[1] * w.shape[2] * w.shape[3]
    pre = F.conv2d(x, w, bias, stride, pad)
    mag = F.conv2d(x.abs(), w.abs(), None if bias is None else bias.abs(), stride, pad)
    return pre, mag, K


def conv_act_bound(x, w, bias, res, act, param=0.0, stride=1, pad=0, upsample2x=False, x2=None,
                   dtype=torch.bfloat16):
    """out = round(act(conv2d(x (cat x2) (nearest 2x), w) + bias)) (+ res) in NCHW: gemm_act_bound on conv_bound's
    pre-activation."""
    pre, mag, K = _conv_pre_mag(x, w, bias, stride, pad, upsample2x, x2)
    if res is not None:
        mag = mag + f64(res).abs()
    return _act_tol(pre, C_ACC * K * E * mag, res, act, param, dtype)


def conv_bound(x, w, bias=None, res=None, stride=1, pad=0, upsample2x=False, x2=None, dtype=torch.bfloat16):
    """out = conv2d(x (cat x2) (nearest 2x), w) + bias + res in NCHW; K = Cin kh kw. dtype: as gemm_bound."""
    pre, mag, K = _conv_pre_mag(x, w, bias, stride, pad, upsample2x, x2)
    res = f64(res)
    ref, tol = pre, 0.0
    if res is not None:
        ref = pre + res
        mag = mag + res.abs()
        tol = u(dtype) * pre.abs()
    return ref, _store(ref, dtype) + tol + C_ACC * K * E * mag


# ------------------------------------------------------------------------------------------------ attention
def attention_probs(q, k, heads, causal=False, key_padding=None):
    """fp64 softmax(q k^T / sqrt(D)) per head: [B, H, Sq, Sk]. causal: key j <= query i; key_padding bool
    [B, Sk], True = attend."""
    B, Sq, HD = q.shape
    Sk, D = k.shape[1], HD // heads
    qh = f64(q).reshape(B, Sq, heads, D).transpose(1, 2)
    kh = f64(k).reshape(B, Sk, heads, D).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(D)
    if causal:
        keep = torch.ones(Sq, Sk, dtype=torch.bool, device=s.device).tril()
        s = s.masked_fill(~keep, -math.inf)
    if key_padding is not None:
        s = s.masked_fill(~key_padding.bool()[:, None, None, :], -math.inf)
    return torch.softmax(s, -1)


def attention_bound(q, k, v, heads, causal=False, key_padding=None, extra_roundings=0):
    """q [B, Sq, H D], k / v [B, Sk, H D] -> [B, Sq, H D]."""
    B, Sq, HD = q.shape
    Sk, D = k.shape[1], HD // heads
    p = attention_probs(q, k, heads, causal, key_padding)
    vh = f64(v).reshape(B, Sk, heads, D).transpose(1, 2)
    ref = (p @ vh).transpose(1, 2).reshape(B, Sq, HD)
    A = (p @ vh.abs()).transpose(1, 2).reshape(B, Sq, HD)
    return ref, _store(ref) + (2 + extra_roundings) * U * A + 1e-6


# ------------------------------------------------------------------------------------------------ norms
def _store_dt(ref, d, dtype):
    """One round to ``dtype`` of a value within d of ref."""
    ud = u(dtype)
    return ud * ref.abs() * (1 + 2 * ud) + TINY[dtype] + d * (1 + ud)


def _silu(pre, d):
    """silu_f(f) = f * rcp(1 + __expf(-f)): exp2 of fl(f log2 e) (|f| e in the exponent, relative after exp), the
    addition of 1, the reciprocal, the product. The error of the denominator is at most that of its exp term.
    1e-36: below f = -87 __expf overflows and the kernel returns 0 for |silu(f)| < 1e-36."""
    ref = F.silu(pre)
    rel = (pre.abs() + 1) * E + EXP2_REL + E + RCP_REL + E
    return ref, SILU_SLOPE * d + rel * ref.abs() + 1e-36


def _silu_div(pre, d):
    """o / (1.0f + expf(-o)) (gn_f32_apply_kernel): expf, the addition of 1 and a true division, e each; the error
    of the denominator is at most that of its exp term. 1e-36: expf overflows below o = -88 and o / inf = 0."""
    ref = F.silu(pre)
    return ref, SILU_SLOPE * d + (EXPF_REL + 2 * E) * ref.abs() + 1e-36


def _gn_values(x, pre_add, x2):
    x = f64(x)
    if x2 is not None:
        x = torch.cat([x, f64(x2)], 1)
    N, C = x.shape[:2]
    pre = torch.zeros(N, C, dtype=torch.float64, device=x.device) if pre_add is None else f64(pre_add)
    return x, pre


def gn_depth(HW, Cg, ppb):
    """(Lb, L) of the GroupNorm statistics kernels for blocks of ppb pixels (csrc/kernels/norm.hip): a lane sums
    every fourth pixel of its block (ceil(ppb / 4) additions), 3 shuffle additions of the pixel-packed forms, the
    division and the subtraction of s2 - s1^2 / cnt; then the 4 waves are merged, a finalize thread merges
    ceil(Cg nb / 256) partials in sequence, and 6 shuffle and 3 LDS merges end the tree."""
    nb = (HW + ppb - 1) // ppb
    Lb = (ppb + 3) // 4 + 5
    return Lb, Lb + 4 + (Cg * nb + 255) // 256 + 9


def gn_f32_form(N, HW, C):
    """(S, P) of cgs_groupnorm_f32 (f32.hip): S = gn_slices(N, HW) pixel slices an image, slice s over the pixels
    [HW s // S, HW (s + 1) // S); P pixel lanes per float4 channel chunk in gn_f32_partial_kernel."""
    S = max(1, min((2048 + N - 1) // N, HW // 32))
    C4 = C // 4
    return S, 1 if C4 >= 256 else 256 // C4


def gn_f32_bounds(N, HW, C):
    S = gn_f32_form(N, HW, C)[0]
    return [HW * s // S for s in range(S + 1)]


def gn_f32_depth(N, HW, C, G, pre_add=False):
    """(Lb, L) of the three kernels of cgs_groupnorm_f32. Partial kernel: a lane adds every P-th pixel of its slice,
    ceil(cnt / P) shifted additions in sequence, + 3 for the rounding of d = v - sft, sum mu and ssq - sum mu; then the
    P - 1 Chan merges of the pixel lanes in sequence. Finalize kernel: a thread adds ceil(S cpg / 256) partials in
    sequence, wave_sum (6), the 4-wave sum (3); the M2 pass has the same depth. pre_add: v = fl(x + pre_add) (gn_ld)
    moves the data by e |v|, one more step of R."""
    S, P = gn_f32_form(N, HW, C)
    b = gn_f32_bounds(N, HW, C)
    cnt = max(b1 - b0 for b0, b1 in zip(b, b[1:]))
    Lb = (cnt + P - 1) // P + 3
    return Lb, Lb + (P - 1) + (S * (C // G) + 255) // 256 + 9 + (1 if pre_add else 0)


def _gn_stats(x, pre, groups, ppb=None, bounds=None, depth=None):
    """fp64 (mean, var) per (n, g) of v = x + pre and their worst-case fp32 errors; all [N, G, 1]. The statistics
    blocks: ppb pixels each with gn_depth's (Lb, L), or the pixel boundaries ``bounds`` with ``depth`` = (Lb, L)."""
    N, C, H, W = x.shape
    v = (x + pre[:, :, None, None]).reshape(N, groups, -1)
    n = v.shape[-1]
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    dev2 = ((v - mean) ** 2).amax(-1, keepdim=True)
    R = v.abs().amax(-1, keepdim=True) + 3 * (v.amax(-1, keepdim=True) - v.amin(-1, keepdim=True))
    if ppb is None and bounds is None:
        Lb = L = n
        E2 = 2 * var + 2 * dev2
    else:
        if bounds is None:
            Lb, L = gn_depth(H * W, C // groups, ppb)
            bounds = list(range(0, H * W, ppb)) + [H * W]
        else:
            Lb, L = depth
        xr = x.reshape(N, C, H * W)
        d2 = torch.cat([(xr[:, :, p0:p1] - xr[:, :, p0:p0 + 1]) ** 2 for p0, p1 in zip(bounds, bounds[1:]) if p1 > p0], -1)
        E2 = d2.reshape(N, groups, -1).mean(-1, keepdim=True)
    dmean = L * E * R
    dvar = 2 * Lb * E * E2 + 8 * L * E * var + 4 * var.sqrt() * dmean + dmean ** 2
    return n, mean, var, dmean, dvar


def _per_channel(t, C):
    """[N, G, 1] -> [N, C, 1, 1]."""
    N, G = t.shape[:2]
    return t.reshape(N, G, 1).repeat_interleave(C // G, dim=1).reshape(N, C, 1, 1)


def _gn_out(x, pre, mean, rstd, dmean, drstd_rel, w, b, silu, dtype):
    N, C = x.shape[:2]
    one = torch.ones(C, dtype=torch.float64, device=x.device)
    gam = (one if w is None else f64(w))[None, :, None, None]
    bet = (0 * one if b is None else f64(b))[None, :, None, None]
    mean, rstd, dmean, drstd_rel = (_per_channel(t, C) for t in (mean, rstd, dmean, drstd_rel))
    pre = pre[:, :, None, None]
    zg = (x + pre - mean) * rstd * gam
    ref = zg + bet
    a = (rstd * gam).abs()
    mag = x.abs() * a + (mean.abs() + pre.abs()) * a + bet.abs()
    d = a * dmean + zg.abs() * drstd_rel + 6 * E * mag
    if silu:
        ref, d = _silu_div(ref, d) if silu == "div" else _silu(ref, d)
    return ref, _store_dt(ref, d, dtype)


def groupnorm_f32_bound(x, groups, w, b, eps, silu, pre_add=None, x2=None):
    """cgs_groupnorm_f32 on fp32 x [N, C1, H, W] (cat x2): the statistics over the kernel's own slices (gn_f32_form,
    gn_f32_depth), the stored a = gamma rstd and b = beta - mean a, fmaf(v, a, b) and the SiLU with a division."""
    x, pre = _gn_values(x, pre_add, x2)
    N, C, H, W = x.shape
    n, mean, var, dmean, dvar = _gn_stats(x, pre, groups, bounds=gn_f32_bounds(N, H * W, C),
                                          depth=gn_f32_depth(N, H * W, C, groups, pre_add is not None))
    rstd = 1 / torch.sqrt(var + eps)
    return _gn_out(x, pre, mean, rstd, dmean, 0.5 * dvar / (var + eps) + RSQRT_REL, w, b, "div" if silu else False,
                   torch.float32)


def groupnorm_bound(x, groups, w, b, eps, silu, pre_add=None, x2=None, ppb=None):
    """GroupNorm (+ SiLU) of cat([x, x2], 1) + pre_add[:, :, None, None]; x [N, C, H, W], pre_add [N, C]. ppb: the
    pixels per statistics block of the kernel that ran (None: a reduction of unknown structure)."""
    dtype = x.dtype
    x, pre = _gn_values(x, pre_add, x2)
    n, mean, var, dmean, dvar = _gn_stats(x, pre, groups, ppb)
    rstd = 1 / torch.sqrt(var + eps)
    return _gn_out(x, pre, mean, rstd, dmean, 0.5 * dvar / (var + eps) + RSQRT_REL, w, b, silu, dtype)


def groupnorm_stats_bound(x, groups, pre_add=None, x2=None, ppb=None):
    """The fp32 (mean, M2) per (n, g): [N, G, 2]."""
    x, pre = _gn_values(x, pre_add, x2)
    n, mean, var, dmean, dvar = _gn_stats(x, pre, groups, ppb)
    ref = torch.cat([mean, n * var], -1)
    tol = torch.cat([dmean + E * mean.abs(), n * dvar + E * n * var], -1) + TINY[torch.float32]
    return ref, tol


def groupnorm_apply_bound(x, groups, w, b, mean_rstd, silu, pre_add=None, x2=None):
    """The apply pass with given fp32 (mean, rstd) [N, G, 2]: no statistics term."""
    dtype = x.dtype
    x, pre = _gn_values(x, pre_add, x2)
    mr = f64(mean_rstd).reshape(x.shape[0], groups, 2)
    zero = torch.zeros_like(mr[..., :1])
    return _gn_out(x, pre, mr[..., :1], mr[..., 1:], zero, zero, w, b, silu, dtype)


def ln_depth(C):
    """Dependent fp32 additions of a row sum in the LayerNorm kernels (csrc/kernels/norm.hip): a lane adds at most
    LN_MAXK = 8 vectors of 8 values in sequence, then a butterfly over at most 64 lanes; rows over 4096 take the
    scalar kernel, C / 64 values per lane."""
    return min(C, 64 + 6) if C <= 4096 else (C + 63) // 64 + 6


def ln_f32_depth(C):
    """ln_f32_kernel (f32.hip), one wave per row: a lane adds ceil(C / 256) float4s in sequence, each summed as
    (x + y) + (z + w) (2), then wave_sum (6)."""
    return (C + 255) // 256 + 2 + 6


def _ln_stats(x, eps, depth=None):
    """Two-pass row statistics of x [rows, C] in fp64 and their worst-case fp32 errors; all [rows, 1]. depth: the
    dependent additions of a row sum where they are not ln_depth's."""
    C = x.shape[-1]
    L = ln_depth(C) if depth is None else depth
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    dmean = C_ACC * L * E * x.abs().mean(-1, keepdim=True) + E * mean.abs()
    dvar = C_ACC * (L + 4) * E * var + dmean ** 2
    rstd = 1 / torch.sqrt(var + eps)
    return mean, rstd, dmean, 0.5 * dvar / (var + eps) + RSQRT_REL


def layernorm_bound(x, w=None, b=None, eps=1e-5, depth=None):
    """LayerNorm over the last dim; weight and bias optional. depth = ln_f32_depth(C) for cgs_layernorm_f32."""
    dtype, shape = x.dtype, x.shape
    x = f64(x).reshape(-1, shape[-1])
    mean, rstd, dmean, drstd_rel = _ln_stats(x, eps, depth)
    wa = torch.ones(shape[-1], dtype=torch.float64, device=x.device) if w is None else f64(w)
    ba = 0 * wa if b is None else f64(b)
    zw = (x - mean) * rstd * wa
    ref = zw + ba
    d = wa.abs() * rstd * dmean + zw.abs() * drstd_rel + 6 * E * (zw.abs() + ba.abs())
    return ref.reshape(shape), _store_dt(ref, d, dtype).reshape(shape)


def layernorm_stats_bound(x, eps):
    """The fp32 (mean, rstd) per row: [rows, 2]."""
    x = f64(x).reshape(-1, x.shape[-1])
    mean, rstd, dmean, drstd_rel = _ln_stats(x, eps)
    return torch.cat([mean, rstd], -1), torch.cat([dmean, rstd * drstd_rel], -1) + TINY[torch.float32]


def rs_from_partials_bound(part, eps):
    """(mean, rstd) [M, 2] from part [M, P, 2]: the fp32 (mean, M2) of P groups of 80 columns each."""
    part = f64(part)
    P = part.shape[1]
    m, q = part[..., 0], part[..., 1]
    mean = m.mean(-1, keepdim=True)
    dev = (m - mean).abs().amax(-1, keepdim=True)
    m2 = q.sum(-1, keepdim=True) + 80 * ((m - mean) ** 2).sum(-1, keepdim=True)
    dmean = C_ACC * P * E * (mean.abs() + 4 * dev) + E * mean.abs()
    dm2 = C_ACC * (P + 6) * E * m2 + 320 * P * dev * dmean
    var = m2 / (80 * P)
    rstd = 1 / torch.sqrt(var + eps)
    drstd = rstd * (0.5 * dm2 / (80 * P) / (var + eps) + RSQRT_REL)
    return torch.cat([mean, rstd], -1), torch.cat([dmean, drstd], -1) + TINY[torch.float32]


def partials_merge_tol(part, tol, eps):
    """[M, 2]: how far the (mean, rstd) that part [M, P, 2] stands for move when every partial moves within tol
    [M, P, 2]: mean = mean_p m_p, M2 = sum q_p + 80 sum (m_p - mean)^2, to second order in the means' errors;
    drstd = rstd dM2 / (2 n (var + eps))."""
    part, tol = f64(part), f64(tol)
    m, q, dm, dq = part[..., 0], part[..., 1], tol[..., 0], tol[..., 1]
    n = 80 * m.shape[1]
    mean, dmean = m.mean(-1, keepdim=True), dm.mean(-1, keepdim=True)
    dev, dd = (m - mean).abs(), dm + dmean
    m2 = q.sum(-1, keepdim=True) + 80 * (dev ** 2).sum(-1, keepdim=True)
    dm2 = dq.sum(-1, keepdim=True) + 80 * (2 * dev * dd + dd ** 2).sum(-1, keepdim=True)
    var = m2 / n
    return torch.cat([dmean, 0.5 * dm2 / n / (var + eps) / torch.sqrt(var + eps)], -1)


RSO_LB = 7              # five trees of four (2) added in sequence (5): the lane sums of pq::run RSO
# the 20 columns of an 80-column chunk that lane fq of a row's four holds (colj, mfma_pp160.h), its first value first
RSO_LANE_COLS = [[32 * p + 8 * fq + t for p in (0, 1) for t in range(8)] + [64 + 4 * fq + t for t in range(4)]
                 for fq in range(4)]


def rowstats_partials_bound(y):
    """The fp32 (mean, M2) [M, N / 80, 2] of every 80-column chunk of every row of the stored y [M, N] (pq::run RSO):
    judges the statistics arithmetic only (module docstring)."""
    y = f64(y)
    M, N = y.shape
    assert N % 80 == 0, N
    v = y.reshape(M, N // 80, 80)
    idx = torch.tensor(RSO_LANE_COLS, device=y.device)
    lv = v[..., idx]                                          # [M, P, 4 lanes, 20]
    d = lv - lv[..., :1]
    S, s2 = d.abs().sum(-1), (d * d).sum(-1)
    mean = lv.mean(-1)
    q = ((lv - mean[..., None]) ** 2).sum(-1)
    dmean = (RSO_LB + 3) * E * S / 20 + torch.minimum(E * mean.abs(), S / 20)
    dq = (3 * RSO_LB + 7) * E * s2
    n = 20
    while mean.shape[-1] > 1:                                 # lanes l ^ 16 (fq 0-1, 2-3), then l ^ 32
        ma, mb, qa, qb = mean[..., 0::2], mean[..., 1::2], q[..., 0::2], q[..., 1::2]
        dd, delta = (mb - ma).abs(), dmean[..., 0::2] + dmean[..., 1::2]
        mean = 0.5 * (ma + mb)
        q = qa + qb + dd * dd * (n / 2)
        dmean = 0.5 * delta + torch.minimum(E * mean.abs(), 0.5 * (dd + delta))
        dq = dq[..., 0::2] + dq[..., 1::2] + n * dd * delta + 0.5 * n * delta ** 2 + 4 * E * dd * dd * (n / 2) + 2 * E * q
        n *= 2
    ref = torch.cat([mean, q], -1)
    return ref, torch.cat([dmean, dq], -1) + TINY[torch.float32]


def sumsq_partials_bound(y, hw):
    """The fp32 sums of squares [M / 64, N] of the stored y [M, N] over each 64-row block (pq::run GNS == 2); hw = rows
    per image, a multiple of 64, so block m / 64 of the tensor is block (m % hw) / 64 of image m / hw."""
    y = f64(y)
    M, N = y.shape
    assert hw % 64 == 0 and M % hw == 0, (M, hw)
    ref = (y * y).reshape(M // 64, 64, N).sum(1)
    return ref, torch.where(ref == 0, 0.0, C_ACC * (8 + 1) * E * ref + 64 * TINY[torch.float32])


def gn_partials_bound(y_nhwc):
    """The fp32 (mean, M2) [N, HW / 64, C, 2] of each 64-pixel block of the stored y [N, ..., C] (pq::run GNS == 1)."""
    y = f64(y_nhwc)
    N, C = y.shape[0], y.shape[-1]
    v = y.reshape(N, -1, 64, C)
    L = 7
    mean = v.mean(2)
    m2 = ((v - mean[:, :, None]) ** 2).sum(2)
    dmean = C_ACC * L * E * v.abs().mean(2) + E * mean.abs()
    dm2 = C_ACC * (L + 4) * E * m2 + 64 * dmean ** 2
    return torch.stack([mean, m2], -1), torch.stack([dmean, dm2], -1) + TINY[torch.float32]


def affine_layernorm_bound(x, scale, shift, add, eps, xa):
    """xa = x (add + scale[n]) + shift[n] (one fp32 addition, one fma, one round) and y = LayerNorm(xa) without
    affine. x [N, ..., C]; scale / shift [N, C]; xa: the tensor the kernel stored, whose LayerNorm y is.
    Returns (xa_ref, xa_tol, y_ref, y_tol)."""
    N, C = x.shape[0], x.shape[-1]
    shp = (N,) + (1,) * (x.dim() - 2) + (C,)
    xd, sc, sh = f64(x), add + f64(scale).reshape(shp), f64(shift).reshape(shp)
    ref = xd * sc + sh
    d = E * (xd * sc).abs() + E * ref.abs()
    y_ref, y_tol = layernorm_bound(xa, None, None, eps)
    return ref, _store_dt(ref, d, x.dtype), y_ref, y_tol


# ------------------------------------------------------------------------------------------------ depthwise conv
def dwconv_bound(x, w_kkc, bias, k, replicate=False):
    """Depthwise k x k conv, stride 1, 'same' zeros or replicate padding. x [N, H, W, C], w_kkc [k k, C]. The
    LayerNorm statistics the fused kernel adds are those of its stored output: layernorm_stats_bound(y, eps)."""
    C = x.shape[-1]
    xn = f64(x).permute(0, 3, 1, 2)
    wt = f64(w_kkc).t().reshape(C, 1, k, k)
    b = f64(bias)
    xp = F.pad(xn, (k // 2,) * 4, mode="replicate" if replicate else "constant")
    ref = F.conv2d(xp, wt, b, 1, 0, 1, C)
    mag = F.conv2d(xp.abs(), wt.abs(), None if b is None else b.abs(), 1, 0, 1, C)
    ref, mag = ref.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)
    return ref, _store_dt(ref, C_ACC * (k * k + 1) * E * mag, x.dtype)


# ------------------------------------------------------------------------------------------------ softmax2
def softmax2_bound(x):
    """p = 2^(x - max) / sum over the last dim of fp32 x, stored as bf16."""
    x = f64(x)
    cols = x.shape[-1]
    mx = x.amax(-1, keepdim=True)
    p = torch.exp2(x - mx)
    ref = p / p.sum(-1, keepdim=True)
    dist = torch.where(torch.isfinite(x), (x - mx).abs(), torch.zeros_like(x))        # -inf: p = 0, not inf * 0
    rel = C_ACC * cols * E + 2 * EXP2_REL + 14 * E + dist * E * math.log(2.0)
    tol = _store_dt(ref, rel * ref, torch.bfloat16)
    return ref, torch.where(torch.isfinite(x), tol, torch.zeros_like(tol))


# ------------------------------------------------------------------------------------------------ GRN
# (N, HW, C) -> the apply form cgs_grn_nhwc_v2 runs at the default cgs_grn_set_rows(1); the smallest shapes that reach
# N > 4 with a bsum tail and a slice tail, N = GRN_MAXN, both sides of the row-tiled predicate (257 and 204 chunks a
# row just miss it, 256 and 205 just meet it), idle threads in the last block of a row (461 chunks)
GRN_V2_SHAPES = {(1, 1, 8): "grid", (5, 35, 264): "grid", (64, 17, 72): "grid", (3, 33, 2056): "grid",
                 (2, 17, 2048): "rows", (2, 16, 1640): "rows", (2, 33, 3688): "rows", (1, 70, 1632): "grid"}
GRN_GNS_SHAPES = [(5, 64, 264), (2, 320, 2048)]
# (input shape, output size) of the resize tests
RESIZE_CASES = [((2, 3, 5, 7), s) for s in [(1, 1), (9, 4), (5, 7), (13, 16), (1, 16), (9, 1)]] + \
               [((1, 2, 1, 1), (3, 2)), ((1, 1, 16, 18), (5, 7))]
RESIZE_MODES = [("nearest", None), ("nearest-exact", None), ("bilinear", False), ("bilinear", True),
                ("bicubic", False), ("bicubic", True), ("area", None)]
GRN_MAXN = 64
GRN_K = 5                # fp32 roundings from (gx, inv) to the value that is stored, the same in every form


def grn_slices(N, HW, C):
    """cgs_grn_slices (image.hip): about 512 pass-1 blocks, at least 16 rows a slice, a multiple of 4."""
    cb = (C // 8 + 63) // 64
    s = min((512 + N * cb - 1) // (N * cb), (HW + 15) // 16)
    return max((s + 3) & ~3, 4)


def grn_row_tiled(HW, C, rows=1):
    """The predicate of grn_apply_launch: the row-tiled apply where at most 20 % of a block's threads idle."""
    rt = {1: 16, 2: 32}.get(rows, 64)
    cpr = C // 8
    groups = (cpr + 255) // 256
    return bool(rows) and (HW + rt - 1) // rt <= 65535 and cpr * 5 >= groups * 1024


def grn_depth(form, N, HW, C):
    """(L, Lm): the dependent fp32 additions of the sum of squares and of the channel mean (module docstring)."""
    nblk = (C + 255) // 256
    Lm = 6 + 2 + (nblk + 63) // 64 + 6
    if form == "v2":
        S = grn_slices(N, HW, C)
        return ((HW + S - 1) // S + 3) // 4 + 2 + S // 4 + 2, Lm
    if form == "gns":
        nbk = HW // 64
        return nbk // 4 + nbk % 4 + 2, Lm
    assert form == "v1", form
    return HW, nblk + 8


def grn_inputs(N, HW, C, dtype, device="cpu", seed=0):
    """x [N, HW, C] = randn s_n s_c with s_n log-spaced over 0.05 .. 8 and s_c over 0.03 .. 10, both permuted; the
    largest s_c is raised until its channel holds nx >= 5 (as far as C allows); one channel of zeros and one of
    -(6 + |randn|) (its GELU is below GELU_ABS); gamma ~ N(0, 0.5) with three entries at -1 / nx of image 0, where
    1 + gamma nx passes near 0; beta ~ N(0, 0.1). Returns (x, gamma, beta, (zero channel, negative channel))."""
    g = torch.Generator().manual_seed(seed)
    s_n = torch.logspace(math.log10(0.05), math.log10(8.0), N)[torch.randperm(N, generator=g)]
    if N == 1:
        s_n = torch.ones(1)
    s_c = torch.logspace(math.log10(0.03), math.log10(10.0), C)[torch.randperm(C, generator=g)]
    x = torch.randn(N, HW, C, generator=g) * s_n[:, None, None] * s_c[None, None, :]
    order = torch.argsort(s_c)
    cz, cn, ctop = int(order[0]), int(order[1]), int(order[-1])
    x[:, :, cz] = 0.0
    x[:, :, cn] = -(6.0 + torch.randn(N, HW, generator=g).abs())
    if C > 6:                                # nx_top = C g_top / (g_top + rest) >= 6  <=>  g_top >= 6 rest / (C - 6)
        gn = x.pow(2).sum(1).sqrt()
        rest = gn.sum(1) - gn[:, ctop]
        x[:, :, ctop] *= (6 * rest / ((C - 6) * gn[:, ctop].clamp_min(1e-30))).clamp_min(1.0)[:, None]
    x = x.to(dtype)
    gx = x.double().pow(2).sum(1).sqrt()
    nx0 = (gx / (gx.mean(1, keepdim=True) + 1e-6))[0]
    gamma = torch.randn(C, generator=g) * 0.5
    for c in torch.argsort(nx0, descending=True)[:3].tolist():
        if nx0[c] > 0.05:
            gamma[c] = -1.0 / nx0[c].item()
    beta = torch.randn(C, generator=g) * 0.1
    return x.to(device), gamma.to(dtype).to(device), beta.to(dtype).to(device), (cz, cn)


def grn_nx(x, pre_gelu=False):
    """fp64 nx [N, C] of x [N, HW, C]."""
    a = F.gelu(f64(x)) if pre_gelu else f64(x)
    gx = a.pow(2).sum(1).sqrt()
    return gx / (gx.mean(1, keepdim=True) + 1e-6)


def _grn_act(x, pre_gelu):
    x = f64(x)
    x = x.reshape(x.shape[0], -1, x.shape[-1])
    return x, (F.gelu(x) if pre_gelu else x)


def grn_stats_bound(x, pre_gelu, depth, part=None):
    """(gx, dgx, inv, dinv): the fp32 gx [N, C] and the per-image inv = 1 / (mean_C gx + 1e-6) [N] with their
    tolerances. x [N, HW, C] or [N, H, W, C]; depth = grn_depth(form, ...). part [N, nbk, C]: the fp32 block sums of
    squares the GNS forms are given instead of x."""
    L, Lm = depth
    if part is not None:
        ss = f64(part).sum(1)
        exact = (f64(part) == 0).all(1)
        HW = 0
    else:
        x, a = _grn_act(x, pre_gelu)
        HW = x.shape[1]
        ss = a.pow(2).sum(1)
        exact = (x == 0).all(1)
    gx = ss.sqrt()
    dgx = gx * (0.5 * C_ACC * (L + 1) * E + E) + TINY[torch.float32]
    if pre_gelu:
        dgx = dgx + math.sqrt(HW) * GELU_ABS
    dgx = torch.where(exact, torch.zeros_like(dgx), dgx)
    mean = gx.mean(1)
    dmean = dgx.mean(1) + C_ACC * Lm * E * mean
    inv = 1 / (mean + 1e-6)
    return gx, dgx, inv, inv * (dmean * inv + 4 * E)


def _grn_out(a, gamma, beta, nx, dnx, pre_gelu, k, dtype, shape):
    g, b = f64(gamma).reshape(1, 1, -1), f64(beta).reshape(1, 1, -1)
    gn = g * nx[:, None, :]
    ref = b + a * (1 + gn)
    d = (a * g).abs() * dnx[:, None, :] + k * E * (b.abs() + a.abs() * (1 + gn.abs()))
    if pre_gelu:
        d = d + GELU_ABS * (1 + gn).abs()
    return ref.reshape(shape), _store_dt(ref, d, dtype).reshape(shape)


def grn_bound(x, gamma, beta, pre_gelu, depth, k=GRN_K):
    """y = beta + a (1 + gamma nx), a = x or gelu(x), with the statistics error of the form that ran."""
    gx, dgx, inv, dinv = grn_stats_bound(x, pre_gelu, depth)
    _, a = _grn_act(x, pre_gelu)
    dnx = dgx * inv[:, None] + gx * dinv[:, None] + dgx * dinv[:, None]
    return _grn_out(a, gamma, beta, gx * inv[:, None], dnx, pre_gelu, k, x.dtype, x.shape)


def _grn_given(gx, bsum=None, inv=None):
    """nx and dnx from the fp32 gx [N, C] and block sums [N, nblk] a kernel is given (or the inv [N] they stand for)."""
    gx = f64(gx)
    C = gx.shape[1]
    nblk = (C + 255) // 256
    inv = 1 / (f64(bsum).sum(1) / C + 1e-6) if inv is None else f64(inv)
    nx = gx * inv[:, None]
    return nx, nx * (C_ACC * ((nblk + 63) // 64 + 6) * E + 4 * E)


def grn_apply_bound(x, gamma, beta, gx, bsum, pre_gelu=False, k=GRN_K):
    """The apply pass with given fp32 gx [N, C] and bsum [N, ceil(C / 256)]: no statistics term."""
    nx, dnx = _grn_given(gx, bsum)
    _, a = _grn_act(x, pre_gelu)
    return _grn_out(a, gamma, beta, nx, dnx, pre_gelu, k, x.dtype, x.shape)


def grn_scale_weight_bound(W, gamma, gx, inv):
    """Wn [N, O, K] = W (1 + gamma nx_n) in bf16 from the fp32 gx [N, K] and inv [N] = 1 / (mean_K gx + 1e-6) in fp64
    from the ceil(K / 256) block sums the kernel is given."""
    nx, dnx = _grn_given(gx, inv=inv)
    Wd, g = f64(W)[None], f64(gamma).reshape(1, 1, -1)
    gn = g * nx[:, None, :]
    ref = Wd * (1 + gn)
    d = (Wd * g).abs() * dnx[:, None, :] + 4 * E * Wd.abs() * (1 + gn.abs())
    return ref, _store_dt(ref, d, torch.bfloat16)


# ------------------------------------------------------------------------------------------------ resize
CUBIC_A = -0.75
CUBIC_SLOPE = 1.35       # max |d w / d t| of the cubic convolution weights with A = -0.75 (cubic1 at t = 0.6)
CUBIC_ABS = 64 * E       # Horner evaluation of one weight in fp32


def _cubic1(t):
    return ((CUBIC_A + 2) * t - (CUBIC_A + 3)) * t * t + 1


def _cubic2(t):
    return ((CUBIC_A * t - 5 * CUBIC_A) * t + 8 * CUBIC_A) * t - 4 * CUBIC_A


def resize_coords(n_in, n_out, mode, align):
    """fp64 source coordinates of one axis, before any clamp (nearest modes: the value that is floored)."""
    o = torch.arange(n_out, dtype=torch.float64)
    if mode in ("bilinear", "bicubic") and align:
        return o * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    if mode == "nearest":
        return o * (n_in / n_out)
    if mode == "nearest-exact":
        return (o + 0.5) * (n_in / n_out)
    return (o + 0.5) * (n_in / n_out) - 0.5


def _resize_axis(n_in, n_out, mode, align):
    """(W, S, k, dw) of one axis: weights [n_out, n_in], tap counts, roundings, weight error."""
    Wm, S = torch.zeros(n_out, n_in, dtype=torch.float64), torch.zeros(n_out, n_in, dtype=torch.float64)
    if mode == "area":
        cnt = 0
        for o in range(n_out):
            a, b = o * n_in // n_out, -((-(o + 1) * n_in) // n_out)
            Wm[o, a:b] = 1.0 / (b - a)
            S[o, a:b] = 1.0
            cnt = max(cnt, b - a)
        return Wm, S, cnt, 0.0
    f = resize_coords(n_in, n_out, mode, align)
    if mode == "bilinear":
        f = f.clamp_min(0.0)
    i0 = torch.floor(f)
    t = f - i0
    if mode == "bilinear":
        taps = [(i0, 1 - t), (i0 + (i0 < n_in - 1), t)]
        k, dw = 3, 3 * E * max(n_in, n_out)
    else:
        taps = [(i0 - 1, _cubic2(t + 1)), (i0, _cubic1(t)), (i0 + 1, _cubic1(1 - t)), (i0 + 2, _cubic2(2 - t))]
        k, dw = 5, CUBIC_SLOPE * 3 * E * max(n_in, n_out) + CUBIC_ABS
    rows = torch.arange(n_out)
    for idx, w in taps:
        idx = idx.clamp(0, n_in - 1).long()
        Wm.index_put_((rows, idx), w, accumulate=True)
        S.index_put_((rows, idx), torch.ones_like(w), accumulate=True)
    return Wm, S, k, dw


def resize_bound(x, size, mode, align=None):
    """F.interpolate(x [N, C, H, W], size, mode, align_corners) as cgs_resize computes it."""
    Ho, Wo = size
    H, W = x.shape[-2:]
    if mode in ("nearest", "nearest-exact"):
        ref = f64(F.interpolate(x.cpu(), size=(Ho, Wo), mode=mode).to(x.device))
        return ref, torch.zeros_like(ref)
    Wy, Sy, ky, dwy = _resize_axis(H, Ho, mode, bool(align))
    Wx, Sx, kx, dwx = _resize_axis(W, Wo, mode, bool(align))
    Wy, Sy, Wx, Sx = (t.to(x.device) for t in (Wy, Sy, Wx, Sx))
    xd = f64(x)
    ref = Wy @ xd @ Wx.t()
    mag = Wy.abs() @ xd.abs() @ Wx.abs().t()
    taps = Sy @ xd.abs() @ Sx.t()
    k = ky * kx + 1 if mode == "area" else ky + kx
    return ref, _store_dt(ref, k * E * mag + (dwy + dwx) * taps, x.dtype)


# ------------------------------------------------------------------------------------------------ upfirdn2d
def upfirdn2d_bound(x, kernel, up, down, pad):
    """x [N, C, H, W]; kernel [kh, kw]; up = (ux, uy), down = (dx, dy), pad = (px0, px1, py0, py1)."""
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad
    N, C, H, W = x.shape
    kh, kw = kernel.shape
    xd = f64(x).reshape(N * C, 1, H, W)
    z = xd.new_zeros(N * C, 1, H * uy, W * ux)
    z[:, :, ::uy, ::ux] = xd
    z = F.pad(z, (max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)))
    z = z[:, :, max(-py0, 0):z.shape[2] - max(-py1, 0), max(-px0, 0):z.shape[3] - max(-px1, 0)]
    w = torch.flip(f64(kernel).to(x.device), [0, 1])[None, None]         # conv2d correlates: flipped = convolution
    ref = F.conv2d(z, w)[:, :, ::dy, ::dx]
    mag = F.conv2d(z.abs(), w.abs())[:, :, ::dy, ::dx]
    shape = (N, C) + tuple(ref.shape[2:])
    ref, mag = ref.reshape(shape), mag.reshape(shape)
    return ref, _store_dt(ref, C_ACC * kh * kw * E * mag, x.dtype)


# ------------------------------------------------------------------------------------------------ fused_bias_act
def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def fused_bias_act_bound(x, bias, slope, scale):
    """leaky_relu(x + bias[c], slope) * scale with c along dim 1."""
    xd = f64(x)
    if bias is not None:
        xd = xd + f64(bias).reshape(1, -1, *([1] * (x.dim() - 2)))
    ref = torch.where(xd >= 0, xd, xd * _f32(slope)) * _f32(scale)
    return ref, _store_dt(ref, 3 * E * ref.abs(), x.dtype)


# ------------------------------------------------------------------------------------------------ softmax_rows
def softmax_rows_bound(x, scale):
    """fp32 softmax over the last dim of x * scale."""
    s = f64(x) * _f32(scale)
    cols = s.shape[-1]
    t = s - s.amax(-1, keepdim=True)
    p = torch.exp(t)
    ref = p / p.sum(-1, keepdim=True)
    ex = (s.abs() + 3 * t.abs()) * E + EXP2_REL
    rel = ex + (ref * ex).sum(-1, keepdim=True) + C_ACC * cols * E + 2 * E
    return ref, E * ref + TINY[torch.float32] + rel * ref


# ------------------------------------------------------------------------------------------------ fp32 attention
def attention_f32_scores(q, k, heads, mask=None, causal=False, key_padding=None):
    """(s, ds) [B, H, Sq, Sk]: the fp64 scores ops.f32.attention hands to cgs_softmax_rows and the bound of their
    error. cgs_gemm_f32 with alpha = fl32(1 / sqrt D): C_ACC D e mag and the rounding of fmaf(acc, alpha, 0); the
    host's sc.add_(mask) rounds once more; masked_fill(-inf) is exact. The mask is normalised as the host does."""
    B, Sq, HD = q.shape
    Sk, D = k.shape[1], HD // heads
    al = _f32(1.0 / math.sqrt(D))
    qh = f64(q).reshape(B, Sq, heads, D).transpose(1, 2)
    kh = f64(k).reshape(B, Sk, heads, D).transpose(1, 2)
    s = al * (qh @ kh.transpose(-1, -2))
    ds = C_ACC * D * E * al * (qh.abs() @ kh.abs().transpose(-1, -2)) + E * s.abs()
    if mask is not None:
        m = mask
        if m.dtype == torch.bool:
            m = torch.zeros(m.shape, dtype=torch.float64, device=m.device).masked_fill(~m, -math.inf)
        m = f64(m)
        while m.dim() < 4:
            m = m.unsqueeze(0) if m.dim() < 3 else m.unsqueeze(1)
        s = s + m
        ds = ds + E * torch.where(torch.isfinite(s), s.abs(), torch.zeros_like(s))
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool, device=s.device).triu(1), -math.inf)
    if key_padding is not None:
        s = s.masked_fill(~key_padding.bool()[:, None, None, :], -math.inf)
    return s, ds


def attention_f32_bound(q, k, v, heads, mask=None, causal=False, key_padding=None):
    """ops.f32.attention, q [B, Sq, H D], k / v [B, Sk, H D] -> [B, Sq, H D], composed from its three launches:
    the scores within ds (attention_f32_scores); cgs_softmax_rows over ld = ceil4(Sk) columns (the pad columns are
    -inf and add exact zeros): softmax_rows_bound's relative term at scale 1, and dp / p <= exp(2 max_row ds) - 1
    for scores that move by ds (the shift of the row maximum included); O = P V, K = Sk products of the stored p:
    tol = store + C_ACC (Sk + 1) e (p |v|) + dp |v|. A row whose keys are all blocked is NaN on this path (the
    row softmax of -inf): ref = tol = nan there."""
    B, Sq, HD = q.shape
    Sk, D = k.shape[1], HD // heads
    ld = (Sk + 3) // 4 * 4
    s, ds = attention_f32_scores(q, k, heads, mask, causal, key_padding)
    fin = torch.isfinite(s)
    blocked = ~fin.any(-1, keepdim=True)
    mx = torch.where(blocked, torch.zeros_like(s[..., :1]), s.amax(-1, keepdim=True))
    t = torch.where(fin, s - mx, torch.full_like(s, -math.inf))
    e = torch.exp(t)
    p = e / e.sum(-1, keepdim=True).clamp_min(1e-300)
    zero = torch.zeros_like(s)
    ex = torch.where(fin, (s.abs() + 3 * t.abs()) * E + EXP2_REL, zero)
    rel = ex + (p * ex).sum(-1, keepdim=True) + C_ACC * ld * E + 2 * E
    dsmax = torch.where(fin, ds, zero).amax(-1, keepdim=True)
    dp = p * (torch.expm1(2 * dsmax) + E + rel) + torch.where(fin, TINY[torch.float32], 0.0)
    vh = f64(v).reshape(B, Sk, heads, D).transpose(1, 2)
    ref = p @ vh
    tol = _store_dt(ref, C_ACC * (Sk + 1) * E * (p @ vh.abs()) + dp @ vh.abs(), torch.float32)
    nan = torch.full_like(ref, math.nan)
    ref, tol = torch.where(blocked, nan, ref), torch.where(blocked, nan, tol)
    return ref.transpose(1, 2).reshape(B, Sq, HD), tol.transpose(1, 2).reshape(B, Sq, HD)


# ------------------------------------------------------------------------------------------------ tome_match
def tome_bound(a, b):
    """(s, ds) [B, Na, Nb]: the cosine similarity of every src row a_i with every dst row b_j."""
    a, b = f64(a), f64(b)
    C = a.shape[-1]
    na, nb = a.norm(dim=-1, keepdim=True), b.norm(dim=-1, keepdim=True)
    ia = torch.where(na > 0, 1 / na.clamp_min(1e-300), torch.zeros_like(na))
    ib = torch.where(nb > 0, 1 / nb.clamp_min(1e-300), torch.zeros_like(nb))
    s = (a * ia) @ (b * ib).transpose(-1, -2)
    mag = (a.abs() * ia) @ (b.abs() * ib).transpose(-1, -2)
    return s, C_ACC * (C + 2) * E * mag + 2 * RSQRT_REL * s.abs()


def assert_tome(vmax, imax, a, b, what):
    """vmax within max_j ds of max_j s; the chosen dst within 2 ds of the best; of bit-identical dst rows the lower
    index. Returns max |vmax - max_j s| / max_j ds."""
    s, ds = tome_bound(a, b)
    best, dmax = s.amax(-1), ds.amax(-1)
    vmax, imax = f64(vmax), imax.long()
    assert bool(torch.isfinite(vmax).all()), f"{what}: non-finite vmax"
    assert bool(((imax >= 0) & (imax < s.shape[-1])).all()), f"{what}: index out of range"
    ratio = ((vmax - best).abs() / dmax.clamp_min(1e-300)).max().item()
    print(f"BOUND {what}: max |vmax - max_j s| / max_j ds {ratio:.3f}")
    assert ratio <= 1, f"{what}: vmax over tol, worst {ratio:.3f} x tol"
    picked = torch.gather(s, -1, imax[..., None])[..., 0]
    assert bool((picked >= best - 2 * dmax).all()), f"{what}: a chosen dst row is over tol below the best"
    bb = b.reshape(b.shape[0], b.shape[1], -1)
    for bt in range(bb.shape[0]):
        same = (bb[bt][:, None, :] == bb[bt][None, :, :]).all(-1).tril(-1)       # same[j, l]: row l < j is row j
        first = torch.where(same.any(-1), same.double().argmax(-1), torch.arange(same.shape[0], device=same.device))
        assert bool((first[imax[bt]] == imax[bt]).all()), f"{what}: a tie went to the higher index"
    return ratio


# ------------------------------------------------------------------------------------------------ shared test inputs
UPFIRDN_KERNELS = {"3x5": (3, 5), "1x4": (1, 4), "4x1": (4, 1)}
# (up_x, up_y), (down_x, down_y), (px0, px1, py0, py1)
UPFIRDN_CFGS = [((2, 1), (1, 2), (2, 1, 0, 3)), ((1, 2), (2, 1), (-1, 2, 1, -1)), ((2, 2), (1, 2), (-1, 2, 1, -1)),
                ((2, 2), (2, 1), (2, 1, 0, 3))]
FBA_SHAPES = [(37, 24), (2, 24, 5), (3, 24, 11, 7), (2, 6, 2, 3, 5)]
SMR_ROWS, SMR_COLS = [1, 5, 257], [1, 63, 64, 65, 200]
TOME_SHAPES = [(2, 1, 1, 8), (3, 65, 37, 40), (1, 130, 64, 72), (2, 64, 129, 320)]


def upfirdn_kernel(kh, kw):
    """Distinct values, no symmetry: 1, 2, 3 ... with the odd taps at -0.5, scaled to |sum| 1."""
    k = torch.arange(1.0, kh * kw + 1).reshape(kh, kw)
    k[..., 1::2] *= -0.5
    return k / k.abs().sum()


def smr_inputs(rows, cols, dtype, device="cpu", seed=0):
    """8 randn with one +30 spike per row, at a column that moves with the row (the last one in row 0)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * 8
    x[torch.arange(rows), (cols - 1 - torch.arange(rows) * 7) % cols] += 30
    return x.to(dtype).to(device)


def tome_inputs(B, Na, Nb, C, dtype, device="cpu", seed=0):
    """a, b as column slices of wider tensors (row stride C + 24); dst rows 0 and Nb - 1 bit-identical and the best
    match of src row 0, which is a multiple of them; the last src row all zero (where Na > 1)."""
    g = torch.Generator().manual_seed(seed)
    wa = torch.randn(B, Na, C + 24, generator=g).to(dtype)
    wb = torch.randn(B, Nb, C + 24, generator=g).to(dtype)
    if Nb > 1:
        wb[:, -1] = wb[:, 0]
    if Na > 1:
        wa[:, 0] = wb[:, 0] * 2
        wa[:, -1] = 0
    wa, wb = wa.to(device), wb.to(device)
    return wa[:, :, 8:8 + C], wb[:, :, 8:8 + C]


# ------------------------------------------------------------------------------------------------ fp32 kernels (f32.hip)
F32_ACTS = [None, "gelu", "gelu_tanh", "quick_gelu", "silu", "relu"]
# (M, N, K) of ops.linear on the 128 x 128 x 32 tile: one row; one past a tile in M, N and K; K % 4 != 0 (the host pads
# the rows, the kernel keeps its own K); K < 4; K just under a tile; three K tiles
F32_LINEAR_SHAPES = [(1, 5, 4), (129, 132, 36), (130, 127, 33), (257, 5, 3), (64, 260, 31), (3, 129, 68)]
# (N, C1, C2, H, W, Cout, k, stride, pad, up2, res)
F32_CONV_CASES = [(2, 4, 0, 9, 9, 5, 3, 1, 1, False, False), (1, 3, 0, 6, 5, 8, 3, 1, 1, False, True),
                  (2, 8, 4, 9, 9, 12, 3, 2, 0, False, True), (1, 8, 0, 4, 6, 16, 3, 1, 1, True, False),
                  (1, 12, 0, 3, 3, 130, 1, 1, 0, False, False), (1, 6, 6, 5, 5, 8, 3, 1, 1, False, False)]
# (N, C1, C2, G, H, W)
F32_GN_CASES = [(2, 8, 0, 2, 1, 1), (3, 64, 0, 32, 5, 7), (2, 320, 0, 32, 10, 10), (1, 1280, 0, 32, 8, 8),
                (2, 1028, 0, 4, 2, 3), (2, 12, 20, 4, 6, 7), (2, 6, 10, 4, 6, 7)]
F32_LN_C, F32_LN_ROWS = [4, 252, 256, 260, 1280], [1, 5]
SPIKE = 48.0


def mixed_scales(n, g, lo=1e-3, hi=10.0):
    """n scales log-spaced over lo .. hi in a random order (one scale: 1)."""
    if n == 1:
        return torch.ones(1)
    return torch.logspace(math.log10(lo), math.log10(hi), n)[torch.randperm(n, generator=g)]


def f32_gemm_inputs(M, N, K, seed=0, device="cpu"):
    """fp32 a [M, K] = randn s_m s_k, w [N, K] = randn s_n / sqrt K, bias [N] = randn s_n, res [M, N] = randn s_m s_n, the
    scales log-spaced over 1e-3 .. 10 and permuted (s_k over 0.03 .. 3). Spikes of +-48 s_m on element K - 1 of every
    third row and on element 32 of every fourth (the first of the second K tile)."""
    g = torch.Generator().manual_seed(seed)
    s_m, s_n, s_k = mixed_scales(M, g), mixed_scales(N, g), mixed_scales(K, g, 0.03, 3.0)
    a = torch.randn(M, K, generator=g) * s_m[:, None] * s_k[None, :]
    a[::3, K - 1] = SPIKE * s_m[::3]
    if K > 32:
        a[::4, 32] = -SPIKE * s_m[::4]
    w = torch.randn(N, K, generator=g) * s_n[:, None] / math.sqrt(K)
    b = torch.randn(N, generator=g) * s_n
    r = torch.randn(M, N, generator=g) * s_m[:, None] * s_n[None, :]
    return tuple(t.to(device) for t in (a, w, b, r)) + ((s_m, s_n, s_k),)


def f32_conv_inputs(N, C1, C2, H, W, Cout, k, seed=0, device="cpu"):
    """fp32 NCHW x [N, C1, H, W], x2 [N, C2, H, W] or None, w [Cout, C1 + C2, k, k], bias, the image, input-channel and
    output-channel scales log-spaced and permuted. Spikes of +-48 s_n: the first and the last pixel of every image
    (both sides of an image boundary of the implicit GEMM's rows), the channels on both sides of the dual-source
    seam at the centre pixel, and the weights' last tap carries no smaller weights than the others."""
    g = torch.Generator().manual_seed(seed)
    C = C1 + C2
    s_i, s_c, s_o = mixed_scales(N, g), mixed_scales(C, g, 0.03, 3.0), mixed_scales(Cout, g)
    x = torch.randn(N, C, H, W, generator=g) * s_i[:, None, None, None] * s_c[None, :, None, None]
    x[:, 0, 0, 0] = SPIKE * s_i
    x[:, C - 1, H - 1, W - 1] = -SPIKE * s_i
    if C2:
        x[:, C1 - 1, H // 2, W // 2] = SPIKE * s_i
        x[:, C1, H // 2, W // 2] = -SPIKE * s_i
    w = torch.randn(Cout, C, k, k, generator=g) * s_o[:, None, None, None] / math.sqrt(C * k * k)
    b = torch.randn(Cout, generator=g) * s_o
    x = x.to(device)
    x1, x2 = (x[:, :C1].contiguous(), x[:, C1:].contiguous()) if C2 else (x, None)
    return x1, x2, w.to(device), b.to(device), (s_i, s_c, s_o)


def f32_gn_inputs(N, C1, C2, H, W, seed=0, device="cpu", shift=0.0):
    """fp32 x [N, C1, H, W] (x2 [N, C2, H, W]) = shift + randn s_n s_c, gamma = randn s_c', beta = 0.1 randn s_c',
    pre_add [N, C] = randn s_n s_c; spikes of +-48 s_n s_c on the last pixel of every slice of cgs_groupnorm_f32 and
    on the channels on both sides of the seam."""
    g = torch.Generator().manual_seed(seed)
    C = C1 + C2
    s_n, s_c, s_g = mixed_scales(N, g), mixed_scales(C, g, 0.03, 3.0), mixed_scales(C, g)
    sc = s_n[:, None, None] * s_c[None, :, None]
    x = torch.randn(N, C, H * W, generator=g) * sc
    for p in gn_f32_bounds(N, H * W, C)[1:]:
        x[:, (p * 5) % C, p - 1] = SPIKE * sc[:, (p * 5) % C, 0]
    if C2:
        x[:, C1 - 1, (H * W) // 2] = SPIKE * sc[:, C1 - 1, 0]
        x[:, C1, (H * W) // 2] = -SPIKE * sc[:, C1, 0]
    x = (x + shift).reshape(N, C, H, W)
    gamma, beta = torch.randn(C, generator=g) * s_g, 0.1 * torch.randn(C, generator=g) * s_g
    pa = (torch.randn(N, C, generator=g) * sc[:, :, 0]).to(device)
    x = x.to(device)
    x1, x2 = (x[:, :C1].contiguous(), x[:, C1:].contiguous()) if C2 else (x, None)
    return x1, x2, gamma.to(device), beta.to(device), pa


def f32_ln_inputs(rows, C, seed=0, device="cpu", shift=0.0):
    """fp32 x [rows, C] = shift + randn s_r s_c with a spike of 48 s_r on the last element; w = randn s_c', b = 0.1 randn
    s_c'."""
    g = torch.Generator().manual_seed(seed)
    s_r, s_c, s_w = mixed_scales(rows, g), mixed_scales(C, g, 0.03, 3.0), mixed_scales(C, g)
    x = torch.randn(rows, C, generator=g) * s_r[:, None] * s_c[None, :]
    x[:, C - 1] = SPIKE * s_r
    x = x + shift
    return x.to(device), (torch.randn(C, generator=g) * s_w).to(device), (0.1 * torch.randn(C, generator=g) * s_w).to(device)


def f32_attn_inputs(B, heads, Sq, Sk, D, seed=0, device="cpu"):
    """q, k, v as views of one fused [B, S, 3 H D] tensor (S = max(Sq, Sk)): q = randn, k = randn with a head scale over
    0.3 .. 3 (flat and peaked rows), v = randn s_h s_d over 1e-3 .. 10 with spikes of +-48 s_h on the last key and
    on key 32."""
    g = torch.Generator().manual_seed(seed)
    HD, S = heads * D, max(Sq, Sk)
    qkv = torch.randn(B, S, 3 * HD, generator=g)
    s_k = mixed_scales(heads, g, 0.3, 3.0).repeat_interleave(D)
    s_h = mixed_scales(heads, g).repeat_interleave(D)
    s_v = s_h * mixed_scales(HD, g, 0.1, 1.0)
    qkv[:, :, HD:2 * HD] *= s_k
    qkv[:, :, 2 * HD:] *= s_v
    qkv[:, Sk - 1, 2 * HD:] = SPIKE * s_h
    if Sk > 32:
        qkv[:, 32, 2 * HD:] = -SPIKE * s_h
    qkv = qkv.to(device)
    return qkv[:, :Sq, :HD], qkv[:, :Sk, HD:2 * HD], qkv[:, :Sk, 2 * HD:], s_h


# ------------------------------------------------------------------------------------------------ sampling loop
_M64, _M32 = (1 << 64) - 1, 0xFFFFFFFF
TWO_PI_F = _f32(6.2831853)                       # the kernel's literal 6.2831853f
NORMAL_A = 2 * math.pi + SINCOSF_REL / E         # tol = e (A r + B |z|), module docstring
NORMAL_B = 2 + LOGF_REL / (2 * E)
# flat sizes of the fp32 kernels: one element, both sides of a block of 256, several blocks with a ragged end; past
# the 8192-block cap of ew_blocks (elementwise.hip) the grid-stride loop makes its second trip
EW_SIZES = [1, 255, 256, 257, 4099]
EW_CAP_N = 8192 * 256 + 513
SILU_SIZES = [1, 7, 8, 9, 2055]                  # the scalar tail alone, no tail, one vector and a tail
SILU_CAP_N = 8192 * 256 * 8 + 13                 # second trip and a tail in one call
SEED63 = (1 << 63) + 5                           # a seed with bit 63 set
# cgs_philox_randn: tails, image bases that are no multiple of 4 (the scalar store path), several images
RNG_SHAPES = [(1, 1), (1, 3), (2, 5), (2, 1027), (3, 4, 8, 8)]
RNG_SEEDS = [0, 1234567, SEED63, (1 << 64) - 1]
RNG_INDEX0 = [0, (1 << 31) - 1, 1 << 40]
RNG_STREAMS = [0, (1 << 32) + 7, (1 << 63) - 1]
RNG_CAP_SHAPE = (17, 1 << 20)                    # 17 * 2^18 groups: past the 16384-block cap of rng_blocks (rng.hip)
TEMB_SHAPES = [(1, 2), (5, 6), (3, 320), (2, 1280)]
TEMB_T = [0.0, 0.5, 999.0, 1000.0]


def _sc(v):
    """A scalar as the fp32 value the kernel is passed (an fp32 tensor element is taken as it is)."""
    return float(v) if torch.is_tensor(v) else _f32(v)


def cfg_combine_bound(c, u, s):
    """out = u + (c - u) s in fp32 (cgs_cfg_combine, the den of cgs_sampler_step_dev)."""
    c, u, s = f64(c), f64(u), _sc(s)
    ref = u + (c - u) * s
    return ref, (2 * E * (c - u).abs() * abs(s) + E * ref.abs()) * (1 + 2 * E)


def euler_step_bound(x, den, noise, sigma, sigma_down, sigma_up):
    """x + (x - den) / sigma (sigma_down - sigma) + noise sigma_up in fp32 (cgs_euler_step and the fused forms);
    noise None, or sigma_up <= 0: no noise term."""
    x, den = f64(x), f64(den)
    s, sd, sup = _sc(sigma), _sc(sigma_down), _sc(sigma_up)
    ddt = (x - den) / s * (sd - s)
    ref = x + ddt
    tol = 5 * E * ddt.abs() + E * ref.abs()
    if noise is not None and sup > 0:
        q = f64(noise) * sup
        ref = ref + q
        tol = tol + E * q.abs() + E * ref.abs()
    return ref, tol * (1 + 8 * E)


def philox_words(seed, inds, groups, stream):
    """The four Philox4x32-10 output words [len(inds), groups] (int64) of every element group, from the integer code
    of the CPU mirror: key = image_key(seed, index), counter = (group lo, hi, stream lo, hi)."""
    from comfy_gen_server_amd.sampling import rng
    inds = [int(i) for i in inds]
    k0, k1 = rng._key_tensors(seed, inds)
    g = torch.arange(groups, dtype=torch.int64).view(1, -1)
    s = int(stream) & _M64
    c0 = (g & _M32).expand(len(inds), -1)
    c1 = (g >> 32).expand(len(inds), -1)
    c2, c3 = torch.full_like(c0, s & _M32), torch.full_like(c0, s >> 32)
    return rng._philox10(c0, c1, c2, c3, k0.expand_as(c0), k1.expand_as(c0))


def normal_bound(seed, inds, n, stream, dtype=torch.float32):
    """(ref, tol) [len(inds), n] of the N(0, 1) values of (seed, image, stream): fp64 Box-Muller on the mirror's
    fp32 uniforms (module docstring). dtype bfloat16: the store of cgs_philox_randn's bf16 form."""
    from comfy_gen_server_amd.sampling import rng
    groups = (n + 3) // 4
    un = [rng._u01(w).double() for w in philox_words(seed, inds, groups, stream)]
    refs, tols = [], []
    for u0, u1 in ((un[0], un[1]), (un[2], un[3])):
        r = torch.sqrt(-2.0 * torch.log(u0))
        t = TWO_PI_F * u1
        for trig in (torch.cos, torch.sin):
            z = r * trig(t)
            refs.append(z)
            tols.append(E * (NORMAL_A * r + NORMAL_B * z.abs()) * (1 + 8 * E))
    ref = torch.stack(refs, -1).reshape(len(un[0]), groups * 4)[:, :n].contiguous()
    tol = torch.stack(tols, -1).reshape(len(un[0]), groups * 4)[:, :n].contiguous()
    if dtype != torch.float32:
        tol = _store_dt(ref, tol, dtype)
    return ref, tol


def sampler_step_bound(x, c, u, cfg, row, seed, index0, step):
    """cgs_sampler_step_dev on fp32 x, c, u (None: den = c) [B, ...] with row = params[step] = (sigma, sigma_down,
    sigma_up, s_noise, ...) in fp32. Returns ((ref, tol) of x, (ref, tol) of den_out)."""
    row = row.detach().to("cpu", torch.float32)
    s, sd, sup = float(row[0]), float(row[1]), float(row[2] * row[3])        # the fp32 product, rounded once
    if u is None:
        den = f64(c)
        dtol = torch.zeros_like(den)
    else:
        den, dtol = cfg_combine_bound(c, u, cfg)
    z, extra = None, abs((sd - s) / s) * dtol
    if sup > 0:
        B = x.shape[0]
        z, ztol = normal_bound(seed, range(int(index0), int(index0) + B), x[0].numel(), step)
        z, ztol = z.reshape(x.shape).to(x.device), ztol.reshape(x.shape).to(x.device)
        extra = extra + sup * ztol
    ref, tol = euler_step_bound(x, den, z, s, sd, sup)
    return (ref, (tol + extra) * (1 + 8 * E)), (den, dtol)


def timestep_embedding_bound(t, dim, max_period=10000.0, flip=True):
    """[cos | sin] (flip) or [sin | cos] of t exp(-ln P k / half), k < half = dim // 2, for fp32 t [n]."""
    t = f64(t.detach().float())
    half = dim // 2
    lnp = float(torch.log(torch.tensor(float(max_period), dtype=torch.float32)))
    xk = lnp * torch.arange(half, dtype=torch.float64, device=t.device) / half
    a = t[:, None] * torch.exp(-xk)[None]
    da = a.abs() * (EXP2_REL + 4 * E * (1 + xk))[None]
    c, s = torch.cos(a), torch.sin(a)
    tc, ts = (da + SINCOSF_REL * (v.abs() + da) for v in (c, s))
    exact = (t == 0)[:, None]
    tc, ts = tc.masked_fill(exact, 0.0), ts.masked_fill(exact, 0.0)
    if flip:
        return torch.cat([c, s], -1), torch.cat([tc, ts], -1)
    return torch.cat([s, c], -1), torch.cat([ts, tc], -1)


def silu_bound(x):
    """cgs_silu on bf16 / fp16 x: the SIG-family activation error and one store in x's dtype."""
    ref, tol = _act_tol(f64(x), 0.0, None, "silu", 0.0, dtype=x.dtype)
    return ref, tol + TINY[x.dtype]


def ew_inputs(n, seed=0, device="cpu"):
    """Four fp32 vectors of n elements (x, cond / den, uncond, noise) = randn s with the scales log-spaced over
    1e-3 .. 10 and permuted; the last x is a spike of 48, and in the middle den == x (a difference of exactly 0)."""
    g = torch.Generator().manual_seed(seed)
    x, c, u, z = (torch.randn(n, generator=g) * mixed_scales(n, g) for _ in range(4))
    x[n - 1] = SPIKE
    c[n // 2] = x[n // 2]
    return tuple(v.to(device) for v in (x, c, u, z))


def silu_inputs(n, dtype, seed=0, device="cpu"):
    """4 randn in ``dtype``; the first elements are +-0, +-48 and the largest and smallest normal of the dtype, both
    signs; the last two (the scalar tail where n % 8 >= 2) -48 and the smallest normal."""
    g = torch.Generator().manual_seed(seed)
    fi = torch.finfo(dtype)
    x = torch.randn(n, generator=g) * 4
    special = torch.tensor([0.0, -0.0, SPIKE, -SPIKE, fi.max, -fi.max, fi.tiny, -fi.tiny], dtype=torch.float64)
    k = min(n, special.numel())
    x = x.double()
    x[:k] = special[:k]
    if n > special.numel() + 2:
        x[n - 1], x[n - 2] = -SPIKE, fi.tiny
    return x.to(dtype).to(device)
