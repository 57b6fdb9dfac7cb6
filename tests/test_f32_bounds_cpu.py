"""Self-test of the fp32 bounds of tests/_bounds.py (csrc/kernels/f32.hip, ops/f32.py) on the CPU. Each kernel is
emulated in fp32 torch in its own structure -- the GEMM and the implicit-GEMM conv over 32-deep K tiles with the
fmaf / activation / residual epilogue, GroupNorm as shifted slice sums, sequential Chan merges over the P pixel lanes
and the two finalize passes, LayerNorm in two passes over lane-strided float4s, attention as its three launches over
ld-padded scores -- and must lie within the bound in every element. Then faults are injected: each passes the judge
of test_f32_gpu.py (max |y - ref| / max |ref| under 2e-6 or 1e-5, asserted here) and is rejected by assert_within.
The inputs are mixed-scale (rows, channels, images and heads log-spaced over 1e-3 .. 10, permuted) with spikes of
+-48, so a per-element bound bites where a max-norm judge cannot."""
import math

import pytest
import torch
import torch.nn.functional as F

from _bounds import (C_ACC, E, F32_ACTS, F32_CONV_CASES, F32_GN_CASES, F32_LINEAR_SHAPES, F32_LN_C, F32_LN_ROWS, U,
                     assert_within, attention_f32_bound, conv_act_bound, conv_bound, f32_attn_inputs,
                     f32_conv_inputs, f32_gemm_inputs, f32_gn_inputs, f32_ln_inputs, f64, gemm_act_bound, gemm_bound,
                     gn_f32_bounds, gn_f32_depth, gn_f32_form, groupnorm_f32_bound, layernorm_bound, ln_f32_depth)
from test_f32_gpu import _err

FP = torch.float32
OLD_GEMM, OLD_NORM = 2e-6, 1e-5           # the thresholds of test_f32_gpu.py
# act_family (common.h): a, b of x * sigmoid(x (c0 + c1 x^2)) as -c0 log2 e, -c1 log2 e
SIG_AB = {"gelu_tanh": (-2.302208198e+00, -1.029432396e-01), "quick_gelu": (-2.455466953e+00, 0.0),
          "silu": (-1.442695041e+00, 0.0)}


def _rejected(y, ref, tol, what):
    with pytest.raises(AssertionError, match="over tol"):
        assert_within(y, ref, tol, what)


def _fma(a, b, c):
    """One rounding: fp32 products are exact in fp64."""
    return (a.double() * b.double() + c.double()).float()


def _act(v, act):
    """gelu_f and act_fam (common.h) in fp32."""
    if act is None:
        return v
    if act == "gelu":
        return (0.5 * v) * (1.0 + torch.erf(v * 0.70710678118654752))
    if act == "relu":
        return v.clamp_min(0.0)
    a, b = SIG_AB[act]
    return v * (1.0 / (1.0 + torch.exp2(v * _fma(v * v, torch.tensor(b), torch.tensor(a)))))


def _emulate_gemm(a, w, b=None, r=None, act=None, alpha=1.0, K=None):
    """f32_gemm_kernel: the accumulator over 32-deep K tiles, fmaf(acc, alpha, bias), the activation, + R."""
    K = a.shape[1] if K is None else K
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k0 in range(0, K, 32):
        k1 = min(k0 + 32, K)
        acc = acc + a[:, k0:k1] @ w[:, k0:k1].t()
    v = _fma(acc, torch.tensor(alpha, dtype=FP), torch.zeros(()) if b is None else b)
    v = _act(v, act)
    return v if r is None else v + r


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("M,N,K", F32_LINEAR_SHAPES + [(300, 200, 132)])
def test_gemm_f32_emulation_within_bound(M, N, K):
    a, w, b, r, _ = f32_gemm_inputs(M, N, K)
    for bias, res in ((None, None), (b, None), (b, r)):
        ref, tol = gemm_bound(a, w, bias, res, dtype=FP)
        assert_within(_emulate_gemm(a, w, bias, res), ref, tol, f"emulated f32 gemm {M}x{N}x{K}")
    for act in F32_ACTS[1:]:
        for res in (None, r):
            ref, tol = gemm_act_bound(a, w, b, res, act, dtype=FP)
            assert_within(_emulate_gemm(a, w, b, res, act), ref, tol, f"emulated f32 gemm {M}x{N}x{K} {act}")
    al = 1.0 / math.sqrt(40)
    ref, tol = gemm_bound(a, w, b, None, alpha=al, dtype=FP)
    assert_within(_emulate_gemm(a, w, b, alpha=al), ref, tol, f"emulated f32 gemm {M}x{N}x{K} alpha")


def test_gelu_f_bound_is_not_gelu_abs():
    """The fp32 kernel's erf GELU is judged to roundoffs, not to GELU_ABS = 2.6e-5; far below zero, where 1 + erf
    cancels, the bound stays absolute (0.5 |x| times the error of erff)."""
    x = torch.tensor([[-9.0, -3.0, -0.5, 1e-3, 0.7, 4.0]])
    eye = torch.ones(1, 1)
    for i in range(x.shape[1]):
        ref, tol = gemm_act_bound(x[:, i:i + 1], eye, None, None, "gelu", dtype=FP)
        assert tol.item() < 20 * E * max(abs(x[0, i].item()), 1e-3), (x[0, i], tol)
        assert_within(_act(x[:, i:i + 1], "gelu"), ref, tol, f"gelu_f({x[0, i].item()})")
    _, tol = gemm_act_bound(x[:, :1], eye, None, None, "gelu", dtype=FP)
    assert tol.item() > 4 * E                     # not relative to gelu(-9) = -5e-19


def _low_rows(a, r, s_m, rows, scale=1e-3):
    """Rows ``rows`` of a (and of the residual) brought to one low scale: a low-scale row block."""
    f = (scale / s_m[rows])[:, None]
    a[rows] *= f
    r[rows] *= f


def test_gemm_f32_fault_reduced_precision_rows():
    """The rows of scale <= 1e-3 multiplied after A is rounded to 10 mantissa bits (a 16-bit operand path)."""
    M, N, K = 130, 127, 33
    a, w, b, r, (s_m, _, _) = f32_gemm_inputs(M, N, K)
    low = s_m <= 1.2e-3
    _low_rows(a, r, s_m, slice(64, 80))
    low[64:80] = True
    a10 = ((a.view(torch.int32) + 0x1000) & ~0x1FFF).view(FP)
    ref, tol = gemm_bound(a, w, b, r, dtype=FP)
    y = _emulate_gemm(torch.where(low[:, None], a10, a), w, b, r)
    assert _err(y, ref) < OLD_GEMM
    _rejected(y, ref, tol, "f32 gemm: 10-bit A on the low-scale rows")


def test_gemm_f32_fault_k_tail_dropped():
    """The last K % 4 elements (the scalar tail of ld_k4) missing for one low-scale 16-row block."""
    M, N, K = 130, 127, 33
    a, w, b, r, (s_m, _, _) = f32_gemm_inputs(M, N, K)
    _low_rows(a, r, s_m, slice(64, 80))
    a[64:80, K - 1] = 2e-4 * torch.linspace(0.5, 2.0, 16)        # no spike on the tail of these rows
    ref, tol = gemm_bound(a, w, b, r, dtype=FP)
    y = _emulate_gemm(a, w, b, r)
    y[64:80] = _emulate_gemm(a[64:80], w, b, r[64:80], K=K - K % 4)
    assert _err(y, ref) < OLD_GEMM
    _rejected(y, ref, tol, "f32 gemm: K tail dropped for rows 64..79")


def test_gemm_f32_fault_bias_dropped():
    """The bias missing on the last row of one low-scale column."""
    M, N, K = 130, 127, 33
    a, w, b, r, (_, s_n, _) = f32_gemm_inputs(M, N, K)
    n = int(s_n.argmin())
    ref, tol = gemm_bound(a, w, b, None, dtype=FP)
    y = _emulate_gemm(a, w, b)
    y[-1, n] -= b[n]
    assert _err(y, ref) < OLD_GEMM
    _rejected(y, ref, tol, "f32 gemm: bias dropped at the last row of a low-scale column")


def test_default_dtype_is_the_bf16_bound_bit_for_bit():
    """The generalised functions with the default dtype: the formulas they had before, with U, bit for bit."""
    g = torch.Generator().manual_seed(3)
    a, w = torch.randn(33, 40, generator=g).bfloat16(), (torch.randn(24, 40, generator=g) / 6).bfloat16()
    b, r = torch.randn(24, generator=g).bfloat16(), torch.randn(33, 24, generator=g).bfloat16()
    pre = 0.25 * (f64(a) @ f64(w).t()) + f64(b)
    mag = 0.25 * (f64(a).abs() @ f64(w).abs().t()) + f64(b).abs() + f64(r).abs()
    ref, tol = gemm_bound(a, w, b, r, alpha=0.25)
    old_ref = pre + f64(r)
    assert torch.equal(ref, old_ref)
    assert torch.equal(tol, U * old_ref.abs() * (1 + 2 * U) + U * pre.abs() + C_ACC * 40 * E * mag)
    ref, tol = gemm_act_bound(a, w, b, r, "relu", alpha=0.25)
    y = pre.clamp_min(0.0)
    assert torch.equal(ref, y + f64(r))
    assert torch.equal(tol, U * (y + f64(r)).abs() * (1 + 2 * U) + (1.0 * (C_ACC * 40 * E * mag) + 0.0 + U * y.abs()) * (1 + U))
    x = torch.randn(2, 8, 5, 5, generator=g).bfloat16()
    cw, cr = (torch.randn(6, 8, 3, 3, generator=g) / 8).bfloat16(), torch.randn(2, 6, 5, 5, generator=g).bfloat16()
    cb = torch.randn(6, generator=g).bfloat16()
    pre = F.conv2d(f64(x), f64(cw), f64(cb), 1, 1)
    mag = F.conv2d(f64(x).abs(), f64(cw).abs(), f64(cb).abs(), 1, 1) + f64(cr).abs()
    ref, tol = conv_bound(x, cw, cb, cr, 1, 1)
    old_ref = pre + f64(cr)
    assert torch.equal(ref, old_ref)
    assert torch.equal(tol, U * old_ref.abs() * (1 + 2 * U) + U * pre.abs() + C_ACC * 72 * E * mag)
    ref, tol = conv_act_bound(x, cw, cb, cr, "relu", stride=1, pad=1)
    y = pre.clamp_min(0.0)
    assert torch.equal(ref, y + f64(cr))
    assert torch.equal(tol, U * (y + f64(cr)).abs() * (1 + 2 * U) + (1.0 * (C_ACC * 72 * E * mag) + 0.0 + U * y.abs()) * (1 + U))


# ------------------------------------------------------------------------------------------------ conv
def _im2col(x, k, stride, pad, up2):
    """A [N Ho Wo, k k C] of the implicit GEMM, K ordered (ky, kx, c) as load_a reads it; (A, Ho, Wo)."""
    if up2:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    N, C, H, W = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    cols = F.unfold(x, k, padding=pad, stride=stride)
    return cols.reshape(N, C, k * k, Ho * Wo).permute(0, 3, 2, 1).reshape(N * Ho * Wo, k * k * C), Ho, Wo


def _conv_from(A, w, b, r, N, Ho, Wo):
    wm = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    rm = None if r is None else r.permute(0, 2, 3, 1).reshape(-1, w.shape[0])
    return _emulate_gemm(A, wm, b, rm).reshape(N, Ho, Wo, -1).permute(0, 3, 1, 2)


def _conv_case(case, seed=0):
    N, C1, C2, H, W, Cout, k, stride, pad, up2, res = case
    x, x2, w, b, scales = f32_conv_inputs(N, C1, C2, H, W, Cout, k, seed)
    xin = x if x2 is None else torch.cat([x, x2], 1)
    A, Ho, Wo = _im2col(xin, k, stride, pad, up2)
    g = torch.Generator().manual_seed(seed + 100)
    r = None
    if res:
        r = torch.randn(N, Cout, Ho, Wo, generator=g) * scales[0][:, None, None, None] * scales[2][None, :, None, None]
    return x, x2, w, b, r, A, Ho, Wo, scales


@pytest.mark.parametrize("case", F32_CONV_CASES)
def test_conv_f32_emulation_within_bound(case):
    N, C1, C2, H, W, Cout, k, stride, pad, up2, res = case
    x, x2, w, b, r, A, Ho, Wo, _ = _conv_case(case)
    ref, tol = conv_bound(x, w, b, r, stride, pad, up2, x2, dtype=FP)
    assert_within(_conv_from(A, w, b, r, N, Ho, Wo), ref, tol, f"emulated f32 conv {case}")


def test_conv_f32_fault_next_image_pixel():
    """An out-of-range tap at the last pixel of a low-scale image reads pixel (0, 0) of the next image instead of
    zero (the row index taken without the image bound)."""
    case = (3, 4, 0, 9, 9, 5, 3, 1, 1, False, False)
    N, C, H, W, k = 3, 4, 9, 9, 3
    x, x2, w, b, r, A, Ho, Wo, (s_i, _, _) = _conv_case(case, seed=1)
    order = torch.argsort(s_i)                 # the two low-scale images side by side, the large one first
    x = x[[int(order[2]), int(order[0]), int(order[1])]].contiguous()
    x[2, :, 0, 0] = torch.randn(C, generator=torch.Generator().manual_seed(7)) * s_i[order[1]] * 0.01          # no spike on the pixel the fault reads
    A, Ho, Wo = _im2col(x, k, 1, 1, False)
    ref, tol = conv_bound(x, w, b, None, 1, 1, dtype=FP)
    m = 2 * H * W - 1                                   # the last pixel of image 1
    assert bool((A[m, (k * k - 1) * C:] == 0).all())    # tap (2, 2) is outside the image there
    A[m, (k * k - 1) * C:] = x[2, :, 0, 0]
    y = _conv_from(A, w, b, None, N, Ho, Wo)
    assert _err(y, ref) < OLD_GEMM
    _rejected(y, ref, tol, "f32 conv: the next image's first pixel for an out-of-range tap")


# ------------------------------------------------------------------------------------------------ GroupNorm
def _butterfly(v):
    """wave_sum: v [..., 64] -> [...]."""
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def _block_sum(terms):
    """A 256-thread block sums ``terms``: thread t adds elements t, t + 256, ... in sequence, wave_sum, then the four
    waves in order."""
    n = terms.numel()
    t = torch.zeros((n + 255) // 256 * 256)
    t[:n] = terms
    s = torch.zeros(256)
    for row in t.reshape(-1, 256):
        s = s + row
    wv = _butterfly(s.reshape(4, 64))
    return ((wv[0] + wv[1]) + wv[2]) + wv[3]


def _gn_partials(v, N, HW, C):
    """gn_f32_partial_kernel on v [N, HW, C] (x + pre_add, rounded): (mean, M2) [N, S, C] each."""
    S, P = gn_f32_form(N, HW, C)
    bd = gn_f32_bounds(N, HW, C)
    pm, pq = torch.zeros(N, S, C), torch.zeros(N, S, C)
    for n in range(N):
        for s in range(S):
            p0, p1 = bd[s], bd[s + 1]
            sft = v[n, p0]
            lanes = []
            for pl in range(P):
                d = v[n, p0 + pl:p1:P] - sft
                sm, sq = torch.zeros(C), torch.zeros(C)
                for row in d:
                    sm = sm + row
                    sq = _fma(row, row, sq)
                k = d.shape[0]
                mu = sm / k if k else torch.zeros(C)
                lanes.append((float(k), sft + mu, (sq - sm * mu).clamp_min(0.0) if k else torch.zeros(C)))
            nA, mA, MA = lanes[0]
            for nB, mB, MB in lanes[1:]:
                if nB == 0:
                    continue
                nAB = nA + nB
                d = mB - mA
                mA = mA + d * (torch.tensor(nB) / torch.tensor(nAB))
                MA = MA + (MB + d * d * (torch.tensor(nA) * torch.tensor(nB) / torch.tensor(nAB)))
                nA = nAB
            pm[n, s], pq[n, s] = mA, MA
    return pm, pq


def _gn_finalize(pm, pq, N, HW, C, G):
    """gn_f32_finalize_kernel: (mean, var) [N, G] from the partials, two passes."""
    S = pm.shape[1]
    bd = gn_f32_bounds(N, HW, C)
    cnt = torch.tensor([float(b1 - b0) for b0, b1 in zip(bd, bd[1:])])
    cpg = C // G
    total = torch.tensor(float(HW)) * cpg
    mean, var = torch.zeros(N, G), torch.zeros(N, G)
    for n in range(N):
        for g in range(G):
            m = pm[n, :, g * cpg:(g + 1) * cpg]               # [S, cpg]: e = s cpg + c
            mean[n, g] = _block_sum((cnt[:, None] * m).reshape(-1)) / total
            d = m - mean[n, g]
            var[n, g] = _block_sum((pq[n, :, g * cpg:(g + 1) * cpg] + cnt[:, None] * d * d).reshape(-1)) / total
    return mean, var


def _gn_apply(v, mean, var, w, b, eps, silu, G):
    """The (a, b) of the finalize kernel and gn_f32_apply_kernel on v [N, HW, C]; NCHW-shaped [N, C, HW] result."""
    N, HW, C = v.shape
    rstd = torch.rsqrt(var + eps).repeat_interleave(C // G, dim=1)         # [N, C]
    a = (torch.ones(C) if w is None else w) * rstd
    bb = (torch.zeros(C) if b is None else b) - mean.repeat_interleave(C // G, dim=1) * a
    o = _fma(v, a[:, None, :], bb[:, None, :])
    if silu:
        o = o / (1.0 + torch.exp(-o))
    return o.permute(0, 2, 1)


def _gn_values32(x, x2, pa):
    xin = x if x2 is None else torch.cat([x, x2], 1)
    N, C, H, W = xin.shape
    v = xin.reshape(N, C, H * W).permute(0, 2, 1)
    return (v if pa is None else v + pa[:, None, :]).contiguous(), N, C, H, W


def _emulate_gn(x, x2, G, w, b, eps, silu, pa):
    v, N, C, H, W = _gn_values32(x, x2, pa)
    pm, pq = _gn_partials(v, N, H * W, C)
    mean, var = _gn_finalize(pm, pq, N, H * W, C, G)
    return _gn_apply(v, mean, var, w, b, eps, silu, G).reshape(N, C, H, W)


@pytest.mark.parametrize("case", F32_GN_CASES)
@pytest.mark.parametrize("silu,pre", [(False, False), (True, True)])
def test_groupnorm_f32_emulation_within_bound(case, silu, pre):
    N, C1, C2, G, H, W = case
    x, x2, w, b, pa = f32_gn_inputs(N, C1, C2, H, W)
    pa = pa if pre else None
    ref, tol = groupnorm_f32_bound(x, G, w, b, 1e-6, silu, pa, x2)
    assert_within(_emulate_gn(x, x2, G, w, b, 1e-6, silu, pa), ref, tol, f"emulated f32 groupnorm {case} silu={silu} pre={pre}")


def test_groupnorm_f32_form_and_depth():
    """The mirror of gn_slices and of the lane count: the cases of the issue by hand."""
    assert gn_f32_form(2, 100, 320) == (3, 3) and gn_f32_bounds(2, 100, 320) == [0, 33, 66, 100]
    assert gn_f32_form(1, 64, 1280) == (2, 1) and gn_f32_form(2, 6, 1028) == (1, 1) and gn_f32_form(2, 1, 8) == (1, 128)
    assert gn_f32_form(4096, 4096, 64) == (1, 16) and gn_f32_form(1, 1 << 20, 64)[0] == 2048
    # 34 pixels over 3 lanes (12) + 3, the 2 merges, one finalize trip (30 partials), 6 + 3
    assert gn_f32_depth(2, 100, 320, 32) == (15, 15 + 2 + 1 + 9)
    assert gn_f32_depth(2, 6, 1028, 4) == (9, 9 + 0 + 2 + 9)            # C / G = 257: a second finalize trip


def test_groupnorm_f32_large_mean_and_one_pass_fault():
    """x = 300 + noise: the shifted kernel stays within the bound; a variance taken as E[x^2] - mean^2 on one group
    of small gamma passes the max-norm judge and is rejected."""
    N, C, G, H, W = 2, 64, 8, 10, 10
    x, _, w, b, _ = f32_gn_inputs(N, C, 0, H, W, seed=4)
    g = torch.Generator().manual_seed(5)
    x = 300.0 + torch.randn(N, C, H, W, generator=g)
    cpg = C // G
    w[:cpg] = 1e-3 * torch.randn(cpg, generator=g)
    b[:cpg] = 1e-4 * torch.randn(cpg, generator=g)
    ref, tol = groupnorm_f32_bound(x, G, w, b, 1e-6, False)
    assert_within(_emulate_gn(x, None, G, w, b, 1e-6, False, None), ref, tol, "emulated f32 groupnorm at mean 300")
    v, _, _, _, _ = _gn_values32(x, None, None)
    pm, pq = _gn_partials(v, N, H * W, C)
    mean, var = _gn_finalize(pm, pq, N, H * W, C, G)
    vals = v[:, :, :cpg].reshape(N, -1)                                   # group 0 of every image, in one pass
    s1, s2 = torch.cumsum(vals, 1)[:, -1], torch.cumsum(vals * vals, 1)[:, -1]
    m1 = s1 / vals.shape[1]
    mean[:, 0], var[:, 0] = m1, (s2 / vals.shape[1] - m1 * m1).clamp_min(0.0)
    y = _gn_apply(v, mean, var, w, b, 1e-6, False, G).reshape(N, C, H, W)
    assert _err(y, ref) < OLD_NORM
    _rejected(y, ref, tol, "f32 groupnorm: one-pass variance at mean 300")


# ------------------------------------------------------------------------------------------------ LayerNorm
def _emulate_ln(x, w, b, eps, short_mean_row=None):
    """ln_f32_kernel: lane l adds the float4s l, l + 64, ... each as (x + y) + (z + w), wave_sum; two passes."""
    rows, C = x.shape
    trips = (C // 4 + 63) // 64
    xp, ok = torch.zeros(rows, trips * 256), torch.zeros(rows, trips * 256)
    xp[:, :C], ok[:, :C] = x, 1.0
    xp, ok = xp.reshape(rows, trips, 64, 4), ok.reshape(rows, trips, 64, 4)
    s = torch.zeros(rows, 64)
    for i in range(trips):
        t = xp[:, i]
        s = s + ((t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3]))
    mean = _butterfly(s) / C
    if short_mean_row is not None:        # the fault: the last float4 of this row missing from the mean
        mean[short_mean_row] = x[short_mean_row, :C - 4].sum() / (C - 4)
    q = torch.zeros(rows, 64)
    for i in range(trips):
        d = (xp[:, i] - mean[:, None, None]) * ok[:, i]
        q = q + ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + (d[..., 2] * d[..., 2] + d[..., 3] * d[..., 3]))
    rstd = torch.rsqrt(_butterfly(q) / C + eps)
    o = (x - mean[:, None]) * rstd[:, None]
    if w is not None:
        o = o * w
    return o if b is None else o + b


@pytest.mark.parametrize("C", F32_LN_C)
@pytest.mark.parametrize("rows", F32_LN_ROWS)
def test_layernorm_f32_emulation_within_bound(rows, C):
    for shift in (0.0, 1000.0):
        x, w, b = f32_ln_inputs(rows, C, shift=shift)
        for wa, ba in ((w, b), (None, b), (w, None), (None, None)):
            ref, tol = layernorm_bound(x, wa, ba, 1e-5, depth=ln_f32_depth(C))
            assert_within(_emulate_ln(x, wa, ba, 1e-5), ref, tol, f"emulated f32 layernorm {rows}x{C} shift {shift}")


def test_layernorm_f32_fault_short_mean():
    """The mean of one row of a low-scale image taken over C - 4 elements."""
    rows, C = 5, 1280
    x, w, b = f32_ln_inputs(rows, C, seed=2)
    row = int(x.abs().mean(1).argmin())
    x[row, C - 4:] = 0.1 * x[row, C - 8:C - 4]                   # no spike in the float4 the fault drops
    ref, tol = layernorm_bound(x, w, b, 1e-5, depth=ln_f32_depth(C))
    y = _emulate_ln(x, w, b, 1e-5, short_mean_row=row)
    assert _err(y, ref) < OLD_NORM
    _rejected(y, ref, tol, "f32 layernorm: the mean over C - 4 elements")


# ------------------------------------------------------------------------------------------------ attention
def _emulate_attention(q, k, v, heads, mask=None, causal=False, kp=None, pad_fault_head=None):
    """ops.f32.attention: S = Q K^T / sqrt D into rows of stride ld = ceil4(Sk) whose pad columns hold -inf, the
    masks, the row softmax over ld columns (max, sum of exp, exp times the reciprocal), O = P V over K = Sk."""
    B, Sq, HD = q.shape
    Sk, D = k.shape[1], HD // heads
    ld = (Sk + 3) // 4 * 4
    o = torch.zeros(B, Sq, HD)
    m4 = None
    if mask is not None:
        m4 = mask
        if m4.dtype == torch.bool:
            m4 = torch.zeros(m4.shape).masked_fill(~m4, -math.inf)
        while m4.dim() < 4:
            m4 = m4.unsqueeze(0) if m4.dim() < 3 else m4.unsqueeze(1)
        m4 = m4.expand(B, heads, Sq, Sk)
    for bi in range(B):
        for h in range(heads):
            hs = slice(h * D, (h + 1) * D)
            s = torch.full((Sq, ld), -math.inf)
            s[:, :Sk] = _emulate_gemm(q[bi, :, hs], k[bi, :, hs], alpha=1.0 / math.sqrt(D))
            if h == pad_fault_head:
                s[:, Sk:] = 0.0
            if m4 is not None:
                s[:, :Sk] += m4[bi, h]
            if causal:
                s[:, :Sk].masked_fill_(torch.ones(Sq, Sk, dtype=torch.bool).triu(1), -math.inf)
            if kp is not None:
                s[:, :Sk].masked_fill_(~kp[bi][None, :], -math.inf)
            e = torch.exp(s - s.amax(-1, keepdim=True))
            p = e * (1.0 / e.sum(-1, keepdim=True))
            o[bi, :, hs] = _emulate_gemm(p, v[bi, :, hs].t().contiguous(), K=Sk)
    return o


def _attn_masks(B, heads, Sq, Sk, kind):
    g = torch.Generator().manual_seed(9)
    mask = kp = None
    if kind == "padding":
        kp = torch.ones(B, Sk, dtype=torch.bool)
        for bi in range(B):
            kp[bi, Sk - 1 - 13 * bi - 5:] = False
    elif kind == "float":
        mask = 2.0 * torch.randn(B, 1, Sq, Sk, generator=g)
    elif kind == "bool":
        mask = torch.rand(Sq, Sk, generator=g) > 0.3
        mask[:, 0] = True
    return mask, kind == "causal", kp


@pytest.mark.parametrize("kind", ["plain", "causal", "padding", "float", "bool"])
def test_attention_f32_emulation_within_bound(kind):
    B, heads, Sq, Sk, D = 2, 3, 130, 77, 40
    q, k, v, _ = f32_attn_inputs(B, heads, Sq, Sk, D)
    mask, causal, kp = _attn_masks(B, heads, Sq, Sk, kind)
    ref, tol = attention_f32_bound(q, k, v, heads, mask, causal, kp)
    assert_within(_emulate_attention(q, k, v, heads, mask, causal, kp), ref, tol, f"emulated f32 attention {kind}")


@pytest.mark.parametrize("B,heads,Sq,Sk,D", [(1, 2, 5, 1, 4), (1, 1, 1, 3, 8)])
def test_attention_f32_emulation_tiny(B, heads, Sq, Sk, D):
    q, k, v, _ = f32_attn_inputs(B, heads, Sq, Sk, D)
    ref, tol = attention_f32_bound(q, k, v, heads)
    assert_within(_emulate_attention(q, k, v, heads), ref, tol, f"emulated f32 attention {B}x{heads}x{Sq}x{Sk}x{D}")


def test_attention_f32_blocked_row_is_nan_in_the_bound():
    B, heads, Sq, Sk, D = 1, 2, 9, 6, 8
    q, k, v, _ = f32_attn_inputs(B, heads, Sq, Sk, D)
    mask = torch.ones(Sq, Sk, dtype=torch.bool)
    mask[4] = False
    ref, tol = attention_f32_bound(q, k, v, heads, mask)
    y = _emulate_attention(q, k, v, heads, mask)
    assert bool(torch.isnan(ref[:, 4]).all()) and bool(torch.isnan(tol[:, 4]).all()) and bool(torch.isnan(y[:, 4]).all())
    rows = [i for i in range(Sq) if i != 4]
    assert_within(y[:, rows], ref[:, rows], tol[:, rows], "emulated f32 attention beside a blocked row")


def test_attention_f32_fault_pad_columns_zero():
    """The pad columns Sk .. ld of the score rows left at 0 instead of -inf for the head of the smallest values."""
    B, heads, Sq, Sk, D = 2, 3, 130, 77, 40
    q, k, v, s_h = f32_attn_inputs(B, heads, Sq, Sk, D)
    h = int(s_h.reshape(heads, D)[:, 0].argmin())
    ref, tol = attention_f32_bound(q, k, v, heads)
    y = _emulate_attention(q, k, v, heads, pad_fault_head=h)
    assert _err(y, ref) < OLD_NORM
    _rejected(y, ref, tol, "f32 attention: pad columns of the scores at 0")
