"""Per-element worst-case error bounds of the bf16 GEMM, conv and attention kernels (test_kernel_bounds_*.py) and
of the bf16 / fp16 GroupNorm, LayerNorm, depthwise-conv and softmax2 kernels (test_norm_bounds_gpu.py).

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
TINY = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -126}


def u(dtype):
    """Unit roundoff of a 16-bit storage type."""
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def f64(t):
    return None if t is None else t.detach().to(torch.float64)


def _store(ref):
    return U * ref.abs() * (1 + 2 * U)


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


def gemm_bound(a, w, bias=None, res=None, alpha=1.0, K=None):
    """out = alpha a w^T + bias + res. a [M, K], w [N, K] (fp8 weights: pass them decoded, the decode is exact)."""
    K = a.shape[-1] if K is None else K
    pre, mag = _pre_mag(a, w, bias, alpha)
    ref, tol = pre, 0.0
    if res is not None:
        res = f64(res)
        ref = pre + res
        mag = mag + res.abs()
        tol = U * pre.abs()
    return ref, _store(ref) + tol + C_ACC * K * E * mag


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


def lnfold_bound(a, w2, b2, rs, cs, geglu=False):
    """The LayerNorm-folded GEMM from the operands the kernel is given: out = rstd (a w2^T - mean cs) + b2, with
    rs [M, 2] = (mean, rstd) per row, w2 = W gamma (bf16), cs = rowsum(w2) (fp32), b2 (bf16). Judges the kernel's
    arithmetic only; mag also takes |rstd mean cs|. geglu: w2 / cs / b2 in the plain row order."""
    K = a.shape[-1]
    a, w2, b2, rs, cs = f64(a), f64(w2), f64(b2), f64(rs), f64(cs)
    mu, rstd = rs[:, :1], rs[:, 1:2]
    ref = rstd * (a @ w2.t() - mu * cs[None, :])
    mag = rstd.abs() * (a.abs() @ w2.abs().t()) + (rstd * mu * cs[None, :]).abs()
    if b2 is not None:
        ref = ref + b2
        mag = mag + b2.abs()
    if geglu:
        (x1, g), (m1, mg) = ref.chunk(2, dim=-1), mag.chunk(2, dim=-1)
        return _geglu_tol(x1, g, C_ACC * K * E * m1, C_ACC * K * E * mg)
    return ref, _store(ref) + C_ACC * K * E * mag


# ------------------------------------------------------------------------------------------------ conv
def conv_bound(x, w, bias=None, res=None, stride=1, pad=0, upsample2x=False, x2=None):
    """out = conv2d(x (cat x2) (nearest 2x), w) + bias + res in NCHW; K = Cin kh kw."""
    x, w, bias, res = f64(x), f64(w), f64(bias), f64(res)
    if x2 is not None:
        x = torch.cat([x, f64(x2)], 1)
    if upsample2x:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    K = w.shape[1] * w.shape[2] * w.shape[3]
    pre = F.conv2d(x, w, bias, stride, pad)
    mag = F.conv2d(x.abs(), w.abs(), None if bias is None else bias.abs(), stride, pad)
    ref, tol = pre, 0.0
    if res is not None:
        ref = pre + res
        mag = mag + res.abs()
        tol = U * pre.abs()
    return ref, _store(ref) + tol + C_ACC * K * E * mag


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


def _gn_stats(x, pre, groups, ppb=None):
    """fp64 (mean, var) per (n, g) of v = x + pre and their worst-case fp32 errors; all [N, G, 1]."""
    N, C, H, W = x.shape
    v = (x + pre[:, :, None, None]).reshape(N, groups, -1)
    n = v.shape[-1]
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    dev2 = ((v - mean) ** 2).amax(-1, keepdim=True)
    R = v.abs().amax(-1, keepdim=True) + 3 * (v.amax(-1, keepdim=True) - v.amin(-1, keepdim=True))
    if ppb is None:
        Lb = L = n
        E2 = 2 * var + 2 * dev2
    else:
        Lb, L = gn_depth(H * W, C // groups, ppb)
        xr = x.reshape(N, C, H * W)
        d2 = torch.cat([(xr[:, :, p:p + ppb] - xr[:, :, p:p + 1]) ** 2 for p in range(0, H * W, ppb)], -1)
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
        ref, d = _silu(ref, d)
    return ref, _store_dt(ref, d, dtype)


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


def _ln_stats(x, eps):
    """Two-pass row statistics of x [rows, C] in fp64 and their worst-case fp32 errors; all [rows, 1]."""
    C = x.shape[-1]
    L = ln_depth(C)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    dmean = C_ACC * L * E * x.abs().mean(-1, keepdim=True) + E * mean.abs()
    dvar = C_ACC * (L + 4) * E * var + dmean ** 2
    rstd = 1 / torch.sqrt(var + eps)
    return mean, rstd, dmean, 0.5 * dvar / (var + eps) + RSQRT_REL


def layernorm_bound(x, w=None, b=None, eps=1e-5):
    """LayerNorm over the last dim; weight and bias optional."""
    dtype, shape = x.dtype, x.shape
    x = f64(x).reshape(-1, shape[-1])
    mean, rstd, dmean, drstd_rel = _ln_stats(x, eps)
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
