"""Per-element worst-case error bounds of the bf16 GEMM, conv and attention kernels (test_kernel_bounds_*.py).

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
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -8
E = 2.0 ** -24
C_ACC = 2
GELU_SLOPE = 1.13        # max |gelu'(x)| (1.129 at x = sqrt(2))
GELU_ABS = 2.6e-5        # absolute error bound of gelu_sig (csrc/kernels/common.h)


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
    ratio = (y - ref).abs() / tol
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
