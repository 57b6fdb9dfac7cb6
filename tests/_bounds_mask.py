"""Per-element worst-case bound of masked attention (test_attention_mask_gpu.py), beside _bounds.py.

    tol = u |ref| (1 + 2u) + 2 u A + 4 e M A + 1e-6,   A = p |v|,   M = max over a row's open keys of |s| + |m|

p is the fp64 softmax of s + m, s = q k^T / sqrt(D), with the mask m as the kernel receives it: a bf16 or fp32 mask
converts to fp64 exactly, fp16 is handed to the kernel as fp32 (exact) and bool as bf16 0 / -inf. The first, second and
last terms are attention_bound's (_bounds.py): the bf16 store, the bf16 rounding of P and the normaliser, the floor.

The third term is the addition of the mask. The kernel works in the exp2 domain: x = fma(m, L, fl(s c)) with L =
fl(log2 e) and c = fl(log2 e / sqrt(D)). fl(s c) is the unmasked kernel's own (inside attention_bound's margin). New
are the rounding of L, |m| log2(e) e, and the rounding of the fma, e |x| <= e log2(e) (|s| + |m|): together |dx| <= 2 e
log2(e) (|s| + |m|). A probability is proportional to 2^x, so its relative error is ln(2) |dx| <= 2 e (|s| + |m|); the
normalised probability carries that of its numerator and, at most, the same again from the normaliser: 4 e M over the
row's open keys (blocked keys have p = 0 exactly: -inf stays -inf through the fma). With |s| + |m| of a few tens this
is 1e-5 of A against 2 u = 8e-3: it is itemised, not needed to pass.

A row whose keys are all blocked has ref = 0 and tol = 1e-6 here (the kernel returns exact zeros, which the tests assert
separately); torch.softmax would give NaN.
"""
import math

import torch

from _bounds import E, U, _store, f64


def mask_as_kernel(mask):
    """The additive fp64 mask [.., Sq, Sk] (4-D, broadcastable) the kernel adds for ``mask`` as ops.attention takes it."""
    if mask.dtype == torch.bool:
        m = torch.zeros(mask.shape, dtype=torch.float64, device=mask.device).masked_fill(~mask, -math.inf)
    else:
        m = f64(mask)
    while m.ndim < 4:
        m = m.unsqueeze(0) if m.ndim < 3 else m.unsqueeze(1)
    return m


def masked_attention_bound(q, k, v, heads, mask, causal=False, key_padding=None):
    """q [B, Sq, H D], k / v [B, Sk, H D], mask as ops.attention takes it -> (ref, tol) [B, Sq, H D]."""
    B, Sq, HD = q.shape
    Sk, D = k.shape[1], HD // heads
    qh = f64(q).reshape(B, Sq, heads, D).transpose(1, 2)
    kh = f64(k).reshape(B, Sk, heads, D).transpose(1, 2)
    vh = f64(v).reshape(B, Sk, heads, D).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(D)
    m = mask_as_kernel(mask).to(s.device).expand(B, heads, Sq, Sk)
    x = s + m
    if causal:
        keep = torch.ones(Sq, Sk, dtype=torch.bool, device=s.device).tril()
        x = x.masked_fill(~keep, -math.inf)
    if key_padding is not None:
        x = x.masked_fill(~key_padding.bool()[:, None, None, :], -math.inf)
    open_ = torch.isfinite(x)
    dead = ~open_.any(-1, keepdim=True)
    p = torch.softmax(x.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0)
    M = torch.where(open_, s.abs() + m.abs(), torch.zeros_like(s)).amax(-1, keepdim=True)
    ref = (p @ vh).transpose(1, 2).reshape(B, Sq, HD)
    A = p @ vh.abs()
    tol = ((2 * U + 4 * E * M) * A).transpose(1, 2).reshape(B, Sq, HD)
    return ref, _store(ref) + tol + 1e-6
