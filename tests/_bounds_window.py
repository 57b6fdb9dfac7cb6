"""Per-element worst-case bound of the fused window attention (test_window_attention_gpu.py), beside _bounds_mask.py.

    tol = masked_attention_bound's  +  k e M A,    k = 10 + [cosine] 2 (DP + 7)

masked_attention_bound (q, k, v of the partitioned windows; the table bias plus the shift mask as one additive fp32
mask, which is the kernel's own add = fl(table + -100)) grants the bf16 store, the bf16 rounding of P, the normaliser,
fl(s c) and 4 e M A for x = fma(m, L, fl(s c)). cgs_window_attn_fwd (csrc/kernels/window_attn.hip) instead computes

    x = fl(fl(s qs) + add);   p = exp2(fl(fl(x - mx) L)),  L = fl(log2 e)

with M >= |x| the row's max of |s| + |m|, in natural-log units of the exponent:
  e |x| <= e M             the addition of add (the "second addition")
  e |x - mx| <= 2 e M      the subtraction of the row max (the error of mx itself moves every exponent of the row alike
                           and cancels in the normalisation)
  2 e |x - mx| <= 4 e M    the rounding of L and of the product
7 e M relative on a probability and as much again from the normaliser: 14 e M A, of which the base has 4: k = 10.
cosine (SwinV2): s = (q . k) rq rk hs, every factor applied to the fp32 score. A norm is a sum of DP squares by
sequential fma (relative DP e), its square root (halves it, + e) and a division (e): (DP / 2 + 2) e each, (DP + 4) e for
the two; fl(scale hs), its product with rq, s qs and (.) rk are four roundings, one of which (s qs) the base grants as
fl(s c): (DP + 7) e |s| <= (DP + 7) e M more on x, and twice that through the normaliser: 2 (DP + 7) e M A. With |s| up
to 100 this is 2e-3 of A against 2 u = 8e-3: itemised, not a margin. The reference normalises in fp64 from the bf16
rows (the kernel rounds no normalised copy of q or k).
"""
import math

import torch

from _bounds import E, f64
from _bounds_mask import masked_attention_bound


def window_attention_bound(q, k, v, heads, add, cosine=False, head_scale=None):
    """q / k / v [Bw, N, heads D] (bf16-rounded, partitioned windows), add [Bw, heads, N, N] fp32 -> (ref, tol)
    [Bw, N, heads D]. Plain: s = q k^T / sqrt(D). cosine: s = cos(q, k) head_scale[h]."""
    Bw, N, HD = q.shape
    D = HD // heads
    DP = 32 if D <= 32 else 64
    qh, kh = f64(q).reshape(Bw, N, heads, D), f64(k).reshape(Bw, N, heads, D)
    if cosine:       # fold the exact norms and hs sqrt(D) into fp64 q, k: masked_attention_bound's s is then hs cos
        qh = qh / qh.norm(dim=-1, keepdim=True).clamp_min(1e-12) * (f64(head_scale).reshape(1, 1, heads, 1) * math.sqrt(D))
        kh = kh / kh.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    ref, tol = masked_attention_bound(qh.reshape(Bw, N, HD), kh.reshape(Bw, N, HD), v, heads, add)
    s = qh.transpose(1, 2) @ kh.transpose(1, 2).transpose(-1, -2) / math.sqrt(D)
    m = f64(add)
    p = torch.softmax(s + m, -1)
    M = (s.abs() + m.abs()).amax(-1, keepdim=True)
    A = p @ f64(v).reshape(Bw, N, heads, D).transpose(1, 2).abs()
    kk = 10 + (2 * (DP + 7) if cosine else 0)
    return ref, tol + (kk * E * M * A).transpose(1, 2).reshape(Bw, N, HD)
