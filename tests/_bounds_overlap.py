"""Per-element worst-case bound of the fused overlapping cross-attention (test_overlap_attention_gpu.py), beside
_bounds_window.py.

    tol = masked_attention_bound's  +  kk e M A,    kk = 10 + 14 (NB - 1),   M = max(1, row max of |s| + |add|)

masked_attention_bound (q of the partitioned windows, k / v of the unfolded neighbourhoods, the gathered table as one
additive fp32 mask) grants the bf16 store, the bf16 rounding of P, the normaliser, fl(s c) and 4 e M A for x = fma(m, L,
fl(s c)). cgs_overlap_attn_fwd (csrc/kernels/overlap_attn.hip) takes the keys in NB bands (ws 8: 1, ws 16: 3) and
computes, per band with the running max m' (a max of fp32 values, exact) and L = fl(log2 e),

    x = fl(fl(s scale) + add);   p = exp2(fl(fl(x - m') L));   earlier bands: al = exp2(fl(fl(m - m') L)), fl(O al), fl(l al)

A key outside the image has s = 0 exactly and x = add. Relative error of a probability, natural-log units:
  e |x| <= e M              the addition of add
  e |x - m'| <= 2 e M       the subtraction of the running max (|m'| <= M)
  2 e |x - m'| <= 4 e M     the rounding of L and of the product
7 e M, and as much again from the normaliser: 14 e M A, of which the base has 4: 10, as _bounds_window.py. In exact
arithmetic the al of the later bands multiply p to exp((x - m_final)); each of the at most NB - 1 rescales a band
lives through adds
  e |m - m'| <= 2 e M       its subtraction
  2 e |m - m'| <= 4 e M     L and the product
  e                         the product of O (or l) by al; e <= e M with M >= 1, which is why M is clamped
7 e M a rescale, on the numerator and again on the normaliser: 14 (NB - 1) e M A. Single pass (NB = 1) has none.
"""
import torch

from _bounds import E, f64
from _bounds_mask import masked_attention_bound


def overlap_attention_bound(q, k, v, heads, add):
    """q [Bw, Nq, heads D], k / v [Bw, Nk, heads D] (bf16-rounded), add [Bw or 1, heads, Nq, Nk] fp32 -> (ref, tol)
    [Bw, Nq, heads D]. Nk = 144: single pass, 576: three bands."""
    Bw, Nq, HD = q.shape
    Nk, D = k.shape[1], HD // heads
    NB = {144: 1, 576: 3}[Nk]
    ref, tol = masked_attention_bound(q, k, v, heads, add)
    qh, kh = f64(q).reshape(Bw, Nq, heads, D).transpose(1, 2), f64(k).reshape(Bw, Nk, heads, D).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / D ** 0.5
    m = f64(add)
    p = torch.softmax(s + m, -1)
    M = (s.abs() + m.abs()).amax(-1, keepdim=True).clamp_min(1.0)
    A = p @ f64(v).reshape(Bw, Nk, heads, D).transpose(1, 2).abs()
    kk = 10 + 14 * (NB - 1)
    return ref, tol + (kk * E * M * A).transpose(1, 2).reshape(Bw, Nq, HD)
