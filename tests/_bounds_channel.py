"""Per-element worst-case bound of the channel attention kernels (test_channel_attention_gpu.py), beside
_bounds_window.py. The reference is fp64 from the bf16 inputs; the bound follows cgs_channel_attn_fwd
(csrc/kernels/channel_attn.hip) step by step, e = 2^-24, U = 2^-8:

G and the norms. A chunk of L tokens is summed by four waves, a wave its L / 4 tokens on the MFMA (order inside unknown:
C_ACC), then 3 additions over the waves and at most nchunks over the chunks: Kg = L / 4 + 3 + nchunks. A squared norm is
summed by a lane over its L / 16 tokens (the squares are exact), then 2 shuffles, 3 waves, the chunks: Kn = L / 16 + 5 +
nchunks, every term positive, so relative. With a = max(nq, 1e-12), b likewise, sum |q| |k| <= a b (Cauchy-Schwarz):
  |dG| / (a b) <= C_ACC Kg e
  r = 1 / max(sqrt(n2), 1e-12): Kn e / 2 (the root halves it) + RSQRT_REL (the root) + RCP_REL (the division)
  s = fl(fl(G rq) rk), x = fl(s t):  |dx| <= |t| (C_ACC Kg e + |s| (Kn e + 2 RSQRT_REL + 2 RCP_REL + 2 e)) + e |x|
Softmax, as _bounds_window.py, M = max(1, row max of |x|): p = exp2(fl(fl(x - mx) L)) has the relative error
dX + 6 e M + EXP2_REL with dX the row's largest |dx| (the error of mx moves the whole row and cancels); the normaliser
has the same, 32 e for its additions, RCP_REL for 1 / sum and e for the product:
  rp = expm1(2 (dX + 6 e M + EXP2_REL)) + 33 e + RCP_REL
P is rounded to bf16: U (1 + rp). The apply adds at most 32 products in fp32 on the MFMA: C_ACC 32 e. With
A = sum_j P |v|:   tol = _store(ref) + (rp + U (1 + rp) + C_ACC 32 e) A (1 + U).
"""
import torch

from _bounds import C_ACC, E, EXP2_REL, RCP_REL, RSQRT_REL, U, _store, f64


def channel_attention_probs(qkv, heads, temperature):
    """fp64 (P [B, h, D, D], x = temperature s, v [B, h, N, D]) of bf16-rounded qkv [B, N, 3 heads D]."""
    B, N, C3 = qkv.shape
    D = C3 // 3 // heads
    q, k, v = f64(qkv).view(B, N, 3, heads, D).permute(2, 0, 3, 1, 4).unbind(0)          # [B, h, N, D]
    nq, nk = q.norm(dim=2).clamp_min(1e-12), k.norm(dim=2).clamp_min(1e-12)               # [B, h, D]
    x = (q.transpose(-1, -2) @ k) / (nq[..., :, None] * nk[..., None, :]) * f64(temperature).reshape(1, heads, 1, 1)
    return torch.softmax(x, -1), x, v


def channel_attention_bound(qkv, heads, temperature, chunk=None):
    """-> (ref, tol) [B, N, heads D]; ``chunk`` = cgs_channel_attn_chunk's L for this shape (None: one chunk holds
    all N tokens, the deepest sum any split can have)."""
    B, N, C3 = qkv.shape
    chunk = chunk or -(-N // 128) * 128
    P, x, v = channel_attention_probs(qkv, heads, temperature)
    L = min(chunk, -(-N // 128) * 128)
    nchunks = -(-N // chunk)
    Kg, Kn = L // 4 + 3 + nchunks, L // 16 + 5 + nchunks
    t = f64(temperature).reshape(1, heads, 1, 1).abs()
    dx = C_ACC * Kg * E * t + x.abs() * (Kn * E + 2 * RSQRT_REL + 2 * RCP_REL + 3 * E)
    M = x.abs().amax(-1, keepdim=True).clamp_min(1.0)
    rp = torch.expm1(2 * (dx.amax(-1, keepdim=True) + 6 * E * M + EXP2_REL)) + 33 * E + RCP_REL     # [B, h, D, 1]
    ref = (v @ P.transpose(-1, -2)).permute(0, 2, 1, 3).reshape(B, N, C3 // 3)
    A = v.abs() @ P.transpose(-1, -2)                                                                 # [B, h, N, D]
    d = (rp + U * (1 + rp) + C_ACC * 32 * E).transpose(-1, -2) * A
    return ref, _store(ref) + d.permute(0, 2, 1, 3).reshape(B, N, C3 // 3) * (1 + U)
