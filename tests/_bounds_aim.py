"""Per-element worst-case bounds of the token-layout depthwise conv and of DAT's adaptive interaction module
(csrc/kernels/token_mix.hip; test_aim_gpu.py). The reference is fp64 in plain torch from the bf16 operands and
parameters; the bound follows the three kernels step by step, e = 2^-24, U = 2^-8:

conv: pre = b + nine fmas, dwconv_bound's form: d_pre = C_ACC (9 + 1) e mag, mag = sum |w| |x| + |b|.
_bn_gelu (one device function in all three kernels): s = gamma rsqrt(var + eps) has RSQRT_REL and the product (e), then
  pre - mean (e) and the fma with beta (e): d_z = |s| d_pre + (RSQRT_REL + 4 e)(|s (pre - mean)| + |beta|); gelu_sig:
  d_g = GELU_SLOPE d_z + GELU_ABS. token_dwconv3x3 stores round(g), or round(m pre): |m| d_pre + e |m pre|.
conv is rounded to bf16 before aim_mix_kernel reads it: d_conv = U |g| (1 + 2U) + d_g (1 + U).
Pool: a thread adds the 16 rows of its column in sequence, two shuffles join a wave's 4 columns, 3 additions the waves,
  aim_cmap_kernel adds the np patches in patch order and divides by N: Lp = 16 + 2 + 3 + np + 1,
  d_mean = C_ACC Lp e mean |v| (+ mean d_g where the pooled values are the conv's own fp32 output).
Channel gate: a = W1 mean + b1, a lane adds ceil(C / 64) products, wave_sum (6), the bias: d_a = |W1| d_mean + C_ACC
  (ceil(C / 64) + 7) e mag; _bn_gelu; x = W2 h + b2, hc fmas in sequence and the bias: C_ACC (hc + 1) e mag.
_sigmoid, rcp(1 + exp2(fl(-x L))), L the fp32 log2 e: the product is off by 2 e |x L|, 2 e |x| relative after the
  exponential (granted 4), then EXP2_REL, the addition of 1 (e), RCP_REL; the denominator's error is at most that of
  its exp term; the sigmoid's slope is at most 1 / 4: d = d_x / 4 + (4 |x| e + EXP2_REL + RCP_REL + 2 e) gate.
Token gate: a = W1 src + b1 on the MFMA over K = C products (the pads are exact zeros) plus the bias: d_a = |W1| d_src +
  C_ACC (C + 1) e mag, d_src = d_conv in a channel block (src = conv) and 0 in a spatial block (src = att, exact);
  _bn_gelu; the dot with w2 is 4 fmas in sequence, two shuffles and b2 over the padded 16: C_ACC (16 + 3) e mag.
Output y = fma(att, ga, fl(conv gb)): d = |att| d_ga + |g| d_gb + gb d_conv + d_conv d_gb + 3 e (|att ga| + |g gb|),
  tol = U |ref| (1 + 2U) + d (1 + U).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from _bounds import (C_ACC, E, EXP2_REL, GELU_ABS, GELU_SLOPE, RCP_REL, RSQRT_REL, U, _f32, _store, _store_dt, f64)

from comfy_gen_server_amd.models.dat import _aim_branches
from comfy_gen_server_amd.ops.core import _aim_tensors

BF = torch.bfloat16


def aim_modules(C, hc, hs, seed):
    """A DAT block's (dwconv, channel_interaction, spatial_interaction) with the seeded test parameters; eval, fp32."""
    g = torch.Generator().manual_seed(seed)
    mods = nn.ModuleList(_aim_branches(C, hc, hs)).eval()
    scale = {"0.0.weight": 1 / 3, "2.0.weight": C ** -0.5, "2.3.weight": 2.0}       # dwconv, spatial W1, spatial w2
    with torch.no_grad():
        for n, p in list(mods.named_parameters()) + list(mods.named_buffers()):
            if p.is_floating_point():
                r = torch.randn(p.shape, generator=g)
                p.copy_(0.5 + torch.rand(p.shape, generator=g) if n.endswith("var") else 0.1 * r if p.dim() == 1 else
                        scale.get(n, 1.0) * r)
                if p.dim() == 1 and n.endswith("weight"):                           # BatchNorm scale
                    p.copy_(1 + 0.2 * r)
    return mods


def _bn_gelu(pre, d_pre, w, b, mean, var, eps):
    s = w / torch.sqrt(var + _f32(eps))
    z = s * (pre - mean) + b
    d_z = s.abs() * d_pre + (RSQRT_REL + 4 * E) * ((s * (pre - mean)).abs() + b.abs())
    return F.gelu(z), GELU_SLOPE * d_z + GELU_ABS


def _sigmoid(x, d_x):
    g = torch.sigmoid(x)
    return g, d_x / 4 + (4 * x.abs() * E + EXP2_REL + RCP_REL + 2 * E) * g


def _conv(x, hw, w, bias):
    """(pre, d_pre) [B, N, C] of the depthwise conv of token rows x."""
    B, N, C = x.shape
    xi = f64(x).transpose(1, 2).reshape(B, C, *hw)
    w, b = f64(w), f64(bias)
    pre = F.conv2d(xi, w, b, 1, 1, 1, C)
    mag = F.conv2d(xi.abs(), w.abs(), None if b is None else b.abs(), 1, 1, 1, C)
    return pre.flatten(2).transpose(1, 2), C_ACC * 10 * E * mag.flatten(2).transpose(1, 2)


def token_dwconv_bound(x, hw, w, bias, bn=None, mul=None):
    """-> (ref, tol) [B, N, C] of ops.token_dwconv3x3; bn = (weight, bias, mean, var, eps): BatchNorm + GELU."""
    pre, d = _conv(x, hw, w, bias)
    if bn is not None:
        pre, d = _bn_gelu(pre, d, *(f64(t) for t in bn[:4]), bn[4])
    elif mul is not None:
        m = f64(mul)
        pre, d = m * pre, m.abs() * d + E * (m * pre).abs()
    return pre, _store_dt(pre, d, BF)


def aim_bound(qkv, att, hw, params, kind):
    """-> (ref, tol [B, N, C], token gates [B, N, 1], channel gates [B, 1, C]) of ops.adaptive_interaction, in fp64."""
    ts, eps = _aim_tensors(params)
    t = [f64(v) for v in ts]
    B, N, C3 = qkv.shape
    C, spatial = C3 // 3, kind == "spatial"
    hc, hs = t[6].shape[0], t[14].shape[0]
    A = f64(att)
    G, dG = _bn_gelu(*_conv(qkv[..., 2 * C:], hw, t[0], t[1]), *t[2:6], eps[0])
    dconv = _store(G) + dG * (1 + U)
    Lp = 16 + 2 + 3 + (-(-hw[0] // 16)) * (-(-hw[1] // 16)) + 1
    src = G if spatial else A
    mean = src.mean(1)
    dmean = C_ACC * Lp * E * src.abs().mean(1) + (dG.mean(1) if spatial else 0)                       # [B, C]
    W1, W2 = t[6].view(hc, C), t[12].view(C, hc)
    a = mean @ W1.t() + t[7]
    da = dmean @ W1.abs().t() + C_ACC * (-(-C // 64) + 7) * E * (mean.abs() @ W1.abs().t() + t[7].abs())
    h, dh = _bn_gelu(a, da, *t[8:12], eps[1])
    x = h @ W2.t() + t[13]
    cg, dcg = _sigmoid(x, dh @ W2.abs().t() + C_ACC * (hc + 1) * E * (h.abs() @ W2.abs().t() + t[13].abs()))
    cg, dcg = cg[:, None, :], dcg[:, None, :]
    s, ds = (A, torch.zeros_like(A)) if spatial else (G, dconv)
    W1, w2 = t[14].view(hs, C), t[20].view(hs)
    a = s @ W1.t() + t[15]
    da = ds @ W1.abs().t() + C_ACC * (C + 1) * E * (s.abs() @ W1.abs().t() + t[15].abs())
    h, dh = _bn_gelu(a, da, *t[16:20], eps[2])
    x = h @ w2 + t[21]
    tg, dtg = _sigmoid(x, dh @ w2.abs() + C_ACC * (16 + 3) * E * (h.abs() @ w2.abs() + t[21].abs()))
    tg, dtg = tg[..., None], dtg[..., None]
    ga, dga, gb, dgb = (cg, dcg, tg, dtg) if spatial else (tg, dtg, cg, dcg)
    ref = A * ga + G * gb
    d = A.abs() * dga + G.abs() * dgb + gb * dconv + dconv * dgb + 3 * E * ((A * ga).abs() + (G * gb).abs())
    return ref, _store(ref) + d * (1 + U), tg, cg
