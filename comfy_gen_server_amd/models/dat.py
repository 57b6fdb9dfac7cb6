"""DAT — Dual Aggregation Transformer super-resolution (parity: ``comfy_extras/chainner_models/
architecture/DAT.py:897-1182``). Residual groups alternate two block kinds:

* spatial blocks: the channels are split in half, each half attends inside rectangular windows
  (``split_size`` and its transpose) with a dynamic (MLP-generated) relative position bias and
  periodic half-window shifts (``ops.rect_window_attention`` on the packed qkv, ``CGS_RECT_ATTN``);
  a depthwise-conv branch on V is mixed in through the adaptive
  interaction module (channel map from the conv branch, spatial map from the attention branch;
  ``ops.adaptive_interaction``, ``CGS_DAT_AIM``);
* channel blocks: transposed (d x d) attention per head with a learned temperature
  (``ops.channel_attention`` on the packed qkv, ``CGS_CHANNEL_ATTN``), mixed with the same conv
  branch the other way round;

each followed by the spatial-gate feed-forward (SGFN; its gate conv is ``ops.token_dwconv3x3``,
``CGS_DAT_SGATE``). Projections are ``layers.Linear``, dense convs ``layers.Conv2d``; the depthwise convs and
BatchNorms stay torch modules as parameter holders, which the two ops read or, switched off, call. Shift masks and
position tables are derived from the geometry, not read from the file.
"""
from __future__ import annotations

import math
import re

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .layers import Conv2d, LayerNorm, Linear
from .swin_sr import _resi_conv, _Upsample, _to_img, _to_tokens


class _DynPosBias(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        p = dim // 4
        self.pos_proj = Linear(2, p)
        self.pos1 = nn.Sequential(LayerNorm(p), nn.ReLU(), Linear(p, p))
        self.pos2 = nn.Sequential(LayerNorm(p), nn.ReLU(), Linear(p, p))
        self.pos3 = nn.Sequential(LayerNorm(p), nn.ReLU(), Linear(p, heads))

    def forward(self, b):
        return self.pos3(self.pos2(self.pos1(self.pos_proj(b))))


class _RectWindowAttention(nn.Module):
    """One branch of the spatial block (``wh x ww`` windows over C/2 channels): its position MLP and table."""

    def __init__(self, dim, heads, wh, ww):
        super().__init__()
        self.heads, self.wh, self.ww = heads, wh, ww
        self.scale = (dim // heads) ** -0.5
        self.pos = _DynPosBias(dim // 4, heads)
        dh = torch.arange(1 - wh, wh)
        dw = torch.arange(1 - ww, ww)
        self.register_buffer("rpe_tab", torch.stack(torch.meshgrid(dh, dw, indexing="ij")).flatten(1).t().float(),
                             persistent=False)

    def table(self):
        """The branch's relative-position table [(2wh-1)(2ww-1), heads], fp32, from the position MLP."""
        return self.pos(self.rpe_tab.to(self.pos.pos_proj.weight.dtype)).float()


def _aim_branches(dim, hc=None, hs=None):
    """The parameter holders of the adaptive interaction module; hidden widths ``hc`` / ``hs`` default to dim / 8, / 16."""
    hc, hs = hc or dim // 8, hs or dim // 16
    dw = nn.Sequential(nn.Conv2d(dim, dim, 3, padding=1, groups=dim), nn.BatchNorm2d(dim), nn.GELU())
    ci = nn.Sequential(nn.AdaptiveAvgPool2d(1), Conv2d(dim, hc, 1), nn.BatchNorm2d(hc), nn.GELU(), Conv2d(hc, dim, 1))
    si = nn.Sequential(Conv2d(dim, hs, 1), nn.BatchNorm2d(hs), nn.GELU(), Conv2d(hs, 1, 1))
    return dw, ci, si


class AdaptiveSpatialAttention(nn.Module):
    def __init__(self, dim, heads, split, shifted: bool):
        super().__init__()
        self.split, self.shifted = split, shifted
        self.shift = [split[0] // 2, split[1] // 2]
        self.qkv = Linear(dim, dim * 3)
        self.proj = Linear(dim, dim)
        self.attns = nn.ModuleList([_RectWindowAttention(dim // 2, heads // 2, split[0], split[1]),
                                    _RectWindowAttention(dim // 2, heads // 2, split[1], split[0])])
        self.dwconv, self.channel_interaction, self.spatial_interaction = _aim_branches(dim)

    def forward(self, x, H, W):
        B, L, C = x.shape
        qkv = self.qkv(x)
        att = ops.rect_window_attention(qkv, (H, W), self.split, self.shifted, 2 * self.attns[0].heads,
                                        [a.table() for a in self.attns], scale=self.attns[0].scale,
                                        fused=ops.rect_window_attention_enabled(self.split))
        return self.proj(ops.adaptive_interaction(
            qkv, att, (H, W), (self.dwconv, self.channel_interaction, self.spatial_interaction), "spatial",
            fused=ops.adaptive_interaction_enabled()))


class AdaptiveChannelAttention(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.temperature = nn.Parameter(torch.ones(heads, 1, 1), requires_grad=False)
        self.qkv = Linear(dim, dim * 3)
        self.proj = Linear(dim, dim)
        self.dwconv, self.channel_interaction, self.spatial_interaction = _aim_branches(dim)

    def forward(self, x, H, W):
        B, N, C = x.shape
        h = self.heads
        qkv = self.qkv(x)
        att = ops.channel_attention(qkv, h, self.temperature, fused=ops.channel_attention_enabled())
        return self.proj(ops.adaptive_interaction(
            qkv, att, (H, W), (self.dwconv, self.channel_interaction, self.spatial_interaction), "channel",
            fused=ops.adaptive_interaction_enabled()))


class _SpatialGate(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm = LayerNorm(dim)
        self.conv = nn.Conv2d(dim, dim, 3, padding=1, groups=dim)

    def forward(self, x, H, W):
        a, g = x.chunk(2, -1)
        return ops.token_dwconv3x3(self.norm(g), (H, W), self.conv.weight, self.conv.bias, mul=a,
                                   fused=ops.token_dwconv_enabled())


class _SGFN(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = Linear(dim, hidden)
        self.sg = _SpatialGate(hidden // 2)
        self.fc2 = Linear(hidden // 2, dim)

    def forward(self, x, H, W):
        return self.fc2(self.sg(F.gelu(self.fc1(x)), H, W))


def _is_shifted(rg: int, b: int) -> bool:
    """Shift pattern of the reference: blocks 2, 6, 10… in even groups; 0, 4, 8… in odd groups."""
    return (rg % 2 == 0 and b > 0 and (b - 2) % 4 == 0) or (rg % 2 != 0 and b % 4 == 0)


class DATB(nn.Module):
    def __init__(self, dim, heads, split, expansion, rg, b):
        super().__init__()
        self.norm1 = LayerNorm(dim)
        if b % 2 == 0:
            self.attn = AdaptiveSpatialAttention(dim, heads, split, _is_shifted(rg, b))
        else:
            self.attn = AdaptiveChannelAttention(dim, heads)
        self.norm2 = LayerNorm(dim)
        self.ffn = _SGFN(dim, int(dim * expansion))

    def forward(self, x, hw):
        H, W = hw
        x = x + self.attn(self.norm1(x), H, W)
        return x + self.ffn(self.norm2(x), H, W)


class ResidualGroup(nn.Module):
    def __init__(self, dim, heads, split, expansion, depth, resi, rg):
        super().__init__()
        self.blocks = nn.ModuleList([DATB(dim, heads, split, expansion, rg, b) for b in range(depth)])
        self.conv = _resi_conv(dim, resi)

    def forward(self, x, hw):
        y = x
        for blk in self.blocks:
            y = blk(y, hw)
        return _to_tokens(self.conv(_to_img(y, hw))) + x


class DAT(nn.Module):
    def __init__(self, state_dict, strict: bool = True):
        super().__init__()
        sd = state_dict
        keys = set(sd)
        self.model_arch = "DAT"
        if "conv_before_upsample.0.weight" in keys and "conv_up1.weight" not in keys:
            up = "pixelshuffle"
        elif "upsample.0.weight" in keys and "conv_before_upsample.0.weight" not in keys:
            up = "pixelshuffledirect"
        else:
            raise ValueError("DAT: only the pixelshuffle / pixelshuffledirect heads exist in the reference")
        self.upsampler = up
        in_ch = sd["conv_first.weight"].shape[1]
        dim = sd["conv_first.weight"].shape[0]
        nf = 64
        if up == "pixelshuffle":
            upscale = 1.0
            for k in keys:
                if re.match(r"^upsample\.\d+\.weight$", k):
                    upscale *= math.sqrt(sd[k].shape[0] // nf)
            upscale = int(round(upscale))
        else:
            upscale = int(math.sqrt(sd["upsample.0.bias"].shape[0] // in_ch))
        blocks = [tuple(map(int, m.groups())) for k in keys
                  for m in [re.match(r"^layers\.(\d+)\.blocks\.(\d+)\.norm1\.weight$", k)] if m]
        n_layers = 1 + max(b[0] for b in blocks)
        depth = 1 + max(b[1] for b in blocks)
        heads = sd["layers.0.blocks.1.attn.temperature"].shape[0] if "layers.0.blocks.1.attn.temperature" in keys \
            else depth
        expansion = sd["layers.0.blocks.0.ffn.fc1.weight"].shape[0] / dim
        resi = "3conv" if "layers.0.conv.4.weight" in keys else "1conv"
        split = [2, 4]
        if "layers.0.blocks.0.attn.attns.0.rpe_biases" in keys:
            split = [int(v) + 1 for v in sd["layers.0.blocks.0.attn.attns.0.rpe_biases"][-1]]
        self.in_nc = self.out_nc = in_ch
        self.scale = self.upscale = upscale
        self.embed_dim, self.split_size, self.depth, self.num_heads = dim, split, [depth] * n_layers, [heads] * n_layers
        self.img_range = 1.0
        mean = torch.tensor([0.4488, 0.4371, 0.4040]).view(1, 3, 1, 1) if in_ch == 3 else torch.zeros(1, 1, 1, 1)
        self.register_buffer("mean", mean, persistent=False)
        self.conv_first = Conv2d(in_ch, dim, 3, padding=1)
        self.before_RG = nn.Sequential(nn.Identity(), LayerNorm(dim))
        self.layers = nn.ModuleList([ResidualGroup(dim, heads, split, expansion, depth, resi, i)
                                     for i in range(n_layers)])
        self.norm = LayerNorm(dim)
        self.conv_after_body = _resi_conv(dim, resi)
        if up == "pixelshuffle":
            self.conv_before_upsample = nn.Sequential(Conv2d(dim, nf, 3, padding=1), nn.LeakyReLU(0.01))
            self.upsample = _Upsample(upscale, nf)
            self.conv_last = Conv2d(nf, in_ch, 3, padding=1)
        else:
            self.upsample = nn.Sequential(Conv2d(dim, upscale ** 2 * in_ch, 3, padding=1), nn.PixelShuffle(upscale))
        missing, _ = self.load_state_dict(sd, strict=False)
        if missing and strict:
            raise ValueError(f"DAT: missing keys {missing[:4]}")
        self.eval()

    def forward(self, x):
        mean = self.mean.to(x.dtype)
        x = (x - mean) * self.img_range
        f = self.conv_first(x)
        hw = f.shape[-2:]
        t = self.before_RG[1](_to_tokens(f))
        for layer in self.layers:
            t = layer(t, hw)
        y = self.conv_after_body(_to_img(self.norm(t), hw)) + f
        if self.upsampler == "pixelshuffle":
            y = self.conv_last(self.upsample(self.conv_before_upsample(y)))
        else:
            y = self.upsample(y)
        return y / self.img_range + mean
