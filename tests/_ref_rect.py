"""fp64 reference of DAT's two-branch rectangular-window attention (test_rect_attention_gpu.py, _cpu.py) in plain
torch, with the per-element bound of _bounds_window.py: cgs_rect_attn_fwd (csrc/kernels/rect_attn.hip) is single pass
and keeps window_attn.hip's score arithmetic, x = fl(fl(s scale) + add), p = exp2(fl(fl(x - mx) L)), with
add = fl(table + -100), so window_attention_bound (plain scores) applies as it stands."""
import torch
import torch.nn.functional as F

from _bounds_window import window_attention_bound


def rect_attention_reference(qkv, H, W, split, shifted, heads, tables):
    """qkv [B, H*W, 3C] (as the kernel reads it), tables two fp32 [(2wh-1)(2ww-1), heads/2] -> (ref, tol) fp64
    [B, H*W, C]: per branch zero-pad, roll, partition, add = table[rel] + mask in fp32, the bound, and back."""
    B, C = qkv.shape[0], qkv.shape[-1] // 3
    h, Cb, m = heads // 2, C // 2, max(split)
    Hp, Wp = -(-H // m) * m, -(-W // m) * m
    x = F.pad(qkv.double().view(B, H, W, 3, C), (0, 0, 0, 0, 0, Wp - W, 0, Hp - H))
    refs, tols = [], []
    for i in range(2):
        wh, ww = (split[1], split[0]) if i else split
        sh, sw = (wh // 2, ww // 2) if shifted else (0, 0)
        t = torch.roll(x[..., i * Cb:(i + 1) * Cb], (-sh, -sw), (1, 2))

        def part(u):
            X = u.shape[-1]
            return u.reshape(-1, Hp // wh, wh, Wp // ww, ww, X).permute(0, 1, 3, 2, 4, 5).reshape(-1, wh * ww, X)

        yy, xx = (g.flatten() for g in torch.meshgrid(torch.arange(wh), torch.arange(ww), indexing="ij"))
        rel = (yy[:, None] - yy[None, :] + wh - 1) * (2 * ww - 1) + (xx[:, None] - xx[None, :] + ww - 1)   # [q, k]
        add = tables[i].float()[rel].permute(2, 0, 1)[None]
        if shifted:
            iy, ix = torch.arange(Hp), torch.arange(Wp)
            lab = 3 * ((iy >= Hp - wh).long() + (iy >= Hp - sh).long())[:, None] + \
                ((ix >= Wp - ww).long() + (ix >= Wp - sw).long())[None, :]
            lab = part(lab[None, :, :, None])[..., 0]                                  # [nW, N]
            mask = torch.where(lab[:, :, None] != lab[:, None, :], -100.0, 0.0).float()
            add = add + mask.repeat(B, 1, 1)[:, None]
        ref, tol = window_attention_bound(part(t[..., 0, :]), part(t[..., 1, :]), part(t[..., 2, :]), h,
                                          add.expand(B * (Hp // wh) * (Wp // ww), h, wh * ww, wh * ww))
        for dst, w in ((refs, ref), (tols, tol)):
            w = w.view(B, Hp // wh, Wp // ww, wh, ww, Cb).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, Cb)
            dst.append(torch.roll(w, (sh, sw), (1, 2))[:, :H, :W])
    return torch.cat(refs, -1).reshape(B, H * W, C), torch.cat(tols, -1).reshape(B, H * W, C)
