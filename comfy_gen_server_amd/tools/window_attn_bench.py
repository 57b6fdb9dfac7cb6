"""Fused shifted-window attention against the composed path (profiles/r14/window_attn.md).

In one process on one device, ``CGS_WINDOW_ATTN=0`` and ``1`` alternated, medians of ``--reps`` event-timed windows
of ``--iters`` calls after a warm-up, ``--rounds`` figures of each side:
  attend  the attention segment of one block (qkv projection, attention, proj and everything between) at dim 180,
          6 heads, one ``--hw``^2 tile: 8 x 8 windows (SwinIR), 8 x 8 cosine (Swin2SR), 16 x 16 (HAT's geometry);
          unshifted and shifted
  e2e     whole forwards of SwinIR-M, Swin2SR and HAT (dim 180, 6 groups of 6 blocks, random weights) on one
          ``--hw``^2 tile, with the relative output difference of the two paths
With random weights at dim 180 the K = 180 GEMMs run on the vendor library on both sides (K % 8 != 0).

  python -m comfy_gen_server_amd.tools.window_attn_bench [--hw 256] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

from .act_bench import timed


def swin_seed(kind, dim=180, ws=8, heads=6, layers=6, depth=6, nf=64):
    """Shape-defining keys of a SwinIR / Swin2SR / HAT state dict; the rest is initialised at random."""
    Z, b0 = torch.zeros, "layers.0.residual_group.blocks.0."
    sd = {"conv_first.weight": Z(dim, 3, 3, 3), b0 + "mlp.fc1.bias": Z(dim * 2),
          "conv_before_upsample.0.weight": Z(nf, dim, 3, 3), "upsample.0.weight": Z(4 * nf, nf, 3, 3),
          "conv_last.weight": Z(3, nf, 3, 3), b0 + "attn.relative_position_index": Z(ws * ws, ws * ws)}
    for i in range(layers):
        for j in range(depth):
            blk = f"layers.{i}.residual_group.blocks.{j}."
            sd[blk + "norm1.weight"] = Z(dim)
            if kind == "hat":
                sd[blk + "conv_block.cab.0.weight"] = Z(dim // 3, dim, 3, 3)
                sd[blk + "conv_block.cab.3.attention.1.weight"] = Z(dim // 30, dim, 1, 1)
    if kind == "swin2sr":
        sd.update({"patch_embed.proj.weight": Z(dim, dim, 1, 1), b0 + "attn.logit_scale": Z(heads, 1, 1)})
    else:
        sd[b0 + "attn.relative_position_bias_table"] = Z((2 * ws - 1) ** 2, heads)
    if kind == "hat":
        ows = ws + ws // 2
        sd.update({"relative_position_index_SA": Z(ws * ws, ws * ws), "layers.0.conv.weight": Z(dim, dim, 3, 3),
                   "layers.0.residual_group.overlap_attn.relative_position_bias_table": Z((ws + ows - 1) ** 2, heads)})
    return sd


def swin_model(kind, seed=4, **shape):
    """A randomly initialised SwinIR / Swin2SR / HAT of ``swin_seed``'s shapes (fp32, CPU)."""
    from ..models import swin_sr
    from ..models.layers import init_random_
    sd = swin_seed(kind, **shape)
    m = swin_sr.HAT(sd, strict=False) if kind == "hat" else swin_sr.SwinIR(sd, v2=kind == "swin2sr", strict=False)
    init_random_(m, seed=seed)
    return m


def _alternate(fn, args, iters):
    """``rounds`` figures (us) of fn with the switch off and on, taking turns."""
    a, b = [], []
    for _ in range(args.rounds):
        for sw, dst in (("0", a), ("1", b)):
            os.environ["CGS_WINDOW_ATTN"] = sw
            dst.append(timed(fn, iters, args.reps))
    return a, b


def _row(name, a, b, **extra):
    row = {"what": name, "off_us": [round(v, 1) for v in a], "on_us": [round(v, 1) for v in b],
           "off_mean": round(statistics.mean(a), 1), "on_mean": round(statistics.mean(b), 1),
           "off_spread": round(max(a) - min(a), 1), **extra}
    print(json.dumps(row), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "window_attn_bench needs a GPU"
    from ..models import swin_sr
    from ..models.layers import init_random_
    dev, bf = torch.device("cuda", 0), torch.bfloat16
    hw = (args.hw, args.hw)
    rows = []
    with torch.inference_mode():
        x = torch.randn(1, args.hw * args.hw, 180, generator=torch.Generator().manual_seed(0)).to(dev, bf)
        for name, ws, v2 in (("ws8", 8, False), ("ws8 cosine", 8, True), ("ws16", 16, False)):
            for shift in (0, ws // 2):
                blk = swin_sr.SwinBlock(180, 6, ws, shift, 2.0, 64, v2=v2)
                init_random_(blk, seed=1)
                blk = blk.eval().to(device=dev, dtype=bf)
                a, b = _alternate(lambda: blk._attend(x, hw), args, args.iters)
                rows.append(_row(f"attend {name} shift {shift}", a, b))
        img = torch.rand(1, 3, args.hw, args.hw, generator=torch.Generator().manual_seed(1)).to(dev, bf)
        for kind, ws in (("swinir", 8), ("swin2sr", 8), ("hat", 16)):
            m = swin_model(kind, ws=ws).to(device=dev, dtype=bf)
            out = {}
            for sw in ("0", "1"):
                os.environ["CGS_WINDOW_ATTN"] = sw
                out[sw] = m(img).float()
            diff = ((out["1"] - out["0"]).norm() / out["0"].norm()).item()
            a, b = _alternate(lambda: m(img), args, max(1, args.iters // 5))
            rows.append(_row(f"e2e {kind} ws {ws}", a, b, rel_diff=round(diff, 5)))
            del m
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
