"""Fused rectangular-window attention (DAT's spatial blocks) against the composed path (profiles/r18/rect_attn.md).

In one process on one device, ``CGS_RECT_ATTN=0`` and ``1`` alternated, medians of ``--reps`` event-timed windows of
``--iters`` calls after a warm-up, ``--rounds`` figures of each side, bf16, dim 180 / 6 heads and dim 60 / 6 heads,
splits 8 x 32 and 8 x 16, one 256 x 256 tile and one 64 x 64 tile:
  segment  one spatial block's attention (``AdaptiveSpatialAttention.forward``: the qkv linear, the two position MLPs,
           the attention, the conv branch, proj), un-shifted and shifted
  e2e      the whole DAT forward (``--groups`` groups of 6 blocks, random weights), with the relative output difference
           of the two paths

  python -m comfy_gen_server_amd.tools.rect_attn_bench [--hw 256,64] [--splits 8x32,8x16] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

from .act_bench import timed
from .overlap_attn_bench import _row


def dat_model(dim=180, heads=6, groups=6, depth=6, split=(8, 32), seed=4):
    """A randomly initialised DAT with ``split`` windows (pixelshuffle head, x2, expansion 2; fp32, CPU)."""
    from ..models.dat import DAT
    from ..models.layers import init_random_
    Z = torch.zeros
    sd = {"conv_first.weight": Z(dim, 3, 3, 3), "conv_before_upsample.0.weight": Z(64, dim, 3, 3),
          "upsample.0.weight": Z(256, 64, 3, 3), "conv_last.weight": Z(3, 64, 3, 3),
          "layers.0.blocks.1.attn.temperature": Z(heads, 1, 1), "layers.0.blocks.0.ffn.fc1.weight": Z(2 * dim, dim),
          "layers.0.blocks.0.attn.attns.0.rpe_biases": torch.tensor([[split[0] - 1.0, split[1] - 1.0]])}
    sd.update({f"layers.{i}.blocks.{j}.norm1.weight": Z(dim) for i in range(groups) for j in range(depth)})
    m = DAT(sd, strict=False)
    assert m.split_size == list(split)
    init_random_(m, seed=seed)
    return m


def _alternate(fn, args, iters):
    """``rounds`` figures (us) of fn with the switch off and on, taking turns."""
    a, b = [], []
    for _ in range(args.rounds):
        for sw, dst in (("0", a), ("1", b)):
            os.environ["CGS_RECT_ATTN"] = sw
            dst.append(timed(fn, iters, args.reps))
    return a, b


def _both(fn):
    out = {}
    for sw in ("0", "1"):
        os.environ["CGS_RECT_ATTN"] = sw
        out[sw] = fn().float()
    return ((out["1"] - out["0"]).norm() / out["0"].norm()).item()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", default="256,64")
    ap.add_argument("--dims", default="180,60")
    ap.add_argument("--splits", default="8x32,8x16")
    ap.add_argument("--groups", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--e2e", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "rect_attn_bench needs a GPU"
    from ..models.dat import AdaptiveSpatialAttention
    from ..models.layers import init_random_
    dev, bf = torch.device("cuda", 0), torch.bfloat16
    rows = []
    with torch.inference_mode():
        for split in ([int(v) for v in s.split("x")] for s in args.splits.split(",")):
            name = f"{split[0]}x{split[1]}"
            for dim in (int(d) for d in args.dims.split(",")):
                blks = {}
                for shifted in (False, True):
                    blk = AdaptiveSpatialAttention(dim, 6, split, shifted)
                    init_random_(blk, seed=1)
                    blks[shifted] = blk.eval().to(device=dev, dtype=bf)
                m = dat_model(dim, 6, args.groups, split=split).to(device=dev, dtype=bf) if args.e2e else None
                for hw in (int(s) for s in args.hw.split(",")):
                    x = torch.randn(1, hw * hw, dim, generator=torch.Generator().manual_seed(0)).to(dev, bf)
                    for shifted, blk in blks.items():
                        diff = _both(lambda: blk(x, hw, hw))
                        a, b = _alternate(lambda: blk(x, hw, hw), args, args.iters)
                        rows.append(_row(f"segment {name} {'shifted' if shifted else 'plain'} dim {dim} hw {hw}", a, b,
                                         rel_diff=round(diff, 5)))
                    if m is not None:
                        img = torch.rand(1, 3, hw, hw, generator=torch.Generator().manual_seed(1)).to(dev, bf)
                        diff = _both(lambda: m(img))
                        a, b = _alternate(lambda: m(img), args, max(1, args.iters // 5))
                        rows.append(_row(f"e2e dat {name} dim {dim} hw {hw}", a, b, rel_diff=round(diff, 5)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
