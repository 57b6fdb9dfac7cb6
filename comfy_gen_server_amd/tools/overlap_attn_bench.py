"""Fused overlapping cross-attention (HAT's OCAB) against the composed path (profiles/r16/overlap_attn.md).

In one process on one device, ``CGS_OVERLAP_ATTN=0`` and ``1`` alternated, medians of ``--reps`` event-timed windows
of ``--iters`` calls after a warm-up, ``--rounds`` figures of each side:
  segment  the attention segment of one OCAB (qkv linear with norm1 through proj with the residual) at dim 180,
           6 heads, one ``--hw``^2 tile, for (ws, ows) = (16, 24) and (8, 12)
  e2e      the whole HAT forward (dim 180, 6 groups of 6 blocks and one OCAB each, ws 16, random weights) on one
           ``--hw``^2 tile, with the relative output difference of the two paths

  python -m comfy_gen_server_amd.tools.overlap_attn_bench [--hw 256] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

from .act_bench import timed
from .window_attn_bench import swin_model


def _segment(blk, x, hw):
    """qkv (norm1 folded in where the narrow kernel serves it), the attention, proj + residual: OCAB.forward's
    first half, on whichever path the switch selects."""
    from .. import ops
    from ..models.swin_sr import _ln, _narrow_ok
    if _narrow_ok(x, blk.qkv, blk.proj, blk.mlp.fc1, blk.mlp.fc2):
        qkv = ops.narrow_linear(x, blk.qkv.weight, blk.qkv.bias, ln=_ln(blk.norm1))
        o = blk.attend(qkv, hw)
        return ops.narrow_linear(o, blk.proj.weight, blk.proj.bias, residual=x)
    return blk.proj(blk.attend(blk.qkv(blk.norm1(x)), hw)) + x


def _alternate(fn, args, iters):
    """``rounds`` figures (us) of fn with the switch off and on, taking turns."""
    a, b = [], []
    for _ in range(args.rounds):
        for sw, dst in (("0", a), ("1", b)):
            os.environ["CGS_OVERLAP_ATTN"] = sw
            dst.append(timed(fn, iters, args.reps))
    return a, b


def _row(name, a, b, **extra):
    row = {"what": name, "off_us": [round(v, 1) for v in a], "on_us": [round(v, 1) for v in b],
           "off_mean": round(statistics.mean(a), 1), "on_mean": round(statistics.mean(b), 1),
           "off_spread": round(max(a) - min(a), 1), "on_spread": round(max(b) - min(b), 1), **extra}
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
    assert torch.cuda.is_available(), "overlap_attn_bench needs a GPU"
    from ..models import swin_sr
    from ..models.layers import init_random_
    dev, bf = torch.device("cuda", 0), torch.bfloat16
    hw = (args.hw, args.hw)
    rows = []
    with torch.inference_mode():
        x = torch.randn(1, args.hw * args.hw, 180, generator=torch.Generator().manual_seed(0)).to(dev, bf)
        for ws in (16, 8):
            blk = swin_sr.OCAB(180, 6, ws, 0.5, 2.0)
            init_random_(blk, seed=1)
            blk = blk.eval().to(device=dev, dtype=bf)
            out = {}
            for sw in ("0", "1"):
                os.environ["CGS_OVERLAP_ATTN"] = sw
                out[sw] = _segment(blk, x, hw).float()
            diff = ((out["1"] - out["0"]).norm() / out["0"].norm()).item()
            a, b = _alternate(lambda: _segment(blk, x, hw), args, args.iters)
            rows.append(_row(f"segment ws {ws} ows {blk.ows}", a, b, rel_diff=round(diff, 5)))
        img = torch.rand(1, 3, args.hw, args.hw, generator=torch.Generator().manual_seed(1)).to(dev, bf)
        m = swin_model("hat", ws=16).to(device=dev, dtype=bf)
        out = {}
        for sw in ("0", "1"):
            os.environ["CGS_OVERLAP_ATTN"] = sw
            out[sw] = m(img).float()
        diff = ((out["1"] - out["0"]).norm() / out["0"].norm()).item()
        a, b = _alternate(lambda: m(img), args, max(1, args.iters // 5))
        rows.append(_row("e2e hat ws 16", a, b, rel_diff=round(diff, 5)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
