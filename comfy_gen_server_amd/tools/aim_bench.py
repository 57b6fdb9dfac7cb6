"""Fused adaptive interaction module and token-layout gate conv of DAT against the composed path (profiles/r19/aim.md).

In one process on one device, ``CGS_DAT_AIM`` / ``CGS_DAT_SGATE`` = 0 and 1 alternated, medians of ``--reps``
event-timed windows of ``--iters`` calls after a warm-up, ``--rounds`` figures of each side, bf16, dim 180 / 6 heads
and dim 60 / 6 heads, one 256 x 256 tile and one 64 x 64 tile:
  segment  one block's attention module (``AdaptiveSpatialAttention.forward`` un-shifted, split 8 x 32, and
           ``AdaptiveChannelAttention.forward``: the qkv linear, the attention, the interaction module, proj)
  sgfn     one spatial-gate feed-forward (``_SGFN.forward``) at expansion 2 and 4
  e2e      the whole DAT forward (``--groups`` groups of 6 blocks, random weights), both switches together, with the
           relative output difference of the two paths

  python -m comfy_gen_server_amd.tools.aim_bench [--hw 256,64] [--dims 180,60] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

from .act_bench import timed
from .overlap_attn_bench import _row
from .rect_attn_bench import dat_model

SWITCHES = ("CGS_DAT_AIM", "CGS_DAT_SGATE")


def _set(sw):
    for name in SWITCHES:
        os.environ[name] = sw


def _alternate(fn, args, iters):
    """``rounds`` figures (us) of fn with the switches off and on, taking turns."""
    a, b = [], []
    for _ in range(args.rounds):
        for sw, dst in (("0", a), ("1", b)):
            _set(sw)
            dst.append(timed(fn, iters, args.reps))
    return a, b


def _both(fn):
    out = {}
    for sw in ("0", "1"):
        _set(sw)
        out[sw] = fn().float()
    return ((out["1"] - out["0"]).norm() / out["0"].norm()).item()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", default="256,64")
    ap.add_argument("--dims", default="180,60")
    ap.add_argument("--groups", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--e2e", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "aim_bench needs a GPU"
    from ..models.dat import AdaptiveChannelAttention, AdaptiveSpatialAttention, _SGFN
    from ..models.layers import init_random_
    dev, bf = torch.device("cuda", 0), torch.bfloat16
    rows = []
    saved = {k: os.environ.get(k) for k in SWITCHES}
    with torch.inference_mode():
        for dim in (int(d) for d in args.dims.split(",")):
            mods = {"segment spatial": AdaptiveSpatialAttention(dim, 6, [8, 32], False),
                    "segment channel": AdaptiveChannelAttention(dim, 6), "sgfn x2": _SGFN(dim, 2 * dim),
                    "sgfn x4": _SGFN(dim, 4 * dim)}
            for m in mods.values():
                init_random_(m, seed=1)
                m.eval().to(device=dev, dtype=bf)
            model = dat_model(dim, 6, args.groups).to(device=dev, dtype=bf) if args.e2e else None
            for hw in (int(s) for s in args.hw.split(",")):
                x = torch.randn(1, hw * hw, dim, generator=torch.Generator().manual_seed(0)).to(dev, bf)
                for name, m in mods.items():
                    diff = _both(lambda: m(x, hw, hw))
                    a, b = _alternate(lambda: m(x, hw, hw), args, args.iters)
                    rows.append(_row(f"{name} dim {dim} hw {hw}", a, b, rel_diff=round(diff, 5)))
                if model is not None:
                    img = torch.rand(1, 3, hw, hw, generator=torch.Generator().manual_seed(1)).to(dev, bf)
                    diff = _both(lambda: model(img))
                    a, b = _alternate(lambda: model(img), args, max(1, args.iters // 5))
                    rows.append(_row(f"e2e dat dim {dim} hw {hw}", a, b, rel_diff=round(diff, 5)))
    for k, v in saved.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
