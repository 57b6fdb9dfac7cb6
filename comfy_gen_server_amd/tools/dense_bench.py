"""Dense-block convs on channel slices against the concatenating path (profiles/r13/dense_block.md).

In one process on one device, old and new alternated, medians of ``--reps`` event-timed windows of ``--iters``
calls after a warm-up, ``--rounds`` figures of each side:
  conv    the five convs of one ESRGAN dense block (nf 64, gc 32) at one 512^2 image. old: the ``torch.cat`` the
          conv needs, the tuned ``ops.conv2d`` (activation included), and for conv5 the scale-and-add; new:
          ``ops.conv2d_into`` on the block's feature buffer. With achieved TFLOP/s and TB/s (input + output bytes).
  block   one ResidualDenseBlock5C and one RRDB, ``CGS_DENSE_CONV=0`` against ``1``
  e2e     23-block ESRGAN 4x, random weights, one 512^2 image (the model of tools/act_bench.py --e2e)
The default rule: the dense path is on when the RRDB's old mean exceeds the new mean by more than twice the spread
(max - min) of the old side's own figures of this run.

  python -m comfy_gen_server_amd.tools.dense_bench [--hw 512] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

from .act_bench import timed


def _alternate(old, new, args, iters):
    """``rounds`` figures (us) of each side, old and new taking turns."""
    a, b = [], []
    for _ in range(args.rounds):
        a.append(timed(old, iters, args.reps))
        b.append(timed(new, iters, args.reps))
    return a, b


def _row(name, a, b, **extra):
    row = {"what": name, "old_us": [round(v, 1) for v in a], "new_us": [round(v, 1) for v in b],
           "old_mean": round(statistics.mean(a), 1), "new_mean": round(statistics.mean(b), 1),
           "old_spread": round(max(a) - min(a), 1), **extra}
    row["gain_us"] = round(row["old_mean"] - row["new_mean"], 1)
    row["wins"] = row["gain_us"] > 2 * row["old_spread"]
    print(json.dumps(row), flush=True)
    return row


def conv_rows(args, dev):
    from .. import ops
    from ..models import upscalers
    from ..models.layers import init_random_fast_
    nf, gc, hw = 64, 32, args.hw
    m = upscalers.ResidualDenseBlock5C(nf, gc).to(device=dev, dtype=torch.bfloat16)
    init_random_fast_(m, seed=1)
    buf = torch.randn(1, nf + 4 * gc, hw, hw, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    nxt = torch.empty_like(buf)
    feats = [buf[:, :nf].contiguous(memory_format=torch.channels_last)] + \
        [buf[:, nf + i * gc:nf + (i + 1) * gc].contiguous(memory_format=torch.channels_last) for i in range(4)]
    rows = []
    for i in range(5):
        c = getattr(m, f"conv{i + 1}")[0]
        cin, cout = nf + i * gc, (nf if i == 4 else gc)
        wn = c.weight_nhwc()

        def old(i=i, c=c):
            x = torch.cat(feats[:i + 1], 1) if i else feats[0]
            if i < 4:
                return c(x, act="leaky_relu", act_param=0.2)
            return c(x) * 0.2 + feats[0]

        def new(i=i, c=c, cin=cin, wn=wn):
            if i < 4:
                return ops.conv2d_into(buf[:, :cin], c.weight, c.bias, buf[:, cin:cin + gc], weight_nhwc=wn,
                                       act="leaky_relu", act_param=0.2)
            return ops.conv2d_into(buf, c.weight, c.bias, nxt[:, :nf], weight_nhwc=wn, alpha=0.2, residual=buf[:, :nf])

        old()                      # (tunes the old path's conv)
        a, b = _alternate(old, new, args, args.iters)
        flop = 2.0 * hw * hw * 9 * cin * cout
        byts = 2.0 * hw * hw * (cin + cout + (nf if i == 4 else 0))
        nm = statistics.mean(b)
        rows.append(_row(f"conv{i + 1} {cin}->{cout} @ {hw}^2", a, b, new_tflops=round(flop / nm / 1e6, 1),
                         new_tbps=round(byts / nm / 1e6, 3), old_tflops=round(flop / statistics.mean(a) / 1e6, 1)))
    return rows


def _modes(fn):
    def run(mode):
        def go():
            os.environ["CGS_DENSE_CONV"] = mode
            return fn()
        return go
    return run("0"), run("1")


def block_rows(args, dev):
    from ..models import upscalers
    from ..models.layers import init_random_fast_
    rows = []
    x = torch.randn(1, 64, args.hw, args.hw, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    for name, mod in (("dense block (64, 32)", upscalers.ResidualDenseBlock5C(64, 32)), ("RRDB (64, 32)", upscalers.RRDB(64, 32))):
        mod = mod.to(device=dev, dtype=torch.bfloat16)
        init_random_fast_(mod, seed=2)
        old, new = _modes(lambda mod=mod: mod(x))
        old(), new()
        a, b = _alternate(old, new, args, max(1, args.iters // 5))
        rows.append(_row(f"{name} @ {args.hw}^2", a, b))
    return rows


def e2e_rows(args, dev):
    from ..models import upscalers
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g) * 0.03          # noqa: E731
    nf, gc, nb = 64, 32, 23
    sd = {"conv_first.weight": r(nf, 3, 3, 3), "conv_first.bias": r(nf)}
    for blk in range(nb):
        for j in range(1, 4):
            for c in range(1, 6):
                sd[f"body.{blk}.rdb{j}.conv{c}.weight"] = r(nf if c == 5 else gc, nf + (c - 1) * gc, 3, 3)
                sd[f"body.{blk}.rdb{j}.conv{c}.bias"] = r(nf if c == 5 else gc)
    for n_ in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
        sd[f"{n_}.weight"], sd[f"{n_}.bias"] = r(nf, nf, 3, 3), r(nf)
    sd["conv_last.weight"], sd["conv_last.bias"] = r(3, nf, 3, 3), r(3)
    m = upscalers.load_state_dict(sd).eval().to(device=dev, dtype=torch.bfloat16)
    x = torch.rand(1, 3, args.hw, args.hw, device=dev).to(torch.bfloat16)
    old, new = _modes(lambda: m(x))
    old(), new()
    a, b = [], []
    for _ in range(args.rounds):
        a.append(timed(old, 2, args.reps, warm=1))
        b.append(timed(new, 2, args.reps, warm=1))
    return [_row(f"ESRGAN 4x, 23 blocks, one {args.hw}^2 image", a, b)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--only", default="", help="conv, block or e2e")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dense_bench needs the GPU: timings elsewhere say nothing about it")
    dev = torch.device("cuda", 0)
    keep = os.environ.get("CGS_DENSE_CONV")
    res = {}
    with torch.inference_mode():
        for name, fn in (("conv", conv_rows), ("block", block_rows), ("e2e", e2e_rows)):
            if args.only in ("", name):
                res[name] = fn(args, dev)
    if keep is None:
        os.environ.pop("CGS_DENSE_CONV", None)
    else:
        os.environ["CGS_DENSE_CONV"] = keep
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
