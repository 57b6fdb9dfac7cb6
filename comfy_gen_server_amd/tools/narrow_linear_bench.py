"""The narrow-K linear with fused LayerNorm against the composed path (profiles/r15/narrow_linear.md).

In one process on one device, ``CGS_NARROW_LINEAR=0`` and ``1`` alternated, medians of ``--reps`` event-timed windows
of ``--iters`` calls after a warm-up, ``--rounds`` figures of each side, at ``--hw``^2 tokens:
  linear  the four linears of a block at dim 180 and dim 60, each alone, as the blocks call them: off = the composed
          ops (LayerNorm, linear, F.gelu, add), on = one ``ops.narrow_linear`` launch
  ln      the row LayerNorm alone and with the res-post-norm residual (off: LayerNorm, add)
  e2e     whole forwards of SwinIR-M, Swin2SR and HAT (dim 180, 6 groups of 6 blocks, random weights) on one
          ``--hw``^2 tile, with the relative output difference of the two paths
``gbs``: the bytes the fused form has to move (x, y and the residual once each, 2 bytes an element; weights not
counted) over the on side's mean time -- the achieved rate of the new kernel, not of the composed path.

  python -m comfy_gen_server_amd.tools.narrow_linear_bench [--hw 256] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

from .act_bench import timed
from .window_attn_bench import swin_model


def _alternate(fn_off, fn_on, args, iters):
    """``rounds`` figures (us) of the off and the on side, taking turns."""
    a, b = [], []
    for _ in range(args.rounds):
        for sw, fn, dst in (("0", fn_off, a), ("1", fn_on, b)):
            os.environ["CGS_NARROW_LINEAR"] = sw
            dst.append(timed(fn, iters, args.reps))
    return a, b


def _row(name, a, b, nbytes=None, **extra):
    row = {"what": name, "off_us": [round(v, 1) for v in a], "on_us": [round(v, 1) for v in b],
           "off_mean": round(statistics.mean(a), 1), "on_mean": round(statistics.mean(b), 1),
           "off_spread": round(max(a) - min(a), 1), **extra}
    if nbytes is not None:
        row["gbs"] = round(nbytes / statistics.mean(b) / 1e3, 1)       # bytes / us / 1e3 = GB/s
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
    assert torch.cuda.is_available(), "narrow_linear_bench needs a GPU"
    from .. import ops
    dev, bf = torch.device("cuda", 0), torch.bfloat16
    T = args.hw * args.hw
    g = torch.Generator().manual_seed(0)
    rows = []

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(dev, bf)

    with torch.inference_mode():
        for C in (180, 60):
            x, h, r = rnd(T, C), rnd(T, 2 * C), rnd(T, C)
            gam, bet = rnd(C, scale=0.1) + 1, rnd(C, scale=0.1)
            ln = (gam, bet, 1e-5)
            # name -> (input, N, ln, act, residual)
            for name, (a, N, lnp, act, res) in {"ln->qkv": (x, 3 * C, ln, None, None), "proj+res": (x, C, None, None, r),
                                                "ln->fc1+gelu": (x, 2 * C, ln, "gelu", None),
                                                "fc2+res": (h, C, None, None, r)}.items():
                K = a.shape[-1]
                w, b = rnd(N, K, scale=K ** -0.5), rnd(N, scale=0.1)

                def off(a=a, w=w, b=b, lnp=lnp, act=act, res=res):
                    y = ops.linear(a if lnp is None else ops.layer_norm(a, *lnp), w, b)
                    y = F.gelu(y) if act else y
                    return y if res is None else res + y

                def on(a=a, w=w, b=b, lnp=lnp, act=act, res=res):
                    return ops.narrow_linear(a, w, b, ln=lnp, act=act, residual=res)

                ta, tb = _alternate(off, on, args, args.iters)
                rows.append(_row(f"linear dim {C} {name} K {K} N {N}", ta, tb,
                                 nbytes=2 * T * (K + N + (N if res is not None else 0))))
            for name, res in (("ln", None), ("ln+res", r)):
                ta, tb = _alternate(lambda: ops.layer_norm(x, gam, bet, 1e-5) if res is None
                                    else res + ops.layer_norm(x, gam, bet, 1e-5),
                                    lambda: ops.layer_norm(x, gam, bet, 1e-5, residual=res), args, args.iters)
                rows.append(_row(f"{name} dim {C}", ta, tb, nbytes=2 * T * C * (2 if res is None else 3)))
        img = torch.rand(1, 3, args.hw, args.hw, generator=torch.Generator().manual_seed(1)).to(dev, bf)
        for kind, ws in (("swinir", 8), ("swin2sr", 8), ("hat", 16)):
            m = swin_model(kind, ws=ws).to(device=dev, dtype=bf)
            out = {}
            for sw in ("0", "1"):
                os.environ["CGS_NARROW_LINEAR"] = sw
                out[sw] = m(img).float()
            diff = ((out["1"] - out["0"]).norm() / out["0"].norm()).item()
            ta, tb = _alternate(lambda: m(img), lambda: m(img), args, max(1, args.iters // 5))
            rows.append(_row(f"e2e {kind} ws {ws}", ta, tb, rel_diff=round(diff, 5)))
            del m
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
