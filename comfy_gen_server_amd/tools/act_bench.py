"""Per-shape timing of the activation epilogues (profiles/r07/act_epilogue.md).

For every conv -> activation and linear -> activation shape below, in one process on one device:
  before   the plain op by its tuned kernel choice, then the ATen activation (what the models ran before)
  split    the plain op, then the native in-place activation (``ops.activation``)
  fused    each kernel whose epilogue carries the activation
  tuned    what ``ops.conv2d(act=...)`` / ``ops.linear(act=...)`` picks with the autotuner on
Medians of ``--reps`` event-timed windows of ``--iters`` calls after a warm-up.

  python -m comfy_gen_server_amd.tools.act_bench [--e2e] [--out FILE]

``--e2e`` runs only the two end-to-end figures (23-block ESRGAN 4x on one 512^2 image, CLIP-L + CLIP-G text
towers on 8 prompts) with random weights; it uses nothing the activation work added, so the same file runs
against an older tree for the comparison.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F


def timed(fn, iters, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) * 1000.0 / iters)
    return statistics.median(out)


ATEN = {"leaky_relu": lambda y, p: F.leaky_relu(y, p), "relu": lambda y, p: torch.relu(y),
        "quick_gelu": lambda y, p: y * torch.sigmoid(1.702 * y), "gelu": lambda y, p: F.gelu(y)}


def conv_rows(args, dev):
    from .. import ops
    from ..ops import autotune
    rows = []
    # ESRGAN (nf 64, gc 32) at a 512^2 input: the four activated dense-block convs, the upsample conv; TAESD 64 -> 64
    shapes = [("esrgan rdb conv1", 64, 32, 512, False, "leaky_relu", 0.2), ("esrgan rdb conv2", 96, 32, 512, False, "leaky_relu", 0.2),
              ("esrgan rdb conv3", 128, 32, 512, False, "leaky_relu", 0.2), ("esrgan rdb conv4", 160, 32, 512, False, "leaky_relu", 0.2),
              ("esrgan upconv (2x)", 64, 64, 512, True, "leaky_relu", 0.2), ("esrgan hr conv", 64, 64, 2048, False, "leaky_relu", 0.2),
              ("taesd 64->64", 64, 64, 512, False, "relu", 0.0)]
    for name, cin, cout, hw, up, act, p in shapes:
        if hw > args.max_hw:
            continue
        torch.manual_seed(0)
        x = torch.randn(1, cin, hw, hw, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        w = (torch.randn(cout, cin, 3, 3, device=dev) / (3 * cin ** 0.5)).to(torch.bfloat16)
        b = torch.randn(cout, device=dev).to(torch.bfloat16)
        wn = w.permute(0, 2, 3, 1).contiguous()
        key = "|".join(str(v) for v in ("conv", 1, hw, hw, cin, cout, 3, 1, 1, 16 if up else 0, 0, "act", act, p))
        row = {"shape": f"{name}: {cin}->{cout} @ {hw}^2" + (" up2x" if up else ""), "act": act}
        os.environ.pop("CGS_TUNE_OVERRIDE", None)
        plain = lambda: ops.conv2d(x, w, b, 1, 1, weight_nhwc=wn, upsample2x=up)      # noqa: E731
        plain()                                                                        # (tunes the plain conv)
        row["plain"] = timed(plain, args.iters, args.reps)
        row["before"] = timed(lambda: ATEN[act](plain(), p), args.iters, args.reps)
        run = lambda: ops.conv2d(x, w, b, 1, 1, weight_nhwc=wn, upsample2x=up, act=act, act_param=p)   # noqa: E731
        for cand in ("split", "v3", "v4", "v8"):
            os.environ["CGS_TUNE_OVERRIDE"] = json.dumps({key: cand})
            row[cand] = timed(run, args.iters, args.reps)
        os.environ.pop("CGS_TUNE_OVERRIDE", None)
        run()
        row["choice"] = autotune.table().get(key, {}).get("choice")
        row["tuner_us"] = {k: round(v * 1000.0, 1) for k, v in autotune.table().get(key, {}).get("ms", {}).items()}
        row["tuned"] = timed(run, args.iters, args.reps)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def gemm_rows(args, dev):
    from .. import ops
    from ..ops import core
    rows = []
    for name, k, n, act in (("clip-l fc1", 768, 3072, "quick_gelu"), ("clip-g fc1", 1280, 5120, "gelu"),
                            ("clip-h fc1", 1024, 4096, "gelu")):
        for m in (77, 616):
            torch.manual_seed(0)
            a = torch.randn(m, k, device=dev).to(torch.bfloat16)
            w = (torch.randn(n, k, device=dev) / k ** 0.5).to(torch.bfloat16)
            b = torch.randn(n, device=dev).to(torch.bfloat16)
            row = {"shape": f"{name}: M={m} K={k} N={n}", "act": act}
            plain = lambda: ops.linear(a, w, b)                     # noqa: E731
            plain()
            row["plain"] = timed(plain, args.iters, args.reps)
            row["before"] = timed(lambda: ATEN[act](plain(), 0.0), args.iters, args.reps)
            row["split"] = timed(lambda: ops.activation(plain(), act, inplace=True), args.iters, args.reps)
            epi = core.EPI_BIAS | core.EPI_GELU | (0 if act == "gelu" else core.ACT_CODES[act] << 8)
            out = torch.empty(m, n, device=dev, dtype=torch.bfloat16)
            for cand, v in (("hip", -1), ("v6", 6), ("v4", 4), ("v8", 8)):
                if m <= 128 and v != -1:
                    continue
                fn = lambda v=v: core._gemm_launch(a, w, out, b, None, m, n, k, epi, v)           # noqa: E731
                row[cand] = timed(fn, args.iters, args.reps)
            run = lambda: ops.linear(a, w, b, act=act)              # noqa: E731
            run()
            row["tuned"] = timed(run, args.iters, args.reps)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def e2e(args, dev):
    from ..models import clip as clip_mod
    from ..models import upscalers
    from ..models.layers import init_random_fast_
    res = {}
    with torch.inference_mode():
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
        x = torch.rand(1, 3, 512, 512, device=dev).to(torch.bfloat16)
        m(x)                                                        # warm-up incl. kernel choice
        res["esrgan_4x_512_ms"] = timed(lambda: m(x), 2, args.reps, warm=1) / 1000.0
        tokens = torch.randint(1, 49000, (8, 77), device=dev)
        tokens[:, -1] = 49407
        towers = []
        for cfg in (clip_mod.CLIP_L_CONFIG, clip_mod.CLIP_G_CONFIG):
            t = clip_mod.CLIPTextModel(cfg, dtype=torch.bfloat16, device=dev)
            init_random_fast_(t, seed=1)
            towers.append(t)
        enc = lambda: [t(tokens, intermediate_output=-2) for t in towers]       # noqa: E731
        enc()
        res["clip_l_g_8_prompts_ms"] = timed(enc, 5, args.reps, warm=2) / 1000.0
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-hw", type=int, default=2048)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--conv-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("act_bench needs the GPU: timings elsewhere say nothing about it")
    dev = torch.device("cuda", 0)
    with torch.inference_mode():
        res = {"e2e": e2e(args, dev)} if args.e2e else {"conv": conv_rows(args, dev), "gemm": [] if args.conv_only else gemm_rows(args, dev)}
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
