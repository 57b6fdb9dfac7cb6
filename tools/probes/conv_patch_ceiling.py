"""What the v6 3 x 3 conv could gain at most from staging its input patch once: the unmodified kernel against the
same kernel with the A DMAs of tap 0 only (cgs_conv2d_nhwc_probe: B DMAs and MFMAs unchanged, results wrong by
design), on the fifteen 3 x 3 / stride 1 convs of the SDXL UNet at batch 16. One process, one warm-up round, then
alternating rounds of 5 launches, medians in ms; spread = max - min of the unmodified kernel's rounds.

python tools/probes/conv_patch_ceiling.py [rounds] [out.md]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.getcwd())
from comfy_gen_server_amd import _native  # noqa: E402
from comfy_gen_server_amd.ops import core  # noqa: E402

#         N, H, Cin, Cout, residual
SHAPES = [(16, 128, 320, 320, False), (16, 128, 320, 320, True), (16, 128, 640, 320, False), (16, 128, 960, 320, False),
          (16, 64, 320, 640, False), (16, 64, 640, 640, False), (16, 64, 640, 640, True), (16, 64, 960, 640, False),
          (16, 64, 1280, 640, False), (16, 64, 1920, 640, False),
          (16, 32, 640, 1280, False), (16, 32, 1280, 1280, False), (16, 32, 1280, 1280, True),
          (16, 32, 1920, 1280, False), (16, 32, 2560, 1280, False)]


def timed(f, n=5):
    f()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def operands(dev, N, H, Cin, Cout, res):
    x = (torch.rand(N, H, H, Cin, device=dev) * 2 - 1).to(torch.bfloat16)
    wn = ((torch.rand(Cout, 3, 3, Cin, device=dev) * 2 - 1) / (9 * Cin) ** 0.5).to(torch.bfloat16)
    b = torch.randn(Cout, device=dev).to(torch.bfloat16)
    r = torch.randn(N, H, H, Cout, device=dev).to(torch.bfloat16) if res else None
    return x, wn, b, r


def name(N, H, Cin, Cout, res):
    return f"{N} x {H}^2, {Cin} -> {Cout}" + (" + res" if res else "")


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = sys.argv[2] if len(sys.argv) > 2 else "profiles/r12/conv_patch_ceiling.md"
    dev = torch.device("cuda", 0)
    lib = _native.load_kernels()
    st = core._stream()
    rows = []
    for N, H, Cin, Cout, res in SHAPES:
        x, wn, b, r = operands(dev, N, H, Cin, Cout, res)
        y = torch.empty(N, H, H, Cout, device=dev, dtype=torch.bfloat16)

        def v6():
            assert lib.cgs_conv2d_nhwc_v(x.data_ptr(), None, Cin, wn.data_ptr(), b.data_ptr(), core._ptr(r),
                                         y.data_ptr(), N, H, H, Cin, Cout, 3, 3, 1, 1, H, H, 0, 6, st) == 0

        def probe():
            assert lib.cgs_conv2d_nhwc_probe(x.data_ptr(), wn.data_ptr(), b.data_ptr(), core._ptr(r), y.data_ptr(),
                                             N, H, H, Cin, Cout, 3, 3, 1, 1, H, H, st) == 0
        ts = {"v6": [], "probe": []}
        for rnd in range(rounds + 1):
            for k, f in (("v6", v6), ("probe", probe)):
                t = timed(f)
                if rnd:
                    ts[k].append(t)
        m6, mp = statistics.median(ts["v6"]), statistics.median(ts["probe"])
        spread = max(ts["v6"]) - min(ts["v6"])
        tf = 2.0 * N * H * H * Cin * Cout * 9 / m6 / 1e9
        rows.append((name(N, H, Cin, Cout, res), m6, spread, tf, mp, m6 - mp))
        print(f"{rows[-1][0]}: v6 {[round(t, 3) for t in ts['v6']]} probe {[round(t, 3) for t in ts['probe']]}",
              flush=True)
        del x, wn, b, r, y
        torch.cuda.empty_cache()
    lines = ["| conv | v6 ms | spread | TF/s | one-tap A DMAs ms | ceiling ms | ceiling % | > 2 x spread |",
             "|---|---:|---:|---:|---:|---:|---:|---|"]
    for n, m6, sp, tf, mp, c in rows:
        lines.append(f"| {n} | {m6:.3f} | {sp:.3f} | {tf:.0f} | {mp:.3f} | {c:.3f} | {100 * c / m6:.1f} | "
                     f"{'yes' if c > 2 * sp else 'no'} |")
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
