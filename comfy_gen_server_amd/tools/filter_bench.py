"""Timing of the device image filters against the torch paths they replace (profiles/r11/filters.md).

In one process on one device, for inputs that live on the device as node outputs do; the parent of every case is
the op's torch path on the device (dense ``F.pad`` + depthwise ``F.conv2d`` through MIOpen, ``F.max_pool2d``, the
ATen Canny with its host-synchronised hysteresis loop), the other side is the HIP path:
  blur    8 x 1024^2 x 3 fp32 IMAGE at r = 1, 5, 31 (unit taps, sigma 1), ``cgs_filter_sep`` in the form
          ``ops.filter_sep`` picks; at r = 8, 16, 31 also its one-launch form against its two-launch form (horizontal
          taps into an fp32 temporary, then vertical taps)
  sag     16 x 4 x 128^2 bf16, k = 9 pixel taps
  dilate  8 x 1024^2 x 3 fp32 IMAGE at k = 3, 31, 255, ``cgs_morph_box``
  canny   1 x and 8 x 3 x 1024^2: a synthetic image with long contours and no checkpoint behind it -- rings around
          three random centres per channel, f = mean of sin(0.06 r), value 0.5 + 0.5 tanh(4 f) (soft steps along the
          zero crossings of f), plus 1 % uniform noise -- low 0.1, high 0.3
  copy    ``y.copy_(x)`` of the blur input: the bytes-per-second yardstick (read + write of the same bytes)
Both paths of a case are warmed, then timed alternately: a host clock around a window of calls that ends in a
device synchronise, ``--reps`` windows each, medians reported with the spread (max - min) of the windows.

  python -m comfy_gen_server_amd.tools.filter_bench [--out FILE.md]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000.0 / iters


def ab(parent, device, parent_iters, device_iters, reps):
    """Medians (ms per call) of ``reps`` alternating windows of the two paths, each warmed first."""
    for _ in range(2):
        parent()
    for _ in range(3):
        device()
    p, d = [], []
    for _ in range(reps):
        p.append(window(parent, parent_iters))
        d.append(window(device, device_iters))
    return statistics.median(p), statistics.median(d), p, d


def contours(n, size, device):
    """[n, 3, size, size] in [0, 1]: soft-stepped rings around three centres per channel (long contours) + 1 % noise."""
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(size, dtype=torch.float32), torch.arange(size, dtype=torch.float32),
                            indexing="ij")
    out = []
    for _ in range(n):
        img = torch.zeros(3, size, size)
        for c in range(3):
            f = torch.zeros(size, size)
            for _k in range(3):
                cy, cx = (torch.rand(2, generator=g) * size).tolist()
                f += torch.sin(0.06 * torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2))
            img[c] = 0.5 + 0.5 * torch.tanh(4 * f / 3)
        out.append(img)
    x = torch.stack(out) + 0.01 * torch.rand((n, 3, size, size), generator=g)
    return x.clamp(0, 1).to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50, help="device-path calls per timed window")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("filter_bench needs the GPU: timings elsewhere say nothing about it")
    from .. import ops
    dev = torch.device("cuda", 0)
    rows = []

    def case(name, fn, parent_iters, nbytes=None, compare="max"):
        def parent():
            with ops.torch_reference():
                return fn()
        a, b = parent(), fn()
        if isinstance(a, tuple):
            a, b = a[-1], b[-1]
        diff = (a.float() - b.float()).abs()
        note = f"max |diff| {diff.max().item():.2e}" if compare == "max" else \
            f"{int(b.sum())} edge pixels of {diff.numel()}, {int((diff > 0).sum())} differ"
        pm, dm, p, d = ab(parent, fn, parent_iters, args.iters, args.reps)
        row = {"case": name, "parent_ms": pm, "device_ms": dm, "speedup": pm / dm, "outputs": note,
               "parent_windows_ms": p, "device_windows_ms": d}
        if nbytes:
            row["device_gbps"] = nbytes / dm / 1e6
        rows.append(row)
        print(json.dumps(row), flush=True)
        return row

    with torch.inference_mode():
        torch.manual_seed(0)
        img = torch.rand(8, 1024, 1024, 3, device=dev)
        rw_bytes = 2 * img.numel() * 4
        dst = torch.empty_like(img)
        for _ in range(3):
            dst.copy_(img)
        copy_ms = statistics.median(window(lambda: dst.copy_(img), args.iters) for _ in range(args.reps))
        copy_gbps = rw_bytes / copy_ms / 1e6
        print(json.dumps({"case": "copy 8 x 1024^2 x 3 fp32", "device_ms": copy_ms, "device_gbps": copy_gbps}), flush=True)
        for r in (1, 5, 31):
            taps = ops.gaussian_taps(2 * r + 1, 1.0, dev)
            case(f"blur 8 x 1024^2 x 3, r = {r}", lambda: ops.filter_sep(img, taps, layout="nhwc"),
                 5 if r < 31 else 1, rw_bytes)
        from ..ops import core
        xl = img.movedim(-1, 1)
        ab_rows = []
        for r in (8, 16, 31):
            taps = ops.gaussian_taps(2 * r + 1, 1.0, dev)

            def form(two):
                return core._filter_sep_hip(xl, taps, taps, "reflect", "nhwc", 0.0, 1.0, None, two_launch=two)
            same = torch.equal(form(False), form(True))
            for _ in range(3):
                form(False), form(True)
            f_w, t_w = [], []
            for _ in range(args.reps):
                f_w.append(window(lambda: form(False), args.iters))
                t_w.append(window(lambda: form(True), args.iters))
            ab_rows.append({"case": f"blur r = {r}: one launch against two (h into an fp32 temporary, then v)",
                            "r": r, "fused_ms": statistics.median(f_w), "two_launch_ms": statistics.median(t_w),
                            "fused_windows_ms": f_w, "two_launch_windows_ms": t_w, "same_bits": same})
            print(json.dumps(ab_rows[-1]), flush=True)

        z = torch.randn(16, 4, 128, 128, device=dev, dtype=torch.bfloat16)
        t9 = ops.gaussian_taps(9, 2.0, dev, span="pixel")
        case("sag 16 x 4 x 128^2 bf16, k = 9", lambda: ops.filter_sep(z, t9), 20, 2 * z.numel() * 2)
        for k in (3, 31, 255):
            case(f"dilate 8 x 1024^2 x 3, k = {k}", lambda: ops.morph_box(img, k, "dilate", layout="nhwc"),
                 5 if k < 255 else 1, rw_bytes)
        for n in (1, 8):
            cimg = contours(n, 1024, dev)
            case(f"canny {n} x 1024^2", lambda: ops.canny(cimg, 0.1, 0.3), 1, None, compare="edges")
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write("| case | parent ms (torch path on the device) | device ms | speed-up | device GB/s (read + write) "
                    "| outputs |\n|---|---|---|---|---|---|\n")
            for r in rows:
                gb = f"{r['device_gbps']:.0f}" if "device_gbps" in r else "-"
                f.write(f"| {r['case']} | {r['parent_ms']:.3f} | {r['device_ms']:.4f} | {r['speedup']:.1f}x | {gb} | "
                        f"{r['outputs']} |\n")
            f.write(f"\nDevice copy of the blur input (the same bytes read and written): {copy_ms:.4f} ms, "
                    f"{copy_gbps:.0f} GB/s.\n")
            f.write("\nOne launch against two (the same kernel: horizontal taps into an fp32 temporary, then vertical taps):\n\n"
                    "| r | one launch ms | two launches ms | same bits |\n|---|---|---|---|\n")
            for t in ab_rows:
                f.write(f"| {t['r']} | {t['fused_ms']:.4f} | {t['two_launch_ms']:.4f} | {t['same_bits']} |\n")
            f.write("\n")
            for t in ab_rows:
                f.write(f"- r = {t['r']} windows: one {[round(v, 4) for v in t['fused_windows_ms']]}, "
                        f"two {[round(v, 4) for v in t['two_launch_windows_ms']]}\n")
            f.write("\nWindows (ms per call), spread = max - min:\n\n")
            for r in rows:
                p, d = r["parent_windows_ms"], r["device_windows_ms"]
                f.write(f"- {r['case']}: parent {[round(v, 3) for v in p]} (spread {max(p) - min(p):.3f}), "
                        f"device {[round(v, 4) for v in d]} (spread {max(d) - min(d):.4f})\n")


if __name__ == "__main__":
    main()
