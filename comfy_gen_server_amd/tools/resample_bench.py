"""Timing of the device Lanczos / bislerp resamplers against the paths they replace (profiles/r09/resample.md).

In one process on one device, for inputs that live on the device as node outputs do:
  lanczos  8 x 1024^2 -> 512^2 and 1 x 4096^2 -> 2048^2 (fp32 RGB, passed as the NHWC movedim view):
           parent = the PIL path (device -> host copy, PIL on one CPU thread, host -> device copy),
           device = ``cgs_lanczos_u8_h`` + ``cgs_lanczos_u8_v``
  bislerp  16 x 4 x 128^2 -> 192^2 (fp32): parent = the torch code on the device (ATen kernels),
           device = two ``cgs_bislerp`` launches
Both paths of a case are warmed, then timed alternately: a host clock around ``--iters`` calls that end in a
device synchronise, ``--reps`` windows each, medians reported. The outputs of the two paths are compared on
the timed inputs (Lanczos: equal; bislerp: largest difference).

  python -m comfy_gen_server_amd.tools.resample_bench [--out FILE.md]
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
    parent()
    for _ in range(3):
        device()
    p, d = [], []
    for _ in range(reps):
        p.append(window(parent, parent_iters))
        d.append(window(device, device_iters))
    return statistics.median(p), statistics.median(d), p, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=500, help="device-path calls per timed window")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resample_bench needs the GPU: timings elsewhere say nothing about it")
    from .. import ops
    dev = torch.device("cuda", 0)
    rows = []
    with torch.inference_mode():
        for n, s, o in ((8, 1024, 512), (1, 4096, 2048)):
            torch.manual_seed(0)
            x = (torch.rand(n, s, s, 3, device=dev) * 1.2 - 0.1).movedim(-1, 1)

            def parent():
                with ops.torch_reference():
                    return ops.lanczos_resize(x, o, o)

            def device():
                return ops.lanczos_resize(x, o, o)

            same = torch.equal(parent(), device())
            pm, dm, p, d = ab(parent, device, 1, args.iters, args.reps)
            rows.append({"case": f"lanczos {n} x {s}^2 -> {o}^2", "parent": "PIL, transfers included",
                         "parent_ms": pm, "device_ms": dm, "speedup": pm / dm, "outputs": "equal" if same else "DIFFER",
                         "parent_windows_ms": p, "device_windows_ms": d})
            print(json.dumps(rows[-1]), flush=True)
        torch.manual_seed(0)
        z = torch.randn(16, 4, 128, 128, device=dev)

        def parent_b():
            with ops.torch_reference():
                return ops.bislerp(z, 192, 192)

        def device_b():
            return ops.bislerp(z, 192, 192)

        diff = (parent_b() - device_b()).abs().max().item()
        pm, dm, p, d = ab(parent_b, device_b, 20, args.iters, args.reps)
        rows.append({"case": "bislerp 16 x 4 x 128^2 -> 192^2", "parent": "torch code on the device",
                     "parent_ms": pm, "device_ms": dm, "speedup": pm / dm, "outputs": f"max |diff| {diff:.2e}",
                     "parent_windows_ms": p, "device_windows_ms": d})
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write("| case | parent path | parent ms | device ms | speed-up | outputs |\n|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['case']} | {r['parent']} | {r['parent_ms']:.3f} | {r['device_ms']:.4f} | "
                        f"{r['speedup']:.0f}x | {r['outputs']} |\n")
            f.write("\nWindows (ms per call):\n\n")
            for r in rows:
                f.write(f"- {r['case']}: parent {[round(v, 3) for v in r['parent_windows_ms']]}, "
                        f"device {[round(v, 4) for v in r['device_windows_ms']]}\n")


if __name__ == "__main__":
    main()
