"""The patch form of the 3 x 3 conv (variant 22, in-tree build) against the v6 conv the packaged tune table names, on
the fifteen 3 x 3 / stride 1 convs of the SDXL UNet at batch 16, and on the GroupNorm-partials form of those without
a residual. CGS_LIB=<other libcgs_kernels.so> runs the v6 arm on that build (the parent commit's,
tools/build_rev_lib.sh); the in-tree v6 is timed beside it (the existing instantiations must not get slower), and
the one-tap probe (tools/probes/conv_patch_ceiling.py) gives the ceiling in the same process. One warm-up round, then
alternating rounds of 5 launches, medians in ms; spread = max - min of the parent's rounds. A shape passes when its
gain exceeds twice that spread.

python tools/probes/conv_patch_ab.py [rounds] [out.md]"""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from comfy_gen_server_amd import _native  # noqa: E402
from comfy_gen_server_amd.ops import core  # noqa: E402
from conv_patch_ceiling import SHAPES, name, operands, timed  # noqa: E402


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = sys.argv[2] if len(sys.argv) > 2 else "profiles/r12/conv_patch_ab.md"
    dev = torch.device("cuda", 0)
    new = _native.load_kernels()
    old = new
    if os.environ.get("CGS_LIB"):
        old = ctypes.CDLL(os.path.abspath(os.environ["CGS_LIB"]), mode=ctypes.RTLD_LOCAL)
        _native._declare(old)
    st = core._stream()
    print(f"v6 arm: {os.environ.get('CGS_LIB', 'in-tree')}; rounds {rounds}", flush=True)
    rows = []
    for N, H, Cin, Cout, res in SHAPES:
        for gns in ((False, True) if not res else (False,)):
            x, wn, b, r = operands(dev, N, H, Cin, Cout, res)
            yo = torch.empty(N, H, H, Cout, device=dev, dtype=torch.bfloat16)
            yn = torch.empty_like(yo)
            part = torch.empty(N * (H * H // 64) * Cout * 2, device=dev, dtype=torch.float32)
            pre = (x.data_ptr(), None, Cin, wn.data_ptr(), b.data_ptr(), core._ptr(r))
            dims = (N, H, H, Cin, Cout, 3, 3, 1, 1, H, H, 0)

            def v6(lib, y):
                if gns:
                    assert lib.cgs_conv2d_nhwc_gns(*pre, y.data_ptr(), *dims, part.data_ptr(), st) == 0
                else:
                    assert lib.cgs_conv2d_nhwc_v(*pre, y.data_ptr(), *dims, 6, st) == 0

            def v6p():
                if gns:
                    assert new.cgs_conv2d_nhwc_gns_v(*pre, yn.data_ptr(), *dims, part.data_ptr(), 22, st) == 0
                else:
                    assert new.cgs_conv2d_nhwc_v(*pre, yn.data_ptr(), *dims, 22, st) == 0

            def probe():
                assert new.cgs_conv2d_nhwc_probe(x.data_ptr(), wn.data_ptr(), b.data_ptr(), core._ptr(r), yn.data_ptr(),
                                                 N, H, H, Cin, Cout, 3, 3, 1, 1, H, H, st) == 0
            arms = [("parent", lambda: v6(old, yo)), ("v6", lambda: v6(new, yn)), ("v6p", v6p)]
            if not gns:
                arms.append(("probe", probe))
            ts = {k: [] for k, _ in arms}
            for rnd in range(rounds + 1):
                for k, f in arms:
                    t = timed(f)
                    if rnd:
                        ts[k].append(t)
            v6(old, yo)
            v6p()
            torch.cuda.synchronize()
            diff = (yn.float() - yo.float()).abs()
            rel = (diff.norm() / yo.float().norm()).item()
            med = {k: statistics.median(v) for k, v in ts.items()}
            spread = max(ts["parent"]) - min(ts["parent"])
            nm = name(N, H, Cin, Cout, res) + (" (GNS)" if gns else "")
            rows.append((nm, med, spread, rel, diff.max().item()))
            print(f"{nm}: " + "  ".join(f"{k} {[round(t, 3) for t in v]}" for k, v in ts.items())
                  + f"  rel diff {rel:.2e} max {diff.max().item():.4f}", flush=True)
            assert rel < 1e-2
            del x, wn, b, r, yo, yn, part, diff
            torch.cuda.empty_cache()
    lines = ["| conv | parent v6 ms | spread | in-tree v6 ms | v6p ms | gain ms | gain % | ceiling ms | ships on |",
             "|---|---:|---:|---:|---:|---:|---:|---:|---|"]
    for nm, med, sp, rel, mx in rows:
        gain = med["parent"] - med["v6p"]
        ceil = f"{med['parent'] - med['probe']:.3f}" if "probe" in med else ""
        lines.append(f"| {nm} | {med['parent']:.3f} | {sp:.3f} | {med['v6']:.3f} | {med['v6p']:.3f} | {gain:.3f} | "
                     f"{100 * gain / med['parent']:.1f} | {ceil} | {'v6p' if gain > 2 * sp else 'v6'} |")
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
