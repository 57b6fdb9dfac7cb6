"""Upsample + conv: the tap form (csrc/kernels/upconv.hip, in-tree build) against CONV_UP2X on the variant the
packaged tune table names, on the production shapes (SDXL UNet batch 16 / 2, VAE decode batch 8 / 1). One process,
interleaved rounds, median of the rounds; CGS_LIB=<other libcgs_kernels.so> runs the CONV_UP2X arm on that build
(the parent commit's, tools/build_rev_lib.sh). The tap form is timed at each tile group of GROUPS
(cgs_upconv_set_tile_group), the first being the default. Round 0 of every arm is a warm-up and is not counted. A shape passes when its gain exceeds twice the
spread of the CONV_UP2X rounds.

python tools/probes/upconv_taps_ab.py [rounds]"""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.getcwd())
from comfy_gen_server_amd import _native  # noqa: E402
from comfy_gen_server_amd.ops import core  # noqa: E402

dev = torch.device("cuda", 0)
new = _native.load_kernels()
old = new
if os.environ.get("CGS_LIB"):
    old = ctypes.CDLL(os.path.abspath(os.environ["CGS_LIB"]), mode=ctypes.RTLD_LOCAL)
    _native._declare(old)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
GROUPS = (16, 8, 4)
#         N, H, Cin, Cout, CONV_UP2X variant (data/tune_mi355x.json)
SHAPES = [(16, 32, 1280, 1280, 5), (16, 64, 640, 640, 6), (8, 128, 512, 512, 5), (8, 256, 512, 512, 5),
          (8, 512, 256, 256, 5), (2, 32, 1280, 1280, 6), (2, 64, 640, 640, 6), (1, 128, 512, 512, 5),
          (1, 256, 512, 512, 5), (1, 512, 256, 256, 5)]


def _t(f, n=5):
    f()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


print(f"CONV_UP2X arm: {os.environ.get('CGS_LIB', 'in-tree')}; rounds {ROUNDS}", flush=True)
for N, H, Cin, Cout, variant in SHAPES:
    x = (torch.rand(N, H, H, Cin, device=dev) * 2 - 1).to(torch.bfloat16)
    w = ((torch.rand(Cout, Cin, 3, 3, device=dev) * 2 - 1) / (9 * Cin) ** 0.5).to(torch.bfloat16)
    b = torch.randn(Cout, device=dev).to(torch.bfloat16)
    wn = w.permute(0, 2, 3, 1).contiguous()
    wt = core.upconv_tap_weights(w)
    yo = torch.empty(N, 2 * H, 2 * H, Cout, device=dev, dtype=torch.bfloat16)
    yn = torch.empty_like(yo)
    st = core._stream()

    def run_old():
        assert old.cgs_conv2d_nhwc_v(x.data_ptr(), None, Cin, wn.data_ptr(), b.data_ptr(), None, yo.data_ptr(), N, H, H,
                                     Cin, Cout, 3, 3, 1, 1, 2 * H, 2 * H, 16, variant, st) == 0

    def run_new(g):
        new.cgs_upconv_set_tile_group(g)
        assert new.cgs_upconv_taps_nhwc(x.data_ptr(), wt.data_ptr(), b.data_ptr(), yn.data_ptr(), N, H, H, Cin, Cout,
                                        st) == 0

    ts = {"conv_up2x": []}
    ts.update({g: [] for g in GROUPS})
    for rnd in range(ROUNDS + 1):
        t = _t(run_old)
        if rnd:
            ts["conv_up2x"].append(t)
        for g in GROUPS:
            t = _t(lambda: run_new(g))
            if rnd:
                ts[g].append(t)
    run_new(GROUPS[0])
    torch.cuda.synchronize()
    diff = (yn.float() - yo.float()).abs()
    rel = (diff.norm() / yo.float().norm()).item()
    base = ts["conv_up2x"]
    mo, spread = statistics.median(base), max(base) - min(base)
    print(f"N={N} {H}x{H} {Cin}->{Cout} (v{variant}): conv_up2x rounds {[round(t, 3) for t in base]} ms, median "
          f"{mo:.3f}, spread {spread:.3f}; max |taps - conv_up2x| {diff.max().item():.4f}, rel {rel:.2e}", flush=True)
    for g in GROUPS:
        t = ts[g]
        mn = statistics.median(t)
        print(f"    taps group {g:2d}: rounds {[round(v, 3) for v in t]} ms, median {mn:.3f}  x{mo / mn:.2f}  gain "
              f"{mo - mn:.3f} ms  {'PASS' if mo - mn > 2 * spread else 'no'}", flush=True)
    assert rel < 1e-2
    del x, w, wn, wt, yo, yn, diff
    torch.cuda.empty_cache()
