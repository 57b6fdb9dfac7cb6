"""The fused rectangular-window attention kernel (csrc/kernels/rect_attn.hip, ops.rect_window_attention) on the
device: per-element bounds against the fp64 reference of _ref_rect.py, output integrity, entry refusals, and DAT with
the switch on and off."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bounds import assert_within                                          # noqa: E402
from _ref_rect import rect_attention_reference                             # noqa: E402

from comfy_gen_server_amd import _native, ops                              # noqa: E402
from comfy_gen_server_amd.tools.rect_attn_bench import dat_model           # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
INVALID = 1          # hipErrorInvalidValue
# the last case: heads / 2 = 4 is staged as two chunks of two heads
CASES = [(1, 5, 7, (8, 16), 2, 2, True), (1, 8, 16, (8, 16), 2, 10, False), (1, 16, 16, (8, 16), 2, 30, True),
         (2, 24, 40, (16, 8), 6, 30, True), (1, 32, 32, (8, 32), 2, 16, False), (1, 32, 64, (32, 8), 4, 32, True),
         (1, 40, 72, (8, 32), 6, 30, True), (1, 8, 20, (16, 8), 8, 6, True)]


@pytest.mark.parametrize("B,H,W,split,heads,D,shifted", CASES)
def test_rect_attention_bound(cuda, B, H, W, split, heads, D, shifted):
    g = torch.Generator().manual_seed(H * W + D)
    qkv = torch.randn(B, H * W, 3 * heads * D, generator=g).to(BF)
    tables = [torch.randn((2 * split[0] - 1) * (2 * split[1] - 1), heads // 2, generator=g) for _ in range(2)]
    ref, tol = rect_attention_reference(qkv, H, W, split, shifted, heads, tables)
    ops.reset_stats()
    y = ops.rect_window_attention(qkv.to(cuda), (H, W), split, shifted, heads, [t.to(cuda) for t in tables])
    st = ops.stats()
    assert st.get(("rect_window_attention", "hip"), 0) == 1 and not [k for k in st if k[1] == "lib"], st
    assert_within(y.cpu(), ref, tol, f"rect_window_attention {(B, H, W, split, heads, D, shifted)}")


def test_rect_attention_refusals_and_integrity(cuda):
    """A good call writes every element of o and no bit around it; each single broken rule returns
    hipErrorInvalidValue and leaves o's bits alone."""
    lib = _native.load_kernels()
    good = dict(H=20, W=24, heads=6, D=16, s0=8, s1=16, off=0, table=True)
    broken = {"split": dict(s1=12), "odd heads": dict(heads=5), "odd D": dict(D=15), "D cap": dict(D=34),
              "table": dict(table=False), "align": dict(off=2)}
    qkv = torch.randn(20 * 24 * 3 * 6 * 34 + 8, device=cuda).to(BF)          # large enough for every variant
    tables = [torch.randn(15 * 31, 3, device=cuda) for _ in range(2)]
    for name, change in [("good", {})] + list(broken.items()):
        a = {**good, **change}
        n = a["H"] * a["W"] * a["heads"] * a["D"]
        buf = torch.full((n + 512,), float("nan"), device=cuda, dtype=BF)
        before = buf.view(torch.int16).clone()
        err = lib.cgs_rect_attn_fwd(qkv.data_ptr() + a["off"], buf.data_ptr() + 512, tables[0].data_ptr(),
                                    tables[1].data_ptr() if a["table"] else None, a["D"] ** -0.5, 1, a["H"], a["W"],
                                    a["heads"], a["D"], a["s0"], a["s1"], 1, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        after = buf.view(torch.int16)
        if name == "good":
            assert err == 0 and bool(torch.isfinite(buf[256:256 + n]).all())
            assert torch.equal(after[:256], before[:256]) and torch.equal(after[256 + n:], before[256 + n:])
        else:
            assert err == INVALID, (name, err)
            assert torch.equal(after, before), name


def test_dat_switch(cuda, monkeypatch):
    """Switch on: one fused launch per spatial block (2: one un-shifted, one shifted); off: none. Both within 3e-2 of
    the fp32 CPU model, with the same vendor-library counts."""
    m = dat_model(dim=96, heads=6, groups=2, depth=2, split=(8, 16))
    assert [blk.attn.shifted for layer in m.layers for blk in layer.blocks[::2]] == [False, True]
    x = torch.rand(1, 3, 20, 24, generator=torch.Generator().manual_seed(1))
    libs = {}
    with torch.no_grad():
        ref = m(x)
        g = m.to(device=cuda, dtype=BF)
        for sw in ("1", "0"):
            monkeypatch.setenv("CGS_RECT_ATTN", sw)
            ops.reset_stats()
            out = g(x.to(cuda, BF)).float().cpu()
            st = ops.stats()
            assert st.get(("rect_window_attention", "hip"), 0) == (2 if sw == "1" else 0), st
            libs[sw] = {k: v for k, v in st.items() if k[1] == "lib"}
            assert ((out - ref).norm() / ref.norm()).item() < 3e-2
    assert libs["1"] == libs["0"], libs
