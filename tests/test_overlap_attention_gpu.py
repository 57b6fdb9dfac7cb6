"""The fused overlapping cross-attention kernel (csrc/kernels/overlap_attn.hip, ops.overlap_attention) on the device:
per-element bounds against an fp64 unfold reference written here in plain torch, output integrity, entry refusals, and
HAT with the switch on and off."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bounds import assert_within                                          # noqa: E402
from _bounds_overlap import overlap_attention_bound                        # noqa: E402

from comfy_gen_server_amd import _native, ops                              # noqa: E402
from comfy_gen_server_amd.models.swin_sr import _rel_index_oca             # noqa: E402
from comfy_gen_server_amd.tools.window_attn_bench import swin_model        # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
INVALID = 1          # hipErrorInvalidValue


def _windows(t, H, W, ws):
    B, X = t.shape[0], t.shape[-1]
    return t.reshape(B, H // ws, ws, W // ws, ws, X).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, X)


def _neighbourhoods(t, H, W, ws, ows):
    """[B, H*W, X] -> zero-padded ows x ows neighbourhood of every window, [B * nW, ows*ows, X]."""
    B, X = t.shape[0], t.shape[-1]
    u = F.unfold(t.reshape(B, H, W, X).permute(0, 3, 1, 2), ows, stride=ws, padding=(ows - ws) // 2)
    return u.view(B, X, ows * ows, -1).permute(0, 3, 2, 1).reshape(-1, ows * ows, X)


CASES = [(1, 8, 8, 8, 2, 10), (2, 16, 24, 8, 6, 30), (1, 24, 24, 8, 3, 16), (1, 16, 32, 16, 1, 32),
         (1, 16, 16, 16, 5, 24), (1, 48, 48, 16, 6, 30)]


@pytest.mark.parametrize("B,H,W,ws,heads,D", CASES)
def test_overlap_attention_bound(cuda, B, H, W, ws, heads, D):
    g = torch.Generator().manual_seed(H * W + D)
    C, ows = heads * D, ws * 3 // 2
    qkv = torch.randn(B, H * W, 3 * C, generator=g).to(BF)
    table = torch.randn((ws + ows - 1) ** 2, heads, generator=g)
    q, k, v = qkv.double().split(C, -1)
    add = table[_rel_index_oca(ws, ows)].permute(2, 0, 1)[None]            # negative indices wrap, as in the reference
    ref, tol = overlap_attention_bound(_windows(q, H, W, ws), _neighbourhoods(k, H, W, ws, ows),
                                       _neighbourhoods(v, H, W, ws, ows), heads, add)
    unw = lambda w: w.reshape(B, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H * W, C)  # noqa: E731
    ops.reset_stats()
    y = ops.overlap_attention(qkv.to(cuda), (H, W), ws, ows, heads, table.to(cuda))
    st = ops.stats()
    assert st.get(("overlap_attention", "hip"), 0) == 1 and not [k_ for k_ in st if k_[1] == "lib"], st
    assert_within(y.cpu(), unw(ref), unw(tol), f"overlap_attention {(B, H, W, ws, heads, D)}")


def _call(qkv, o, table, B, H, W, heads, D, ws, ows, off=0):
    lib = _native.load_kernels()
    err = lib.cgs_overlap_attn_fwd(qkv.data_ptr() + off, o.data_ptr(), None if table is None else table.data_ptr(),
                                   D ** -0.5, B, H, W, heads, D, ws, ows, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return err


def test_overlap_attention_refusals_and_integrity(cuda):
    """A good call writes every element of o and no bit around it; each single broken rule returns
    hipErrorInvalidValue and leaves o's bits alone."""
    good = dict(B=1, H=16, W=24, heads=3, D=16, ws=8, ows=12, off=0, table=True)
    broken = {"ows": dict(ows=16), "ws": dict(ws=12, ows=18, H=24), "H": dict(H=12), "odd D": dict(D=15),
              "D cap": dict(D=34), "table": dict(table=False), "align": dict(off=2)}
    qkv = torch.randn(24 * 24 * 3 * 3 * 34 + 8, device=cuda).to(BF)          # large enough for every variant
    table = torch.randn(29 * 29, 3, device=cuda)
    for name, change in [("good", {})] + list(broken.items()):
        a = {**good, **change}
        n = a["B"] * a["H"] * a["W"] * a["heads"] * a["D"]
        buf = torch.full((n + 512,), float("nan"), device=cuda, dtype=BF)
        before = buf.view(torch.int16).clone()
        err = _call(qkv, buf[256:256 + n], table if a["table"] else None, a["B"], a["H"], a["W"], a["heads"], a["D"],
                    a["ws"], a["ows"], a["off"])
        after = buf.view(torch.int16)
        if name == "good":
            assert err == 0 and bool(torch.isfinite(buf[256:256 + n]).all())
            assert torch.equal(after[:256], before[:256]) and torch.equal(after[256 + n:], before[256 + n:])
        else:
            assert err == INVALID, (name, err)
            assert torch.equal(after, before), name


def test_hat_switch(cuda, monkeypatch):
    """Switch on: one fused launch per OCAB (2); off: none. Both within 3e-2 of the fp32 CPU model, with the same
    vendor-library counts. CGS_STRICT_NATIVE: the fused forward raises nothing."""
    m = swin_model("hat", dim=48, ws=8, heads=3, layers=2, depth=2, nf=32)
    x = torch.rand(1, 3, 40, 32, generator=torch.Generator().manual_seed(1))
    libs = {}
    with torch.no_grad():
        ref = m(x)
        g = m.to(device=cuda, dtype=BF)
        for sw in ("1", "0"):
            monkeypatch.setenv("CGS_OVERLAP_ATTN", sw)
            ops.reset_stats()
            out = g(x.to(cuda, BF)).float().cpu()
            st = ops.stats()
            assert st.get(("overlap_attention", "hip"), 0) == (2 if sw == "1" else 0), st
            libs[sw] = {k for k in st if k[1] == "lib"}
            assert ((out - ref).norm() / ref.norm()).item() < 3e-2
        assert libs["1"] == libs["0"], libs
        if not libs["1"]:
            monkeypatch.setenv("CGS_OVERLAP_ATTN", "1")
            monkeypatch.setenv("CGS_STRICT_NATIVE", "1")
            g(x.to(cuda, BF))
