"""The fused shifted-window attention kernel (csrc/kernels/window_attn.hip, ops.window_attention) on the device:
per-element bounds against an fp64 reference written here in plain torch, output integrity, entry refusals, the
Swin-family models with the switch on and off, and hipGraph capture of one RSTB."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bounds import assert_within                                          # noqa: E402
from _bounds_window import window_attention_bound                          # noqa: E402

from comfy_gen_server_amd import _native, ops                              # noqa: E402
from comfy_gen_server_amd.models import swin_sr                            # noqa: E402
from comfy_gen_server_amd.models.layers import init_random_                # noqa: E402
from comfy_gen_server_amd.tools.window_attn_bench import swin_model        # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
INVALID = 1          # hipErrorInvalidValue


def _windows(t, H, W, ws, shift):
    """[B, H*W, X] -> rolled, partitioned [B * nW, ws*ws, X]."""
    B, X = t.shape[0], t.shape[-1]
    y = torch.roll(t.reshape(B, H, W, X), (-shift, -shift), (1, 2))
    return y.reshape(B, H // ws, ws, W // ws, ws, X).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, X)


def _unwindows(w, B, H, W, ws, shift):
    X = w.shape[-1]
    y = w.reshape(B, H // ws, W // ws, ws, ws, X).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, X)
    return torch.roll(y, (shift, shift), (1, 2)).reshape(B, H * W, X)


def _score_terms(table, B, H, W, ws, shift):
    """fp32 [B * nW, heads, N, N]: the gathered position bias plus the 0 / -100 shift mask."""
    ys, xs = torch.arange(ws * ws) // ws, torch.arange(ws * ws) % ws
    r = (ys[:, None] - ys[None, :] + ws - 1) * (2 * ws - 1) + (xs[:, None] - xs[None, :] + ws - 1)
    bias = table.float()[r].permute(2, 0, 1)                               # [heads, N(q), N(k)]
    lab = torch.zeros(H, W)                                                # region labels of the rolled image
    if shift:
        for i, hs in enumerate((slice(0, -ws), slice(-ws, -shift), slice(-shift, None))):
            for j, wsl in enumerate((slice(0, -ws), slice(-ws, -shift), slice(-shift, None))):
                lab[hs, wsl] = 3 * i + j
    win = _windows(lab.reshape(1, H * W, 1), H, W, ws, 0)[..., 0]          # [nW, N]
    mask = torch.where(win[:, :, None] != win[:, None, :], -100.0, 0.0)
    return (bias[None] + mask[:, None]).repeat(B, 1, 1, 1)


CASES = [(2, 16, 24, 8, 4, 6, 30, "plain"), (1, 16, 24, 8, 0, 6, 30, "plain"), (1, 8, 16, 8, 3, 6, 10, "plain"),
         (1, 32, 48, 16, 8, 6, 30, "plain"), (1, 16, 16, 16, 5, 2, 64, "plain"), (2, 16, 16, 8, 4, 3, 60, "cosine"),
         (1, 16, 32, 8, 4, 4, 32, "plain")]


@pytest.mark.parametrize("B,H,W,ws,shift,heads,D,mode", CASES)
def test_window_attention_bound(cuda, B, H, W, ws, shift, heads, D, mode):
    g = torch.Generator().manual_seed(H * W + D)
    C = heads * D
    qkv = torch.randn(B, H * W, 3 * C, generator=g).to(BF)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    cosine = mode == "cosine"
    hs = torch.tensor([10.0, 25.0, 100.0]) if cosine else None
    q, k, v = (_windows(t, H, W, ws, shift) for t in qkv.float().split(C, -1))
    ref, tol = window_attention_bound(q, k, v, heads, _score_terms(table, B, H, W, ws, shift), cosine, hs)
    ref, tol = _unwindows(ref, B, H, W, ws, shift), _unwindows(tol, B, H, W, ws, shift)
    ops.reset_stats()
    y = ops.window_attention(qkv.to(cuda), (H, W), ws, shift, heads, table.to(cuda),
                             scale=1.0 if cosine else None, cosine=cosine, head_scale=None if hs is None else hs.to(cuda))
    st = ops.stats()
    assert st.get(("window_attention", "hip"), 0) == 1 and not [k_ for k_ in st if k_[1] == "lib"], st
    assert_within(y.cpu(), ref, tol, f"window_attention {(B, H, W, ws, shift, heads, D, mode)}")


def _call(qkv, o, table, B, H, W, heads, D, ws, shift, off=0):
    lib = _native.load_kernels()
    err = lib.cgs_window_attn_fwd(qkv.data_ptr() + off, o.data_ptr(), None if table is None else table.data_ptr(),
                                  D ** -0.5, 0, None, B, H, W, heads, D, ws, shift, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return err


def test_window_attention_writes_all_and_only_o(cuda):
    """Every element of o is written, and no bit outside o changes when o lies inside a larger buffer."""
    B, H, W, ws, shift, heads, D = 2, 16, 24, 8, 4, 6, 30
    C, n = heads * D, 2 * 16 * 24 * 6 * 30
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B, H * W, 3 * C, generator=g).to(cuda, BF)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g).to(cuda)
    buf = torch.full((n + 512,), float("nan"), device=cuda, dtype=BF)
    before = buf.view(torch.int16).clone()
    o = buf[256:256 + n]
    assert _call(qkv, o, table, B, H, W, heads, D, ws, shift) == 0
    assert bool(torch.isfinite(o).all())
    after = buf.view(torch.int16)
    assert torch.equal(after[:256], before[:256]) and torch.equal(after[256 + n:], before[256 + n:])
    assert torch.equal(o.view(B, H * W, C), ops.window_attention(qkv, (H, W), ws, shift, heads, table))


def test_window_attention_refusals(cuda):
    """Each single broken rule returns hipErrorInvalidValue and leaves o's bits alone; the unbroken call returns 0."""
    good = dict(B=1, H=16, W=16, heads=2, D=16, ws=8, shift=4, off=0, table=True)
    broken = {"ws": dict(ws=7, H=14, W=14, shift=3), "H": dict(H=12), "shift": dict(shift=8), "odd D": dict(D=15),
              "D cap": dict(D=66), "table": dict(table=False), "align": dict(off=2)}
    qkv = torch.randn(1 * 16 * 16 * 3 * 2 * 66 + 8, device=cuda).to(BF)      # large enough for every variant
    table = torch.randn(15 * 15, 2, device=cuda)
    for name, change in [("good", {})] + list(broken.items()):
        a = {**good, **change}
        o = torch.full((a["B"] * a["H"] * a["W"] * a["heads"] * a["D"],), float("nan"), device=cuda, dtype=BF)
        before = o.view(torch.int16).clone()
        err = _call(qkv, o, table if a["table"] else None, a["B"], a["H"], a["W"], a["heads"], a["D"], a["ws"],
                    a["shift"], a["off"])
        if name == "good":
            assert err == 0 and bool(torch.isfinite(o).all())
        else:
            assert err == INVALID, (name, err)
            assert torch.equal(o.view(torch.int16), before), name


def _swin_model(kind):
    """SwinIR / Swin2SR / HAT at the shapes of test_upscale.py's _random_swin, randomly initialised."""
    return swin_model(kind, dim=48, ws=8, heads=3, layers=2, depth=2, nf=32)


@pytest.mark.parametrize("kind", ["swinir", "swin2sr", "hat"])
def test_swin_models_switch(cuda, monkeypatch, kind):
    """Switch on: one fused launch per window-attention block (4); off: none. Both within 3e-2 of the fp32 CPU
    model, with the same vendor-library counts. CGS_STRICT_NATIVE: the fused forward raises nothing."""
    m = _swin_model(kind)
    x = torch.rand(1, 3, 40, 32, generator=torch.Generator().manual_seed(1))
    out, libs = {}, {}
    with torch.no_grad():
        ref = m(x)
        g = m.to(device=cuda, dtype=BF)
        for sw in ("1", "0"):
            monkeypatch.setenv("CGS_WINDOW_ATTN", sw)
            ops.reset_stats()
            out[sw] = g(x.to(cuda, BF)).float().cpu()
            st = ops.stats()
            assert st.get(("window_attention", "hip"), 0) == (4 if sw == "1" else 0), st
            libs[sw] = {k for k in st if k[1] == "lib"}
            assert ((out[sw] - ref).norm() / ref.norm()).item() < 3e-2
        assert libs["1"] == libs["0"], libs
        if not libs["1"]:
            monkeypatch.setenv("CGS_WINDOW_ATTN", "1")
            monkeypatch.setenv("CGS_STRICT_NATIVE", "1")
            g(x.to(cuda, BF))


def test_rstb_graph_capture(cuda, monkeypatch):
    """One SwinIR RSTB captured once and replayed on new input contents equals the eager result bit for bit."""
    monkeypatch.setenv("CGS_WINDOW_ATTN", "1")
    hw = (16, 24)
    with torch.inference_mode():
        m = swin_sr.RSTB(48, 2, 3, 8, 2.0, 64, "1conv")
        init_random_(m, seed=8)
        m = m.eval().to(device=cuda, dtype=BF)
        g0 = torch.Generator().manual_seed(3)
        x1 = torch.randn(1, hw[0] * hw[1], 48, generator=g0).to(cuda, BF)
        x2 = torch.randn(1, hw[0] * hw[1], 48, generator=g0).to(cuda, BF)
        xs = x1.clone()
        m(xs, hw)                                   # autotune and cached weight layouts outside the capture
        ops.reset_stats()
        eager = m(x2, hw).clone()
        assert ops.stats().get(("window_attention", "hip"), 0) == 2
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                y = m(xs, hw)
        torch.cuda.current_stream().wait_stream(s)
        xs.copy_(x2)
        for _ in range(3):
            y.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, eager)
