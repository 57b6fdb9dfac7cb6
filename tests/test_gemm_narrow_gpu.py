"""The narrow-K linear with fused LayerNorm and the row LayerNorm for C % 8 != 0 (csrc/kernels/gemm_narrow.hip;
ops.narrow_linear, ops.layer_norm) on the device: per-element bounds against fp64 references, output integrity, entry
refusals, and the dim-60 Swin-family models with CGS_NARROW_LINEAR on (strictly native) and off."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bounds import assert_within                                          # noqa: E402
from _bounds_narrow import layernorm_rows4_bound, narrow_linear_bound      # noqa: E402

from comfy_gen_server_amd import _native, ops                              # noqa: E402
from comfy_gen_server_amd.tools.window_attn_bench import swin_model        # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
INVALID = 1          # hipErrorInvalidValue

# (M, N, K, lda - K, ln: None | "gb" (gamma, beta) | "g" (gamma only), bias, act, residual)
CASES = [(1, 4, 4, 0, None, False, None, False), (129, 4, 4, 0, "g", False, None, True),
         (129, 68, 60, 0, "gb", True, None, False), (200, 4, 60, 4, "gb", True, "gelu", True),
         (200, 540, 180, 0, "gb", True, None, False), (129, 68, 180, 4, None, True, None, True),
         (200, 68, 180, 0, "g", True, "gelu", False), (1, 540, 180, 0, "gb", False, "silu", False),
         (129, 540, 252, 0, "g", True, "gelu", True), (1, 68, 252, 0, None, False, "silu", False),
         (129, 68, 360, 0, None, True, None, True), (200, 540, 360, 0, "gb", False, "silu", True)]


def _ln_params(C, g, kind):
    if kind is None:
        return None
    return (1 + 0.2 * torch.randn(C, generator=g)).to(BF), \
        (0.2 * torch.randn(C, generator=g)).to(BF) if kind == "gb" else None, 1e-5


@pytest.mark.parametrize("M,N,K,pad,ln,bias,act,res", CASES)
def test_narrow_linear_bound(cuda, monkeypatch, M, N, K, pad, ln, bias, act, res):
    monkeypatch.setenv("CGS_NARROW_LINEAR", "1")
    g = torch.Generator().manual_seed(1000 * K + N + M)
    xp = (torch.randn(M, K + pad, generator=g) + (3.0 if ln else 0.0)).to(BF)
    x = xp[:, :K]
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF)
    b = torch.randn(N, generator=g).to(BF) if bias else None
    r = torch.randn(M, N, generator=g).to(BF) if res else None
    lnp = _ln_params(K, g, ln)
    ref, tol = narrow_linear_bound(x, w, b, lnp, act, r)
    dev = lambda t: None if t is None else t.to(cuda)                                    # noqa: E731
    ops.reset_stats()
    y = ops.narrow_linear(xp.to(cuda)[:, :K], dev(w), dev(b), None if lnp is None else (dev(lnp[0]), dev(lnp[1]), lnp[2]), act,
                          dev(r))
    st = ops.stats()
    assert st.get(("gemm", "hip"), 0) == 1 and not [k for k in st if k[1] == "lib"], st
    assert_within(y.cpu(), ref, tol, f"narrow_linear {(M, N, K, pad, ln, bias, act, res)}")


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("rows", [1, 67])
@pytest.mark.parametrize("C", [4, 60, 180, 1020])
def test_layernorm_rows4_bound(cuda, monkeypatch, C, rows, res):
    monkeypatch.setenv("CGS_NARROW_LINEAR", "1")
    g = torch.Generator().manual_seed(C + rows)
    x = (torch.randn(rows, C, generator=g) + 3.0).to(BF)
    w, b, eps = _ln_params(C, g, "gb")
    r = torch.randn(rows, C, generator=g).to(BF) if res else None
    ref, tol = layernorm_rows4_bound(x, w, b, eps, r)
    ops.reset_stats()
    y = ops.layer_norm(x.to(cuda), w.to(cuda), b.to(cuda), eps, residual=None if r is None else r.to(cuda))
    assert ops.stats() == {("layernorm", "hip"): 1}, ops.stats()
    assert_within(y.cpu(), ref, tol, f"layernorm_rows4 {(C, rows, res)}")


def _call(x, w, y, M, N, K, lda, ldc, off=0):
    err = _native.load_kernels().cgs_gemm_narrow(x.data_ptr() + off, lda, None if w is None else w.data_ptr(), None, None,
                                                 None, 0.0, 0, None, 0, y.data_ptr(), ldc, M, N, K, 0,
                                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return err


def test_narrow_linear_writes_all_and_only_y(cuda):
    """y is a pitch-padded view inside a NaN-filled buffer: every element of y is written, and no bit outside it, pad
    columns included, changes."""
    M, N, K, ldc = 129, 68, 180, 72
    g = torch.Generator().manual_seed(7)
    x = torch.randn(M, K, generator=g).to(cuda, BF)
    w = torch.randn(N, K, generator=g).to(cuda, BF)
    buf = torch.full((M * ldc + 512,), float("nan"), device=cuda, dtype=BF)
    before = buf.view(torch.int16).clone()
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=cuda)
    inside[256:256 + M * ldc].view(M, ldc)[:, :N] = True
    assert _call(x, w, buf[256:], M, N, K, K, ldc) == 0
    assert bool(torch.isfinite(buf[inside]).all())
    assert torch.equal(buf.view(torch.int16)[~inside], before[~inside])
    assert torch.equal(buf[inside].view(M, N), ops.narrow_linear(x, w))


def test_narrow_linear_refusals(cuda):
    """Each single broken rule returns hipErrorInvalidValue and leaves y's bits alone; the unbroken call returns 0."""
    good = dict(M=8, N=8, K=8, lda=8, w=True, off=0)
    broken = {"K % 4": dict(K=6, lda=8), "K cap": dict(K=388, lda=388), "N % 4": dict(N=6), "lda % 4": dict(lda=10),
              "align": dict(off=2), "null W": dict(w=False)}
    x = torch.randn(8 * 388 + 8, device=cuda).to(BF)            # large enough for every variant
    w = torch.randn(8 * 388, device=cuda).to(BF)
    for name, change in [("good", {})] + list(broken.items()):
        a = {**good, **change}
        y = torch.full((a["M"] * 8,), float("nan"), device=cuda, dtype=BF)
        before = y.view(torch.int16).clone()
        err = _call(x, w if a["w"] else None, y, a["M"], a["N"], a["K"], a["lda"], 8, a["off"])
        if name == "good":
            assert err == 0 and bool(torch.isfinite(y).all())
        else:
            assert err == INVALID, (name, err)
            assert torch.equal(y.view(torch.int16), before), name


@pytest.mark.parametrize("kind", ["swinir", "swin2sr", "hat"])
def test_swin_dim60_native(cuda, monkeypatch, kind):
    """dim 60 (every K fails K % 8 == 0). Switch on: the forward runs under CGS_STRICT_NATIVE with no vendor-library
    call; off: exactly the GEMM and LayerNorm fallbacks of before. Both within 3e-2 of the fp32 CPU model."""
    m = swin_model(kind, dim=60, ws=8, heads=6, layers=2, depth=2, nf=32)
    x = torch.rand(1, 3, 40, 32, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        monkeypatch.setenv("CGS_NARROW_LINEAR", "0")
        ref = m(x)
        g = m.to(device=cuda, dtype=BF)
        for sw in ("1", "0"):
            monkeypatch.setenv("CGS_NARROW_LINEAR", sw)
            monkeypatch.setenv("CGS_STRICT_NATIVE", sw)
            ops.reset_stats()
            out = g(x.to(cuda, BF)).float().cpu()
            libs = {k for k in ops.stats() if k[1] == "lib"}
            assert libs == (set() if sw == "1" else {("gemm", "lib"), ("layernorm", "lib")}), libs
            assert ((out - ref).norm() / ref.norm()).item() < 3e-2
