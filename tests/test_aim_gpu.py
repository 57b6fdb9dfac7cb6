"""ops.token_dwconv3x3 and ops.adaptive_interaction (csrc/kernels/token_mix.hip) on the device: per-element bounds
against an fp64 reference in plain torch, output integrity, entry refusals, and DAT with the two switches on and off."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bounds import assert_within                                                        # noqa: E402
from _bounds_aim import BF, aim_bound, aim_modules, token_dwconv_bound                   # noqa: E402

from comfy_gen_server_amd import _native, ops                                            # noqa: E402
from comfy_gen_server_amd.ops.core import _aim_tensors                                   # noqa: E402

pytestmark = pytest.mark.gpu
CONV_CASES = [(1, 1, 1, 4, "plain"), (1, 3, 5, 12, "plain"), (2, 17, 19, 60, "slice"), (1, 16, 33, 180, "bn"),
              (1, 35, 16, 68, "mul")]
AIM_CASES = [(1, 1, 1, 16, 2, 1), (1, 5, 7, 16, 2, 1), (2, 17, 19, 60, 7, 3), (1, 16, 33, 180, 22, 11),
             (1, 35, 16, 256, 32, 16)]


@pytest.mark.parametrize("B,H,W,C,mode", CONV_CASES)
def test_token_dwconv3x3_bound(cuda, B, H, W, C, mode):
    g = torch.Generator().manual_seed(100 * H + C)
    N = H * W
    wide = torch.randn(B, N, 3 * C, generator=g).to(BF)
    x = wide[..., 2 * C:] if mode == "slice" else wide[..., :C].contiguous()
    dw = aim_modules(max(C, 16), 1, 1, C)[0]
    w, b = dw[0].weight[:C].to(BF).contiguous(), dw[0].bias[:C].to(BF).contiguous()
    bn = tuple(t[:C].to(BF).contiguous() for t in (dw[1].weight, dw[1].bias, dw[1].running_mean, dw[1].running_var)) \
        + (1e-5,) if mode == "bn" else None
    mul = torch.randn(B, N, 2 * C, generator=g).to(BF)[..., :C] if mode == "mul" else None
    ref, tol = token_dwconv_bound(x, (H, W), w, b, bn, mul)
    dev = lambda t: None if t is None else t.to(cuda)                                    # noqa: E731
    xd = wide.to(cuda)[..., 2 * C:] if mode == "slice" else x.to(cuda)
    md = None if mul is None else torch.cat([mul, mul], -1).to(cuda)[..., :C]
    kw = dict(bn=None if bn is None else tuple(dev(t) for t in bn[:4]) + (1e-5,), act="gelu" if bn else None, mul=md)
    ops.reset_stats()
    y, st = ops.token_dwconv3x3(xd, (H, W), dev(w), dev(b), **kw), ops.stats()
    assert st.get(("token_dwconv3x3", "hip"), 0) == 1 and not [k for k in st if k[1] == "lib"], st
    assert_within(y.cpu(), ref, tol, f"token_dwconv3x3 {(B, H, W, C, mode)}")
    assert torch.equal(y, ops.token_dwconv3x3(xd, (H, W), dev(w), dev(b), **kw))


@pytest.mark.parametrize("kind", ["spatial", "channel"])
@pytest.mark.parametrize("B,H,W,C,hc,hs", AIM_CASES)
def test_adaptive_interaction_bound(cuda, kind, B, H, W, C, hc, hs):
    g = torch.Generator().manual_seed(100 * H + C)
    N = H * W
    qkv, att = torch.randn(B, N, 3 * C, generator=g).to(BF), torch.randn(B, N, C, generator=g).to(BF)
    mods = aim_modules(C, hc, hs, C + hs + 10).to(BF)
    ref, tol, tg, cg = aim_bound(qkv, att, (H, W), mods, kind)
    assert N < 35 or ((tg > 0.1) & (tg < 0.9)).double().mean().item() >= 0.3
    assert cg.min().item() < 0.5 < cg.max().item()
    mods = mods.to(cuda)
    ops.reset_stats()
    y, st = ops.adaptive_interaction(qkv.to(cuda), att.to(cuda), (H, W), mods, kind), ops.stats()
    assert st.get(("adaptive_interaction", "hip"), 0) == 1 and not [k for k in st if k[1] == "lib"], st
    assert_within(y.cpu(), ref, tol, f"adaptive_interaction {kind} {(B, H, W, C, hc, hs)}")
    assert torch.equal(y, ops.adaptive_interaction(qkv.to(cuda), att.to(cuda), (H, W), mods, kind))


def test_aim_refusals_and_integrity(cuda):
    """A good call writes every output element finite from inputs that end a NaN-filled buffer and no bit around the
    output; each single broken rule returns hipErrorInvalidValue and leaves the output's bits alone."""
    lib = _native.load_kernels()
    B, H, W, C, hc, hs = 1, 5, 7, 20, 2, 1
    N = H * W
    mods = aim_modules(C, hc, hs, 3).to(BF).to(cuda)
    ts, eps = _aim_tensors(mods)
    ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    g = torch.Generator().manual_seed(5)
    qbuf = torch.full((4096 + N * 3 * C,), float("nan"), device=cuda, dtype=BF)
    qbuf[4096:] = torch.randn(N * 3 * C, generator=g).to(BF).to(cuda)
    abuf = torch.full((4096 + N * C,), float("nan"), device=cuda, dtype=BF)
    abuf[4096:] = torch.randn(N * C, generator=g).to(BF).to(cuda)
    nbytes = lib.cgs_aim_ws_bytes(B, H, W, C)
    ws = torch.zeros(nbytes, device=cuda, dtype=torch.uint8)
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(B=B, H=H, W=W, C=C, hc=hc, hs=hs, ws=True, short=0, qoff=0, ooff=0, pitch=C, epi=2)

    def aim(a, o):
        return lib.cgs_aim_fwd(qbuf.data_ptr() + 8192 + a["qoff"], abuf.data_ptr() + 8192, o + a["ooff"], ptrs, *eps,
                               ws.data_ptr() if a["ws"] else None, nbytes - a["short"], a["B"], a["H"], a["W"], a["C"],
                               a["hc"], a["hs"], 0, stream)

    def conv(a, o):      # y = m (conv + b): x the v third of qkv's rows, m = att
        return lib.cgs_token_dwconv3(qbuf.data_ptr() + 8192 + 4 * C + a["qoff"], 3 * a["pitch"], ts[0].data_ptr(),
                                     ts[1].data_ptr(), None, None, None, None, 0.0,
                                     abuf.data_ptr() + 8192 if a["epi"] == 2 else None, a["pitch"], o + a["ooff"], None,
                                     0, None, a["B"], a["H"], a["W"], a["C"], 2, stream)
    shape = {"C % 4": dict(C=18), "B": dict(B=0), "H": dict(H=0), "W": dict(W=0), "range": dict(H=46341, W=46341),
             "x align": dict(qoff=4), "y align": dict(ooff=4)}
    broken = {aim: {**shape, "C low": dict(C=12), "C cap": dict(C=260), "hc": dict(hc=33), "hs": dict(hs=17),
                    "no ws": dict(ws=False), "small ws": dict(short=16)},
              conv: {**shape, "pitch": dict(pitch=C + 2), "no m": dict(epi=0)}}
    for fn, cases in broken.items():
        for name, change in [("good", {})] + list(cases.items()):
            n = N * C
            buf = torch.full((n + 512,), float("nan"), device=cuda, dtype=BF)
            before = buf.view(torch.int16).clone()
            err = fn({**good, **change}, buf.data_ptr() + 512)
            torch.cuda.synchronize()
            after = buf.view(torch.int16)
            if name == "good":
                assert err == 0 and bool(torch.isfinite(buf[256:256 + n]).all()), fn.__name__
                assert torch.equal(after[:256], before[:256]) and torch.equal(after[256 + n:], before[256 + n:])
            else:
                assert err == 1, (fn.__name__, name, err)          # hipErrorInvalidValue
                assert torch.equal(after, before), name


def test_dat_aim_switch(cuda, monkeypatch):
    """The small two-group DAT of test_dat_switch. On: one fused AIM and one fused gate conv per block (8 each); off:
    none. Both within 3e-2 of the fp32 CPU model; the fused run reaches no vendor library the composed run does not."""
    from comfy_gen_server_amd.tools.rect_attn_bench import dat_model
    m = dat_model(64, 4, groups=2, depth=4, split=(2, 4))
    x = torch.rand(1, 3, 40, 32, generator=torch.Generator().manual_seed(1))
    libs = {}
    with torch.no_grad():
        ref = m(x)
        g = m.to(device=cuda, dtype=BF)
        for sw in ("1", "0"):
            monkeypatch.setenv("CGS_DAT_AIM", sw)
            monkeypatch.setenv("CGS_DAT_SGATE", sw)
            ops.reset_stats()
            out = g(x.to(cuda, BF)).float().cpu()
            st = ops.stats()
            assert st.get(("adaptive_interaction", "hip"), 0) == st.get(("token_dwconv3x3", "hip"), 0) == 8 * int(sw)
            libs[sw] = {k for k in st if k[1] == "lib"}
            assert ((out - ref).norm() / ref.norm()).item() < 3e-2
    assert libs["1"] <= libs["0"], libs
