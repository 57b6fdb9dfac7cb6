"""The activation set on the device: the elementwise kernel (cgs_act), the GEMM epilogue (EPI_GELU + code),
the conv epilogue (cgs_conv2d_nhwc_act), the op layer on top of them and the three model families that use
them, against plain PyTorch fp32 references. Every test asserts that the native path ran (ops.stats)."""
import json
import math

import pytest
import torch
import torch.nn.functional as F

from comfy_gen_server_amd import ops, _native
from comfy_gen_server_amd.ops import core

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _native_loaded(cuda, monkeypatch):
    assert _native.load_kernels() is not None, _native.kernels_error()
    monkeypatch.setenv("CGS_AUTOTUNE", "0")    # the tests pick the kernel explicitly
    ops.reset_stats()
    yield


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _ref_act(y, act, p=0.0):
    return core._act_torch(y, act, p)


ACTS = ["gelu", "gelu_tanh", "quick_gelu", "silu", "relu", "leaky_relu"]


# ------------------------------------------------------------------------------------------ elementwise
@pytest.mark.parametrize("n", [1, 7, 2051, 1 << 20])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("act", ACTS)
def test_activation_elementwise(cuda, n, dtype, act):
    """fp32: relu / leaky_relu exact, the others within 5e-5 absolute of torch's fp32 result on [-8, 8] (a
    tenth of the 4.7e-4 between tanh-GELU and erf-GELU, so this pins each GELU form). bf16 / fp16: the kernel
    rounds a value within 5e-5 of the fp32 reference to the output type, which adds at most half an ulp of
    the output (unit roundoff 2^-8 / 2^-11 relative), per element: |y - ref| <= 5e-5 (1 + half ulp) + half ulp |ref|."""
    torch.manual_seed(n)
    p = 0.2 if act == "leaky_relu" else 0.0
    x = ((torch.rand(n, device=cuda) * 16 - 8)).to(dtype)
    ref = _ref_act(x.float(), act, p)
    x0 = x.clone()
    y = ops.activation(x, act, p)
    assert ops.stats().get(("act", "hip"), 0) == 1
    assert y.dtype == dtype and y.shape == x.shape and torch.equal(x, x0)
    z = ops.activation(x, act, p, inplace=True)
    assert z.data_ptr() == x.data_ptr() and torch.equal(z, y)
    assert ops.stats().get(("act", "hip"), 0) == 2 and not any(k[1] == "lib" for k in ops.stats())
    if dtype == torch.float32:
        err = (y - ref).abs().max().item()
        print(f"act {act} n={n} fp32 max abs err {err:.3e}")
        if act in ("relu", "leaky_relu"):
            assert torch.equal(y, ref)
        else:
            assert err <= 5e-5, err
    else:
        half_ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11      # unit roundoff: 8 / 11 significand bits
        over = ((y.float() - ref).abs() - (5.01e-5 + half_ulp * ref.abs())).max().item()
        print(f"act {act} n={n} {dtype} max excess over the tolerance {over:.3e}")
        assert over <= 0, over


def test_gelu_op_is_native(cuda):
    x = torch.randn(3, 77, 320, device=cuda).to(torch.bfloat16)
    y = ops.gelu(x)
    yt = ops.gelu(x, approximate="tanh")
    assert ops.stats().get(("act", "hip"), 0) == 2
    assert _rel(y, F.gelu(x.float())) < 2.0 ** -8 and _rel(yt, F.gelu(x.float(), approximate="tanh")) < 2.0 ** -8
    # a channels_last image and a strided view
    img = torch.randn(2, 16, 5, 7, device=cuda).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    yi = ops.activation(img, "relu")
    assert yi.shape == img.shape and torch.equal(yi, torch.relu(img))
    v = x[:, :, 8:40]
    assert torch.equal(ops.activation(v, "relu"), torch.relu(v))
    ops.activation(v, "relu", inplace=True)
    assert torch.equal(x[:, :, 8:40], torch.relu(v)) and (x[:, :, 8:40] >= 0).all()


# ------------------------------------------------------------------------------------------ GEMM epilogue
GEMM_SHAPES = [(1000, 320, 128, 6), (4096, 1280, 320, 6), (1152, 8192, 256, 8), (300, 640, 96, 10),
               (64, 512, 256, -1), (2048, 256, 512, 4), (577, 264, 64, 14)]


def _gemm_case(cuda, M, N, K, res, seed=5):
    torch.manual_seed(seed)
    a = torch.randn(M, K, device=cuda).to(torch.bfloat16)
    w = (torch.randn(N, K, device=cuda) / math.sqrt(K)).to(torch.bfloat16)
    b = torch.randn(N, device=cuda).to(torch.bfloat16)
    r = torch.randn(M, N, device=cuda).to(torch.bfloat16) if res else None
    return a, w, b, r, a.float() @ w.float().t() + b.float()


@pytest.mark.parametrize("M,N,K,variant", GEMM_SHAPES)
@pytest.mark.parametrize("act", ["quick_gelu", "gelu_tanh", "silu", "relu"])
@pytest.mark.parametrize("res", [False, True])
def test_gemm_act_epilogue(cuda, M, N, K, variant, act, res):
    """EPI_GELU | code << 8: out = act(A W^T + b) (+ R) on v6, the mc::tile family and skinny. Bound 4e-3:
    bf16 output rounding alone is 1.66e-3 on these distributions, and an erf GELU where quick_gelu was asked
    would score 9.8e-3 (6.7e-3 with the residual) -- under the usual 1e-2."""
    a, w, b, r, h = _gemm_case(cuda, M, N, K, res)
    out = torch.empty(M, N, device=cuda, dtype=torch.bfloat16)
    epi = core.EPI_BIAS | core.EPI_GELU | (core.ACT_CODES[act] << 8) | (core.EPI_RESIDUAL if res else 0)
    rc = _native.load_kernels().cgs_gemm_bf16_v(a.data_ptr(), w.data_ptr(), out.data_ptr(), b.data_ptr(),
                                                 None if r is None else r.data_ptr(), M, N, K, K, K, N,
                                                 N if res else 0, epi, 1.0, variant, core._stream())
    assert rc == 0
    ref = _ref_act(h, act) + (r.float() if res else 0.0)
    e1 = _rel(out, ref)
    y = ops.linear(a, w, b, residual=r, act=act)
    e2 = _rel(y, ref)
    print(f"gemm_act M={M} N={N} K={K} v={variant} {act} res={res}: C entry {e1:.3e} ops.linear {e2:.3e}")
    assert e1 < 4e-3, e1
    assert e2 < 4e-3, e2
    assert ops.stats().get(("gemm", "hip"), 0) == 1 and ops.stats().get(("act_fused", "hip"), 0) == 1
    if act == "quick_gelu":     # farther from the erf GELU than from its own definition
        erf = F.gelu(h) + (r.float() if res else 0.0)
        assert _rel(out, erf) > e1 and _rel(y, erf) > e2


def test_gemm_act_skinny_clip_l_fc1(cuda):
    a, w, b, _, h = _gemm_case(cuda, 77, 3072, 768, False, seed=7)      # CLIP-L fc1 at one prompt
    y = ops.linear(a, w, b, act="quick_gelu")
    ref = _ref_act(h, "quick_gelu")
    assert _rel(y, ref) < 4e-3 and _rel(y, F.gelu(h)) > _rel(y, ref)
    assert ops.stats().get(("gemm", "hip"), 0) == 1


def test_gemm_act_bits_refused_elsewhere(cuda):
    """Entry points without the activation set return an error for its code bits (nothing is launched)."""
    lib = _native.load_kernels()
    M, N, K = 256, 256, 512
    a, w, b, _, h = _gemm_case(cuda, M, N, K, False, seed=9)
    out = torch.zeros(M, N, device=cuda, dtype=torch.bfloat16)
    ws = torch.empty(int(lib.cgs_splitk_ws_bytes(M, N, 2)), device=cuda, dtype=torch.uint8)
    qg = core.ACT_CODES["quick_gelu"] << 8

    def splitk(epi):
        return lib.cgs_gemm_bf16_splitk(a.data_ptr(), w.data_ptr(), out.data_ptr(), b.data_ptr(), None, None, None,
                                        M, N, K, K, K, N, 0, epi, 1.0, 2, 8, ws.data_ptr(), ws.numel(), core._stream())
    assert splitk(core.EPI_BIAS | core.EPI_GELU | qg) != 0
    torch.cuda.synchronize()
    assert not out.any()                                         # untouched
    assert splitk(core.EPI_BIAS | core.EPI_GELU) == 0            # the erf GELU it does know
    assert _rel(out, F.gelu(h)) < 1e-2
    # w6: no activation epilogue at all; the dispatcher refuses code bits without EPI_GELU and leaky_relu
    assert lib.cgs_gemm_w6_ok(2048, 1280, 1280, 1280, 1280, 1280, 0, core.EPI_BIAS, 256) == 1
    assert lib.cgs_gemm_w6_ok(2048, 1280, 1280, 1280, 1280, 1280, 0, core.EPI_BIAS | core.EPI_GELU | qg, 256) == 0
    assert lib.cgs_gemm_w6_ok(2048, 1280, 1280, 1280, 1280, 1280, 0, core.EPI_BIAS | qg, 256) == 0
    out.zero_()
    for epi in (core.EPI_BIAS | qg, core.EPI_BIAS | core.EPI_GELU | (core.ACT_CODES["leaky_relu"] << 8)):
        assert lib.cgs_gemm_bf16_v(a.data_ptr(), w.data_ptr(), out.data_ptr(), b.data_ptr(), None, M, N, K, K, K, N,
                                   0, epi, 1.0, 8, core._stream()) != 0
    torch.cuda.synchronize()
    assert not out.any()


# ------------------------------------------------------------------------------------------ conv epilogue
CONV_SHAPES = [(2, 64, 16, 16, 64, 3, 1, 1), (2, 96, 20, 20, 160, 3, 1, 1), (1, 160, 24, 24, 32, 3, 1, 1),
               (1, 128, 7, 9, 256, 1, 1, 0), (1, 320, 33, 17, 640, 3, 2, 1)]
CONV_ACTS = [("relu", 0.0), ("leaky_relu", 0.2), ("leaky_relu", 0.1), ("silu", 0.0)]


def _conv_act_entry(x, x2, w, b, r, s, p, up, variant, act, param):
    N, C1, H, W = x.shape
    Cin = C1 + (0 if x2 is None else x2.shape[1])
    Cout, _, kh, kw = w.shape
    Hl, Wl = (2 * H, 2 * W) if up else (H, W)
    Ho, Wo = (Hl + 2 * p - kh) // s + 1, (Wl + 2 * p - kw) // s + 1
    wn = w.permute(0, 2, 3, 1).contiguous()
    out = torch.empty((N, Cout, Ho, Wo), device=x.device, dtype=x.dtype, memory_format=torch.channels_last)
    rc = _native.load_kernels().cgs_conv2d_nhwc_act(
        x.data_ptr(), None if x2 is None else x2.data_ptr(), C1, wn.data_ptr(), b.data_ptr(),
        None if r is None else r.data_ptr(), out.data_ptr(), N, H, W, Cin, Cout, kh, kw, s, p, Ho, Wo,
        16 if up else 0, variant, core.ACT_CODES[act] if act else 0, param, core._stream())
    return rc, out


def _nhwc(t):
    return t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("N,Cin,H,W,Cout,k,s,p", CONV_SHAPES)
@pytest.mark.parametrize("variant", [3, 4, 8])
@pytest.mark.parametrize("res", [False, True])
def test_conv_act_epilogue(cuda, N, Cin, H, W, Cout, k, s, p, variant, res):
    """out = act(conv + bias) (+ r) through cgs_conv2d_nhwc_act, _rel < 1e-2 (test_conv2d's bound; another
    slope or no activation is >= 0.10 away). One conv reference per shape serves the four activations."""
    torch.manual_seed(0)
    x = _nhwc(torch.randn(N, Cin, H, W, device=cuda))
    w = (torch.randn(Cout, Cin, k, k, device=cuda) / math.sqrt(Cin * k * k)).to(torch.bfloat16)
    b = torch.randn(Cout, device=cuda).to(torch.bfloat16)
    h = F.conv2d(x.float(), w.float(), b.float(), s, p)
    r = _nhwc(torch.randn_like(h)) if res else None
    for act, param in CONV_ACTS:
        rc, out = _conv_act_entry(x, None, w, b, r, s, p, False, variant, act, param)
        assert rc == 0
        ref = _ref_act(h, act, param) + (r.float() if res else 0.0)
        err = _rel(out, ref)
        print(f"conv_act {N}x{Cin}x{H}x{W}->{Cout} k{k}s{s} v={variant} {act}({param}) res={res}: {err:.3e}")
        assert out.shape == ref.shape and err < 1e-2, (act, param, err)


@pytest.mark.parametrize("variant", [3, 4, 8])
@pytest.mark.parametrize("res", [False, True])
def test_conv_act_upsample_and_dual(cuda, variant, res):
    torch.manual_seed(1)
    x = _nhwc(torch.randn(1, 64, 12, 12, device=cuda))
    x2 = _nhwc(torch.randn(1, 64, 12, 12, device=cuda))
    b = torch.randn(64, device=cuda).to(torch.bfloat16)
    w1 = (torch.randn(64, 64, 3, 3, device=cuda) / 24).to(torch.bfloat16)
    w2 = (torch.randn(64, 128, 3, 3, device=cuda) / 34).to(torch.bfloat16)
    h_up = F.conv2d(F.interpolate(x.float(), scale_factor=2.0, mode="nearest"), w1.float(), b.float(), 1, 1)
    h_dual = F.conv2d(torch.cat([x, x2], 1).float(), w2.float(), b.float(), 1, 1)
    for act, param in CONV_ACTS:
        for h, args in ((h_up, (x, None, w1)), (h_dual, (x, x2, w2))):
            r = _nhwc(torch.randn_like(h)) if res else None
            rc, out = _conv_act_entry(args[0], args[1], args[2], b, r, 1, 1, args[1] is None, variant, act, param)
            assert rc == 0
            ref = _ref_act(h, act, param) + (r.float() if res else 0.0)
            assert out.shape == ref.shape and _rel(out, ref) < 1e-2, (act, param, _rel(out, ref))


def test_conv_act_refused_forms(cuda):
    """Variants without the activation epilogue and narrow outputs are an error code, not a launch."""
    x = _nhwc(torch.randn(1, 64, 8, 8, device=cuda))
    b = torch.randn(64, device=cuda).to(torch.bfloat16)
    w = (torch.randn(64, 64, 3, 3, device=cuda) / 24).to(torch.bfloat16)
    for variant in (-1, -2, 2, 5, 6, 7, 18, 21):
        rc, _ = _conv_act_entry(x, None, w, b, None, 1, 1, False, variant, "relu", 0.0)
        assert rc != 0, variant
    rc, _ = _conv_act_entry(x, None, w[:8], b[:8], None, 1, 1, False, 8, "relu", 0.0)
    assert rc != 0
    rc, out = _conv_act_entry(x, None, w, b, None, 1, 1, False, 8, None, 0.0)      # act 0: the plain conv
    assert rc == 0 and _rel(out, F.conv2d(x.float(), w.float(), b.float(), 1, 1)) < 1e-2


# ------------------------------------------------------------------------------------------ op-level conv
@pytest.mark.parametrize("fused", [None, "v4", "v8", "v3"])
def test_conv2d_op_act(cuda, fused, monkeypatch):
    """Autotune off: "split" (plain conv + the native activation). A table override picks a fused kernel."""
    N, Cin, H, W, Cout = 2, 96, 20, 20, 160
    torch.manual_seed(2)
    x = _nhwc(torch.randn(N, Cin, H, W, device=cuda))
    w = (torch.randn(Cout, Cin, 3, 3, device=cuda) / math.sqrt(Cin * 9)).to(torch.bfloat16)
    b = torch.randn(Cout, device=cuda).to(torch.bfloat16)
    r = _nhwc(torch.randn(N, Cout, H, W, device=cuda))
    wn = w.permute(0, 2, 3, 1).contiguous()
    ref = F.leaky_relu(F.conv2d(x.float(), w.float(), b.float(), 1, 1), 0.2)
    if fused is not None:
        monkeypatch.setenv("CGS_AUTOTUNE", "1")
        keys = {"|".join(str(p) for p in ("conv", N, H, W, Cin, Cout, 3, 1, 1, 0, rr, "act", "leaky_relu", 0.2)): fused
                for rr in (0, 1)}
        monkeypatch.setenv("CGS_TUNE_OVERRIDE", json.dumps(keys))
    y = ops.conv2d(x, w, b, 1, 1, weight_nhwc=wn, act="leaky_relu", act_param=0.2)
    st = ops.stats()
    assert st.get(("conv", "hip"), 0) == 1 and not any(k[1] == "lib" for k in st)
    if fused is None:
        assert st.get(("act", "hip"), 0) == 1 and st.get(("act_fused", "hip"), 0) == 0
    else:
        assert st.get(("act_fused", "hip"), 0) == 1 and st.get(("act", "hip"), 0) == 0
    assert y.shape == ref.shape and _rel(y, ref) < 1e-2
    y2 = ops.conv2d(x, w, b, 1, 1, residual=r, weight_nhwc=wn, act="leaky_relu", act_param=0.2)
    assert _rel(y2, ref + r.float()) < 1e-2


# ------------------------------------------------------------------------------------------ models
def _native_act_ran():
    st = ops.stats()
    return (st.get(("act", "hip"), 0) + st.get(("act_fused", "hip"), 0)) > 0 and not any(
        k[1] == "lib" for k in st if k[0] in ("act", "act_fused", "gemm", "conv"))


@pytest.mark.parametrize("hidden_act", ["quick_gelu", "gelu"])
def test_clip_text_model_bf16(cuda, hidden_act):
    """Tiny CLIP text tower in bf16 on the device against the same weights in fp32 on the CPU; 3e-2 is the
    bound of the production-scale CLIP check (test_golden_sdxl_gpu.py)."""
    from comfy_gen_server_amd.models import clip as clip_mod
    from comfy_gen_server_amd.models.layers import init_random_
    cfg = dict(num_hidden_layers=2, hidden_size=64, num_attention_heads=1, intermediate_size=256, projection_dim=64,
               vocab_size=1000, max_position_embeddings=77, hidden_act=hidden_act)
    with torch.no_grad():
        m = clip_mod.CLIPTextModel(cfg, dtype=torch.float32)
        init_random_(m, seed=1)
        tokens = torch.randint(1, 999, (2, 77))
        tokens[:, -1] = 999
        want = m(tokens)[0]
        md = clip_mod.CLIPTextModel(cfg, dtype=torch.float32)
        md.load_state_dict(m.state_dict())
        md = md.to(device=cuda, dtype=torch.bfloat16)
        ops.reset_stats()
        got = md(tokens.to(cuda))[0]
    assert _native_act_ran() and ops.stats().get(("act_fused", "hip"), 0) == 2, ops.stats()     # one fc1 per layer
    assert _rel(got.cpu(), want) < 3e-2, _rel(got.cpu(), want)


def test_rdb_bf16(cuda):
    """One ESRGAN dense block (64, 32) at 24 x 24; 3e-2 is test_upscale_esrgan_gpu's bound."""
    from comfy_gen_server_amd.models import upscalers
    from comfy_gen_server_amd.models.layers import init_random_
    with torch.no_grad():
        m = upscalers.ResidualDenseBlock5C(64, 32)
        init_random_(m, seed=2)
        x = torch.randn(1, 64, 24, 24)
        want = m(x)
        md = upscalers.ResidualDenseBlock5C(64, 32)
        md.load_state_dict(m.state_dict())
        md = md.to(device=cuda, dtype=torch.bfloat16)
        ops.reset_stats()
        got = md(_nhwc(x.to(cuda)))
    assert _native_act_ran() and ops.stats().get(("conv", "hip"), 0) == 5, ops.stats()
    assert _rel(got.cpu(), want) < 3e-2, _rel(got.cpu(), want)


def test_taesd_block_bf16(cuda):
    """One TAESD Block(64, 64) at 16 x 16, with the bound of the other bf16 conv stacks (3e-2)."""
    from comfy_gen_server_amd.models import taesd
    from comfy_gen_server_amd.models.layers import init_random_
    with torch.no_grad():
        m = taesd.Block(64, 64)
        init_random_(m, seed=3)
        x = torch.randn(1, 64, 16, 16)
        want = m(x)
        md = taesd.Block(64, 64)
        md.load_state_dict(m.state_dict())
        md = md.to(device=cuda, dtype=torch.bfloat16)
        ops.reset_stats()
        got = md(_nhwc(x.to(cuda)))
    assert _native_act_ran() and ops.stats().get(("act", "hip"), 0) == 3, ops.stats()    # two split convs + the last
    assert (got >= 0).all() and _rel(got.cpu(), want) < 3e-2, _rel(got.cpu(), want)
