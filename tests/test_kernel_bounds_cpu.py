"""Self-test of tests/_bounds.py on the CPU: a plain emulation of what the kernels compute (fp32 accumulate, one
bf16 round; for attention a 64-key-tile online softmax with bf16 P) stays inside the bound in every element, and
each of a set of injected faults -- every one of them under the 1e-2 (attention 2e-2) Frobenius-norm threshold
of the older kernel tests -- is rejected by assert_within."""
import math

import pytest
import torch
import torch.nn.functional as F

from _bounds import assert_within, attention_bound, conv_bound, geglu_bound, gemm_bound, lnfold_bound, rel

BF = torch.bfloat16
GEMM_SHAPES = [(33, 40, 32), (300, 320, 640), (129, 136, 192), (257, 264, 5120)]
FAULT_SHAPES = [(300, 320, 640), (512, 328, 1280), (257, 264, 5120)]     # large enough for the norm to hide the fault


def _gemm_inputs(M, N, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(M, K, generator=g) + 0.5).to(BF)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF)
    b = torch.randn(N, generator=g).to(BF)
    r = torch.randn(M, N, generator=g).to(BF)
    return a, w, b, r


def _emulate_gemm(a, w, b=None, r=None):
    """fp32 accumulate and epilogue, one bf16 round."""
    acc = a.float() @ w.float().t()
    if b is not None:
        acc = acc + b.float()
    if r is not None:
        acc = acc + r.float()
    return acc.to(BF)


def _rejected(y, ref, tol, what):
    with pytest.raises(AssertionError, match="over tol"):
        assert_within(y, ref, tol, what)


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("epi", ["none", "bias", "bias_res"])
def test_gemm_emulation_within_bound(M, N, K, epi):
    a, w, b, r = _gemm_inputs(M, N, K)
    b = b if epi != "none" else None
    r = r if epi == "bias_res" else None
    ref, tol = gemm_bound(a, w, b, r)
    assert_within(_emulate_gemm(a, w, b, r), ref, tol, f"emulated gemm {M}x{N}x{K} {epi}")
    if r is not None:                 # the two-rounding epilogue of the tile kernels: bf16(bf16(pre) + res)
        y2 = ((a.float() @ w.float().t() + b.float()).to(BF).float() + r.float()).to(BF)
        assert_within(y2, ref, tol, f"emulated gemm {M}x{N}x{K} bias, bf16 round, + res")


@pytest.mark.parametrize("M,N,K", FAULT_SHAPES)
@pytest.mark.parametrize("what", ["bias", "res"])
def test_gemm_fault_edge_vector_epilogue_dropped(M, N, K, what):
    """Bias or residual missing on the last 8-wide vector of the last row."""
    a, w, b, r = _gemm_inputs(M, N, K)
    ref, tol = gemm_bound(a, w, b, r)
    acc = a.float() @ w.float().t() + b.float() + r.float()
    acc[-1, -8:] -= b.float()[-8:] if what == "bias" else r.float()[-1, -8:]
    y = acc.to(BF)
    assert rel(y, ref) < 1e-2
    _rejected(y, ref, tol, f"gemm {M}x{N}x{K}: {what} dropped on the last vector")


@pytest.mark.parametrize("M,N,K", FAULT_SHAPES)
def test_gemm_fault_bf16_accumulator(M, N, K):
    """The accumulator rounded to bf16 after every 64-wide K step (a partial kept in bf16)."""
    a, w, b, r = _gemm_inputs(M, N, K)
    ref, tol = gemm_bound(a, w, b, None)
    acc = torch.zeros(M, N)
    for k0 in range(0, K, 64):
        acc = (acc + a[:, k0:k0 + 64].float() @ w[:, k0:k0 + 64].float().t()).to(BF).float()
    y = (acc + b.float()).to(BF)
    assert rel(y, ref) < 1e-2
    _rejected(y, ref, tol, f"gemm {M}x{N}x{K}: bf16 accumulator")


def test_gemm_fault_k_tail_dropped():
    """The last 8 of K missing for one 16-row block: coherent, because the activations have mean 0.5."""
    M, N, K = 257, 264, 5120
    a, w, b, r = _gemm_inputs(M, N, K)
    ref, tol = gemm_bound(a, w, b, None)
    acc = a.float() @ w.float().t() + b.float()
    acc[64:80] -= a[64:80, -8:].float() @ w[:, -8:].float().t()
    y = acc.to(BF)
    assert rel(y, ref) < 1e-2
    _rejected(y, ref, tol, "gemm 257x264x5120: K tail dropped for rows 64..79")


def test_gemm_bound_alpha_and_explicit_k():
    a, w, b, r = _gemm_inputs(65, 72, 96)
    ref, tol = gemm_bound(a, w, b, r, alpha=0.25)
    assert_within(((a.float() @ w.float().t()) * 0.25 + b.float() + r.float()).to(BF), ref, tol, "gemm alpha 0.25")
    ref2, tol2 = gemm_bound(a, w, b, r, alpha=0.25, K=192)
    assert torch.equal(ref, ref2) and (tol2 > tol).all()


def test_geglu_and_lnfold_emulation_within_bound():
    M, N2, K = 70, 96, 128
    a, w, _, _ = _gemm_inputs(M, N2, K, seed=1)
    b = torch.randn(N2, generator=torch.Generator().manual_seed(2)).to(BF)
    ref, tol = geglu_bound(a, w, b)
    h = a.float() @ w.float().t() + b.float()
    x1, g = h.chunk(2, -1)
    assert_within((x1 * F.gelu(g)).to(BF), ref, tol, "emulated geglu")
    y = (x1 * F.gelu(g)).clone()
    y[-1, -8:] = (x1 * g)[-1, -8:]                       # the gate's GELU skipped on the last vector
    _rejected(y.to(BF), ref, tol, "geglu: gelu skipped on the last vector")
    # LayerNorm fold from the operands the kernel gets
    x = (a.float() * 3 + 1.5).to(BF)
    mu = x.float().mean(1)
    rs = torch.stack([mu, torch.rsqrt(x.float().var(1, unbiased=False) + 1e-5)], 1)
    cs = w.float().sum(1)
    ref, tol = lnfold_bound(x, w, b, rs, cs)
    y = rs[:, 1:2] * (x.float() @ w.float().t() - rs[:, :1] * cs[None]) + b.float()
    assert_within(y.to(BF), ref, tol, "emulated lnfold")
    ln = F.layer_norm(x.double(), (K,), eps=1e-5) @ w.double().t() + b.double()
    assert rel(ref, ln) < 1e-5                            # the folded form is the LayerNorm -> Linear it stands for
    y[3, 8:16] += (rs[:, 1:2] * rs[:, :1] * cs[None])[3, 8:16] * 0.02      # 2 % of the mean term off on one vector
    _rejected(y.to(BF), ref, tol, "lnfold: mean term off on one vector")
    ref, tol = lnfold_bound(x, w, b, rs, cs, geglu=True)
    x1, g = (rs[:, 1:2] * (x.float() @ w.float().t() - rs[:, :1] * cs[None]) + b.float()).chunk(2, -1)
    assert_within((x1 * F.gelu(g)).to(BF), ref, tol, "emulated lnfold geglu")


# ------------------------------------------------------------------------------------------------ conv
def _conv_inputs(N, C1, C2, H, W, Cout, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, C1, H, W, generator=g) + 0.5).to(BF)
    x2 = (torch.randn(N, C2, H, W, generator=g) + 0.5).to(BF)
    w = (torch.randn(Cout, C1 + C2, 3, 3, generator=g) / math.sqrt((C1 + C2) * 9)).to(BF)
    b = torch.randn(Cout, generator=g).to(BF)
    return g, x, x2, w, b


@pytest.mark.parametrize("stride,up", [(1, False), (2, False), (1, True)])
def test_conv_emulation_within_bound(stride, up):
    g, x, x2, w, b = _conv_inputs(3, 24, 8, 5, 7, 8)
    ref, tol = conv_bound(x, w, b, None, stride, 1, upsample2x=up, x2=x2)
    xin = torch.cat([x, x2], 1).float()
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    acc = F.conv2d(xin, w.float(), b.float(), stride, 1)
    r = torch.randn(acc.shape, generator=g).to(BF)
    assert_within(acc.to(BF), ref, tol, f"emulated conv s{stride} up={up}")
    ref_r, tol_r = conv_bound(x, w, b, r, stride, 1, upsample2x=up, x2=x2)
    assert_within((acc + r.float()).to(BF), ref_r, tol_r, f"emulated conv s{stride} up={up} + res")


def test_conv_fault_corner_mispadded():
    """One corner of the last image mis-padded: its out-of-image tap (-1, -1) reads pixel (0, 0) instead of 0."""
    g, x, x2, w, b = _conv_inputs(3, 24, 8, 24, 24, 16)
    ref, tol = conv_bound(x, w, b, None, 1, 1, x2=x2)
    xin = torch.cat([x, x2], 1).float()
    y = F.conv2d(xin, w.float(), b.float(), 1, 1)
    assert_within(y.to(BF), ref, tol, "emulated conv 3x32x24x24")
    y[-1, :, 0, 0] += (xin[-1, :, 0, 0][None] * w.float()[:, :, 0, 0]).sum(1)
    assert rel(y.to(BF), ref) < 1e-2
    _rejected(y.to(BF), ref, tol, "conv: one corner mis-padded")


# ------------------------------------------------------------------------------------------------ attention
def _emulate_flash(q, k, v, heads, tile=64, ignore_last_key_rows=None):
    """Online softmax over 64-key tiles: fp32 scores, running max / sum, P rounded to bf16 before P V, the
    normaliser summed from the unrounded P, one bf16 round of the output."""
    B, Sq, HD = q.shape
    Sk, D = k.shape[1], HD // heads
    qh = q.float().reshape(B, Sq, heads, D).transpose(1, 2)
    kh = k.float().reshape(B, Sk, heads, D).transpose(1, 2)
    vh = v.float().reshape(B, Sk, heads, D).transpose(1, 2)
    m = torch.full((B, heads, Sq, 1), -math.inf)
    l = torch.zeros(B, heads, Sq, 1)
    o = torch.zeros(B, heads, Sq, D)
    for j0 in range(0, Sk, tile):
        s = (qh @ kh[:, :, j0:j0 + tile].transpose(-1, -2)) * (1.0 / math.sqrt(D))
        if ignore_last_key_rows is not None and j0 + tile >= Sk:
            b_, h_, rows = ignore_last_key_rows
            s[b_, h_, rows, -1] = -math.inf
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        p = torch.exp(s - m_new)
        c = torch.exp(m - m_new)
        l = l * c + p.sum(-1, keepdim=True)
        o = o * c + p.to(BF).float() @ vh[:, :, j0:j0 + tile]
        m = m_new
    return (o / l).transpose(1, 2).reshape(B, Sq, HD).to(BF)


def _attn_inputs(B, H, Sq, Sk, D, seed=0, spike=False):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Sq, H * D, generator=g)
    k = torch.randn(B, Sk, H * D, generator=g)
    v = torch.randn(B, Sk, H * D, generator=g)
    if spike:
        q *= 3.0
        for j in range(Sk // 3, Sk, max(1, Sk // 5)):
            k[:, j, :] *= 1.0 + 0.5 * (j * 7 % 11)
    return q.to(BF), k.to(BF), v.to(BF)


@pytest.mark.parametrize("B,H,Sq,Sk,D,spike", [(2, 5, 300, 77, 64, False), (1, 2, 129, 130, 40, False),
                                               (2, 3, 63, 200, 64, True), (1, 1, 1, 1, 64, False)])
def test_attention_emulation_within_bound(B, H, Sq, Sk, D, spike):
    q, k, v = _attn_inputs(B, H, Sq, Sk, D, spike=spike)
    ref, tol = attention_bound(q, k, v, H)
    assert_within(_emulate_flash(q, k, v, H), ref, tol, f"emulated attention {B}x{H}x{Sq}x{Sk} D={D} spike={spike}")


def test_attention_bound_masks():
    """causal and key_padding in the bound follow the definitions of ops.attention's reference."""
    from comfy_gen_server_amd.ops import core
    q, k, v = _attn_inputs(2, 3, 20, 20, 32, seed=5)
    kp = torch.ones(2, 20, dtype=torch.bool)
    kp[0, 13:] = False
    kp[1, 1:] = False
    for causal, pad in ((True, None), (False, kp), (True, kp)):
        ref, tol = attention_bound(q, k, v, 3, causal=causal, key_padding=pad)
        want = core.attention_reference(q.float(), k.float(), v.float(), 3, causal=causal, key_padding=pad)
        assert (ref - want.double()).abs().max().item() < 1e-5 and bool((tol > 0).all())


def test_attention_faults():
    B, H, Sq, Sk, D = 2, 5, 300, 77, 64
    q, k, v = _attn_inputs(B, H, Sq, Sk, D)
    ref, tol = attention_bound(q, k, v, H)
    good = _emulate_flash(q, k, v, H)
    # one 8-wide output vector taken from the neighbouring query
    y = good.clone()
    y[1, 200, 3 * D + 8:3 * D + 16] = good[1, 201, 3 * D + 8:3 * D + 16]
    assert rel(y, ref) < 2e-2
    _rejected(y, ref, tol, "attention: one output vector from the neighbouring query")
    # the last key ignored for the last 16 queries of one head
    y = _emulate_flash(q, k, v, H, ignore_last_key_rows=(1, 2, slice(Sq - 16, Sq)))
    assert rel(y, ref) < 2e-2
    _rejected(y, ref, tol, "attention: last key ignored for 16 queries of one head")
    # a split partial kept in bf16 needs its extra rounding: two 64-key slices merged by log-sum-exp
    ref1, tol1 = attention_bound(q, k, v, H, extra_roundings=1)
    assert torch.equal(ref, ref1) and bool((tol1 > tol).all())
