"""Self-test of tests/_bounds.py on the CPU: a plain emulation of what the kernels compute (fp32 accumulate, one
bf16 round; for attention a 64-key-tile online softmax with bf16 P) stays inside the bound in every element, and
each of a set of injected faults -- every one of them under the 1e-2 (attention 2e-2) Frobenius-norm threshold
of the older kernel tests -- is rejected by assert_within. The norm, depthwise and softmax2 bounds are checked in
bf16 and fp16 against emulations of the kernels' own algorithms (shifted block sums and Chan merges for GroupNorm,
two passes for LayerNorm). The GRN family and the planar image-space kernels (upfirdn2d, fused_bias_act, resize,
softmax_rows, tome_match) follow at the end: an emulation of each kernel's own slice, merge and tap structure, and
the faults its older tests could not see. Last, the fused epilogues: the activation set behind the GEMM and conv
epilogues from the kernel's own constants, and the statistics partials a producer writes beside its output (row
statistics, sums of squares, GroupNorm partials) in the lane and register order of mfma_pp160.h."""
import math

import pytest
import torch
import torch.nn.functional as F

from _bounds import (FBA_SHAPES, GRN_GNS_SHAPES, GRN_V2_SHAPES, RESIZE_CASES, RESIZE_MODES, RSO_LANE_COLS, SMR_COLS,
                     SMR_ROWS, TOME_SHAPES, UPFIRDN_CFGS, UPFIRDN_KERNELS, affine_layernorm_bound, assert_tome,
                     assert_within, attention_bound, conv_act_bound, conv_bound, dwconv_bound, fused_bias_act_bound,
                     geglu_bound, gemm_act_bound, gemm_bound, gn_partials_bound, grn_apply_bound, grn_bound, grn_depth,
                     grn_inputs, grn_nx, grn_row_tiled, grn_scale_weight_bound, grn_slices, grn_stats_bound,
                     groupnorm_apply_bound, groupnorm_bound, groupnorm_stats_bound, layernorm_bound,
                     layernorm_stats_bound, lnfold_bound, partials_merge_tol, rel, resize_bound, resize_coords,
                     rowstats_partials_bound, rs_from_partials_bound, smr_inputs, softmax2_bound, softmax_rows_bound,
                     sumsq_partials_bound, tome_inputs, upfirdn2d_bound, upfirdn_kernel)

BF = torch.bfloat16
DTYPES = [torch.bfloat16, torch.float16]
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


# ------------------------------------------------------------------------------------------------ GroupNorm
SPIKE = 48.0


def _gn_inputs(N, C, H, W, G, dtype, ppb, shift=1.0, seed=0, narrow=False):
    """x NCHW (a view of NHWC rows) = 3 randn + shift with a spike at the last pixel of every statistics block (one
    channel of the first and of the last group), at the first and last element of every image's first and last
    row; gamma, beta, and pre_add as columns 104 .. 104 + C of a [N, 1000 + C] tensor. narrow: gamma within 3 %
    of 1 and a pre_add of 0.03 randn, so that a misplaced vector of either stays under the Frobenius threshold."""
    g = torch.Generator().manual_seed(seed)
    HW = H * W
    xr = torch.randn(N, HW, C, generator=g) * 3 + shift
    for p in list(range(ppb - 1, HW, ppb)) + [HW - 1]:
        xr[:, p, 0] = SPIKE
        xr[:, p, C - 1] = -SPIKE
    xr[:, 0, 0] = xr[:, -1, -1] = SPIKE
    xr[:, 0, -1] = xr[:, -1, 0] = -SPIKE
    x = xr.to(dtype).reshape(N, H, W, C).permute(0, 3, 1, 2)
    w = (1 + 0.03 * torch.randn(C, generator=g) if narrow else torch.randn(C, generator=g) + 1).to(dtype)
    b = torch.randn(C, generator=g).to(dtype)
    wide = (torch.randn(N, 1000 + C, generator=g) * (0.03 if narrow else 1.0)).to(dtype)
    return x, w, b, wide, wide[:, 104:104 + C]


def _emulate_gn(x, G, w, b, eps, silu, pre, ppb, fault=None, wide=None):
    """What the GroupNorm kernels compute, in fp32: per pixel block and channel the sums of d = x - (the block's
    first pixel) -> (mean, M2); Chan merge over blocks and channels per group; a = rstd gamma, b = (pre - mean) a
    + beta; x a + b; sigmoid; one round. fault: 'coef' the first row of every image n > 0 takes image n - 1's
    (a, b); 'tail' the last pixel of the last block left out; 'gamma' the last 8-channel vector takes its
    neighbour's gamma; 'pld' the pre_add row of image n > 0 read at n * C instead of n * stride out of ``wide``."""
    dt = x.dtype
    N, C, H, W = x.shape
    HW, Cg = H * W, C // G
    xf = x.float().permute(0, 2, 3, 1).reshape(N, HW, C)
    pr = torch.zeros(N, C) if pre is None else pre.float()
    if fault == "pld":
        flat = wide.float().reshape(-1)
        pr = torch.stack([flat[104 + n * C:104 + (n + 1) * C] for n in range(N)])
    nb = (HW + ppb - 1) // ppb
    cnt, mean, m2 = torch.zeros(N, G), torch.zeros(N, G), torch.zeros(N, G)
    for bi in range(nb):
        blk = xf[:, bi * ppb:min(HW, (bi + 1) * ppb)]
        if fault == "tail" and bi == nb - 1 and blk.shape[1] > 1:
            blk = blk[:, :-1]
        c = float(blk.shape[1])
        d = blk - blk[:, :1]
        s1, s2 = d.sum(1), (d * d).sum(1)
        bm = (blk[:, 0] + s1 / c + pr).reshape(N, G, Cg)
        bq = (s2 - s1 * s1 / c).clamp_min(0).reshape(N, G, Cg)
        for cc in range(Cg):
            nn = cnt + c
            dd, f = bm[:, :, cc] - mean, c / nn
            mean = mean + dd * f
            m2 = m2 + bq[:, :, cc] + dd * dd * cnt * f
            cnt = nn
    rstd = torch.rsqrt((m2 / cnt).clamp_min(0) + eps)
    gm = torch.ones(C) if w is None else w.float().clone()
    bt = torch.zeros(C) if b is None else b.float()
    if fault == "gamma":
        gm[-8:] = gm[-16:-8]
    a = rstd.repeat_interleave(Cg, 1) * gm[None]
    bb = (pr - mean.repeat_interleave(Cg, 1)) * a + bt[None]
    A, B = a[:, None, :].expand(N, HW, C).clone(), bb[:, None, :].expand(N, HW, C).clone()
    if fault == "coef":
        A[1:, 0], B[1:, 0] = a[:-1], bb[:-1]
    f = xf * A + B
    if silu:
        f = f * torch.sigmoid(f)
    return f.to(dt).reshape(N, H, W, C).permute(0, 3, 1, 2), torch.stack([mean, m2], -1), torch.stack([mean, rstd], -1)


GN_EMU_SHAPES = [(2, 64, 13, 15, 32, 64, 1.0), (5, 320, 13, 15, 32, 16, 1.0), (2, 520, 9, 9, 8, 64, 8.0),
                 (2, 128, 16, 16, 32, 64, 40.0), (2, 64, 1, 3, 32, 64, 1.0)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("N,C,H,W,G,ppb,shift", GN_EMU_SHAPES)
def test_groupnorm_emulation_within_bound(N, C, H, W, G, ppb, shift, silu, dtype):
    x, w, b, wide, pre = _gn_inputs(N, C, H, W, G, dtype, ppb, shift)
    what = f"emulated groupnorm {N}x{C}x{H}x{W} G={G} silu={silu} {dtype}"
    for pa in (None, pre):
        y, stats, mr = _emulate_gn(x, G, w, b, 1e-5, silu, pa, ppb)
        ref, tol = groupnorm_bound(x, G, w, b, 1e-5, silu, pa, ppb=ppb)
        assert_within(y, ref, tol, what + f" pre={pa is not None}")
        ref, tol = groupnorm_stats_bound(x, G, pa, ppb=ppb)
        assert_within(stats, ref, tol, what + " (mean, M2)")
        ref, tol = groupnorm_apply_bound(x, G, w, b, mr, silu, pa)
        assert_within(y, ref, tol, what + " apply")
    C1 = C // 2 - C // 2 % 8
    ref2, tol2 = groupnorm_bound(x[:, :C1], G, w, b, 1e-5, silu, pre, x2=x[:, C1:])
    ref, tol = groupnorm_bound(x, G, w, b, 1e-5, silu, pre)
    assert torch.equal(ref, ref2) and torch.equal(tol, tol2)


GN_FAULT_SHAPES = [(3, 320, 24, 24, 32, 64), (4, 128, 28, 28, 32, 64)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fault", ["coef", "tail", "gamma", "pld"])
@pytest.mark.parametrize("N,C,H,W,G,ppb", GN_FAULT_SHAPES)
def test_groupnorm_faults(N, C, H, W, G, ppb, fault, dtype):
    x, w, b, wide, pre = _gn_inputs(N, C, H, W, G, dtype, ppb, narrow=True)
    ref, tol = groupnorm_bound(x, G, w, b, 1e-5, True, pre, ppb=ppb)
    y, stats, mr = _emulate_gn(x, G, w, b, 1e-5, True, pre, ppb, fault=fault, wide=wide)
    assert rel(y, ref) < 1e-2
    _rejected(y, ref, tol, f"groupnorm {N}x{C}x{H}x{W} {dtype}: fault {fault}")
    if fault == "tail":
        ref, tol = groupnorm_stats_bound(x, G, pre, ppb=ppb)
        _rejected(stats, ref, tol, f"groupnorm (mean, M2) {N}x{C}x{H}x{W} {dtype}: fault {fault}")
    if fault in ("coef", "gamma"):              # faults of the apply pass: its own (mean, rstd) are what it was given
        ref, tol = groupnorm_apply_bound(x, G, w, b, mr, True, pre)
        _rejected(y, ref, tol, f"groupnorm apply {N}x{C}x{H}x{W} {dtype}: fault {fault}")


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_inputs(rows, C, dtype, mean=0.5, spread=2.0, spike=SPIKE, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * spread + mean
    if spike:
        x[:, 0] = mean + spike
        x[:, -1] = mean - spike
    return x.to(dtype), (torch.randn(C, generator=g) + 1).to(dtype), torch.randn(C, generator=g).to(dtype)


def _emulate_ln(x, w, b, eps, fault=None):
    """Two-pass fp32 LayerNorm, one round. fault: 'chunk' the last 8 elements missing from both sums; 'onepass'
    the variance as E[x^2] - mean^2."""
    xf = x.float()
    C = x.shape[-1]
    xs = xf[:, :-8] if fault == "chunk" else xf
    m = xs.sum(-1, keepdim=True) / C
    if fault == "onepass":
        q = ((xf * xf).sum(-1, keepdim=True) / C - m * m).clamp_min(0)
    else:
        q = ((xs - m) ** 2).sum(-1, keepdim=True) / C
    r = torch.rsqrt(q + eps)
    f = (xf - m) * r
    if w is not None:
        f = f * w.float()
    if b is not None:
        f = f + b.float()
    return f.to(x.dtype), torch.cat([m, r], -1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,mean,spread", [(8, 0.5, 2.0), (72, 40.0, 2.0), (520, 0.5, 2.0), (2048, 200.0, 0.5),
                                           (5120, 0.5, 2.0)])
def test_layernorm_emulation_within_bound(C, mean, spread, dtype):
    x, w, b = _ln_inputs(33, C, dtype, mean, spread)
    for wi, bi in ((w, b), (w, None), (None, None)):
        y, rs = _emulate_ln(x, wi, bi, 1e-5)
        ref, tol = layernorm_bound(x, wi, bi, 1e-5)
        assert_within(y, ref, tol,
                      f"emulated layernorm C={C} mean {mean} {dtype} w={wi is not None} b={bi is not None}")
    ref, tol = layernorm_stats_bound(x, 1e-5)
    assert_within(rs, ref, tol, f"emulated layernorm (mean, rstd) C={C} mean {mean} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [2048, 4096])
def test_layernorm_fault_last_chunk_missing(C, dtype):
    x, w, b = _ln_inputs(64, C, dtype, spike=0.0)
    ref, tol = layernorm_bound(x, w, b, 1e-5)
    y, rs = _emulate_ln(x, w, b, 1e-5, fault="chunk")
    assert rel(y, ref) < 1e-2
    _rejected(y, ref, tol, f"layernorm C={C} {dtype}: last chunk missing from the sums")
    ref, tol = layernorm_stats_bound(x, 1e-5)
    _rejected(rs, ref, tol, f"layernorm (mean, rstd) C={C} {dtype}: last chunk missing from the sums")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [72, 2048])
def test_layernorm_fault_one_pass_variance(C, dtype):
    """E[x^2] - mean^2 in fp32 on rows of mean 200, spread 0.5: x^2 = 4e4 carries 2.4e-3 of rounding each against
    a variance of 0.25."""
    x, w, b = _ln_inputs(64, C, dtype, mean=200.0, spread=0.5, spike=0.0)
    ref, tol = layernorm_bound(x, w, b, 1e-5)
    y, rs = _emulate_ln(x, w, b, 1e-5, fault="onepass")
    assert rel(y, ref) < 1e-2
    _rejected(y, ref, tol, f"layernorm C={C} {dtype}: one-pass variance")
    ref, tol = layernorm_stats_bound(x, 1e-5)
    _rejected(rs, ref, tol, f"layernorm (mean, rstd) C={C} {dtype}: one-pass variance")


def _partials(x, P):
    """fp64 (mean, M2) of the P groups of 80 columns of x [M, 80 P], as the fp32 tensor the kernel reads."""
    xg = x.double().reshape(x.shape[0], P, 80)
    m = xg.mean(-1)
    return torch.stack([m, ((xg - m[..., None]) ** 2).sum(-1)], -1).float()


def _emulate_rs_from_partials(part, eps, skip_last=False):
    n, mean, m2 = 80.0, part[:, 0, 0].clone(), part[:, 0, 1].clone()
    for c in range(1, part.shape[1] - (1 if skip_last else 0)):
        nn = n + 80.0
        d, f = part[:, c, 0] - mean, 80.0 / nn
        mean = mean + d * f
        m2 = m2 + part[:, c, 1] + d * d * n * f
        n = nn
    return torch.stack([mean, torch.rsqrt(m2 / n + eps)], -1)


@pytest.mark.parametrize("P", [1, 2, 3, 8, 18])
@pytest.mark.parametrize("mean", [0.5, 40.0])
def test_rs_from_partials_emulation_and_fault(P, mean):
    x, _, _ = _ln_inputs(65, 80 * P, torch.bfloat16, mean=mean)
    part = _partials(x, P)
    ref, tol = rs_from_partials_bound(part, 1e-5)
    assert_within(_emulate_rs_from_partials(part, 1e-5), ref, tol, f"emulated rs from {P} partials, mean {mean}")
    full, _ = layernorm_stats_bound(x, 1e-5)
    assert (ref - full).abs().max().item() < 1e-4 * max(1.0, mean)       # the partials stand for the whole row
    if P > 2 and mean == 40.0:                   # from 3 partials on the skipped one stays under the norm threshold
        bad = _emulate_rs_from_partials(part, 1e-5, skip_last=True)
        assert rel(bad, ref) < 1e-2
        _rejected(bad, ref, tol, f"rs from {P} partials: last one skipped")


@pytest.mark.parametrize("dtype", DTYPES)
def test_affine_layernorm_emulation_and_fault(dtype):
    N, HW, C = 3, 35, 1280
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(N, HW, C, generator=g) * 2 + 0.5).to(dtype)
    co = (torch.randn(N, 2 * C, generator=g) * 0.05).to(dtype)
    sc, sh = co[:, :C], co[:, C:]

    def emulate(fault):
        a = (1.0 + sc.float())[:, None, :].expand(N, HW, C).clone()
        if fault:
            a[1:, 0] = (1.0 + sc.float())[:-1]                      # the first row of image n takes image n - 1's scale
        xa = torch.addcmul(sh.float()[:, None, :], x.float(), a).to(dtype)
        return xa, _emulate_ln(xa.reshape(-1, C), None, None, 1e-6)[0].reshape(N, HW, C)

    xa, y = emulate(False)
    xa_ref, xa_tol, y_ref, y_tol = affine_layernorm_bound(x, sc, sh, 1.0, 1e-6, xa)
    assert_within(xa, xa_ref, xa_tol, f"emulated affine layernorm xa {dtype}")
    assert_within(y, y_ref, y_tol, f"emulated affine layernorm y {dtype}")
    xa, y = emulate(True)
    assert rel(xa, xa_ref) < 1e-2
    _rejected(xa, xa_ref, xa_tol, f"affine layernorm {dtype}: one row with the previous image's scale")


# ------------------------------------------------------------------------------------------------ depthwise conv
def _dw_inputs(N, H, W, C, k, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, H, W, C, generator=g) + 0.5).to(dtype)
    w = (torch.randn(k * k, C, generator=g) / k).to(dtype)
    return x, w, torch.randn(C, generator=g).to(dtype)


def _emulate_dw(x, w, b, k, replicate):
    C = x.shape[-1]
    xp = F.pad(x.float().permute(0, 3, 1, 2), (k // 2,) * 4, mode="replicate" if replicate else "constant")
    y = F.conv2d(xp, w.float().t().reshape(C, 1, k, k), None if b is None else b.float(), 1, 0, 1, C)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("replicate", [False, True])
def test_dwconv_emulation_within_bound(k, replicate, dtype):
    x, w, b = _dw_inputs(2, 5, 6, 64, k, dtype)
    for bias in (b, None):
        ref, tol = dwconv_bound(x, w, bias, k, replicate)
        y = _emulate_dw(x, w, bias, k, replicate).to(dtype)
        assert_within(y, ref, tol, f"emulated dwconv k={k} replicate={replicate} bias={bias is not None} {dtype}")
    ref, tol = layernorm_stats_bound(y.reshape(-1, 64), 1e-6)
    rs = _emulate_ln(y.reshape(-1, 64), None, None, 1e-6)[1]
    assert_within(rs, ref, tol, f"emulated dwconv row statistics {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_dwconv_fault_border_tap_replicated(dtype):
    """Tap (-1, -1) of output pixel (0, 0) of the last image reads pixel (0, 0) instead of zero."""
    x, w, b = _dw_inputs(3, 24, 24, 64, 3, dtype)
    ref, tol = dwconv_bound(x, w, b, 3, False)
    y = _emulate_dw(x, w, b, 3, False)
    y[-1, 0, 0] += x[-1, 0, 0].float() * w[0].float()
    assert rel(y.to(dtype), ref) < 1e-2
    _rejected(y.to(dtype), ref, tol, f"dwconv {dtype}: one border tap replicated")


# ------------------------------------------------------------------------------------------------ softmax2
def _sm2_inputs(rows, cols, seed=0):
    """Rows of 6 randn in log2 units: a spike in the last column, a constant row, a row with -inf entries, a row
    of magnitude 1e4."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * 6
    x[:, -1] += 30
    x[0] = 3.0
    x[1, ::2] = -math.inf
    x[2] = torch.randn(cols, generator=g) * 1e4
    x[3] = 1e4 + torch.randn(cols, generator=g)
    return x


def _emulate_sm2(x, drop=0):
    p = torch.exp2(x - x.amax(-1, keepdim=True))
    s = (p[:, :-drop] if drop else p).sum(-1, keepdim=True)
    return (p * (1.0 / s)).to(BF)


@pytest.mark.parametrize("cols", [4, 1020, 4100])
def test_softmax2_emulation_within_bound(cols):
    x = _sm2_inputs(37, cols)
    ref, tol = softmax2_bound(x)
    y = _emulate_sm2(x)
    assert_within(y, ref, tol, f"emulated softmax2 cols={cols}")
    assert bool((tol[1, ::2] == 0).all()) and bool((y[1, ::2] == 0).all())
    y[1, 0] = 1e-30                                                 # a -inf input must give exactly 0
    _rejected(y, ref, tol, f"softmax2 cols={cols}: a masked entry not 0")


def test_softmax2_fault_normaliser_tail_dropped():
    """The last 4 of 1020 columns, which hold 0.8 % of each row's mass, missing from the normaliser."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(37, 1020, generator=g) * 0.25
    x[:, -4:] += 1.0
    ref, tol = softmax2_bound(x)
    assert_within(_emulate_sm2(x), ref, tol, "emulated softmax2 1020")
    y = _emulate_sm2(x, drop=4)
    assert rel(y, ref) < 1e-2
    _rejected(y, ref, tol, "softmax2: the last 4 columns missing from the normaliser")


# ------------------------------------------------------------------------------------------------ GRN
ALL_DTYPES = [torch.float32, torch.bfloat16, torch.float16]
GELU_C = (-2.301121339e+00, -1.067757240e-01, 1.014263055e-03)        # kGeluC0 .. 2 (csrc/kernels/common.h)


def _gelu_sig(x):
    """gelu_sig2 in fp32: x * rcp(1 + exp2(xc * q(xc^2))), xc = x clamped to +-8."""
    xc = x.clamp(-8.0, 8.0)
    x2 = xc * xc
    q = (x2 * GELU_C[2] + GELU_C[1]) * x2 + GELU_C[0]
    return x * (1.0 / (torch.exp2(xc * q) + 1.0))


def _grn_parts(x, N, HW, C):
    """fp32 block sums of squares over 64 rows, as the GELU GEMM's epilogue leaves them: [N, HW / 64, C]."""
    return x.float().pow(2).reshape(N, HW // 64, 64, C).sum(2)


def _emulate_grn(x, gamma, beta, pre_gelu, fault=None, part=None):
    """cgs_grn_nhwc_v2 in fp32: per slice, four row groups each adding every fourth row, merged as a tree; the
    finalize loop over S / 4 groups of four slices; sqrt; block sums of 256 channels; inv = 1 / (sum / C + 1e-6);
    y = beta + a * (1 + gamma * (gx * inv)). part: the GNS form, four chains over the given partials. Faults: 'nx1',
    'inv0' image 0's inv for all, 'row' the last row of the last slice dropped, 'bsum' the last block sum dropped,
    'gns' the last partial dropped, 'gelu_stats' the GELU in the apply pass only. Returns (y, gx, bsum)."""
    N, HW, C = x.shape
    xf = x.float()
    a = _gelu_sig(xf) if pre_gelu else xf
    st = xf if fault == "gelu_stats" else a
    if part is None:
        S = grn_slices(N, HW, C)
        rp = (HW + S - 1) // S
        parts = []
        for sl in range(S):
            r0, r1 = sl * rp, min(HW, sl * rp + rp)
            if fault == "row" and r1 == HW and r0 < r1:
                r1 -= 1
            rg = []
            for g in range(4):
                acc = torch.zeros(N, C)
                for r in range(r0 + g, r1, 4):
                    acc = acc + st[:, r] * st[:, r]
                rg.append(acc)
            parts.append((rg[0] + rg[1]) + (rg[2] + rg[3]))
        ss = torch.zeros(N, C)
        for q in range(S // 4):
            ss = ss + ((parts[4 * q] + parts[4 * q + 1]) + (parts[4 * q + 2] + parts[4 * q + 3]))
    else:
        nbk = part.shape[1] - (1 if fault == "gns" else 0)
        ch = [torch.zeros(N, C) for _ in range(4)]
        b = 0
        while b + 4 <= nbk:
            for j in range(4):
                ch[j] = ch[j] + part[:, b + j]
            b += 4
        for bb in range(b, nbk):
            ch[0] = ch[0] + part[:, bb]
        ss = (ch[0] + ch[1]) + (ch[2] + ch[3])
    gx = ss.sqrt()
    nblk = (C + 255) // 256
    bsum = torch.stack([gx[:, i * 256:(i + 1) * 256].sum(1) for i in range(nblk)], 1)
    used = bsum[:, :-1] if fault == "bsum" else bsum
    inv = 1.0 / (used.sum(1) / C + 1e-6)
    if fault == "inv0":
        inv = inv[:1].expand(N)
    nx = torch.ones(N, C) if fault == "nx1" else gx * inv[:, None]
    y = beta.float() + a * (1.0 + gamma.float() * nx)[:, None, :]
    return y.to(x.dtype), gx, bsum


def test_grn_tables_name_the_form_that_runs():
    """grn_slices and the row-tiled predicate at the table's shapes; nx of the structured input spans [0, 5]."""
    assert _gelu_sig(torch.zeros(3)).abs().max().item() == 0.0
    assert {k: grn_slices(*k) for k in GRN_V2_SHAPES} == {(1, 1, 8): 4, (5, 35, 264): 4, (64, 17, 72): 4,
                                                         (3, 33, 2056): 4, (2, 17, 2048): 4, (2, 16, 1640): 4,
                                                         (2, 33, 3688): 4, (1, 70, 1632): 8}
    assert grn_slices(4, 4096, 1536) == 44 and grn_slices(2, 576, 8192) == 16
    for (N, HW, C), form in GRN_V2_SHAPES.items():
        assert ("rows" if grn_row_tiled(HW, C) else "grid") == form, (N, HW, C)
        assert not grn_row_tiled(HW, C, rows=0)
    assert not grn_row_tiled(35, 2056)           # the case test_grn_apply_row_tiled_matches_grid_stride cannot tell
    for N, HW, C in list(GRN_V2_SHAPES) + GRN_GNS_SHAPES + [(65, 17, 72), (3, 35, 264)]:
        for dtype in DTYPES:
            x, gamma, beta, (cz, cn) = grn_inputs(N, HW, C, dtype)
            for pre_gelu in (False, True):
                nx = grn_nx(x, pre_gelu)
                assert nx.min().item() == 0.0 and nx.max().item() >= 5.0, (N, HW, C, dtype, pre_gelu, nx.max())
            assert bool((x[:, :, cz] == 0).all()) and x[:, :, cn].max().item() <= -6.0
            if N > 1:
                inv = 1 / (x.double().pow(2).sum(1).sqrt().mean(1) + 1e-6)
                assert (inv.max() / inv.min()).item() > 20


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pre_gelu", [False, True])
@pytest.mark.parametrize("N,HW,C", list(GRN_V2_SHAPES))
def test_grn_emulation_within_bound(N, HW, C, pre_gelu, dtype):
    x, gamma, beta, _ = grn_inputs(N, HW, C, dtype)
    y, gx, bsum = _emulate_grn(x, gamma, beta, pre_gelu)
    what = f"emulated grn {N}x{HW}x{C} gelu={pre_gelu} {dtype}"
    depth = grn_depth("v2", N, HW, C)
    ref, tol = grn_bound(x, gamma, beta, pre_gelu, depth)
    assert_within(y, ref, tol, what)
    gref, gtol, iref, itol = grn_stats_bound(x, pre_gelu, depth)
    assert_within(gx, gref, gtol, what + " gx")
    assert_within(1 / (bsum.double().sum(1) / C + 1e-6), iref, itol, what + " inv")
    ref, tol = grn_apply_bound(x, gamma, beta, gx, bsum, pre_gelu)
    assert_within(y, ref, tol, what + " apply")
    if not pre_gelu:                                  # the atomics of v1 in any order: the looser depth holds too
        ref, tol = grn_bound(x, gamma, beta, False, grn_depth("v1", N, HW, C))
        assert_within(y, ref, tol, what + " at the depth of v1")
    # the exact rounding of the reference uses the store term almost in full and no more
    ref, tol = grn_bound(x, gamma, beta, pre_gelu, depth)
    worst = assert_within(ref.to(dtype), ref, tol, what + " rounded reference")
    assert worst <= 1.0


@pytest.mark.parametrize("N,HW,C", GRN_GNS_SHAPES)
def test_grn_gns_emulation_and_scale_weight(N, HW, C):
    x, gamma, beta, _ = grn_inputs(N, HW, C, BF)
    part = _grn_parts(x, N, HW, C)
    y, gx, bsum = _emulate_grn(x, gamma, beta, False, part=part)
    depth = grn_depth("gns", N, HW, C)
    gref, gtol, iref, itol = grn_stats_bound(None, False, depth, part=part)
    assert_within(gx, gref, gtol, f"emulated grn gns {N}x{HW}x{C} gx")
    assert_within(1 / (bsum.double().sum(1) / C + 1e-6), iref, itol, f"emulated grn gns {N}x{HW}x{C} inv")
    ref, tol = grn_apply_bound(x, gamma, beta, gx, bsum)
    assert_within(y, ref, tol, f"emulated grn gns {N}x{HW}x{C} apply")
    # against x itself the torch block sums add 64 + 1 roundings in unknown order to the depth
    gref, gtol, _, _ = grn_stats_bound(x, False, (depth[0] + 65, depth[1]))
    assert_within(gx, gref, gtol, f"emulated grn gns {N}x{HW}x{C} gx against x")
    bad = _emulate_grn(x, gamma, beta, False, fault="gns", part=part)
    gref, gtol, iref, itol = grn_stats_bound(None, False, depth, part=part)
    _rejected(bad[1], gref, gtol, f"grn gns {N}x{HW}x{C}: last partial dropped, gx")
    ref, tol = grn_bound(x, gamma, beta, False, (depth[0] + 65, depth[1]))
    assert_within(y, ref, tol, f"emulated grn gns {N}x{HW}x{C} against x")
    _rejected(bad[0], ref, tol, f"grn gns {N}x{HW}x{C}: last partial dropped, y")
    # the weight-folding consumer
    O = 24
    W = torch.randn(O, C, generator=torch.Generator().manual_seed(1)).to(BF)
    inv = 1.0 / (bsum.sum(1) / C + 1e-6)
    Wn = (W.float()[None] * (1.0 + gamma.float()[None, None] * gx[:, None] * inv[:, None, None])).to(BF)
    ref, tol = grn_scale_weight_bound(W, gamma, gx, 1 / (bsum.double().sum(1) / C + 1e-6))
    assert_within(Wn, ref, tol, f"emulated grn_scale_weight {N}x{O}x{C}")
    Wn[1:] = (W.float()[None] * (1.0 + gamma.float()[None, None] * gx[1:, None] * inv[:1, None, None])).to(BF)
    _rejected(Wn, ref, tol, f"grn_scale_weight {N}x{O}x{C}: image 0's normaliser for all")


# fault -> (iid shape at which the old check accepts it, structured shape at which the bound rejects it)
GRN_FAULTS = {"nx1": ((2, 4096, 264), (5, 35, 264)), "inv0": ((3, 1024, 264), (5, 35, 264)),
              "row": ((3, 1024, 264), (5, 35, 264)), "bsum": ((2, 256, 1544), (5, 35, 264)),
              "gns": ((2, 1024, 264), (5, 320, 264)), "gelu_stats": ((2, 4096, 264), (5, 35, 264))}


@pytest.mark.parametrize("fault", list(GRN_FAULTS))
def test_grn_faults(fault):
    """Each fault is under the Frobenius threshold of the older tests on their iid inputs and rejected on the
    structured ones."""
    pre_gelu = fault == "gelu_stats"
    (N, HW, C), small = GRN_FAULTS[fault]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, HW, C, generator=g).to(BF)
    gamma, beta = (torch.randn(C, generator=g) * 0.5).to(BF), (torch.randn(C, generator=g) * 0.1).to(BF)
    part = _grn_parts(x, N, HW, C) if fault == "gns" else None
    y = _emulate_grn(x, gamma, beta, pre_gelu, fault=fault, part=part)[0]
    xd = F.gelu(x.double()) if pre_gelu else x.double()
    ref = beta.double() + xd * (1 + gamma.double() * grn_nx(x, pre_gelu))[:, None, :]
    old = rel(y, ref)
    print(f"grn fault {fault}: Frobenius rel {old:.2e} on iid {N}x{HW}x{C}")
    assert old < 1e-2
    N, HW, C = small
    for dtype in DTYPES:
        x, gamma, beta, _ = grn_inputs(N, HW, C, dtype)
        part = _grn_parts(x, N, HW, C) if fault == "gns" else None
        L, Lm = grn_depth("gns" if part is not None else "v2", N, HW, C)
        ref, tol = grn_bound(x, gamma, beta, pre_gelu, (L + 65 if part is not None else L, Lm))
        y, gx, bsum = _emulate_grn(x, gamma, beta, pre_gelu, part=part)
        assert_within(y, ref, tol, f"emulated grn {N}x{HW}x{C} {dtype}")
        y, gx, bsum = _emulate_grn(x, gamma, beta, pre_gelu, fault=fault, part=part)
        _rejected(y, ref, tol, f"grn {N}x{HW}x{C} {dtype}: fault {fault}")
        if fault in ("nx1", "inv0"):                  # faults of the apply pass: the statistics it was given are right
            ref, tol = grn_apply_bound(x, gamma, beta, gx, bsum, pre_gelu)
            _rejected(y, ref, tol, f"grn apply {N}x{HW}x{C} {dtype}: fault {fault}")
        if fault in ("row", "gelu_stats"):
            gref, gtol, _, _ = grn_stats_bound(x, pre_gelu, (L, Lm))
            _rejected(gx, gref, gtol, f"grn gx {N}x{HW}x{C} {dtype}: fault {fault}")


def _no_effect(bad, good):
    """A fault that cannot show in this configuration: the same values up to fp32 rounding."""
    return (bad.double() - good.double()).abs().max().item() <= 1e-5 * good.double().abs().max().item()


# ------------------------------------------------------------------------------------------------ upfirdn2d
def _emulate_upfirdn(x, k, up, down, pad, fault=None):
    """The gather form of upfirdn2d_kernel in fp32. Faults: 'noflip', 'kt' the tap row stride kh instead of kw,
    'pad' px0 / py0 swapped, 'up' up_x / up_y swapped."""
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad
    N, C, H, W = x.shape
    kh, kw = k.shape
    Ho, Wo = (H * uy + py0 + py1 - kh) // dy + 1, (W * ux + px0 + px1 - kw) // dx + 1
    if fault == "pad":
        px0, py0 = py0, px0
    if fault == "up":
        ux, uy = uy, ux
    xf, taps = x.float(), k.float().reshape(-1)
    oy, ox = torch.arange(Ho)[:, None], torch.arange(Wo)[None, :]
    acc = torch.zeros(N, C, Ho, Wo)
    for i in range(kh):
        vy = oy * dy + i - py0
        for j in range(kw):
            vx = ox * dx + j - px0
            ok = (vy >= 0) & (vy % uy == 0) & (vy // uy < H) & (vx >= 0) & (vx % ux == 0) & (vx // ux < W)
            iy, ix = (vy // uy).clamp(0, H - 1).expand(Ho, Wo), (vx // ux).clamp(0, W - 1).expand(Ho, Wo)
            t = i * kw + j if fault == "noflip" else (kh - 1 - i) * (kh if fault == "kt" else kw) + (kw - 1 - j)
            acc = acc + torch.where(ok, xf[:, :, iy, ix], torch.zeros(())) * taps[t]
    return acc.to(x.dtype)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("kname", list(UPFIRDN_KERNELS))
def test_upfirdn2d_emulation_and_faults(kname, dtype):
    x = torch.randn(2, 3, 9, 6, generator=torch.Generator().manual_seed(0)).to(dtype)
    k = upfirdn_kernel(*UPFIRDN_KERNELS[kname])
    seen = set()
    for up, down, pad in UPFIRDN_CFGS:
        ref, tol = upfirdn2d_bound(x, k, up, down, pad)
        what = f"upfirdn2d {kname} up={up} down={down} pad={pad} {dtype}"
        assert_within(_emulate_upfirdn(x, k, up, down, pad), ref, tol, "emulated " + what)
        for fault in ("noflip", "kt", "pad", "up"):
            if ((fault == "kt" and 1 in k.shape)     # a 1 x n or n x 1 kernel: the row stride never matters
                    or (fault == "pad" and pad[0] == pad[2]) or (fault == "up" and up[0] == up[1])):
                continue
            bad = _emulate_upfirdn(x, k, up, down, pad, fault)
            if _no_effect(bad, _emulate_upfirdn(x, k, up, down, pad)):
                continue                              # up 2, down 2 and an odd pad under a 1-row kernel: all zero
            _rejected(bad, ref, tol, what + f": fault {fault}")
            seen.add(fault)
    assert seen >= ({"noflip", "pad", "up"} | ({"kt"} if kname == "3x5" else set()))


# ------------------------------------------------------------------------------------------------ fused_bias_act
@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("shape", FBA_SHAPES)
def test_fused_bias_act_emulation_and_fault(shape, dtype):
    g = torch.Generator().manual_seed(0)
    x, b = torch.randn(*shape, generator=g).to(dtype), torch.randn(shape[1], generator=g).to(dtype)
    C, inner = shape[1], math.prod(shape[2:])
    for slope in (0.2, 0.0):
        for bias in (b, None):
            ref, tol = fused_bias_act_bound(x, bias, slope, 2 ** 0.5)
            i = torch.arange(x.numel())
            for fault in (False, True):
                v = x.float().reshape(-1)
                if bias is not None:
                    v = v + bias.float()[(i % C) if fault else (i // inner) % C]
                y = (torch.where(v >= 0, v, v * torch.tensor(slope)) * torch.tensor(2 ** 0.5)).to(dtype).reshape(shape)
                what = f"fused_bias_act {shape} slope={slope} bias={bias is not None} {dtype}"
                if not fault:
                    assert_within(y, ref, tol, "emulated " + what)
                elif bias is not None and inner > 1:
                    _rejected(y, ref, tol, what + ": bias index i % C")


# ------------------------------------------------------------------------------------------------ resize
def _emulate_resize(x, size, mode, align, fault=None):
    """resize_kernel in fp32. Faults: 'nohalf' bilinear without the half-pixel offset, 'noclamp' bicubic taps
    outside the image read as 0 instead of the border pixel, 'floor' the area window's end floored."""
    N, C, H, W = x.shape
    Ho, Wo = size
    xf = x.float()
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
    interp = mode in ("bilinear", "bicubic")

    def scale(n_in, n_out):
        if align and interp:
            return f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
        return f32(n_in) / f32(n_out)

    oy, ox, sh, sw = torch.arange(Ho).float(), torch.arange(Wo).float(), scale(H, Ho), scale(W, Wo)
    if not interp and mode != "area":
        off = 0.5 if mode == "nearest-exact" else 0.0
        iy = torch.floor((oy + off) * sh).long().clamp_max(H - 1)
        ix = torch.floor((ox + off) * sw).long().clamp_max(W - 1)
        return xf[:, :, iy][:, :, :, ix].to(x.dtype)
    if mode == "bilinear":
        half = not align and fault != "nohalf"
        fy = ((oy + 0.5) * sh - 0.5).clamp_min(0) if half else oy * sh
        fx = ((ox + 0.5) * sw - 0.5).clamp_min(0) if half else ox * sw
        y0, x0 = fy.long().clamp_max(H - 1), fx.long().clamp_max(W - 1)
        y1, x1 = y0 + (y0 < H - 1), x0 + (x0 < W - 1)
        ly, lx = (fy - y0)[:, None], fx - x0
        px = lambda yy, xx: xf[:, :, yy][:, :, :, xx]
        v = (1 - ly) * ((1 - lx) * px(y0, x0) + lx * px(y0, x1)) + ly * ((1 - lx) * px(y1, x0) + lx * px(y1, x1))
        return v.to(x.dtype)
    if mode == "bicubic":
        A = -0.75
        c1 = lambda t: ((A + 2) * t - (A + 3)) * t * t + 1
        c2 = lambda t: ((A * t - 5 * A) * t + 8 * A) * t - 4 * A
        fy = oy * sh if align else (oy + 0.5) * sh - 0.5
        fx = ox * sw if align else (ox + 0.5) * sw - 0.5
        iy, ix = torch.floor(fy), torch.floor(fx)
        ty, tx = fy - iy, fx - ix
        wy, wx = [c2(ty + 1), c1(ty), c1(1 - ty), c2(2 - ty)], [c2(tx + 1), c1(tx), c1(1 - tx), c2(2 - tx)]
        v = torch.zeros(N, C, Ho, Wo)
        for a in range(4):
            yy = iy.long() - 1 + a
            row = torch.zeros(N, C, Ho, Wo)
            for b in range(4):
                xx = ix.long() - 1 + b
                p = xf[:, :, yy.clamp(0, H - 1)][:, :, :, xx.clamp(0, W - 1)]
                if fault == "noclamp":
                    inside = ((yy >= 0) & (yy < H))[:, None] & ((xx >= 0) & (xx < W))[None, :]
                    p = torch.where(inside, p, torch.zeros(()))
                row = row + wx[b] * p
            v = v + wy[a][:, None] * row
        return v.to(x.dtype)
    v = torch.zeros(N, C, Ho, Wo)
    for o in range(Ho):
        y0, y1 = o * H // Ho, -((-(o + 1) * H) // Ho)
        if fault == "floor":
            y1 = max((o + 1) * H // Ho, y0 + 1)
        for q in range(Wo):
            x0, x1 = q * W // Wo, -((-(q + 1) * W) // Wo)
            if fault == "floor":
                x1 = max((q + 1) * W // Wo, x0 + 1)
            s = torch.zeros(N, C)
            for yy in range(y0, y1):
                for xx in range(x0, x1):
                    s = s + xf[:, :, yy, xx]
            v[:, :, o, q] = s / f32((y1 - y0) * (x1 - x0))
    return v.to(x.dtype)


def test_resize_sizes_have_no_floor_ambiguity():
    """No source coordinate of the listed sizes lies within 1e-4 of an integer unless it is exactly one, and those
    that are floor to it in fp32 as well."""
    from fractions import Fraction
    import numpy as np
    for (_, _, H, W), (Ho, Wo) in RESIZE_CASES:
        for n_in, n_out in ((H, Ho), (W, Wo)):
            for mode, align in RESIZE_MODES:
                if mode == "area":
                    continue
                c = resize_coords(n_in, n_out, mode, bool(align))
                for o in range(n_out):
                    if align and mode in ("bilinear", "bicubic"):
                        ex = Fraction(o) * (Fraction(n_in - 1, n_out - 1) if n_out > 1 else 0)
                        sc = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
                        f = np.float32(o) * sc
                    else:
                        off = Fraction(0) if mode == "nearest" else Fraction(1, 2)
                        ex = (o + off) * Fraction(n_in, n_out) - (0 if mode.startswith("nearest") else Fraction(1, 2))
                        f = (np.float32(o) + np.float32(float(off))) * (np.float32(n_in) / np.float32(n_out))
                        f = f if mode.startswith("nearest") else f - np.float32(0.5)
                    assert abs(float(ex) - c[o].item()) < 1e-12
                    if ex.denominator == 1:
                        if mode.startswith("nearest"):
                            assert int(np.floor(f)) == int(ex), (n_in, n_out, mode, o, f)
                    else:
                        assert abs(ex - round(ex)) >= Fraction(1, 10000), (n_in, n_out, mode, align, o)


def _resize_x(shape, dtype):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(0)) * 2 + 0.5).to(dtype)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("mode,align", RESIZE_MODES)
def test_resize_emulation_within_bound(mode, align, dtype):
    for shape, size in RESIZE_CASES:
        x = _resize_x(shape, dtype)
        ref, tol = resize_bound(x, size, mode, align)
        y = _emulate_resize(x, size, mode, align)
        assert_within(y, ref, tol, f"emulated resize {mode} align={align} {shape}->{size} {dtype}")
        if mode.startswith("nearest"):
            assert bool((tol == 0).all())
        else:                                     # the fp64 weights are those of F.interpolate
            kw = {"align_corners": align} if align is not None else {}
            want = F.interpolate(x.double(), size=size, mode=mode, **kw)
            assert (ref - want).abs().max().item() < 1e-9


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("mode,fault", [("bilinear", "nohalf"), ("bicubic", "noclamp"), ("area", "floor")])
def test_resize_faults(mode, fault, dtype):
    align = None if mode == "area" else False
    hit = 0
    for shape, size in RESIZE_CASES:
        x = _resize_x(shape, dtype)
        ref, tol = resize_bound(x, size, mode, align)
        y = _emulate_resize(x, size, mode, align, fault)
        if _no_effect(y, _emulate_resize(x, size, mode, align)):
            continue                              # e.g. the same size: no offset, no border tap, no partial window
        _rejected(y, ref, tol, f"resize {mode} {shape}->{size} {dtype}: fault {fault}")
        hit += 1
    assert hit >= 4


# ------------------------------------------------------------------------------------------------ softmax_rows
def _emulate_smr(x, scale, tail=True):
    s = x.float() * scale
    n = s.shape[-1] if tail else 64 * (s.shape[-1] // 64)
    mx = s[:, :n].amax(-1, keepdim=True)
    p = torch.exp(s - mx)
    return p * (1.0 / p[:, :n].sum(-1, keepdim=True))


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("cols", SMR_COLS)
def test_softmax_rows_emulation_and_fault(cols, dtype):
    for rows in SMR_ROWS:
        for scale in (0.125, 1.0):
            x = smr_inputs(rows, cols, dtype)
            ref, tol = softmax_rows_bound(x, scale)
            what = f"softmax_rows {rows}x{cols} scale={scale} {dtype}"
            assert_within(_emulate_smr(x, scale), ref, tol, "emulated " + what)
            if cols > 64 and cols % 64:
                _rejected(_emulate_smr(x, scale, tail=False), ref, tol, what + ": lane tail ignored")


# ------------------------------------------------------------------------------------------------ tome_match
def _emulate_tome(a, b, k_tail=True, high_tie=False):
    C = a.shape[-1] if k_tail else 32 * (a.shape[-1] // 32)
    af, bf = a.float(), b.float()
    inv = lambda t: torch.where(t.pow(2).sum(-1) > 0, torch.rsqrt(t.pow(2).sum(-1)), torch.zeros(()))
    s = (af[..., :C] @ bf[..., :C].transpose(-1, -2)) * inv(af)[..., :, None] * inv(bf)[..., None, :]
    v = s.amax(-1)
    hit = s == v[..., None]
    n = s.shape[-1]
    idx = (n - 1 - hit.flip(-1).double().argmax(-1)) if high_tie else hit.double().argmax(-1)
    return v, idx


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,Na,Nb,C", TOME_SHAPES)
def test_tome_emulation_and_faults(B, Na, Nb, C, dtype):
    a, b = tome_inputs(B, Na, Nb, C, dtype)
    assert a.stride(1) == C + 24 and b.stride(1) == C + 24
    what = f"tome_match {B}x{Na}x{Nb}x{C} {dtype}"
    v, idx = _emulate_tome(a, b)
    assert_tome(v, idx, a, b, "emulated " + what)
    if Na > 1:
        assert bool((v[:, -1] == 0).all()) and bool((idx[:, 0] == 0).all())
    if C % 32:
        with pytest.raises(AssertionError, match="over tol"):
            assert_tome(*_emulate_tome(a, b, k_tail=False), a, b, what + ": k tail ignored")
    if Nb > 1:
        with pytest.raises(AssertionError, match="higher index"):
            assert_tome(*_emulate_tome(a, b, high_tie=True), a, b, what + ": ties to the higher index")


# ------------------------------------------------------------------------------------------------ fused epilogues
# a / b of act_family (csrc/kernels/common.h): -c0 log2 e, -c1 log2 e of x sigmoid(x (c0 + c1 x^2))
ACT_AB = {"gelu_tanh": (-2.302208198e+00, -1.029432396e-01), "quick_gelu": (-2.455466953e+00, 0.0),
          "silu": (-1.442695041e+00, 0.0)}
ACT_CASES = [(None, 0.0), ("gelu", 0.0), ("gelu_tanh", 0.0), ("quick_gelu", 0.0), ("silu", 0.0), ("relu", 0.0),
             ("leaky_relu", 0.2), ("leaky_relu", -0.3)]


def _emulate_act(x, act, param=0.0):
    """act_fam in fp32: gelu_sig; x * rcp(1 + exp2(x * fma(x * x, b, a))); x >= 0 ? x : a * x."""
    if act is None:
        return x
    if act == "gelu":
        return _gelu_sig(x)
    if act in ACT_AB:
        a, b = ACT_AB[act]
        return x * (1.0 / (1.0 + torch.exp2(x * ((x * x) * b + a))))
    if act == "relu":
        return x.clamp_min(0.0)
    return torch.where(x >= 0, x, x * torch.tensor(param, dtype=torch.float32))


def _act_inputs(M, N, K, seed=0):
    """_gemm_inputs with eight pre-activation columns pushed to +-9 through the bias: the clamp of gelu_sig at +-8 and
    the saturated sigmoid."""
    a, w, b, r = _gemm_inputs(M, N, K, seed)
    b[:4], b[4:8] = 9.0, -9.0
    return a, w, b, r


def _emulate_gemm_act(a, w, b, r, act, param=0.0, two_roundings=True, after_res=False):
    """round(act(a w^T + b)) (+ r): the mc::tile kernels round, add r to the bf16 tile and round again; v6, skinny and
    the split-K reduce add r in fp32. after_res: the fault act(pre + r)."""
    pre = a.float() @ w.float().t() + b.float()
    if after_res:
        return _emulate_act(pre + r.float(), act, param).to(BF)
    y = _emulate_act(pre, act, param)
    if r is None:
        return y.to(BF)
    return (y.to(BF).float() + r.float()).to(BF) if two_roundings else (y + r.float()).to(BF)


@pytest.mark.parametrize("act,param", ACT_CASES)
@pytest.mark.parametrize("M,N,K", [(33, 40, 32), (129, 136, 192), (257, 168, 640)])
def test_gemm_act_emulation_within_bound(M, N, K, act, param):
    a, w, b, r = _act_inputs(M, N, K)
    pre = a.double() @ w.double().t() + b.double()
    assert bool((pre[:, :4] > 8).any()) and bool((pre[:, 4:8] < -8).any())      # both sides of gelu_sig's clamp
    for res in (None, r):
        ref, tol = gemm_act_bound(a, w, b, res, act, param)
        for two in ((False, True) if res is not None else (False,)):
            assert_within(_emulate_gemm_act(a, w, b, res, act, param, two), ref, tol,
                          f"emulated gemm {M}x{N}x{K} {act}({param}) res={res is not None} two roundings={two}")
    if act is None:                                          # the identity is gemm_bound's own case
        ref0, tol0 = gemm_bound(a, w, b, r)
        assert torch.equal(ref, ref0) and bool((tol >= tol0).all()) and bool((tol <= tol0 * 1.01).all())


def test_gemm_act_bound_lnfold_and_conv():
    """The two other pre-activations: the LayerNorm fold (rs / cs) and conv_bound's."""
    M, N, K = 70, 96, 128
    a, w, b, _ = _act_inputs(M, N, K, seed=1)
    x = (a.float() * 3 + 1.5).to(BF)
    rs = torch.stack([x.float().mean(1), torch.rsqrt(x.float().var(1, unbiased=False) + 1e-5)], 1)
    cs = w.float().sum(1)
    pre = rs[:, 1:2] * (x.float() @ w.float().t() - rs[:, :1] * cs[None]) + b.float()
    ref, tol = gemm_act_bound(x, w, b, None, "gelu", rs=rs, cs=cs)
    assert_within(_gelu_sig(pre).to(BF), ref, tol, "emulated lnfold + gelu")
    _rejected(pre.to(BF), ref, tol, "lnfold + gelu: activation skipped")
    ref0, tol0 = lnfold_bound(x, w, b, rs, cs)
    ref1, tol1 = gemm_act_bound(x, w, b, None, None, rs=rs, cs=cs)
    assert torch.equal(ref0, ref1) and bool((tol1 >= tol0).all())
    g, xc, x2, wc, bc = _conv_inputs(2, 24, 8, 9, 8, 24)
    bc[:2], bc[2:4] = 9.0, -9.0
    cat = torch.cat([xc, x2], 1).float()
    for act, param in ACT_CASES:
        for stride, up in ((1, False), (2, False), (1, True)):
            xin = F.interpolate(cat, scale_factor=2.0, mode="nearest") if up else cat
            pre = F.conv2d(xin, wc.float(), bc.float(), stride, 1)
            res = torch.randn(pre.shape, generator=g).to(BF) if not up else None
            y = _emulate_act(pre, act, param).to(BF)
            y = (y.float() + res.float()).to(BF) if res is not None else y
            ref, tol = conv_act_bound(xc, wc, bc, res, act, param, stride, 1, upsample2x=up, x2=x2)
            assert_within(y, ref, tol, f"emulated conv {act}({param}) s{stride} up={up}")
    ref, tol = conv_act_bound(xc, wc, bc, None, "leaky_relu", 0.2, 1, 1, x2=x2)
    _rejected(F.conv2d(cat, wc.float(), bc.float(), 1, 1).clamp_min(0).to(BF), ref, tol, "conv: leaky slope 0")
    ref0, tol0 = conv_bound(xc, wc, bc, None, 1, 1, x2=x2)                 # the identity is conv_bound's own case
    ref1, tol1 = conv_act_bound(xc, wc, bc, None, None, 0.0, 1, 1, x2=x2)
    assert torch.equal(ref0, ref1) and bool((tol1 >= tol0).all()) and bool((tol1 <= tol0 * 1.01).all())


SIG_SET = ["gelu", "gelu_tanh", "quick_gelu", "silu"]


@pytest.mark.parametrize("res", [False, True])
def test_gemm_act_faults(res):
    M, N, K = 257, 136, 96                                   # bm + 1, bn + 8 of the 256 x 128 tiles
    a, w, b, r = _act_inputs(M, N, K)
    r = r if res else None
    for want in SIG_SET:                                     # another member of the set, pairwise
        ref, tol = gemm_act_bound(a, w, b, r, want)
        for got in SIG_SET:
            if got != want:
                _rejected(_emulate_gemm_act(a, w, b, r, got), ref, tol, f"{want} asked, {got} applied")
    ref, tol = gemm_act_bound(a, w, b, r, "leaky_relu", 0.2)
    _rejected(_emulate_gemm_act(a, w, b, r, "relu"), ref, tol, "leaky_relu(0.2): slope 0")
    if res:
        for act, param in ACT_CASES[1:]:
            ref, tol = gemm_act_bound(a, w, b, r, act, param)
            _rejected(_emulate_gemm_act(a, w, b, r, act, param, after_res=True), ref, tol, f"{act} after the residual")
    # the same faults in the last row's last vector only: under the Frobenius-norm threshold of the older tests (the
    # two GELUs are within 5e-4 of each other, over a bf16 ulp only where -3 < x < -1.5: eight values need not hold one,
    # so that pair is judged on the whole matrix above; so is the activation after the residual, which moves eight
    # values of a matrix this small by enough to show in the norm)
    for want, param, got in [("quick_gelu", 0.0, "silu"), ("silu", 0.0, "gelu_tanh"), ("gelu_tanh", 0.0, "silu"),
                             ("gelu", 0.0, "quick_gelu"), ("leaky_relu", 0.2, "relu")]:
        ref, tol = gemm_act_bound(a, w, b, r, want, param)
        y = _emulate_gemm_act(a, w, b, r, want, param)
        y[-1, -8:] = _emulate_gemm_act(a, w, b, r, got)[-1, -8:]
        assert rel(y, ref) < 4e-3
        _rejected(y, ref, tol, f"{want} asked, {got} in the last vector of the last row")


# ---- row-statistics partials (pq::run RSO)
def _emulate_rowstats(y, shifted=True, drop_lane=False):
    """fp32 (mean, M2) [M, N / 80, 2] as the RSO epilogue forms them: per lane 20 values shifted by its first, five
    trees of four added in sequence, m2 = s2 - s1^2 / 20; then the merges with lane ^ 16 and lane ^ 32. Faults:
    shifted=False (sh = 0), drop_lane (lane 1's values never enter: lane 0 merges with itself)."""
    M, N = y.shape
    lv = y.float().reshape(M, N // 80, 80)[..., torch.tensor(RSO_LANE_COLS)]           # [M, P, 4, 20]
    sh = lv[..., :1] if shifted else torch.zeros_like(lv[..., :1])
    d = (lv - sh).reshape(M, N // 80, 4, 5, 4)
    s1, s2 = torch.zeros(M, N // 80, 4), torch.zeros(M, N // 80, 4)
    for j in range(5):
        d0, d1, d2, d3 = d[..., j, :].unbind(-1)
        s1 = s1 + ((d0 + d1) + (d2 + d3))
        s2 = s2 + ((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3))
    i20 = torch.tensor(1.0 / 20.0, dtype=torch.float32)
    mean, m2 = sh[..., 0] + s1 * i20, (s2 - s1 * s1 * i20).clamp_min(0.0)
    if drop_lane:
        mean[..., 1], m2[..., 1] = mean[..., 0], m2[..., 0]
    for n in (20.0, 40.0):
        ma, mb = mean[..., 0::2], mean[..., 1::2]
        dd = mb - ma
        mean, m2 = 0.5 * (ma + mb), m2[..., 0::2] + m2[..., 1::2] + dd * dd * (0.5 * n)
    return torch.cat([mean, m2], -1)


@pytest.mark.parametrize("mean", [0.5, 40.0])
@pytest.mark.parametrize("P", [2, 4])
def test_rowstats_partials_emulation_and_faults(P, mean):
    """With the +-48 spikes of _ln_inputs in the first and last column the first lane of a row is shifted by an outlier:
    its s2 is as large as an unshifted one and the bound says so. The unshifted fault is planted on the data without
    them, where the shift keeps s2 at the spread."""
    for spike in (SPIKE, 0.0):
        y, _, _ = _ln_inputs(65, 80 * P, BF, mean=mean, spike=spike)
        y[3] = y[3, 0]                                       # a row of identical values: M2 exact up to tiny
        y[4, :80] = y[4, 5]
        ref, tol = rowstats_partials_bound(y)
        assert bool((ref[3, :, 1] == 0).all()) and tol[3, :, 1].max().item() < 1e-37 and tol[4, 0, 1].item() < 1e-37
        assert (ref - _partials(y, P).double()).abs().max().item() < 1e-3 * max(1.0, mean)
        what = f"rowstats partials P={P} mean {mean} spike {spike}"
        part = _emulate_rowstats(y)
        assert_within(part, ref, tol, "emulated " + what)
        _rejected(part.flip(1), ref, tol, what + ": chunks swapped")
        _rejected(_emulate_rowstats(y, drop_lane=True), ref, tol, what + ": one lane left out of the merge")
        if mean == 40.0 and not spike:
            _rejected(_emulate_rowstats(y, shifted=False), ref, tol, what + ": unshifted one-pass M2")
    # the merged statistics: inside rs_from_partials_bound, and inside the row's own bound widened by the partials' tol
    rs = _emulate_rs_from_partials(part, 1e-5)
    r1, t1 = rs_from_partials_bound(part, 1e-5)
    assert_within(rs, r1, t1, what + ": rs from the emulated partials")
    r2, t2 = layernorm_stats_bound(y, 1e-5)
    assert_within(rs, r2, t2 + t1 + partials_merge_tol(ref, tol, 1e-5), what + ": rs against the row")


# ---- sum-of-squares and GroupNorm partials (pq::run GNS)
def _row16_sum(t):
    """row16_sum over dim -2 (16 lanes): quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror."""
    k = torch.arange(16)
    for perm in (k ^ 1, k ^ 2, (k & 8) | (7 - (k & 7)), 15 - k):
        t = t + t[..., perm, :]
    return t[..., 0, :]


def _emulate_block_stats(y, form, src=None, shift=0, extra=0):
    """The GNS epilogues on the stored y [M, N] (M % 64 == 0): a wave holds rows 16 i + fr of its 64 in NI = 4
    registers per column. form 'sumsq' [M / 64, N]; 'gn' (mean, M2) [M / 64, N, 2] in two passes. Faults: src (the
    statistics of other values than the stored ones), shift (every block but the last reads its rows shift rows
    later), extra (every block but the last also adds the next block's first rows)."""
    M, N = y.shape
    v = (y if src is None else src).float()
    rows = torch.arange(M).reshape(M // 64, 64)
    rows[:-1] += shift
    u = v[rows].reshape(M // 64, 4, 16, N)
    if form == "sumsq":
        q = torch.zeros(M // 64, 16, N)
        for i in range(4):
            q = q + u[:, i] * u[:, i]
        out = _row16_sum(q)
        if extra:
            out[:-1] += (v[rows[1:, :extra]] ** 2).sum(1)
        return out
    mu = u[:, 0]
    for i in range(1, 4):
        mu = mu + u[:, i]
    mu = _row16_sum(mu) * (1.0 / 64.0)
    if extra:
        mu[:-1] += v[rows[1:, :extra]].sum(1) / 64.0
    q = torch.zeros(M // 64, 16, N)
    for i in range(4):
        dx = u[:, i] - mu[:, None]
        q = q + dx * dx
    return torch.stack([mu, _row16_sum(q)], -1)


@pytest.mark.parametrize("form", ["sumsq", "gn"])
def test_block_partials_emulation_and_faults(form):
    images, hw, N, K = 5, 64, 24, 128                         # hw = 64: every block boundary is an image boundary
    M = images * hw
    a, w, b, _ = _gemm_inputs(M, N, K, seed=4)
    a = (a.float() * torch.linspace(0.25, 4.0, images).repeat_interleave(hw)[:, None]).to(BF)      # images differ
    acc = a.float() @ w.float().t() + b.float()
    acc = _gelu_sig(acc) if form == "sumsq" else acc
    acc[64:128, 5] = 0.0                                      # an all-zero block: exact
    y = acc.to(BF)
    if form == "sumsq":
        ref, tol = sumsq_partials_bound(y, hw)
        assert ref[1, 5].item() == 0 and tol[1, 5].item() == 0
        view = lambda t: t
    else:
        ref, tol = gn_partials_bound(y.reshape(images, 8, 8, N))
        view = lambda t: t.reshape(images, 1, N, 2)
    assert_within(view(_emulate_block_stats(y, form)), ref, tol, f"emulated {form} partials")
    for name, kw in [("a block read across the image boundary", dict(shift=16)),
                     ("rows of the next block included", dict(extra=16)),
                     ("statistics of the unrounded fp32 values", dict(src=acc))]:
        _rejected(view(_emulate_block_stats(y, form, **kw)), ref, tol, f"{form} partials: {name}")
