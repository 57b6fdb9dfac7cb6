"""Per-element error bounds (tests/_bounds.py) on the device for the fp32 kernels of csrc/kernels/f32.hip behind
``--fp32-vae`` / ``--force-fp32``: cgs_gemm_f32 (ops.linear and the raw batched launch of ops.f32.gemm), cgs_conv_f32,
cgs_groupnorm_f32, cgs_layernorm_f32 and the fp32 attention ops/f32.py composes from two batched GEMMs and
cgs_softmax_rows. References are fp64 on the device; every op call must count one ("...", "hip") and no "lib"
entry. The tile is 128 x 128 x 32 and the shapes are the smallest that reach each edge of the kernels and of the host
code (tests/_bounds.py: F32_LINEAR_SHAPES, F32_CONV_CASES, F32_GN_CASES); the inputs are mixed-scale with spikes of
+-48 where an index can go wrong. Outputs the caller owns are written inside guarded buffers: everything outside
them must keep its bits."""
import math

import pytest
import torch

from comfy_gen_server_amd import ops, _native
from comfy_gen_server_amd.ops import core, f32

from _bounds import (F32_ACTS, F32_CONV_CASES, F32_GN_CASES, F32_LINEAR_SHAPES, F32_LN_C, F32_LN_ROWS, assert_within,
                     attention_f32_bound, conv_bound, f32_attn_inputs, f32_conv_inputs, f32_gemm_inputs, f32_gn_inputs,
                     f32_ln_inputs, gemm_act_bound, gemm_bound, gn_f32_form, groupnorm_f32_bound, layernorm_bound,
                     ln_f32_depth)
from _guards import GUARD, _check_guard, _guarded32, _native_loaded, _ran_native  # noqa: F401

pytestmark = pytest.mark.gpu
FP = torch.float32
CL = torch.channels_last


def _guarded_out(cuda, rows, ld):
    """A [rows, ld] fp32 tensor inside a guarded int32 buffer: (buf, before, tensor)."""
    buf, before, ptr = _guarded32(cuda, rows * ld, GUARD)
    out = buf.view(FP)[GUARD:GUARD + rows * ld].view(rows, ld)
    assert out.data_ptr() == ptr and ptr % 16 == 0
    return buf, before, out


def _cols_kept(cuda, rows, ld, n):
    return (torch.arange(ld, device=cuda) < n)[None, :].expand(rows, ld)


# ------------------------------------------------------------------------------------------------ ops.linear
def _a_form(a, form):
    """The same values as a [M, K] behind another layout."""
    M, K = a.shape
    if form == "slice":                      # a column slice of a wider tensor: 16-byte-aligned base, lda != K
        wide = torch.full((M, K + 24), 7.0, device=a.device)
        wide[:, 8:8 + K] = a
        v = wide[:, 8:8 + K]
    elif form == "rows2":                    # every second row
        big = torch.full((2 * M, K), 7.0, device=a.device)
        big[::2] = a
        v = big[::2]
    else:                                    # a 4-byte-misaligned view: the host copies
        flat = torch.full((M * K + 1,), 7.0, device=a.device)
        flat[1:] = a.reshape(-1)
        v = flat[1:].view(M, K)
        assert v.data_ptr() % 16 == 4
    assert torch.equal(v, a)
    return v


@pytest.mark.parametrize("M,N,K", F32_LINEAR_SHAPES)
def test_linear_f32_bound(cuda, M, N, K):
    a, w, b, r, _ = f32_gemm_inputs(M, N, K, device=cuda)
    b[0] = 9.0
    b[1] = -9.0                              # a saturated sigmoid, the far tail of erf
    for bias, res in ((None, None), (b, None), (b, r)):
        y = ops.linear(a, w, bias, residual=res)
        _ran_native("gemm")
        ref, tol = gemm_bound(a, w, bias, res, dtype=FP)
        assert_within(y, ref, tol, f"f32/linear {M}x{N}x{K} bias={bias is not None} res={res is not None}")
    for act in F32_ACTS[1:]:
        for res in (None, r):
            y = ops.linear(a, w, b, residual=res, act=act)
            _ran_native("gemm")
            ref, tol = gemm_act_bound(a, w, b, res, act, dtype=FP)
            assert_within(y, ref, tol, f"f32/linear {M}x{N}x{K} {act} res={res is not None}")


@pytest.mark.parametrize("form", ["slice", "rows2", "misaligned"])
@pytest.mark.parametrize("M,N,K", F32_LINEAR_SHAPES)
def test_linear_f32_bound_strided_a(cuda, M, N, K, form):
    a, w, b, r, _ = f32_gemm_inputs(M, N, K, seed=1, device=cuda)
    wv = _a_form(w, form) if form == "misaligned" else w          # a dense weight on a misaligned base as well
    y = ops.linear(_a_form(a, form), wv, b, residual=r, act="silu")
    _ran_native("gemm")
    ref, tol = gemm_act_bound(a, w, b, r, "silu", dtype=FP)
    assert_within(y, ref, tol, f"f32/linear {M}x{N}x{K} A as {form}")


@pytest.mark.parametrize("M,N,K", F32_LINEAR_SHAPES)
def test_linear_f32_out_writes_only_its_output(cuda, M, N, K):
    a, w, b, r, _ = f32_gemm_inputs(M, N, K, seed=2, device=cuda)
    buf, before, out = _guarded_out(cuda, M, N)
    y = ops.linear(a, w, b, residual=r, out=out)
    _ran_native("gemm")
    assert y.data_ptr() == out.data_ptr()
    got = _check_guard(buf, before, torch.ones(M, N, dtype=torch.bool, device=cuda), FP, f"f32/linear out= {M}x{N}x{K}")
    ref, tol = gemm_bound(a, w, b, r, dtype=FP)
    assert_within(got.view(M, N), ref, tol, f"f32/linear out= guarded {M}x{N}x{K}")


# ------------------------------------------------------------------------------------------------ ops.f32.gemm raw
HEADS = 3


@pytest.mark.parametrize("bkn", [False, True], ids=["nt", "bkn"])
@pytest.mark.parametrize("N", [4, 40, 132])
@pytest.mark.parametrize("M", [1, 130])
def test_gemm_f32_raw_batched(cuda, M, N, bkn):
    """batch = 3 over head strides as ops.f32.attention launches it: A and B are per-head column slices of fused
    rows (K = 77 on rows of stride 80 a head), C [3, M, ld] with ld = N + 4 > N, alpha = 1 / sqrt(40) with a bias."""
    K, Ks = 77, 80
    al = 1.0 / math.sqrt(40)
    A = torch.zeros(M, HEADS * Ks, device=cuda)
    ws, b = [], None
    for h in range(HEADS):
        a, w, b, _, _ = f32_gemm_inputs(M, N, K, seed=10 + h, device=cuda)
        A[:, h * Ks:h * Ks + K] = a
        A[:, h * Ks + K:(h + 1) * Ks] = 1e4                  # past K: never multiplied
        ws.append(w)
    if bkn:                                                 # B [K, heads N]: head h in columns h N .. h N + N
        B = torch.cat([w.t() for w in ws], 1).contiguous()
        ldb, sbb = HEADS * N, N
    else:                                                   # B [N, heads Ks]
        B = torch.full((N, HEADS * Ks), 1e4, device=cuda)
        for h, w in enumerate(ws):
            B[:, h * Ks:h * Ks + K] = w
        ldb, sbb = HEADS * Ks, Ks
    ld = N + 4
    buf, before, out = _guarded_out(cuda, HEADS * M, ld)
    f32.gemm(A, B, out, bias=b, alpha=al, bkn=bkn, batch=HEADS, sab=Ks, sbb=sbb, scb=M * ld, M=M, N=N, K=K,
             lda=HEADS * Ks, ldb=ldb, ldc=ld)
    got = _check_guard(buf, before, _cols_kept(cuda, HEADS * M, ld, N), FP, f"f32/gemm raw {M}x{N} bkn={bkn}")
    got = got.view(HEADS, M, N)
    for h in range(HEADS):
        ref, tol = gemm_bound(A[:, h * Ks:h * Ks + K], ws[h], b, None, alpha=al, dtype=FP)
        assert_within(got[h], ref, tol, f"f32/gemm raw head {h} {M}x{N}x{K} bkn={bkn}")


@pytest.mark.parametrize("what", ["lda", "base", "bkn_n", "act6"])
def test_gemm_f32_raw_refusals(cuda, what):
    """Operands the kernel's float4 loads cannot take, and an activation code outside the set: an error, no write."""
    M, N, K = 5, 8, 8
    a = torch.randn(M * (K + 1) + 4, device=cuda)
    w = torch.randn(K * N + 4, device=cuda)
    out = torch.full((M, N), 3.0, device=cuda)
    kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N)
    if what == "lda":
        kw["lda"] = K + 1
    elif what == "base":
        a = a[1:]
        assert a.data_ptr() % 16 == 4
    elif what == "bkn_n":
        kw.update(bkn=True, N=5, ldb=8, ldc=5)
    else:
        kw["act_code"] = core.ACT_CODES["leaky_relu"]
        assert kw["act_code"] == 6
    with pytest.raises(RuntimeError, match="cgs_gemm_f32 failed"):
        f32.gemm(a, w, out, **kw)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()), f"{what}: a refused launch wrote"


# ------------------------------------------------------------------------------------------------ ops.conv2d
def _conv_operands(cuda, case, seed=0):
    N, C1, C2, H, W, Cout, k, stride, pad, up2, res = case
    x, x2, w, b, (s_i, _, s_o) = f32_conv_inputs(N, C1, C2, H, W, Cout, k, seed, device=cuda)
    Hl, Wl = (2 * H, 2 * W) if up2 else (H, W)
    Ho, Wo = (Hl + 2 * pad - k) // stride + 1, (Wl + 2 * pad - k) // stride + 1
    r = None
    if res:
        g = torch.Generator().manual_seed(seed + 100)
        r = (torch.randn(N, Cout, Ho, Wo, generator=g) * s_i[:, None, None, None] * s_o[None, :, None, None]).to(cuda)
    return x, x2, w, b, r, Ho, Wo


@pytest.mark.parametrize("nhwc_w", [False, True], ids=["w_nchw", "w_nhwc"])
@pytest.mark.parametrize("case", F32_CONV_CASES)
def test_conv_f32_bound(cuda, case, nhwc_w):
    N, C1, C2, H, W, Cout, k, stride, pad, up2, res = case
    x, x2, w, b, r, Ho, Wo = _conv_operands(cuda, case)
    ref, tol = conv_bound(x, w, b, r, stride, pad, up2, x2, dtype=FP)
    wn = w.permute(0, 2, 3, 1).contiguous() if nhwc_w else None
    y = ops.conv2d(x.contiguous(memory_format=CL), w, b, stride, pad, residual=None if r is None else r.contiguous(memory_format=CL),
                   weight_nhwc=wn, upsample2x=up2, x2=None if x2 is None else x2.contiguous(memory_format=CL))
    _ran_native("conv")
    assert tuple(y.shape) == (N, Cout, Ho, Wo)
    assert_within(y, ref, tol, f"f32/conv {case} weight_nhwc={nhwc_w}")


def test_conv_f32_bound_from_nchw_input(cuda):
    case = F32_CONV_CASES[2]
    N, C1, C2, H, W, Cout, k, stride, pad, up2, res = case
    x, x2, w, b, r, Ho, Wo = _conv_operands(cuda, case, seed=1)
    assert x.is_contiguous() and x2.is_contiguous() and r.is_contiguous()
    y = ops.conv2d(x, w, b, stride, pad, residual=r, upsample2x=up2, x2=x2)
    _ran_native("conv")
    ref, tol = conv_bound(x, w, b, r, stride, pad, up2, x2, dtype=FP)
    assert_within(y, ref, tol, f"f32/conv {case} from NCHW-contiguous operands")


@pytest.mark.parametrize("case", [c for c in F32_CONV_CASES if c[1] % 4 == 0 and c[2] % 4 == 0])
def test_conv_f32_writes_only_its_output(cuda, case):
    """cgs_conv_f32 on the operands ops.f32.conv2d hands it, y inside a guarded buffer."""
    N, C1, C2, H, W, Cout, k, stride, pad, up2, res = case
    x, x2, w, b, r, Ho, Wo = _conv_operands(cuda, case, seed=2)
    xc = x.permute(0, 2, 3, 1).contiguous()
    x2c = None if x2 is None else x2.permute(0, 2, 3, 1).contiguous()
    wn = w.permute(0, 2, 3, 1).contiguous()
    rc = None if r is None else r.permute(0, 2, 3, 1).contiguous()
    rows = N * Ho * Wo
    buf, before, out = _guarded_out(cuda, rows, Cout)
    rc_ = _native.load_kernels().cgs_conv_f32(xc.data_ptr(), core._ptr(x2c), wn.data_ptr(), b.data_ptr(), core._ptr(rc),
                                              out.data_ptr(), N, H, W, C1, C2, Cout, k, k, stride, pad, 1 if up2 else 0, Ho,
                                              Wo, core._stream())
    assert rc_ == 0
    got = _check_guard(buf, before, torch.ones(rows, Cout, dtype=torch.bool, device=cuda), FP, f"f32/conv {case}")
    ref, tol = conv_bound(x, w, b, r, stride, pad, up2, x2, dtype=FP)
    assert_within(got.view(N, Ho, Wo, Cout).permute(0, 3, 1, 2), ref, tol, f"f32/conv guarded {case}")


# ------------------------------------------------------------------------------------------------ ops.group_norm
def _gn_run(cuda, case, silu, pre, shift=0.0, seed=0):
    N, C1, C2, G, H, W = case
    C = C1 + C2
    x, x2, w, b, pa = f32_gn_inputs(N, C1, C2, H, W, seed, device=cuda, shift=shift)
    pa = pa if pre else None
    S = gn_f32_form(N, H * W, C)[0]
    assert int(_native.load_kernels().cgs_groupnorm_f32_ws(N, H * W, C)) == 2 * N * C * (S + 1)
    y = ops.group_norm(x.contiguous(memory_format=CL), G, w, b, 1e-6, silu=silu, pre_add=pa,
                       x2=None if x2 is None else x2.contiguous(memory_format=CL))
    _ran_native("groupnorm")
    ref, tol = groupnorm_f32_bound(x, G, w, b, 1e-6, silu, pa, x2)
    return assert_within(y, ref, tol, f"f32/groupnorm {case} silu={silu} pre={pre} shift={shift}")


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "pre_add"])
@pytest.mark.parametrize("silu", [False, True], ids=["id", "silu"])
@pytest.mark.parametrize("case", F32_GN_CASES)
def test_groupnorm_f32_bound(cuda, case, silu, pre):
    _gn_run(cuda, case, silu, pre)


def test_groupnorm_f32_bound_large_mean(cuda):
    _gn_run(cuda, (2, 320, 0, 32, 10, 10), True, True, shift=300.0, seed=3)


def test_groupnorm_f32_bound_apply_second_trip(cuda):
    """N HW C / 4 > 16384 x 256 chunks: the apply kernel's grid-stride loop runs a second time; 2048 slices."""
    case = (1, 64, 0, 8, 513, 513)
    assert 513 * 513 * 64 // 4 > 16384 * 256 and gn_f32_form(1, 513 * 513, 64) == (2048, 16)
    _gn_run(cuda, case, True, False, seed=4)


# ------------------------------------------------------------------------------------------------ ops.layer_norm
@pytest.mark.parametrize("C", F32_LN_C)
@pytest.mark.parametrize("rows", F32_LN_ROWS)
def test_layernorm_f32_bound(cuda, rows, C):
    x, w, b = f32_ln_inputs(rows, C, device=cuda)
    for wa, ba in ((w, b), (None, b), (w, None), (None, None)):
        y = ops.layer_norm(x, wa, ba, 1e-5)
        _ran_native("layernorm")
        ref, tol = layernorm_bound(x, wa, ba, 1e-5, depth=ln_f32_depth(C))
        assert_within(y, ref, tol, f"f32/layernorm {rows}x{C} w={wa is not None} b={ba is not None}")


def test_layernorm_f32_bound_large_mean(cuda):
    rows, C = 5, 260
    x, w, b = f32_ln_inputs(rows, C, seed=1, device=cuda, shift=1000.0)
    y = ops.layer_norm(x, w, b, 1e-5)
    _ran_native("layernorm")
    ref, tol = layernorm_bound(x, w, b, 1e-5, depth=ln_f32_depth(C))
    assert_within(y, ref, tol, f"f32/layernorm {rows}x{C} at mean 1000")


@pytest.mark.parametrize("rows,C", [(1, 4), (5, 260)])
def test_layernorm_f32_writes_only_its_rows(cuda, rows, C):
    """Four rows a block: the rows past the last (the idle waves of the last block) must keep their bits."""
    x, w, b = f32_ln_inputs(rows, C, seed=2, device=cuda)
    buf, before, out = _guarded_out(cuda, rows, C)
    assert _native.load_kernels().cgs_layernorm_f32(x.data_ptr(), out.data_ptr(), w.data_ptr(), b.data_ptr(), rows, C, 1e-5,
                                                    core._stream()) == 0
    got = _check_guard(buf, before, torch.ones(rows, C, dtype=torch.bool, device=cuda), FP, f"f32/layernorm {rows}x{C}")
    ref, tol = layernorm_bound(x, w, b, 1e-5, depth=ln_f32_depth(C))
    assert_within(got.view(rows, C), ref, tol, f"f32/layernorm guarded {rows}x{C}")


# ------------------------------------------------------------------------------------------------ ops.attention
def _attn_masks(cuda, B, Sq, Sk, kind):
    g = torch.Generator().manual_seed(9)
    mask = kp = None
    if kind == "padding":                                  # ragged: another length in every image
        kp = torch.ones(B, Sk, dtype=torch.bool)
        for bi in range(B):
            kp[bi, Sk - 6 - 13 * bi:] = False
        kp = kp.to(cuda)
    elif kind == "float":
        mask = (2.0 * torch.randn(B, 1, Sq, Sk, generator=g)).to(cuda)
    elif kind == "bool":
        mask = torch.rand(Sq, Sk, generator=g) > 0.3
        mask[:, 0] = True
        mask = mask.to(cuda)
    return mask, kind == "causal", kp


@pytest.mark.parametrize("kind", ["plain", "causal", "padding", "float", "bool"])
def test_attention_f32_bound(cuda, kind):
    B, heads, Sq, Sk, D = 2, 3, 130, 77, 40
    q, k, v, _ = f32_attn_inputs(B, heads, Sq, Sk, D, device=cuda)
    assert not q.is_contiguous() and q.stride(1) == 3 * heads * D              # views of one fused tensor
    mask, causal, kp = _attn_masks(cuda, B, Sq, Sk, kind)
    o = ops.attention(q, k, v, heads, mask=mask, causal=causal, key_padding=kp)
    _ran_native("attention")
    ref, tol = attention_f32_bound(q, k, v, heads, mask, causal, kp)
    assert_within(o, ref, tol, f"f32/attention {B}x{heads}x{Sq}x{Sk}x{D} {kind}")


@pytest.mark.parametrize("B,heads,Sq,Sk,D", [(1, 2, 5, 1, 4), (1, 1, 1, 3, 8)])
def test_attention_f32_bound_tiny(cuda, B, heads, Sq, Sk, D):
    """Sk < 4: every score row is mostly pad columns."""
    q, k, v, _ = f32_attn_inputs(B, heads, Sq, Sk, D, device=cuda)
    o = ops.attention(q, k, v, heads)
    _ran_native("attention")
    ref, tol = attention_f32_bound(q, k, v, heads)
    assert_within(o, ref, tol, f"f32/attention {B}x{heads}x{Sq}x{Sk}x{D}")


def test_attention_f32_bound_chunked_with_blocked_row(cuda, monkeypatch):
    """Score chunks of 50 rows, the last of 29. Query row 90 has every key blocked: it is row 40 of the second
    chunk (mid-chunk) and stays as NaN in the stale tail of the buffer under the last chunk. That row is NaN (the
    convention of this path, ops.attention); every other row is finite and within its bound."""
    B, heads, Sq, Sk, D = 2, 2, 129, 132, 64
    monkeypatch.setattr(f32, "SCORE_BUDGET", 50 * heads * Sk)
    q, k, v, _ = f32_attn_inputs(B, heads, Sq, Sk, D, seed=1, device=cuda)
    o = ops.attention(q, k, v, heads)
    _ran_native("attention")
    ref, tol = attention_f32_bound(q, k, v, heads)
    assert_within(o, ref, tol, f"f32/attention chunked {B}x{heads}x{Sq}x{Sk}x{D}")
    mask = torch.ones(Sq, Sk, dtype=torch.bool, device=cuda)
    mask[90] = False
    o = ops.attention(q, k, v, heads, mask=mask)
    _ran_native("attention")
    ref, tol = attention_f32_bound(q, k, v, heads, mask)
    assert bool(torch.isnan(ref[:, 90]).all()) and bool(torch.isnan(o[:, 90]).all())
    rows = [i for i in range(Sq) if i != 90]
    assert bool(torch.isfinite(ref[:, rows]).all())
    assert_within(o[:, rows], ref[:, rows], tol[:, rows], "f32/attention chunked, beside a blocked row")
