"""Per-element error bounds (tests/_bounds.py) on the device for the fused epilogues: the activation epilogues of the
GEMMs (mc::tile family, v6 ACT, skinny, the split-K reduce, the LayerNorm-folded forms) and of the convs
(cgs_conv2d_nhwc_act), and the statistics partials a producer writes beside its output -- the row statistics of
cgs_gemm_bf16_rowstats_v, the sums of squares of cgs_gemm_bf16_gelu_gns and the GroupNorm partials of
cgs_conv2d_nhwc_gns -- each compared with fp64 statistics of the tensor the kernel stored, and then through the
consumer the model runs (cgs_ln_rs_from_partials, cgs_grn_apply_gns, cgs_groupnorm_nhwc_part).

The kernel table, the shapes (a partial tile, one row / one vector past a tile, more tiles than a persistent grid)
and the guarded C buffer are test_kernel_bounds_gpu.py's. Every partials buffer is pre-filled with one NaN bit
pattern and has guard rows before and after: every entry the kernel owns must be finite, every other must keep its
bits. Two pre-activation columns are pushed to +-9 through the bias (the clamp of gelu_sig, a saturated sigmoid)."""
import math

import pytest
import torch

from comfy_gen_server_amd import ops, _native
from comfy_gen_server_amd.ops import core

from _bounds import (assert_within, conv_act_bound, conv_bound, gemm_act_bound, gemm_bound, gn_partials_bound,
                     grn_apply_bound, grn_bound, grn_depth, groupnorm_bound, layernorm_stats_bound, partials_merge_tol,
                     rowstats_partials_bound, rs_from_partials_bound, sumsq_partials_bound)
from _guards import _check_guard as _check_guard_flat, _guarded
from test_kernel_bounds_gpu import (CONV_CASES, GEMM_KERNELS, LNFOLD_KERNELS, SPLITK_TILES, _check_guard,
                                    _conv_in_domain, _edge_shape, _guarded_c, _in_domain, _native_loaded,  # noqa: F401
                                    _operands, _partial_shape, _persistent_shape, _pick_bn, _ptr, _splitk)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN_BITS = 0x7FC12345                # the fill of every partials buffer: a quiet NaN no kernel produces
GUARD_ROWS = 8


def _push_bias(b):
    b[0], b[1] = 9.0, -9.0
    return b


def _nan_guarded(cuda, rows, row_floats):
    """rows x row_floats fp32 partials with GUARD_ROWS rows before and after, all NAN_BITS: (buffer, pointer, view)."""
    buf = torch.full(((rows + 2 * GUARD_ROWS) * row_floats,), NAN_BITS, dtype=torch.int32, device=cuda)
    own = buf[GUARD_ROWS * row_floats:(GUARD_ROWS + rows) * row_floats]
    assert own.data_ptr() % 16 == 0
    return buf, own.data_ptr(), own.view(torch.float32).view(rows, row_floats)


def _guards_kept(buf, rows, row_floats, what):
    torch.cuda.synchronize()
    g = GUARD_ROWS * row_floats
    assert bool((buf[:g] == NAN_BITS).all()) and bool((buf[g + rows * row_floats:] == NAN_BITS).all()), \
        f"{what}: the guard rows around the partials changed"


# ------------------------------------------------------------------------------------------------ GEMM activations
# (code in bits 8-10 beside EPI_GELU, the activation it stands for): 0 = the flag alone
GEMM_ACTS = [(0, "gelu"), (1, "gelu")] + [(core.ACT_CODES[n], n) for n in ("gelu_tanh", "quick_gelu", "silu", "relu")]
ACT_KERNELS = ["skinny", "v3w4", "v3w8", "v6pp160", "v8t128", "v10t64x128", "v11t128x64", "v12t64x128s6",
               "v13t128x64s6", "v14t128s5"]


def _act_cases():
    cases = []
    for name in ACT_KERNELS:
        s = GEMM_KERNELS[name]
        shapes = [_partial_shape(s) + (s["min_k"],), _edge_shape(s) + (3 * s["k_step"],)]
        if name == "skinny":
            shapes.append((1, 8, 32))
        cases += [(name,) + sh for sh in shapes]
    return cases


def _gemm_act(name, a, w, c, b, r, M, N, K, ldc, code):
    lib, s = _native.load_kernels(), GEMM_KERNELS[name]
    assert _in_domain(s, M, N, K) and (name != "v6pp160" or (K % 64 == 0 and K >= 128)), (name, M, N, K)
    if name in ("v3w4", "v3w8"):
        assert _pick_bn(M, N) == s["bn"]
    epi = core.EPI_BIAS | core.EPI_GELU | (code << 8) | (core.EPI_RESIDUAL if r is not None else 0)
    return lib.cgs_gemm_bf16_v(a.data_ptr(), w.data_ptr(), c, b.data_ptr(), _ptr(r), M, N, K, a.stride(0), w.stride(0),
                               ldc, r.stride(0) if r is not None else 0, epi, 1.0, s["variant"], core._stream())


@pytest.mark.parametrize("res", [False, True], ids=["bias", "bias_res"])
@pytest.mark.parametrize("name,M,N,K", _act_cases())
def test_gemm_act_bound(cuda, name, M, N, K, res):
    a, w, b, r = _operands(cuda, M, N, K, "bias_res" if res else "bias")
    _push_bias(b)
    for code, act in GEMM_ACTS:
        out = torch.empty(M, N, device=cuda, dtype=BF)
        assert _gemm_act(name, a, w, out.data_ptr(), b, r, M, N, K, N, code) == 0
        ref, tol = gemm_act_bound(a, w, b, r, act)
        assert_within(out, ref, tol, f"act/gemm/{name} {M}x{N}x{K} code {code} ({act}) res={res}")


@pytest.mark.parametrize("name", ACT_KERNELS)
def test_gemm_act_writes_only_its_output(cuda, name):
    s = GEMM_KERNELS[name]
    M, N = _partial_shape(s)
    K = s["min_k"]
    a, w, b, r = _operands(cuda, M, N, K, "bias_res", lda=K + 8, ldw=K + 16, ldr=N + 16)
    _push_bias(b)
    for code, act in ((core.ACT_CODES["silu"], "silu"), (0, "gelu")):
        buf, before, ldc = _guarded_c(cuda, M, N, s["bm"])
        assert _gemm_act(name, a, w, buf.data_ptr() + 2 * 4096, b, r, M, N, K, ldc, code) == 0
        torch.cuda.synchronize()
        out = _check_guard(buf, before, M, N, ldc, f"act/gemm/{name} {act}")
        ref, tol = gemm_act_bound(a, w, b, r, act)
        assert_within(out, ref, tol, f"act/gemm/{name} guarded, strided {M}x{N}x{K} {act}")


def test_gemm_act_bound_v6_persistent_ragged_round(cuda):
    s = GEMM_KERNELS["v6pp160"]
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    M, N = _persistent_shape(s, cus)
    K = s["min_k"]
    a, w, b, r = _operands(cuda, M, N, K, "bias_res")
    _push_bias(b)
    for code, act in ((0, "gelu"), (core.ACT_CODES["gelu_tanh"], "gelu_tanh"), (core.ACT_CODES["relu"], "relu")):
        out = torch.empty(M, N, device=cuda, dtype=BF)
        assert _gemm_act("v6pp160", a, w, out.data_ptr(), b, r, M, N, K, N, code) == 0
        ref, tol = gemm_act_bound(a, w, b, r, act)
        assert_within(out, ref, tol, f"act/gemm/v6pp160 persistent {M}x{N}x{K} on {cus} CUs {act}")


# ---- the erf GELU elsewhere
@pytest.mark.parametrize("res", [False, True], ids=["bias", "bias_res"])
@pytest.mark.parametrize("splits,K", [(2, 64), (3, 288)])
@pytest.mark.parametrize("variant", sorted(SPLITK_TILES))
def test_gemm_act_bound_splitk(cuda, variant, splits, K, res):
    lib = _native.load_kernels()
    bm, bn = SPLITK_TILES[variant]
    for M, N in ((bm - 3, bn - 8), (bm + 1, bn + 8)):
        a, w, b, r = _operands(cuda, M, N, K, "bias_res" if res else "bias")
        _push_bias(b)
        ws = torch.full((int(lib.cgs_splitk_ws_bytes(M, N, splits)),), 0x7F, dtype=torch.uint8, device=cuda)
        out = torch.empty(M, N, device=cuda, dtype=BF)
        flags = core.EPI_BIAS | core.EPI_GELU | (core.EPI_RESIDUAL if res else 0)
        assert lib.cgs_gemm_bf16_splitk(a.data_ptr(), w.data_ptr(), out.data_ptr(), b.data_ptr(), _ptr(r), None, None, M,
                                        N, K, K, K, N, N if res else 0, flags, 1.0, splits, variant, ws.data_ptr(),
                                        ws.numel(), core._stream()) == 0
        ref, tol = gemm_act_bound(a, w, b, r, "gelu")
        assert_within(out, ref, tol, f"act/gemm/splitk v{variant} x{splits} {M}x{N}x{K} gelu res={res}")


def _lnfold_operands(cuda, M, N, K, seed=1):
    """test_gemm_lnfold_bound's: (x, rs, w2, cs, b2) from ops.layernorm_stats / ops.lnfold_weights."""
    torch.manual_seed(seed)
    x = (torch.randn(M, K, device=cuda) * 3 + 1.5).to(BF)
    gamma = (torch.rand(K, device=cuda) + 0.5).to(BF)
    beta = (torch.randn(K, device=cuda) * 0.2).to(BF)
    w = (torch.randn(N, K, device=cuda) / math.sqrt(K)).to(BF)
    b = torch.randn(N, device=cuda).to(BF)
    rs = ops.layernorm_stats(x, 1e-5)
    w2, cs, b2 = ops.lnfold_weights(w, b, gamma, beta)
    return x, rs, w2, cs, _push_bias(b2.clone())


@pytest.mark.parametrize("name", ["v6pp160", "v8t128", "v10t64x128", "v11t128x64"])
def test_gemm_act_bound_lnfold(cuda, name):
    lib, s = _native.load_kernels(), GEMM_KERNELS[name]
    n_part, n_edge = LNFOLD_KERNELS[name]
    for M, N, K in [(M, N, K) for M, N in ((s["bm"] - 3, n_part), (s["bm"] + 1, n_edge)) for K in (128, 192)]:
        assert _in_domain(s, M, N, K) and K % 64 == 0 and (name != "v6pp160" or N % 160 == 0)
        x, rs, w2, cs, b2 = _lnfold_operands(cuda, M, N, K)
        out = torch.empty(M, N, device=cuda, dtype=BF)
        assert lib.cgs_gemm_bf16_lnfold_v(x.data_ptr(), w2.data_ptr(), out.data_ptr(), b2.data_ptr(), rs.data_ptr(),
                                          cs.data_ptr(), M, N, K, K, K, N, core.EPI_BIAS | core.EPI_GELU, None, 0,
                                          s["variant"], core._stream()) == 0
        ref, tol = gemm_act_bound(x, w2, b2, None, "gelu", rs=rs, cs=cs)
        assert_within(out, ref, tol, f"act/gemm/lnfold {name} {M}x{N}x{K} gelu")


# ------------------------------------------------------------------------------------------------ conv activations
CONV_ACTS = [("relu", 0.0), ("leaky_relu", 0.2), ("leaky_relu", -0.3), ("silu", 0.0), (None, 0.0)]
# (N, C1, C2, H, W, Cout, k, stride, pad, upsample2x): N Ho Wo = 63, and one output row past the kernel's tile
CONV_ACT_EXTRA = {3: [(1, 96, 0, 7, 9, 24, 3, 1, 1, False), (1, 96, 0, 1, 257, 24, 3, 1, 1, False)],
                  4: [(1, 96, 0, 7, 9, 24, 3, 1, 1, False), (1, 96, 0, 1, 257, 24, 3, 1, 1, False)],
                  8: [(1, 96, 0, 7, 9, 24, 3, 1, 1, False), (1, 96, 0, 3, 43, 24, 3, 1, 1, False)]}
CONV_ACT_CASES = [c[1:] for c in CONV_CASES if c[1] in (3, 4, 8)] + \
                 [(v,) + sh for v, shs in CONV_ACT_EXTRA.items() for sh in shs]


def _nhwc(t):
    return t.to(BF).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("res", [False, True], ids=["bias", "bias_res"])
@pytest.mark.parametrize("variant,N,C1,C2,H,W,Cout,k,s,p,up", CONV_ACT_CASES)
def test_conv_act_bound(cuda, variant, N, C1, C2, H, W, Cout, k, s, p, up, res):
    assert _conv_in_domain(variant, C1, C2, Cout, k) and Cout == 24
    mine = [c for c in CONV_ACT_CASES if c[0] == variant]               # every variant: stride 2, upsample2x, two sources
    assert any(c[8] == 2 for c in mine) and any(c[10] for c in mine) and any(c[3] for c in mine)
    lib = _native.load_kernels()
    torch.manual_seed(0)
    x = _nhwc(torch.randn(N, C1, H, W, device=cuda) + 0.5)
    x2 = _nhwc(torch.randn(N, C2, H, W, device=cuda) + 0.5) if C2 else None
    Cin = C1 + C2
    w = (torch.randn(Cout, Cin, k, k, device=cuda) / math.sqrt(Cin * k * k)).to(BF)
    wn = w.permute(0, 2, 3, 1).contiguous()
    b = _push_bias(torch.randn(Cout, device=cuda).to(BF))
    Hl, Wl = (2 * H, 2 * W) if up else (H, W)
    Ho, Wo = (Hl + 2 * p - k) // s + 1, (Wl + 2 * p - k) // s + 1
    r = _nhwc(torch.randn(N, Cout, Ho, Wo, device=cuda)) if res else None
    for act, param in CONV_ACTS:
        out = torch.empty((N, Cout, Ho, Wo), device=cuda, dtype=BF, memory_format=torch.channels_last)
        assert lib.cgs_conv2d_nhwc_act(x.data_ptr(), _ptr(x2), C1, wn.data_ptr(), b.data_ptr(), _ptr(r), out.data_ptr(),
                                       N, H, W, Cin, Cout, k, k, s, p, Ho, Wo, 16 if up else 0, variant,
                                       core.ACT_CODES[act] if act else 0, param, core._stream()) == 0
        ref, tol = conv_act_bound(x, w, b, r, act, param, s, p, upsample2x=up, x2=x2)
        assert_within(out, ref, tol, f"act/conv/v{variant} {N}x{C1}+{C2}x{H}x{W}->{Cout} k{k}s{s} up={up} "
                                     f"{act}({param}) res={res}")


# ------------------------------------------------------------------------------------------------ row statistics
RSO_KERNELS = {6: "v6pp160", 19: "v6m128", 20: "v6w4"}


def _rowstats_case(cuda, lib, variant, M, N, K, res, what, shift=None):
    """One cgs_gemm_bf16_rowstats_v call and its four assertions, numbered as they run. shift: the residual at
    randn 3 + shift."""
    s = GEMM_KERNELS[RSO_KERNELS[variant]]
    assert _in_domain(s, M, N, K) and N % 160 == 0
    P = N // 80
    a, w, b, r = _operands(cuda, M, N, K, "bias_res" if res else "bias", ldr=N + 16)
    if shift is not None:
        r = (torch.randn(M, N + 16, device=cuda) * 3 + shift).to(BF)[:, :N]
    ldr = r.stride(0) if res else 0
    epi = core.EPI_BIAS | (core.EPI_RESIDUAL if res else 0)
    st = core._stream()
    plain = torch.empty(M, N, device=cuda, dtype=BF)
    assert lib.cgs_gemm_bf16_v(a.data_ptr(), w.data_ptr(), plain.data_ptr(), b.data_ptr(), _ptr(r), M, N, K, K, K, N, ldr,
                               epi, 1.0, variant, st) == 0
    buf, before, ldc = _guarded_c(cuda, M, N, s["bm"])
    pbuf, pptr, part = _nan_guarded(cuda, M, 2 * P)
    assert lib.cgs_gemm_bf16_rowstats_v(a.data_ptr(), w.data_ptr(), buf.data_ptr() + 2 * 4096, b.data_ptr(), _ptr(r), M, N,
                                        K, K, K, ldc, ldr, epi, 1.0, pptr, variant, st) == 0
    torch.cuda.synchronize()
    out = _check_guard(buf, before, M, N, ldc, what)
    ref, tol = gemm_bound(a, w, b, r)
    assert_within(out, ref, tol, what + " C")                                           # 1
    assert torch.equal(out, plain), what + ": C differs from cgs_gemm_bf16_v of the same variant"      # 2
    _guards_kept(pbuf, M, 2 * P, what)                                                  # 3
    part = part.view(M, P, 2)
    pref, ptol = rowstats_partials_bound(out)
    assert_within(part, pref, ptol, what + " partials")
    rs = torch.empty(M, 2, device=cuda, dtype=torch.float32)                            # 4
    assert lib.cgs_ln_rs_from_partials(pptr, rs.data_ptr(), M, P, 1e-5, st) == 0
    torch.cuda.synchronize()
    r1, t1 = rs_from_partials_bound(part, 1e-5)
    assert_within(rs, r1, t1, what + " rs from the partials")
    r2, t2 = layernorm_stats_bound(out, 1e-5)
    assert_within(rs, r2, t2 + t1 + partials_merge_tol(pref, ptol, 1e-5), what + " rs against the stored rows")


@pytest.mark.parametrize("N", [160, 320, 480])
@pytest.mark.parametrize("variant", sorted(RSO_KERNELS))
def test_rowstats_partials_bound(cuda, variant, N):
    lib, bm = _native.load_kernels(), GEMM_KERNELS[RSO_KERNELS[variant]]["bm"]
    for M in (1, bm - 3, bm + 1):
        for K in (128, 192):
            for res in (False, True):
                _rowstats_case(cuda, lib, variant, M, N, K, res, f"rowstats/v{variant} {M}x{N}x{K} res={res}")


@pytest.mark.parametrize("variant", sorted(RSO_KERNELS))
def test_rowstats_partials_bound_persistent_and_shifted(cuda, variant):
    """More tiles than workgroups at N = 320 (the last tile row one row high), and a residual at randn 3 + 40: the
    rows' mean is far from their spread, so the shift by the lane's first value is what keeps M2."""
    lib, s = _native.load_kernels(), GEMM_KERNELS[RSO_KERNELS[variant]]
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    N = 320
    tiles_n, grid = -(-N // s["bn"]), s["grid"] * cus
    tiles_m = grid // tiles_n + 2
    M = (tiles_m - 1) * s["bm"] + 1
    assert grid < tiles_m * tiles_n < 2 * grid
    _rowstats_case(cuda, lib, variant, M, N, 128, True, f"rowstats/v{variant} persistent {M}x{N}x128 on {cus} CUs")
    _rowstats_case(cuda, lib, variant, s["bm"] + 1, N, 192, True, f"rowstats/v{variant} {s['bm'] + 1}x{N}x192 res at 40",
                   shift=40.0)


# ------------------------------------------------------------------------------------------------ GELU + sum of squares
GNS_IMAGES = [(64, 1), (64, 5), (128, 3), (256, 2), (192, 3)]          # (rows per image, images): M = 64 .. 576


def _gelu_gns(lib, a, w, c, b, rs, cs, M, N, K, ldc, epi, part, hw):
    return lib.cgs_gemm_bf16_gelu_gns(a.data_ptr(), w.data_ptr(), c, _ptr(b), _ptr(rs), _ptr(cs), M, N, K, a.stride(0),
                                      w.stride(0), ldc, epi, part, hw, core._stream())


@pytest.mark.parametrize("lnfold", [False, True], ids=["plain", "lnfold"])
@pytest.mark.parametrize("hw,images", GNS_IMAGES)
def test_gelu_sumsq_partials_bound(cuda, hw, images, lnfold):
    lib = _native.load_kernels()
    M = hw * images
    for N in (8, 152, 168):
        for K in (128, 192):
            what = f"sumsq/gelu_gns {images}x{hw}x{N}x{K} lnfold={lnfold}"
            if lnfold:
                a, rs, w, cs, b = _lnfold_operands(cuda, M, N, K, seed=N + K)
            else:
                a, w, b, _ = _operands(cuda, M, N, K, "bias", seed=N + K)
                rs = cs = None
                _push_bias(b)
            buf, before, ldc = _guarded_c(cuda, M, N, 256)
            pbuf, pptr, part = _nan_guarded(cuda, M // 64, N)
            epi = core.EPI_BIAS | core.EPI_GELU | (core.EPI_LNFOLD if lnfold else 0)
            assert _gelu_gns(lib, a, w, buf.data_ptr() + 2 * 4096, b, rs, cs, M, N, K, ldc, epi, pptr, hw) == 0
            torch.cuda.synchronize()
            h = _check_guard(buf, before, M, N, ldc, what)
            ref, tol = gemm_act_bound(a, w, b, None, "gelu", rs=rs, cs=cs)
            assert_within(h, ref, tol, what + " C")                                     # 1
            _guards_kept(pbuf, M // 64, N, what)                                        # 2
            pref, ptol = sumsq_partials_bound(h, hw)
            assert_within(part, pref, ptol, what + " partials")
            # 3: the GRN the model runs on these partials
            torch.manual_seed(N)
            hc = h.contiguous().view(images, hw, N)
            gamma, beta = (torch.randn(N, device=cuda) * 0.5).to(BF), (torch.randn(N, device=cuda) * 0.1).to(BF)
            nblk = (N + 255) // 256
            y = torch.empty_like(hc)
            ws = torch.empty(images * (N + nblk), device=cuda, dtype=torch.float32)
            assert lib.cgs_grn_apply_gns(hc.data_ptr(), pptr, gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                         ws.data_ptr(), images, hw, N, core._stream()) == 0
            torch.cuda.synchronize()
            gx, bsum = ws[:images * N].view(images, N), ws[images * N:].view(images, nblk)
            ref, tol = grn_apply_bound(hc, gamma, beta, gx, bsum)
            assert_within(y, ref, tol, what + " grn apply")
            L, Lm = grn_depth("gns", images, hw, N)
            ref, tol = grn_bound(hc, gamma, beta, False, (L + 8 + 1, Lm))       # the partials' own L = 8 and the square
            assert_within(y, ref, tol, what + " grn against h")


def test_gelu_sumsq_refusals(cuda):
    """hw % 64, M % hw, no bias, a code in the activation bits: an error, and neither C nor the partials are written."""
    lib = _native.load_kernels()
    M, N, K = 192, 152, 128
    a, w, b, _ = _operands(cuda, M, N, K, "bias")
    ok = core.EPI_BIAS | core.EPI_GELU
    for hw, bias, epi in [(96, b, ok), (128, b, ok), (64, None, ok), (64, None, core.EPI_GELU),
                          (64, b, ok | (core.ACT_CODES["silu"] << 8))]:
        buf, before, ldc = _guarded_c(cuda, M, N, 256)
        pbuf, pptr, part = _nan_guarded(cuda, M // 64, N)
        assert _gelu_gns(lib, a, w, buf.data_ptr() + 2 * 4096, bias, None, None, M, N, K, ldc, epi, pptr, hw) != 0
        torch.cuda.synchronize()
        assert torch.equal(buf, before) and bool((pbuf == NAN_BITS).all()), (hw, bias is None, epi)


# ------------------------------------------------------------------------------------------------ conv GroupNorm partials
# (H, W, stride) of the input: Ho Wo = 256, 512, and 256 from a 32 x 32 input at stride 2
GN_IMAGES = [(16, 16, 1), (16, 32, 1), (32, 32, 2)]


def _conv_gns_case(cuda, lib, N, C1, C2, H, W, Cout, stride, bias, res, what):
    Cin, k, p = C1 + C2, 3, 1
    assert Cin % 64 == 0 and (C2 == 0 or C1 % 64 == 0) and k * k * Cin >= 128 and Cout % 8 == 0      # conv_variant_ok(a, 6)
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    HW = Ho * Wo
    assert HW % 256 == 0
    torch.manual_seed(Cout + HW)
    x = _nhwc(torch.randn(N, C1, H, W, device=cuda) + 0.5)
    x2 = _nhwc(torch.randn(N, C2, H, W, device=cuda) + 0.5) if C2 else None
    w = (torch.randn(Cout, Cin, k, k, device=cuda) / math.sqrt(Cin * k * k)).to(BF)
    wn = w.permute(0, 2, 3, 1).contiguous()
    b = (torch.randn(Cout, device=cuda) + 2).to(BF) if bias else None
    r = _nhwc(torch.randn(N, Cout, Ho, Wo, device=cuda)) if res else None
    buf, before, optr = _guarded(cuda, N * HW * Cout, 256 * Cout)        # the NHWC output, a tile of rows after it
    gbuf, gptr, gnp = _nan_guarded(cuda, N * (HW // 64), Cout * 2)
    st = core._stream()
    assert lib.cgs_conv2d_nhwc_gns(x.data_ptr(), _ptr(x2), C1, wn.data_ptr(), _ptr(b), _ptr(r), optr, N, H, W, Cin, Cout,
                                   k, k, stride, p, Ho, Wo, 0, gptr, st) == 0
    own = torch.ones(N * HW * Cout, dtype=torch.bool, device=cuda)
    out = _check_guard_flat(buf, before, own, BF, what).view(N, Ho, Wo, Cout)
    ref, tol = conv_bound(x, w, b, r, stride, p, x2=x2)
    assert_within(out.permute(0, 3, 1, 2), ref, tol, what + " out")                     # 1
    _guards_kept(gbuf, N * (HW // 64), Cout * 2, what)                                  # 2
    pref, ptol = gn_partials_bound(out)
    assert_within(gnp.view(N, HW // 64, Cout, 2), pref, ptol, what + " partials")
    G = 2 if Cout == 8 else 8                                                           # 3
    g, be = torch.randn(Cout, device=cuda).to(BF), torch.randn(Cout, device=cuda).to(BF)
    ab = torch.empty(N * Cout * 2, device=cuda)
    oc = out.contiguous()
    y = torch.empty_like(oc)
    assert lib.cgs_groupnorm_nhwc_part(oc.data_ptr(), y.data_ptr(), g.data_ptr(), be.data_ptr(), None, gptr,
                                       ab.data_ptr(), N, HW, Cout, G, 64, 1e-5, 1, core._DT[BF], st) == 0
    torch.cuda.synchronize()
    ref, tol = groupnorm_bound(oc.permute(0, 3, 1, 2), G, g, be, 1e-5, True, ppb=64)
    assert_within(y.permute(0, 3, 1, 2), ref, tol, what + " groupnorm from the partials")


@pytest.mark.parametrize("Cout", [8, 168])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W,stride", GN_IMAGES)
def test_conv_gn_partials_bound(cuda, H, W, stride, N, Cout):
    lib = _native.load_kernels()
    for bias in (True, False):
        for res in (False, True):
            _conv_gns_case(cuda, lib, N, 64, 0, H, W, Cout, stride, bias, res,
                           f"gn-partials/conv {N}x64x{H}x{W}->{Cout} s{stride} bias={bias} res={res}")


def test_conv_gn_partials_bound_dual_source(cuda):
    _conv_gns_case(cuda, _native.load_kernels(), 3, 64, 64, 16, 16, 168, 1, True, True,
                   "gn-partials/conv 3x64+64x16x16->168 dual source")
