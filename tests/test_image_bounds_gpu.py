"""Per-element error bounds (tests/_bounds.py) on the device for the GRN family and the planar image-space kernels of
csrc/kernels/image.hip: cgs_grn_nhwc_v2 / cgs_grn_nhwc / cgs_grn_apply_gns / cgs_grn_stats / cgs_grn_stats_gns /
cgs_grn_scale_weight, cgs_resize, cgs_upfirdn2d, cgs_fused_bias_act, cgs_softmax_rows, cgs_tome_match.

The kernels are called through _native.load_kernels() with buffers of the test's own: every output and every
workspace, sized exactly as the launcher's comment states, lies in the middle of a pattern-filled buffer whose
surroundings must keep their bits. Each op is also called once through ops.* with the dispatch counter asserted.
References are fp64 on the device. The GRN inputs vary per image and per channel (grn_inputs: nx spans 0 .. 6), so
the per-image table, the bsum tail block, the slice tail and the GNS partial sums all show in the output; the table
GRN_V2_SHAPES names the apply form every shape runs, and grn_slices / grn_row_tiled are asserted against the
library and the table."""
import math

import pytest
import torch

from comfy_gen_server_amd import ops, _native
from comfy_gen_server_amd.ops import core

from _bounds import (C_ACC, E, FBA_SHAPES, GRN_GNS_SHAPES, GRN_MAXN, GRN_V2_SHAPES, RESIZE_CASES, RESIZE_MODES,
                     SMR_COLS, SMR_ROWS, TOME_SHAPES, UPFIRDN_CFGS, UPFIRDN_KERNELS, assert_tome, assert_within, f64,
                     fused_bias_act_bound, grn_apply_bound, grn_bound, grn_depth, grn_inputs, grn_row_tiled,
                     grn_scale_weight_bound, grn_slices, grn_stats_bound, resize_bound, smr_inputs, softmax_rows_bound,
                     tome_inputs, u, upfirdn2d_bound, upfirdn_kernel)
from _guards import _check_guard, _guarded, _native_loaded, _ran_native  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DTYPES = [torch.bfloat16, torch.float16]
ALL_DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS2, IDS3 = ["bf16", "f16"], ["f32", "bf16", "f16"]


def _out(cuda, numel, dtype):
    """A guarded output of numel elements of dtype: (pointer, done(what) -> the elements, guards checked)."""
    w = torch.empty(0, dtype=dtype).element_size() // 2
    buf, before, ptr = _guarded(cuda, numel * w, 4096)

    def done(what):
        return _check_guard(buf, before, torch.ones(numel * w, dtype=torch.bool, device=cuda), dtype, what)
    return ptr, done


def _inv(bsum, C):
    return 1 / (bsum.double().sum(1) / C + 1e-6)


# ------------------------------------------------------------------------------------------------ GRN v2
def test_grn_form_mirror():
    """cgs_grn_slices and the row-tiled predicate restated in Python agree with the library and with the table."""
    lib = _native.load_kernels()
    shapes = list(GRN_V2_SHAPES) + GRN_GNS_SHAPES + [(2, 576, 8192), (4, 4096, 1536), (1, 35, 64), (64, 4096, 8)]
    for N, HW, C in shapes:
        assert int(lib.cgs_grn_slices(N, HW, C)) == grn_slices(N, HW, C), (N, HW, C)
    for (N, HW, C), form in GRN_V2_SHAPES.items():
        assert ("rows" if grn_row_tiled(HW, C) else "grid") == form, (N, HW, C)
    assert max(N for N, _, _ in GRN_V2_SHAPES) == GRN_MAXN
    assert any(C % 256 and C > 256 and N > 4 and HW % grn_slices(N, HW, C) for N, HW, C in GRN_V2_SHAPES)


def _grn_v2(lib, cuda, x, gamma, beta, pre_gelu, what):
    """cgs_grn_nhwc_v2 into guarded y and ws -> (y, gx, bsum)."""
    N, HW, C = x.shape
    S, nblk = grn_slices(N, HW, C), (C + 255) // 256
    yp, ydone = _out(cuda, N * HW * C, x.dtype)
    wp, wdone = _out(cuda, N * ((S + 1) * C + nblk), torch.float32)
    assert lib.cgs_grn_nhwc_v2(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), yp, wp, N, HW, C, int(pre_gelu),
                               core._DT[x.dtype], core._stream()) == 0
    y, ws = ydone(what + " y").reshape(N, HW, C), wdone(what + " ws")
    return y, ws[N * S * C:N * (S + 1) * C].reshape(N, C), ws[N * (S + 1) * C:].reshape(N, nblk)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS2)
@pytest.mark.parametrize("pre_gelu", [False, True])
@pytest.mark.parametrize("N,HW,C", list(GRN_V2_SHAPES))
def test_grn_v2_bound(cuda, N, HW, C, pre_gelu, dtype):
    lib = _native.load_kernels()
    form = GRN_V2_SHAPES[(N, HW, C)]
    assert int(lib.cgs_grn_slices(N, HW, C)) == grn_slices(N, HW, C)
    x, gamma, beta, (cz, _) = grn_inputs(N, HW, C, dtype, cuda)
    depth = grn_depth("v2", N, HW, C)
    ref, tol = grn_bound(x, gamma, beta, pre_gelu, depth)
    gref, gtol, iref, itol = grn_stats_bound(x, pre_gelu, depth)
    try:
        for rows in ((0, 1, 2, 3) if form == "rows" else (1,)):
            assert grn_row_tiled(HW, C, rows) == (form == "rows" and rows > 0)
            lib.cgs_grn_set_rows(rows)
            ran = f"rows{rows}" if grn_row_tiled(HW, C, rows) else "grid"
            what = f"grn_v2/{ran} {N}x{HW}x{C} gelu={pre_gelu} {dtype}"
            y, gx, bsum = _grn_v2(lib, cuda, x, gamma, beta, pre_gelu, what)
            assert_within(y, ref, tol, what)
            assert_within(gx, gref, gtol, what + " gx")
            assert bool((gx[:, cz] == 0).all())
            assert_within(_inv(bsum, C), iref, itol, what + " inv from bsum")
            aref, atol = grn_apply_bound(x, gamma, beta, gx, bsum, pre_gelu)
            assert_within(y, aref, atol, what + " apply")
    finally:
        lib.cgs_grn_set_rows(1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS2)
@pytest.mark.parametrize("pre_gelu", [False, True])
def test_grn_ops_v2_and_fall_to_v1(cuda, pre_gelu, dtype):
    """ops.grn_nhwc: the v2 kernel at N = 5; N = 65 > GRN_MAXN falls to the v1 kernel (the GELU then runs in torch and
    is rounded to the dtype before the kernel: the bound is that of v1 on the rounded gelu(x))."""
    N, HW, C = 5, 35, 264
    x, gamma, beta, _ = grn_inputs(N, HW, C, dtype, cuda)
    y = ops.grn_nhwc(x.reshape(N, 5, 7, C), gamma, beta, pre_gelu=pre_gelu)
    _ran_native("grn")
    ref, tol = grn_bound(x, gamma, beta, pre_gelu, grn_depth("v2", N, HW, C))
    assert_within(y.reshape(N, HW, C), ref, tol, f"ops.grn_nhwc v2 {N}x{HW}x{C} gelu={pre_gelu} {dtype}")
    N, HW, C = 65, 17, 72
    x, gamma, beta, _ = grn_inputs(N, HW, C, dtype, cuda)
    y = ops.grn_nhwc(x.reshape(N, 1, 17, C), gamma, beta, pre_gelu=pre_gelu)
    _ran_native("grn")
    xa = torch.nn.functional.gelu(x) if pre_gelu else x
    ref, tol = grn_bound(xa, gamma, beta, False, grn_depth("v1", N, HW, C))
    assert_within(y.reshape(N, HW, C), ref, tol, f"ops.grn_nhwc v1 {N}x{HW}x{C} gelu={pre_gelu} {dtype}")


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=IDS3)
def test_grn_v1_bound(cuda, dtype, monkeypatch):
    """The v1 kernel (atomics) through ops.grn_nhwc: fp32 goes there by itself, bf16 / fp16 with v2 reported missing."""
    N, HW, C = 3, 35, 264
    has = _native.has_kernel
    monkeypatch.setattr(_native, "has_kernel", lambda name: name != "cgs_grn_nhwc_v2" and has(name))
    x, gamma, beta, _ = grn_inputs(N, HW, C, dtype, cuda)
    y = ops.grn_nhwc(x.reshape(N, 5, 7, C), gamma, beta)
    _ran_native("grn")
    ref, tol = grn_bound(x, gamma, beta, False, grn_depth("v1", N, HW, C))
    assert_within(y.reshape(N, HW, C), ref, tol, f"grn_v1 {N}x{HW}x{C} {dtype}")


# ------------------------------------------------------------------------------------------------ GRN from GNS partials
def _parts(h):
    N, HW, C = h.shape
    return h.float().pow(2).reshape(N, HW // 64, 64, C).sum(2).contiguous()


@pytest.mark.parametrize("N,HW,C", GRN_GNS_SHAPES)
def test_grn_apply_gns_bound(cuda, N, HW, C):
    """(5, 64, 264): one partial, N > 4, a bsum tail; (2, 320, 2048): nbk = 5, the 4-chain loop and its tail, the
    row-tiled apply."""
    lib = _native.load_kernels()
    h, gamma, beta, _ = grn_inputs(N, HW, C, BF, cuda)
    part, nblk = _parts(h), (C + 255) // 256
    assert (HW // 64) % 4 == 1 and grn_row_tiled(HW, C) == (C == 2048)
    yp, ydone = _out(cuda, N * HW * C, BF)
    wp, wdone = _out(cuda, N * (C + nblk), torch.float32)
    assert lib.cgs_grn_apply_gns(h.data_ptr(), part.data_ptr(), gamma.data_ptr(), beta.data_ptr(), yp, wp, N, HW, C,
                                 core._stream()) == 0
    what = f"grn_apply_gns {N}x{HW}x{C}"
    y, ws = ydone(what + " y").reshape(N, HW, C), wdone(what + " ws")
    gx, bsum = ws[:N * C].reshape(N, C), ws[N * C:].reshape(N, nblk)
    L, Lm = grn_depth("gns", N, HW, C)
    gref, gtol, iref, itol = grn_stats_bound(None, False, (L, Lm), part=part)
    assert_within(gx, gref, gtol, what + " gx")
    assert_within(_inv(bsum, C), iref, itol, what + " inv from bsum")
    ref, tol = grn_apply_bound(h, gamma, beta, gx, bsum)
    assert_within(y, ref, tol, what + " apply")
    ref, tol = grn_bound(h, gamma, beta, False, (L + 65, Lm))       # torch's block sums: 64 + 1 more roundings
    assert_within(y, ref, tol, what + " against h")
    h4 = h.reshape(N, HW // 16, 16, C)                               # through ops: the partials attached to the tensor
    h4._cgs_grnpart = (part, h4.data_ptr(), HW)
    y2 = ops.grn_nhwc(h4, gamma, beta)
    _ran_native("grn")
    assert torch.equal(y2.reshape(N, HW, C), y)


@pytest.mark.parametrize("N,HW,C", GRN_GNS_SHAPES)
def test_grn_stats_routes_and_scale_weight_bound(cuda, N, HW, C):
    """cgs_grn_stats_gns -> cgs_grn_scale_weight against cgs_grn_stats -> cgs_grn_scale_weight, O = 24."""
    lib = _native.load_kernels()
    O = 24
    h, gamma, beta, _ = grn_inputs(N, HW, C, BF, cuda)
    torch.manual_seed(1)
    W = torch.randn(O, C, device=cuda).to(BF)
    part, nblk, S = _parts(h), (C + 255) // 256, grn_slices(N, HW, C)
    L, Lm = grn_depth("gns", N, HW, C)
    res = {}
    for route in ("stats", "gns"):
        wp, wdone = _out(cuda, N * ((S + 1) * C + nblk), torch.float32)
        if route == "stats":
            assert lib.cgs_grn_stats(h.data_ptr(), wp, N, HW, C, 0, core._DT[BF], core._stream()) == 0
            depth = grn_depth("v2", N, HW, C)
        else:
            assert lib.cgs_grn_stats_gns(part.data_ptr(), wp, N, HW, C, core._stream()) == 0
            depth = (L + 65, Lm)
        op, odone = _out(cuda, N * O * C, BF)
        assert lib.cgs_grn_scale_weight(W.data_ptr(), gamma.data_ptr(), wp, N, HW, O, C, op, core._stream()) == 0
        what = f"grn_scale_weight/{route} {N}x{O}x{C}"
        Wn, ws = odone(what).reshape(N, O, C), wdone(what + " ws")
        gx, bsum = ws[N * S * C:N * (S + 1) * C].reshape(N, C), ws[N * (S + 1) * C:].reshape(N, nblk)
        gref, gtol, iref, itol = grn_stats_bound(h, False, depth)
        assert_within(gx, gref, gtol, what + " gx")
        assert_within(_inv(bsum, C), iref, itol, what + " inv from bsum")
        ref, tol = grn_scale_weight_bound(W, gamma, gx, _inv(bsum, C))
        assert_within(Wn, ref, tol, what)
        res[route] = (Wn, ref, tol, gtol * iref[:, None] + gref * itol[:, None])
    dnx = res["stats"][3] + res["gns"][3]
    tol = res["stats"][2] + (f64(W)[None] * f64(gamma)[None, None]).abs() * dnx[:, None, :] * (1 + u(BF))
    assert_within(res["gns"][0], res["stats"][1], tol, f"grn_scale_weight gns against the stats route {N}x{O}x{C}")
    Wn = ops.grn_fold_weight(h.reshape(N, HW // 16, 16, C), W, gamma)
    _ran_native("grn")
    assert torch.equal(Wn, res["stats"][0])


# ------------------------------------------------------------------------------------------------ resize
_MODE = {"nearest": 0, "nearest-exact": 1, "bilinear": 2, "bicubic": 3, "area": 4}


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=IDS3)
@pytest.mark.parametrize("mode,align", RESIZE_MODES)
def test_resize_bound(cuda, mode, align, dtype):
    lib = _native.load_kernels()
    for shape, (Ho, Wo) in RESIZE_CASES:
        torch.manual_seed(0)
        x = (torch.randn(*shape, device=cuda) * 2 + 0.5).to(dtype)
        N, C, H, W = shape
        yp, ydone = _out(cuda, N * C * Ho * Wo, dtype)
        assert lib.cgs_resize(x.data_ptr(), yp, N * C, H, W, Ho, Wo, _MODE[mode], int(bool(align)), core._DT[dtype],
                              core._stream()) == 0
        what = f"resize {mode} align={align} {shape}->{(Ho, Wo)} {dtype}"
        y = ydone(what).reshape(N, C, Ho, Wo)
        ref, tol = resize_bound(x, (Ho, Wo), mode, align)
        assert_within(y, ref, tol, what)
        if mode.startswith("nearest"):
            assert bool((tol == 0).all())
    y2 = ops.interpolate(x, (Ho, Wo), mode, align_corners=align)
    _ran_native("resize")
    assert torch.equal(y2, y)


# ------------------------------------------------------------------------------------------------ upfirdn2d
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=IDS3)
@pytest.mark.parametrize("kname", list(UPFIRDN_KERNELS))
def test_upfirdn2d_bound(cuda, kname, dtype):
    lib = _native.load_kernels()
    torch.manual_seed(0)
    x = torch.randn(2, 3, 9, 6, device=cuda).to(dtype)
    kh, kw = UPFIRDN_KERNELS[kname]
    k = upfirdn_kernel(kh, kw).to(cuda)
    N, C, H, W = x.shape
    for (ux, uy), (dx, dy), (px0, px1, py0, py1) in UPFIRDN_CFGS:
        Ho, Wo = (H * uy + py0 + py1 - kh) // dy + 1, (W * ux + px0 + px1 - kw) // dx + 1
        yp, ydone = _out(cuda, N * C * Ho * Wo, dtype)
        assert lib.cgs_upfirdn2d(x.data_ptr(), k.data_ptr(), yp, N * C, H, W, ux, uy, dx, dy, px0, px1, py0, py1, kh,
                                 kw, core._DT[dtype], core._stream()) == 0
        what = f"upfirdn2d {kname} up={(ux, uy)} down={(dx, dy)} pad={(px0, px1, py0, py1)} {dtype}"
        y = ydone(what).reshape(N, C, Ho, Wo)
        ref, tol = upfirdn2d_bound(x, k, (ux, uy), (dx, dy), (px0, px1, py0, py1))
        assert tuple(ref.shape) == (N, C, Ho, Wo)
        assert_within(y, ref, tol, what)
    y2 = ops.upfirdn2d(x, k, up=(ux, uy), down=(dx, dy), pad=(px0, px1, py0, py1))
    _ran_native("upfirdn2d")
    assert torch.equal(y2, y)


# ------------------------------------------------------------------------------------------------ fused_bias_act
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=IDS3)
@pytest.mark.parametrize("shape", FBA_SHAPES)
def test_fused_bias_act_bound(cuda, shape, dtype):
    lib = _native.load_kernels()
    torch.manual_seed(0)
    x, b = torch.randn(*shape, device=cuda).to(dtype), torch.randn(shape[1], device=cuda).to(dtype)
    C, inner, scale = shape[1], math.prod(shape[2:]), 2 ** 0.5
    for slope in (0.2, 0.0):
        for bias in (b, None):
            yp, ydone = _out(cuda, x.numel(), dtype)
            assert lib.cgs_fused_bias_act(x.data_ptr(), core._ptr(bias), yp, x.numel(), C, inner, slope, scale,
                                          core._DT[dtype], core._stream()) == 0
            what = f"fused_bias_act {shape} slope={slope} bias={bias is not None} {dtype}"
            y = ydone(what).reshape(shape)
            ref, tol = fused_bias_act_bound(x, bias, slope, scale)
            assert_within(y, ref, tol, what)
    y2 = ops.fused_bias_act(x, None, 0.0, scale)
    _ran_native("fused_bias_act")
    assert torch.equal(y2, y)


# ------------------------------------------------------------------------------------------------ softmax_rows
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=IDS3)
@pytest.mark.parametrize("cols", SMR_COLS)
def test_softmax_rows_bound(cuda, cols, dtype):
    lib = _native.load_kernels()
    for rows in SMR_ROWS:
        x = smr_inputs(rows, cols, dtype, cuda, seed=rows)
        for scale in (0.125, 1.0):
            yp, ydone = _out(cuda, rows * cols, torch.float32)
            assert lib.cgs_softmax_rows(x.data_ptr(), yp, rows, cols, scale, core._DT[dtype], core._stream()) == 0
            what = f"softmax_rows {rows}x{cols} scale={scale} {dtype}"
            y = ydone(what).reshape(rows, cols)
            ref, tol = softmax_rows_bound(x, scale)
            assert_within(y, ref, tol, what)
    y2 = ops.softmax_rows(x, 1.0)
    _ran_native("softmax")
    assert torch.equal(y2, y)


# ------------------------------------------------------------------------------------------------ tome_match
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS2)
@pytest.mark.parametrize("B,Na,Nb,C", TOME_SHAPES)
def test_tome_match_bound(cuda, B, Na, Nb, C, dtype):
    lib = _native.load_kernels()
    a, b = tome_inputs(B, Na, Nb, C, dtype, cuda)
    assert a.stride(1) == C + 24 and b.stride(1) == C + 24 and a.stride(2) == 1
    wp, wdone = _out(cuda, B * (Na + Nb), torch.float32)
    vp, vdone = _out(cuda, B * Na, torch.float32)
    ip, idone = _out(cuda, B * Na, torch.int64)
    assert lib.cgs_tome_match(a.data_ptr(), b.data_ptr(), wp, vp, ip, B, Na, Nb, C, a.stride(0), a.stride(1),
                              b.stride(0), b.stride(1), core._DT[dtype], core._stream()) == 0
    what = f"tome_match {B}x{Na}x{Nb}x{C} {dtype}"
    vmax, imax, ws = vdone(what + " vmax").reshape(B, Na), idone(what + " imax").reshape(B, Na), wdone(what + " ws")
    assert_tome(vmax, imax, a, b, what)
    inv = torch.cat([1 / f64(a).norm(dim=-1).reshape(-1), 1 / f64(b).norm(dim=-1).reshape(-1)])
    fin = torch.isfinite(inv)
    assert bool((ws[~fin] == 0).all())
    Ln = (C + 63) // 64 + 6                   # the row norms: a sum of squares of depth Ln, halved by the root, rsqrtf
    assert ((ws.double() - inv)[fin].abs() <= (C_ACC * (Ln + 1) / 2 + 2) * E * inv[fin]).all()
    if Na > 1:
        assert bool((vmax[:, -1] == 0).all()) and bool((imax[:, 0] == 0).all())
    v2, i2 = ops.tome_match(a, b)
    _ran_native("tome")
    assert torch.equal(v2, vmax) and torch.equal(i2, imax)
