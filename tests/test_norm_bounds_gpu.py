"""Per-element error bounds (tests/_bounds.py) on the device for the GroupNorm, LayerNorm, depthwise-conv and
softmax2 kernels, in bf16 and fp16 (softmax2: bf16 only).

The shapes are the smallest that reach each path: every form of the GroupNorm statistics kernel (gn_slices and
gn_pix_per_block of csrc/kernels/norm.hip are mirrored below and the selected form is asserted per case), a tail
block, 1 x 1 and 1 x 3 maps, a dual-source seam inside a group and inside a slice, a strided pre-add, the apply
loop's second trip; each lanes-per-row form of the LayerNorm kernels on both sides of its limit; the 1 / 2 / 4
pixels-per-thread depthwise forms; every registers-per-thread form of softmax2. The inputs carry spikes of +-48
where an index can go wrong: the last pixel of a statistics block, the first and last element of a row, both sides
of an image boundary and of the dual-source seam. References are fp64 on the device. The guard tests put the
output in the middle of a pattern-filled buffer and require everything around it to keep its bits."""
import math

import pytest
import torch

from comfy_gen_server_amd import ops, _native
from comfy_gen_server_amd.ops import core

from _bounds import (affine_layernorm_bound, assert_within, dwconv_bound, groupnorm_apply_bound, groupnorm_bound,
                     groupnorm_stats_bound, layernorm_bound, layernorm_stats_bound, rs_from_partials_bound,
                     softmax2_bound)
from _guards import GN_BLOCKS, _check_guard, _guarded, _native_loaded, _ran_native  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DTYPES = [torch.bfloat16, torch.float16]
SPIKE = 48.0


# ------------------------------------------------------------------------------------------------ GroupNorm
def _gn_slices(C):           # gn_slices (norm.hip)
    ns0 = (C + 2047) // 2048
    if 512 < C <= 1024 and C % 16 == 0:
        return 2
    if C <= 1024 or C % 8:
        return ns0
    tot, best, bu = C // 8, ns0, -1.0
    for ns in range((C + 511) // 512, tot + 1):
        if tot % ns:
            continue
        nch = tot // ns
        lanes = 8 if nch <= 8 else 16 if nch <= 16 else 32 if nch <= 32 else 64
        if nch / lanes >= 0.9:
            return ns
        if nch / lanes > bu:
            bu, best = nch / lanes, ns
    return best


def _gn_form(C):             # groupnorm_impl: (slices, channels per slice, statistics kernel form)
    ns = _gn_slices(C)
    nch = C // ns // 8
    form = "PK8" if nch <= 8 else "PK4" if nch <= 16 else "PK2" if nch <= 32 else f"KM{(nch + 63) // 64}"
    return ns, C // ns, form


def _gn_ppb(N, HW):          # gn_pix_per_block
    per_n = (GN_BLOCKS + N - 1) // N
    ppb = max(16, (HW + per_n - 1) // per_n)
    return 64 if N <= 4 and ppb < 64 else ppb


# C, G -> (slices, channels per slice, form)
GN_FORMS = {(64, 32): (1, 64, "PK8"), (128, 32): (1, 128, "PK4"), (256, 32): (1, 256, "PK2"),
            (320, 32): (1, 320, "KM1"), (512, 32): (1, 512, "KM1"), (520, 8): (1, 520, "KM2"),
            (1016, 8): (1, 1016, "KM2"), (640, 32): (2, 320, "KM1"), (1032, 8): (3, 344, "KM1"),
            (1048, 8): (131, 8, "PK8"), (1280, 32): (5, 256, "PK2"), (1920, 32): (4, 480, "KM1"),
            (2560, 32): (5, 512, "KM1")}
# N, H, W -> (pixels per block, blocks, pixels of the last block)
GN_MAPS = {(2, 13, 15): (64, 4, 3), (5, 13, 15): (16, 13, 3), (2, 1, 1): (64, 1, 1), (2, 1, 3): (64, 1, 3)}


def test_groupnorm_form_mirror():
    """Every reachable KM > 1 form is KM = 2, on exactly the 32 channel counts 512 < C <= 1024 with C % 16 == 8."""
    km = {C: _gn_form(C)[2] for C in range(8, 8193, 8)}
    assert {f for f in km.values() if f.startswith("KM")} == {"KM1", "KM2"}
    assert [C for C, f in km.items() if f == "KM2"] == list(range(520, 1017, 16))


def _gn_inputs(cuda, N, C, H, W, dtype, ppb, seam=None, seed=0):
    """x as NHWC rows [N, HW, C] = 3 randn + 1 with the spikes of the module docstring; gamma, beta; pre_add."""
    torch.manual_seed(seed)
    HW = H * W
    xr = torch.randn(N, HW, C, device=cuda) * 3 + 1
    for p in list(range(ppb - 1, HW, ppb)) + [HW - 1]:
        xr[:, p, 0] = SPIKE
        xr[:, p, C - 1] = -SPIKE
    xr[:, 0, 0] = xr[:, -1, -1] = SPIKE
    xr[:, 0, -1] = xr[:, -1, 0] = -SPIKE
    if seam:
        xr[:, HW // 2, seam - 1] = SPIKE
        xr[:, HW // 2, seam] = -SPIKE
    x = xr.to(dtype).reshape(N, H, W, C).permute(0, 3, 1, 2)
    w = (torch.randn(C, device=cuda) + 1).to(dtype)
    b = torch.randn(C, device=cuda).to(dtype)
    pre = torch.randn(N, C, device=cuda).to(dtype)
    return x, w, b, pre


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("C,G", list(GN_FORMS))
def test_groupnorm_bound(cuda, C, G, dtype):
    assert _gn_form(C) == GN_FORMS[(C, G)]
    for (N, H, W), (ppb, nb, tail) in GN_MAPS.items():
        HW = H * W
        assert (_gn_ppb(N, HW), (HW + ppb - 1) // ppb, HW - (nb - 1) * ppb) == (ppb, nb, tail)
        x, w, b, pre = _gn_inputs(cuda, N, C, H, W, dtype, ppb)
        for silu in (False, True):
            for pa in (None, pre):
                y = ops.group_norm(x, G, w, b, 1e-5, silu=silu, pre_add=pa)
                _ran_native("groupnorm")
                ref, tol = groupnorm_bound(x, G, w, b, 1e-5, silu, pa, ppb=ppb)
                assert_within(y, ref, tol, f"groupnorm/{GN_FORMS[(C, G)][2]} C={C} G={G} {N}x{H}x{W} {dtype} "
                                           f"silu={silu} pre={pa is not None}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("C1,C2,G", [(192, 128, 32), (640, 640, 32)])
def test_groupnorm_bound_dual_source(cuda, C1, C2, G, dtype):
    """cat([x, x2], 1) read in place: the seam inside a group (192 + 128: 10 channels per group) and inside a
    256-channel statistics slice (640 + 640)."""
    C = C1 + C2
    ns, CS, _ = _gn_form(C)
    assert C1 % (C // G) or C1 % CS
    for (N, H, W), (ppb, nb, tail) in GN_MAPS.items():
        x, w, b, pre = _gn_inputs(cuda, N, C, H, W, dtype, ppb, seam=C1)
        cl = lambda t: t.contiguous(memory_format=torch.channels_last)
        xa, xb = cl(x[:, :C1]), cl(x[:, C1:])
        for silu, pa in ((True, pre), (False, None)):
            y = ops.group_norm(xa, G, w, b, 1e-5, silu=silu, pre_add=pa, x2=xb)
            _ran_native("groupnorm")
            ref, tol = groupnorm_bound(xa, G, w, b, 1e-5, silu, pa, x2=xb, ppb=ppb)
            assert_within(y, ref, tol, f"groupnorm/dual {C1}+{C2} G={G} {N}x{H}x{W} {dtype} silu={silu}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("N", [2, 1])
def test_groupnorm_bound_strided_pre_add(cuda, N, dtype):
    """pre_add as a column slice of a [N, 1000] tensor, read in place through its row stride."""
    C, G, H, W = 320, 32, 13, 15
    ppb = _gn_ppb(N, H * W)
    x, w, b, _ = _gn_inputs(cuda, N, C, H, W, dtype, ppb)
    wide = torch.randn(N, 1000, device=cuda).to(dtype)
    pre = wide[:, 104:104 + C]
    assert not pre.is_contiguous() or N == 1
    before = wide.clone()
    for x2 in (None, x[:, 192:].contiguous(memory_format=torch.channels_last)):
        xa = x if x2 is None else x[:, :192].contiguous(memory_format=torch.channels_last)
        y = ops.group_norm(xa, G, w, b, 1e-5, silu=True, pre_add=pre, x2=x2)
        _ran_native("groupnorm")
        ref, tol = groupnorm_bound(xa, G, w, b, 1e-5, True, pre, x2=x2, ppb=ppb)
        assert_within(y, ref, tol, f"groupnorm/strided pre_add N={N} {dtype} dual={x2 is not None}")
    assert torch.equal(wide, before)


def test_groupnorm_bound_conv_epilogue_statistics(cuda):
    """cgs_groupnorm_nhwc_part on the (mean, M2) partials the v6 conv epilogue wrote for its stored output: the
    bound is the GroupNorm of that output (64-pixel blocks; a two-pass M2 is within the shifted-sum bound)."""
    lib = _native.load_kernels()
    torch.manual_seed(3)
    N, H, W, Cin, Cout, G = 2, 16, 32, 128, 160, 32
    HW = H * W
    x = (torch.rand(N, H, W, Cin, device=cuda) * 2 - 1).to(BF)
    w = ((torch.rand(Cout, 3, 3, Cin, device=cuda) * 2 - 1) / math.sqrt(Cin * 9)).to(BF)
    b = (torch.randn(Cout, device=cuda) + 2).to(BF)
    g, be = torch.randn(Cout, device=cuda).to(BF), torch.randn(Cout, device=cuda).to(BF)
    pre = torch.randn(N, Cout, device=cuda).to(BF)
    out = torch.empty(N, H, W, Cout, device=cuda, dtype=BF)
    gnp = torch.full((N * (HW // 64) * Cout * 2,), float("nan"), device=cuda)
    ab = torch.empty(N * Cout * 2, device=cuda)
    y = torch.empty_like(out)
    st = core._stream()
    assert lib.cgs_conv2d_nhwc_gns(x.data_ptr(), None, Cin, w.data_ptr(), b.data_ptr(), None, out.data_ptr(), N, H, W,
                                   Cin, Cout, 3, 3, 1, 1, H, W, 0, gnp.data_ptr(), st) == 0
    assert lib.cgs_groupnorm_nhwc_part(out.data_ptr(), y.data_ptr(), g.data_ptr(), be.data_ptr(), pre.data_ptr(),
                                       gnp.data_ptr(), ab.data_ptr(), N, HW, Cout, G, 64, 1e-5, 1, core._DT[BF],
                                       st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gnp).all())
    ref, tol = groupnorm_bound(out.permute(0, 3, 1, 2), G, g, be, 1e-5, True, pre, ppb=64)
    assert_within(y.permute(0, 3, 1, 2), ref, tol, f"groupnorm/conv-epilogue statistics {N}x{Cout}x{H}x{W}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_groupnorm_bound_apply_loop_wraps(cuda, dtype):
    """N HW C / 8 > 2 * 8192 * 256 vectors: the apply kernel's paired trip, its remainder and an image boundary
    inside one grid stride."""
    N, C, H, W, G = 3, 64, 432, 432, 32
    assert N * H * W * C // 8 > 2 * 8192 * 256
    ppb = _gn_ppb(N, H * W)
    x, w, b, pre = _gn_inputs(cuda, N, C, H, W, dtype, ppb)
    y = ops.group_norm(x, G, w, b, 1e-5, silu=True, pre_add=pre)
    _ran_native("groupnorm")
    ref, tol = groupnorm_bound(x, G, w, b, 1e-5, True, pre, ppb=ppb)
    assert_within(y, ref, tol, f"groupnorm/apply wrap {N}x{C}x{H}x{W} {dtype}")


def _band_stats(lib, x, x2, pre, N, HW, C, G, dtype):
    ws = torch.empty((int(lib.cgs_groupnorm_workspace(N, HW, C)) + 3) // 4, device=x.device, dtype=torch.float32)
    stats = torch.full((N, G, 2), float("nan"), device=x.device)
    assert lib.cgs_groupnorm_band_stats(x.data_ptr(), core._ptr(x2), x.shape[1], core._ptr(pre), ws.data_ptr(),
                                        stats.data_ptr(), N, HW, C, G, core._DT[dtype], core._stream()) == 0
    return stats


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("C1,C2,G", [(320, 0, 32), (520, 0, 8), (192, 128, 32), (1280, 0, 32)])
def test_groupnorm_band_stats_and_apply_bound(cuda, C1, C2, G, dtype):
    """The two halves of the row-sharded GroupNorm: fp32 (mean, M2) per (n, g) from cgs_groupnorm_band_stats, and
    cgs_groupnorm_apply_stats with given fp32 (mean, rstd); the latter writes into a guarded buffer."""
    lib = _native.load_kernels()
    C = C1 + C2
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    for (N, H, W), (ppb, nb, tail) in GN_MAPS.items():
        HW = H * W
        x, w, b, pre = _gn_inputs(cuda, N, C, H, W, dtype, ppb, seam=C1 if C2 else None)
        xa, xb = (cl(x[:, :C1]), cl(x[:, C1:])) if C2 else (cl(x), None)
        for pa in (None, pre):
            stats = _band_stats(lib, xa, xb, pa, N, HW, C, G, dtype)
            ref, tol = groupnorm_stats_bound(xa, G, pa, x2=xb, ppb=ppb)
            what = f"{C1}+{C2} G={G} {N}x{H}x{W} {dtype} pre={pa is not None}"
            assert_within(stats, ref, tol, "groupnorm/band stats " + what)
            mr = torch.stack([ref[..., 0], 1 / torch.sqrt(ref[..., 1] / (HW * C // G) + 1e-5)], -1).float().contiguous()
            ab = torch.empty(N * C * 2, device=cuda)
            buf, before, yp = _guarded(cuda, N * HW * C, 4096)
            assert lib.cgs_groupnorm_apply_stats(xa.data_ptr(), core._ptr(xb), C1, yp, w.data_ptr(), b.data_ptr(),
                                                 core._ptr(pa), mr.data_ptr(), ab.data_ptr(), N, HW, C, G, 1,
                                                 core._DT[dtype], core._stream()) == 0
            keep = torch.ones(N * HW * C, dtype=torch.bool, device=cuda)
            y = _check_guard(buf, before, keep, dtype, "groupnorm apply").reshape(N, H, W, C).permute(0, 3, 1, 2)
            ref, tol = groupnorm_apply_bound(xa, G, w, b, mr, True, pa, x2=xb)
            assert_within(y, ref, tol, "groupnorm/apply stats " + what)


# ------------------------------------------------------------------------------------------------ LayerNorm
# cgs_layernorm: 8 lanes per row up to C = 512, 16 to 1024, 32 to 2048, 64 to 4096, the scalar kernel above.
LN_CS = [8, 72, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104, 5120]
LN_ROWS = [1, 33, 257]


def _ln_lanes(C):
    nch = C // 8
    return 8 if nch <= 64 else 16 if nch <= 128 else 32 if nch <= 256 else 64 if nch <= 512 else 0


def _ln_inputs(cuda, rows, C, dtype, mean=0.5, spread=2.0, spike=SPIKE, seed=0):
    torch.manual_seed(seed)
    x = torch.randn(rows, C, device=cuda) * spread + mean
    if spike:
        x[:, 0] = mean + spike
        x[:, -1] = mean - spike
    return x.to(dtype), (torch.randn(C, device=cuda) + 1).to(dtype), torch.randn(C, device=cuda).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("C", LN_CS)
def test_layernorm_bound(cuda, C, dtype):
    assert [_ln_lanes(c) for c in LN_CS] == [8, 8, 8, 16, 16, 32, 32, 64, 64, 0, 0]
    for rows in LN_ROWS:
        x, w, b = _ln_inputs(cuda, rows, C, dtype)
        for wi, bi in ((w, b), (w, None), (None, None)):
            y = ops.layer_norm(x, wi, bi, 1e-5)
            _ran_native("layernorm")
            ref, tol = layernorm_bound(x, wi, bi, 1e-5)
            assert_within(y, ref, tol, f"layernorm C={C} rows={rows} {dtype} w={wi is not None} b={bi is not None}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("C", [72, 2048, 5120])
def test_layernorm_bound_large_mean(cuda, C, dtype):
    """Rows of mean 200 and spread 0.5: a one-pass variance is off by whole percents here."""
    x, w, b = _ln_inputs(cuda, 33, C, dtype, mean=200.0, spread=0.5, spike=0.0)
    y = ops.layer_norm(x, w, b, 1e-5)
    _ran_native("layernorm")
    ref, tol = layernorm_bound(x, w, b, 1e-5)
    assert_within(y, ref, tol, f"layernorm C={C} mean 200 spread 0.5 {dtype}")
    if C <= 2048:
        rs = ops.layernorm_stats(x, 1e-5)
        _ran_native("layernorm")
        ref, tol = layernorm_stats_bound(x, 1e-5)
        assert_within(rs, ref, tol, f"layernorm_stats C={C} mean 200 spread 0.5 {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("C", [8, 520, 1032, 2056, 5120])
def test_layernorm_writes_only_its_rows(cuda, C, dtype):
    """33 rows: the last block of every lanes-per-row form has dead rows, which must not be stored."""
    lib = _native.load_kernels()
    rows = 33
    x, w, b = _ln_inputs(cuda, rows, C, dtype)
    buf, before, yp = _guarded(cuda, rows * C, 32 * C)
    assert lib.cgs_layernorm(x.data_ptr(), yp, w.data_ptr(), b.data_ptr(), rows, C, 1e-5, core._DT[dtype],
                             core._stream()) == 0
    y = _check_guard(buf, before, torch.ones(rows * C, dtype=torch.bool, device=cuda), dtype, f"layernorm C={C}")
    ref, tol = layernorm_bound(x, w, b, 1e-5)
    assert_within(y.reshape(rows, C), ref, tol, f"layernorm guarded C={C} {dtype}")


@pytest.mark.parametrize("case", ["f32_params", "bias_only", "strided_weight"])
def test_layernorm_parameter_normalisation(cuda, case):
    """ops.layer_norm brings weight and bias to x's dtype, contiguous, each on its own."""
    rows, C = 33, 520
    x, w, b = _ln_inputs(cuda, rows, C, BF)
    if case == "f32_params":
        wi, bi = torch.randn(C, device=cuda) + 1, torch.randn(C, device=cuda)
    elif case == "bias_only":
        wi, bi = w, torch.randn(C, device=cuda)
    else:
        wi, bi = (torch.randn(2 * C, device=cuda) + 1).to(BF)[::2], b
        assert not wi.is_contiguous()
    y = ops.layer_norm(x, wi, bi, 1e-5)
    _ran_native("layernorm")
    ref, tol = layernorm_bound(x, wi.to(BF), bi.to(BF), 1e-5)
    assert_within(y, ref, tol, f"layernorm parameters {case}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("C", [8, 72, 520, 1032, 2048])
def test_layernorm_stats_bound(cuda, C, dtype):
    for rows in LN_ROWS:
        x, _, _ = _ln_inputs(cuda, rows, C, dtype)
        rs = ops.layernorm_stats(x, 1e-5)
        _ran_native("layernorm")
        ref, tol = layernorm_stats_bound(x, 1e-5)
        assert_within(rs, ref, tol, f"layernorm_stats C={C} rows={rows} {dtype}")


def test_layernorm_stats_rejects_wide_rows(cuda):
    x, _, _ = _ln_inputs(cuda, 4, 2056, BF)
    with pytest.raises(RuntimeError, match="cgs_layernorm_stats"):
        ops.layernorm_stats(x, 1e-5)


@pytest.mark.parametrize("M", [1, 257])
@pytest.mark.parametrize("P,misaligned", [(1, False), (2, False), (3, False), (8, False), (10, False), (16, False),
                                          (18, False), (8, True)])
def test_ln_rs_from_partials_bound(cuda, M, P, misaligned):
    """The 16-byte forms (P even, <= 8 and <= 16), the loop form (P odd, P > 16, or a part pointer off 16 bytes)."""
    lib = _native.load_kernels()
    x, _, _ = _ln_inputs(cuda, M, 80 * P, BF, mean=40.0)
    xg = x.double().reshape(M, P, 80)
    m = xg.mean(-1)
    store = torch.zeros(M * P * 2 + 4, device=cuda)
    part = store[2:2 + M * P * 2] if misaligned else store[:M * P * 2]
    part.copy_(torch.stack([m, ((xg - m[..., None]) ** 2).sum(-1)], -1).float().reshape(-1))
    assert part.data_ptr() % 16 == (8 if misaligned else 0)
    rs = torch.full((M, 2), float("nan"), device=cuda)
    assert lib.cgs_ln_rs_from_partials(part.data_ptr(), rs.data_ptr(), M, P, 1e-5, core._stream()) == 0
    ref, tol = rs_from_partials_bound(part.reshape(M, P, 2), 1e-5)
    assert_within(rs, ref, tol, f"ln_rs_from_partials M={M} P={P} misaligned={misaligned}")
    full, _ = layernorm_stats_bound(x, 1e-5)
    assert (ref - full).abs().max().item() < 1e-4


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("C", [64, 1280, 4096])
def test_channel_affine_layernorm_bound(cuda, C, dtype):
    """HW = 35: a row group of the kernel spans two images. Scale and shift: the halves of one [N, 2 C] tensor."""
    N, H, W = 3, 5, 7
    torch.manual_seed(0)
    x = torch.randn(N, H, W, C, device=cuda) * 2 + 0.5
    x[:, 0, 0, 0] = x[:, -1, -1, -1] = SPIKE
    x[:, 0, 0, -1] = x[:, -1, -1, 0] = -SPIKE
    x = x.to(dtype)
    co = (torch.randn(N, 2 * C, device=cuda) * 0.5).to(dtype)
    sc, sh = co[:, :C], co[:, C:]
    xa, y = ops.channel_affine_layernorm_nhwc(x, sc, sh, add=1.0, eps=1e-6)
    st = ops.stats()
    assert st.get(("channel_affine", "hip"), 0) == 1 and st.get(("layernorm", "hip"), 0) == 1, st
    xa_ref, xa_tol, y_ref, y_tol = affine_layernorm_bound(x, sc, sh, 1.0, 1e-6, xa)
    assert_within(xa, xa_ref, xa_tol, f"affine_layernorm xa C={C} {dtype}")
    assert_within(y, y_ref, y_tol, f"affine_layernorm y C={C} {dtype}")


# ------------------------------------------------------------------------------------------------ depthwise conv
def _dw_inputs(cuda, N, H, W, C, k, dtype, seed=0):
    torch.manual_seed(seed)
    x = torch.randn(N, H, W, C, device=cuda) + 0.5
    x[:, 0, 0, 0] = x[:, -1, -1, -1] = SPIKE
    x[:, 0, -1, -1] = x[:, -1, 0, 0] = -SPIKE
    w = (torch.randn(k * k, C, device=cuda) / k).to(dtype)
    return x.to(dtype), w, torch.randn(C, device=cuda).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("C", [64, 320, 2048])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_dwconv_lnstats_bound(cuda, k, C, dtype):
    for H, W in ((1, 1), (5, 6), (17, 9)):
        x, w, b = _dw_inputs(cuda, 2, H, W, C, k, dtype)
        for replicate in (False, True):
            for bias in (b, None):
                y, rs = ops.depthwise_conv2d_nhwc_lnstats(x, w, bias, k, 1e-6, replicate=replicate)
                _ran_native("dwconv")
                what = f"k={k} C={C} {H}x{W} {dtype} replicate={replicate} bias={bias is not None}"
                ref, tol = dwconv_bound(x, w, bias, k, replicate)
                assert_within(y, ref, tol, "dwconv_lnstats y " + what)
                ref, tol = layernorm_stats_bound(y, 1e-6)
                assert_within(rs, ref, tol, "dwconv_lnstats (mean, rstd) " + what)


def _dw_px(W):               # cgs_dwconv_nhwc at the default of 4 pixels per thread (3 x 3, zero padding only)
    return 4 if W % 4 == 0 else 1 if W % 2 else 2


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("W", [4, 6, 7])
def test_dwconv_bound(cuda, W, dtype):
    assert [_dw_px(w_) for w_ in (4, 6, 7)] == [4, 2, 1]
    for H in (1, 5):
        for k in (3, 5, 7, 9):
            x, w, b = _dw_inputs(cuda, 2, H, W, 72, k, dtype)
            for replicate in (False, True):
                for bias in (b, None):
                    y = ops.depthwise_conv2d_nhwc(x, w, bias, k, replicate=replicate)
                    _ran_native("dwconv")
                    ref, tol = dwconv_bound(x, w, bias, k, replicate)
                    px = _dw_px(W) if k == 3 and not replicate else 1
                    assert_within(y, ref, tol, f"dwconv px={px} k={k} {H}x{W} {dtype} replicate={replicate} "
                                               f"bias={bias is not None}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("W", [4, 6, 7])
def test_dwconv_writes_only_its_output(cuda, W, dtype):
    lib = _native.load_kernels()
    N, H, C = 2, 5, 72
    x, w, b = _dw_inputs(cuda, N, H, W, C, 3, dtype)
    buf, before, yp = _guarded(cuda, x.numel(), 4096)
    assert lib.cgs_dwconv_nhwc(x.data_ptr(), w.data_ptr(), b.data_ptr(), yp, N, H, W, C, 3, 0, core._DT[dtype],
                               core._stream()) == 0
    y = _check_guard(buf, before, torch.ones(x.numel(), dtype=torch.bool, device=cuda), dtype, f"dwconv px={_dw_px(W)}")
    ref, tol = dwconv_bound(x, w, b, 3, False)
    assert_within(y.reshape(x.shape), ref, tol, f"dwconv guarded px={_dw_px(W)} {H}x{W} {dtype}")


# ------------------------------------------------------------------------------------------------ softmax2
@pytest.mark.parametrize("cols", [4, 1020, 1024, 1028, 2052, 4100, 8196, 16384])
def test_softmax2_bound(cuda, cols):
    """x [rows, ldx = cols + 4] fp32 in log2 units -> y [rows, ldy = cols + 8] bf16 inside a guarded buffer. Rows:
    a spike in the last column, a constant row, -inf entries, magnitudes around 1e4, plain noise."""
    lib = _native.load_kernels()
    rows, ldx, ldy = 6, cols + 4, cols + 8
    torch.manual_seed(cols)
    xs = torch.randn(rows, ldx, device=cuda) * 6
    x = xs[:, :cols]
    x[0, -1] += 30
    x[1] = 3.0
    x[2, ::2] = -math.inf
    x[3] = torch.randn(cols, device=cuda) * 1e4
    x[4] = 1e4 + torch.randn(cols, device=cuda)
    buf, before, yp = _guarded(cuda, rows * ldy, 4096)
    assert xs.data_ptr() % 16 == 0 and yp % 8 == 0
    assert lib.cgs_softmax2_f32_bf16(xs.data_ptr(), yp, rows, cols, ldx, ldy, core._stream()) == 0
    keep = torch.zeros(rows, ldy, dtype=torch.bool, device=cuda)
    keep[:, :cols] = True
    y = _check_guard(buf, before, keep, BF, f"softmax2 cols={cols}").reshape(rows, cols)
    ref, tol = softmax2_bound(x)
    assert_within(y, ref, tol, f"softmax2 cols={cols} ldx={ldx} ldy={ldy}")
    assert bool((y[2, ::2] == 0).all())
