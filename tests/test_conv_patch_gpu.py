"""The patch form of the 3 x 3 conv (variant 22, csrc/kernels/mfma_pp160p.h) against the per-element bound of the
conv kernels (tests/_bounds.py conv_bound, unchanged): zero elements over the bound, nothing written outside the
output or the GroupNorm partials.

Each case is the smallest shape that reaches one edge of the kernel: one partial patch holding all four borders
(5 x 7), 2 x 2 patches with seams and partial patches in both axes (17 x 19), exact patches (16 x 16, 32 x 16), one /
two / three 64-channel slabs (no swap, a buffer swap, an odd slab count), a partial column tile and two column tiles
(Cout = 8, 24, 168), an image boundary between consecutive units (N = 3) and more units than compute units (N = 5,
64 x 64, Cout = 640: 320 units) for the cross-unit prefetch. Every pixel of the input is distinct (a ramp over the
pixels plus noise), so a wrong neighbour cannot cancel. ``CGS_CONV_PATCH=1`` forces the form wherever ``ops.conv2d``
may take it; a spy on the library handle shows which launcher ran and with which variant."""
import faulthandler
import math

import pytest
import torch

from comfy_gen_server_amd import ops, _native
from comfy_gen_server_amd.ops import core

from _bounds import assert_within, conv_bound, gn_partials_bound, groupnorm_bound
from _guards import _check_guard, _guarded
from test_epilogue_bounds_gpu import _guards_kept, _nan_guarded

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TIME_LIMIT_S = 120
PATCH = 22                           # CONV_VARIANTS["v6p"]


class _Spy:
    """The kernel library with the (name, arguments) of the launchers called through it."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


@pytest.fixture(autouse=True)
def _setup(cuda, monkeypatch):
    assert _native.load_kernels() is not None, _native.kernels_error()
    assert _native.has_kernel("cgs_conv2d_nhwc_gns_v")
    monkeypatch.setenv("CGS_AUTOTUNE", "0")
    monkeypatch.setenv("CGS_CONV_PATCH", "1")
    ops.reset_stats()
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)     # each test under its own time limit
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture
def spy(monkeypatch):
    s = _Spy(_native.load_kernels())
    monkeypatch.setattr(core, "_lib", lambda: s)
    return s


def _ptr(t):
    return None if t is None else t.data_ptr()


def _operands(dev, N, Cin, Cout, H, W, bias, res, k=3, Ho=None, Wo=None):
    g = torch.Generator(device="cpu").manual_seed(N * 7 + Cin * 3 + Cout + H * 31 + W)
    ramp = torch.arange(N * H * W, dtype=torch.float32).view(N, 1, H, W) / (N * H * W) * 4 - 2
    x = (ramp + 0.5 * torch.randn(N, Cin, H, W, generator=g)).to(dev).to(BF).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(k * k * Cin)).to(dev).to(BF)
    b = torch.randn(Cout, generator=g).to(dev).to(BF) if bias else None
    r = None
    if res:
        r = torch.randn(N, Cout, Ho or H, Wo or W, generator=g).to(dev).to(BF).contiguous(memory_format=torch.channels_last)
    return x, w, b, r


#        N, Cin, Cout, H, W, bias, residual
CASES = [(2, 64, 24, 5, 7, True, False),        # one partial patch, all four borders; one slab
         (2, 64, 24, 5, 7, False, True),
         (1, 192, 8, 5, 7, False, False),       # three slabs (odd: the patch buffers swap parity between units)
         (2, 128, 168, 17, 19, True, True),     # 2 x 2 patches, seams and partial patches; two column tiles
         (1, 128, 168, 17, 19, False, False),
         (1, 64, 8, 16, 16, True, False),       # an exact patch; a partial column tile
         (1, 192, 24, 32, 16, True, True),      # two exact patches
         (3, 128, 24, 16, 16, True, False),     # an image boundary between consecutive units
         (5, 64, 640, 64, 64, True, True)]      # 320 units: more than one per compute unit


@pytest.mark.parametrize("N,Cin,Cout,H,W,bias,res", CASES)
def test_conv_patch_bound(cuda, N, Cin, Cout, H, W, bias, res):
    what = f"conv v6p {N}x{Cin}x{H}x{W}->{Cout} bias={bias} res={res}"
    x, w, b, r = _operands(cuda, N, Cin, Cout, H, W, bias, res)
    wn = w.permute(0, 2, 3, 1).contiguous()
    buf, before, optr = _guarded(cuda, N * H * W * Cout, 256 * Cout)   # the NHWC output, a tile of rows after it
    lib = _native.load_kernels()
    assert lib.cgs_conv2d_nhwc_v(x.data_ptr(), None, Cin, wn.data_ptr(), _ptr(b), _ptr(r), optr, N, H, W, Cin, Cout,
                                 3, 3, 1, 1, H, W, 0, PATCH, core._stream()) == 0
    own = torch.ones(N * H * W * Cout, dtype=torch.bool, device=cuda)
    out = _check_guard(buf, before, own, BF, what).view(N, H, W, Cout)
    ref, tol = conv_bound(x, w, b, r, 1, 1)
    assert_within(out.permute(0, 3, 1, 2), ref, tol, what)


def _patch_blocks(out):
    """The stored NHWC output [N, H, W, C] in the block order of the kernel's partials: block patch * 4 + q holds
    rows 4 q .. 4 q + 3 of the 16 x 16 patch (patches row-major over the image), 64 pixels each."""
    N, H, W, C = out.shape
    v = out.view(N, H // 16, 4, 4, W // 16, 16, C).permute(0, 1, 4, 2, 3, 5, 6)     # n, ty, tx, q, row, x, c
    return v.reshape(N, (H * W) // 64, 64, C)


@pytest.mark.parametrize("Cout", [8, 168])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", [(16, 16), (32, 16)])
def test_conv_patch_gn_partials_bound(cuda, H, W, N, Cout):
    lib = _native.load_kernels()
    Cin, HW = 64, H * W
    for bias in (True, False):
        for res in (False, True):
            what = f"gn-partials/conv v6p {N}x{Cin}x{H}x{W}->{Cout} bias={bias} res={res}"
            x, w, b, r = _operands(cuda, N, Cin, Cout, H, W, bias, res)
            wn = w.permute(0, 2, 3, 1).contiguous()
            buf, before, optr = _guarded(cuda, N * HW * Cout, 256 * Cout)
            gbuf, gptr, gnp = _nan_guarded(cuda, N * (HW // 64), Cout * 2)
            st = core._stream()
            assert lib.cgs_conv2d_nhwc_gns_v(x.data_ptr(), None, Cin, wn.data_ptr(), _ptr(b), _ptr(r), optr, N, H, W,
                                             Cin, Cout, 3, 3, 1, 1, H, W, 0, gptr, PATCH, st) == 0
            own = torch.ones(N * HW * Cout, dtype=torch.bool, device=cuda)
            out = _check_guard(buf, before, own, BF, what).view(N, H, W, Cout)
            ref, tol = conv_bound(x, w, b, r, 1, 1)
            assert_within(out.permute(0, 3, 1, 2), ref, tol, what + " out")                     # 1
            _guards_kept(gbuf, N * (HW // 64), Cout * 2, what)                                  # 2
            pref, ptol = gn_partials_bound(_patch_blocks(out.contiguous()))
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


def _variants(spy):
    """(launcher, variant) of the conv launches seen by the spy."""
    pos = {"cgs_conv2d_nhwc_v": -2, "cgs_conv2d_nhwc_gns_v": -2}
    return [(n, a[pos[n]] if n in pos else None) for n, a in spy.calls]


def test_ops_takes_the_patch_form(cuda, spy):
    N, Cin, Cout, H, W = 2, 128, 168, 17, 19
    x, w, b, r = _operands(cuda, N, Cin, Cout, H, W, True, True)
    ref, tol = conv_bound(x, w, b, r, 1, 1)
    y = ops.conv2d(x, w, b, 1, 1, residual=r, weight_nhwc=w.permute(0, 2, 3, 1).contiguous())
    assert _variants(spy) == [("cgs_conv2d_nhwc_v", PATCH)], _variants(spy)
    assert ops.stats().get(("conv", "hip"), 0) == 1
    assert y.shape == (N, Cout, H, W) and y.is_contiguous(memory_format=torch.channels_last)
    assert_within(y, ref, tol, "ops.conv2d on the patch form")


def test_ops_gn_stats_takes_the_patch_form(cuda, spy):
    N, Cin, Cout, H, W = 3, 64, 168, 32, 16
    x, w, b, _ = _operands(cuda, N, Cin, Cout, H, W, True, False)
    ref, tol = conv_bound(x, w, b, None, 1, 1)
    y = ops.conv2d(x, w, b, 1, 1, weight_nhwc=w.permute(0, 2, 3, 1).contiguous(), gn_stats=True)
    assert _variants(spy) == [("cgs_conv2d_nhwc_gns_v", PATCH)], _variants(spy)
    assert_within(y, ref, tol, "ops.conv2d gn_stats on the patch form")
    part, optr = y._cgs_gnpart
    assert optr == y.data_ptr()
    pref, ptol = gn_partials_bound(_patch_blocks(y.permute(0, 2, 3, 1).contiguous()))
    assert_within(part.view(N, H * W // 64, Cout, 2), pref, ptol, "ops.conv2d gn_stats partials")


def test_env_zero_keeps_the_old_kernel(cuda, spy, monkeypatch):
    monkeypatch.setenv("CGS_CONV_PATCH", "0")
    x, w, b, _ = _operands(cuda, 2, 64, 24, 5, 7, True, False)
    ref, tol = conv_bound(x, w, b, None, 1, 1)
    y = ops.conv2d(x, w, b, 1, 1, weight_nhwc=w.permute(0, 2, 3, 1).contiguous())
    assert len(spy.calls) == 1 and all(v != PATCH for _, v in _variants(spy)), _variants(spy)
    assert_within(y, ref, tol, "conv CGS_CONV_PATCH=0")


@pytest.mark.parametrize("refuse", ["stride2", "1x1", "x2", "upsample2x", "cin96"])
def test_refused_forms_take_the_old_kernel(cuda, spy, refuse):
    N, Cin, Cout, H, W = 2, 128, 24, 6, 8
    k, stride, pad, up, x2 = 3, 1, 1, False, None
    if refuse == "stride2":
        stride = 2
    elif refuse == "1x1":
        k, pad = 1, 0
    elif refuse == "upsample2x":
        up = True
    elif refuse == "cin96":
        Cin = 96
    x, w, b, _ = _operands(cuda, N, Cin, Cout, H, W, True, False, k=k)
    xa = x
    if refuse == "x2":
        xa, x2 = x[:, :64].contiguous(memory_format=torch.channels_last), x[:, 64:].contiguous(memory_format=torch.channels_last)
    ref, tol = conv_bound(xa, w, b, None, stride, pad, upsample2x=up, x2=x2)
    y = ops.conv2d(xa, w, b, stride, pad, weight_nhwc=w.permute(0, 2, 3, 1).contiguous(), upsample2x=up, x2=x2)
    assert len(spy.calls) == 1 and all(v != PATCH for _, v in _variants(spy)), _variants(spy)
    assert_within(y, ref, tol, f"conv refused by the patch form ({refuse})")


def test_launcher_refuses_outside_the_domain(cuda):
    """Variant 22 asked for directly on a shape outside its domain is an error, not another kernel."""
    lib = _native.load_kernels()
    x, w, b, _ = _operands(cuda, 1, 64, 24, 6, 8, True, False)
    wn = w.permute(0, 2, 3, 1).contiguous()
    out = torch.empty(1, 3, 4, 24, device=cuda, dtype=BF)
    assert lib.cgs_conv2d_nhwc_v(x.data_ptr(), None, 64, wn.data_ptr(), b.data_ptr(), None, out.data_ptr(), 1, 6, 8,
                                 64, 24, 3, 3, 2, 1, 3, 4, 0, PATCH, core._stream()) != 0
