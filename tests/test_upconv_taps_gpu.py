"""The tap form of the upsample conv (csrc/kernels/upconv.hip) against the per-element bound of the conv kernels
(tests/_bounds.py conv_bound, unchanged): zero elements over the bound.

``CGS_UPCONV_TAPS=1`` forces the tap form wherever ``ops.conv2d`` may take it; a spy on the library handle shows
which launcher ran. Shapes are the smallest that reach an edge of the kernel: one partial patch with all four image
borders in it, several patches with interior and halo seams in both axes, exactly one 14 x 14 interior block and
one pixel over, each of the four patch shapes the launcher picks from (16 x 16, 18 x 14, 14 x 18, 34 x 7), Cin with
and without a half K tile at the end (Cin % 64 == 32), and Cout that is not a multiple of the 16-channel group.
Every pixel of the input is distinct (a ramp over the pixels plus noise), so a wrong neighbour cannot cancel."""
import faulthandler
import math

import pytest
import torch

from comfy_gen_server_amd import ops, _native
from comfy_gen_server_amd.models.layers import Conv2d
from comfy_gen_server_amd.ops import core

from _bounds import assert_within, conv_bound

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TIME_LIMIT_S = 120


class _Spy:
    """The kernel library with the names of the launchers called through it."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


@pytest.fixture(autouse=True)
def _setup(cuda, monkeypatch):
    assert _native.load_kernels() is not None, _native.kernels_error()
    assert _native.has_kernel("cgs_upconv_taps_nhwc")
    monkeypatch.setenv("CGS_AUTOTUNE", "0")
    monkeypatch.setenv("CGS_UPCONV_TAPS", "1")
    ops.reset_stats()
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)     # each test under its own time limit
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture
def spy(monkeypatch):
    s = _Spy(_native.load_kernels())
    monkeypatch.setattr(core, "_lib", lambda: s)
    return s


def _operands(dev, N, Cin, Cout, H, W, bias):
    g = torch.Generator(device="cpu").manual_seed(N * 7 + Cin * 3 + Cout + H * 31 + W)
    ramp = torch.arange(N * H * W, dtype=torch.float32).view(N, 1, H, W) / (N * H * W) * 4 - 2
    x = (ramp + 0.5 * torch.randn(N, Cin, H, W, generator=g)).to(dev).to(BF).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).to(dev).to(BF)
    b = torch.randn(Cout, generator=g).to(dev).to(BF) if bias else None
    return x, w, b


#        N, Cin, Cout, H, W
CASES = [(2, 32, 16, 5, 7),      # one partial patch, all four borders
         (2, 64, 48, 17, 19),    # 2 x 2 patches of 16 x 16: seams in both axes, three channel groups
         (1, 96, 16, 14, 14),    # exactly one interior block; Cin % 64 == 32
         (1, 96, 16, 15, 15),    # one pixel over: 18 x 14 patches
         (1, 64, 24, 5, 32),     # the 34 x 7 patch; half a channel group
         (1, 32, 24, 16, 12)]    # the 14 x 18 patch


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("N,Cin,Cout,H,W", CASES)
def test_upconv_taps_bound(cuda, spy, N, Cin, Cout, H, W, bias):
    x, w, b = _operands(cuda, N, Cin, Cout, H, W, bias)
    ref, tol = conv_bound(x, w, b, None, 1, 1, upsample2x=True)
    y = ops.conv2d(x, w, b, 1, 1, weight_nhwc=w.permute(0, 2, 3, 1).contiguous(), upsample2x=True,
                   weight_taps=core.upconv_tap_weights(w))
    assert spy.calls == ["cgs_upconv_taps_nhwc"], spy.calls
    assert ops.stats().get(("conv", "hip"), 0) == 1
    assert y.shape == (N, Cout, 2 * H, 2 * W) and y.is_contiguous(memory_format=torch.channels_last)
    assert_within(y, ref, tol, f"upconv_taps {N}x{Cin}x{H}x{W}->{Cout} bias={bias}")


@pytest.mark.parametrize("refuse", ["residual", "x2"])
def test_refused_forms_take_the_old_kernel(cuda, spy, refuse):
    N, Cin, Cout, H, W = 2, 128, 24, 5, 7
    x, w, b = _operands(cuda, N, Cin, Cout, H, W, True)
    r = x2 = None
    if refuse == "residual":
        r = torch.randn(N, Cout, 2 * H, 2 * W, device=cuda).to(BF).contiguous(memory_format=torch.channels_last)
        xa = x
    else:
        xa, x2 = x[:, :64], x[:, 64:]
    ref, tol = conv_bound(xa, w, b, r, 1, 1, upsample2x=True, x2=x2)
    y = ops.conv2d(xa, w, b, 1, 1, residual=r, weight_nhwc=w.permute(0, 2, 3, 1).contiguous(), upsample2x=True,
                   x2=x2, weight_taps=core.upconv_tap_weights(w))
    assert "cgs_upconv_taps_nhwc" not in spy.calls and len(spy.calls) == 1, spy.calls
    assert_within(y, ref, tol, f"upconv refused ({refuse})")


def test_env_zero_keeps_the_old_kernel(cuda, spy, monkeypatch):
    monkeypatch.setenv("CGS_UPCONV_TAPS", "0")
    x, w, b = _operands(cuda, 2, 64, 24, 5, 7, True)
    ref, tol = conv_bound(x, w, b, None, 1, 1, upsample2x=True)
    y = ops.conv2d(x, w, b, 1, 1, weight_nhwc=w.permute(0, 2, 3, 1).contiguous(), upsample2x=True,
                   weight_taps=core.upconv_tap_weights(w))
    assert spy.calls == ["cgs_conv2d_nhwc_v"], spy.calls
    assert_within(y, ref, tol, "upconv CGS_UPCONV_TAPS=0")


def test_layer_caches_the_tap_copy(cuda, spy):
    conv = Conv2d(64, 48, 3, padding=1, dtype=BF, device=cuda)
    x, w, b = _operands(cuda, 2, 64, 48, 17, 19, True)
    conv.weight.data.copy_(w)
    conv.bias.data.copy_(b)
    y1 = conv(x, upsample2x=True)
    wt = conv.__dict__["_derived"]["w_taps"]
    y2 = conv(x, upsample2x=True)
    assert conv.__dict__["_derived"]["w_taps"] is wt and torch.equal(wt, core.upconv_tap_weights(w))
    assert spy.calls == ["cgs_upconv_taps_nhwc"] * 2, spy.calls
    ref, tol = conv_bound(x, w, b, None, 1, 1, upsample2x=True)
    assert_within(y1, ref, tol, "upconv_taps through Conv2d")
    assert torch.equal(y1, y2)
