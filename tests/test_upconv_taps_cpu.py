"""The identity behind the tap form of the upsample conv (csrc/kernels/upconv.hip), in fp64 on the CPU.

    T[dy,dx][n, i, j, co] = sum_ci x[n, i, j, ci] W[co, ci, dy, dx]                      (low resolution)
    out[n, 2i+a, 2j+b, co] = bias[co] + sum_{dy,dx} T[dy,dx][n, (2i+a+dy-1) >> 1, (2j+b+dx-1) >> 1, co]

with a tap dropped where its upsampled coordinate leaves the image -- which is where its low-resolution source
pixel leaves the image too, so zero rows around T do it. ``upconv_taps_ref`` is that sum; ``_tap_planes`` builds T
from ``ops.core.upconv_tap_weights``, the copy the kernel reads, so the row order of that copy is checked as well."""
import pytest
import torch
import torch.nn.functional as F

from comfy_gen_server_amd.ops import core


def nb(a, d):
    """Source offset of tap d for output parity a: ((2 i + a + d - 1) >> 1) - i."""
    return ((a + d - 1) >> 1)


def _tap_planes(x, w):
    """T [N, 3, 3, Cout, H, W] from the tap-ordered weight copy: rows (g * 9 + tap) * 16 + c."""
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    wt = core.upconv_tap_weights(w)                                   # [G * 144, Cin]
    G = wt.shape[0] // 144
    t = torch.einsum("nchw,rc->nrhw", x, wt).view(N, G, 9, 16, H, W)
    t = t.permute(0, 2, 1, 3, 4, 5).reshape(N, 9, G * 16, H, W)
    assert bool((t[:, :, Cout:] == 0).all())                          # channels past Cout: zero rows
    return t[:, :, :Cout].reshape(N, 3, 3, Cout, H, W)


def upconv_taps_ref(x, w, b=None):
    """conv2d(nearest2x(x), w, b, stride 1, pad 1) by the identity above; x [N, Cin, H, W], w [Cout, Cin, 3, 3]."""
    N, _, H, W = x.shape
    Cout = w.shape[0]
    Tp = F.pad(_tap_planes(x, w), (1, 1, 1, 1))                        # zero halo: dropped taps
    out = x.new_zeros((N, Cout, 2 * H, 2 * W))
    for a in range(2):
        for c in range(2):
            acc = x.new_zeros((N, Cout, H, W))
            for dy in range(3):
                for dx in range(3):
                    oy, ox = 1 + nb(a, dy), 1 + nb(c, dx)
                    acc = acc + Tp[:, dy, dx, :, oy:oy + H, ox:ox + W]
            out[:, :, a::2, c::2] = acc
    return out if b is None else out + b[None, :, None, None]


def test_nb_is_the_shifted_index():
    for i in range(5):
        for a in range(2):
            for d in range(3):
                assert i + nb(a, d) == (2 * i + a + d - 1) >> 1
    assert [[nb(a, d) for d in range(3)] for a in range(2)] == [[-1, 0, 0], [0, 0, 1]]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("Cout", [4, 24])
@pytest.mark.parametrize("Cin", [8, 32])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 7), (17, 19)])
def test_identity_matches_conv_of_upsampled(H, W, Cin, Cout, bias):
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + Cin + Cout)
    x = torch.randn(2, Cin, H, W, dtype=torch.float64, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, dtype=torch.float64, generator=g) / (9 * Cin) ** 0.5
    b = torch.randn(Cout, dtype=torch.float64, generator=g) if bias else None
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, 1, 1)
    got = upconv_taps_ref(x, w, b)
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() <= 1e-12


def test_tap_weight_copy_layout():
    w = torch.arange(24 * 8 * 9, dtype=torch.float32).view(24, 8, 3, 3)
    wt = core.upconv_tap_weights(w)
    assert wt.shape == (2 * 144, 8) and wt.is_contiguous()
    for co, dy, dx in [(0, 0, 0), (5, 1, 2), (15, 2, 2), (16, 0, 1), (23, 2, 0)]:
        row = ((co // 16) * 9 + 3 * dy + dx) * 16 + co % 16
        assert torch.equal(wt[row], w[co, :, dy, dx])
    assert bool((wt.view(2, 9, 16, 8)[1, :, 8:] == 0).all())
