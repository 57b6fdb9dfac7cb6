"""Image-filter ops on the CPU: the nodes keep their results bit for bit (the ops' torch path is the code the nodes
ran before), the clamped-window identity ``cgs_morph_box`` relies on, and the argument checks."""
import pytest
import torch

from comfy_gen_server_amd import ops
from comfy_gen_server_amd.nodes import extras_image as NI
from comfy_gen_server_amd.nodes.extras_model import gaussian_blur_2d

import _filters as FX


def _image(seed=0, shape=(2, 24, 31, 3)):
    return FX.filter_input(shape, seed=seed)


@pytest.mark.parametrize("radius,sigma", [(1, 1.0), (5, 0.7), (11, 10.0)])
def test_image_blur_node_unchanged(radius, sigma):
    img = _image()
    ops.reset_stats()
    y = NI.ImageBlur().blur(img, radius, sigma)[0]
    assert ops.stats() == {("filter", "torch"): 1}
    assert torch.equal(y, FX.blur_frozen(img, radius, sigma))


@pytest.mark.parametrize("radius,sigma,alpha", [(1, 1.0, 1.0), (3, 0.5, 5.0), (7, 2.0, 0.3)])
def test_image_sharpen_node_unchanged(radius, sigma, alpha):
    img = _image(1)
    ops.reset_stats()
    y = NI.ImageSharpen().sharpen(img, radius, sigma, alpha)[0]
    assert ops.stats() == {("filter", "torch"): 1}
    assert torch.equal(y, FX.sharpen_frozen(img, radius, sigma, alpha))
    assert y.min() >= 0 and y.max() <= 1


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("operation", FX.MORPH_OPS)
def test_morphology_node_unchanged(operation, k):
    img = _image(2)
    ops.reset_stats()
    y = NI.Morphology().process(img, operation, k)[0]
    st = ops.stats()
    assert set(st) == {("morph", "torch")} and st[("morph", "torch")] >= 1
    assert torch.equal(y, FX.morphology_frozen(img, operation, k))


def test_canny_node_unchanged():
    img = FX.field(0, size=(48, 64)).movedim(1, -1).contiguous()
    ops.reset_stats()
    y = NI.Canny().detect_edge(img, 0.1, 0.3)[0]
    assert ops.stats() == {("canny", "torch"): 1}
    mag, edges = FX.canny_edges(img.movedim(-1, 1).float(), 0.1, 0.3)
    assert edges.sum() > 0
    assert torch.equal(y, edges.repeat(1, 3, 1, 1).movedim(1, -1))
    m2, e2 = NI.canny_edges(img.movedim(-1, 1).float(), 0.1, 0.3)       # still importable, delegates
    assert torch.equal(m2, mag) and torch.equal(e2, edges)
    # the split ops compose to the same result
    m3, cls = ops.canny_classes(img.movedim(-1, 1).float(), 0.1, 0.3)
    assert cls.dtype == torch.uint8 and torch.equal(m3, mag) and torch.equal(ops.hysteresis(cls), edges)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sag_blur_unchanged(dtype):
    x = FX.filter_input((2, 4, 20, 23), dtype, seed=3)
    ops.reset_stats()
    y = gaussian_blur_2d(x, 9, 2.0)
    assert ops.stats() == {("filter", "torch"): 1}
    assert y.dtype == dtype and torch.equal(y, FX.gaussian_blur_2d(x, 9, 2.0))


def test_filter_sep_torch_path_without_dense_kernel():
    """Without ``dense`` the torch path builds K = ax delta + ay (t_h (x) t_w) itself, in either layout."""
    x = FX.filter_input((1, 3, 12, 14), seed=4)
    tw, th = ops.gaussian_taps(5, 0.8), ops.gaussian_taps(3, 1.0, span="pixel")
    k = -2.0 * torch.outer(th, tw)
    k[1, 2] += 3.0
    for border, mode in (("reflect", "reflect"), ("replicate", "replicate"), ("zero", "constant")):
        want = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (2, 2, 1, 1), mode=mode), k.expand(3, 1, 3, 5),
                                          groups=3).clamp(0, 1)
        y = ops.filter_sep(x, tw, th, border=border, ax=3.0, ay=-2.0, clamp=(0, 1))
        assert torch.equal(y, want)
        y2 = ops.filter_sep(x.movedim(1, -1), tw, th, border=border, layout="nhwc", ax=3.0, ay=-2.0, clamp=(0, 1))
        assert y2.shape == (1, 12, 14, 3) and torch.equal(y2, want.movedim(1, -1))


@pytest.mark.parametrize("k", [3, 4, 13, 41])
def test_clamped_window_identity(k):
    """max_pool2d after replicate padding (p, k - 1 - p) is the maximum over [i - p, i + k - 1 - p] clamped to the
    image: what cgs_morph_box computes, even k and k beyond the image included."""
    x = FX.filter_input((1, 2, 13, 17), seed=5)
    H, W = x.shape[-2:]
    p, q = k // 2, k - 1 - k // 2
    hi = torch.empty_like(x)
    lo = torch.empty_like(x)
    for i in range(H):
        for j in range(W):
            win = x[..., max(i - p, 0):min(i + q, H - 1) + 1, max(j - p, 0):min(j + q, W - 1) + 1]
            hi[..., i, j] = win.amax((-2, -1))
            lo[..., i, j] = win.amin((-2, -1))
    assert torch.equal(hi, FX._dilate(x, k)) and torch.equal(lo, FX._erode(x, k))
    ops.reset_stats()
    assert torch.equal(ops.morph_box(x, k, "dilate"), hi) and torch.equal(ops.morph_box(x, k, "erode"), lo)
    assert torch.equal(ops.morph_box(x.movedim(1, -1), k, "erode", layout="nhwc"), lo.movedim(1, -1))
    assert ops.stats() == {("morph", "torch"): 3}


def test_validation():
    x = torch.zeros(1, 1, 5, 7)
    t9, t11 = ops.gaussian_taps(9, 1.0), ops.gaussian_taps(11, 1.0)
    ops.filter_sep(x, t9)                                   # r = 4 = H - 1: the largest reflect radius
    with pytest.raises(ValueError):
        ops.filter_sep(x, t11)                              # r = 5 = H
    with pytest.raises(ValueError):
        ops.filter_sep(x, ops.gaussian_taps(15, 1.0), ops.gaussian_taps(3, 1.0))   # r = 7 = W
    ops.filter_sep(x, t11, border="replicate")
    with pytest.raises(ValueError):
        ops.filter_sep(x, torch.ones(4) / 4)                # even tap count
    with pytest.raises(ValueError):
        ops.filter_sep(x, t9, torch.ones(2) / 2)
    with pytest.raises(ValueError):
        ops.filter_sep(x, t9, border="wrap")
    with pytest.raises(ValueError):
        ops.morph_box(x, 3, "open")
    with pytest.raises(ValueError):
        ops.gaussian_taps(5, 1.0, span="inch")


@pytest.mark.parametrize("span", ["unit", "pixel"])
def test_gaussian_taps_sum_to_one(span):
    for k, sigma in [(3, 1.0), (9, 2.0), (63, 0.1), (63, 10.0), (5, 1.0)]:
        t = ops.gaussian_taps(k, sigma, span=span)
        assert t.dtype == torch.float32 and t.shape == (k,)
        assert abs(t.double().sum().item() - 1.0) <= 4 * 2.0 ** -24
        assert torch.equal(t, t.flip(0))
    # Canny's five taps are the pixel span at sigma 1
    ax = torch.arange(5, dtype=torch.float32) - 2
    g1 = torch.exp(-ax ** 2 / 2.0)
    assert torch.equal(ops.gaussian_taps(5, 1.0, span="pixel"), g1 / g1.sum())
