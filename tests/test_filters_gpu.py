"""Device image filters: ``cgs_filter_sep`` within a derived per-element bound of the dense fp64 formula,
``cgs_morph_box`` and ``cgs_hysteresis_sweep`` exact, ``cgs_canny_nms`` against fp64 wherever the fp64 decision is
not marginal, the nodes on device tensors, and graph capture of the SAG blur."""
import pytest
import torch

from comfy_gen_server_amd import ops
from comfy_gen_server_amd.nodes import extras_image as NI
from comfy_gen_server_amd.nodes.extras_model import gaussian_blur_2d

import _filters as FX
from _bounds import assert_within

pytestmark = pytest.mark.gpu

FILTER_TILE = (32, 64)   # rows x (interleaved) columns of one cgs_filter_sep workgroup


# ---------------------------------------------------------------- 4. filter_sep
def _blur_case(cuda, x_nchw, radius, sigma, layout, what):
    """ImageBlur's form (unit taps, reflect) on ``x_nchw`` given to the op in ``layout``."""
    ks = 2 * radius + 1
    ref, tol = FX.filter_ref_and_tol(x_nchw, FX.gaussian_kernel64(ks, sigma))
    xd = x_nchw.to(cuda)
    taps = ops.gaussian_taps(ks, sigma, cuda, "unit")
    ops.reset_stats()
    if layout == "nhwc":
        xd = xd.movedim(1, -1).contiguous()
        y = ops.filter_sep(xd, taps, layout="nhwc")
        assert y.is_contiguous() and y.shape == xd.shape
        y = y.movedim(-1, 1)
    else:
        y = ops.filter_sep(xd, taps)
        assert y.is_contiguous()
    assert ops.stats() == {("filter", "hip"): 1}
    assert y.dtype == x_nchw.dtype
    assert_within(y.cpu(), ref, tol, what)


@pytest.mark.parametrize("radius,sigma", [(1, 1.0), (5, 1.0), (31, 1.0), (31, 0.1), (31, 10.0)])
def test_filter_sep_image_nhwc(cuda, radius, sigma):
    x = FX.filter_input((2, 70, 90, 3)).movedim(-1, 1)
    _blur_case(cuda, x, radius, sigma, "nhwc", f"blur nhwc 2x70x90x3 r={radius} sigma={sigma}")


@pytest.mark.parametrize("shape,radius", [((1, 3, 33, 32), 31), ((1, 1, 5, 7), 4), ((1, 3, 150, 270), 5)],
                         ids=["halo-exceeds-image", "r=H-1", "multi-tile"])
def test_filter_sep_planar_shapes(cuda, shape, radius):
    if radius == 5:   # the multi-tile case spans at least two tiles each way
        assert shape[2] > FILTER_TILE[0] and shape[3] > FILTER_TILE[1]
    _blur_case(cuda, FX.filter_input(shape, seed=1), radius, 1.0, "nchw", f"blur nchw {shape} r={radius}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_filter_sep_sag_form(cuda, dtype):
    """SAG's blur: NCHW latent, 9 pixel-span taps, 16-bit storage; the node helper takes the same path."""
    x = FX.filter_input((2, 4, 40, 40), dtype, seed=2)
    ref, tol = FX.filter_ref_and_tol(x, FX.pixel_kernel64(9, 2.0))
    ops.reset_stats()
    y = ops.filter_sep(x.to(cuda), ops.gaussian_taps(9, 2.0, cuda, span="pixel"))
    assert ops.stats() == {("filter", "hip"): 1} and y.dtype == dtype
    assert_within(y.cpu(), ref, tol, f"sag blur {dtype}")
    assert torch.equal(gaussian_blur_2d(x.to(cuda), 9, 2.0), y)


@pytest.mark.parametrize("border", ["replicate", "zero"])
def test_filter_sep_borders(cuda, border):
    x = FX.filter_input((1, 3, 21, 37), seed=3)
    ref, tol = FX.filter_ref_and_tol(x, FX.gaussian_kernel64(5, 1.0), border=border)
    y = ops.filter_sep(x.to(cuda), ops.gaussian_taps(5, 1.0, cuda), border=border)
    assert_within(y.cpu(), ref, tol, f"blur {border} r=2")


def test_filter_sep_sharpen(cuda):
    """alpha = 5: ax = 51, ay = -50, clamp to [0, 1] acting on both sides; oracle = the node's dense kernel in fp64."""
    x = FX.filter_input((2, 70, 90, 3), seed=4).movedim(-1, 1)
    g2 = FX.gaussian_kernel64(7, 1.0)
    ref, tol = FX.filter_ref_and_tol(x, g2, ax=51.0, ay=-50.0, clamp=(0, 1), ref_kernel=FX.sharpen_kernel(g2.clone(), 5.0))
    assert (ref == 0).any() and (ref == 1).any()
    img = x.movedim(1, -1).contiguous().to(cuda)
    ops.reset_stats()
    y = NI.ImageSharpen().sharpen(img, 3, 1.0, 5.0)[0]
    assert ops.stats() == {("filter", "hip"): 1} and y.shape == img.shape and y.is_contiguous()
    assert_within(y.movedim(-1, 1).cpu(), ref, tol, "sharpen alpha=5 r=3")


def test_filter_sep_layouts_agree_and_overrides(cuda):
    x = FX.filter_input((2, 4, 40, 45), seed=5).to(cuda)
    taps = ops.gaussian_taps(9, 2.0, cuda, span="pixel")
    y = ops.filter_sep(x, taps)
    assert torch.equal(ops.filter_sep(x.contiguous(memory_format=torch.channels_last), taps), y)
    img = FX.filter_input((2, 33, 70, 3), seed=6).to(cuda)
    t3 = ops.gaussian_taps(11, 1.0, cuda)
    assert torch.equal(ops.filter_sep(img, t3, layout="nhwc").movedim(-1, 1),
                       ops.filter_sep(img.movedim(-1, 1).contiguous(), t3))
    ops.reset_stats()
    with ops.torch_reference():
        yt = ops.filter_sep(x, taps)
    ops.set_backend_override("filter", "torch")
    try:
        assert torch.equal(ops.filter_sep(x, taps), yt)
    finally:
        ops.set_backend_override("filter", None)
    assert ops.stats() == {("filter", "torch"): 2}
    assert torch.allclose(yt, y, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_filter_sep_two_launch_form_gives_the_same_bits(cuda, dtype):
    """From ``_FILTER_TWO_LAUNCH_TAPS`` taps on, the op runs the kernel twice through an fp32 temporary: the same
    bits as one launch, at the threshold, below it, with unequal tap counts and with the sharpen epilogue."""
    from comfy_gen_server_amd.ops import core
    n = core._FILTER_TWO_LAUNCH_TAPS
    x = FX.filter_input((2, 70, 90, 3), dtype, seed=14).to(cuda).movedim(-1, 1)
    for kw, kh in ((n, n), (n - 2, n - 2), (n + 2, 3), (5, 63)):
        tw, th = ops.gaussian_taps(kw, 1.0, cuda), ops.gaussian_taps(kh, 0.5, cuda)
        args = (x, tw, th, "reflect", "nhwc", 3.0, -2.0, (0, 1))
        one = core._filter_sep_hip(*args, two_launch=False)
        assert torch.equal(core._filter_sep_hip(*args, two_launch=True), one)
        assert torch.equal(ops.filter_sep(x.movedim(1, -1), tw, th, layout="nhwc", ax=3.0, ay=-2.0, clamp=(0, 1)), one)
        ref, tol = FX.filter_ref_and_tol(x.cpu(), torch.outer(th.cpu().double(), tw.cpu().double()), ax=3.0, ay=-2.0,
                                         clamp=(0, 1))
        assert_within(one.movedim(-1, 1).cpu(), ref, tol, f"two forms {kh}x{kw} {dtype}")


def test_filter_sep_outside_the_kernel_domain_is_counted_lib(cuda, monkeypatch):
    x = FX.filter_input((1, 1, 80, 80), seed=7).to(cuda)
    ops.reset_stats()
    y = ops.filter_sep(x, ops.gaussian_taps(65, 1.0, cuda), border="replicate")
    assert y.shape == x.shape and ops.stats() == {("filter", "lib"): 1}
    monkeypatch.setenv("CGS_STRICT_NATIVE", "1")
    with pytest.raises(ops.dispatch.VendorFallbackError):
        ops.filter_sep(x, ops.gaussian_taps(65, 1.0, cuda), border="replicate")


# ---------------------------------------------------------------- 5. morph_box
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("k", [3, 4, 5, 31, 64, 255])
def test_morph_box_exact(cuda, k, dtype):
    x = FX.filter_input((2, 3, 70, 90), dtype, seed=8).to(cuda)
    ops.reset_stats()
    hi, lo = ops.morph_box(x, k, "dilate"), ops.morph_box(x, k, "erode")
    assert ops.stats() == {("morph", "hip"): 2}
    assert hi.dtype == dtype and hi.is_contiguous()
    assert torch.equal(hi, FX._dilate(x, k)) and torch.equal(lo, FX._erode(x, k))


def test_morph_box_k999_and_nhwc(cuda):
    x = FX.filter_input((1, 1, 40, 50), seed=9).to(cuda)
    assert torch.equal(ops.morph_box(x, 999, "dilate"), FX._dilate(x, 999))
    assert torch.equal(ops.morph_box(x, 999, "erode"), FX._erode(x, 999))
    tall = FX.filter_input((1, 2, 1100, 9), seed=10).to(cuda)       # a 999-long window that is not the whole axis
    assert torch.equal(ops.morph_box(tall, 999, "dilate"), FX._dilate(tall, 999))
    img = FX.filter_input((2, 70, 90, 3), seed=11).to(cuda)
    ops.reset_stats()
    for k in (4, 13):
        y = ops.morph_box(img, k, "dilate", layout="nhwc")
        assert y.shape == img.shape and y.is_contiguous()
        assert torch.equal(y, FX._dilate(img.movedim(-1, 1), k).movedim(1, -1))
        assert torch.equal(ops.morph_box(img.movedim(-1, 1), k, "erode"), FX._erode(img.movedim(-1, 1), k))
    assert ops.stats() == {("morph", "hip"): 4}


@pytest.mark.parametrize("operation", FX.MORPH_OPS)
def test_morphology_node(cuda, operation):
    img = FX.filter_input((2, 70, 90, 3), seed=12).clamp(0, 1).to(cuda)
    ops.reset_stats()
    y = NI.Morphology().process(img, operation, 5)[0]
    st = ops.stats()
    assert set(st) == {("morph", "hip")}
    assert y.shape == img.shape and torch.equal(y.to(cuda), FX.morphology_frozen(img, operation, 5))


# ---------------------------------------------------------------- 6. hysteresis
def _hysteresis_equals(cuda, cls, want):
    ops.reset_stats()
    info = {}
    y = ops.hysteresis(cls.to(cuda), info)
    assert ops.stats() == {("canny", "hip"): 1}
    assert y.dtype == torch.float32 and y.shape == cls.shape
    assert torch.equal(y.cpu(), want)
    return info


def test_hysteresis_random_map(cuda):
    cls = FX.random_classes()
    _hysteresis_equals(cuda, cls, FX.hysteresis_frozen(cls))


def test_hysteresis_serpentine(cuda):
    """Growth has to travel up and left along the whole path, across every tile border many times."""
    cls, path = FX.serpentine()
    # the frozen loop grows one pixel per round, about 20000 rounds here: run on the device, where a round is
    # a handful of small launches
    want = FX.hysteresis_frozen(cls.to(cuda)).cpu()
    assert torch.equal(want, path.float())           # every path pixel ends as 1, the rows between stay 0
    info = _hysteresis_equals(cuda, cls, want)
    assert info["batches"] >= 2 and info["sweeps"] <= cls.shape[-2] * cls.shape[-1]


def test_hysteresis_trivial_maps(cuda):
    cls, _ = FX.serpentine(strong=False)              # the path without its strong pixel: nothing to grow
    assert not FX.hysteresis_frozen(cls).any()
    info = _hysteresis_equals(cuda, cls, torch.zeros(cls.shape))
    assert info["batches"] == 1
    weak = torch.ones((1, 1, 70, 90), dtype=torch.uint8)
    weak[0, 0, 0, 0] = 2
    _hysteresis_equals(cuda, weak, torch.ones(weak.shape))
    info = _hysteresis_equals(cuda, torch.zeros((2, 1, 70, 90), dtype=torch.uint8), torch.zeros((2, 1, 70, 90)))
    assert info["batches"] == 1


# ---------------------------------------------------------------- 7. canny_classes
@pytest.mark.parametrize("seed", range(4))
def test_canny_classes_against_fp64(cuda, seed):
    img, mag64, cls64, margin = FX.canny_case(seed)
    ops.reset_stats()
    mag, cls = ops.canny_classes(img.to(cuda), 0.1, 0.3)
    assert ops.stats() == {("canny", "hip"): 1}
    assert mag.dtype == torch.float32 and cls.dtype == torch.uint8 and cls.shape == mag.shape == mag64.shape
    err = (mag.cpu().double() - mag64).abs().max().item()
    decided = margin > 2 * FX.CANNY_DELTA
    excluded = 1.0 - decided.double().mean().item()
    print(f"canny seed {seed}: max |mag - mag64| {err:.3e} (delta {FX.CANNY_DELTA:.3e}), excluded {excluded:.4%}, "
          f"classes {[int((cls64 == c).sum()) for c in (0, 1, 2)]}")
    assert err <= FX.CANNY_DELTA
    assert excluded <= 0.01
    assert (cls64 == 2).any() and (cls64 == 1).any()
    assert torch.equal(cls.cpu()[decided], cls64[decided])


def test_canny_classes_flat_images(cuda):
    for img in (torch.full((1, 3, 40, 70), 0.37), torch.zeros((2, 3, 40, 70)), torch.full((1, 1, 33, 65), 1.0)):
        _, cls = ops.canny_classes(img.to(cuda), 0.1, 0.3)
        assert not cls.any()


# ---------------------------------------------------------------- 8. canny end to end, nodes
def test_canny_end_to_end_and_node(cuda):
    img = torch.cat([FX.field(0), FX.field(1)]).to(cuda)
    ops.reset_stats()
    mag, edges = ops.canny(img, 0.1, 0.3)
    assert ops.stats() == {("canny", "hip"): 1}
    mag2, cls = ops.canny_classes(img, 0.1, 0.3)
    assert torch.equal(mag, mag2)
    assert torch.equal(edges.cpu(), FX.hysteresis_frozen(cls.cpu())) and edges.sum() > 0
    ops.reset_stats()
    y = NI.Canny().detect_edge(img.movedim(1, -1).contiguous(), 0.1, 0.3)[0]
    assert ops.stats() == {("canny", "hip"): 1}
    assert y.shape == (2, 70, 90, 3) and bool(((y == 0) | (y == 1)).all())
    assert torch.equal(y.to(cuda), edges.repeat(1, 3, 1, 1).movedim(1, -1))


def test_nodes_run_under_strict_native(cuda, monkeypatch):
    monkeypatch.setenv("CGS_STRICT_NATIVE", "1")
    img = FX.field(2).movedim(1, -1).contiguous().to(cuda)
    ops.reset_stats()
    b = NI.ImageBlur().blur(img, 5, 1.0)[0]
    s = NI.ImageSharpen().sharpen(img, 2, 1.0, 1.0)[0]
    m = NI.Morphology().process(img, "gradient", 7)[0]
    c = NI.Canny().detect_edge(img, 0.1, 0.3)[0]
    assert b.shape == s.shape == m.shape == c.shape == img.shape
    st = ops.stats()
    assert st == {("filter", "hip"): 2, ("morph", "hip"): 2, ("canny", "hip"): 1}
    assert torch.allclose(b.to(cuda), FX.blur_frozen(img, 5, 1.0), atol=1e-5)


# ---------------------------------------------------------------- 9. graph capture
def test_filter_sep_graph_capture(cuda):
    # under inference_mode, as the samplers capture: capture_begin updates the default generator's graph state in
    # place, and an earlier capture of the session may have created that state as inference tensors
    with torch.inference_mode():
        x = FX.filter_input((16, 4, 128, 128), torch.bfloat16, seed=13).to(cuda)
        taps = ops.gaussian_taps(9, 2.0, cuda, span="pixel")       # allocated before the capture
        eager = ops.filter_sep(x, taps)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                y = ops.filter_sep(x, taps)
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(2):
            y.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, eager)
