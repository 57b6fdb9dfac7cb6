"""Lanczos / bislerp resampling ops on the CPU: the PIL-free integer Lanczos reference against PIL itself,
and the torch paths of ``common_upscale(..., "lanczos" | "bislerp")`` against what they returned before
they became ops."""
import pytest
import torch

from comfy_gen_server_amd import ops
from comfy_gen_server_amd.utils import image as U

from _resample import (LANCZOS_IDS, LANCZOS_SHAPES, bislerp_fp32, bislerp_input, lanczos_input, pil_lanczos)


@pytest.mark.parametrize("src,dst", LANCZOS_SHAPES, ids=LANCZOS_IDS)
def test_lanczos_reference_equals_pil(src, dst):
    x = lanczos_input(1, *src)
    want = U.lanczos(x, dst[1], dst[0])
    assert torch.equal(want, pil_lanczos(x, dst[1], dst[0]))
    got = ops.lanczos_reference(x, dst[1], dst[0])
    assert got.shape == want.shape and got.dtype == want.dtype
    assert torch.equal(got, want)


def test_lanczos_tables_are_pil_coefficients():
    # 4 -> 2: scale 2, support 6, every window clamped to the whole axis; taps sum to 2^22 within rounding
    bounds, coef = ops.lanczos_tables(4, 2)
    assert bounds.tolist() == [[0, 4], [0, 4]] and coef.shape == (2, 4)
    assert abs(int(coef[0].sum()) - (1 << 22)) <= 2 and coef[0].tolist() == coef[1].tolist()[::-1]
    bounds, coef = ops.lanczos_tables(5, 11)
    assert bounds[:, 0].min() == 0 and (bounds[:, 0] + bounds[:, 1]).max() == 5
    assert (coef < 0).any()


def test_common_upscale_lanczos_cpu_is_the_pil_path():
    x = lanczos_input(2, 24, 31)
    ops.reset_stats()
    y = U.common_upscale(x, 17, 40, "lanczos", "disabled")
    assert ops.stats().get(("resample", "torch")) == 1 and ("resample", "hip") not in ops.stats()
    assert torch.equal(y, pil_lanczos(x, 17, 40))
    # other channel counts and dtypes keep going through PIL
    x4 = lanczos_input(1, 12, 10)[:, :1].expand(-1, 4, -1, -1).contiguous()
    assert torch.equal(U.common_upscale(x4, 7, 9, "lanczos", "disabled"), pil_lanczos(x4, 7, 9))
    xh = x.half()
    assert torch.equal(U.common_upscale(xh, 17, 40, "lanczos", "disabled"), pil_lanczos(xh, 17, 40))
    # center crop happens before the resize, as before
    yc = U.common_upscale(x, 16, 16, "lanczos", "center")
    assert torch.equal(yc, pil_lanczos(x[:, :, :, 4:27], 16, 16))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_common_upscale_bislerp_cpu_is_the_torch_path(dtype):
    x = bislerp_input((2, 4, 9, 13), dtype)
    ops.reset_stats()
    y = U.common_upscale(x, 30, 21, "bislerp", "disabled")
    assert ops.stats().get(("resample", "torch")) == 1 and ("resample", "hip") not in ops.stats()
    assert y.dtype == dtype and y.shape == (2, 4, 21, 30)
    assert torch.equal(y, bislerp_fp32(x, 30, 21))
    xp = bislerp_input("pairs", dtype)
    assert torch.equal(U.bislerp(xp, 11, 7), bislerp_fp32(xp, 11, 7))


def test_bislerp_tables_are_the_reference_coords():
    c1, c2, r = ops.bislerp_tables(13, 30)
    ramp = torch.arange(30, dtype=torch.float32) * (13 / 30)
    assert torch.equal(c1, ramp.floor().long()) and torch.equal(r, ramp - ramp.floor())
    assert torch.equal(c2, (c1 + 1).clamp(max=12)) and r.dtype == torch.float32
