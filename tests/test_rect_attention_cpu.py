"""ops.rect_window_attention on the CPU (the composed path, moved out of DAT's spatial block) against the fp64
reference of _ref_rect.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _ref_rect import rect_attention_reference                             # noqa: E402

from comfy_gen_server_amd import ops                                       # noqa: E402


@pytest.mark.parametrize("B,H,W,split,heads,D,shifted", [(2, 12, 20, (8, 16), 4, 6, True),
                                                         (1, 32, 16, (32, 8), 2, 8, False)])
def test_rect_attention_cpu(B, H, W, split, heads, D, shifted):
    g = torch.Generator().manual_seed(H * W + D)
    qkv = torch.randn(B, H * W, 3 * heads * D, generator=g)
    tables = [torch.randn((2 * split[0] - 1) * (2 * split[1] - 1), heads // 2, generator=g) for _ in range(2)]
    ref, _ = rect_attention_reference(qkv, H, W, split, shifted, heads, tables)
    ops.reset_stats()
    y = ops.rect_window_attention(qkv, (H, W), split, shifted, heads, tables)
    assert ops.stats().get(("rect_window_attention", "torch"), 0) == 1
    # fp32 composition rounding: outputs are convex combinations of |v| = O(1), a few dozen fp32 operations each
    torch.testing.assert_close(y.double(), ref, rtol=1e-5, atol=1e-5)
    assert torch.equal(y, ops.rect_window_attention(qkv, (H, W), split, shifted, heads, tables, fused=False))
