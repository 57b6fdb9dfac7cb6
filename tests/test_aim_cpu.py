"""ops.adaptive_interaction and ops.token_dwconv3x3 on the CPU: bit for bit the lines DAT's blocks had."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bounds_aim import aim_modules                                                      # noqa: E402

from comfy_gen_server_amd import ops                                                     # noqa: E402

B, H, W, C = 2, 5, 7, 24


@pytest.mark.parametrize("kind", ["spatial", "channel"])
def test_adaptive_interaction_cpu_is_the_old_composition(kind):
    g = torch.Generator().manual_seed(2)
    qkv, att = torch.randn(B, H * W, 3 * C, generator=g), torch.randn(B, H * W, C, generator=g)
    dw, ci, si = mods = aim_modules(C, 3, 1, 7)
    img = lambda t: t.transpose(1, 2).reshape(B, C, H, W)                                # noqa: E731
    with torch.no_grad():
        v = img(qkv[..., 2 * C:])
        conv = dw(v.contiguous() if kind == "spatial" else v)      # the channel block passed the strided view
        if kind == "spatial":
            want = att * torch.sigmoid(ci(conv).view(B, 1, C)) \
                + (torch.sigmoid(si(img(att))) * conv).flatten(2).transpose(1, 2)
        else:
            want = att * torch.sigmoid(si(conv).flatten(2).transpose(1, 2)) \
                + (conv * torch.sigmoid(ci(img(att)))).flatten(2).transpose(1, 2)
        ops.reset_stats()
        for fused in (True, False):
            assert torch.equal(ops.adaptive_interaction(qkv, att, (H, W), mods, kind, fused=fused), want)
    assert ops.stats().get(("adaptive_interaction", "torch"), 0) == 2


def test_token_dwconv3x3_cpu_is_the_old_gate():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, H * W, 2 * C, generator=g)
    a, gt = x.chunk(2, -1)
    conv = aim_modules(C, 3, 1, 8)[0][0]
    with torch.no_grad():
        want = a * conv(gt.transpose(1, 2).reshape(B, C, H, W).contiguous()).flatten(2).transpose(1, 2)
        assert torch.equal(ops.token_dwconv3x3(gt, (H, W), conv.weight, conv.bias, mul=a), want)
