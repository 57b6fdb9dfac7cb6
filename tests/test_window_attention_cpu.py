"""ops.window_attention on the CPU: the composed fp32 path equals the Swin models' own roll / partition /
attention_bias / reverse / roll composition, and the models give the same output with CGS_WINDOW_ATTN off and on."""
import math

import pytest
import torch

from comfy_gen_server_amd import ops
from comfy_gen_server_amd.models import swin_sr
from comfy_gen_server_amd.models.layers import init_random_
from comfy_gen_server_amd.tools.window_attn_bench import swin_model


@pytest.mark.parametrize("shift,v2", [(4, False), (4, True)])
def test_cpu_path_equals_model_composition(shift, v2):
    B, H, W, ws, heads, dim = 2, 16, 24, 8, 3, 24
    attn = swin_sr.WindowAttention(dim, ws, heads, v2=v2)
    init_random_(attn, seed=3)
    x = torch.randn(B, H * W, dim, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        y = torch.roll(x.view(B, H, W, dim), (-shift, -shift), (1, 2))
        y = attn(swin_sr._partition(y, ws), swin_sr.shift_mask(H, W, ws, shift, x.device))
        want = torch.roll(swin_sr._reverse(y, ws, B, H, W), (shift, shift), (1, 2)).reshape(B, H * W, dim)
        if v2:
            table = 16 * torch.sigmoid(attn.cpb_mlp(attn.coords_table))
            o = ops.window_attention(attn._qkv(x), (H, W), ws, shift, heads, table, scale=1.0, cosine=True,
                                     head_scale=torch.clamp(attn.logit_scale, max=math.log(100.0)).exp())
        else:
            o = ops.window_attention(attn._qkv(x), (H, W), ws, shift, heads, attn.relative_position_bias_table)
        got = attn.proj(o)
    assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item()


def _swin_model(kind):
    """SwinIR / Swin2SR / HAT at the shapes of test_upscale.py's _random_swin, randomly initialised."""
    return swin_model(kind, dim=48, ws=8, heads=3, layers=2, depth=2, nf=32)


@pytest.mark.parametrize("kind", ["swinir", "swin2sr", "hat"])
def test_models_same_output_switch_off_and_on(monkeypatch, kind):
    m = _swin_model(kind)
    x = torch.rand(1, 3, 24, 16, generator=torch.Generator().manual_seed(1))
    out = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("CGS_WINDOW_ATTN", sw)
        ops.reset_stats()
        with torch.no_grad():
            out[sw] = m(x)
        assert ops.stats().get(("window_attention", "torch"), 0) == (4 if sw == "1" else 0)
    assert (out["1"] - out["0"]).abs().max().item() <= 1e-5 * out["0"].abs().max().item()
