"""ops.narrow_linear on the CPU: the fp32 composition written out, and the SwinIR dim-60 model with
CGS_NARROW_LINEAR off and on (the fused wiring of the blocks against the composed one)."""
import pytest
import torch
import torch.nn.functional as F

from comfy_gen_server_amd import ops
from comfy_gen_server_amd.tools.window_attn_bench import swin_model


@pytest.mark.parametrize("act,res", [(None, False), ("gelu", False), (None, True), ("gelu", True)])
def test_cpu_path_equals_composition(act, res):
    g = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(2, 7, 60, generator=g) + 3.0, torch.randn(24, 60, generator=g), torch.randn(24, generator=g)
    gamma, beta, r = torch.randn(60, generator=g), torch.randn(60, generator=g), torch.randn(2, 7, 24, generator=g)
    want = F.linear(F.layer_norm(x, (60,), gamma, beta, 1e-5), w, b)
    want = F.gelu(want) if act else want
    want = want + r if res else want
    got = ops.narrow_linear(x, w, b, ln=(gamma, beta, 1e-5), act=act, residual=r if res else None)
    assert torch.equal(got, want)
    assert ops.narrow_linear_domain(60, 24) and not ops.narrow_linear_domain(62, 24) \
        and not ops.narrow_linear_domain(388, 24) and not ops.narrow_linear_domain(60, 6)


@pytest.mark.parametrize("kind", ["swinir", "swin2sr", "hat"])
def test_models_same_output_switch_off_and_on(monkeypatch, kind):
    m = swin_model(kind, dim=60, ws=8, heads=6, layers=2, depth=2, nf=32)
    x = torch.rand(1, 3, 24, 16, generator=torch.Generator().manual_seed(1))
    out = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("CGS_NARROW_LINEAR", sw)
        assert ops.narrow_linear_enabled() == (sw == "1")
        with torch.no_grad():
            out[sw] = m(x)
    assert (out["1"] - out["0"]).abs().max().item() <= 1e-5 * out["0"].abs().max().item()
