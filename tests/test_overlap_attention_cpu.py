"""ops.overlap_attention on the CPU (the composed path) against an fp64 unfold reference written here, and HAT with
the switch on and off."""
import pytest
import torch
import torch.nn.functional as F

from comfy_gen_server_amd import ops
from comfy_gen_server_amd.models.swin_sr import _rel_index_oca
from comfy_gen_server_amd.tools.window_attn_bench import swin_model


@pytest.mark.parametrize("ws,ows", [(8, 12), (16, 24)])
def test_overlap_attention_cpu(monkeypatch, ws, ows):
    B, H, W, heads, D = 2, 2 * ws, 3 * ws, 3, 10
    C, Nq, Nk = heads * D, ws * ws, ows * ows
    g = torch.Generator().manual_seed(ws)
    qkv = torch.randn(B, H * W, 3 * C, generator=g)
    table = torch.randn((ws + ows - 1) ** 2, heads, generator=g)
    img = qkv.double().reshape(B, H, W, 3, C)
    q = img[..., 0, :].reshape(B, H // ws, ws, W // ws, ws, heads, D).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, heads, Nq, D)
    kv = F.unfold(img[..., 1:, :].reshape(B, H, W, 2 * C).permute(0, 3, 1, 2), ows, stride=ws, padding=(ows - ws) // 2)
    k, v = kv.view(B, 2, heads, D, Nk, -1).permute(1, 0, 5, 2, 4, 3).reshape(2, -1, heads, Nk, D)
    bias = table.double()[_rel_index_oca(ws, ows)].permute(2, 0, 1)
    o = torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5 + bias, -1) @ v
    ref = o.reshape(B, H // ws, W // ws, heads, ws, ws, D).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, H * W, C)
    ops.reset_stats()
    y = ops.overlap_attention(qkv, (H, W), ws, ows, heads, table)
    assert ops.stats().get(("overlap_attention", "torch"), 0) == 1
    assert (y.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()

    m = swin_model("hat", dim=48, ws=ws, heads=3, layers=1, depth=2, nf=32)
    x = torch.rand(1, 3, 2 * ws + 3, 2 * ws, generator=g)
    out = {}
    with torch.no_grad():
        for sw in ("0", "1"):
            monkeypatch.setenv("CGS_OVERLAP_ATTN", sw)
            out[sw] = m(x)
    assert (out["1"] - out["0"]).abs().max().item() <= 1e-5 * out["0"].abs().max().item()
