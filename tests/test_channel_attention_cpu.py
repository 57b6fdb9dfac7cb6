"""ops.channel_attention on the CPU (the composed path, bit for bit the four lines DAT's channel block had), its
domain and switch, and DAT with the switch on and off."""
import pytest
import torch
import torch.nn.functional as F

from comfy_gen_server_amd import ops


def test_channel_attention_cpu_is_the_old_composition():
    B, N, h, D = 2, 45, 3, 10
    C = h * D
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B, N, 3 * C, generator=g)
    temperature = torch.linspace(2, -1, h).view(h, 1, 1)
    q, k, v = qkv.view(B, N, 3, h, C // h).permute(2, 0, 3, 4, 1).unbind(0)
    s = F.normalize(q.float(), dim=-1) @ F.normalize(k.float(), dim=-1).transpose(-2, -1)
    att = (torch.softmax(s * temperature.float(), -1).to(v.dtype) @ v)
    att = att.permute(0, 3, 1, 2).reshape(B, N, C)
    ops.reset_stats()
    for fused in (True, False):
        for t in (temperature, temperature.reshape(h)):
            assert torch.equal(ops.channel_attention(qkv, h, t, fused=fused), att)
    assert ops.stats().get(("channel_attention", "torch"), 0) == 4


@pytest.mark.parametrize("heads,D,ok", [(1, 2, True), (6, 30, True), (8, 32, True), (6, 10, True), (4, 15, False),
                                        (4, 34, False), (4, 0, False), (0, 16, False)])
def test_channel_attention_domain(heads, D, ok):
    assert ops.channel_attention_domain(heads, D) is ok


def test_channel_attention_switch(monkeypatch):
    monkeypatch.delenv("CGS_CHANNEL_ATTN", raising=False)
    assert ops.channel_attention_enabled() is ops.core._CHANNEL_ATTN_DEFAULT
    for env, want in (("1", True), ("0", False), ("yes", False)):
        monkeypatch.setenv("CGS_CHANNEL_ATTN", env)
        assert ops.channel_attention_enabled() is want


def test_dat_channel_blocks_call_the_op(monkeypatch):
    from comfy_gen_server_amd.models.dat import AdaptiveChannelAttention
    from comfy_gen_server_amd.models.layers import init_random_
    blk = AdaptiveChannelAttention(32, 2)
    init_random_(blk, seed=2)
    blk.eval()
    x = torch.randn(1, 6 * 5, 32, generator=torch.Generator().manual_seed(0))
    out = {}
    with torch.no_grad():
        for sw in ("0", "1"):
            monkeypatch.setenv("CGS_CHANNEL_ATTN", sw)
            ops.reset_stats()
            out[sw] = blk(x, 6, 5)
            assert ops.stats().get(("channel_attention", "torch"), 0) == 1
    assert torch.equal(out["0"], out["1"])
