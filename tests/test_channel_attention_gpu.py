"""The channel attention kernels (csrc/kernels/channel_attn.hip, ops.channel_attention) on the device: per-element
bounds against an fp64 reference in plain torch, output integrity, entry refusals, and DAT with the switch on and off."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _bounds import assert_within                                                        # noqa: E402
from _bounds_channel import channel_attention_bound, channel_attention_probs            # noqa: E402

from comfy_gen_server_amd import _native, ops                                            # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
INVALID = 1          # hipErrorInvalidValue
CASES = [(1, 1, 1, 2), (1, 37, 2, 10), (1, 257, 3, 16), (1, 64, 1, 18), (2, 300, 6, 30), (3, 1024, 8, 32),
         (1, 4099, 6, 30)]


def _inputs(B, N, heads, D):
    """Peaked, asymmetric P: k is q rolled by one channel plus noise, temperatures from 6 down to -4."""
    g = torch.Generator().manual_seed(1000 * N + D)
    q = torch.randn(B, N, heads, D, generator=g)
    k = 0.8 * torch.roll(q, 1, -1) + 0.6 * torch.randn(B, N, heads, D, generator=g)
    v = torch.randn(B, N, heads, D, generator=g)
    temp = torch.linspace(6, -4, heads) if heads > 1 else torch.tensor([6.0])
    return torch.stack([q, k, v], 2).reshape(B, N, 3 * heads * D).to(BF), temp


@pytest.mark.parametrize("B,N,heads,D", CASES)
def test_channel_attention_bound(cuda, B, N, heads, D):
    qkv, temp = _inputs(B, N, heads, D)
    chunk = _native.load_kernels().cgs_channel_attn_chunk(B, N, heads, D)
    assert chunk > 0 and (N != 4099 or -(-N // chunk) >= 3), chunk      # several chunks with a tail in the last
    ref, tol = channel_attention_bound(qkv, heads, temp, chunk)
    if N >= 37:
        assert channel_attention_probs(qkv, heads, temp)[0][:, 0].amax(-1).min().item() > 0.5
    ops.reset_stats()
    y = ops.channel_attention(qkv.to(cuda), heads, temp.to(cuda))
    st = ops.stats()
    assert st.get(("channel_attention", "hip"), 0) == 1 and not [k for k in st if k[1] == "lib"], st
    assert_within(y.cpu(), ref, tol, f"channel_attention {(B, N, heads, D)}")
    assert torch.equal(y, ops.channel_attention(qkv.to(cuda), heads, temp.to(cuda)))       # fixed summation order


def test_channel_attention_refusals_and_integrity(cuda):
    """A good call writes every element of o finite (qkv ends its NaN-filled buffer: an unmasked pad read would
    poison o) and no bit around it; each single broken rule returns hipErrorInvalidValue and leaves o's bits alone."""
    lib = _native.load_kernels()
    good = dict(B=1, N=37, heads=3, D=18, temp=True, ws=True, short=0, qoff=0, ooff=0)
    broken = {"odd D": dict(D=17), "D cap": dict(D=34), "D low": dict(D=0), "heads": dict(heads=0), "N": dict(N=0),
              "B": dict(B=0), "temperature": dict(temp=False), "no ws": dict(ws=False), "small ws": dict(short=16),
              "qkv align": dict(qoff=2), "o align": dict(ooff=2)}
    n3 = 37 * 3 * 3 * 18
    src, temp = _inputs(1, 37, 3, 18)
    qbuf = torch.full((4096 + n3,), float("nan"), device=cuda, dtype=BF)
    qbuf[4096:] = src.reshape(-1).to(cuda)
    temp = temp.to(cuda)
    nbytes = lib.cgs_channel_attn_ws_bytes(1, 37, 3, 18)
    ws = torch.zeros(nbytes, device=cuda, dtype=torch.uint8)
    for name, change in [("good", {})] + list(broken.items()):
        a = {**good, **change}
        n = 37 * 3 * 18
        buf = torch.full((n + 512,), float("nan"), device=cuda, dtype=BF)
        before = buf.view(torch.int16).clone()
        err = lib.cgs_channel_attn_fwd(qbuf.data_ptr() + 2 * 4096 + a["qoff"], buf.data_ptr() + 512 + a["ooff"],
                                       temp.data_ptr() if a["temp"] else None, ws.data_ptr() if a["ws"] else None,
                                       nbytes - a["short"], a["B"], a["N"], a["heads"], a["D"],
                                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        after = buf.view(torch.int16)
        if name == "good":
            assert err == 0 and bool(torch.isfinite(buf[256:256 + n]).all())
            assert torch.equal(after[:256], before[:256]) and torch.equal(after[256 + n:], before[256 + n:])
        else:
            assert err == INVALID, (name, err)
            assert torch.equal(after, before), name


def test_dat_switch(cuda, monkeypatch):
    """Switch on: one fused call per channel block (4); off: none. Both within 3e-2 of the fp32 CPU model; the fused
    run reaches no vendor library that the composed run does not."""
    from comfy_gen_server_amd.models import upscalers
    from comfy_gen_server_amd.models.dat import DAT
    from comfy_gen_server_amd.models.layers import init_random_
    Z = torch.zeros
    seed = {"conv_first.weight": Z(64, 3, 3, 3), "conv_before_upsample.0.weight": Z(64, 64, 3, 3),
            "upsample.0.weight": Z(256, 64, 3, 3), "conv_last.weight": Z(3, 64, 3, 3),
            "layers.0.blocks.1.attn.temperature": Z(4, 1, 1), "layers.0.blocks.0.ffn.fc1.weight": Z(128, 64),
            "layers.0.blocks.2.attn.attn_mask_0": Z(1)}
    seed.update({f"layers.{i}.blocks.{j}.norm1.weight": Z(64) for i in range(2) for j in range(4)})
    m = DAT(seed, strict=False)
    init_random_(m, seed=4)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["layers.0.blocks.2.attn.attn_mask_0"] = Z(1)
    m = upscalers.load_state_dict(sd)
    x = torch.rand(1, 3, 40, 32, generator=torch.Generator().manual_seed(1))
    libs = {}
    with torch.no_grad():
        ref = m(x)
        g = m.to(device=cuda, dtype=BF)
        for sw in ("1", "0"):
            monkeypatch.setenv("CGS_CHANNEL_ATTN", sw)
            ops.reset_stats()
            out = g(x.to(cuda, BF)).float().cpu()
            st = ops.stats()
            assert st.get(("channel_attention", "hip"), 0) == (4 if sw == "1" else 0), st
            libs[sw] = {k for k in st if k[1] == "lib"}
            assert ((out - ref).norm() / ref.norm()).item() < 3e-2
    assert libs["1"] <= libs["0"], libs
