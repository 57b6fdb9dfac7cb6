"""``ops.conv2d_into`` without a device: the layout helper, the aliasing rules, the torch path (the oracle of the
device tests) on views of wider channels-last buffers, and the dense blocks of models/upscalers.py, whose CPU
forward must not move."""
import pytest
import torch
import torch.nn.functional as F

from comfy_gen_server_amd import ops
from comfy_gen_server_amd.models import upscalers
from comfy_gen_server_amd.models.layers import init_random_
from comfy_gen_server_amd.ops.core import conv_slice_layout


def _buf(N, C, H, W, dtype=torch.float32, fill=None):
    b = torch.empty((N, C, H, W), dtype=dtype).contiguous(memory_format=torch.channels_last)
    if fill is None:
        b.copy_(torch.randn(N, C, H, W))
    else:
        b.fill_(fill)
    return b


def _layout(t):
    return conv_slice_layout(t.shape, t.stride(), t.storage_offset())


def test_layout_accepts():
    buf = _buf(2, 192, 5, 7)
    assert _layout(buf[:, :96]) == (192, 5 * 7 * 192, True)              # prefix
    assert _layout(buf[:, 32:96]) == (192, 5 * 7 * 192, True)            # interior slice, channel offset 32
    assert _layout(buf[:, 96:128]) == (192, 5 * 7 * 192, True)
    assert _layout(_buf(2, 64, 5, 7)) == (64, 5 * 7 * 64, True)          # dense, P == C
    assert _layout(buf[:1, :64])[2] and _layout(_buf(1, 32, 1, 9))[2]    # size-1 dimensions: their stride is free


def test_layout_rejects():
    assert not _layout(torch.randn(2, 64, 5, 7))[2]                      # NCHW-contiguous
    assert not _layout(torch.randn(2, 64, 5, 7)[:, :32])[2]
    assert not _layout(_buf(2, 100, 5, 7)[:, :64])[2]                    # pitch 100: no multiple of 8
    assert not _layout(_buf(2, 192, 5, 7)[:, 4:68])[2]                   # channel offset 4
    assert not _layout(_buf(2, 192, 5, 7)[:, :, ::2])[2]                 # rows not packed
    assert not conv_slice_layout((64, 5, 7), (1, 7 * 64, 64), 0)[2]      # not 4-D
    assert not conv_slice_layout((2, 64, 5, 7, 1), (2240, 1, 448, 64, 1), 0)[2]


def _wb(cin, cout, bias=True):
    w = torch.randn(cout, cin, 3, 3) / (9 * cin) ** 0.5
    return w, (torch.randn(cout) if bias else None)


def test_aliasing_and_shape_errors():
    buf = _buf(1, 192, 6, 6)
    w, b = _wb(64, 32)
    before = buf.clone()
    with pytest.raises(ValueError):          # out inside the channels read
        ops.conv2d_into(buf[:, :64], w, b, buf[:, 32:64])
    with pytest.raises(ValueError):          # out straddles their end
        ops.conv2d_into(buf[:, :64], w, b, buf[:, 48:80])
    with pytest.raises(ValueError):          # residual partially over out
        ops.conv2d_into(buf[:, :64], w, b, buf[:, 64:96], residual=buf[:, 80:112])
    with pytest.raises(ValueError):          # residual2 partially over out
        ops.conv2d_into(buf[:, :64], w, b, buf[:, 64:96], residual2=buf[:, 48:80])
    other = _buf(1, 64, 6, 5)
    with pytest.raises(ValueError):          # W differs
        ops.conv2d_into(buf[:, :64], w, b, other[:, :32])
    with pytest.raises(ValueError):          # N differs
        ops.conv2d_into(buf[:, :64], w, b, _buf(2, 32, 6, 6))
    with pytest.raises(ValueError):          # H of the residual differs
        ops.conv2d_into(buf[:, :64], w, b, buf[:, 64:96], residual=_buf(1, 32, 5, 6))
    with pytest.raises(ValueError):          # weight for another Cin
        ops.conv2d_into(buf[:, :96], w, b, buf[:, 96:128])
    with pytest.raises(ValueError):
        ops.conv2d_into(buf[:, :64], w, b, buf[:, 64:96], act="tanh")
    assert torch.equal(buf, before)          # nothing ran
    # legal: out behind or before the channels read, the residuals out itself or apart from it
    ops.conv2d_into(buf[:, :64], w, b, buf[:, 64:96], residual=buf[:, 64:96], residual2=buf[:, 96:128])
    ops.conv2d_into(buf[:, 32:96], w, b, buf[:, :32], residual=buf[:, 160:192])


EPILOGUES = [dict(), dict(act="leaky_relu", act_param=0.2), dict(act="silu"), dict(alpha=0.2, res=True),
             dict(alpha=0.04, beta=0.2, res=True, res2=True), dict(bias=False)]


@pytest.mark.parametrize("epi", EPILOGUES, ids=lambda e: "-".join(e) or "bias")
def test_torch_path_matches_cat_formula(epi):
    """conv2d_into on CPU views against the same fp32 formula on materialised tensors, bit for bit; the buffer's
    other channels keep their bits."""
    torch.manual_seed(1)
    N, H, W, nf, gc = 2, 5, 7, 32, 16
    buf = _buf(N, nf + 4 * gc, H, W)
    rbuf, r2buf = _buf(N, 64, H, W), _buf(N, 40, H, W)
    feats = [buf[:, :nf].clone()] + [buf[:, nf + i * gc:nf + (i + 1) * gc].clone() for i in range(2)]
    cin = nf + 2 * gc
    w, b = _wb(cin, gc, epi.get("bias", True))
    res = rbuf[:, 16:16 + gc] if epi.get("res") else None
    res2 = r2buf[:, 8:8 + gc] if epi.get("res2") else None
    alpha, beta, act, p = epi.get("alpha", 1.0), epi.get("beta", 1.0), epi.get("act"), epi.get("act_param", 0.0)
    want = F.conv2d(torch.cat(feats, 1), w, b, 1, 1)
    if act == "leaky_relu":
        want = F.leaky_relu(want, p)
    elif act == "silu":
        want = F.silu(want)
    want = alpha * want
    if res is not None:
        want = want + beta * res.clone()
    if res2 is not None:
        want = want + res2.clone()
    before = buf.clone()
    ops.reset_stats()
    got = ops.conv2d_into(buf[:, :cin], w, b, buf[:, cin:cin + gc], act=act, act_param=p, alpha=alpha, residual=res,
                          beta=beta, residual2=res2)
    assert ops.stats() == {("conv", "torch"): 1}, ops.stats()
    assert got.data_ptr() == buf[:, cin:cin + gc].data_ptr() and got.stride() == buf[:, cin:cin + gc].stride()
    assert torch.equal(buf[:, cin:cin + gc], want)
    assert torch.equal(buf[:, :cin], before[:, :cin]) and torch.equal(buf[:, cin + gc:], before[:, cin + gc:])


def test_torch_path_bf16_and_in_place_residual():
    """bf16 views: fp32 math, one rounding at the store; ``residual2`` being ``out`` itself reads before it writes."""
    torch.manual_seed(2)
    buf = _buf(1, 96, 6, 9, torch.bfloat16)
    w, b = _wb(64, 32)
    w, b = w.to(torch.bfloat16), b.to(torch.bfloat16)
    old = buf[:, 64:96].clone()
    want = (0.5 * F.conv2d(buf[:, :64].float(), w.float(), b.float(), 1, 1) + old.float()).to(torch.bfloat16)
    ops.conv2d_into(buf[:, :64], w, b, buf[:, 64:96], alpha=0.5, residual2=buf[:, 64:96])
    assert torch.equal(buf[:, 64:96], want)


def _rdb_old(m, x):
    """ResidualDenseBlock5C.forward as it was before the dense path."""
    feats = [x]
    for i in range(4):
        c = getattr(m, f"conv{i + 1}")[0]
        feats.append(F.leaky_relu(F.conv2d(torch.cat(feats, 1), c.weight, c.bias, 1, 1), 0.2))
    return F.conv2d(torch.cat(feats, 1), m.conv5[0].weight, m.conv5[0].bias, 1, 1) * 0.2 + x


@pytest.mark.parametrize("mode", ["", "0", "1"])
def test_models_cpu_unchanged(monkeypatch, mode):
    """On the CPU the dense blocks compute what they always did, whatever CGS_DENSE_CONV says."""
    if mode:
        monkeypatch.setenv("CGS_DENSE_CONV", mode)
    else:
        monkeypatch.delenv("CGS_DENSE_CONV", raising=False)
    with torch.no_grad():
        m = upscalers.ResidualDenseBlock5C(32, 16)
        init_random_(m, seed=4)
        x = torch.randn(2, 32, 9, 7)
        assert torch.equal(m(x), _rdb_old(m, x))
        r = upscalers.RRDB(32, 16)
        init_random_(r, seed=5)
        want = _rdb_old(r.RDB3, _rdb_old(r.RDB2, _rdb_old(r.RDB1, x))) * 0.2 + x
        assert torch.equal(r(x), want)
        t = upscalers._Trunk(32, 2, 16)
        init_random_(t, seed=6)
        h = x
        for blk in t.sub[:-1]:
            h = _rdb_old(blk.RDB3, _rdb_old(blk.RDB2, _rdb_old(blk.RDB1, h))) * 0.2 + h
        c = t.sub[-1]
        assert torch.equal(t(x), F.conv2d(h, c.weight, c.bias, 1, 1) + x)
