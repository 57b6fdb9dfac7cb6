"""cgs_conv3x3_slice / ``ops.conv2d_into`` on the device (csrc/kernels/dense.hip): the kernel against its per-element
bound, channel slices of wider buffers (what is read, what is written, what is left alone), the refusals of the C
entry, the dense blocks of models/upscalers.py on it, and graph capture."""
import ctypes
import json

import pytest
import torch

from comfy_gen_server_amd import _native, ops
from comfy_gen_server_amd.models import upscalers
from comfy_gen_server_amd.models.layers import init_random_

from _bounds import assert_within
from _bounds_dense import conv_into_bound

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
INVALID = 1      # hipErrorInvalidValue

# (N, Cin, H, W, Cout)
SHAPES = [(2, 32, 5, 7, 32),        # one chunk, image smaller than a patch, image index
          (1, 64, 16, 16, 32),      # exact patch
          (1, 96, 24, 20, 32),      # odd chunk count, partial patches on both axes
          (1, 160, 17, 33, 32),     # one-pixel overhang
          (1, 192, 16, 48, 64),     # NB = 4
          (1, 64, 9, 40, 16),       # NB = 1
          (1, 128, 20, 20, 48)]     # NB = 3
EPILOGUES = {"bias": dict(), "lrelu": dict(act="leaky_relu", act_param=0.2), "silu": dict(act="silu"),
             "alpha-res": dict(alpha=0.2, res=True), "alpha-beta-res-res2": dict(alpha=0.04, beta=0.2, res=True, res2=True),
             "nobias": dict(bias=False)}


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _operands(N, Cin, H, W, Cout, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g).to(BF)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).to(BF)
    b = torch.randn(Cout, generator=g).to(BF) if bias else None
    r = torch.randn(N, Cout, H, W, generator=g).to(BF)
    r2 = torch.randn(N, Cout, H, W, generator=g).to(BF)
    return x, w, b, r, r2


def _wn(w, dev):
    return w.to(dev).permute(0, 2, 3, 1).contiguous()


def _buffer(N, C, H, W, dev, fill=float("nan")):
    return torch.full((N, C, H, W), fill, device=dev, dtype=BF).contiguous(memory_format=torch.channels_last)


def _bits(t):
    """Every element of the storage under ``t`` as int16 (NaN payloads included)."""
    return torch.empty(0, dtype=torch.int16, device=t.device).set_(
        t.untyped_storage(), 0, (t.untyped_storage().nbytes() // 2,)).clone()


def _view_of(bits, like):
    """The elements of the view ``like`` inside ``bits``, a flat int16 copy of its storage."""
    return bits.as_strided(tuple(like.shape), tuple(like.stride()), like.storage_offset())


def _dense_counts():
    st = ops.stats()
    assert not any(k[1] == "lib" for k in st), st
    return st.get(("conv_dense", "hip"), 0)


@pytest.mark.parametrize("epi", list(EPILOGUES), ids=list(EPILOGUES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_bound(cuda, shape, epi):
    N, Cin, H, W, Cout = shape
    e = EPILOGUES[epi]
    x, w, b, r, r2 = _operands(N, Cin, H, W, Cout, seed=sum(shape), bias=e.get("bias", True))
    res, res2 = (r if e.get("res") else None), (r2 if e.get("res2") else None)
    act, p, alpha, beta = e.get("act"), e.get("act_param", 0.0), e.get("alpha", 1.0), e.get("beta", 1.0)
    ref, tol = conv_into_bound(x, w, b, act, p, alpha, res, beta, res2)
    out = torch.empty((N, Cout, H, W), device=cuda, dtype=BF).contiguous(memory_format=torch.channels_last)
    ops.reset_stats()
    y = ops.conv2d_into(_nhwc(x.to(cuda)), w.to(cuda), None if b is None else b.to(cuda), out, weight_nhwc=_wn(w, cuda),
                        act=act, act_param=p, alpha=alpha, residual=None if res is None else _nhwc(res.to(cuda)),
                        beta=beta, residual2=None if res2 is None else _nhwc(res2.to(cuda)))
    assert y is out and _dense_counts() == 1
    assert ops.stats().get(("act_fused", "hip"), 0) == (1 if act else 0)
    assert_within(out.cpu(), ref, tol, f"conv2d_into {shape} {epi}")


# ---------------------------------------------------------------------------------------------------------- slices
def _slice_case(cuda, N, H, W, Cin, Cout, c0, make_out, seed, res_kind=None, res2_is_out=False):
    """x = buf[:, c0:c0 + Cin] of a [N, 192, H, W] buffer that is NaN outside those channels; ``make_out(buf)`` returns
    (out view, the buffers to watch). Checks the bound, and that no element outside out's slice changed."""
    x, w, b, r, r2 = _operands(N, Cin, H, W, Cout, seed)
    buf = _buffer(N, 192, H, W, cuda)
    buf[:, c0:c0 + Cin] = x.to(cuda)
    out, watch = make_out(buf)
    res = res2 = None
    rv = r2v = None
    if res_kind == "pitch":          # a residual from a buffer of another pitch than out's
        rbuf = _buffer(N, 96, H, W, cuda)
        rbuf[:, 8:8 + Cout] = r.to(cuda)
        res, rv = rbuf[:, 8:8 + Cout], r
        watch = watch + [rbuf]
    if res2_is_out:
        out.copy_(r2.to(cuda))
        res2, r2v = out, r2
    alpha, beta = (0.04, 0.2) if res is not None else (0.5, 1.0)
    ref, tol = conv_into_bound(x, w, b, "leaky_relu", 0.2, alpha, rv, beta, r2v)
    before = [_bits(t) for t in watch]
    ops.reset_stats()
    ops.conv2d_into(buf[:, c0:c0 + Cin], w.to(cuda), b.to(cuda), out, weight_nhwc=_wn(w, cuda), act="leaky_relu",
                    act_param=0.2, alpha=alpha, residual=res, beta=beta, residual2=res2)
    assert _dense_counts() == 1
    assert_within(out.cpu(), ref, tol, f"slice case c0={c0} Cin={Cin} Cout={Cout}")
    for t, b0 in zip(watch, before):
        a0 = _bits(t)
        if t.untyped_storage().data_ptr() == out.untyped_storage().data_ptr():
            _view_of(a0, out).copy_(_view_of(b0, out))      # out's own elements put back: nothing else may differ
        assert torch.equal(a0, b0), "an element outside out's slice changed"


def test_slice_in_place(cuda):
    """out right behind the channels read, in the same buffer."""
    _slice_case(cuda, 2, 9, 21, 96, 32, 0, lambda buf: (buf[:, 96:128], [buf]), seed=31)


def test_slice_other_buffer(cuda):
    """out in a second buffer at pitch 256, channel offset 64."""
    def make(buf):
        o = _buffer(buf.shape[0], 256, buf.shape[2], buf.shape[3], buf.device)
        return o[:, 64:96], [buf, o]
    _slice_case(cuda, 2, 9, 21, 96, 32, 0, make, seed=32)


def test_slice_plain_out(cuda):
    def make(buf):
        o = _buffer(buf.shape[0], 48, buf.shape[2], buf.shape[3], buf.device)
        return o, [buf, o]
    _slice_case(cuda, 1, 17, 18, 128, 48, 0, make, seed=33)


def test_slice_interior_x(cuda):
    """x = buf[:, 32:96]: channels 0-31 and 96-191 are NaN, so one channel read too many or too early shows."""
    _slice_case(cuda, 2, 9, 21, 64, 32, 32, lambda buf: (buf[:, 96:128], [buf]), seed=34)
    _slice_case(cuda, 1, 18, 9, 64, 16, 32, lambda buf: (buf[:, 8:24], [buf]), seed=35)


def test_slice_residual_other_pitch(cuda):
    _slice_case(cuda, 2, 9, 21, 96, 32, 0, lambda buf: (buf[:, 96:128], [buf]), seed=36, res_kind="pitch")


def test_slice_residual2_is_out(cuda):
    _slice_case(cuda, 2, 9, 21, 96, 64, 0, lambda buf: (buf[:, 128:192], [buf]), seed=37, res2_is_out=True)
    _slice_case(cuda, 1, 20, 17, 96, 32, 0, lambda buf: (buf[:, 96:128], [buf]), seed=38, res_kind="pitch",
                res2_is_out=True)


# ------------------------------------------------------------------------------------------------- entry refusals
def _entry(x, xp, xs, w, bias, out, op, os_, N, H, W, Cin, Cout, res=None, rp=0, rs=0):
    lib = _native.load_kernels()
    return lib.cgs_conv3x3_slice(x, xp, xs, w, bias, res, rp, rs, None, 0, 0, out, op, os_, N, H, W, Cin, Cout, 0, 0.0,
                                 1.0, 1.0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_entry_refusals(cuda):
    """Each broken rule returns hipErrorInvalidValue and launches nothing: the buffers keep their bits."""
    N, H, W = 1, 8, 8
    buf = _buffer(N, 192, H, W, cuda, fill=1.0)
    odd = _buffer(N, 100, H, W, cuda, fill=1.0)
    w = torch.ones(80 * 9 * 192, device=cuda, dtype=BF)
    b = torch.ones(80, device=cuda, dtype=BF)
    p, P = buf.data_ptr(), 192
    S = H * W * P
    before = [_bits(buf), _bits(odd)]
    ok = dict(x=p, xp=P, xs=S, w=w.data_ptr(), bias=b.data_ptr(), out=p + 2 * 64, op=P, os_=S, N=N, H=H, W=W, Cin=64,
              Cout=32)
    bad = {"Cin = 48": dict(Cin=48, out=p + 2 * 48),
           "Cout = 80": dict(Cout=80),
           "pitch 100": dict(x=odd.data_ptr(), xp=100, xs=H * W * 100, Cin=64, out=p),
           "out pitch 100": dict(out=odd.data_ptr(), op=100, os_=H * W * 100),
           "misaligned x": dict(x=p + 8, out=p + 2 * 96),
           "misaligned out": dict(out=p + 2 * 68),
           "out inside the channels read": dict(out=p + 2 * 32),
           "out across their end": dict(out=p + 2 * 48),
           "residual partly over out": dict(res=p + 2 * 80, rp=P, rs=S),
           "H = 0": dict(H=0),
           "null weight": dict(w=None)}
    for what, change in bad.items():
        assert _entry(**{**ok, **change}) == INVALID, what
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), before[0]) and torch.equal(_bits(odd), before[1])
    assert _entry(**ok) == 0          # the unbroken call is taken
    torch.cuda.synchronize()
    assert not torch.equal(_bits(buf), before[0])


def test_op_refuses_before_launch(cuda):
    buf = _buffer(1, 192, 8, 8, cuda, fill=1.0)
    w = torch.ones(32, 64, 3, 3, device=cuda, dtype=BF)
    before = _bits(buf)
    ops.reset_stats()
    with pytest.raises(ValueError):
        ops.conv2d_into(buf[:, :64], w, None, buf[:, 48:80], weight_nhwc=_wn(w, cuda))
    with pytest.raises(ValueError):
        ops.conv2d_into(buf[:, :64], w, None, buf[:, 64:96], weight_nhwc=_wn(w, cuda), residual=buf[:, 80:112])
    torch.cuda.synchronize()
    assert ops.stats() == {} and torch.equal(_bits(buf), before)


# ----------------------------------------------------------------------------------------------------------- models
def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-12)).item()


def _pin_old_path(monkeypatch, N, H, W, nf, gc):
    """The old path's activated convs on their fused kernel (v3), not on whatever the tuner times fastest here, so
    that its ("act_fused", "hip") count is a fixed number to compare with: one per activated conv."""
    keys = {"|".join(str(v) for v in ("conv", N, H, W, nf + i * gc, gc, 3, 1, 1, 0, 0, "act", "leaky_relu", 0.2)): "v3"
            for i in range(4)}
    monkeypatch.setenv("CGS_TUNE_OVERRIDE", json.dumps(keys))


def _esrgan_sd(nf, gc, nb, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g) * (0.5 / max(1, s[1] * 9 if len(s) == 4 else 1) ** 0.5)   # noqa: E731
    sd = {"conv_first.weight": r(nf, 3, 3, 3), "conv_first.bias": r(nf)}
    for blk in range(nb):
        for j in range(1, 4):
            for c in range(1, 6):
                sd[f"body.{blk}.rdb{j}.conv{c}.weight"] = r(nf if c == 5 else gc, nf + (c - 1) * gc, 3, 3)
                sd[f"body.{blk}.rdb{j}.conv{c}.bias"] = r(nf if c == 5 else gc)
    for n_ in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
        sd[f"{n_}.weight"], sd[f"{n_}.bias"] = r(nf, nf, 3, 3), r(nf)
    sd["conv_last.weight"], sd["conv_last.bias"] = r(3, nf, 3, 3), r(3)
    return sd


def _model_pair(kind, cuda):
    """(fp32 CPU model, the same weights in bf16 on the device, CPU input, dense blocks, dense convs per block)."""
    if kind == "rdb":
        make, x, blocks, per = (lambda: upscalers.ResidualDenseBlock5C(64, 32)), torch.randn(1, 64, 24, 24), 1, 5
    elif kind == "rrdb":
        make, x, blocks, per = (lambda: upscalers.RRDB(64, 32)), torch.randn(1, 64, 20, 36), 3, 5
    elif kind == "rrdb128":
        make, x, blocks, per = (lambda: upscalers.RRDB(128, 32)), torch.randn(1, 128, 16, 16), 3, 4
    else:
        sd = _esrgan_sd(64, 32, 2, seed=9)
        m = upscalers.load_state_dict(dict(sd)).eval()
        md = upscalers.load_state_dict(dict(sd)).eval().to(device=cuda, dtype=BF)
        return m, md, torch.rand(1, 3, 40, 24), 6, 5
    m = make()
    init_random_(m, seed=7)
    md = make()
    md.load_state_dict(m.state_dict())
    return m.eval(), md.eval().to(device=cuda, dtype=BF), x, blocks, per


@pytest.mark.parametrize("kind", ["rdb", "rrdb", "rrdb128", "rrdbnet"])
def test_models_dense_path(cuda, monkeypatch, kind):
    torch.manual_seed(11)
    with torch.no_grad():
        m, md, x, blocks, per = _model_pair(kind, cuda)
        want = m(x)
        xd = _nhwc(x.to(cuda, BF))
        nf = 128 if kind == "rrdb128" else 64
        _pin_old_path(monkeypatch, 1, x.shape[2], x.shape[3], nf, 32)
        monkeypatch.setenv("CGS_DENSE_CONV", "0")
        md(xd)        # the convs outside the dense blocks make their kernel choice here, timing runs included
        ops.reset_stats()
        old = md(xd).float().cpu()
        st_old = ops.stats()
        monkeypatch.setenv("CGS_DENSE_CONV", "1")
        ops.reset_stats()
        new = md(xd).float().cpu()
        st_new = ops.stats()
    print(f"DENSE {kind}: rel old {_rel(old, want):.3e} new {_rel(new, want):.3e}; old {st_old}; new {st_new}")
    assert _rel(old, want) < 3e-2 and _rel(new, want) < 3e-2
    assert st_old.get(("conv_dense", "hip"), 0) == 0
    assert st_new.get(("conv_dense", "hip"), 0) == per * blocks, st_new
    assert not any(k[1] == "lib" for k in st_new) and not any(k[1] == "lib" for k in st_old), (st_old, st_new)
    for key in (("conv", "hip"), ("act_fused", "hip")):
        assert st_new.get(key, 0) == st_old.get(key, 0), (key, st_old, st_new)


def test_rrdb_graph_capture(cuda, monkeypatch):
    """The dense RRDB captured once and replayed on new input contents equals the eager dense result bit for bit."""
    monkeypatch.setenv("CGS_DENSE_CONV", "1")
    with torch.inference_mode():
        m = upscalers.RRDB(64, 32)
        init_random_(m, seed=8)
        m = m.eval().to(device=cuda, dtype=BF)
        g0 = torch.Generator().manual_seed(3)
        x1 = _nhwc(torch.randn(1, 64, 20, 36, generator=g0).to(cuda, BF))
        x2 = _nhwc(torch.randn(1, 64, 20, 36, generator=g0).to(cuda, BF))
        xs = x1.clone()
        m(xs)                                        # builds the cached weight layouts outside the capture
        ops.reset_stats()
        eager = m(x2).clone()
        assert _dense_counts() == 15
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                y = m(xs)
        torch.cuda.current_stream().wait_stream(s)
        xs.copy_(x2)
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)
