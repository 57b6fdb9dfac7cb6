"""ops.attention(mask=...) on the generic flash kernel (cgs_flash_attn_fwd_mask): additive fp32 / bf16 / fp16 and bool
masks read through broadcast strides, against the per-element fp64 bound of _bounds_mask.py. Every device call must
count ("attention", "hip") once and no "lib": a masked call used to leave the hand-written kernels."""
import functools
import math

import pytest
import torch

from comfy_gen_server_amd import ops, _native
from comfy_gen_server_amd.ops import core

from _bounds import assert_within, rel
from _bounds_mask import masked_attention_bound

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B, H = 3, 3
DIMS = [40, 64, 160]
# a partial last tile, a partial last run of 4, unaligned rows, more than one Q block, a single key
SHAPES = [(1, 4), (63, 65), (129, 130), (257, 63), (130, 77), (64, 1)]
# name -> (mask shape for (B, H, Sq, Sk), dtype)
FORMS = {
    "SqSk-f32": (lambda b, h, sq, sk: (sq, sk), torch.float32),
    "BSqSk-bf16": (lambda b, h, sq, sk: (b, sq, sk), BF),
    "1HSqSk-bf16": (lambda b, h, sq, sk: (1, h, sq, sk), BF),
    "BHSqSk-f32": (lambda b, h, sq, sk: (b, h, sq, sk), torch.float32),
    "B1SqSk-bool": (lambda b, h, sq, sk: (b, 1, sq, sk), torch.bool),
    "B1SqSk-f16": (lambda b, h, sq, sk: (b, 1, sq, sk), torch.float16),
}


@pytest.fixture(autouse=True)
def _native_loaded(cuda, monkeypatch):
    assert _native.load_kernels() is not None, _native.kernels_error()
    monkeypatch.setenv("CGS_AUTOTUNE", "0")
    ops.reset_stats()
    yield


def _qkv(B, H, Sq, Sk, D, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, S, H * D, generator=g).to(BF) for S in (Sq, Sk, Sk))
    return q, k, v


def make_mask(shape, dtype, seed, keep_col0=False):
    """A CPU mask of ``shape`` [..., Sq, Sk]: a third of the entries blocked, a third 0, a third multiples of 0.25 in
    [-4, 4] (exact in bf16 and fp16); bool: a third blocked. Every query row keeps one key at 0 / True (column 0 with
    ``keep_col0``), which is checked here."""
    g = torch.Generator().manual_seed(seed)
    sk = shape[-1]
    kind = torch.randint(0, 3, shape, generator=g)
    vals = torch.randint(-16, 17, shape, generator=g).float() / 4
    m = torch.where(kind == 0, torch.full(shape, -math.inf), torch.where(kind == 1, torch.zeros(shape), vals))
    keep = torch.zeros(shape[:-1], dtype=torch.long) if keep_col0 else torch.randint(0, sk, shape[:-1], generator=g)
    m.scatter_(-1, keep.unsqueeze(-1), 0.0)
    assert bool(torch.isfinite(m).any(-1).all()), "a query row lost every key"
    assert float(m[torch.isfinite(m)].abs().max()) <= 4
    if dtype == torch.bool:
        return torch.isfinite(m)
    out = m.to(dtype)
    assert torch.equal(out.float(), m), "mask values must be exact in the mask's dtype"
    return out


def _attn(q, k, v, heads, **kw):
    ops.reset_stats()
    o = ops.attention(q, k, v, heads, **kw)
    st = ops.stats()
    assert st.get(("attention", "hip"), 0) == 1 and not any(key[1] == "lib" for key in st), st
    return o


@functools.lru_cache(maxsize=None)
def _case(D, form, Sq, Sk):
    """(q, k, v, mask, ref, tol) on the device, built once and shared by the plain and the strict run."""
    dev = torch.device("cuda", 0)
    shape_of, dtype = FORMS[form]
    q, k, v = (t.to(dev) for t in _qkv(B, H, Sq, Sk, D, seed=Sq * 1000 + Sk + D))
    mask = make_mask(shape_of(B, H, Sq, Sk), dtype, seed=Sq * 7 + Sk).to(dev)
    ref, tol = masked_attention_bound(q, k, v, H, mask)
    return q, k, v, mask, ref, tol


@pytest.mark.parametrize("strict", [False, True], ids=["plain", "strict-native"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("D", DIMS)
def test_masked_attention_bound(cuda, monkeypatch, D, form, strict):
    if strict:
        monkeypatch.setenv("CGS_STRICT_NATIVE", "1")      # a vendor fallback raises
    for Sq, Sk in SHAPES:
        q, k, v, mask, ref, tol = _case(D, form, Sq, Sk)
        o = _attn(q, k, v, H, mask=mask)
        assert_within(o, ref, tol, f"masked attention D={D} {form} Sq={Sq} Sk={Sk}")


@pytest.mark.parametrize("Sq,Sk", [(130, 128), (130, 77)])
def test_mask_broadcast_is_by_stride(cuda, Sq, Sk):
    D = 64
    q, k, v = (t.to(cuda) for t in _qkv(B, H, Sq, Sk, D, seed=5))
    m = make_mask((1, 1, Sq, Sk), BF, seed=6).to(cuda)
    keep = m.clone()
    o = _attn(q, k, v, H, mask=m)
    assert torch.equal(m, keep), "the op changed the caller's mask"
    full = m.expand(B, H, Sq, Sk).contiguous()
    assert torch.equal(_attn(q, k, v, H, mask=full), o)
    # a column slice of a wider tensor: row stride Sk + 24, base 8 elements into the row
    wide = torch.zeros(Sq, Sk + 24, device=cuda, dtype=BF)
    wide[:, 8:8 + Sk] = m[0, 0]
    view = wide[:, 8:8 + Sk]
    assert view.stride(0) != Sk and not view.is_contiguous()
    keep = wide.clone()
    assert torch.equal(_attn(q, k, v, H, mask=view), o)
    assert torch.equal(wide, keep)
    ref, tol = masked_attention_bound(q, k, v, H, m)
    assert_within(o, ref, tol, f"broadcast mask Sq={Sq} Sk={Sk}")


def test_mask_with_causal(cuda):
    S, D = 77, 64
    q, k, v = (t.to(cuda) for t in _qkv(B, H, S, S, D, seed=11))
    m = make_mask((B, 1, S, S), BF, seed=12, keep_col0=True).to(cuda)        # row 0 sees key 0 only
    o = _attn(q, k, v, H, mask=m, causal=True)
    ref, tol = masked_attention_bound(q, k, v, H, m, causal=True)
    assert_within(o, ref, tol, "mask + causal")


def test_mask_with_key_padding(cuda):
    Sq, Sk, D = 130, 77, 64
    q, k, v = (t.to(cuda) for t in _qkv(B, H, Sq, Sk, D, seed=13))
    m = make_mask((B, H, Sq, Sk), torch.float32, seed=14, keep_col0=True).to(cuda)
    lens = torch.tensor([77, 1, 40], device=cuda)                            # ragged; key 0 always kept
    kp = torch.arange(Sk, device=cuda)[None, :] < lens[:, None]
    o = _attn(q, k, v, H, mask=m, key_padding=kp)
    ref, tol = masked_attention_bound(q, k, v, H, m, key_padding=kp)
    assert_within(o, ref, tol, "mask + key padding")


def test_fully_blocked_row_is_zero(cuda):
    Sq, Sk, D = 130, 77, 64
    q, k, v = (t.to(cuda) for t in _qkv(B, H, Sq, Sk, D, seed=15))
    m = make_mask((B, 1, Sq, Sk), BF, seed=16).to(cuda)
    m[1, 0, 70] = -math.inf
    o = _attn(q, k, v, H, mask=m)
    assert bool(torch.isfinite(o).all())
    assert bool((o[1, 70] == 0).all()) and not bool((o[1, 69] == 0).all())
    ref, tol = masked_attention_bound(q, k, v, H, m)
    assert_within(o, ref, tol, "one fully blocked row")


def test_no_score_tensor(cuda):
    Bm, Hm, S, D = 2, 10, 1024, 64
    q, k, v = (t.to(cuda) for t in _qkv(Bm, Hm, S, S, D, seed=17))
    m = make_mask((1, 1, S, S), BF, seed=18).to(cuda)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    o = _attn(q, k, v, Hm, mask=m)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    scores = Bm * Hm * S * S * 4
    print(f"peak rise {rise / 1e6:.1f} MB, fp32 score tensor {scores / 1e6:.1f} MB")
    assert rise < scores / 4, (rise, scores)
    ref, tol = masked_attention_bound(q[:1], k[:1], v[:1], Hm, m)
    assert_within(o[:1], ref, tol, "level-2-like masked attention, batch entry 0")


def test_masked_attention_graph_capture(cuda):
    Sq, Sk, D = 130, 77, 64
    q, k, v = (t.to(cuda) for t in _qkv(B, H, Sq, Sk, D, seed=19))
    m = make_mask((B, 1, Sq, Sk), torch.bool, seed=20).to(cuda)
    eager = _attn(q, k, v, H, mask=m)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = ops.attention(q, k, v, H, mask=m)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_mask_launcher_domain(cuda):
    """Invalid arguments only: each call must return an error code before anything is launched."""
    lib = _native.load_kernels()
    Bq, Hq, S = 1, 1, 64

    def call(D, mask_ptr, kind=2, msq=S):
        q = torch.zeros(Bq, S, Hq * D, device=cuda, dtype=BF)
        o = torch.full_like(q, 7.0)
        err = lib.cgs_flash_attn_fwd_mask(*core._attn_operands(q, q, q, o, Hq), 1.0 / math.sqrt(D), mask_ptr, kind,
                                          0, 0, msq, None, 0, core._stream())
        torch.cuda.synchronize()
        assert bool((o == 7.0).all()), "the refused call wrote the output"
        return err

    m = torch.zeros(S, S, device=cuda, dtype=BF)
    assert call(512, m.data_ptr()) != 0
    assert call(36, m.data_ptr()) != 0
    assert call(64, None) != 0
    assert call(64, m.data_ptr(), kind=3) != 0
    assert call(64, m.data_ptr(), msq=S + 2) != 0          # rows not a multiple of 4 elements apart


def _rel_cpu(y, ref):
    return rel(y.float().cpu(), ref)


def _cross_attention_pair(cuda):
    from comfy_gen_server_amd.models.attention import CrossAttention
    from comfy_gen_server_amd.models.layers import init_random_
    cpu = CrossAttention(320, 768, heads=5, dim_head=64)
    init_random_(cpu, seed=21)
    dev = CrossAttention(320, 768, heads=5, dim_head=64, dtype=BF, device=cuda)
    dev.load_state_dict(cpu.state_dict())
    cpu.load_state_dict({n: t.to(BF).float() for n, t in cpu.state_dict().items()})   # the bf16 weights, in fp32
    g = torch.Generator().manual_seed(22)
    x = torch.randn(2, 130, 320, generator=g).to(BF)
    ctx = torch.randn(2, 77, 768, generator=g).to(BF)
    mask = make_mask((2, 1, 130, 77), torch.bool, seed=23)
    return cpu, dev, x, ctx, mask


def test_cross_attention_module_with_mask(cuda):
    cpu, dev, x, ctx, mask = _cross_attention_pair(cuda)
    with torch.no_grad():
        ref = cpu(x.float(), context=ctx.float(), mask=mask)
        ops.reset_stats()
        y = dev(x.to(cuda), context=ctx.to(cuda), mask=mask.to(cuda))
    st = ops.stats()
    assert st.get(("attention", "hip"), 0) == 1 and not any(key[1] == "lib" for key in st), st
    assert _rel_cpu(y, ref) < 2e-2


@pytest.mark.parametrize("skip_reshape", [False, True])
def test_compat_attention_with_mask(cuda, skip_reshape):
    from comfy_gen_server_amd.compat_names import _ref_attention
    cpu, dev, x, ctx, mask = _cross_attention_pair(cuda)
    heads, D = 5, 64
    with torch.no_grad():
        qc, (kc, vc) = cpu.to_q(x.float()), cpu.project_kv(ctx.float())
        ref = core.attention_reference(qc, kc, vc, heads, mask=mask)
        q, k, v = (t.to(BF).to(cuda) for t in (qc, kc, vc))
        if skip_reshape:
            q, k, v = (t.reshape(2, t.shape[1], heads, D).transpose(1, 2) for t in (q, k, v))
        ops.reset_stats()
        o = _ref_attention(q, k, v, heads, mask=mask.to(cuda), skip_reshape=skip_reshape)
    st = ops.stats()
    assert st.get(("attention", "hip"), 0) == 1 and not any(key[1] == "lib" for key in st), st
    assert tuple(o.shape) == (2, 130, heads * D)
    assert _rel_cpu(o, ref) < 2e-2
