"""The kernels of the sampler loop against per-element worst-case bounds (tests/_bounds.py, "The kernels of the
sampling loop"): cgs_cfg_combine, cgs_euler_step, cgs_silu, cgs_timestep_embedding, cgs_upsample_nearest2x_nhwc
(elementwise.hip) and cgs_philox_randn, cgs_euler_ancestral_philox, cgs_brownian_increment, cgs_sampler_step_dev,
cgs_step_param, cgs_step_advance (rng.hip). The sizes are the smallest that reach each path: scalar tails, more than
one block, the second trip of a grid-stride loop past the block cap, image bases that are no multiple of 4. Every
test reads ops.stats() to prove which path ran; the guard cases prove that the torch path ran and gave the result."""
import math

import pytest
import torch
import torch.nn.functional as F

from _bounds import (EW_CAP_N, EW_SIZES, RNG_CAP_SHAPE, RNG_INDEX0, RNG_SEEDS, RNG_SHAPES, RNG_STREAMS, SEED63, SILU_CAP_N,
                     SILU_SIZES, TEMB_SHAPES, TEMB_T, _f32, assert_within, cfg_combine_bound, euler_step_bound, ew_inputs,
                     normal_bound, sampler_step_bound, silu_bound, silu_inputs, timestep_embedding_bound)
from comfy_gen_server_amd import _native, ops
from comfy_gen_server_amd.sampling import rng

pytestmark = pytest.mark.gpu

SIG = tuple(_f32(v) for v in (2.5, 1.7, 0.9))            # sigma, sigma_down, sigma_up as fp32 values


@pytest.fixture(autouse=True)
def _native_loaded(cuda):
    assert _native.load_kernels() is not None, _native.kernels_error()
    ops.reset_stats()
    yield


def _ran(op, backend="hip"):
    return ops.stats().get((op, backend), 0)


def _numel1(shape):
    n = 1
    for d in shape[1:]:
        n *= d
    return n


# ------------------------------------------------------------------------------------------------ elementwise.hip
@pytest.mark.parametrize("n", EW_SIZES + [EW_CAP_N])
def test_cfg_combine_bound(cuda, n):
    _, c, u, _ = ew_inputs(n, device=cuda)
    c0, u0 = c.clone(), u.clone()
    for s in (1.0, 7.5, 0.0, -2.0):
        y = ops.cfg_combine(c, u, s)
        assert_within(y, *cfg_combine_bound(c0, u0, s), f"cfg_combine n={n} s={s}")
    assert _ran("cfg") == 4, ops.stats()
    assert torch.equal(c, c0) and torch.equal(u, u0)


@pytest.mark.parametrize("n", EW_SIZES + [EW_CAP_N])
def test_euler_step_bound(cuda, n):
    x, den, _, z = ew_inputs(n, device=cuda)
    x0, den0, z0 = x.clone(), den.clone(), z.clone()
    s, sd, su = SIG
    assert_within(ops.euler_step(x, den, z, s, sd, su), *euler_step_bound(x0, den0, z0, s, sd, su), f"euler_step n={n}")
    plain = ops.euler_step(x, den, None, s, sd, 0.0)
    assert_within(plain, *euler_step_bound(x0, den0, None, s, sd, 0.0), f"euler_step n={n} no noise")
    assert torch.equal(ops.euler_step(x, den, z, s, sd, 0.0), plain)          # sigma_up = 0: the noise is ignored
    assert _ran("euler") == 3, ops.stats()
    assert torch.equal(x, x0) and torch.equal(den, den0) and torch.equal(z, z0)      # the wrapper works on a clone


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n", SILU_SIZES + [SILU_CAP_N])
def test_silu_bound(cuda, n, dtype):
    x = silu_inputs(n, dtype, device=cuda)
    x0 = x.clone()
    y = ops.silu(x)
    assert _ran("silu") == 1, ops.stats()
    assert y.dtype == dtype and y.shape == x.shape
    assert_within(y, *silu_bound(x0), f"silu n={n} {dtype}")
    assert torch.equal(x.view(torch.int16), x0.view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(1, 8, 1, 1), (2, 24, 3, 5), (1, 64, 8, 8)])
def test_upsample_nearest2x_bit_exact(cuda, shape, dtype):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(dtype)
    y = ops.upsample_nearest2x(x.to(cuda))
    assert _ran("upsample") == 1, ops.stats()
    ref = F.interpolate(x.float(), scale_factor=2.0, mode="nearest").to(dtype)          # moves values: exact
    assert y.shape == ref.shape and y.dtype == dtype
    assert torch.equal(y.cpu().view(torch.int16), ref.view(torch.int16))


def _temb_t(n, o):
    return torch.tensor([TEMB_T[(i + o) % len(TEMB_T)] for i in range(n)], dtype=torch.float32)


@pytest.mark.parametrize("n,dim", TEMB_SHAPES)
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("period", [10000.0, 100.0])
def test_timestep_embedding_bound(cuda, n, dim, flip, period):
    for o in range(len(TEMB_T)):
        t = _temb_t(n, o)
        y = ops.timestep_embedding(t.to(cuda), dim, period, flip)
        assert y.shape == (n, dim) and y.dtype == torch.float32
        assert_within(y.cpu(), *timestep_embedding_bound(t, dim, period, flip),
                      f"timestep_embedding n={n} dim={dim} flip={flip} P={period} o={o}")
    assert _ran("timestep_embedding") == len(TEMB_T), ops.stats()


def test_timestep_embedding_fallbacks(cuda):
    """Odd dim and an empty t take the torch path: a zero last column, an empty [0, dim] result."""
    t = _temb_t(5, 0)
    y = ops.timestep_embedding(t.to(cuda), 321)
    assert y.shape == (5, 321) and bool((y[:, 320] == 0).all())
    assert_within(y[:, :320].cpu(), *timestep_embedding_bound(t, 320), "timestep_embedding dim=321 (torch)")
    for dim in (320, 321):
        e = ops.timestep_embedding(torch.empty(0, device=cuda), dim)
        assert e.shape == (0, dim) and e.dtype == torch.float32 and e.device.type == "cuda"
    torch.cuda.synchronize()
    assert _ran("timestep_embedding") == 0, ops.stats()


# ------------------------------------------------------------------------------------------------ cgs_philox_randn
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("seed", RNG_SEEDS)
def test_philox_randn_bound(cuda, seed, dtype):
    worst, calls = 0.0, 0
    for shape in RNG_SHAPES:
        n = _numel1(shape)
        for i0 in RNG_INDEX0:
            for stream in RNG_STREAMS:
                inds = list(range(i0, i0 + shape[0]))
                z = ops.philox_randn(shape, seed, inds, stream, device=cuda, dtype=dtype)
                calls += 1
                assert z.shape == shape and z.dtype == dtype
                ref, tol = normal_bound(seed, inds, n, stream, dtype)
                worst = max(worst, assert_within(z.reshape(shape[0], n).cpu(), ref, tol,
                                                 f"philox_randn {shape} seed={seed} i0={i0} stream={stream} {dtype}"))
    print(f"BOUND philox_randn seed={seed} {dtype}: worst of {calls} cases {worst:.3f}")
    assert _ran("rng") == calls and _ran("rng", "torch") == 0, ops.stats()


def test_philox_randn_block_cap(cuda):
    """17 images of 2^20 values: more groups than 16384 blocks of 256 threads hold, so the grid-stride loop works
    out the image index again on its second trip."""
    B, n = RNG_CAP_SHAPE
    i0, stream = (1 << 31) - 1, (1 << 32) + 7
    z = ops.philox_randn(RNG_CAP_SHAPE, SEED63, range(i0, i0 + B), stream, device=cuda)
    assert _ran("rng") == 1, ops.stats()
    ref, tol = normal_bound(SEED63, range(i0, i0 + B), n, stream)
    assert_within(z.cpu(), ref, tol, f"philox_randn {RNG_CAP_SHAPE}")


def test_philox_randn_key_scope_reads_the_device_key(cuda):
    """Under rng_key_scope the kernel takes (seed, index0) from the key tensor: the tensor of a seed with bit 63 set,
    built with seed_i64, gives that seed's noise, and rewriting the tensor serves another job without a new scope."""
    shape, stream = (2, 1027), 3
    key = torch.tensor([rng.seed_i64(SEED63), 6], dtype=torch.int64, device=cuda)
    with ops.rng_key_scope(key, SEED63, 6):
        z = ops.philox_randn(shape, SEED63, [6, 7], stream, device=cuda)
        assert_within(z.cpu(), *normal_bound(SEED63, [6, 7], 1027, stream), "philox_randn device key")
        key.copy_(torch.tensor([rng.seed_i64((1 << 64) - 1), 1 << 40], dtype=torch.int64))
        z2 = ops.philox_randn(shape, SEED63, [6, 7], stream, device=cuda)
        assert_within(z2.cpu(), *normal_bound((1 << 64) - 1, [1 << 40, (1 << 40) + 1], 1027, stream),
                      "philox_randn rewritten device key")
        other = ops.philox_randn(shape, 5, [6, 7], stream, device=cuda)          # another (seed, index0): not the key
        assert_within(other.cpu(), *normal_bound(5, [6, 7], 1027, stream), "philox_randn beside the scope")
    assert torch.equal(z, ops.philox_randn(shape, SEED63, [6, 7], stream, device=cuda))
    assert _ran("rng") == 4, ops.stats()


def test_philox_randn_dev_step_batch_and_scatter(cuda):
    shape, stream = (3, 4, 8, 8), (1 << 32) + 7
    step = torch.tensor([3], dtype=torch.int64, device=cuda)
    z = ops.philox_randn(shape, SEED63, [3, 4, 5], stream, device=cuda, dev_step=step)
    assert torch.equal(z, ops.philox_randn(shape, SEED63, [3, 4, 5], stream + 3, device=cuda))
    assert_within(z.reshape(3, 256).cpu(), *normal_bound(SEED63, [3, 4, 5], 256, stream + 3), "philox_randn dev_step")
    # an image's values do not depend on the batch it is drawn in
    one = ops.philox_randn((1,) + shape[1:], SEED63, [4], stream + 3, device=cuda)
    assert torch.equal(z[1:2], one)
    assert _ran("rng") == 3, ops.stats()
    # scattered indices: one launch an image
    sc = ops.philox_randn((2, 1027), SEED63, [9, 2], stream, device=cuda)
    assert _ran("rng") == 5, ops.stats()
    assert_within(sc.cpu(), *normal_bound(SEED63, [9, 2], 1027, stream), "philox_randn scattered")


# ------------------------------------------------------------------------------------------------ euler_ancestral_philox
def _row(s, sd, su, s_noise=1.0):
    return torch.tensor([s, sd, su, s_noise], dtype=torch.float32)


def test_euler_ancestral_philox_bound_and_bits(cuda):
    shape, inds, stream = (3, 4, 8, 8), [4, 5, 6], 11
    x, den, _, _ = (v.reshape(shape) for v in ew_inputs(768, seed=2, device=cuda))
    x0, den0 = x.clone(), den.clone()
    s, sd, su = SIG
    fused = ops.euler_ancestral_philox(x, den, s, sd, su, SEED63, inds, stream)
    assert _ran("euler") == 1 and _ran("rng") == 0, ops.stats()
    (ref, tol), _ = sampler_step_bound(x0, den0, None, 1.0, _row(s, sd, su), SEED63, 4, stream)
    assert_within(fused, ref, tol, "euler_ancestral_philox")
    assert torch.equal(x, x0) and torch.equal(den, den0)
    # the kernel's claim: the same bits as the two-kernel form
    noise = ops.philox_randn(shape, SEED63, inds, stream, device=cuda)
    assert torch.equal(fused, ops.euler_step(x, den, noise, s, sd, su))
    # sigma_up = 0: the plain Euler step, bit for bit
    assert torch.equal(ops.euler_ancestral_philox(x, den, s, sd, 0.0, SEED63, inds, stream),
                       ops.euler_step(x, den, None, s, sd, 0.0))


def test_euler_ancestral_philox_unfused_tail(cuda):
    """n % 4 != 0: cgs_philox_randn and cgs_euler_step in place of the fused kernel, inside the same bound."""
    shape = (2, 5)
    x, den, _, _ = (v.reshape(shape) for v in ew_inputs(10, seed=2, device=cuda))
    s, sd, su = SIG
    y = ops.euler_ancestral_philox(x, den, s, sd, su, SEED63, [4, 5], 11)
    assert _ran("euler") == 1 and _ran("rng") == 1, ops.stats()
    (ref, tol), _ = sampler_step_bound(x, den, None, 1.0, _row(s, sd, su), SEED63, 4, 11)
    assert_within(y, ref, tol, "euler_ancestral_philox (2, 5)")


# ------------------------------------------------------------------------------------------------ brownian_increment
def _inc(cuda, shape, inds, ta, tb, t0=0.0, t1=4.0, tol=1e-4, seed=SEED63, scale=1.0):
    return ops.brownian_increment(shape, seed, inds, t0, t1, ta, tb, tol, 24, scale, device=cuda)


def _inc_mirror(shape, inds, ta, tb, t0=0.0, t1=4.0, tol=1e-4, seed=SEED63, scale=1.0):
    return rng.brownian_reference(shape, seed, inds, t0, t1, ta, tb, tol, 24, scale)


def test_brownian_increment_edges(cuda):
    shape, inds = (2, 4, 8, 8), [3, 4]
    z = _inc(cuda, shape, inds, 2.5, 2.5)
    assert bool((z == 0).all())                                            # ta == tb: the same walk twice
    for ta, tb in ((0.0, 4.0), (-1.0, 4.0)):                               # ta <= t0 < tb == t1
        w = _inc(cuda, shape, inds, ta, tb, scale=0.75)
        ref = _inc_mirror(shape, inds, ta, tb, scale=0.75)
        assert torch.allclose(w.cpu(), ref, atol=5e-5, rtol=1e-4), (w.cpu() - ref).abs().max()
    assert torch.equal(_inc(cuda, shape, inds, -1.0, 4.0), _inc(cuda, shape, inds, 0.0, 4.0))
    assert _ran("rng") == 5 and _ran("rng", "torch") == 0, ops.stats()


def test_brownian_increment_without_descent(cuda):
    """tol above t1 - t0: no midpoint is drawn, W is the straight line from 0 to W(t1)."""
    shape, inds = (2, 4, 8, 8), [3, 4]
    w = _inc(cuda, shape, inds, 1.0, 3.0, tol=5.0)
    ref = _inc_mirror(shape, inds, 1.0, 3.0, tol=5.0)
    assert torch.allclose(w.cpu(), ref, atol=5e-5, rtol=1e-4), (w.cpu() - ref).abs().max()
    # W(t1) itself is the node-0 normal times sqrt(t1 - t0); the increment over half the span is half of it
    full = _inc(cuda, shape, inds, 0.0, 4.0, tol=5.0)
    zr, zt = normal_bound(SEED63, inds, 256, rng.tree_stream(0, 0))
    assert_within(full.reshape(2, 256).cpu(), 2.0 * zr, 2.0 * zt, "brownian W(t1)")      # times 2 and times 1: exact
    assert torch.allclose(w, 0.5 * full, atol=1e-6, rtol=1e-6)
    assert _ran("rng") == 2, ops.stats()


def test_brownian_increment_batch_independence_and_tail(cuda):
    shape = (3, 4, 8, 8)
    w = _inc(cuda, shape, [3, 4, 5], 0.7, 3.1)
    assert torch.equal(w[1:2], _inc(cuda, (1,) + shape[1:], [4], 0.7, 3.1))
    assert _ran("rng") == 2 and _ran("rng", "torch") == 0, ops.stats()
    # n % 4 != 0: no kernel for it, the mirror's values on the device
    t = _inc(cuda, (2, 5), [3, 4], 0.7, 3.1)
    assert _ran("rng") == 2 and _ran("rng", "torch") == 1, ops.stats()
    assert t.device.type == "cuda" and torch.equal(t.cpu(), _inc_mirror((2, 5), [3, 4], 0.7, 3.1))


# ------------------------------------------------------------------------------------------------ sampler_step_dev
def _step_table(cols, device):
    """8 rows of (sigma, sigma_down, sigma_up, s_noise): row 0 with s_noise = 0.5, row 5 with sigma_up = 0, distinct
    values everywhere else; the columns past the fourth hold a sentinel that no row may read."""
    sig = [14.6, 11.2, 8.3, 6.1, 4.4, 3.0, 1.9, 0.9]
    rows = []
    for j, s in enumerate(sig):
        down = 0.62 * s + 0.01 * j
        up = 0.0 if j == 5 else 0.55 * s
        rows.append([s, down, up, 0.5 if j == 0 else 1.0] + [777.0] * (cols - 4))
    return torch.tensor(rows, dtype=torch.float32, device=device)


@pytest.mark.parametrize("cols", [4, 6])
@pytest.mark.parametrize("with_den_out", [False, True])
@pytest.mark.parametrize("with_u", [False, True])
@pytest.mark.parametrize("shape", [(1, 4), (3, 4, 8, 8), (2, 1028)])
def test_sampler_step_dev_bound(cuda, shape, with_u, with_den_out, cols):
    n = math.prod(shape)
    xs, c, u, _ = (v.reshape(shape) for v in ew_inputs(n, seed=4, device=cuda))
    u = u if with_u else None
    params = _step_table(cols, cuda)
    c0, u0, p0 = c.clone(), None if u is None else u.clone(), params.clone()
    calls = 0
    for step in (0, 2, 5):
        for seed in (9, SEED63):
            for cfg in (1.0, 6.0):
                meta = torch.tensor([step, rng.seed_i64(seed), 7], dtype=torch.int64, device=cuda)
                m0 = meta.clone()
                x = xs.clone()
                den_out = torch.full_like(x, -7.0) if with_den_out else None
                assert ops.sampler_step_dev(x, c, u, den_out, cfg, params, meta) is x
                calls += 1
                what = f"sampler_step_dev {shape} u={with_u} cols={cols} step={step} seed={seed} cfg={cfg}"
                (ref, tol), (dref, dtol) = sampler_step_bound(xs, c0, u0, cfg, p0[step], seed, 7, step)
                assert_within(x, ref, tol, what)
                if with_den_out:
                    assert_within(den_out, dref, dtol, what + " den_out")
                assert torch.equal(meta, m0)
    assert torch.equal(c, c0) and torch.equal(params, p0) and (u is None or torch.equal(u, u0))
    assert _ran("euler") == calls, ops.stats()


@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_step_param_writes_its_slice_only(cuda, B):
    params = _step_table(6, cuda)
    for col in (0, 3):
        for step in (0, 5):
            meta = torch.tensor([step, rng.seed_i64(SEED63), 7], dtype=torch.int64, device=cuda)
            buf = torch.full((B + 16,), -7.0, device=cuda)
            out = buf[8:8 + B]
            assert ops.step_param(out, params, meta, col) is out
            assert bool((out == params[step, col]).all()), (B, col, step)
            assert bool((buf[:8] == -7.0).all()) and bool((buf[8 + B:] == -7.0).all()), (B, col, step)
            assert meta.tolist() == [step, rng.seed_i64(SEED63), 7]


def test_step_advance(cuda):
    meta = torch.tensor([0, rng.seed_i64(SEED63), 7], dtype=torch.int64, device=cuda)
    for _ in range(3):
        ops.step_advance(meta)
    assert meta.tolist() == [3, rng.seed_i64(SEED63), 7] and meta[1].item() < 0


def test_step_chain_in_one_graph(cuda):
    """step_param -> sampler_step_dev -> step_advance captured once as one linear chain and replayed three times
    from meta[0] = 0: every replay is one reference step of the x the replay before it left."""
    shape, cfg, seed = (3, 4, 8, 8), 6.0, SEED63
    x0, c, u, _ = (v.reshape(shape) for v in ew_inputs(768, seed=6, device=cuda))
    params = _step_table(6, cuda)
    x, den = x0.clone(), torch.zeros_like(x0)
    sig = torch.zeros(shape[0], device=cuda)
    meta = torch.tensor([0, rng.seed_i64(seed), 7], dtype=torch.int64, device=cuda)

    def body():
        ops.step_param(sig, params, meta, 0)
        ops.sampler_step_dev(x, c, u, den, cfg, params, meta)
        ops.step_advance(meta)

    # capture and replay under inference_mode, as the samplers do: the suite's earlier captures leave the
    # generator's graph state as inference tensors, which a capture outside that mode may not update
    with torch.inference_mode():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            body()                                       # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            body()
        torch.cuda.synchronize()
        x.copy_(x0)
        meta[0] = 0
        for step in range(3):
            prev = x.clone()
            g.replay()
            torch.cuda.synchronize()
            (ref, tol), (dref, dtol) = sampler_step_bound(prev, c, u, cfg, params[step], seed, 7, step)
            assert_within(x, ref, tol, f"graph replay {step}")
            assert_within(den, dref, dtol, f"graph replay {step} den")
            assert bool((sig == params[step, 0]).all())
            assert meta.tolist() == [step + 1, rng.seed_i64(seed), 7]
        assert meta[0].item() == 3


# ------------------------------------------------------------------------------------------------ wrapper guards
def test_euler_step_noise_guards(cuda):
    """A noise tensor the flat fp32 kernel cannot index goes to the torch path and gives the same update."""
    shape = (3, 4, 8, 8)
    x, den, _, z = (v.reshape(shape) for v in ew_inputs(768, seed=5, device=cuda))
    s, sd = SIG[:2]
    su = 0.5                                         # a power of two: the bf16 product noise sigma_up is exact
    zb = z.to(torch.bfloat16)
    y = ops.euler_step(x, den, zb, s, sd, su)
    assert y.dtype == torch.float32
    assert_within(y, *euler_step_bound(x, den, zb, s, sd, su), "euler_step bf16 noise (torch)")
    z1 = z[:1].contiguous()                          # broadcastable [1, ...]: a third of the elements
    y = ops.euler_step(x, den, z1, s, sd, su)
    assert_within(y, *euler_step_bound(x, den, z1.expand(shape), s, sd, su), "euler_step [1, ...] noise (torch)")
    assert _ran("euler") == 0, ops.stats()
    ops.euler_step(x, den, zb, s, sd, 0.0)           # sigma_up = 0: the noise is never read, the kernel serves it
    assert _ran("euler") == 1, ops.stats()


def test_cfg_combine_uncond_guards(cuda):
    shape = (3, 4, 8, 8)
    _, c, u, _ = (v.reshape(shape) for v in ew_inputs(768, seed=5, device=cuda))
    ub = u.to(torch.bfloat16)
    y = ops.cfg_combine(c, ub, 7.5)
    assert y.dtype == torch.float32
    assert_within(y, *cfg_combine_bound(c, ub, 7.5), "cfg_combine bf16 uncond (torch)")
    u1 = u[:1].contiguous()
    y = ops.cfg_combine(c, u1, 7.5)
    assert_within(y, *cfg_combine_bound(c, u1.expand(shape), 7.5), "cfg_combine [1, ...] uncond (torch)")
    assert _ran("cfg") == 0, ops.stats()


def test_upsample_nearest2x_four_channels(cuda):
    x = torch.randn(1, 4, 3, 3, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    y = ops.upsample_nearest2x(x.to(cuda))
    assert _ran("upsample") == 0, ops.stats()
    ref = F.interpolate(x.float(), scale_factor=2.0, mode="nearest").to(torch.bfloat16)
    assert y.shape == ref.shape and torch.equal(y.cpu().view(torch.int16), ref.view(torch.int16))


def test_silu_misaligned_view(cuda):
    """buf[1:] of a 16-bit buffer is contiguous and 2 bytes off a 16-byte boundary."""
    buf = silu_inputs(2056, torch.bfloat16, device=cuda)
    x = buf[1:]
    assert x.is_contiguous() and x.data_ptr() % 16 != 0
    y = ops.silu(x)
    assert _ran("silu") == 0, ops.stats()
    assert_within(y, *silu_bound(x), "silu buf[1:] (torch)")
    assert _ran("silu") == 0 and ops.silu(buf).shape == buf.shape and _ran("silu") == 1
