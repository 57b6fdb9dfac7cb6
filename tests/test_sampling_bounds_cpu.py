"""Self-test of the sampling-loop bounds of tests/_bounds.py on the CPU: the fp32 torch path of every op (for the noise
the CPU mirror, for the device-parameterised step a plain fp32 emulation of the kernel's lines) lies inside its bound
in every element, and four results that are wrong in a plausible way are rejected: the noise of the neighbouring
image, the noise of the next step, a sigma_up that was not scaled by s_noise, and a swapped sin and cos."""
import pytest
import torch
import torch.nn.functional as F

from _bounds import (EW_CAP_N, EW_SIZES, RNG_INDEX0, RNG_SEEDS, RNG_SHAPES, RNG_STREAMS, SEED63, SILU_CAP_N, SILU_SIZES,
                     TEMB_SHAPES, TEMB_T, _f32, assert_within, cfg_combine_bound, euler_step_bound, ew_inputs,
                     normal_bound, sampler_step_bound, silu_bound, silu_inputs, timestep_embedding_bound)
from comfy_gen_server_amd import ops
from comfy_gen_server_amd.sampling import rng

SIG = tuple(_f32(v) for v in (2.5, 1.7, 0.9))            # sigma, sigma_down, sigma_up as fp32 values


def _rejected(y, ref, tol, what):
    with pytest.raises(AssertionError, match="over tol"):
        assert_within(y, ref, tol, what)


@pytest.mark.parametrize("n", EW_SIZES + [EW_CAP_N])
def test_cfg_combine_torch_within_bound(n):
    x, c, u, z = ew_inputs(n)
    for s in (1.0, 7.5, 0.0, -2.0):
        assert_within(ops.cfg_combine(c, u, s), *cfg_combine_bound(c, u, s), f"cfg torch n={n} s={s}")


@pytest.mark.parametrize("n", EW_SIZES + [EW_CAP_N])
def test_euler_step_torch_within_bound(n):
    x, den, u, z = ew_inputs(n)
    s, sd, su = SIG
    assert_within(ops.euler_step(x, den, z, s, sd, su), *euler_step_bound(x, den, z, s, sd, su), f"euler torch n={n}")
    assert_within(ops.euler_step(x, den, None, s, sd, 0.0), *euler_step_bound(x, den, None, s, sd, 0.0),
                  f"euler torch n={n} no noise")
    ref, tol = euler_step_bound(x, den, z, s, sd, 0.0)
    assert torch.equal(ref, euler_step_bound(x, den, None, s, sd, 0.0)[0])       # sigma_up = 0: the noise is ignored
    assert_within(ops.euler_step(x, den, z, s, sd, 0.0), ref, tol, f"euler torch n={n} sigma_up=0")


def test_euler_step_bound_rejects_a_missing_rounding_budget():
    """The bound is a few ulps wide: the update with sigma in place of sigma_down (one step's dt off) is far outside."""
    x, den, u, z = ew_inputs(4099)
    s, sd, su = SIG
    ref, tol = euler_step_bound(x, den, z, s, sd, su)
    _rejected(ops.euler_step(x, den, z, s, _f32(1.7001), su), ref, tol, "euler dt off by 1e-4")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n", SILU_SIZES + [SILU_CAP_N])
def test_silu_torch_within_bound(n, dtype):
    x = silu_inputs(n, dtype)
    ref, tol = silu_bound(x)
    assert_within(ops.silu(x), ref, tol, f"silu torch n={n} {dtype}")
    if n >= 9:
        _rejected(F.silu(x.float() * 0.99).to(dtype), ref, tol, "silu of 0.99 x")


def _temb_t(n, o):
    return torch.tensor([TEMB_T[(i + o) % len(TEMB_T)] for i in range(n)], dtype=torch.float32)


@pytest.mark.parametrize("n,dim", TEMB_SHAPES)
@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("period", [10000.0, 100.0])
def test_timestep_embedding_torch_within_bound(n, dim, flip, period):
    for o in range(len(TEMB_T)):
        t = _temb_t(n, o)
        y = ops.timestep_embedding(t, dim, period, flip)
        ref, tol = timestep_embedding_bound(t, dim, period, flip)
        assert_within(y, ref, tol, f"temb torch n={n} dim={dim} flip={flip} P={period} o={o}")
        assert bool((tol[t == 0] == 0).all())                  # t = 0: exact
        if bool((t != 0).any()):                               # sin and cos swapped
            _rejected(ops.timestep_embedding(t, dim, period, not flip), ref, tol, "temb swapped")


@pytest.mark.parametrize("seed", RNG_SEEDS)
def test_mirror_within_normal_bound(seed):
    worst = 0.0
    for shape in RNG_SHAPES:
        n = 1
        for d in shape[1:]:
            n *= d
        for i0 in RNG_INDEX0:
            for stream in RNG_STREAMS:
                inds = list(range(i0, i0 + shape[0]))
                z = rng.randn_reference(shape, seed, inds, stream).reshape(shape[0], n)
                ref, tol = normal_bound(seed, inds, n, stream)
                worst = max(worst, assert_within(z, ref, tol, f"mirror {shape} seed={seed} i0={i0} stream={stream}"))
                zb = z.to(torch.bfloat16)
                assert_within(zb, *normal_bound(seed, inds, n, stream, torch.bfloat16), "mirror bf16")
    assert worst > 0                                           # the bound is not met by copying the reference


def test_normal_bound_rejects_the_neighbouring_image_and_stream():
    shape, seed, stream = (3, 4, 8, 8), SEED63, 7
    ref, tol = normal_bound(seed, [3, 4, 5], 256, stream)
    good = rng.randn_reference(shape, seed, [3, 4, 5], stream).reshape(3, 256)
    assert_within(good, ref, tol, "mirror")
    _rejected(rng.randn_reference(shape, seed, [4, 5, 6], stream).reshape(3, 256), ref, tol, "image b + 1")
    _rejected(rng.randn_reference(shape, seed, [3, 4, 5], stream + 1).reshape(3, 256), ref, tol, "stream + 1")
    _rejected(rng.randn_reference(shape, seed - (1 << 63), [3, 4, 5], stream).reshape(3, 256), ref, tol,
              "seed without bit 63")
    # one element of 768 from the neighbouring image
    bad = good.clone()
    bad[1, 77] = rng.randn_reference((1,) + shape[1:], seed, [5], stream).reshape(-1)[77]
    _rejected(bad, ref, tol, "one foreign element")


def _emulate_step(x, c, u, cfg, row, seed, index0, step, scale_noise=True, stream=None):
    """The lines of sampler_step_dev_kernel in fp32 torch ops, the noise from the CPU mirror."""
    cfg = torch.tensor(cfg, dtype=torch.float32)
    den = c if u is None else u + (c - u) * cfg
    sigma, sdown = row[0], row[1]
    sup = row[2] * row[3] if scale_noise else row[2]
    x = x + (x - den) * (1.0 / sigma) * (sdown - sigma)
    if float(sup) > 0:
        inds = range(index0, index0 + x.shape[0])
        x = x + rng.randn_reference(tuple(x.shape), seed, inds, step if stream is None else stream) * sup
    return x, den


STEP_ROWS = torch.tensor([[14.6, 9.1, 7.3, 1.0, 0, 0], [9.1, 5.2, 4.4, 0.5, 0, 0], [5.2, 2.0, 0.0, 1.0, 0, 0],
                          [2.0, 0.0, 0.0, 1.0, 0, 0]], dtype=torch.float32)


@pytest.mark.parametrize("shape", [(1, 4), (3, 4, 8, 8), (2, 1028)])
@pytest.mark.parametrize("with_u", [False, True])
def test_sampler_step_emulation_within_bound(shape, with_u):
    n = 1
    for d in shape:
        n *= d
    x, c, u, _ = (v.reshape(shape) for v in ew_inputs(n, seed=3))
    u = u if with_u else None
    for step, row in enumerate(STEP_ROWS):
        for seed in (9, SEED63):
            got, den = _emulate_step(x, c, u, 6.0, row, seed, 5, step)
            (ref, tol), (dref, dtol) = sampler_step_bound(x, c, u, 6.0, row, seed, 5, step)
            assert_within(got, ref, tol, f"step emulation {shape} u={with_u} step={step} seed={seed}")
            assert_within(den, dref, dtol, f"step emulation den {shape} u={with_u} step={step}")
            if not with_u:
                assert bool((dtol == 0).all())


def test_sampler_step_bound_rejects_wrong_noise():
    shape = (3, 4, 8, 8)
    x, c, u, _ = (v.reshape(shape) for v in ew_inputs(768, seed=3))
    row, step = STEP_ROWS[1], 1                                # sigma_up 4.4, s_noise 0.5
    (ref, tol), _ = sampler_step_bound(x, c, u, 6.0, row, SEED63, 5, step)
    assert_within(_emulate_step(x, c, u, 6.0, row, SEED63, 5, step)[0], ref, tol, "step emulation")
    _rejected(_emulate_step(x, c, u, 6.0, row, SEED63, 5, step, stream=step + 1)[0], ref, tol, "stream step + 1")
    _rejected(_emulate_step(x, c, u, 6.0, row, SEED63, 5, step, scale_noise=False)[0], ref, tol,
              "sigma_up without s_noise")
    _rejected(_emulate_step(x, c, u, 6.0, row, SEED63, 6, step)[0], ref, tol, "image b + 1")
    _rejected(_emulate_step(x, c, u, 6.0, row, 5, 5, step)[0], ref, tol, "seed without bit 63")
