"""The CPU mirror of the device RNG (sampling/rng.py) on its own: the published known-answer vectors of
Philox4x32-10 tie its integer code to the generator it names, seed_i64 keeps all 64 bits of a seed through an int64
tensor, the rounding of the 24-bit uniform at its two ends is pinned, and an image's noise does not depend on the
batch it is drawn in."""
import math

import pytest
import torch

from comfy_gen_server_amd.sampling import rng

M64 = (1 << 64) - 1
# counter, key, output: the known-answer vectors of Philox4x32-10 (Random123, kat_vectors)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def _i64(v):
    return torch.tensor([v], dtype=torch.int64)


@pytest.mark.parametrize("counter,key,want", PHILOX_KAT)
def test_philox10_known_answers(counter, key, want):
    got = rng._philox10(*(_i64(c) for c in counter), *(_i64(k) for k in key))
    assert tuple(int(w) for w in got) == want, [hex(int(w)) for w in got]


@pytest.mark.parametrize("seed", [0, 5, (1 << 63) - 1, 1 << 63, (1 << 63) + 5, (1 << 64) - 1])
def test_seed_i64_round_trip(seed):
    s = rng.seed_i64(seed)
    assert -(1 << 63) <= s < (1 << 63)
    t = torch.tensor([s], dtype=torch.int64)               # what step_graph / run_graph store for the kernels
    assert int(t[0]) & M64 == seed
    assert rng.seed_i64(seed + (1 << 64)) == s             # only the low 64 bits count


def test_bit_63_of_the_seed_reaches_the_noise():
    a = rng.normal_groups(5, [0, 1], 8, 3)
    b = rng.normal_groups((1 << 63) + 5, [0, 1], 8, 3)
    assert not torch.equal(a, b)
    assert (a - b).abs().max().item() > 0.5
    assert torch.equal(b, rng.normal_groups(rng.seed_i64((1 << 63) + 5), [0, 1], 8, 3))


def test_u01_ends_and_rounding():
    """(k + 0.5) 2^-24 in fp32: exact below k = 2^23, rounded to even from there, 1.0 at the top."""
    u = rng._u01(torch.tensor([0, 0xFF, 0x100, ((1 << 23) - 1) << 8, ((1 << 23) + 1) << 8, ((1 << 23) + 2) << 8,
                               0xFFFFFFFF], dtype=torch.int64))
    assert u.dtype == torch.float32
    want = [2.0 ** -25, 2.0 ** -25, 1.5 * 2.0 ** -24, ((1 << 23) - 0.5) * 2.0 ** -24, ((1 << 23) + 2) * 2.0 ** -24,
            ((1 << 23) + 2) * 2.0 ** -24, 1.0]
    assert u.double().tolist() == want
    # the normals of the two ends: finite, and exactly 0 at u = 1
    ends = torch.tensor([2.0 ** -25, 1.0], dtype=torch.float32)
    r = torch.sqrt(-2.0 * torch.log(ends))
    assert bool(torch.isfinite(r).all()) and r[1].item() == 0.0
    assert abs(r[0].item() - math.sqrt(50 * math.log(2.0))) < 1e-5
    for t in (0.0, 1.0):
        z = r * torch.cos(torch.tensor(rng.TWO_PI, dtype=torch.float32) * t)
        assert bool(torch.isfinite(z).all()) and z[1].item() == 0.0


def test_all_ones_words_give_finite_normals():
    """A group whose four words are 0xFFFFFFFF (u = 1.0 four times) and one of zeros, through the mirror's own
    Box-Muller lines."""
    for word in (0xFFFFFFFF, 0):
        u = rng._u01(_i64(word))
        r = torch.sqrt(-2.0 * torch.log(u))
        t = torch.tensor(rng.TWO_PI, dtype=torch.float32) * u
        z = torch.stack([r * torch.cos(t), r * torch.sin(t)])
        assert bool(torch.isfinite(z).all()), (word, z)


def test_batch_independence_of_the_mirror():
    shape, seed, stream = (3, 4, 5, 7), (1 << 63) + 5, (1 << 32) + 7
    z = rng.randn_reference(shape, seed, [3, 4, 5], stream)
    for j, i in enumerate([3, 4, 5]):
        assert torch.equal(z[j:j + 1], rng.randn_reference((1,) + shape[1:], seed, [i], stream))
    assert not torch.equal(z[0], z[1])


def test_tail_is_a_prefix():
    a = rng.randn_reference((2, 7), 9, [0, 1], 2)
    b = rng.randn_reference((2, 8), 9, [0, 1], 2)
    assert torch.equal(a, b[:, :7])
