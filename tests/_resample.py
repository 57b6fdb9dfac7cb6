"""Shared inputs and oracles of the Lanczos / bislerp resampling tests (tests/test_resample_*.py).

``pil_lanczos`` and ``bislerp_fp32`` are frozen copies of what ``utils.image.lanczos`` / ``bislerp`` were
before they became ops: the tests pin the ops' torch path to them. ``bislerp_ref64`` is the same formula
in fp64 on the fp32-built tables, the oracle of the device bound.
"""
import numpy as np
import torch

# (H, W) -> (h, w): down, up, W only, H only, same size, windows clamped at both ends, more than one tile
LANCZOS_SHAPES = [((37, 53), (16, 20)), ((16, 20), (37, 53)), ((64, 48), (64, 31)), ((33, 40), (70, 40)),
                  ((40, 40), (40, 40)), ((9, 200), (5, 7)), ((300, 1100), (130, 517))]
LANCZOS_IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in LANCZOS_SHAPES]


def lanczos_input(n, h, w, seed=0):
    """[n, 3, h, w] fp32: uniform noise in [-0.1, 1.1] (both clamps), a run of exact 0 and 1, and the ramp
    k / 255 for every k, whose quantisation the truncation after the fp32 multiply decides."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((n, 3, h, w), generator=g) * 1.2 - 0.1
    flat = x.view(n, -1)
    flat[:, :256] = torch.arange(256, dtype=torch.float32) / 255.0
    flat[:, 256:288] = 0.0
    flat[:, 288:320] = 1.0
    return x


def pil_lanczos(samples, width, height):
    from PIL import Image
    imgs = [Image.fromarray(np.clip(255.0 * im.movedim(0, -1).cpu().numpy(), 0, 255).astype(np.uint8)) for im in samples]
    imgs = [im.resize((width, height), resample=Image.Resampling.LANCZOS) for im in imgs]
    imgs = [torch.from_numpy(np.array(im).astype(np.float32) / 255.0).movedim(-1, 0) for im in imgs]
    return torch.stack(imgs).to(samples.device, samples.dtype)


def _coords(l_in, l_out):
    ramp = torch.arange(l_out, dtype=torch.float32) * (l_in / l_out)
    c1 = ramp.floor().long()
    ratios = ramp - c1
    c2 = (c1 + 1).clamp(max=l_in - 1)
    return c1, c2, ratios


def _slerp(b1, b2, r, margins=None):
    c = b1.shape[-1]
    n1 = torch.norm(b1, dim=-1, keepdim=True)
    n2 = torch.norm(b2, dim=-1, keepdim=True)
    b1n = b1 / n1
    b2n = b2 / n2
    b1n[n1.expand(-1, c) == 0.0] = 0.0
    b2n[n2.expand(-1, c) == 0.0] = 0.0
    dot = (b1n * b2n).sum(1)
    if margins is not None:
        margins.append(float((dot.abs() - (1 - 1e-5)).abs().min()))
    omega = torch.acos(dot)
    so = torch.sin(omega)
    res = (torch.sin((1.0 - r.squeeze(1)) * omega) / so).unsqueeze(1) * b1n + \
          (torch.sin(r.squeeze(1) * omega) / so).unsqueeze(1) * b2n
    res *= (n1 * (1.0 - r) + n2 * r).expand(-1, c)
    res[dot > 1 - 1e-5] = b1[dot > 1 - 1e-5]
    res[dot < 1e-5 - 1] = (b1 * (1.0 - r) + b2 * r)[dot < 1e-5 - 1]
    return res


def _bislerp(samples, width, height, margins=None):
    n, c, h, w = samples.shape
    h_new, w_new = height, width
    c1, c2, r = _coords(w, w_new)
    c1 = c1.view(1, 1, 1, -1).expand((n, c, h, w_new))
    c2 = c2.view(1, 1, 1, -1).expand((n, c, h, w_new))
    r = r.to(samples.dtype).view(1, 1, 1, -1).expand((n, 1, h, w_new))
    p1 = samples.gather(-1, c1).movedim(1, -1).reshape((-1, c))
    p2 = samples.gather(-1, c2).movedim(1, -1).reshape((-1, c))
    r = r.movedim(1, -1).reshape((-1, 1))
    result = _slerp(p1, p2, r, margins).reshape(n, h, w_new, c).movedim(-1, 1)
    c1, c2, r = _coords(h, h_new)
    c1 = c1.view(1, 1, -1, 1).expand((n, c, h_new, w_new))
    c2 = c2.view(1, 1, -1, 1).expand((n, c, h_new, w_new))
    r = r.to(samples.dtype).view(1, 1, -1, 1).expand((n, 1, h_new, w_new))
    p1 = result.gather(-2, c1).movedim(1, -1).reshape((-1, c))
    p2 = result.gather(-2, c2).movedim(1, -1).reshape((-1, c))
    r = r.movedim(1, -1).reshape((-1, 1))
    return _slerp(p1, p2, r, margins).reshape(n, h_new, w_new, c).movedim(-1, 1)


def bislerp_fp32(samples, width, height):
    """The fp32 torch bislerp as it stood in utils/image.py (CPU tensors)."""
    return _bislerp(samples.float(), width, height).to(samples.dtype)


def bislerp_ref64(samples, width, height):
    """(result, margin): the same formula in fp64 on the fp32-built (c1, c2, ratio) tables, and the smallest
    ``| |dot| - (1 - 1e-5) |`` over every pair of both passes (the result jumps where that is 0)."""
    margins = []
    y = _bislerp(samples.detach().cpu().double(), width, height, margins)
    return y, min(margins)


# (N, C, H, W) -> (h, w), dtype
BISLERP_CASES = [((2, 4, 9, 13), (21, 30), torch.float32), ((1, 4, 16, 16), (24, 40), torch.float32),
                 ((2, 16, 7, 5), (3, 11), torch.float32), ((1, 4, 12, 20), (12, 7), torch.float32),
                 ((2, 4, 9, 13), (21, 30), torch.bfloat16), ("pairs", (7, 11), torch.float32)]
BISLERP_IDS = ["2x4x9x13-21x30", "1x4x16x16-24x40", "2x16x7x5-3x11", "1x4x12x20-12x7", "bf16", "pairs"]


def bislerp_input(shape, dtype, seed=0):
    """Gaussian noise, or for ``"pairs"`` a (1, 4, 4, 6) tensor whose neighbours along W and along H are zero
    vectors, parallel pairs (b2 = 2 b1) and antiparallel pairs (b2 = -0.5 b1)."""
    g = torch.Generator().manual_seed(seed)
    if shape != "pairs":
        return torch.randn(shape, generator=g).to(dtype)
    v, u, t = (torch.randn(4, generator=g) for _ in range(3))
    row = torch.stack([v, 2 * v, torch.zeros(4), u, -0.5 * u, t], dim=1)      # [C, 6]
    x = torch.stack([row, 2 * row, -row, torch.zeros_like(row)], dim=1)       # [C, 4, 6]: rows 1-2 antiparallel
    return x[None].to(dtype)
