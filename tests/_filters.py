"""Shared inputs and oracles of the image-filter tests (tests/test_filters_*.py).

``gaussian_kernel``, ``_depthwise``, ``_dilate``, ``_erode``, ``canny_edges`` and ``gaussian_blur_2d`` are frozen
copies of what ``nodes/extras_image.py`` and ``nodes/extras_model.py`` ran before the filters became ops: the
tests pin the ops' torch path, and the nodes on CPU tensors, to them bit for bit. The fp64 oracles of the device
bounds follow the same formulas.
"""
import functools

import torch
import torch.nn.functional as F

from _bounds import C_ACC, E, TINY, u


# ---------------------------------------------------------------- frozen copies
def gaussian_kernel(kernel_size, sigma, device=None):
    lin = torch.linspace(-1, 1, kernel_size, device=device)
    y, x = torch.meshgrid(lin, lin, indexing="ij")
    g = torch.exp(-(x * x + y * y) / (2.0 * sigma * sigma))
    return g / g.sum()


def _depthwise(image_bhwc, kernel, radius):
    c = image_bhwc.shape[-1]
    x = image_bhwc.movedim(-1, 1)
    x = F.pad(x, (radius, radius, radius, radius), mode="reflect")
    k = kernel.to(x.dtype).expand(c, 1, *kernel.shape)
    y = F.conv2d(x, k, groups=c)
    return y.movedim(1, -1)


def blur_frozen(image, blur_radius, sigma):
    return _depthwise(image, gaussian_kernel(2 * blur_radius + 1, sigma, device=image.device), blur_radius)


def sharpen_kernel(gauss, alpha):
    """The unsharp-mask kernel as ImageSharpen builds it from its Gaussian (fp32 frozen, fp64 for the oracle)."""
    k = gauss * -(alpha * 10)
    c = k.shape[0] // 2
    k[c, c] = k[c, c] - k.sum() + 1.0
    return k


def sharpen_frozen(image, sharpen_radius, sigma, alpha):
    k = sharpen_kernel(gaussian_kernel(2 * sharpen_radius + 1, sigma, device=image.device), alpha)
    return _depthwise(image, k, sharpen_radius).clamp(0, 1)


def _dilate(x, k):
    p = k // 2
    return F.max_pool2d(F.pad(x, (p, k - 1 - p, p, k - 1 - p), mode="replicate"), k, stride=1)


def _erode(x, k):
    return -_dilate(-x, k)


MORPH_OPS = ["erode", "dilate", "open", "close", "gradient", "bottom_hat", "top_hat"]


def morphology_frozen(image, operation, k):
    x = image.movedim(-1, 1).float()
    y = {"erode": lambda: _erode(x, k), "dilate": lambda: _dilate(x, k), "open": lambda: _dilate(_erode(x, k), k),
         "close": lambda: _erode(_dilate(x, k), k), "gradient": lambda: _dilate(x, k) - _erode(x, k),
         "top_hat": lambda: x - _dilate(_erode(x, k), k), "bottom_hat": lambda: _erode(_dilate(x, k), k) - x}[operation]()
    return y.movedim(1, -1)


def canny_edges(img_bchw, low, high):
    if img_bchw.shape[1] == 3:
        gray = (0.299 * img_bchw[:, 0] + 0.587 * img_bchw[:, 1] + 0.114 * img_bchw[:, 2])[:, None]
    else:
        gray = img_bchw[:, :1]
    ax = torch.arange(5, dtype=gray.dtype, device=gray.device) - 2
    g1 = torch.exp(-ax ** 2 / 2.0)
    g1 = g1 / g1.sum()
    blur = F.conv2d(F.pad(gray, (2, 2, 2, 2), mode="reflect"), (g1[:, None] * g1[None, :])[None, None])
    sx = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], dtype=gray.dtype, device=gray.device)
    p = F.pad(blur, (1, 1, 1, 1), mode="replicate")
    gx = F.conv2d(p, sx[None, None])
    gy = F.conv2d(p, sx.t()[None, None])
    mag = torch.sqrt(gx * gx + gy * gy + 1e-6)
    ang = torch.rad2deg(torch.atan2(gy, gx)) % 180.0
    q = (((ang + 22.5) // 45) % 4).long()
    mp = F.pad(mag, (1, 1, 1, 1))
    H, W = mag.shape[-2:]

    def shift(dy, dx):
        return mp[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    offs = [((0, 1), (0, -1)), ((1, 1), (-1, -1)), ((1, 0), (-1, 0)), ((1, -1), (-1, 1))]
    n1 = torch.zeros_like(mag)
    n2 = torch.zeros_like(mag)
    for i, (a, b) in enumerate(offs):
        sel = q == i
        n1 = torch.where(sel, shift(*a), n1)
        n2 = torch.where(sel, shift(*b), n2)
    nms = torch.where((mag >= n1) & (mag >= n2), mag, torch.zeros_like(mag))
    strong = nms > high
    weak = (nms > low) & ~strong
    edges = strong.float()
    for _ in range(max(H, W)):
        grown = (F.max_pool2d(edges, 3, stride=1, padding=1) > 0) & weak
        new = torch.maximum(edges, grown.float())
        if torch.equal(new, edges):
            break
        edges = new
    return mag, edges


def gaussian_blur_2d(img, kernel_size, sigma):
    half = (kernel_size - 1) * 0.5
    t = torch.linspace(-half, half, steps=kernel_size, device=img.device, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (t / sigma).pow(2))
    k1 = (pdf / pdf.sum()).to(dtype=img.dtype)
    k2 = torch.outer(k1, k1).expand(img.shape[-3], 1, kernel_size, kernel_size)
    p = kernel_size // 2
    return F.conv2d(F.pad(img, (p, p, p, p), mode="reflect"), k2, groups=img.shape[-3])


def hysteresis_frozen(cls):
    """The hysteresis loop of ``canny_edges`` on a class map (2 strong, 1 weak), run until nothing changes."""
    strong, weak = cls == 2, cls == 1
    edges = strong.float()
    while True:
        grown = (F.max_pool2d(edges, 3, stride=1, padding=1) > 0) & weak
        new = torch.maximum(edges, grown.float())
        if torch.equal(new, edges):
            return edges
        edges = new


# ---------------------------------------------------------------- inputs
def filter_input(shape, dtype=torch.float32, seed=0):
    """Uniform in [-0.1, 1.1]: the sharpen clamp acts on both sides."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 1.2 - 0.1).to(dtype)


def field(seed, size=(70, 90)):
    """A smooth random RGB field with long contours plus a little noise, in [0, 1]: [1, 3, H, W]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((1, 3, 9, 11), generator=g)
    x = F.interpolate(x, size=size, mode="bicubic", align_corners=True)
    x = x + 0.02 * torch.randn(x.shape, generator=g)
    return x.clamp(0, 1)


def random_classes(seed=0, shape=(2, 1, 70, 90)):
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(shape, generator=g)
    return torch.where(r < 0.02, 2, torch.where(r < 0.52, 1, 0)).to(torch.uint8)


def serpentine(H=150, W=270, strong=True):
    """A one-pixel weak path: every even row over the full width, joined at alternating ends by one pixel of the
    odd row between; one strong pixel at its last cell. Returns (class map [1, 1, H, W], path mask)."""
    cls = torch.zeros((1, 1, H, W), dtype=torch.uint8)
    rows = list(range(0, H, 2))
    for i, r in enumerate(rows):
        cls[0, 0, r, :] = 1
        if i + 1 < len(rows):
            cls[0, 0, r + 1, W - 1 if i % 2 == 0 else 0] = 1
    path = cls == 1
    last = (rows[-1], W - 1 if (len(rows) - 1) % 2 == 0 else 0)
    if strong:
        cls[0, 0, last[0], last[1]] = 2
    return cls, path


# ---------------------------------------------------------------- fp64 oracles
def gaussian_kernel64(kernel_size, sigma):
    lin = torch.linspace(-1, 1, kernel_size, dtype=torch.float64)
    y, x = torch.meshgrid(lin, lin, indexing="ij")
    g = torch.exp(-(x * x + y * y) / (2.0 * sigma * sigma))
    return g / g.sum()


def pixel_kernel64(kernel_size, sigma):
    half = (kernel_size - 1) * 0.5
    t = torch.linspace(-half, half, steps=kernel_size, dtype=torch.float64)
    pdf = torch.exp(-0.5 * (t / sigma).pow(2))
    k1 = pdf / pdf.sum()
    return torch.outer(k1, k1)


def _corr64(x64, k2, border):
    rh, rw = k2.shape[0] // 2, k2.shape[1] // 2
    c = x64.shape[1]
    xp = F.pad(x64, (rw, rw, rh, rh)) if border == "zero" else F.pad(x64, (rw, rw, rh, rh), mode=border)
    return F.conv2d(xp, k2.expand(c, 1, *k2.shape), groups=c)


def filter_ref_and_tol(x_nchw, g2, ax=0.0, ay=1.0, clamp=None, border="reflect", ref_kernel=None):
    """fp64 reference of ``clamp(ax x + ay (G * x))`` with the dense normalised 2-D kernel ``g2`` (fp64; or the
    correlation with ``ref_kernel``, the dense kernel a node builds with ax / ay folded in), and the per-element
    bound of ``cgs_filter_sep``:

      tol = u(dtype) |ref| (1 + 2u) + tiny + C_ACC (kw + kh + 6) e mag,   mag = |ax| |x| + |ay| (|G| * |x|)

    The kernel forms each horizontal sum as a chain of kw fmaf's and each vertical sum as a chain of kh over those:
    a chain of k fused terms is within k e of its exact value relative to the sum of magnitudes (first order; C_ACC = 2
    covers the higher orders and the second pass acting on the rounded first), so the two passes give
    (kw + kh) e (|t_h| (x) |t_w| * |x|). The + 6: the fp32 taps differ from the fp64 ones by the roundings of
    linspace, the square, the division by 2 sigma^2 and expf (the argument error is weighted by the tap itself, and
    sum t_i arg_i <= 1/2 for a Gaussian), the normalising sum and the division: 3 e relative at the most; then the
    product ay * acc, the fused ax * x + (.) and nothing else: 2 e; 1 e spare. The clamp moves no value away from
    the reference. The store adds one rounding of the result to the dtype of x (none beyond fp32's own for fp32)."""
    x64 = x_nchw.double()
    kh, kw = g2.shape
    ref = _corr64(x64, ref_kernel, border) if ref_kernel is not None else ax * x64 + ay * _corr64(x64, g2, border)
    if clamp is not None:
        ref = ref.clamp(*clamp)
    mag = abs(ax) * x64.abs() + abs(ay) * _corr64(x64.abs(), g2.abs(), border)
    ud = u(x_nchw.dtype)
    tol = ud * ref.abs() * (1 + 2 * ud) + TINY[x_nchw.dtype] + C_ACC * (kw + kh + 6) * E * mag
    return ref, tol


# delta of |mag - mag64| for canny_classes on inputs in [0, 1] (e = 2^-24):
#   gray: three products with coefficients rounded to fp32 and two sums, values <= 1          ->   6 e
#   blur: the filter bound with kw = kh = 5 and mag <= 1, C_ACC (5 + 5 + 6) e = 32 e, plus the gray error -> 38 e
#   Sobel: sum |coef| = 8 carries 8 x 38 e = 304 e; its own differences, doubling and sums (|gx| <= 4) 20 e -> 324 e
#   mag = sqrt(gx^2 + gy^2 + 1e-6) is 1-Lipschitz in (gx, gy): sqrt(2) x 324 e = 458 e; two squares, two sums and the
#   square root at 3 e relative of mag <= 4 sqrt(2): 17 e                                        -> 475 e
CANNY_DELTA = 480 * E


def canny_ref64(img, low, high):
    """fp64 Canny up to the classes -> (mag, classes uint8, decision margin per pixel)."""
    x = img.double()
    gray = (0.299 * x[:, 0] + 0.587 * x[:, 1] + 0.114 * x[:, 2])[:, None] if x.shape[1] == 3 else x[:, :1]
    blur = _corr64(gray, pixel_kernel64(5, 1.0), "reflect")
    sx = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], dtype=torch.float64)
    p = F.pad(blur, (1, 1, 1, 1), mode="replicate")
    gx = F.conv2d(p, sx[None, None])
    gy = F.conv2d(p, sx.t()[None, None])
    mag = torch.sqrt(gx * gx + gy * gy + 1e-6)
    ang = torch.rad2deg(torch.atan2(gy, gx)) % 180.0
    q = (((ang + 22.5) // 45) % 4).long()
    mp = F.pad(mag, (1, 1, 1, 1))
    H, W = mag.shape[-2:]

    def shift(dy, dx):
        return mp[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    offs = [((0, 1), (0, -1)), ((1, 1), (-1, -1)), ((1, 0), (-1, 0)), ((1, -1), (-1, 1))]
    n1 = torch.zeros_like(mag)
    n2 = torch.zeros_like(mag)
    for i, (a, b) in enumerate(offs):
        sel = q == i
        n1 = torch.where(sel, shift(*a), n1)
        n2 = torch.where(sel, shift(*b), n2)
    nms = torch.where((mag >= n1) & (mag >= n2), mag, torch.zeros_like(mag))
    cls = torch.where(nms > high, 2, torch.where(nms > low, 1, 0)).to(torch.uint8)
    d = (ang - 22.5) % 45.0                      # degrees past the last sector boundary
    dtheta = torch.deg2rad(torch.minimum(d, 45.0 - d))
    margin = torch.stack([(mag - n1).abs(), (mag - n2).abs(), (mag - low).abs(), (mag - high).abs(),
                          mag * torch.sin(dtheta)]).amin(0)
    return mag, cls, margin


@functools.lru_cache(maxsize=None)
def canny_case(seed, low=0.1, high=0.3):
    img = field(seed)
    return (img,) + canny_ref64(img, low, high)
