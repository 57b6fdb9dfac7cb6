"""Per-element bound of ``ops.conv2d_into`` (csrc/kernels/dense.hip), in the terms of tests/_bounds.py.

    out = round_bf16(alpha * act(conv(x) + bias) + beta * res + res2)

The kernel accumulates the conv in fp32 (d_pre = C_ACC K e mag, as every conv bound here), applies the activation
with its own error d_act (``_act_tol`` with no residual), and forms the three-term sum in fp32: alpha and beta are
the fp32 values the kernel is passed, each product and each of the two additions rounds once, so every term is
charged 3 e of its magnitude. One rounding to bf16 at the store.
"""
import torch

from _bounds import C_ACC, E, U, _act_tol, _conv_pre_mag, _f32, _store, act_ref, f64


def conv_into_bound(x, w, bias, act, param, alpha, res, beta, res2):
    """(ref, tol) in fp64 for NCHW operands (``bias``, ``res``, ``res2`` may be None; ``act`` None: identity)."""
    pre, mag, K = _conv_pre_mag(x, w, bias, 1, 1, False, None)
    d_pre = C_ACC * K * E * mag
    y = act_ref(pre, act, param)
    # d_act: what _act_tol allows around round(act(pre)) without a residual, less that rounding
    _, t_act = _act_tol(pre, d_pre, None, act, param)
    d_act = (t_act - _store(y)) / (1 + U)
    alpha, beta = _f32(alpha), _f32(beta)
    r1 = torch.zeros_like(y) if res is None else f64(res)
    r2 = torch.zeros_like(y) if res2 is None else f64(res2)
    ref = alpha * y + beta * r1 + r2
    d = abs(alpha) * d_act + 3 * E * ((alpha * y).abs() + (beta * r1).abs() + r2.abs())
    tol = U * ref.abs() * (1 + 2 * U) + d * (1 + U)
    return ref, tol
