"""Per-element worst-case bounds of cgs_gemm_narrow and cgs_layernorm_rows4 (csrc/kernels/gemm_narrow.hip;
test_gemm_narrow_gpu.py), from the pieces of _bounds.py.

LN-linear, ref = act(LN64(x) W^T + b) + res with the LayerNorm in fp64 and unrounded. The kernel rounds the
normalised row to bf16 in LDS: every element is within tol_LN = layernorm_bound(x, gamma, beta, eps, depth) of LN64,
store included. The pre-activation is then off by the accumulation over the KP staged columns (the next multiple of
32 of K; the pad is zero) of operands of magnitude |LN| + tol_LN, and by the operand error through |W|:

    d_pre = C_ACC KP e mag + tol_LN |W|^T,    mag = (|LN| + tol_LN) |W|^T + |b| + |res|

fed through _act_tol as every fused epilogue is. Without LN the bound is gemm_act_bound(..., K=KP).
Dependent fp32 additions of a row sum (the ``depth`` of layernorm_bound), restated from the kernels:
  gemm_narrow  4 lanes a row; a lane adds its ceil(K / 16) 8-byte units in sequence, each summed as (a + b) + (c + d)
               (2); a 2-step butterfly: ceil(K / 16) + 4
  rows4        16 lanes a row; ceil(C / 64) units in sequence, each as a tree (2); a 4-step butterfly: ceil(C / 64) + 6
"""
from _bounds import C_ACC, E, _act_tol, _store, f64, gemm_act_bound, layernorm_bound


def narrow_ln_depth(K):
    return (K + 15) // 16 + 4


def rows4_ln_depth(C):
    return (C + 63) // 64 + 6


def narrow_linear_bound(x, w, bias, ln, act, res):
    """x [M, K] bf16, w [N, K], bias [N] | None, ln = (gamma | None, beta | None, eps) | None -> (ref, tol) [M, N]."""
    KP = (x.shape[-1] + 31) // 32 * 32
    if ln is None:
        return gemm_act_bound(x, w, bias, res, act, K=KP)
    z, tol_ln = layernorm_bound(x, ln[0], ln[1], ln[2], depth=narrow_ln_depth(x.shape[-1]))
    wa = f64(w).abs().t()
    pre, mag = z @ f64(w).t(), (z.abs() + tol_ln) @ wa
    if bias is not None:
        pre, mag = pre + f64(bias), mag + f64(bias).abs()
    if res is not None:
        mag = mag + f64(res).abs()
    return _act_tol(pre, C_ACC * KP * E * mag + tol_ln @ wa, res, act, 0.0)


def layernorm_rows4_bound(x, w, b, eps, res):
    """y = round(LN(x) w + b + res): layernorm_bound at the kernel's depth; with a residual the store is that of the
    sum, and the u |LN| of layernorm_bound's own store term stays as the allowance _act_tol makes for a residual."""
    ref, tol = layernorm_bound(x, w, b, eps, depth=rows4_ln_depth(x.shape[-1]))
    if res is None:
        return ref, tol
    return ref + f64(res), tol + _store(ref + f64(res))
