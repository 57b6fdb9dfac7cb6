"""Per-element error bounds (tests/_bounds.py) on the device for the bf16 GEMM, conv and attention kernels.

Every case names one kernel and a shape inside that kernel's own dispatch domain, so the kernel of the test id is
the one that runs (gemm_dispatch / conv_launch / flash_attn_dispatch fall through to another kernel outside it; only
test_conv_bound_variant_fallback relies on that, to pin where the convs fall). References are fp64 on the device. The shapes are the smallest that reach an edge: a single
partial tile, one row / one 8-wide vector past a full tile, the minimum K, an odd number of K steps, more tiles
than a persistent kernel's workgroups, the workspace (split-K) paths. The guard tests place C with ldc = N + 8 in
the middle of a pattern-filled buffer and require every element outside [0, M) x [0, N) to keep its bits; their
four row strides all differ (lda = K + 8, ldw = K + 16, ldc = N + 8, ldr = N + 16, every operand a view of a wider
allocation), so a launcher that swaps two of them misses the bound; test_attention_bound_distinct_strides does the
same for the attention entries' twelve strides."""
import math

import pytest
import torch

from comfy_gen_server_amd import ops, _native
from comfy_gen_server_amd.ops import core

from _bounds import assert_within, attention_bound, conv_bound, geglu_bound, gemm_bound, lnfold_bound

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(autouse=True)
def _native_loaded(cuda, monkeypatch):
    assert _native.load_kernels() is not None, _native.kernels_error()
    monkeypatch.setenv("CGS_AUTOTUNE", "0")    # the tests pick the kernel explicitly
    ops.reset_stats()
    yield


# ------------------------------------------------------------------------------------------------ GEMM domains
# Read from gemm_dispatch and the launchers (csrc/kernels/gemm.hip, gemm_w6.hip cgs_gemm_w6_ok):
#   variant  the number cgs_gemm_bf16_v takes        min_k / k_mod  smallest K and its modulus
#   k_step   K consumed per main-loop step           n_mod          modulus of N
#   bm x bn  tile                                    min_m / min_n / max_m  bounds on M and N
#   grid     persistent kernels: workgroups launched per CU (the launcher caps the grid there), else 0
# v3: bn = mc::pick_bn(M, N), 128 for every grid under one round of 256 tiles (checked per case by _pick_bn).
# v2: bn = 128 for N < 1024. skinny: all M <= 128 rows in one workgroup of 16 columns.
def _k(variant, min_k, k_mod, k_step, n_mod, bm, bn, min_m=1, min_n=8, max_m=1 << 30, grid=0, entry="v"):
    return dict(variant=variant, min_k=min_k, k_mod=k_mod, k_step=k_step, n_mod=n_mod, bm=bm, bn=bn, min_m=min_m,
                min_n=min_n, max_m=max_m, grid=grid, entry=entry)


GEMM_KERNELS = {
    "v1": _k(1, 8, 8, 64, 8, 128, 128),
    "v2": _k(2, 64, 64, 64, 8, 256, 128, min_m=256, min_n=128),
    "v3w4": _k(3, 32, 32, 32, 8, 256, 128),
    "v3w8": _k(4, 32, 32, 32, 8, 256, 128),
    "v5pp": _k(5, 64, 64, 64, 8, 256, 256),
    "v6pp160": _k(6, 128, 64, 64, 8, 256, 160, grid=1),
    "v7ppk": _k(7, 128, 64, 64, 8, 256, 256, grid=1),
    "v8t128": _k(8, 32, 32, 32, 8, 128, 128),
    "v10t64x128": _k(10, 32, 32, 32, 8, 64, 128),
    "v11t128x64": _k(11, 32, 32, 32, 8, 128, 64),
    "v12t64x128s6": _k(12, 32, 32, 32, 8, 64, 128),
    "v13t128x64s6": _k(13, 32, 32, 32, 8, 128, 64),
    "v14t128s5": _k(14, 32, 32, 32, 8, 128, 128),
    "skinny": _k(9, 32, 32, 32, 8, 128, 16, max_m=128),
    "w6": _k(16, 128, 128, 128, 16, 256, 256, grid=1),
    "w6n160": _k(17, 128, 128, 128, 16, 256, 160, grid=1),
    "v6m128": _k(19, 128, 64, 64, 8, 128, 160, grid=1),
    "v6w4": _k(20, 128, 64, 64, 8, 128, 80, grid=2),
    "w8": _k(None, 8, 8, 64, 8, 128, 128, entry="w8"),
}
EPIS = ["none", "bias", "bias_res"]


def _in_domain(s, M, N, K):
    return (K >= s["min_k"] and K % s["k_mod"] == 0 and N % s["n_mod"] == 0 and s["min_m"] <= M <= s["max_m"]
            and N >= s["min_n"])


def _pick_bn(M, N):      # mc::pick_bn (mfma_core.h)
    tm = (M + 255) // 256
    t256, t128 = tm * ((N + 255) // 256), tm * ((N + 127) // 128)
    return 128 if ((t128 + 255) // 256) * 128 < ((t256 + 255) // 256) * 256 else 256


def _partial_shape(s):
    """One partial tile: M < bm and N < bn with N % 8 == 0 and N % 16 != 0 (w6: N % 16 == 0 and N % 32 != 0); a
    kernel with a minimum M / N of a full tile gets one row / one vector more than that."""
    M = s["bm"] - 3 if s["min_m"] < s["bm"] else s["min_m"] + 1
    N = s["bn"] - s["n_mod"] if s["min_n"] < s["bn"] else s["min_n"] + s["n_mod"]
    return M, N


def _edge_shape(s):
    """M = bm + 1 and N = bn + 8 (one n_mod): a second tile row and column that hold one row / one vector."""
    return min(s["bm"] + 1, s["max_m"]), s["bn"] + s["n_mod"]


def _gemm_cases():
    cases = []
    for name, s in GEMM_KERNELS.items():
        (Mp, Np), (Me, Ne) = _partial_shape(s), _edge_shape(s)
        ks = {s["min_k"], 3 * s["k_step"]}
        if s["k_mod"] < s["k_step"]:
            ks.add(s["k_step"] + s["k_mod"])            # a last K step that is not full (v1 / w8: K = 72)
        shapes = {(Mp, Np, s["min_k"])} | {(Me, Ne, K) for K in ks}
        if name == "skinny":
            shapes |= {(1, 8, 32), (1, 24, 96), (17, 24, 32)}
        if name in ("v3w4", "v3w8"):
            shapes.add((4097, 2056, 32))                # pick_bn == 256
        cases += [(name,) + sh for sh in sorted(shapes)]
    return cases


def _operands(cuda, M, N, K, epi, lda=None, ldw=None, ldr=None, seed=0, w8=False):
    """Activations randn + 0.5 (a dropped K slab is coherent, not noise), weights randn / sqrt(K) (w8: as fp8
    e4m3fn), bias and residual randn; a / w / r optionally as row-strided views of a wider buffer (the fp8 weights
    are converted whole and sliced after: .to() on a view packs it)."""
    torch.manual_seed(seed)
    lda, ldw, ldr = lda or K, ldw or K, ldr or N
    a = (torch.randn(M, lda, device=cuda) + 0.5).to(BF)[:, :K]
    w = (torch.randn(N, ldw, device=cuda) / math.sqrt(K)).to(BF)
    w = (w.to(torch.float8_e4m3fn) if w8 else w)[:, :K]
    b = torch.randn(N, device=cuda).to(BF) if epi != "none" else None
    r = torch.randn(M, ldr, device=cuda).to(BF)[:, :N] if epi == "bias_res" else None
    return a, w, b, r


def _ptr(t):
    return None if t is None else t.data_ptr()


def _launch_gemm(name, a, w, c, b, r, M, N, K, ldc):
    """Run the named kernel through its C entry; c = pointer of C[0, 0]."""
    lib, s = _native.load_kernels(), GEMM_KERNELS[name]
    assert _in_domain(s, M, N, K), (name, M, N, K)
    epi = (core.EPI_BIAS if b is not None else 0) | (core.EPI_RESIDUAL if r is not None else 0)
    lda, ldr = a.stride(0), (r.stride(0) if r is not None else 0)
    if name in ("v3w4", "v3w8"):
        assert _pick_bn(M, N) == (256 if (M, N) == (4097, 2056) else s["bn"])
    if name == "v2":
        assert N < 1024
    if s["entry"] == "w8":
        assert w.dtype == torch.float8_e4m3fn
        return lib.cgs_gemm_bf16_w8(a.data_ptr(), w.data_ptr(), c, _ptr(b), _ptr(r), M, N, K, lda, w.stride(0), ldc,
                                    ldr, epi, 1.0, core._stream())
    if name in ("w6", "w6n160"):
        assert lib.cgs_gemm_w6_ok(M, N, K, lda, w.stride(0), ldc, ldr, epi, s["bn"]) == 1
        assert all(p is None or p % 16 == 0 for p in (a.data_ptr(), w.data_ptr(), c, _ptr(b), _ptr(r)))
    return lib.cgs_gemm_bf16_v(a.data_ptr(), w.data_ptr(), c, _ptr(b), _ptr(r), M, N, K, lda, w.stride(0), ldc, ldr,
                               epi, 1.0, s["variant"], core._stream())


def _is_w8(name):
    return GEMM_KERNELS[name]["entry"] == "w8"


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("name,M,N,K", _gemm_cases())
def test_gemm_bound(cuda, name, M, N, K, epi):
    a, w, b, r = _operands(cuda, M, N, K, epi, w8=_is_w8(name))
    out = torch.empty(M, N, device=cuda, dtype=BF)
    assert _launch_gemm(name, a, w, out.data_ptr(), b, r, M, N, K, N) == 0
    ref, tol = gemm_bound(a, w.float(), b, r)
    assert_within(out, ref, tol, f"gemm/{name} {M}x{N}x{K} {epi}")


def _persistent_shape(s, cus):
    """More tiles than the grid (grid = s['grid'] workgroups per CU), the last round ragged: 5 tile columns (the
    last one 8 wide) x enough tile rows (the last one row high) for grid + 5 .. grid + 10 tiles."""
    grid = s["grid"] * cus
    tiles_m = grid // 5 + 2
    M, N = (tiles_m - 1) * s["bm"] + 1, 4 * s["bn"] + s["n_mod"]
    T = tiles_m * 5
    assert grid < T < 2 * grid and T % grid
    return M, N


@pytest.mark.parametrize("epi", ["bias_res"])
@pytest.mark.parametrize("name", [n for n, s in GEMM_KERNELS.items() if s["grid"]])
def test_gemm_bound_persistent_ragged_round(cuda, name, epi):
    s = GEMM_KERNELS[name]
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    M, N = _persistent_shape(s, cus)
    K = s["min_k"]
    a, w, b, r = _operands(cuda, M, N, K, epi)
    out = torch.empty(M, N, device=cuda, dtype=BF)
    assert _launch_gemm(name, a, w, out.data_ptr(), b, r, M, N, K, N) == 0
    ref, tol = gemm_bound(a, w, b, r)
    assert_within(out, ref, tol, f"gemm/{name} persistent {M}x{N}x{K} on {cus} CUs {epi}")


# ---- workspace (split-K) paths
@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("M,N,K", [(300, 264, 3072), (253, 248, 4096)])
def test_gemm_bound_v7_split_tail(cuda, M, N, K, epi):
    lib = _native.load_kernels()
    assert _in_domain(GEMM_KERNELS["v7ppk"], M, N, K)
    ws_bytes = lib.cgs_v7_ws_bytes(M, N, K)
    assert ws_bytes > 0, "shape chosen to take the split tail"
    a, w, b, r = _operands(cuda, M, N, K, epi)
    ws = torch.full((ws_bytes,), 0x7F, dtype=torch.uint8, device=cuda)
    out = torch.empty(M, N, device=cuda, dtype=BF)
    flags = (1 if b is not None else 0) | (2 if r is not None else 0)
    assert lib.cgs_gemm_bf16_v7ws(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(b), _ptr(r), M, N, K, K, K, N,
                                  N if r is not None else 0, flags, 1.0, ws.data_ptr(), ws_bytes, core._stream()) == 0
    ref, tol = gemm_bound(a, w, b, r)
    assert_within(out, ref, tol, f"gemm/v7ppk split tail {M}x{N}x{K} {epi}")


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("M,N,K", [(1, 8, 4096), (77, 264, 4096), (128, 24, 4128)])
def test_gemm_bound_skinny_split(cuda, M, N, K, epi):
    lib = _native.load_kernels()
    assert _in_domain(GEMM_KERNELS["skinny"], M, N, K)
    ws_bytes = lib.cgs_gemm_skinny_ws_bytes(M, N, K)
    assert ws_bytes > 0, "shape chosen to take the K-split"
    a, w, b, r = _operands(cuda, M, N, K, epi)
    ws = torch.full((ws_bytes,), 0x7F, dtype=torch.uint8, device=cuda)
    out = torch.empty(M, N, device=cuda, dtype=BF)
    flags = (1 if b is not None else 0) | (2 if r is not None else 0)
    assert lib.cgs_gemm_skinny_ws(a.data_ptr(), w.data_ptr(), out.data_ptr(), _ptr(b), _ptr(r), M, N, K, K, K, N,
                                  N if r is not None else 0, flags, 1.0, ws.data_ptr(), ws_bytes, core._stream()) == 0
    ref, tol = gemm_bound(a, w, b, r)
    assert_within(out, ref, tol, f"gemm/skinny split {M}x{N}x{K} {epi}")


SPLITK_TILES = {8: (128, 128), 10: (64, 128), 11: (128, 64), 14: (128, 128)}     # cgs_gemm_bf16_splitk: bm x bn


def _splitk(lib, variant, splits, a, w, c, b, r, M, N, K, ldc, ws):
    flags = (1 if b is not None else 0) | (2 if r is not None else 0)
    assert K % (32 * splits) == 0 and N % 8 == 0
    return lib.cgs_gemm_bf16_splitk(a.data_ptr(), w.data_ptr(), c, _ptr(b), _ptr(r), None, None, M, N, K, a.stride(0),
                                    w.stride(0), ldc, r.stride(0) if r is not None else 0, flags, 1.0, splits, variant,
                                    ws.data_ptr(), ws.numel(), core._stream())


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("splits,K", [(2, 64), (3, 288), (8, 256)])
@pytest.mark.parametrize("variant", sorted(SPLITK_TILES))
def test_gemm_bound_splitk(cuda, variant, splits, K, epi):
    lib = _native.load_kernels()
    bm, bn = SPLITK_TILES[variant]
    for M, N in ((bm - 3, bn - 8), (bm + 1, bn + 8)):
        a, w, b, r = _operands(cuda, M, N, K, epi)
        ws = torch.full((int(lib.cgs_splitk_ws_bytes(M, N, splits)),), 0x7F, dtype=torch.uint8, device=cuda)
        out = torch.empty(M, N, device=cuda, dtype=BF)
        assert _splitk(lib, variant, splits, a, w, out.data_ptr(), b, r, M, N, K, N, ws) == 0
        ref, tol = gemm_bound(a, w, b, r)
        assert_within(out, ref, tol, f"gemm/splitk v{variant} x{splits} {M}x{N}x{K} {epi}")


# ---- a kernel writes only its own output
def _guarded_c(cuda, M, N, bm):
    """C = rows of ldc = N + 8 in the middle of an int16 pattern: 4096 elements before, bm rows after."""
    ldc = N + 8
    n = 4096 + (M + bm) * ldc
    buf = ((torch.arange(n, device=cuda, dtype=torch.int64) * 2654435761 >> 7) & 0x7FFF).to(torch.int16)
    return buf, buf.clone(), ldc


def _check_guard(buf, before, M, N, ldc, what):
    c = buf[4096:4096 + M * ldc].view(M, ldc)
    keep = before.clone()
    keep[4096:4096 + M * ldc].view(M, ldc)[:, :N] = c[:, :N]
    changed = (buf != keep).nonzero().flatten()
    assert changed.numel() == 0, (f"{what}: {changed.numel()} elements outside [0, {M}) x [0, {N}) changed, first at "
                                  f"buffer offset {int(changed[0])} (C starts at 4096, ldc {ldc})")
    return c[:, :N].view(BF)


@pytest.mark.parametrize("name", list(GEMM_KERNELS))
def test_gemm_writes_only_its_output(cuda, name):
    s = GEMM_KERNELS[name]
    M, N = _partial_shape(s)
    K = s["min_k"]
    a, w, b, r = _operands(cuda, M, N, K, "bias_res", lda=K + 8, ldw=K + 16, ldr=N + 16, w8=_is_w8(name))
    buf, before, ldc = _guarded_c(cuda, M, N, s["bm"])
    assert _launch_gemm(name, a, w, buf.data_ptr() + 2 * 4096, b, r, M, N, K, ldc) == 0
    torch.cuda.synchronize()
    out = _check_guard(buf, before, M, N, ldc, f"gemm/{name}")
    ref, tol = gemm_bound(a, w.float(), b, r)
    assert_within(out, ref, tol, f"gemm/{name} guarded, strided {M}x{N}x{K}")


@pytest.mark.parametrize("kind", ["v7ws", "skinny_ws"] + [f"splitk{v}" for v in sorted(SPLITK_TILES)])
def test_gemm_workspace_paths_write_only_their_output(cuda, kind):
    lib = _native.load_kernels()
    if kind == "v7ws":
        M, N, K, bm = 253, 248, 3072, 256
        ws_bytes = lib.cgs_v7_ws_bytes(M, N, K)
    elif kind == "skinny_ws":
        M, N, K, bm = 125, 8, 4096, 128
        ws_bytes = lib.cgs_gemm_skinny_ws_bytes(M, N, K)
    else:
        bm, bn = SPLITK_TILES[int(kind[6:])]
        M, N, K = bm - 3, bn - 8, 64
        ws_bytes = lib.cgs_splitk_ws_bytes(M, N, 2)
    assert ws_bytes > 0
    a, w, b, r = _operands(cuda, M, N, K, "bias_res", lda=K + 8, ldw=K + 16, ldr=N + 16)
    ws = torch.full((int(ws_bytes),), 0x7F, dtype=torch.uint8, device=cuda)
    buf, before, ldc = _guarded_c(cuda, M, N, bm)
    c = buf.data_ptr() + 2 * 4096
    if kind == "v7ws":
        rc = lib.cgs_gemm_bf16_v7ws(a.data_ptr(), w.data_ptr(), c, b.data_ptr(), r.data_ptr(), M, N, K, a.stride(0),
                                    w.stride(0), ldc, r.stride(0), 3, 1.0, ws.data_ptr(), ws_bytes, core._stream())
    elif kind == "skinny_ws":
        rc = lib.cgs_gemm_skinny_ws(a.data_ptr(), w.data_ptr(), c, b.data_ptr(), r.data_ptr(), M, N, K, a.stride(0),
                                    w.stride(0), ldc, r.stride(0), 3, 1.0, ws.data_ptr(), ws_bytes, core._stream())
    else:
        rc = _splitk(lib, int(kind[6:]), 2, a, w, c, b, r, M, N, K, ldc, ws)
    assert rc == 0
    torch.cuda.synchronize()
    out = _check_guard(buf, before, M, N, ldc, f"gemm/{kind}")
    ref, tol = gemm_bound(a, w, b, r)
    assert_within(out, ref, tol, f"gemm/{kind} guarded, strided {M}x{N}x{K}")


# ---- GEGLU and LayerNorm-fold forms
# cgs_gemm_bf16_v with EPI_GEGLU (N2 = 2 No columns, N2 % 32; v6: N2 % 160; w6: the 256-wide form only; the
# 128-row v6 forms have none). (M, N2) per kernel: a partial tile, then one row / one 32-column group past a tile.
def _geglu_cases():
    cases = []
    for name in ("v1", "v2", "v3w4", "v3w8", "v5pp", "v6pp160", "v7ppk", "v8t128", "v10t64x128", "v11t128x64",
                 "v12t64x128s6", "v13t128x64s6", "v14t128s5", "w6"):
        s = GEMM_KERNELS[name]
        Mp = s["bm"] - 3 if s["min_m"] < s["bm"] else s["min_m"] + 1
        if name == "v6pp160":
            n2 = (160, 480)
        else:
            n2 = (96 if s["min_n"] < 96 else 160, s["bn"] + 32)
        cases += [(name, Mp, n2[0], s["min_k"]), (name, s["bm"] + 1, n2[1], 3 * s["k_step"])]
    return cases


@pytest.mark.parametrize("name,M,N2,K", _geglu_cases())
def test_gemm_geglu_bound(cuda, name, M, N2, K):
    lib, s = _native.load_kernels(), GEMM_KERNELS[name]
    assert _in_domain(s, M, N2, K) and N2 % 32 == 0 and (name != "v6pp160" or N2 % 160 == 0)
    a, w, b, _ = _operands(cuda, M, N2, K, "bias")
    wi, bi = core.geglu_interleave(w), core.geglu_interleave(b)
    out = torch.empty(M, N2 // 2, device=cuda, dtype=BF)
    epi = core.EPI_BIAS | core.EPI_GEGLU
    if name == "w6":
        assert lib.cgs_gemm_w6_ok(M, N2, K, K, K, N2 // 2, 0, epi, 256) == 1
    assert lib.cgs_gemm_bf16_v(a.data_ptr(), wi.data_ptr(), out.data_ptr(), bi.data_ptr(), None, M, N2, K, K, K,
                               N2 // 2, 0, epi, 1.0, s["variant"], core._stream()) == 0
    ref, tol = geglu_bound(a, w, b)
    assert_within(out, ref, tol, f"geglu/{name} {M}x{N2}x{K}")


# cgs_gemm_bf16_lnfold_v (gemm_lnfold): K % 64, K >= 128; v6 / v6m128: N % 160; v6w4: N % 80; w6: K % 128, N % 16.
# With GEGLU (N counts both halves, N % 32): v6, v7, the small tiles and the 256-wide w6 have the form.
# name -> (N of the partial-tile case, N of the edge case), then the same with GEGLU
LNFOLD_KERNELS = {"v6pp160": (160, 320), "v7ppk": (248, 264), "v8t128": (120, 136), "v10t64x128": (120, 136),
                  "v11t128x64": (56, 72), "v12t64x128s6": (120, 136), "v13t128x64s6": (56, 72),
                  "v14t128s5": (120, 136), "w6": (240, 272), "w6n160": (144, 176), "v6m128": (160, 320),
                  "v6w4": (80, 240)}
LNFOLD_GEGLU_KERNELS = {"v6pp160": (160, 480), "v7ppk": (224, 288), "v8t128": (96, 160), "v10t64x128": (96, 160),
                        "v11t128x64": (32, 96), "v12t64x128s6": (96, 160), "v13t128x64s6": (32, 96),
                        "v14t128s5": (96, 160), "w6": (224, 288)}


@pytest.mark.parametrize("name,geglu", [(n, False) for n in LNFOLD_KERNELS] + [(n, True) for n in LNFOLD_GEGLU_KERNELS])
def test_gemm_lnfold_bound(cuda, name, geglu):
    lib, s = _native.load_kernels(), GEMM_KERNELS[name]
    n_part, n_edge = (LNFOLD_GEGLU_KERNELS if geglu else LNFOLD_KERNELS)[name]
    for M, N, K in ((s["bm"] - 3, n_part, 128), (s["bm"] + 1, n_edge, 3 * max(64, s["k_step"]))):
        assert K % max(64, s["k_mod"]) == 0 and K >= 128 and N % s["n_mod"] == 0 and (not geglu or N % 32 == 0)
        torch.manual_seed(1)
        x = (torch.randn(M, K, device=cuda) * 3 + 1.5).to(BF)
        gamma = (torch.rand(K, device=cuda) + 0.5).to(BF)
        beta = (torch.randn(K, device=cuda) * 0.2).to(BF)
        w = (torch.randn(N, K, device=cuda) / math.sqrt(K)).to(BF)
        b = torch.randn(N, device=cuda).to(BF)
        rs = ops.layernorm_stats(x, 1e-5)
        w2, cs, b2 = ops.lnfold_weights(w, b, gamma, beta)              # plain row order: what the bound reads
        wk, ck, bk = (core.geglu_interleave(t) for t in (w2, cs, b2)) if geglu else (w2, cs, b2)
        nout = N // 2 if geglu else N
        epi = core.EPI_BIAS | (core.EPI_GEGLU if geglu else 0)
        if name in ("w6", "w6n160"):
            assert lib.cgs_gemm_w6_ok(M, N, K, K, K, nout, 0, epi | core.EPI_LNFOLD, s["bn"]) == 1
        out = torch.empty(M, nout, device=cuda, dtype=BF)
        assert lib.cgs_gemm_bf16_lnfold_v(x.data_ptr(), wk.data_ptr(), out.data_ptr(), bk.data_ptr(), rs.data_ptr(),
                                          ck.data_ptr(), M, N, K, K, K, nout, epi, None, 0, s["variant"],
                                          core._stream()) == 0
        ref, tol = lnfold_bound(x, w2, b2, rs, cs, geglu=geglu)
        assert_within(out, ref, tol, f"lnfold/{name} {M}x{N}x{K} geglu={geglu}")


@pytest.mark.parametrize("form", ["geglu", "lnfold", "lnfold_geglu"])
def test_gemm_bound_v7_split_tail_forms(cuda, form):
    """The GEGLU and LayerNorm-fold epilogues of v7 on a tile that the split-K tail reduces."""
    lib = _native.load_kernels()
    geglu, ln = form.endswith("geglu"), form.startswith("lnfold")
    M, N, K = 253, (224 if geglu else 248), 3072
    ws_bytes = lib.cgs_v7_ws_bytes(M, N, K)
    assert ws_bytes > 0 and _in_domain(GEMM_KERNELS["v7ppk"], M, N, K)
    ws = torch.full((ws_bytes,), 0x7F, dtype=torch.uint8, device=cuda)
    nout = N // 2 if geglu else N
    out = torch.empty(M, nout, device=cuda, dtype=BF)
    epi = core.EPI_BIAS | (core.EPI_GEGLU if geglu else 0)
    inter = core.geglu_interleave if geglu else (lambda t: t)
    if ln:
        torch.manual_seed(2)
        x = (torch.randn(M, K, device=cuda) * 3 + 1.5).to(BF)
        gamma = (torch.rand(K, device=cuda) + 0.5).to(BF)
        beta = (torch.randn(K, device=cuda) * 0.2).to(BF)
        w = (torch.randn(N, K, device=cuda) / math.sqrt(K)).to(BF)
        # (mean, rstd) rows from torch: the statistics kernel stops at C = 2048, and a tail only splits above that
        rs = torch.stack([x.float().mean(1), torch.rsqrt(x.float().var(1, unbiased=False) + 1e-5)], 1).contiguous()
        w2, cs, b2 = ops.lnfold_weights(w, torch.randn(N, device=cuda).to(BF), gamma, beta)
        wk, ck, bk = inter(w2), inter(cs), inter(b2)
        assert lib.cgs_gemm_bf16_lnfold_v(x.data_ptr(), wk.data_ptr(), out.data_ptr(), bk.data_ptr(), rs.data_ptr(),
                                          ck.data_ptr(), M, N, K, K, K, nout, epi, ws.data_ptr(), ws_bytes, 7,
                                          core._stream()) == 0
        ref, tol = lnfold_bound(x, w2, b2, rs, cs, geglu=geglu)
    else:
        a, w, b, _ = _operands(cuda, M, N, K, "bias")
        assert lib.cgs_gemm_bf16_v7ws(a.data_ptr(), inter(w).data_ptr(), out.data_ptr(), inter(b).data_ptr(), None, M,
                                      N, K, K, K, nout, 0, epi, 1.0, ws.data_ptr(), ws_bytes, core._stream()) == 0
        ref, tol = geglu_bound(a, w, b)
    assert_within(out, ref, tol, f"{'lnfold' if ln else 'geglu'}/v7ppk split tail {M}x{N}x{K} {form}")


# ------------------------------------------------------------------------------------------------ conv
# conv_shape_ok / conv_launch / conv_variant_ok (csrc/kernels/conv.hip): Cout <= 16 runs the narrow-output kernel
# whatever the variant (2 excepted when Cin % 64 == 0); variant 2 needs Cin % 64; 3 / 4 / 8 take Cin % 32 and
# Cout % 8, > 16; 5 adds Cin % 64 (and C1 % 64 with two sources); 6 / 7 add kh kw Cin >= 128; 18 adds Cout % 128;
# 21 Cout % 80. A forced variant outside its domain runs the 8-wave v3 tile (conv_v3_launch).
# Case: (N, C1, C2, H, W, Cout, k, stride, pad, upsample2x). ops.conv2d reads x2 in the kernel only with
# C1 % 64 == C2 % 64 == 0 and Cout % 8 == 0; every dual case here has that.
def _conv_shapes(cin, cin_k1, cout):
    return [(3, cin, 0, 5, 7, cout, 3, 1, 1, False), (2, cin, 0, 9, 8, cout, 3, 1, 1, False),
            (3, cin, 0, 5, 7, cout, 3, 2, 1, False), (3, cin_k1, 0, 9, 8, cout, 1, 1, 0, False),
            (2, cin, 0, 5, 7, cout, 3, 1, 1, True), (3, 128, 64, 5, 7, cout, 3, 1, 1, False)]


CONV_CASES = (
    [("narrow", -1) + sh for c in (3, 4, 8) for sh in _conv_shapes(32, 96, c) if sh[2] == 0 or c == 8]
    + [("cv2", 2) + sh for c in (4, 24) for sh in _conv_shapes(64, 64, c) if sh[2] == 0 or c == 24]
    + [(n, v) + sh for n, v in (("cv3w4", 3), ("cv3w8", 4), ("cv8t128", 8)) for sh in _conv_shapes(96, 32, 24)]
    + [("cv5pp", 5) + sh for sh in _conv_shapes(64, 64, 24)]
    + [(n, v) + sh for n, v in (("cv6pp160", 6), ("cv7ppk", 7)) for sh in _conv_shapes(64, 128, 24)]
    + [("cv6n128", 18) + sh for sh in _conv_shapes(64, 128, 128)]
    + [("cv6w4", 21) + sh for sh in _conv_shapes(64, 128, 80)])


def _conv_in_domain(variant, C1, C2, Cout, k):
    cin = C1 + C2
    if variant == -1:
        return Cout <= 16 and cin % 32 == 0
    ok = cin % 32 == 0 and (Cout > 16 or variant == 2) and (C2 == 0 or (C1 % 64 == 0 and C2 % 64 == 0 and Cout % 8 == 0))
    if variant == 2:
        return ok and cin % 64 == 0
    ok = ok and Cout % 8 == 0
    if variant in (5, 6, 7, 18, 21):
        ok = ok and cin % 64 == 0 and (C2 == 0 or C1 % 64 == 0)
    if variant in (6, 7, 18, 21):
        ok = ok and k * k * cin >= 128
    return ok and (variant != 18 or Cout % 128 == 0) and (variant != 21 or Cout % 80 == 0)


@pytest.mark.parametrize("epi", ["bias", "bias_res"])
@pytest.mark.parametrize("name,variant,N,C1,C2,H,W,Cout,k,s,p,up", CONV_CASES)
def test_conv_bound(cuda, name, variant, N, C1, C2, H, W, Cout, k, s, p, up, epi):
    assert _conv_in_domain(variant, C1, C2, Cout, k), (name, C1, C2, Cout, k)
    lib = _native.load_kernels()
    torch.manual_seed(0)
    nhwc = lambda t: t.to(BF).contiguous(memory_format=torch.channels_last)
    x = nhwc(torch.randn(N, C1, H, W, device=cuda) + 0.5)
    x2 = nhwc(torch.randn(N, C2, H, W, device=cuda) + 0.5) if C2 else None
    K = (C1 + C2) * k * k
    w = (torch.randn(Cout, C1 + C2, k, k, device=cuda) / math.sqrt(K)).to(BF)
    b = torch.randn(Cout, device=cuda).to(BF)
    ref, tol = conv_bound(x, w, b, None, s, p, upsample2x=up, x2=x2)
    r = None
    if epi == "bias_res":
        r = nhwc(torch.randn(ref.shape, device=cuda))
        ref, tol = conv_bound(x, w, b, r, s, p, upsample2x=up, x2=x2)
    lib.cgs_conv_set_variant(variant)
    try:
        y = ops.conv2d(x, w, b, s, p, residual=r, weight_nhwc=w.permute(0, 2, 3, 1).contiguous(), upsample2x=up, x2=x2)
    finally:
        lib.cgs_conv_set_variant(-1)
    st = ops.stats()
    assert st.get(("conv", "hip"), 0) == 1 and not any(key[1] == "lib" for key in st), st
    assert_within(y, ref, tol, f"conv/{name} {N}x{C1}+{C2}x{H}x{W}->{Cout} k{k}s{s} up={up} {epi}")


@pytest.mark.parametrize("variant,Cin,k,p", [(5, 96, 3, 1), (6, 64, 1, 0), (7, 64, 1, 0), (18, 64, 3, 1), (21, 64, 3, 1)])
def test_conv_bound_variant_fallback(cuda, variant, Cin, k, p):
    """A forced variant outside its domain (conv_variant_ok: Cin % 64; K = 64 < 128 twice; Cout % 128; Cout % 80) runs
    the 8-wave v3 tile, whose domain every case lies in, and stays inside conv_bound."""
    lib = _native.load_kernels()
    N, H, W, Cout = 3, 5, 7, 24
    assert not _conv_in_domain(variant, Cin, 0, Cout, k) and _conv_in_domain(4, Cin, 0, Cout, k)
    nhwc = lambda t: t.to(BF).contiguous(memory_format=torch.channels_last)
    torch.manual_seed(0)
    x = nhwc(torch.randn(N, Cin, H, W, device=cuda) + 0.5)
    w = (torch.randn(Cout, Cin, k, k, device=cuda) / math.sqrt(Cin * k * k)).to(BF)
    b = torch.randn(Cout, device=cuda).to(BF)
    r = nhwc(torch.randn(N, Cout, H, W, device=cuda))
    ref, tol = conv_bound(x, w, b, r, 1, p)
    lib.cgs_conv_set_variant(variant)
    try:
        y = ops.conv2d(x, w, b, 1, p, residual=r, weight_nhwc=w.permute(0, 2, 3, 1).contiguous())
    finally:
        lib.cgs_conv_set_variant(-1)
    st = ops.stats()
    assert st.get(("conv", "hip"), 0) == 1 and not any(key[1] == "lib" for key in st), st
    assert_within(y, ref, tol, f"conv/variant {variant} out of domain {N}x{Cin}x{H}x{W}->{Cout} k{k}")


class _RefusedConv:
    """Operands of one conv call that an entry must refuse: real tensors of the next legal shape (channel counts up to
    a multiple of 64, 24 output channels), so even a launch would stay inside them; ``out`` holds a sentinel."""

    def __init__(self, cuda, Cin, Cout, C1=None, k=3, HW=(5, 7)):
        up64 = lambda c: (c + 63) // 64 * 64
        nhwc = lambda *s: torch.zeros(s, device=cuda, dtype=BF).contiguous(memory_format=torch.channels_last)
        H, W = HW
        self.x = nhwc(1, up64(Cin if C1 is None else C1), H, W)
        self.x2 = None if C1 is None else nhwc(1, up64(Cin - C1), H, W)
        self.w = torch.zeros(24, k, k, up64(Cin), device=cuda, dtype=BF)
        self.b = torch.zeros(24, device=cuda, dtype=BF)
        self.r = nhwc(1, 24, H, W)
        self.out = nhwc(1, 24, H, W).fill_(7.0)
        self.gnp = torch.zeros(1 * (H * W + 63) // 64 * 24 * 2, device=cuda, dtype=torch.float32)
        self.shape = (1, H, W, Cin, Cout, k, k, 1, k // 2, H, W)
        self.C1 = Cin if C1 is None else C1

    def dual(self):      # the operands of the entries that take x2, up to and including flags
        return (self.x.data_ptr(), _ptr(self.x2), self.C1, self.w.data_ptr(), self.b.data_ptr(), self.r.data_ptr(),
                self.out.data_ptr()) + self.shape + (0,)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.out == 7.0).all())


def test_conv_entries_refuse_same_forms(cuda):
    """conv_shape_ok: the four general entries return hipErrorInvalidValue for the same shapes and launch nothing.
    cgs_conv2d_nhwc_gns refuses what it adds to the v6 domain."""
    lib = _native.load_kernels()
    s = core._stream()
    entries = {"ex": lambda o: lib.cgs_conv2d_nhwc_ex(*o.dual(), s),
               "v": lambda o: lib.cgs_conv2d_nhwc_v(*o.dual(), -2, s),
               "v7ws": lambda o: lib.cgs_conv2d_nhwc_v7ws(*o.dual(), None, 0, s),
               "nhwc": lambda o: lib.cgs_conv2d_nhwc(o.x.data_ptr(), o.w.data_ptr(), o.b.data_ptr(), o.r.data_ptr(),
                                                     o.out.data_ptr(), *o.shape, s)}
    single = [dict(Cin=48, Cout=24), dict(Cin=64, Cout=0), dict(Cin=96, Cout=20)]
    dual = [dict(Cin=96, Cout=24, C1=48), dict(Cin=128, Cout=20, C1=32)]
    lib.cgs_conv_set_variant(-1)
    try:
        for name, call in entries.items():
            for form in single + (dual if name != "nhwc" else []):
                o = _RefusedConv(cuda, **form)
                assert call(o) == 1, (name, form)
                assert o.untouched(), (name, form)
        gns = lambda o, gnp: lib.cgs_conv2d_nhwc_gns(*o.dual(), gnp, s)
        for form, with_gnp in [(dict(Cin=64, HW=(16, 16)), False), (dict(Cin=96, HW=(16, 16)), True),
                               (dict(Cin=64, k=1, HW=(16, 16)), True), (dict(Cin=64, HW=(5, 7)), True)]:
            o = _RefusedConv(cuda, Cout=24, **form)
            assert gns(o, o.gnp.data_ptr() if with_gnp else None) == 1, ("gns", form, with_gnp)
            assert o.untouched(), ("gns", form)
    finally:
        lib.cgs_conv_set_variant(-1)


@pytest.mark.parametrize("C1,C2,s,up", [(320, 0, 1, False), (320, 0, 2, False), (320, 0, 1, True), (256, 64, 1, False)])
def test_conv_bound_v7_split_tail(cuda, C1, C2, s, up):
    """cgs_conv2d_nhwc_v7ws on small images whose only tile is a tail tile that splits over K = 9 * 320."""
    lib = _native.load_kernels()
    N, H, W, Cout, k, p = 3, 5, 7, 24, 3, 1
    Cin = C1 + C2
    assert _conv_in_domain(7, C1, C2, Cout, k)
    nhwc = lambda t: t.to(BF).contiguous(memory_format=torch.channels_last)
    torch.manual_seed(0)
    x = nhwc(torch.randn(N, C1, H, W, device=cuda) + 0.5)
    x2 = nhwc(torch.randn(N, C2, H, W, device=cuda) + 0.5) if C2 else None
    w = (torch.randn(Cout, Cin, k, k, device=cuda) / math.sqrt(Cin * k * k)).to(BF)
    b = torch.randn(Cout, device=cuda).to(BF)
    ref, _ = conv_bound(x, w, b, None, s, p, upsample2x=up, x2=x2)
    r = nhwc(torch.randn(ref.shape, device=cuda))
    ref, tol = conv_bound(x, w, b, r, s, p, upsample2x=up, x2=x2)
    Ho, Wo = ref.shape[2], ref.shape[3]
    ws_bytes = lib.cgs_v7_ws_bytes(N * Ho * Wo, Cout, k * k * Cin)
    assert ws_bytes > 0, "shape chosen to take the split tail"
    ws = torch.full((ws_bytes,), 0x7F, dtype=torch.uint8, device=cuda)
    wn = w.permute(0, 2, 3, 1).contiguous()
    y = torch.empty(ref.shape, device=cuda, dtype=BF).contiguous(memory_format=torch.channels_last)
    assert lib.cgs_conv2d_nhwc_v7ws(x.data_ptr(), _ptr(x2), C1, wn.data_ptr(), b.data_ptr(), r.data_ptr(), y.data_ptr(),
                                    N, H, W, Cin, Cout, k, k, s, p, Ho, Wo, 16 if up else 0, ws.data_ptr(), ws_bytes,
                                    core._stream()) == 0
    assert_within(y, ref, tol, f"conv/cv7ppk split tail {N}x{C1}+{C2}x{H}x{W}->{Cout} k{k}s{s} up={up}")


# ------------------------------------------------------------------------------------------------ attention
# flash_attn_dispatch (csrc/kernels/attention.hip): variant 1 = the generic kernel (every head dim, causal, key mask);
# 2 / 4 = the D = 64 kernel on 256-row query blocks, 5 on 128-row blocks, 3 = the short-KV kernel (D = 64,
# Sk <= 128); 2 .. 5 take neither mask. D = 512 has its own kernel whatever the variant.
SQS, SKS = (1, 63, 129, 257), (1, 4, 63, 65, 130)
D64_VARIANTS = {1: "generic", 2: "d64fast", 3: "shortkv", 4: "d64r2", 5: "d64q128"}


def _qkv(cuda, B, H, Sq, Sk, D, seed, spike=False):
    torch.manual_seed(seed)
    q = torch.randn(B, Sq, H * D, device=cuda)
    k = torch.randn(B, Sk, H * D, device=cuda)
    v = torch.randn(B, Sk, H * D, device=cuda)
    if spike:                                   # late keys that force running-max rescales mid-sequence
        q *= 3.0
        for j in range(Sk // 3, Sk, max(1, Sk // 5)):
            k[:, j, :] *= 1.0 + 0.5 * (j * 7 % 11)
    return q.to(BF), k.to(BF), v.to(BF)


@pytest.fixture
def attn_variant(request):
    lib = _native.load_kernels()
    lib.cgs_attn_set_variant(request.param)
    yield request.param
    lib.cgs_attn_set_variant(0)


def _attn(q, k, v, H, **kw):
    ops.reset_stats()
    o = ops.attention(q, k, v, H, **kw)
    st = ops.stats()
    assert st.get(("attention", "hip"), 0) == 1 and not any(key[1] == "lib" for key in st), st
    return o


@pytest.mark.parametrize("attn_variant", [1], indirect=True)
@pytest.mark.parametrize("D", list(core._FLASH_HEAD_DIMS))
def test_attention_bound_head_dims(cuda, attn_variant, D):
    for Sq in SQS:
        for Sk in SKS:
            q, k, v = _qkv(cuda, 2, 3, Sq, Sk, D, seed=Sq * 1000 + Sk)
            ref, tol = attention_bound(q, k, v, 3)
            assert_within(_attn(q, k, v, 3), ref, tol, f"attention/generic D={D} Sq={Sq} Sk={Sk}")


def test_attention_bound_d512(cuda):
    for Sq in SQS:
        for Sk in SKS:
            q, k, v = _qkv(cuda, 2, 1, Sq, Sk, 512, seed=Sq * 1000 + Sk)
            ref, tol = attention_bound(q, k, v, 1)
            assert_within(_attn(q, k, v, 1), ref, tol, f"attention/wide D=512 Sq={Sq} Sk={Sk}")


@pytest.mark.parametrize("spike", [False, True])
@pytest.mark.parametrize("attn_variant", list(D64_VARIANTS), indirect=True)
def test_attention_bound_d64_variants(cuda, attn_variant, spike):
    name = D64_VARIANTS[attn_variant]
    for Sq in SQS:
        for Sk in (s for s in SKS if attn_variant != 3 or s <= 128):
            q, k, v = _qkv(cuda, 2, 3, Sq, Sk, 64, seed=Sq * 1000 + Sk, spike=spike)
            ref, tol = attention_bound(q, k, v, 3)
            assert_within(_attn(q, k, v, 3), ref, tol, f"attention/{name} Sq={Sq} Sk={Sk} spike={spike}")


@pytest.mark.parametrize("attn_variant", list(D64_VARIANTS), indirect=True)
def test_attention_bound_strided_qkv(cuda, attn_variant):
    """q, k, v as column views of one fused QKV buffer (row stride 3 C)."""
    H, D = 5, 64
    C = H * D
    for S in (65, 129) if attn_variant == 3 else (65, 130, 257):
        torch.manual_seed(S)
        qkv = torch.randn(2, S, 3 * C, device=cuda).to(BF)
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        if attn_variant == 3 and S > 128:
            k, v = k[:, :63], v[:, :63]
        before = qkv.clone()
        ref, tol = attention_bound(q, k, v, H)
        assert_within(_attn(q, k, v, H), ref, tol, f"attention/{D64_VARIANTS[attn_variant]} fused QKV S={S}")
        assert torch.equal(qkv, before)


@pytest.mark.parametrize("attn_variant", [0, 1], indirect=True)
@pytest.mark.parametrize("D", [40, 64])
def test_attention_bound_causal_and_key_padding(cuda, attn_variant, D):
    H = 3
    for S in (1, 63, 77, 130):
        q, k, v = _qkv(cuda, 3, H, S, S, D, seed=S)
        ref, tol = attention_bound(q, k, v, H, causal=True)
        assert_within(_attn(q, k, v, H, causal=True), ref, tol, f"attention/generic causal D={D} S={S}")
    for Sq, Sk in ((1, 4), (63, 65), (129, 130), (257, 63)):
        q, k, v = _qkv(cuda, 3, H, Sq, Sk, D, seed=Sq + Sk)
        valid = torch.tensor([1, max(1, Sk // 2), Sk], device=cuda)           # ragged; every row keeps a key
        kp = torch.arange(Sk, device=cuda)[None, :] < valid[:, None]
        ref, tol = attention_bound(q, k, v, H, key_padding=kp)
        assert_within(_attn(q, k, v, H, key_padding=kp), ref, tol,
                      f"attention/generic key_padding D={D} Sq={Sq} Sk={Sk}")


def _padded(t, rows, cols):
    """t [B, S, C] as the corner view of a [B, S + rows, C + cols] buffer: its own batch and row stride."""
    B, S, C = t.shape
    buf = torch.zeros(B, S + rows, C + cols, device=t.device, dtype=t.dtype)
    buf[:, :S, :C] = t
    return buf[:, :S, :C]


def _distinct_mult8(strides):
    return len(set(strides)) == len(strides) and all(s % 8 == 0 for s in strides)


def _bshd_strides(*ts):
    """(batch, token, head) element strides of [B, S, H, D] views, in the order the library entries take them."""
    return [t.stride(i) for t in ts for i in (0, 1, 2)]


def _stride_views(cuda, B, H, Sq, Sk, D, seed):
    """q, k, v, o as [B, S, H, D] views of four differently padded buffers, and o's buffer. q: token-major in
    [B, Sq + 1, H D + 8]; k: head-major in [B, H, Sk + 2, D + 8]; v: token-major in [B, Sk + 3, H (D + 24)] (the
    24 elements of padding per head, not per row: with them at the end of the row v's head stride would be D like
    q's, and two equal strides can be swapped unseen); o: head-major in [B, H, Sq + 1, D + 16], filled with SENTINEL."""
    torch.manual_seed(seed)
    q = torch.randn(B, Sq + 1, H * D + 8, device=cuda).to(BF)[:, :Sq, :H * D].unflatten(2, (H, D))
    k = torch.randn(B, H, Sk + 2, D + 8, device=cuda).to(BF)[:, :, :Sk, :D].transpose(1, 2)
    v = torch.randn(B, Sk + 3, H, D + 24, device=cuda).to(BF)[:, :Sk, :, :D]
    ob = torch.full((B, H, Sq + 1, D + 16), SENTINEL, device=cuda, dtype=BF)
    return q, k, v, ob[:, :, :Sq, :D].transpose(1, 2), ob


SENTINEL = -8192.0


def _flash(lib, entry, q, k, v, o, *tail, lse=None):
    """cgs_flash_attn_fwd (tail: key_mask, causal), _v (tail: variant) or _lse on [B, S, H, D] views."""
    B, Sq, H, D = q.shape
    args = [q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()] + ([] if lse is None else [lse.data_ptr()])
    args += [B, H, Sq, k.shape[1], D] + _bshd_strides(q, k, v, o) + [1.0 / math.sqrt(D)] + list(tail)
    return getattr(lib, entry)(*args, core._stream())


def _stride_cases():
    cases = [("v1", 3, D, Sq, Sk) for D in (40, 64) for Sq, Sk in ((63, 65), (257, 130))]     # generic kernel
    cases += [(f"v{var}", 3, 64, Sq, Sk) for var in (2, 5) for Sq, Sk in ((63, 65), (257, 130))]
    cases += [("v3", 3, 64, Sq, Sk) for Sq, Sk in ((129, 63), (257, 128))]                    # short-KV
    cases += [("wide", 2, 512, Sq, Sk) for Sq, Sk in ((63, 65), (33, 130))]
    cases += [("lse", 3, D, 257, 130) for D in (64, 40)]                                      # fast / generic kernel
    return cases


@pytest.mark.parametrize("form,H,D,Sq,Sk", _stride_cases())
def test_attention_bound_distinct_strides(cuda, form, H, D, Sq, Sk):
    """The library called directly with twelve pairwise distinct strides (every other attention case gives q, k and
    v the same row and batch strides, head stride D and a contiguous output): a launcher that swaps two of them
    misses the bound or writes outside o's view."""
    lib = _native.load_kernels()
    B = 2
    q, k, v, o, ob = _stride_views(cuda, B, H, Sq, Sk, D, seed=Sq * 1000 + Sk + D)
    strides = _bshd_strides(q, k, v, o)
    assert _distinct_mult8(strides), strides
    lse = torch.empty(B, H, Sq, device=cuda, dtype=torch.float32) if form == "lse" else None
    if form == "lse":
        rc = _flash(lib, "cgs_flash_attn_fwd_lse", q, k, v, o, lse=lse)
    elif form == "wide":
        rc = _flash(lib, "cgs_flash_attn_fwd", q, k, v, o, None, 0)
    else:
        rc = _flash(lib, "cgs_flash_attn_fwd_v", q, k, v, o, int(form[1]))
    assert rc == 0
    qc, kc, vc = (t.reshape(B, t.shape[1], H * D) for t in (q, k, v))                       # contiguous copies
    ref, tol = attention_bound(qc, kc, vc, H)
    assert_within(o.reshape(B, Sq, H * D), ref, tol, f"attention/{form} distinct strides D={D} Sq={Sq} Sk={Sk}")
    outside = torch.ones_like(ob, dtype=torch.bool)
    outside[:, :, :Sq, :D] = False
    assert bool((ob[outside] == SENTINEL).all())
    if form == "lse":
        s = (qc.float().view(B, Sq, H, D).transpose(1, 2) @ kc.float().view(B, Sk, H, D).permute(0, 2, 3, 1)) * D ** -0.5
        assert (lse - torch.logsumexp(s, -1)).abs().max().item() < 2e-2


def test_attention_variant_call_leaves_process_setting(cuda):
    """cgs_flash_attn_fwd_v picks its kernel per call: it neither reads nor changes the cgs_attn_set_variant
    setting (one thread; the generic and the D = 64 kernel do not round alike, so a leaked variant shows)."""
    lib = _native.load_kernels()
    B, H, Sq, Sk, D = 2, 3, 257, 130, 64
    q, k, v = (t.unflatten(2, (H, D)) for t in _qkv(cuda, B, H, Sq, Sk, D, seed=5))
    o1, ov, o2 = (torch.empty_like(q) for _ in range(3))
    lib.cgs_attn_set_variant(1)
    try:
        assert _flash(lib, "cgs_flash_attn_fwd", q, k, v, o1, None, 0) == 0
        assert _flash(lib, "cgs_flash_attn_fwd_v", q, k, v, ov, 2) == 0
        assert _flash(lib, "cgs_flash_attn_fwd", q, k, v, o2, None, 0) == 0
    finally:
        lib.cgs_attn_set_variant(0)
    assert torch.equal(o1, o2)
    ref, tol = attention_bound(q.flatten(2), k.flatten(2), v.flatten(2), H)
    assert_within(ov.flatten(2), ref, tol, "attention/d64fast per call under process variant 1")


@pytest.mark.parametrize("rows", [128, 256])
def test_attention_bound_kv2(cuda, rows, monkeypatch):
    lib = _native.load_kernels()
    real = lib.cgs_flash_attn_fwd_kv2
    H, C = 3, 3 * 64
    lib.cgs_attn_set_kv2_rows(rows)
    try:
        for Sq, S2 in ((1, 1), (63, 4), (129, 65), (257, 130)):
            torch.manual_seed(Sq)
            # q and the four sources each in a padded buffer of its own: ten different strides
            q, k1, v1 = (_padded(torch.randn(2, Sq, C, device=cuda).to(BF), i, 8 * i) for i in (1, 2, 3))
            k2, v2 = (_padded(torch.randn(2, S2, C, device=cuda).to(BF), i, 8 * i) for i in (4, 5))
            assert _distinct_mult8([t.stride(i) for t in (q, k1, v1, k2, v2) for i in (0, 1)])
            rcs = []
            with monkeypatch.context() as mp:
                mp.setattr(lib, "cgs_flash_attn_fwd_kv2", lambda *a: rcs.append(real(*a)) or rcs[-1])
                o = ops.attention_kv2(q, k1, v1, k2, v2, H)
            assert rcs == [0]                                   # the two-source kernel ran, not the concat path
            ref, tol = attention_bound(q, torch.cat([k1, k2], 1), torch.cat([v1, v2], 1), H)
            assert_within(o, ref, tol, f"attention/kv2 rows={rows} Sq={Sq} S1={Sq} S2={S2}")
    finally:
        lib.cgs_attn_set_kv2_rows(0)


@pytest.mark.parametrize("ks,Sk", [(2, 449), (4, 961)])
def test_attention_bound_key_split(cuda, ks, Sk):
    """The smallest Sk ops.attention admits for each split: tiles = ceil(Sk / 64) >= 4 ks, last slice not empty.
    The slices' partial outputs are bf16 (ws_o): one more rounding of magnitude u A."""
    lib = _native.load_kernels()
    tiles = (Sk + 63) // 64
    assert tiles == 4 * ks and (ks - 1) * ((tiles + ks - 1) // ks) * 64 < Sk and (Sk - 1 + 63) // 64 < 4 * ks
    B, H, D = 2, 3, 64
    for Sq, spike in ((257, False), (63, True)):
        q, k, v = (_padded(t, i, 8 * i) for i, t in enumerate(_qkv(cuda, B, H, Sq, Sk, D, seed=Sk + Sq, spike=spike), 1))
        o = _padded(torch.empty(B, Sq, H * D, device=cuda, dtype=BF), 4, 32)
        assert _distinct_mult8([t.stride(i) for t in (q, k, v, o) for i in (0, 1)])
        ws_o = torch.empty(ks * B * Sq * H * D, device=cuda, dtype=BF)
        ws_l = torch.empty(ks * B * H * Sq, device=cuda, dtype=torch.float32)
        assert lib.cgs_flash_attn_fwd_ks(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, Sq, Sk,
                                         q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
                                         o.stride(0), o.stride(1), 1.0 / math.sqrt(D), ks, ws_o.data_ptr(),
                                         ws_l.data_ptr(), core._stream()) == 0
        ref, tol = attention_bound(q, k, v, H, extra_roundings=1)
        assert_within(o, ref, tol, f"attention/d64ks{ks} Sq={Sq} Sk={Sk} spike={spike}")
