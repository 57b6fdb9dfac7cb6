"""Launch-trace parity of the GEMM op layer (ops/core.py), no GPU needed.

The real entry functions (``linear``, ``linear_geglu``, ``linear_lnfold``, the fp8 path, ``_attention_wide_mat``)
run on CPU bf16 tensors with the kernel library replaced by a recorder: every exported entry they call is logged
with its full argument list, pointers replaced by role tags (``A``, ``W``, ``bias``, ``R``, ``rs``, ``cs``,
``out=``, ``tmp(shape, dtype)`` for buffers the op allocates, ``A+off`` for an operand plus a byte offset), every
integer and float verbatim. Each shape runs once on the default path and once per autotune candidate that run
offered. Each case's trace is compared with ``tests/golden/gemm_launch_trace.json``, recorded from the commit named
in its ``_meta`` key (``python tests/test_gemm_launch_trace_cpu.py --record`` in a checkout of that commit): the
op layer may be rearranged, the entries it calls and what it passes them may not change. The fixture keeps a
SHA-256 digest of each case's canonical JSON trace, not the trace (1754 traces are 0.7 MB): equal digests are equal
traces; on a mismatch the test prints the trace it got, and ``--dump`` in a checkout of the recorded commit prints
the one it was recorded from.

The variant table check (``GEMM_VARIANTS`` against ``csrc/kernels/gemm_args.h``) lives here too.
"""
import hashlib
import json
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from comfy_gen_server_amd.ops import core, dispatch     # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_launch_trace.json")

SHAPES = [(64, 1280, 1280), (128, 1280, 1280), (300, 1280, 2048), (2048, 1280, 1280), (8192, 640, 640),
          (4096, 1920, 640), (4096, 5120, 640), (16384, 1920, 640), (1152, 2048, 8192), (1152, 2048, 2048),
          (77, 768, 776),      # K % 32 != 0
          (512, 324, 320)]     # N % 8 != 0
SPLITK_SHAPE = (2048, 1280, 1280)      # under-filled: CGS_SPLITK=1 offers the split-K names

# every exported GEMM launcher of the op layer: the grid must reach each of them
ENTRIES = {"cgs_gemm_bf16_v", "cgs_gemm_bf16_v7ws", "cgs_gemm_bf16_rowstats_v", "cgs_gemm_skinny_ws",
           "cgs_gemm_bf16_splitk", "cgs_gemm_bf16_lnfold_v", "cgs_gemm_bf16_gelu_gns", "cgs_gemm_bf16_w8"}

_POINTER = 1 << 40      # host addresses lie above this, every size / stride / flag of the grid far below


class _Tracer:
    """The stub kernel library plus the ``autotune.choose`` and ``torch.empty`` recorders of one case."""

    def __init__(self):
        self.launches, self.chooses, self.allocs, self.operands, self.forced = [], [], [], [], None

    def begin(self, operands, forced):
        self.launches, self.chooses, self.allocs, self.forced = [], [], [], forced
        self.operands = [(name, t.data_ptr(), t.numel() * t.element_size()) for name, t in operands.items()
                         if t is not None]

    def tag(self, v):
        if not isinstance(v, int) or isinstance(v, bool) or v < _POINTER:
            return v
        for name, base, size in self.operands:
            if base <= v < base + size:
                return name if v == base else f"{name}+{v - base}"
        for t in self.allocs:      # (kept alive for the whole case, so no address is handed out twice)
            base = t.data_ptr()
            if base <= v < base + t.numel() * t.element_size():
                name = f"tmp({list(t.shape)}, {str(t.dtype).replace('torch.', '')})"
                return name if v == base else f"{name}+{v - base}"
        return "ptr"

    def __getattr__(self, entry):
        def call(*args):
            self.launches.append([entry] + [self.tag(a) for a in args])
            if entry == "cgs_v7_ws_bytes":
                return 4096 if args[2] % 128 == 0 else 0
            if entry == "cgs_gemm_skinny_ws_bytes":
                return 4096 if args[1] < 4096 else 0
            if entry == "cgs_gemm_w6_ok":
                return int(args[0] % 256 == 0)
            return 0
        return call

    def choose(self, key_parts, candidates, default=None):
        names = [n for n, _ in candidates]
        self.chooses.append(["|".join(str(p) for p in key_parts), names, default])
        if self.forced in names:
            return self.forced
        return names[0] if default is None else default


def _harness(mp):
    tr = _Tracer()
    real_empty = torch.empty

    def empty(*a, **k):
        t = real_empty(*a, **k)
        tr.allocs.append(t)
        return t

    for var in ("CGS_SPLITK", "CGS_SKINNY_SPLIT", "CGS_GRN_GNS"):
        mp.delenv(var, raising=False)
    mp.setattr(core, "backend_for", lambda op, t, kernel=None: "hip")
    mp.setattr(core._native, "has_kernel", lambda name: True)
    mp.setattr(core, "_stream", lambda: 0)
    mp.setattr(core, "_num_cus", lambda: 256)
    mp.setattr(core, "_lib", lambda: tr)
    mp.setattr(core.autotune, "choose", tr.choose)
    mp.setattr(torch, "empty", empty)
    for name, value in (("_LIB_GEMM", False), ("_RSO", True), ("_V7_SPLIT", True), ("_GRN_GNS", True)):
        mp.setattr(core, name, value)
    return tr


def _run(tr, fn, operands, forced):
    core._V7WS.clear()
    core._SKWS.clear()
    before = dispatch.stats()
    tr.begin(operands, forced)
    y = fn()
    after = dispatch.stats()
    out = operands.get("out=")
    res = {"choose": tr.chooses, "launch": tr.launches,
           "result": [list(y.shape), str(y.dtype), bool(out is not None and y.data_ptr() == out.data_ptr())],
           "stats": {f"{k[0]}/{k[1]}": after[k] - before.get(k, 0) for k in sorted(after)
                     if after[k] != before.get(k, 0)}}
    if hasattr(y, "_cgs_rowpart"):
        res["rowpart"] = list(y._cgs_rowpart[0].shape)
    if hasattr(y, "_cgs_grnpart"):
        res["grnpart"] = [list(y._cgs_grnpart[0].shape), y._cgs_grnpart[2]]
    return res


def _forms(M, N, K):
    """(form name, operands by role, call) for one shape; the inputs are made before ``torch.empty`` is wrapped."""
    bf = torch.bfloat16
    x, w, b = torch.zeros(M, K, dtype=bf), torch.zeros(N, K, dtype=bf), torch.zeros(N, dtype=bf)
    r, o = torch.zeros(M, N, dtype=bf), torch.zeros(M, N, dtype=bf)
    xs = torch.zeros(M, K + 8, dtype=bf)[:, :K]                 # row-strided view: stride(0) > K, multiple of 8
    rt = torch.zeros(N, M, dtype=bf).t()                        # non-contiguous residual
    w8 = w.to(torch.float8_e4m3fn)
    rs, cs = torch.zeros(M, 2), torch.zeros(N)
    lin, geglu, lnf = core.linear, core.linear_geglu, core.linear_lnfold
    A, W = {"A": x}, {"W": w}
    forms = [
        ("linear", {**A, **W}, lambda: lin(x, w)),
        ("linear+bias", {**A, **W, "bias": b}, lambda: lin(x, w, b)),
        ("linear+bias+res", {**A, **W, "bias": b, "R": r}, lambda: lin(x, w, b, residual=r)),
        ("linear+gelu", {**A, **W, "bias": b}, lambda: lin(x, w, b, act="gelu")),
        ("linear+silu", {**A, **W, "bias": b}, lambda: lin(x, w, b, act="silu")),
        ("linear+out", {**A, **W, "bias": b, "out=": o}, lambda: lin(x, w, b, out=o)),
        ("linear+rowstats", {**A, **W, "bias": b, "R": r}, lambda: lin(x, w, b, residual=r, row_stats=True)),
        ("linear+strided", {"A": xs, **W, "bias": b}, lambda: lin(xs, w, b)),
        ("linear+res_noncontig", {**A, **W, "bias": b, "R": rt}, lambda: lin(x, w, b, residual=rt)),
        ("linear+fp8", {**A, "W": w8, "bias": b, "R": r}, lambda: lin(x, w8, b, residual=r)),
        ("linear+fp8+gelu", {**A, "W": w8, "bias": b}, lambda: lin(x, w8, b, act="gelu")),
        ("geglu", {**A, **W}, lambda: geglu(x, w, None)),
        ("geglu+bias", {**A, **W, "bias": b}, lambda: geglu(x, w, b)),
    ]
    L = {**A, **W, "bias": b, "rs": rs, "cs": cs}
    forms += [
        ("lnfold", L, lambda: lnf(x, rs, w, cs, b)),
        ("lnfold+geglu", L, lambda: lnf(x, rs, w, cs, b, geglu=True)),
        ("lnfold+gelu+gns", L, lambda: lnf(x, rs, w, cs, b, act="gelu", gns_hw=64)),
        ("lnfold+gelu", L, lambda: lnf(x, rs, w, cs, b, act="gelu")),
    ]
    return forms


def _with_forced(tr, out, prefix, operands, fn):
    """The default path, then once per candidate name that run's ``choose`` calls offered."""
    base = _run(tr, fn, operands, None)
    out[f"{prefix}/default"] = base
    names = []
    for _, offered, _ in base["choose"]:
        names += [n for n in offered if n not in names]
    for n in names:
        out[f"{prefix}/{n}"] = _run(tr, fn, operands, n)


def collect():
    """case id -> trace, for the whole grid (JSON-normalised: tuples as lists)."""
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        tr = _harness(mp)
        for M, N, K in SHAPES:
            for form, operands, fn in _forms(M, N, K):
                _with_forced(tr, out, f"{form}/{M}x{N}x{K}", operands, fn)
        mp.setenv("CGS_SPLITK", "1")
        M, N, K = SPLITK_SHAPE
        for form, operands, fn in _forms(M, N, K):
            if form in ("linear+bias", "linear+bias+res", "linear+gelu", "lnfold"):
                _with_forced(tr, out, f"splitk:{form}/{M}x{N}x{K}", operands, fn)
        mp.delenv("CGS_SPLITK")
        mp.setattr(core, "_WIDE_CHUNK_ELEMS", 256 * 300)       # 256-row chunks of Sq = 300: two per image
        q, k, v = (torch.zeros(2, 300, 512, dtype=torch.bfloat16) for _ in range(3))
        out["wide_attention/2x300x512"] = _run(tr, lambda: core._attention_wide_mat(q, k, v),
                                               {"q": q, "k": k, "v": v}, None)
    return json.loads(json.dumps(out))


def _digest(trace):
    return hashlib.sha256(json.dumps(trace, sort_keys=True, separators=(",", ":")).encode()).hexdigest()[:10]


def _entries(traces):
    """The exported GEMM launchers (not the workspace / domain queries) the traces call."""
    seen = {launch[0] for t in traces.values() for launch in t["launch"]}
    return sorted(e for e in seen if e.startswith("cgs_gemm_") and not e.endswith(("_ws_bytes", "_w6_ok")))


def _grouped(traces):
    """"form/shape/forced name" -> trace as {"form/shape": {forced name: digest}} (the fixture's layout)."""
    out = {}
    for case_id, trace in traces.items():
        group, name = case_id.rsplit("/", 1)
        out.setdefault(group, {})[name] = _digest(trace)
    return out


_cache = {}


def _traces():
    if not _cache:
        with open(FIXTURE) as f:
            want = json.load(f)
        _cache.update(want=want, got=collect())
    return _cache["want"], _cache["got"]


_FORM_NAMES = [f for f, _, _ in _forms(8, 8, 8)]
_ALL_FORMS = _FORM_NAMES + ["splitk:linear+bias", "splitk:linear+bias+res", "splitk:linear+gelu", "splitk:lnfold",
                            "wide_attention"]


@pytest.mark.parametrize("form", _ALL_FORMS)
def test_launch_trace_matches_recorded(form):
    want, traces = _traces()
    want = {g: v for g, v in want["cases"].items() if g.split("/")[0] == form}
    got = {g: v for g, v in _grouped(traces).items() if g.split("/")[0] == form}
    assert want, form
    assert sorted(got) == sorted(want)
    for group in sorted(want):
        assert sorted(got[group]) == sorted(want[group]), group
        for name, digest in want[group].items():
            assert got[group][name] == digest, (f"{group}/{name}", traces[f"{group}/{name}"])


def test_fixture_covers_every_form_and_entry():
    want, traces = _traces()
    assert re.fullmatch(r"[0-9a-f]{7,40}", want["_meta"]["recorded_from"])
    cases = want["cases"]
    assert {g.split("/")[0] for g in cases} == set(_ALL_FORMS)
    assert set(want["_meta"]["entries"]) == ENTRIES == set(_entries(traces))
    for M, N, K in SHAPES:
        assert "default" in cases[f"linear/{M}x{N}x{K}"] and "default" in cases[f"lnfold/{M}x{N}x{K}"]
    assert sum(len(v) - 1 for v in cases.values()) > 100      # forced choices


def test_gemm_variants_match_header():
    """Every number of ``GEMM_VARIANTS`` is a ``GemmVariant`` enumerator; v10..v14 are the small-tile range besides 8."""
    src = open(os.path.join(ROOT, "comfy_gen_server_amd", "csrc", "kernels", "gemm_args.h")).read()
    enum = {name: int(n) for name, n in re.findall(r"\bkVariant(\w+)\s*=\s*(-?\d+)", src)}
    assert len(enum) >= 18
    assert set(core.GEMM_VARIANTS.values()) <= set(enum.values())
    assert len(set(core.GEMM_VARIANTS.values())) == len(core.GEMM_VARIANTS)
    m = re.search(r"small_tile_variant\(int v\)\s*\{\s*return v == kVariant(\w+) \|\| "
                  r"\(v >= kVariant(\w+) && v <= kVariant(\w+)\);", src)
    assert m, "small_tile_variant rule not found"
    assert enum[m.group(1)] == core.GEMM_VARIANTS["v8"] == 8
    small = set(range(enum[m.group(2)], enum[m.group(3)] + 1))
    assert small == {core.GEMM_VARIANTS[f"v{v}"] for v in range(10, 15)} == set(core._SMALL_NAMES.values())
    assert set(core._SMALL_NAMES) == {f"v{v}" for v in range(10, 15)}
    assert (core.W6, core.W6_160, core.V6_M128, core.V6_W4) == tuple(
        core.GEMM_VARIANTS[n] for n in ("w6", "w6n160", "v6m128", "v6w4"))
    assert (enum["W6"], enum["W6n160"], enum["V6m128"], enum["V6w4"]) == (core.W6, core.W6_160, core.V6_M128,
                                                                             core.V6_W4)
    for name in ("v4", "v5", "v6", "v7", "v8"):
        assert enum[name.upper()] == core.GEMM_VARIANTS[name]


if __name__ == "__main__":
    import subprocess
    if sys.argv[1:] not in (["--record"], ["--dump"]):
        sys.exit("usage: test_gemm_launch_trace_cpu.py --record | --dump   (in a clean checkout of the commit to record)")
    traces = collect()
    if sys.argv[1] == "--dump":       # the full traces, one case per line (to diff two checkouts)
        for case_id in sorted(traces):
            print(case_id, json.dumps(traces[case_id], sort_keys=True))
        sys.exit(0)
    commit = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    meta = {"recorded_from": commit, "entries": _entries(traces),
            "how": "python tests/test_gemm_launch_trace_cpu.py --record, in a checkout of that commit"}
    body = ",\n".join(f"{json.dumps(g)}: {json.dumps(v, sort_keys=True)}" for g, v in sorted(_grouped(traces).items()))
    with open(FIXTURE, "w") as f:      # one "form/shape" group per line
        f.write('{"_meta": %s,\n"cases": {\n%s\n}}\n' % (json.dumps(meta, sort_keys=True), body))
    print(f"{len(traces)} cases -> {FIXTURE} ({os.path.getsize(FIXTURE)} bytes)")
