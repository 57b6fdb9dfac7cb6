"""Shared harness of the reference-parity tests (test_reference_parity*.py).

Each case is a script run in a subprocess. Everything the reference implementation contributes -- its outputs,
and the weights it initialises itself -- goes through ``ref_t`` / ``ref_sd`` / ``ref_j``. In a test run these
read the values stored under ``tests/golden/<case>.npz|.json.gz`` and nothing outside the repository is touched.
``oracle/record_golden.py <reference checkout>`` runs the same scripts with ``CGS_REFERENCE_DIR`` set: then the
closures really call the reference's modules (imported read-only, CPU argv) and the fixtures are rewritten.
Only data is stored: tensors, state dicts, names and numbers."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

HEAD = r'''
import gzip, json, os, sys, types
import numpy as np
import torch
REF = os.environ.get("CGS_REFERENCE_DIR")
REC = bool(REF)
if REC:
    sys.path.insert(0, REF); sys.argv = ["x", "--cpu"]
    import comfy.options; comfy.options.enable_args_parsing()
    for _m in ("torchsde", "blake3"):
        sys.modules.setdefault(_m, types.ModuleType(_m))
sys.path.insert(0, ROOT)
from comfy_gen_server_amd.runtime import device as dm
dm.set_cpu_mode(True)
torch.manual_seed(0)
_T, _J = {}, {}
if not REC:
    _i = 0
    while os.path.exists(GOLDEN + (".%d.npz" % _i if _i else ".npz")):
        with np.load(GOLDEN + (".%d.npz" % _i if _i else ".npz")) as _z:
            _T.update({k: _z[k] for k in _z.files})
        _i += 1
    if os.path.exists(GOLDEN + ".json.gz"):
        with gzip.open(GOLDEN + ".json.gz", "rt") as _f:
            _J = json.load(_f)

def ref_t(key, fn):
    """A tensor that the reference (or the recording run's RNG) produced."""
    if REC:
        with torch.no_grad():
            v = fn()
        _T[key] = v.detach().cpu().numpy()
        return v
    return torch.from_numpy(_T[key])

def ref_sd(key, fn):
    """A state dict initialised by the reference."""
    if REC:
        with torch.no_grad():
            sd = fn()
        for k, v in sd.items():
            _T[key + "/" + k] = v.detach().cpu().numpy()
        return sd
    return {k[len(key) + 1:]: torch.from_numpy(v) for k, v in _T.items() if k.startswith(key + "/")}

def ref_j(key, fn):
    """A JSON value (names, numbers, nested lists / dicts with string keys) computed by the reference."""
    if REC:
        _J[key] = fn()
        return json.loads(json.dumps(_J[key]))
    return _J[key]

def save_golden():
    if REC:
        os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
        # committed files stay well below 1 MiB: one <case>.npz if it compresses that far (masks and index
        # tables do), else <case>.npz, <case>.1.npz, ... of at most 800 KiB of raw data each
        shards, size = [{}], 0
        if _T:
            np.savez_compressed(GOLDEN + ".npz", **_T)
        if _T and os.path.getsize(GOLDEN + ".npz") <= 900 * 1024:
            shards = []
        for k, v in _T.items() if shards else ():
            if size + v.nbytes > 800 * 1024 and shards[-1]:
                shards.append({})
                size = 0
            shards[-1][k] = v
            size += v.nbytes + 300
        for i, part in enumerate(shards):
            if part:
                np.savez_compressed(GOLDEN +(".%d.npz" % i if i else ".npz"), **part)
        if _J:
            with open(GOLDEN + ".json.gz", "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as z:
                z.write(json.dumps(_J, sort_keys=True).encode())

def close(a, b, tol=2e-4, what=""):
    assert tuple(a.shape) == tuple(b.shape), (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    assert err <= tol * max(1.0, scale), (what, err, scale)
    return err
'''


def run_case(name, body, timeout=600):
    """Run ``HEAD + body`` for the case ``name``; returns its stdout. The script ends with save_golden()."""
    code = f"ROOT = {ROOT!r}\nGOLDEN = {os.path.join(GOLDEN, name)!r}\n" + HEAD + body + "\nsave_golden()\n"
    env = dict(os.environ, CGS_FORCE_CPU="1", OMP_NUM_THREADS="4", PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout
