#!/usr/bin/env python3
"""Re-record the fixtures of the reference-parity tests (tests/golden/*.npz, *.json).

    python oracle/record_golden.py <path to a checkout of the reference implementation> [case ...]

Runs the very scripts of tests/test_reference_parity*.py with CGS_REFERENCE_DIR set, so that the reference's
modules are imported (read-only, CPU) and their outputs stored; the tests then compare against the stored values
with no reference checkout. Each script still asserts parity while it records. Only data is written."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def cases():
    import test_reference_parity as P
    import test_reference_parity_photomaker as PM
    import test_reference_parity_sampling as PS
    out = {"parity_" + w: P.script(w) for w in P.CASES}
    out.update(PS.CASES)
    out.update(PM.CASES)
    return out


def main(argv):
    if not argv or not os.path.isdir(os.path.join(argv[0], "comfy")):
        sys.exit(__doc__)
    os.environ["CGS_REFERENCE_DIR"] = os.path.abspath(argv[0])
    from _parity import GOLDEN, run_case
    import glob
    todo = cases()
    os.makedirs(GOLDEN, exist_ok=True)
    failed = []
    for name in argv[1:] or sorted(todo) + ["import_surface"]:
        for p in glob.glob(os.path.join(GOLDEN, name + ".*")):
            os.remove(p)
        if name == "import_surface":
            import_surface(argv[0], os.path.join(GOLDEN, name + ".json.gz"))
        else:
            try:
                print(name, run_case(name, todo[name]).strip().splitlines()[-1:], flush=True)
            except AssertionError as ex:
                failed.append(name)
                print(name, "FAILED", str(ex)[-1500:], flush=True)
        for p in glob.glob(os.path.join(GOLDEN, name + ".*")):
            assert os.path.getsize(p) < 1024 * 1024, (p, os.path.getsize(p))
    if failed:
        sys.exit("failed: " + " ".join(failed))


def import_surface(ref, path):
    """alias -> public top-level defs / classes / assignments of the reference module behind each alias that
    a custom node can import (tests/test_custom_nodes_compat.py::test_reference_import_surface_complete)."""
    import ast
    import gzip
    import json
    from comfy_gen_server_amd import compat
    out = {}
    for alias in sorted(set(compat.DIRECT) | set(compat.FACADES)):
        p = os.path.join(ref, *alias.split(".")) + ".py"
        if not os.path.exists(p):
            p = os.path.join(ref, *alias.split("."), "__init__.py")
        if not os.path.exists(p):
            continue
        with open(p) as f:
            tree = ast.parse(f.read())
        names = []
        for node in tree.body:
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                names.append(node.name)
            elif isinstance(node, ast.Assign):
                names += [t.id for t in node.targets if isinstance(t, ast.Name)]
            elif isinstance(node, ast.AnnAssign) and isinstance(node.target, ast.Name):
                names.append(node.target.id)
        out[alias] = [n for n in dict.fromkeys(names) if not n.startswith("_")]
    with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as z:
        z.write(json.dumps(out, sort_keys=True).encode())
    print("import_surface", len(out), "modules", sum(len(v) for v in out.values()), "names", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
