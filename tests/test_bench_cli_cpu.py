"""``bench.py`` command line on the CPU (tiny family): ``--steps`` sets the number of timed jobs, the result
line carries ``ms_per_step``, ``--dump-outputs`` writes the last timed job's images (the same from run to run),
``--full`` is accepted and leaves the result line's fields as they are."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cpu", "--family", "tiny", "--res", "64",
           "--sampler-steps", "2", "--batch-per-gpu", "2"] + list(extra)
    env = dict(os.environ, CGS_FORCE_CPU="1", OMP_NUM_THREADS="2", PYTHONPATH=ROOT)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), r.stderr


def test_dump_samples_a_large_output_identically(tmp_path, monkeypatch):
    """An output above the size limit is written as the same seeded sample of its elements every time."""
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    t = torch.arange(5 * 7 * 11 * 3, dtype=torch.int32).reshape(5, 7, 11, 3).to(torch.uint8)   # values wrap at 256
    bench._dump_outputs(str(tmp_path / "a"), {"images": t, "small": t[:1]})
    bench._dump_outputs(str(tmp_path / "b"), {"images": t.clone(), "small": t[:1]})
    a, b = np.load(tmp_path / "a" / "images.npy"), np.load(tmp_path / "b" / "images.npy")
    assert a.dtype == np.float32 and a.shape == (1000,) and np.array_equal(a, b)
    flat = t.reshape(-1).numpy().astype(np.float32)
    idx = np.sort(np.random.default_rng(0).integers(0, flat.size, size=1000))
    assert np.array_equal(a, flat[idx])
    small = np.load(tmp_path / "a" / "small.npy")
    assert small.shape == (1, 7, 11, 3) and np.array_equal(small, t[:1].numpy().astype(np.float32))


def test_dump_outputs_steps_and_full(tmp_path):
    a, err_a = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    b, _ = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "b"), "--full")
    for res in (a, b):
        assert res["steps"] == 3 and res["warmup"] == 1
        assert res["unit"] == "images/s" and res["higher_is_better"] is True and res["dtype"] == "fp32"
        assert res["ms_per_step"] > 0
        # value and ms_per_step describe the same timed region: global_batch images per step
        assert abs(res["value"] - 2 * 1000.0 / res["ms_per_step"]) <= 0.01 * res["value"]
    assert set(a) == set(b)
    # one log line per job: 1 warm-up + exactly 3 timed
    assert sum("done (pipelined)" in l for l in err_a.splitlines()) == 4, err_a
    assert os.listdir(tmp_path / "a") == ["images.npy"] == os.listdir(tmp_path / "b")
    ia, ib = np.load(tmp_path / "a" / "images.npy"), np.load(tmp_path / "b" / "images.npy")
    assert ia.dtype == np.float32 and ia.shape == (2, 64, 64, 3)
    assert ia.min() >= 0 and ia.max() <= 255 and ia.std() > 1.0      # real pixel values, not a constant
    assert np.array_equal(ia, ib)
