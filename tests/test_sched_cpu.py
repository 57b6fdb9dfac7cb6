"""Node-level multi-rank serving through the prompt API (sched/cluster.py, sched/spmd.py) on the CPU:
``main --gpus 3 --cpu`` starts rank 0 (HTTP server + coordinator) and two worker ranks over Gloo.

* a batch-6 workflow runs SPMD (2 images per rank, noise keyed by global image index) and returns
  the same images as the same prompt served whole on one rank;
* six independent batch-1 prompts are spread over all three ranks;
* a batch-2 prompt on 3 ranks runs SPMD on the rank prefix [0, 2) while rank 2 stays free;
* inside an SPMD prompt only rank 0 reads the checkpoint; the others receive it (R3 broadcast).
"""
import json
import os
import signal
import socket
import subprocess
import sys
import time
import urllib.request

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _get(url):
    with urllib.request.urlopen(url, timeout=10) as r:
        return json.loads(r.read())


def _post(url, obj):
    req = urllib.request.Request(url, data=json.dumps(obj).encode(), headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=30) as r:
        return json.loads(r.read())


def _graph(seed, batch, prefix):
    return {
        "4": {"class_type": "CheckpointLoaderSimple", "inputs": {"ckpt_name": "tiny.safetensors"}},
        "5": {"class_type": "EmptyLatentImage", "inputs": {"width": 64, "height": 64, "batch_size": batch}},
        "6": {"class_type": "CLIPTextEncode", "inputs": {"text": "a photo of a cat", "clip": ["4", 1]}},
        "7": {"class_type": "CLIPTextEncode", "inputs": {"text": "blurry", "clip": ["4", 1]}},
        "3": {"class_type": "KSampler", "inputs": {"seed": seed, "steps": 2, "cfg": 5.0,
                                                  "sampler_name": "euler_ancestral", "scheduler": "normal",
                                                  "denoise": 1.0, "model": ["4", 0], "positive": ["6", 0],
                                                  "negative": ["7", 0], "latent_image": ["5", 0]}},
        "8": {"class_type": "VAEDecode", "inputs": {"samples": ["3", 0], "vae": ["4", 2]}},
        "9": {"class_type": "SaveImage", "inputs": {"filename_prefix": prefix, "images": ["8", 0]}},
    }


def _start(tmp_path_factory, n, extra=()):
    base = tmp_path_factory.mktemp("cgs_cluster")
    for d in ("models/checkpoints", "output", "input", "temp"):
        os.makedirs(base / d, exist_ok=True)
    env = dict(os.environ, CGS_FORCE_CPU="1", OMP_NUM_THREADS="2", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "CGS_SCHED_ROLE"):
        env.pop(k, None)
    subprocess.run([sys.executable, "-c",
                    "import sys, torch; sys.path.insert(0, %r);"
                    "from comfy_gen_server_amd.tools.synth import register_tiny_family, write_checkpoint;"
                    "register_tiny_family(); write_checkpoint('tiny', %r, dtype=torch.float32)"
                    % (ROOT, str(base / "models/checkpoints/tiny.safetensors"))],
                   check=True, env=env, cwd=ROOT, timeout=300)
    env["CGS_REGISTER_TINY"] = "1"
    # The HTTP port is chosen free here but bound by the server seconds later, after the ranks' rendezvous has
    # opened many sockets of its own; one of those can take the port meanwhile. Then the server exits with
    # "address already in use" before it serves anything, and it is started again on another port.
    for attempt in range(3):
        port = _free_port()
        env["MASTER_PORT"] = str(_free_port())
        proc = subprocess.Popen([sys.executable, "-m", "comfy_gen_server_amd.main", "--gpus", str(n), "--cpu",
                                 "--listen", "127.0.0.1", "--port", str(port), "--base-directory", str(base),
                                 "--disable-custom-nodes", "--dont-print-server", "--preview-method", "none"]
                                + list(extra),
                                cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                                start_new_session=True)
        url = f"http://127.0.0.1:{port}"
        deadline = time.time() + 240
        port_taken = False
        while time.time() < deadline:
            if proc.poll() is not None:
                out = proc.stdout.read()
                proc.stdout.close()
                port_taken = ("address already in use" in out.lower() or "EADDRINUSE" in out) and attempt < 2
                if not port_taken:
                    raise RuntimeError(out[-4000:])
                try:
                    os.killpg(proc.pid, signal.SIGKILL)     # its worker ranks, if any is still up
                except ProcessLookupError:
                    pass
                break
            try:
                _get(url + "/queue")
                break
            except Exception:
                time.sleep(0.5)
        else:
            os.killpg(proc.pid, signal.SIGKILL)
            raise RuntimeError("server did not come up")
        if not port_taken:
            break
    return proc, url, base


def _stop(proc):
    os.killpg(proc.pid, signal.SIGTERM)
    try:
        proc.wait(timeout=30)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)


@pytest.fixture(scope="module")
def cluster(tmp_path_factory):
    trace = tmp_path_factory.mktemp("loads") / "reads.txt"
    os.environ["CGS_TRACE_LOADS"] = str(trace)
    try:
        proc, url, base = _start(tmp_path_factory, 3)
    finally:
        os.environ.pop("CGS_TRACE_LOADS", None)
    yield url, base, trace
    _stop(proc)


def _wait(url, pids, timeout=300):
    deadline = time.time() + timeout
    out = {}
    while time.time() < deadline and len(out) < len(pids):
        for p in pids:
            if p not in out:
                h = _get(f"{url}/history/{p}")
                if p in h:
                    out[p] = h[p]
        time.sleep(0.3)
    assert len(out) == len(pids), f"timed out: {len(out)} of {len(pids)}"
    return out


def _images(base, entry):
    from PIL import Image
    imgs = entry["outputs"]["9"]["images"]
    return [np.asarray(Image.open(os.path.join(base, "output", i["subfolder"], i["filename"]))).astype(np.int32)
            for i in imgs]


def test_batch_prompt_split_over_ranks_matches_one_rank(cluster):
    url, base, trace = cluster
    a = _post(url + "/prompt", {"prompt": _graph(11, 6, "spmd")})["prompt_id"]
    b = _post(url + "/prompt", {"prompt": _graph(11, 6, "one"), "extra_data": {"dp": "single"}})["prompt_id"]
    h = _wait(url, [a, b])
    assert h[a]["status"]["status_str"] == "success", h[a]["status"]
    assert h[b]["status"]["status_str"] == "success", h[b]["status"]
    assert h[a]["metrics"]["ranks"] == "all" and isinstance(h[b]["metrics"]["ranks"], int)
    assert h[a]["metrics"]["images_per_rank"] == {"0": 2, "1": 2, "2": 2}, h[a]["metrics"]
    # SaveImage of the sharded batch: every rank writes its own PNGs (rank 0 only names them), so a
    # worker moves at most its own third of the images' bytes -- no all-gather of fp32 IMAGEs
    img_bytes = 6 * 64 * 64 * 3 * 4
    for r, nb in h[a]["metrics"]["comm_bytes_per_rank"].items():
        if r != "0":
            assert nb <= (1 / 3 + 0.05) * img_bytes, (r, nb)
    # R3: one disk read of the checkpoint for the SPMD prompt (rank 0); ranks 1 and 2 received it over the
    # data plane. The single-rank prompt read it once more on its own rank.
    assert h[a]["metrics"]["loads_received_per_rank"] == {"0": 0, "1": 1, "2": 1}, h[a]["metrics"]
    reads = [ln.split() for ln in open(trace).read().splitlines() if "tiny.safetensors" in ln]
    assert len(reads) == 2 and reads[0][0] == "0", reads
    ia, ib = _images(base, h[a]), _images(base, h[b])
    assert len(ia) == len(ib) == 6
    for x, y in zip(ia, ib):
        d = np.abs(x - y)
        assert d.max() <= 2 and d.mean() < 0.25, (d.max(), d.mean())   # per-image noise: same images
    assert np.abs(ia[0] - ia[1]).mean() > 1.0                           # and distinct per index


def test_independent_prompts_use_every_rank(cluster):
    url, base, _ = cluster
    pids = [_post(url + "/prompt", {"prompt": _graph(100 + i, 1, f"ind{i}")})["prompt_id"] for i in range(6)]
    h = _wait(url, pids)
    assert all(e["status"]["status_str"] == "success" for e in h.values())
    ranks = {e["metrics"]["ranks"] for e in h.values()}
    assert ranks == {0, 1, 2}, ranks
    for e in h.values():
        assert len(_images(base, e)) == 1


def test_latency_mode_batch_one_matches_one_rank(tmp_path_factory):
    """``--gpus 2 --latency-mode``: a batch-1 prompt runs on both ranks with each UNet call split
    CFG-parallel (cond on rank 0, uncond on rank 1, outputs all-gathered) -- same image as one rank."""
    proc, url, base = _start(tmp_path_factory, 2, ["--latency-mode"])
    try:
        a = _post(url + "/prompt", {"prompt": _graph(21, 1, "lat")})["prompt_id"]
        b = _post(url + "/prompt", {"prompt": _graph(21, 1, "lat1"), "extra_data": {"dp": "single"}})["prompt_id"]
        h = _wait(url, [a, b])
    finally:
        _stop(proc)
    assert h[a]["status"]["status_str"] == "success", h[a]["status"]
    assert h[a]["metrics"]["ranks"] == "latency"
    x, y = _images(base, h[a])[0], _images(base, h[b])[0]
    d = np.abs(x - y)
    assert d.max() <= 2 and d.mean() < 0.25, (d.max(), d.mean())


def test_small_batch_runs_spmd_on_a_rank_prefix(cluster):
    """A batch of 2 on 3 ranks samples on ranks 0 and 1 (one image each); the result equals one rank."""
    url, base, _ = cluster
    a = _post(url + "/prompt", {"prompt": _graph(12, 2, "pre")})["prompt_id"]
    b = _post(url + "/prompt", {"prompt": _graph(12, 2, "pre1"), "extra_data": {"dp": "single"}})["prompt_id"]
    h = _wait(url, [a, b])
    assert h[a]["status"]["status_str"] == "success", h[a]["status"]
    assert h[a]["metrics"]["ranks"] == [0, 1], h[a]["metrics"]
    assert h[a]["metrics"]["images_per_rank"] == {"0": 1, "1": 1}, h[a]["metrics"]
    for x, y in zip(_images(base, h[a]), _images(base, h[b])):
        d = np.abs(x - y)
        assert d.max() <= 2 and d.mean() < 0.25, (d.max(), d.mean())


def test_spmd_png_metadata_on_every_rank(cluster):
    """SaveImage's workflow metadata (extra_pnginfo) is in every rank's PNGs, not only rank 0's."""
    from PIL import Image
    url, base, _ = cluster
    a = _post(url + "/prompt", {"prompt": _graph(13, 6, "meta"),
                                "extra_data": {"extra_pnginfo": {"workflow": {"nodes": [1, 2, 3]}}}})["prompt_id"]
    h = _wait(url, [a])[a]
    assert h["metrics"]["ranks"] == "all"
    for im in h["outputs"]["9"]["images"]:
        info = Image.open(os.path.join(base, "output", im["subfolder"], im["filename"])).info
        assert json.loads(info["workflow"]) == {"nodes": [1, 2, 3]} and "prompt" in info, im
