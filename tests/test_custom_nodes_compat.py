"""Custom-node import surface: reference-style custom nodes import ``comfy.*``,
``folder_paths``, ``nodes``, ``node_helpers``, ``latent_preview``, ``server`` — these resolve to this
engine's modules through ``compat.install()``. A node written in that style (a websocket image-save node,
``_WS_NODE`` below) is loaded from a temp ``custom_nodes/`` dir and run in a prompt."""
import os

import pytest
import torch

from comfy_gen_server_amd.runtime import device as dm


def test_alias_modules_resolve():
    from comfy_gen_server_amd import compat
    compat.install()
    import comfy.utils
    import comfy.model_management
    import comfy.samplers
    import comfy.sample
    import comfy.sd
    import comfy.model_patcher
    import comfy.ops
    import comfy.k_diffusion.sampling
    import folder_paths
    import nodes
    import node_helpers
    import latent_preview
    import server
    from comfy_extras.nodes_upscale_model import ImageUpscaleWithModel  # noqa: F401
    from comfy_gen_server_amd.runtime import device, patcher
    from comfy_gen_server_amd.api import server as api_server
    assert comfy.model_management is device
    assert comfy.model_management.get_torch_device is device.get_torch_device
    assert comfy.model_patcher.ModelPatcher is patcher.ModelPatcher
    assert "euler_ancestral" in comfy.samplers.KSampler.SAMPLERS
    assert callable(comfy.sample.prepare_noise) and callable(comfy.sd.load_checkpoint_guess_config)
    assert callable(comfy.utils.load_torch_file) and callable(comfy.utils.common_upscale)
    assert comfy.utils.ProgressBar(3).total == 3
    assert comfy.ops.disable_weight_init.Linear is not None
    assert callable(comfy.k_diffusion.sampling.sample_euler)
    assert callable(folder_paths.get_filename_list) and callable(node_helpers.conditioning_set_values)
    assert callable(latent_preview.get_previewer)
    assert server.PromptServer is api_server.PromptServer
    assert "KSampler" in nodes.NODE_CLASS_MAPPINGS or hasattr(nodes, "common_ksampler")
    assert nodes.MAX_RESOLUTION >= 8192


_WS_NODE = '''
"""A custom node written the way reference-style custom nodes are: it imports ``comfy.utils`` and ``PIL``,
declares INPUT_TYPES / RETURN_TYPES / FUNCTION / OUTPUT_NODE / CATEGORY, sends each image of the batch to the
client as a PNG preview through ``comfy.utils.ProgressBar`` and registers itself in NODE_CLASS_MAPPINGS."""
from PIL import Image
import numpy as np
import comfy.utils


class SaveImageWebsocket:
    @classmethod
    def INPUT_TYPES(s):
        return {"required": {"images": ("IMAGE",)}}

    RETURN_TYPES = ()
    FUNCTION = "save_images"
    OUTPUT_NODE = True
    CATEGORY = "api/image"

    def save_images(self, images):
        pbar = comfy.utils.ProgressBar(images.shape[0])
        for step, image in enumerate(images):
            arr = np.clip(255.0 * image.cpu().numpy(), 0, 255).astype(np.uint8)
            pbar.update_absolute(step, images.shape[0], ("PNG", Image.fromarray(arr), None))
        return {}

    @classmethod
    def IS_CHANGED(s, images):
        return float("nan")


NODE_CLASS_MAPPINGS = {"SaveImageWebsocket": SaveImageWebsocket}
'''


def test_reference_style_websocket_node_loads_and_runs(tmp_path):
    dm.set_cpu_mode(True)
    cn = tmp_path / "custom_nodes"
    cn.mkdir()
    (cn / "websocket_image_save.py").write_text(_WS_NODE)
    from comfy_gen_server_amd.graph import registry
    from comfy_gen_server_amd.graph.validation import validate_prompt
    from comfy_gen_server_amd.graph.executor import PromptExecutor
    from comfy_gen_server_amd.utils import progress
    registry.init_nodes(custom_nodes=False)
    times = registry.load_custom_nodes([str(cn)])
    assert times and all(ok for _, _, ok in times), times
    assert "SaveImageWebsocket" in registry.NODE_CLASS_MAPPINGS
    frames = []
    old = progress.PROGRESS_BAR_HOOK
    progress.set_progress_bar_global_hook(lambda v, t, preview: frames.append((v, t, preview)))
    try:
        p = {"1": {"class_type": "EmptyImage", "inputs": {"width": 32, "height": 24, "batch_size": 2, "color": 255}},
             "2": {"class_type": "SaveImageWebsocket", "inputs": {"images": ["1", 0]}}}
        ok, err, outputs, node_errors = validate_prompt(p)
        assert ok, (err, node_errors)
        ex = PromptExecutor()
        ex.execute(p, "ws-1", {}, outputs)
        assert ex.success, ex.status_messages
    finally:
        progress.set_progress_bar_global_hook(old)
    assert [f[0] for f in frames] == [0, 1] and all(f[1] == 2 for f in frames)
    fmt, img, _ = frames[0][2]
    assert fmt == "PNG" and img.size == (32, 24)


def test_reference_import_surface_complete():
    """Every public top-level name of every reference module a custom node can import through the
    alias finder resolves, or is on the documented allow-list (compat_names.ALLOWED_MISSING). The names are
    the recorded list tests/golden/import_surface.json.gz (oracle/record_golden.py: alias -> public top-level
    defs / classes / assignments of the reference module behind it)."""
    import importlib
    import json
    from comfy_gen_server_amd import compat, compat_names
    compat.install()
    import gzip
    with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "import_surface.json.gz"), "rt") as f:
        surface = json.load(f)
    missing, checked = {}, 0
    for alias in sorted(set(compat.DIRECT) | set(compat.FACADES)):
        names = surface.get(alias)
        if names is None:
            continue
        mod = importlib.import_module(alias)
        allowed = compat_names.ALLOWED_MISSING.get(alias, {})
        for n in names:
            checked += 1
            if n in allowed:
                assert allowed[n], (alias, n)       # every exception carries its reason
                continue
            if not hasattr(mod, n):
                missing.setdefault(alias, []).append(n)
    assert checked > 500, checked
    assert not missing, missing


def test_optimized_attention_replace_patch_ipadapter_shape():
    """An IPAdapter-style attn2 replace patch built on ``comfy.ldm.modules.attention.optimized_attention``
    (q/k/v [B, S, heads*D], heads from extra_options) runs inside a transformer block and equals the
    unpatched block when it adds nothing."""
    from comfy_gen_server_amd import compat
    compat.install()
    from comfy.ldm.modules.attention import optimized_attention, attention_basic, optimized_attention_for_device
    from comfy_gen_server_amd.models.attention import BasicTransformerBlock
    from comfy_gen_server_amd.models.layers import init_random_
    torch.manual_seed(0)
    blk = BasicTransformerBlock(64, 2, 32, context_dim=48)
    init_random_(blk, seed=1)
    x, ctx = torch.randn(2, 16, 64), torch.randn(2, 5, 48)
    calls = []

    def ipadapter_attn2(q, k, v, extra_options):
        calls.append(extra_options["n_heads"])
        return optimized_attention(q, k, v, extra_options["n_heads"])
    with torch.inference_mode():
        plain = blk(x, ctx, {})
        to = {"block": ("input", 1), "block_index": 0,
              "patches_replace": {"attn2": {("input", 1, 0): ipadapter_attn2}}}
        patched = blk(x, ctx, to)
    assert calls == [2]
    assert torch.allclose(plain, patched, atol=1e-4, rtol=1e-4)
    q = torch.randn(2, 7, 64)
    ref = attention_basic(q, q, q, 4)
    assert torch.allclose(optimized_attention_for_device(q.device, mask=True)(q, q, q, 4), ref)
    mask = torch.ones(7, 7, dtype=torch.bool)
    assert torch.allclose(optimized_attention(q, q, q, 4, mask=mask), ref, atol=1e-5)


def test_prepare_callback_and_sigma_helpers():
    from comfy_gen_server_amd import compat
    compat.install()
    import latent_preview
    import comfy.k_diffusion.sampling as ks
    import comfy.utils
    s = ks.get_sigmas_karras(10, 0.03, 14.6)
    assert s.shape == (11,) and float(s[-1]) == 0.0 and float(s[0]) == pytest.approx(14.6, rel=1e-5)
    assert torch.all(s[:-1] > s[1:])
    e = ks.get_sigmas_exponential(5, 0.1, 10.0)
    assert float(e[0]) == pytest.approx(10.0) and float(e[-2]) == pytest.approx(0.1)

    class _M:
        load_device = torch.device("cpu")

        class model:
            class latent_format:
                latent_rgb_factors = [[0.3, 0.2, 0.1]] * 4
                taesd_decoder_name = None
    cb = latent_preview.prepare_callback(_M(), 3)
    assert callable(cb)
    cb(0, torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 8, 8), 3)
    m = torch.nn.Sequential(torch.nn.Linear(2, 2))
    prev = comfy.utils.set_attr_param(m, "0.weight", torch.ones(2, 2))
    assert prev.shape == (2, 2) and torch.equal(comfy.utils.get_attr(m, "0.weight"), torch.ones(2, 2))
    comfy.utils.copy_to_param(m, "0.bias", torch.full((2,), 3.0))
    assert torch.equal(m[0].bias, torch.full((2,), 3.0))
