"""Numerical parity against the reference implementation, from stored fixtures (tests/golden/parity_*.npz;
harness and recording: tests/_parity.py, oracle/record_golden.py).

The same random weights go into both implementations (fp32, CPU) and the outputs are compared: SDXL-style UNet,
SVD video UNet (VideoResBlock / SpatialVideoTransformer / AlphaBlender incl. the image-only indicator), KL-VAE
decoder, the SVD temporal VAE decoder, the chaiNNer upscalers and the face restorers. The reference's side of
each comparison (its output, and its own weight initialisation where it sizes itself from a state dict) is the
recorded fixture; 512 x 512 outputs are stored as every second / third pixel."""
import pytest

from _parity import run_case

_SCRIPT = r'''
from comfy_gen_server_amd.models.layers import init_random_
if REC:
    import comfy.ops

def load(ref, ours):
    sd = ours.state_dict()
    m, u = ref.load_state_dict(sd, strict=False)
    assert not m and not u, (m[:5], u[:5])

def check_upscaler(make_ref, x_shape, which):
    """make_ref(): the reference architecture (it sizes itself from a seed state dict). The fixture holds its
    parameter names and shapes, and the values of what it computes itself (buffers, index tables, masks, fixed
    kernels); every other entry is drawn here from a seeded generator (BN stats / PReLU too) and loaded into
    both implementations."""
    from comfy_gen_server_amd.models import upscalers as U
    box = {}
    def ref_fixed():
        torch.manual_seed(3)
        r = box["r"] = make_ref().eval()
        bufs = {n for n, _ in r.named_buffers()}
        return {k: v for k, v in r.state_dict().items()
                if not v.is_floating_point() or k in bufs or k.endswith(("weight_h", "weight_v"))}
    fixed = ref_sd("sd", ref_fixed)
    def manifest():       # [name, shape, name of an earlier entry that is the same tensor (a shared module)]
        first, out = {}, []
        for k, v in box["r"].state_dict().items():
            out.append([k, list(v.shape), first.get(v.data_ptr()) if v.numel() else None])
            first.setdefault(v.data_ptr(), k)
        return out
    params = ref_j("params", manifest)
    g = torch.Generator().manual_seed(3)
    sd = {}
    for k, shape, same_as in params:
        if k in fixed:
            sd[k] = fixed[k]
            continue
        if same_as is not None:
            sd[k] = sd[same_as]
            continue
        sd[k] = torch.randn(shape, generator=g) * (0.1 if len(shape) > 1 else 0.5)
        if "running_var" in k:
            sd[k] = sd[k].abs() + 0.5
    if REC:
        box["r"].load_state_dict(sd)
    x = ref_t("x", lambda: torch.rand(*x_shape))
    scale = ref_j("scale", lambda: box["r"].scale)
    m = U.load_state_dict({"model": sd} if which == "swift" else sd)
    assert m.scale == scale and type(m).__name__ != "RRDBNet", (m.scale, scale)
    with torch.no_grad():
        print(which, close(m(x), ref_t("out", lambda: box["r"](x)), tol=1e-3))

Z = torch.zeros
if which == "unet":
    from comfy_gen_server_amd.models.unet import UNetModel
    cfg = dict(in_channels=4, model_channels=64, out_channels=4, num_res_blocks=[1, 1, 1], channel_mult=[1, 2, 2],
               transformer_depth=[0, 1, 2], transformer_depth_output=[0, 0, 1, 1, 2, 2], transformer_depth_middle=1,
               num_heads=-1, num_head_channels=32, use_linear_in_transformer=True, context_dim=48,
               num_classes="sequential", adm_in_channels=40)
    m = UNetModel(**cfg); init_random_(m, seed=1)
    x = ref_t("x", lambda: torch.randn(2, 4, 16, 16)); t = torch.tensor([900., 10.])
    c = ref_t("c", lambda: torch.randn(2, 9, 48)); y = ref_t("y", lambda: torch.randn(2, 40))
    def ref_out():
        from comfy.ldm.modules.diffusionmodules.openaimodel import UNetModel as R
        r = R(use_spatial_transformer=True, image_size=32, legacy=False, operations=comfy.ops.disable_weight_init, **cfg)
        load(r, m)
        return r(x, t, context=c, y=y, transformer_options={})
    with torch.no_grad():
        print("unet", close(m(x, t, context=c, y=y), ref_t("out", ref_out)))
elif which == "svd":
    from comfy_gen_server_amd.models.unet import UNetModel
    cfg = dict(in_channels=8, model_channels=32, out_channels=4, num_res_blocks=[1, 1], channel_mult=[1, 2],
               transformer_depth=[1, 1], transformer_depth_output=[1, 1, 1, 1], transformer_depth_middle=1,
               num_heads=-1, num_head_channels=16, use_linear_in_transformer=True, context_dim=64,
               num_classes="sequential", adm_in_channels=24, use_temporal_resblock=True, use_temporal_attention=True,
               extra_ff_mix_layer=True, use_spatial_context=True, merge_strategy="learned_with_images",
               merge_factor=0.0, video_kernel_size=[3, 1, 1])
    m = UNetModel(**cfg); init_random_(m, seed=5)
    for k, v in m.state_dict().items():
        if k.endswith("mix_factor"):
            v.fill_(0.3)
    x = ref_t("x", lambda: torch.randn(10, 8, 16, 16)); t = ref_t("t", lambda: torch.rand(10) * 900)
    c = ref_t("c", lambda: torch.randn(10, 1, 64)); y = ref_t("y", lambda: torch.randn(10, 24))
    ind = torch.zeros(2, 5); ind[:, 0] = 1
    box = {}
    def ref_model():
        if "r" not in box:
            from comfy.ldm.modules.diffusionmodules.openaimodel import UNetModel as R
            box["r"] = R(use_spatial_transformer=True, image_size=32, legacy=False,
                         operations=comfy.ops.disable_weight_init, **cfg)
            load(box["r"], m)
        return box["r"]
    with torch.no_grad():
        a = close(m(x, t, context=c, y=y, num_video_frames=5),
                  ref_t("out", lambda: ref_model()(x, t, context=c, y=y, num_video_frames=5, transformer_options={})))
        b = close(m(x, t, context=c, y=y, num_video_frames=5, image_only_indicator=ind),
                  ref_t("out_ind", lambda: ref_model()(x, t, context=c, y=y, num_video_frames=5,
                                                       image_only_indicator=ind, transformer_options={})))
    print("svd", a, b)
elif which in ("vae", "vae_video"):
    from comfy_gen_server_amd.models.vae import Decoder
    video = which == "vae_video"
    kw = dict(ch=32, out_ch=3, ch_mult=[1, 2], num_res_blocks=1, z_channels=4)
    m = Decoder(video_kernel_size=[3, 1, 1], alpha=0.0, **kw) if video else Decoder(**kw)
    init_random_(m, seed=2)
    for k, v in m.state_dict().items():
        if k.endswith("mix_factor"):
            v.fill_(-0.4)
    z = ref_t("z", lambda: torch.randn(6, 4, 8, 8))
    def ref_out():
        if video:
            from comfy.ldm.modules.temporal_ae import VideoDecoder as R
            r = R(attn_resolutions=[], in_channels=3, resolution=64, video_kernel_size=[3, 1, 1], alpha=0.0, **kw)
        else:
            from comfy.ldm.modules.diffusionmodules.model import Decoder as R
            r = R(attn_resolutions=[], in_channels=3, resolution=64, **kw)
        load(r, m)
        return r(z)
    with torch.no_grad():
        print(which, close(m(z), ref_t("out", ref_out)))
elif which == "spsr":
    def make_ref():
        from comfy_extras.chainner_models.architecture.SPSR import SPSRNet as R
        return R({"model.0.weight": Z(16, 3, 3, 3), "f_HR_conv1.0.bias": Z(3),
                  "model.1.sub.20.weight": Z(16, 16, 3, 3), "model.6.weight": Z(16, 16, 3, 3),
                  "model.8.weight": Z(16, 16, 3, 3)})
    check_upscaler(make_ref, (1, 3, 12, 10), which)
elif which == "swift":
    def make_ref():
        from comfy_extras.chainner_models.architecture.SwiftSRGAN import Generator as R
        return R({"initial.cnn.depthwise.weight": Z(3, 1, 9, 9), "initial.cnn.pointwise.weight": Z(16, 3, 1, 1),
                  "final_conv.pointwise.weight": Z(3, 16, 1, 1),
                  "residual.0.block1.cnn.depthwise.weight": Z(16, 1, 3, 3),
                  "residual.1.block1.cnn.depthwise.weight": Z(16, 1, 3, 3),
                  "upsampler.0.conv.depthwise.weight": Z(16, 1, 3, 3),
                  "upsampler.1.conv.depthwise.weight": Z(16, 1, 3, 3)})
    check_upscaler(make_ref, (1, 3, 12, 10), which)
elif which == "omnisr":
    def make_ref():
        from comfy_extras.chainner_models.architecture.OmniSR.OmniSR import OmniSR as R
        return R({"input.weight": Z(32, 3, 3, 3), "up.0.weight": Z(3 * 4, 32, 3, 3),
                  "residual_layer.1.residual_layer.0.layer.0.fn.0.weight": Z(32, 32, 1, 1),
                  "residual_layer.0.residual_layer.0.layer.2.fn.rel_pos_bias.weight": Z(15 * 15, 4)})
    check_upscaler(make_ref, (1, 3, 21, 18), which)
elif which == "dat":
    def make_ref():
        from comfy_extras.chainner_models.architecture.DAT import DAT as R
        R.load_state_dict = lambda self, sd, strict=True: torch.nn.Module.load_state_dict(self, sd, strict=False)
        dim = 64
        seed = {"conv_first.weight": Z(dim, 3, 3, 3), "conv_before_upsample.0.weight": Z(64, dim, 3, 3),
                "upsample.0.weight": Z(256, 64, 3, 3), "conv_last.weight": Z(3, 64, 3, 3),
                "layers.0.blocks.1.attn.temperature": Z(4, 1, 1), "layers.0.blocks.0.ffn.fc1.weight": Z(dim * 2, dim),
                "layers.0.blocks.2.attn.attn_mask_0": Z(32, 32, 32)}
        rpe = torch.stack(torch.meshgrid(torch.arange(-3, 4), torch.arange(-7, 8), indexing="ij")).flatten(1).t().float()
        seed["layers.0.blocks.0.attn.attns.0.rpe_biases"] = rpe
        for i in range(2):
            for j in range(4):
                seed[f"layers.{i}.blocks.{j}.norm1.weight"] = Z(dim)
        r = R(seed)
        assert r.split_size == [4, 8]
        return r
    check_upscaler(make_ref, (1, 3, 20, 28), which)
elif which == "lama":
    from comfy_gen_server_amd.models import upscalers as U
    from comfy_gen_server_amd.models.lama import LaMa
    m = LaMa({}, strict=False); init_random_(m, seed=7)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if "running_var" in k:
                v.abs_().add_(0.5)
    sd = {k.replace("model.model", "generator.model"): v for k, v in m.state_dict().items()}
    m = U.load_state_dict(sd)
    assert type(m).__name__ == "LaMa"
    img = ref_t("img", lambda: torch.rand(1, 3, 64, 48)); mask = ref_t("mask", lambda: (torch.rand(1, 1, 64, 48) > 0.5).float())
    def ref_out():
        # torchvision is not installed: the reference only needs it for a rotation wrapper that the
        # released config never instantiates, so a stub module satisfies the import
        tv = types.ModuleType("torchvision"); tvt = types.ModuleType("torchvision.transforms")
        tvf = types.ModuleType("torchvision.transforms.functional")
        tvf.InterpolationMode = types.SimpleNamespace(BILINEAR=2); tvf.rotate = None
        sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})
        from comfy_extras.chainner_models.architecture.LaMa import LaMa as R
        return R(sd).eval()(img, mask)
    with torch.no_grad():
        print(which, close(m(img, mask), ref_t("out", ref_out), tol=1e-3))
elif which == "gfpgan":
    from comfy_gen_server_amd.models import upscalers as U
    from comfy_gen_server_amd.models.face import GFPGANv1Clean
    m = GFPGANv1Clean({}, strict=False); init_random_(m, seed=8, std_scale=0.5)
    sd = m.state_dict()
    m = U.load_state_dict(sd)
    x = torch.rand(1, 3, 512, 512, generator=torch.Generator().manual_seed(11)) * 2 - 1
    box = {}
    def ref_run():
        if "o" not in box:
            from comfy_extras.chainner_models.architecture.face.gfpganv1_clean_arch import GFPGANv1Clean as R
            box["o"] = R(sd).eval()(x, randomize_noise=False)     # strict load on the reference side
        return box["o"]
    with torch.no_grad():
        a, rgbs_a = m(x, randomize_noise=False)
    assert len(rgbs_a) == ref_j("n_rgbs", lambda: len(ref_run()[1])) == 7
    S = (Ellipsis, slice(None, None, 3), slice(None, None, 3))      # stored: every third pixel
    print(which, close(a[S], ref_t("out", lambda: ref_run()[0][S].contiguous()), tol=2e-3),
          close(rgbs_a[-1][S], ref_t("rgb_last", lambda: ref_run()[1][-1][S].contiguous()), tol=2e-3))
elif which in ("restoreformer", "codeformer"):
    from comfy_gen_server_amd.models import upscalers as U
    from comfy_gen_server_amd.models import face
    m = face.RestoreFormer({}, strict=False) if which == "restoreformer" else face.CodeFormer({}, strict=False)
    init_random_(m, seed=9, std_scale=0.5)
    sd = m.state_dict()
    m = U.load_state_dict(sd)
    x = torch.rand(1, 3, 512, 512, generator=torch.Generator().manual_seed(12)) * 2 - 1
    box = {}
    def ref_run():
        if "o" not in box:
            if which == "restoreformer":
                from comfy_extras.chainner_models.architecture.face.restoreformer_arch import RestoreFormer as R
            else:
                from comfy_extras.chainner_models.architecture.face.codeformer import CodeFormer as R
            r = R(sd).eval()                       # strict loads on the reference side
            box["name"] = type(r).__name__
            box["o"] = r(x)
        return box["o"]
    with torch.no_grad():
        a, la = m(x)
    S = (Ellipsis, slice(None, None, 2), slice(None, None, 2))      # stored: every second pixel
    err = close(a[S], ref_t("out", lambda: ref_run()[0][S].contiguous()), tol=2e-3)
    assert type(m).__name__ == ref_j("class", lambda: box["name"])
    if which == "codeformer":
        assert torch.equal(la.argmax(-1), ref_t("codes", lambda: ref_run()[1].argmax(-1)))       # same code indices
    print(which, err)
elif which == "scunet":
    from comfy_gen_server_amd.models import swin_sr, upscalers as U
    m = swin_sr.SCUNet({}, strict=False); init_random_(m, seed=6)
    sd = m.state_dict()
    m = U.load_state_dict(sd)
    assert type(m).__name__ == "SCUNet"
    x = ref_t("x", lambda: torch.rand(1, 3, 40, 72))
    def ref_out():
        from comfy_extras.chainner_models.architecture.SCUNet import SCUNet as R
        return R(sd).eval()(x)                 # the reference loads strict: key sets must match exactly
    with torch.no_grad():
        print(which, close(m(x), ref_t("out", ref_out), tol=1e-3))
elif which.startswith(("swinir", "swin2sr", "hat")):
    dim, ws, nf = 24, 8, 64
    def blocks(n_layers, depth, extra=()):
        d = {}
        for i in range(n_layers):
            for j in range(depth):
                d[f"layers.{i}.residual_group.blocks.{j}.norm1.weight"] = Z(dim)
                for e in extra:
                    d[f"layers.{i}.residual_group.blocks.{j}.{e[0]}"] = Z(*e[1])
        return d
    b0 = "layers.0.residual_group.blocks.0."
    x_shape = (1, 3, 13, 11)
    if which.startswith("swinir"):
        kind = which.split("_")[1]
        if kind == "denoise":
            ws = 7
        seed = {"conv_first.weight": Z(dim, 3, 3, 3), b0 + "mlp.fc1.bias": Z(dim * 2),
                b0 + "attn.relative_position_bias_table": Z((2 * ws - 1) ** 2, 3),
                b0 + "attn.relative_position_index": Z(ws * ws, ws * ws, dtype=torch.long)}
        seed.update(blocks(2, 2))
        if kind == "classic":
            seed.update({"conv_before_upsample.0.weight": Z(nf, dim, 3, 3), "upsample.0.weight": Z(4 * nf, nf, 3, 3),
                         "upsample.2.weight": Z(4 * nf, nf, 3, 3), "conv_last.weight": Z(3, nf, 3, 3)})
        elif kind == "light":
            seed.update({"upsample.0.weight": Z(12, dim, 3, 3), "upsample.0.bias": Z(12)})
        elif kind == "real":
            seed.update({"conv_before_upsample.0.weight": Z(nf, dim, 3, 3), "conv_up1.weight": Z(nf, nf, 3, 3),
                         "conv_up2.weight": Z(nf, nf, 3, 3), "conv_last.weight": Z(3, nf, 3, 3),
                         "layers.0.conv.4.weight": Z(dim, dim // 4, 3, 3)})
        else:
            seed.update({"conv_last.weight": Z(3, dim, 3, 3), "layers.0.residual_group.blocks.1.attn_mask": Z(4, 49, 49)})
        def make_ref():
            from comfy_extras.chainner_models.architecture.SwinIR import SwinIR as R
            return R(seed)
    elif which.startswith("swin2sr"):
        seed = {"conv_first.weight": Z(dim, 3, 3, 3), "patch_embed.proj.weight": Z(dim, dim, 1, 1),
                b0 + "mlp.fc1.bias": Z(dim * 2), b0 + "attn.relative_position_index": Z(ws * ws, ws * ws, dtype=torch.long),
                "conv_before_upsample.0.weight": Z(nf, dim, 3, 3), "upsample.0.weight": Z(4 * nf, nf, 3, 3),
                "conv_last.weight": Z(3, nf, 3, 3)}
        seed.update(blocks(2, 2))
        if which.endswith("aux"):
            seed["conv_aux.weight"] = Z(3, nf, 3, 3)
        def make_ref():
            from comfy_extras.chainner_models.architecture.Swin2SR import Swin2SR as R
            R.load_state_dict = lambda self, sd, strict=True: torch.nn.Module.load_state_dict(self, sd, strict=False)
            return R(seed)
    else:
        dim, nf = 60, 16
        seed = {"conv_first.weight": Z(dim, 3, 3, 3), "conv_last.weight": Z(3, nf, 3, 3),
                "conv_before_upsample.0.weight": Z(nf, dim, 3, 3), "upsample.0.weight": Z(4 * nf, nf, 3, 3),
                "upsample.2.weight": Z(4 * nf, nf, 3, 3), b0 + "mlp.fc1.bias": Z(dim * 2),
                b0 + "attn.relative_position_bias_table": Z((2 * ws - 1) ** 2, 3),
                "relative_position_index_SA": Z(ws * ws, ws * ws, dtype=torch.long)}
        seed.update(blocks(2, 2, [("conv_block.cab.0.weight", (dim // 3, dim, 3, 3))]))
        x_shape = (1, 3, 19, 16)
        def make_ref():
            from comfy_extras.chainner_models.architecture.HAT import HAT as R
            return R(seed)
    check_upscaler(make_ref, x_shape, which)
'''


CASES = ["unet", "svd", "vae", "vae_video", "spsr", "swift", "swinir_classic", "swinir_light", "swinir_real",
         "swinir_denoise", "swin2sr", "swin2sr_aux", "hat", "scunet", "omnisr", "dat", "lama", "gfpgan",
         "restoreformer", "codeformer"]


def script(which):
    return f"which = {which!r}\n" + _SCRIPT


@pytest.mark.parametrize("which", CASES)
def test_matches_reference(which):
    assert which in run_case("parity_" + which, script(which))
