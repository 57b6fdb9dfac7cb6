"""Sampler / scheduler / cond-batching / tokenizer / LoRA / detection / Cascade parity against the reference, from
stored fixtures (tests/golden/sampling_*.npz|.json.gz; harness and recording: tests/_parity.py,
oracle/record_golden.py). The reference's side of every comparison is the recorded value.

* all schedulers: ``calculate_sigmas`` on the default SD1.x discrete schedule, compared exactly;
* every k-diffusion sampler + UniPC bh1/bh2 on a deterministic nonlinear toy denoiser: ODE samplers
  exactly; stochastic samplers with a zero noise source (their deterministic part exactly -- the
  noise stream itself is different by design: counter-based per image, sampling/rng.py);
* ``calc_cond_batch`` with areas, masks, strengths and timestep ranges."""
from _parity import run_case

_SCHED = r'''
from comfy_gen_server_amd.sampling import schedulers as OS, model_sampling as OMS
class OM(OMS.ModelSamplingDiscrete, OMS.EPS): pass
oms = OM(None)
if REC:
    import comfy.samplers as RS, comfy.model_sampling as RMS
    class RM(RMS.ModelSamplingDiscrete, RMS.EPS): pass
    rms = RM(None)
close(oms.sigmas, ref_t("sigmas", lambda: rms.sigmas), 1e-6, "sigma table")
names = ref_j("scheduler_names", lambda: list(RS.SCHEDULER_NAMES))
assert len(names) >= 6
for name in names:
    for steps in (1, 2, 7, 20, 33):
        close(OS.calculate_sigmas(oms, name, steps),
              ref_t(f"{name}/{steps}", lambda: RS.calculate_sigmas(rms, name, steps)), 1e-5, (name, steps))
for s in (14.6, 3.0, 0.5, 0.03):
    t = torch.tensor([s])
    close(oms.timestep(t).float(), ref_t(f"timestep/{s}", lambda: rms.timestep(t).float()), 1e-6, ("timestep", s))
    close(oms.sigma(oms.timestep(t)), ref_t(f"sigma/{s}", lambda: rms.sigma(rms.timestep(t))), 1e-6, ("sigma", s))
for p in (0.0, 0.3, 0.999, 1.0):
    rp = ref_j(f"percent_to_sigma/{p}", lambda: float(rms.percent_to_sigma(p)))
    assert abs(oms.percent_to_sigma(p) - rp) < 1e-6 * max(1, rp), p
print("schedulers ok")
'''

_SAMPLERS = r'''
from comfy_gen_server_amd.sampling import k_samplers as O, uni_pc as OU, model_sampling as OMS
if REC:
    import comfy.k_diffusion.sampling as R
    import comfy.extra_samplers.uni_pc as RU
    import comfy.samplers as RS, comfy.model_sampling as RMS
    class MS(RMS.ModelSamplingDiscrete, RMS.EPS): pass
else:
    class MS(OMS.ModelSamplingDiscrete, OMS.EPS): pass

class _NS:
    pass

class Toy:   # deterministic, nonlinear, sigma-dependent "denoiser" (+ the model_sampling path ddpm reads)
    def __init__(self):
        self.inner_model = _NS()
        self.inner_model.inner_model = _NS()
        self.inner_model.inner_model.model_sampling = MS(None)
    def __call__(self, x, sigma, **kw):
        s = sigma.reshape(-1, 1, 1, 1).to(x.dtype)
        return torch.tanh(0.7 * x) / (1 + s * s) + 0.05 * torch.sin(3 * x) * s / (1 + s)

model = Toy()
x0 = ref_t("x0", lambda: torch.randn(2, 4, 8, 8) * 14.6)
sig = ref_t("sig", lambda: RS.calculate_sigmas(MS(None), "karras", 10))
zero = lambda a, b: torch.zeros_like(x0)
def run(mod, name, **kw):
    fn = getattr(mod, "sample_" + name)
    return fn(model, x0.clone(), sig.clone(), extra_args={}, disable=True, **kw)
ode = ["euler", "heun", "dpm_2", "lms", "dpmpp_2m", "heunpp2"]
for name in ode:
    print(name, close(run(O, name), ref_t(name, lambda: run(R, name)), 1e-4, name))
noisy = ["euler_ancestral", "dpm_2_ancestral", "dpmpp_2s_ancestral", "dpmpp_sde", "dpmpp_2m_sde", "dpmpp_3m_sde",
         "ddpm", "lcm"]
for name in noisy:
    print(name, close(run(O, name, noise_sampler=zero), ref_t(name, lambda: run(R, name, noise_sampler=zero)), 1e-4, name))
print("dpmpp_2m_sde heun", close(run(O, "dpmpp_2m_sde", noise_sampler=zero, solver_type="heun"),
                                 ref_t("dpmpp_2m_sde_heun", lambda: run(R, "dpmpp_2m_sde", noise_sampler=zero, solver_type="heun")), 1e-4))
print("euler_a eta .5", close(run(O, "euler_ancestral", noise_sampler=zero, eta=0.5),
                              ref_t("euler_a_eta05", lambda: run(R, "euler_ancestral", noise_sampler=zero, eta=0.5)), 1e-4))
smin, smax = float(sig[-2]), float(sig[0])
a = O.sample_dpm_fast(model, x0.clone(), smin, smax, 8, extra_args={}, disable=True)
b = ref_t("dpm_fast", lambda: R.sample_dpm_fast(model, x0.clone(), smin, smax, 8, extra_args={}, disable=True))
print("dpm_fast", close(a, b, 1e-4))
a = O.sample_dpm_adaptive(model, x0.clone(), smin, smax, extra_args={}, disable=True)
b = ref_t("dpm_adaptive", lambda: R.sample_dpm_adaptive(model, x0.clone(), smin, smax, extra_args={}, disable=True))
print("dpm_adaptive", close(a, b, 1e-4))
# UniPC: the reference converts D(x) -> eps -> x0 in the tensor dtype (predict_eps_sigma +
# data_prediction), this engine uses D(x) directly; compared in fp64 so the algorithm (orders,
# B(h), rho solves, corrector) is pinned tightly, and in fp32 at rounding level
for v in ("bh1", "bh2"):
    a = OU.sample_unipc(model, x0.double(), sig.double(), extra_args={}, disable=True, variant=v)
    b = ref_t("unipc64_" + v, lambda: RU.sample_unipc(model, x0.double(), sig.double(), extra_args={}, disable=True, variant=v))
    print("uni_pc fp64", v, close(a, b, 1e-9))
    a = OU.sample_unipc(model, x0.clone(), sig.clone(), extra_args={}, disable=True, variant=v)
    b = ref_t("unipc32_" + v, lambda: RU.sample_unipc(model, x0.clone(), sig.clone(), extra_args={}, disable=True, variant=v))
    print("uni_pc fp32", v, close(a, b, 2e-3))
print("samplers ok")
'''

_COND = r'''
from comfy_gen_server_amd.sampling import samplers as OS, conds as OC
if REC:
    import comfy.samplers as RS, comfy.conds as RC

class Toy:
    """apply_model(x, t, c_crossattn) = x * mean(context) + t (per batch row)."""
    def apply_model(self, input_x, timestep_, **c):
        ctx = c["c_crossattn"]
        return input_x * ctx.mean(dim=(1, 2)).reshape(-1, 1, 1, 1) + timestep_.reshape(-1, 1, 1, 1) * 0.01
    def memory_required(self, shape):
        return 0

def conds_for(lib):
    C = lib.CONDCrossAttn
    g = torch.Generator().manual_seed(1)
    ctx = [torch.randn(1, 7, 8, generator=g) for _ in range(5)]
    mask = (torch.rand(1, 16, 16, generator=g) > 0.5).float()
    pos = [
        {"model_conds": {"c_crossattn": C(ctx[0])}},
        {"model_conds": {"c_crossattn": C(ctx[1])}, "area": (8, 8, 4, 4), "strength": 0.7},
        {"model_conds": {"c_crossattn": C(ctx[2])}, "mask": mask, "mask_strength": 0.5},
        {"model_conds": {"c_crossattn": C(ctx[3])}, "timestep_start": 999.0, "timestep_end": 5.0},
    ]
    neg = [{"model_conds": {"c_crossattn": C(ctx[4])}, "area": (16, 8, 0, 8)},
           {"model_conds": {"c_crossattn": C(ctx[0])}}]
    return pos, neg

x = ref_t("x", lambda: torch.randn(2, 4, 16, 16))
for sigma in (10.0, 2.0, 1.0):
    t = torch.full((2,), sigma)
    op, on = conds_for(OC)
    tok = OS.current_sigma.set(sigma)
    try:
        ours = OS.calc_cond_batch(Toy(), [op, on], x, t, {})
    finally:
        OS.current_sigma.reset(tok)
    assert len(ours) == 2
    for i, a in enumerate(ours):
        b = ref_t(f"full/{sigma}/{i}", lambda: RS.calc_cond_batch(Toy(), list(conds_for(RC)), x, t, {})[i])
        print("cond", sigma, close(a, b, 1e-5))
    # plain cond+uncond fast path (one entry each)
    ours = OS.calc_cond_batch(Toy(), [op[:1], on[1:]], x, t, {})
    assert len(ours) == 2
    for i, a in enumerate(ours):
        def fast():
            rp, rn = conds_for(RC)
            return RS.calc_cond_batch(Toy(), [rp[:1], rn[1:]], x, t, {})[i]
        close(a, ref_t(f"fast/{sigma}/{i}", fast), 1e-5, "fast path")
print("cond ok")
'''

_TOK = r'''
import tempfile
from comfy_gen_server_amd.models import text_encoders as O
from safetensors.torch import save_file
if REC:
    import comfy.sd1_clip as R
d = tempfile.mkdtemp()
g = torch.Generator().manual_seed(3)
emb = ref_t("emb_params", lambda: torch.randn(3, 768, generator=g))
save_file({"emb_params": emb.clone()}, os.path.join(d, "myemb.safetensors"))
prompts = [
    "a photo of a cat",
    "a (photo:1.3) of a ((cat)), [dog] (nested (emphasis:0.5) here:1.2)",
    "escaped \\(not weighted\\) text and (weighted \\) inside:1.1)",
    "newline\nseparated   spaces,and,commas!! unicode: café üñîçødé",
    " ".join(["word%d" % i for i in range(120)]),
    "supercalifragilisticexpialidocious antidisestablishmentarianism " * 12,
    "embedding:myemb, a painting (embedding:myemb:1.4) and embedding:missing_one",
    "",
    "(unclosed paren and: colon",
]
def plain(chunks):
    """The reference's token lists as JSON: an embedding row is stored as its row number in emb_params."""
    out = []
    for c in chunks:
        row = []
        for t in c:
            t = list(t)
            if isinstance(t[0], torch.Tensor):
                hit = (emb == t[0].float().reshape(1, -1)).all(dim=1).nonzero()
                assert hit.numel() == 1
                t[0] = {"emb_row": int(hit[0, 0])}
            else:
                t[0] = int(t[0])
            t[1] = float(t[1])
            row.append(t)
        out.append(row)
    return out
kws = (dict(), dict(pad_with_end=False), dict(pad_to_max_length=False), dict(has_start_token=True, min_length=80))
checked = 0
for ki, kw in enumerate(kws):
    ot = O.SDTokenizer(embedding_directory=d, **kw)
    for pi, p in enumerate(prompts):
        for wid in (False, True):
            a = ot.tokenize_with_weights(p, return_word_ids=wid)
            b = ref_j(f"{ki}/{pi}/{int(wid)}", lambda: plain(
                R.SDTokenizer(embedding_directory=d, **kw).tokenize_with_weights(p, return_word_ids=wid)))
            assert len(a) == len(b), (p, kw, len(a), len(b))
            for ca, cb in zip(a, b):
                assert len(ca) == len(cb), (p, kw, len(ca), len(cb))
                for ta, tb in zip(ca, cb):
                    assert len(ta) == len(tb)
                    if isinstance(tb[0], dict):
                        assert isinstance(ta[0], torch.Tensor) and torch.allclose(ta[0].float(), emb[tb[0]["emb_row"]]), p
                    else:
                        assert ta[0] == tb[0], (p, kw, ta, tb)
                    assert abs(ta[1] - tb[1]) < 1e-6, (p, kw, ta, tb)
                    if wid:
                        assert ta[2] == tb[2], (p, kw, ta, tb)
                    checked += 1
assert checked > 5000, checked
print("tokenizer ok")
'''

_LORA = r'''
import types, copy
from comfy_gen_server_amd.runtime import lora as OL, patcher as OP
from comfy_gen_server_amd.tools import synth
if REC:
    import comfy.lora as RL, comfy.model_patcher as RP, comfy.utils as RUt
g = torch.Generator().manual_seed(7)
rn = lambda *s: torch.randn(*s, generator=g) * 0.1
W = {"lin": rn(64, 48), "conv": rn(32, 16, 3, 3)}
lora = {}
to_load = {}
def add(prefix, target, entries):
    to_load[prefix] = target
    for k, v in entries.items():
        lora[prefix + "." + k] = v
# Linear targets (out 64, in 48), rank 4
add("l_lora", "lin.lora", {"lora_up.weight": rn(64, 4), "lora_down.weight": rn(4, 48), "alpha": torch.tensor(2.0)})
add("l_dora", "lin.dora", {"lora_up.weight": rn(64, 4), "lora_down.weight": rn(4, 48), "alpha": torch.tensor(4.0),
                           "dora_scale": rn(64, 1).abs() + 0.5})
add("l_diffusers", "lin.diffusers", {"lora_linear_layer.up.weight": rn(64, 4), "lora_linear_layer.down.weight": rn(4, 48)})
add("l_loha", "lin.loha", {"hada_w1_a": rn(64, 4), "hada_w1_b": rn(4, 48), "hada_w2_a": rn(64, 4), "hada_w2_b": rn(4, 48),
                           "alpha": torch.tensor(3.0)})
add("l_lokr", "lin.lokr", {"lokr_w1": rn(8, 6), "lokr_w2_a": rn(8, 2), "lokr_w2_b": rn(2, 8), "alpha": torch.tensor(1.0)})
add("l_glora", "lin.glora", {"a1.weight": rn(4, 48), "a2.weight": rn(48, 4), "b1.weight": rn(4, 48), "b2.weight": rn(64, 4),
                             "alpha": torch.tensor(2.0)})
add("l_diff", "lin.diff", {"diff": rn(64, 48)})
# Conv targets (32, 16, 3, 3): LoCon with mid, LoHa with Tucker cores, LoKr full
add("c_locon", "conv.locon", {"lora_up.weight": rn(32, 4, 1, 1), "lora_down.weight": rn(4, 16, 1, 1),
                              "lora_mid.weight": rn(4, 4, 3, 3), "alpha": torch.tensor(2.0)})
add("c_lora", "conv.lora", {"lora_up.weight": rn(32, 4, 1, 1), "lora_down.weight": rn(4, 16, 3, 3)})
add("c_loha", "conv.loha", {"hada_w1_a": rn(4, 32), "hada_w1_b": rn(4, 16), "hada_w2_a": rn(4, 32), "hada_w2_b": rn(4, 16),
                            "hada_t1": rn(4, 4, 3, 3), "hada_t2": rn(4, 4, 3, 3), "alpha": torch.tensor(2.0)})
add("c_lokr", "conv.lokr", {"lokr_w1": rn(4, 2), "lokr_w2": rn(8, 8, 3, 3)})
po = OL.load_lora(lora, to_load)
if REC:
    pr = RL.load_lora(lora, to_load)
    fake = types.SimpleNamespace()
    fake.calculate_weight = lambda p, w, k: RP.ModelPatcher.calculate_weight(fake, p, w, k)
kinds = ref_j("patch_kinds", lambda: {k: pr[k][0] for k in pr})      # patched key -> patch type
assert set(kinds) == set(po) and len(kinds) == 11, (set(kinds) ^ set(po))
for key in sorted(kinds):
    base = W[key.split(".")[0]]
    assert kinds[key] == po[key][0], key
    for strength, smodel in ((1.0, 1.0), (0.6, 0.9)):
        a = OP.calculate_weight([(strength, po[key], smodel)], base.clone(), key)
        b = ref_t(f"w/{key}/{strength}", lambda: fake.calculate_weight([(strength, pr[key], smodel)], base.clone(), key))
        close(a, b, 1e-5, key)
# key maps: SDXL UNet (ldm + diffusers names) and SDXL CLIP-L/G
unet_cfg = dict(synth.SDXL_UNET, num_head_channels=64)
from comfy_gen_server_amd.models.unet import UNetModel
with torch.device("meta"):
    net = UNetModel(**unet_cfg, dtype=torch.float16, device=torch.device("meta"))
keys = ["diffusion_model." + k for k in net.state_dict().keys()]
fm = types.SimpleNamespace(state_dict=lambda: {k: None for k in keys},
                           model_config=types.SimpleNamespace(unet_config=unet_cfg))
J = lambda v: json.loads(json.dumps(v))
ko = J(OL.model_lora_keys_unet(fm, {}))
kr = ref_j("unet_keys", lambda: RL.model_lora_keys_unet(fm, {}))
assert ko == kr and len(kr) > 1000, (len(ko), len(kr), sorted(set(ko) ^ set(kr))[:5])
from comfy_gen_server_amd.runtime import families
ct = families.SDXL(dict(synth.SDXL_UNET)).clip_target()
with torch.device("meta"):
    cm = ct.stack(dtype=torch.float16, device=torch.device("meta"))
ck = {k: None for k in cm.state_dict().keys()}
cf = types.SimpleNamespace(state_dict=lambda: ck)
co, cr = J(OL.model_lora_keys_clip(cf, {})), ref_j("clip_keys", lambda: RL.model_lora_keys_clip(cf, {}))
assert co == cr and len(co) > 100, (len(co), len(cr))
print("lora ok", len(ko), len(co))
'''

_DETECT = r'''
import copy, types
from comfy_gen_server_amd.runtime import detection as OD
from comfy_gen_server_amd.models.unet import UNetModel
from comfy_gen_server_amd.tools import synth
if REC:
    import comfy.model_detection as RD, comfy.supported_models as RSM
def jsonable(d):
    out = {}
    for k, v in d.items():
        try:
            json.dumps(v)
            out[k] = v
        except TypeError:
            pass
    return out
# the reference's registry, in its order: class name, base-class names, declared unet_config / unet_extra_config
registry = ref_j("registry", lambda: [{"name": F.__name__, "mro": [c.__name__ for c in F.__mro__],
                                       "unet_config": jsonable(F.unet_config),
                                       "unet_extra_config": jsonable(F.unet_extra_config)} for F in RSM.models])
TEMPORAL = dict(use_temporal_resblock=True, use_temporal_attention=True, extra_ff_mix_layer=True,
                use_spatial_context=True, merge_strategy="learned_with_images", merge_factor=0.0,
                video_kernel_size=[3, 1, 1], channel_mult=[1, 2, 4, 4], num_res_blocks=[2, 2, 2, 2],
                num_head_channels=64, num_heads=-1, num_classes="sequential",
                transformer_depth_output=[1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0])
BASES = {"SD15": synth.SD15_UNET, "SD20": synth.SD21_UNET, "SDXL": synth.SDXL_UNET,
         "SDXLRefiner": synth.SDXL_REFINER_UNET}
def full_config(F):
    names = F["mro"]
    base = next((BASES[n] for n in names if n in BASES), synth.SD15_UNET)
    cfg = copy.deepcopy(base)
    cfg.update(num_heads=-1, num_head_channels=64)
    part = {k: v for k, v in F["unet_config"].items()}
    cfg.update(part)
    cfg.update(F["unet_extra_config"])
    if cfg.get("adm_in_channels") and cfg.get("num_classes") is None:
        cfg["num_classes"] = "sequential"
    if cfg.get("use_temporal_resblock"):
        for k, v in TEMPORAL.items():
            cfg.setdefault(k, v) if k in part else cfg.__setitem__(k, v)
    td = cfg["transformer_depth"]
    nrb = cfg.get("num_res_blocks", [2] * len(cfg["channel_mult"]))
    if isinstance(nrb, int):
        nrb = [nrb] * len(cfg["channel_mult"])
    if len(td) != sum(nrb):       # KOALA-style shorter lists -> one res block per level
        cfg["num_res_blocks"] = [1] * len(td)
        cfg["channel_mult"] = cfg["channel_mult"][:len(td)]
        nrb = cfg["num_res_blocks"]
    if "transformer_depth_output" not in part:
        out = []
        for lvl in range(len(cfg["channel_mult"])):
            d = td[sum(nrb[:lvl])] if sum(nrb[:lvl]) < len(td) else 0
            out += [d] * (nrb[lvl] + 1)
        cfg["transformer_depth_output"] = out
    cfg["transformer_depth_middle"] = cfg.get("transformer_depth_middle", max(td))
    cfg.pop("image_size", None)
    cfg.pop("use_checkpoint", None)
    return cfg
ok, skipped = [], []
for F in registry:
    if F["name"].startswith("Stable_Cascade"):
        continue
    cfg = full_config(F)
    try:
        with torch.device("meta"):
            net = UNetModel(**cfg, dtype=torch.float16, device=torch.device("meta"))
    except Exception as e:
        skipped.append((F["name"], repr(e)[:120]))
        continue
    sd = {"model.diffusion_model." + k: v for k, v in net.state_dict().items()}
    if F["name"] == "Stable_Zero123":
        sd["cc_projection.weight"] = torch.empty(768, 772, device="meta")
        sd["cc_projection.bias"] = torch.empty(768, device="meta")
    def detect():
        r = RD.model_config_from_unet(sd, "model.diffusion_model.")
        return None if r is None else {"name": type(r).__name__, "unet_config": jsonable(r.unet_config)}
    r = ref_j("detected/" + F["name"], detect)
    o = OD.model_config_from_unet(sd, "model.diffusion_model.")
    rn = r["name"] if r is not None else None
    on = type(o).__name__ if o is not None else None
    assert rn == on, (F["name"], rn, on)
    if r is not None:
        for k, v in r["unet_config"].items():
            if k in o.unet_config:
                ov = o.unet_config[k]
                assert ov == v or (isinstance(v, (list, tuple)) and list(ov) == list(v)), (F["name"], k, v, ov)
    ok.append((F["name"], rn))
print("detect ok", ok, "skipped", skipped)
assert len(ok) >= 14, (ok, skipped)
'''

_CASCADE_CN = r'''
import copy
from comfy_gen_server_amd.models import cascade as SC
from comfy_gen_server_amd.models.cldm import ControlNet as OCN
from comfy_gen_server_amd.models.layers import init_random_
from comfy_gen_server_amd.tools.synth import TINY_UNET
if REC:
    import comfy.ops
    from comfy.ldm.cascade.stage_c import StageC as RC
    from comfy.ldm.cascade.stage_b import StageB as RB
    from comfy.ldm.cascade.stage_a import StageA as RA
    from comfy.cldm.cldm import ControlNet as RCN
    ops_ = comfy.ops.disable_weight_init

def load_same(ours, ref):
    sd = ours.state_dict()
    m, u = ref.load_state_dict(sd, strict=False)
    bufs = {n for n, _ in ref.named_buffers()}
    assert not [k for k in m if k not in bufs] and not u, (m[:5], u[:5])
    return ref

# Stage C (prior) with ControlNet-style residuals
cc = dict(c_in=16, c_out=16, c_r=16, c_cond=32, c_hidden=[32, 32], nhead=[2, 2], blocks=[[1, 1], [1, 1]],
          block_repeat=[[1, 1], [2, 1]], level_config=["CTA", "CTA"], c_clip_text=24, c_clip_text_pooled=24,
          c_clip_img=768, c_clip_seq=2, switch_level=[False])
oc = SC.StageC(**cc); init_random_(oc, seed=7)
g = torch.Generator().manual_seed(0)
x = torch.randn(2, 16, 6, 6, generator=g); r = torch.tensor([0.3, 0.7])
ct, ctp, ci = torch.randn(2, 7, 24, generator=g), torch.randn(2, 1, 24, generator=g), torch.randn(2, 1, 768, generator=g)
with torch.no_grad():
    print("stage_c", close(oc(x, r, ct, ctp, ci),
                           ref_t("stage_c", lambda: load_same(oc, RC(**cc, operations=ops_))(x, r, ct, ctp, ci)), 2e-4))
# Stage B (decoder)
bc = dict(c_in=4, c_out=4, c_r=16, patch_size=2, c_cond=32, c_hidden=[16, 24, 32], nhead=[-1, 2, 2],
          blocks=[[1, 1, 1], [1, 1, 1]], block_repeat=[[1, 1, 1], [2, 1, 1]], level_config=["CT", "CTA", "CTA"],
          c_clip=24, c_clip_seq=2, c_effnet=16)
ob = SC.StageB(**bc); init_random_(ob, seed=8)
xb = torch.randn(2, 4, 16, 16, generator=g); eff = torch.randn(2, 16, 3, 3, generator=g)
clip = torch.randn(2, 1, 24, generator=g)
rb_t = torch.tensor([0.5, 0.25])
with torch.no_grad():
    print("stage_b", close(ob(xb, rb_t, eff, clip),
                           ref_t("stage_b", lambda: load_same(ob, RB(**bc, operations=ops_))(xb, rb_t, eff, clip)), 2e-4))
# Stage A (VQGAN): encode (no quantize) and decode
oa = SC.StageA(levels=2, bottleneck_blocks=2, c_hidden=32, c_latent=4, codebook_size=64); init_random_(oa, seed=9)
oa.eval()
img = torch.rand(1, 3, 32, 32, generator=g)
box = {}
def ra():
    if "ra" not in box:
        box["ra"] = load_same(oa, RA(levels=2, bottleneck_blocks=2, c_hidden=32, c_latent=4, codebook_size=64)).eval()
    return box["ra"]
def first(v):
    return v[0] if isinstance(v, tuple) else v
with torch.no_grad():
    ea, eb = first(oa.encode(img)), ref_t("stage_a_enc", lambda: first(ra().encode(img)))
    print("stage_a enc", close(ea, eb, 2e-4))
    print("stage_a dec", close(oa.decode(eb), ref_t("stage_a_dec", lambda: ra().decode(eb)), 2e-4))
# cldm ControlNet (SD-style, tiny): per-block residual outputs
cfg = copy.deepcopy(TINY_UNET)
cfg.update(num_heads=2, num_head_channels=-1)
ocn = OCN(hint_channels=3, **cfg); init_random_(ocn, seed=3)
xh = torch.randn(2, 4, 8, 8, generator=g); hint = torch.rand(2, 3, 64, 64, generator=g)
ts = torch.tensor([500.0, 20.0]); ctx = torch.randn(2, 9, 64, generator=g)
def cn_ref():
    if "cn" not in box:
        rcfg = dict(cfg); rcfg.pop("out_channels", None)
        rcn = load_same(ocn, RCN(hint_channels=3, operations=ops_, **rcfg))
        box["cn"] = rcn(x=xh, hint=hint, timesteps=ts, context=ctx)
    return box["cn"]
with torch.no_grad():
    a = ocn(x=xh, hint=hint, timesteps=ts, context=ctx)
assert len(a) == ref_j("controlnet_outputs", lambda: len(cn_ref())), len(a)
for i, u in enumerate(a):
    close(u, ref_t(f"controlnet/{i}", lambda: cn_ref()[i]), 2e-4, ("controlnet out", i))
print("cascade/controlnet ok")
'''

CASES = {"sampling_schedulers": _SCHED, "sampling_samplers": _SAMPLERS, "sampling_cond": _COND,
         "sampling_tokenizer": _TOK, "sampling_lora": _LORA, "sampling_detect": _DETECT,
         "sampling_cascade_controlnet": _CASCADE_CN}


def _run(name):
    return run_case(name, CASES[name])


def test_schedulers_match_reference():
    assert "schedulers ok" in _run("sampling_schedulers")


def test_samplers_match_reference():
    assert "samplers ok" in _run("sampling_samplers")


def test_cond_batching_matches_reference():
    assert "cond ok" in _run("sampling_cond")


def test_tokenizer_emphasis_ti_chunking_match_reference():
    """Prompt emphasis / escapes / 77-token chunking / long-word splitting / textual inversion /
    word ids against the reference SDTokenizer's recorded output -- this engine uses its own byte-level BPE."""
    assert "tokenizer ok" in _run("sampling_tokenizer")


def test_lora_lycoris_patches_and_key_maps_match_reference():
    """LoRA / LoCon (mid) / DoRA / diffusers / LoHa (+Tucker) / LoKr / GLoRA / diff patches parsed and
    merged exactly like the reference; UNet (ldm + diffusers names) and CLIP-L/G key maps equal to the
    reference's on the SDXL architecture."""
    assert "lora ok" in _run("sampling_lora")


def test_architecture_detection_matches_reference():
    """``model_config_from_unet`` on meta-tensor state dicts of every UNet family of the reference's
    registry: the same family class is picked in the same registry order and the detected unet_config agrees
    key by key. (Stable Cascade B/C use their own stage models: tests/test_cascade.py.)"""
    out = _run("sampling_detect")
    assert "detect ok" in out, out


def test_stage_c_b_and_controlnet_match_reference_modules():
    """Stable Cascade Stage C / Stage B / Stage A and the cldm ControlNet, loaded with the same random weights
    into this engine's modules and the reference's, give the same outputs (fp32, CPU)."""
    assert "cascade/controlnet ok" in _run("sampling_cascade_controlnet")
