"""PhotoMaker ID-fusion parity against the reference's FuseModule / MLP, from a stored fixture
(tests/golden/photomaker_fuse.npz; harness and recording: tests/_parity.py, oracle/record_golden.py): same
random weights, same prompt embeddings / ID embeddings / class-token mask, CPU fp32. The CLIP-ViT-L vision
tower in front of it is the shared CLIP vision model (C44)."""
from _parity import run_case

_SCRIPT = r'''
from comfy_gen_server_amd.models.layers import init_random_
from comfy_gen_server_amd.nodes.extras_conditioning import FuseModule
ours = FuseModule(64)
init_random_(ours, seed=1)
prompt = ref_t("prompt", lambda: torch.randn(1, 9, 64))
ids = ref_t("ids", lambda: torch.randn(1, 2, 1, 64))
mask = torch.zeros(1, 9, dtype=torch.bool)
mask[0, 3] = mask[0, 4] = True
def ref_out():
    import comfy.ops
    from comfy_extras.nodes_photomaker import FuseModule as RefFuse
    ref = RefFuse(64, comfy.ops.manual_cast)
    m, u = ref.load_state_dict(ours.state_dict(), strict=False)
    assert not m and not u, (m, u)
    return ref(prompt.clone(), ids, mask)
with torch.no_grad():
    a = ours(prompt.clone(), ids, mask)
b = ref_t("out", ref_out)
assert a.shape == b.shape
err = (a - b).abs().max().item()
assert err < 1e-4 * max(1.0, b.abs().max().item()), err
assert torch.equal(a[0, :3], prompt[0, :3]) and (a[0, 3:5] - prompt[0, 3:5]).abs().max() > 1e-3
print("photomaker fuse", err)
'''

CASES = {"photomaker_fuse": _SCRIPT}


def test_photomaker_fuse_matches_reference():
    assert "photomaker fuse" in run_case("photomaker_fuse", _SCRIPT)
