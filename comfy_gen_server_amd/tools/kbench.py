"""Kernel micro-benchmarks on the SDXL shapes of SURVEY Appendix A (B=16 UNet batch = 8 images x CFG).

Compares the hand-written HIP kernels with the vendor library path through ATen (hipBLASLt GEMM,
MIOpen conv, SDPA attention) in one process, interleaved (cdna guide §5.4 rule 24), on random data.
Usage: python -m comfy_gen_server_amd.tools.kbench [--quick] [--attn | --gemm | --mask [--md=PATH]]
--mask: masked attention only (the generic flash kernel with a strided mask against the same kernel without one and
against the materialised fp32 reference a masked call used to run); --md writes the rows as a markdown table.
"""
from __future__ import annotations

import json
import math
import sys
import time

import torch
import torch.nn.functional as F


def _time(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return ts[len(ts) // 2]


def masked_attention_rows(dev, quick=False):
    """One row per (shape, mask form): ops.attention(mask=...) on the generic flash kernel, the unmasked generic
    kernel (cgs_flash_attn_fwd_v, variant 1) on the same q / k / v, and attention_reference with the same mask (the
    path of a masked call before the kernel took masks; "oom" where it does not fit)."""
    from comfy_gen_server_amd import ops
    from comfy_gen_server_amd.ops import core
    lib = ops.dispatch._native.load_kernels()
    B = 16
    shapes = [("level 2", B, 20, 1024, 1024, 64), ("level 1", B, 10, 4096, 4096, 64),
              ("level 2 cross", B, 20, 1024, 77, 64), ("level 1 cross", B, 10, 4096, 77, 64)]
    if quick:
        shapes = shapes[:1]
    rows = []
    for name, b, h, sq, sk, d in shapes:
        q, k, v = (torch.randn(b, s, h * d, device=dev).to(torch.bfloat16) for s in (sq, sk, sk))
        fl = 4.0 * b * h * sq * sk * d

        def unmasked():
            o = torch.empty_like(q)
            core._check(lib.cgs_flash_attn_fwd_v(*core._attn_operands(q, k, v, o, h), 1.0 / math.sqrt(d), 1,
                                                 core._stream()), "cgs_flash_attn_fwd_v")
            return o
        t_un = _time(unmasked)
        forms = [("[1,1,Sq,Sk] bf16", (1, 1, sq, sk), False), ("[B,1,Sq,Sk] bf16", (b, 1, sq, sk), False)]
        if sk % 8:      # the same mask as a view of rows padded to 8 keys: no copy inside the op
            forms.append(("[B,1,Sq,Sk] bf16, rows padded by the caller", (b, 1, sq, sk), True))
        for form, shape, padded in forms:
            kind = torch.randint(0, 3, shape, device=dev)
            vals = torch.randint(-16, 17, shape, device=dev).float() / 4
            m = torch.where(kind == 0, torch.full_like(vals, -math.inf), torch.where(kind == 1, 0 * vals, vals))
            m[..., 0] = 0.0                                  # every query keeps a key
            m = m.to(torch.bfloat16)
            if padded:
                buf = torch.zeros(shape[:3] + ((sk + 7) // 8 * 8,), device=dev, dtype=torch.bfloat16)
                buf[..., :sk] = m
                m = buf[..., :sk]
            ops.reset_stats()
            y = ops.attention(q, k, v, h, mask=m)
            assert ops.stats() == {("attention", "hip"): 1}, ops.stats()
            t_m = _time(lambda: ops.attention(q, k, v, h, mask=m))
            ent = dict(shape=name, B=b, H=h, Sq=sq, Sk=sk, D=d, mask=form, masked_ms=t_m, masked_tflops=fl / t_m / 1e9,
                       unmasked_generic_ms=t_un, masked_over_unmasked=t_un / t_m,
                       mask_bytes_per_tile=128 * 64 * 2, kv_bytes_per_tile=2 * 64 * d * 2)
            try:
                ref = core.attention_reference(q, k, v, h, mask=m)
                ent["maxdiff_vs_reference"] = (y.float() - ref.float()).abs().max().item()
                del ref
                t_ref = _time(lambda: core.attention_reference(q, k, v, h, mask=m), iters=3, warm=1)
                ent.update(reference_ms=t_ref, reference_over_masked=t_ref / t_m)
            except torch.cuda.OutOfMemoryError:
                ent.update(reference_ms="oom", reference_over_masked=None)
                torch.cuda.empty_cache()
            rows.append(ent)
            print(json.dumps(ent), flush=True)
    return rows


def masked_attention_markdown(rows):
    out = ["| shape | B x H x Sq x Sk | mask | masked ms | TFLOP/s | unmasked generic ms | unmasked / masked | "
           "reference ms | reference / masked |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        ref = r["reference_ms"]
        out.append(f"| {r['shape']} | {r['B']} x {r['H']} x {r['Sq']} x {r['Sk']} | {r['mask']} | "
                   f"{r['masked_ms']:.3f} | {r['masked_tflops']:.0f} | {r['unmasked_generic_ms']:.3f} | "
                   f"{r['masked_over_unmasked']:.2f} | " +
                   (f"{ref} | - |" if isinstance(ref, str) else f"{ref:.1f} | {r['reference_over_masked']:.0f}x |"))
    return "\n".join(out) + "\n"


def main(quick=False, attn_only=False, gemm_only=False, mask_only=False, md=None):
    import os
    os.environ["CGS_AUTOTUNE"] = "0"      # explicit variants below; the per-shape tuner would override them
    from comfy_gen_server_amd import ops
    from comfy_gen_server_amd.ops import core
    from comfy_gen_server_amd.ops.dispatch import set_backend_override
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    res = {"gemm": [], "attention": [], "masked_attention": [], "groupnorm": [], "layernorm": [], "conv": []}
    B = 16
    if mask_only:
        res["masked_attention"] = masked_attention_rows(dev, quick)
        if md:
            with open(md, "w") as f:
                f.write(masked_attention_markdown(res["masked_attention"]))
        return res
    gemm_shapes = [(B * 1024, 1280, 1280), (B * 1024, 1280, 3840), (B * 1024, 10240, 1280), (B * 1024, 1280, 5120),
                   (B * 4096, 640, 640), (B * 4096, 5120, 640), (B * 4096, 640, 2560), (B * 77, 1280, 2048)]
    if quick:
        gemm_shapes = gemm_shapes[:3]
    if attn_only:
        gemm_shapes = []
    if gemm_only:
        gemm_shapes = [(4096, 4096, 4096), (8192, 8192, 8192)] + gemm_shapes[:-1]
    for M, N, K in gemm_shapes:
        a = torch.randn(M, K, device=dev).to(torch.bfloat16)
        w = (torch.randn(N, K, device=dev) / math.sqrt(K)).to(torch.bfloat16)
        bias = torch.randn(N, device=dev).to(torch.bfloat16)
        fl = 2.0 * M * N * K
        lib = ops.dispatch._native.load_kernels()
        ent = dict(M=M, N=N, K=K)
        for var in (3, 4, 5, 6):
            lib.cgs_gemm_set_variant(var)
            for g in ((1, 8) if var >= 3 else (8,)):
                lib.cgs_set_tile_group(g)
                t = _time(lambda: ops.linear(a, w, bias))
                ent[f"v{var}g{g}_tflops"] = fl / t / 1e9
        lib.cgs_set_tile_group(8)
        lib.cgs_gemm_set_variant(-1)
        t_lib = _time(lambda: F.linear(a, w, bias))
        ent["lib_tflops"] = fl / t_lib / 1e9
        res["gemm"].append(ent)
        if gemm_only:
            print(json.dumps({k: (round(v) if isinstance(v, float) else v) for k, v in ent.items()}), flush=True)
    if gemm_only:
        return res
    att_shapes = [(B, 20, 1024, 1024, 64), (B, 10, 4096, 4096, 64), (B, 20, 1024, 77, 64), (B, 10, 4096, 77, 64)]
    if quick:
        att_shapes = att_shapes[:2]
    for b, h, sq, sk, d in att_shapes:
        q = torch.randn(b, sq, h * d, device=dev).to(torch.bfloat16)
        k = torch.randn(b, sk, h * d, device=dev).to(torch.bfloat16)
        v = torch.randn(b, sk, h * d, device=dev).to(torch.bfloat16)
        fl = 4.0 * b * h * sq * sk * d
        lib = ops.dispatch._native.load_kernels()
        ent = dict(B=b, H=h, Sq=sq, Sk=sk, D=d)
        ref = None
        for var, name in ((1, "generic"), (2, "d64"), (5, "d64q128"), (0, "auto")):
            lib.cgs_attn_set_variant(var)
            y = ops.attention(q, k, v, h).float()
            if ref is None:
                ref = y
            ent[f"{name}_maxdiff"] = (y - ref).abs().max().item()
            t_hip = _time(lambda: ops.attention(q, k, v, h))
            ent[f"{name}_ms"] = t_hip
            ent[f"{name}_tflops"] = fl / t_hip / 1e9
        lib.cgs_attn_set_variant(0)
        qh, kh, vh = (t.view(b, -1, h, d).transpose(1, 2) for t in (q, k, v))
        t_sdpa = _time(lambda: F.scaled_dot_product_attention(qh, kh, vh))
        ent.update(sdpa_ms=t_sdpa, sdpa_tflops=fl / t_sdpa / 1e9)
        if sq == sk:   # q/k/v as views of one fused QKV projection (the UNet's layout)
            qkv = torch.randn(b, sq, 3 * h * d, device=dev).to(torch.bfloat16)
            qv, kv_, vv = qkv.split(h * d, dim=-1)
            t_f = _time(lambda: ops.attention(qv, kv_, vv, h))
            ent.update(fused_qkv_ms=t_f, fused_qkv_tflops=fl / t_f / 1e9)
        res["attention"].append(ent)
        if attn_only:
            print(json.dumps(ent), flush=True)
    if attn_only:
        return res
    res["masked_attention"] = masked_attention_rows(dev, quick)
    for N, C, H, W in [(B, 320, 128, 128), (B, 640, 64, 64), (B, 1280, 32, 32)]:
        x = torch.randn(N, C, H, W, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        wt = torch.randn(C, device=dev).to(torch.bfloat16)
        bt = torch.randn(C, device=dev).to(torch.bfloat16)
        nbytes = 2 * x.numel() * 2
        t_hip = _time(lambda: ops.group_norm(x, 32, wt, bt, 1e-5, silu=True))
        t_lib = _time(lambda: F.silu(F.group_norm(x, 32, wt, bt, 1e-5)))
        res["groupnorm"].append(dict(shape=[N, C, H, W], hip_ms=t_hip, lib_ms=t_lib, hip_GBps=nbytes / t_hip / 1e6,
                                     lib_GBps=nbytes / t_lib / 1e6))
    for rows, C in [(B * 4096, 640), (B * 1024, 1280)]:
        x = torch.randn(rows, C, device=dev).to(torch.bfloat16)
        wt = torch.randn(C, device=dev).to(torch.bfloat16)
        bt = torch.randn(C, device=dev).to(torch.bfloat16)
        nbytes = 2 * x.numel() * 2
        t_hip = _time(lambda: ops.layer_norm(x, wt, bt))
        t_lib = _time(lambda: F.layer_norm(x, (C,), wt, bt))
        res["layernorm"].append(dict(rows=rows, C=C, hip_ms=t_hip, lib_ms=t_lib, hip_GBps=nbytes / t_hip / 1e6,
                                     lib_GBps=nbytes / t_lib / 1e6))
    for N, Ci, H, W, Co in [(B, 320, 128, 128, 320), (B, 640, 128, 128, 320), (B, 960, 128, 128, 320),
                            (B, 640, 64, 64, 640), (B, 1280, 32, 32, 1280),
                            (B, 1920, 32, 32, 1280), (1, 256, 512, 512, 256), (1, 128, 1024, 1024, 128)]:
        x = torch.randn(N, Ci, H, W, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        wt = (torch.randn(Co, Ci, 3, 3, device=dev) / math.sqrt(Ci * 9)).to(torch.bfloat16)
        bt = torch.randn(Co, device=dev).to(torch.bfloat16)
        fl = 2.0 * N * H * W * Co * Ci * 9
        t_lib = _time(lambda: F.conv2d(x, wt, bt, 1, 1))
        entry = dict(shape=[N, Ci, H, W, Co], lib_ms=t_lib, lib_tflops=fl / t_lib / 1e9)
        if ops.dispatch._native.has_kernel("cgs_conv2d_nhwc"):
            wn = wt.permute(0, 2, 3, 1).contiguous()
            set_backend_override("conv", "hip")
            lib = ops.dispatch._native.load_kernels()
            for var in (2, 3, 4, 5, 6):
                lib.cgs_conv_set_variant(var)
                for g in (8,):
                    lib.cgs_conv_set_tile_group(g)
                    t_hip = _time(lambda: ops.conv2d(x, wt, bt, 1, 1, weight_nhwc=wn))
                    entry.update({f"v{var}g{g}_tflops": fl / t_hip / 1e9})
            lib.cgs_conv_set_tile_group(8)
            lib.cgs_conv_set_variant(-1)
            set_backend_override("conv", None)
        res["conv"].append(entry)
    print(json.dumps(res, indent=1))
    return res


if __name__ == "__main__":
    main(quick="--quick" in sys.argv, attn_only="--attn" in sys.argv, gemm_only="--gemm" in sys.argv,
         mask_only="--mask" in sys.argv, md=next((a[5:] for a in sys.argv if a.startswith("--md=")), None))
