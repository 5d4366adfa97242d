#!/usr/bin/env python3
"""Time token merging (csrc/tome.hip), medians of 20 after a warm-up, at 48 images of 72 x 128 tokens, C = 320, ratios 0.25 and 0.5:

  * each of the four kernels (match with its inverse-norm pre-pass, select, merge, unmerge + residual);
  * the whole self-attention stage, LayerNorm through residual, with token merging off and on (seeded synthetic weights);
  * the whole CFG step (cfg_input, UNet, CFG + DDIM) at the headline latent (1, 4, 24, 72, 128) on seeded synthetic Zeroscope
    weights with token merging off, on, and off again in the same process, with steps/s for each.

Measured numbers only.  `faster_than_both_by_more_than_their_gap` is the condition the README's claim hangs on.

    python tools/tome_bench.py [--out profiles/tome_bench.json] [--iters 20] [--no_step]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vdx  # noqa: E402,F401
from vdx import ops  # noqa: E402
from vdx.tome import partition  # noqa: E402

N_IMG, HH, WW, C = 48, 72, 128, 320
RATIOS = (0.25, 0.5)


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "iters": iters}


def stage(t, W, n_img, S, plan):
    """LayerNorm -> (merge) -> q|k|v -> flash attention -> to_out -> (unmerge) + residual, as vdx/unet3d.py runs it."""
    heads, scale = C // 64, 64 ** -0.5
    ln = ops.layernorm(t, W["g"], W["b"], M=n_img * S)
    if plan is None:
        qkv = ops.gemm(ln, W["qkv"], M=n_img * S)
        o = ops.flash_attn(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], n_seq=n_img, sq=S, skv=S, skv_pad=S, heads=heads, seq_per_kv=1,
                           scale=scale, v_rows=True)
        return ops.gemm(o, W["out"], M=n_img * S, bias=W["out_b"], residual=t)
    src, dst, r = plan
    node_max, node_idx = ops.tome_match(t, src, dst, n_img=n_img, S=S)
    slot, off, items = ops.tome_select(node_max, node_idx, src, dst, S=S, r=r)
    lm = ops.tome_merge(ln, src, dst, slot, off, items, n_img=n_img, S=S, r=r)
    Sm = S - r
    qkv = ops.gemm(lm, W["qkv"], M=n_img * Sm)
    o = ops.flash_attn(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], n_seq=n_img, sq=Sm, skv=Sm, skv_pad=Sm, heads=heads, seq_per_kv=1,
                       scale=scale, v_rows=True)
    a = ops.gemm(o, W["out"], M=n_img * Sm, bias=W["out_b"])
    return ops.tome_unmerge_add(a, slot, t, src, dst, n_img=n_img, S=S, r=r)


def step_times(dev, iters):
    from vdx.scheduler import DDIMScheduler
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    from vdx.weights import synthetic_state_dict
    cfg = UNet3DConfig.zeroscope()
    unet = UNet3DConditionModel(cfg).load_diffusers_state_dict(synthetic_state_dict(cfg, 1234, dev), device=dev)
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(1, 4, 24, 72, 128, generator=g).half().to(dev)
    emb = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).half().to(dev)
    sched = DDIMScheduler()
    sched.set_timesteps(50, device=dev)
    t = sched._host_timesteps[10]

    def step():
        noise = unet(ops.cfg_input(lat, None, 0.0), t, encoder_hidden_states=emb).sample
        return sched.step_cfg(noise, t, lat, 7.5)

    def rate(row):
        row["steps_per_s"] = round(1000.0 / row["median_ms"], 4)
        return row
    out = {"latent": [1, 4, 24, 72, 128], "weights": "synthetic Zeroscope, seed 1234", "timestep": int(t)}
    out["tome_off"] = rate(timed(step, iters))
    for ratio in RATIOS:
        unet.enable_tome(ratio)
        out[f"tome_on_{ratio}"] = rate(timed(step, iters))
    unet.disable_tome()
    out["tome_off_again"] = rate(timed(step, iters))
    a, b, on = out["tome_off"]["median_ms"], out["tome_off_again"]["median_ms"], out["tome_on_0.5"]["median_ms"]
    out["gap_between_off_readings_ms"] = round(abs(a - b), 4)
    out["on_0.5_minus_faster_off_ms"] = round(on - min(a, b), 4)
    out["faster_than_both_by_more_than_their_gap"] = bool(min(a, b) - on > abs(a - b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no_step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    S = HH * WW
    rec = {"job": f"token merging around the level-0 spatial self-attention: {N_IMG} images of {HH} x {WW} tokens, C = {C}",
           "device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(), "ratios": []}
    g = torch.Generator().manual_seed(0)
    t = torch.randn(N_IMG * S, C, generator=g).half().to(dev)
    W = {"g": torch.ones(C), "b": torch.zeros(C), "qkv": torch.randn(3 * C, C, generator=g) * C ** -0.5,
         "out": torch.randn(C, C, generator=g) * C ** -0.5, "out_b": torch.zeros(C)}
    W = {k: v.half().to(dev) for k, v in W.items()}
    rec["stage_tome_off"] = timed(lambda: stage(t, W, N_IMG, S, None), a.iters)
    for ratio in RATIOS:
        part = partition(HH, WW, ratio)
        src, dst, r = part.src_idx.to(dev), part.dst_idx.to(dev), part.r
        row = {"ratio": ratio, "n_src": part.n_src, "n_dst": part.n_dst, "r": r}
        node_max, node_idx = ops.tome_match(t, src, dst, n_img=N_IMG, S=S)
        slot, off, items = ops.tome_select(node_max, node_idx, src, dst, S=S, r=r)
        rows = ops.tome_merge(t, src, dst, slot, off, items, n_img=N_IMG, S=S, r=r)
        row["match"] = timed(lambda: ops.tome_match(t, src, dst, n_img=N_IMG, S=S), a.iters)
        row["match"]["tflops"] = round(2.0 * N_IMG * part.n_src * part.n_dst * C / row["match"]["median_ms"] / 1e9, 1)
        row["select"] = timed(lambda: ops.tome_select(node_max, node_idx, src, dst, S=S, r=r), a.iters)
        row["merge"] = timed(lambda: ops.tome_merge(t, src, dst, slot, off, items, n_img=N_IMG, S=S, r=r), a.iters)
        row["unmerge_add"] = timed(lambda: ops.tome_unmerge_add(rows, slot, t, src, dst, n_img=N_IMG, S=S, r=r), a.iters)
        row["stage_tome_on"] = timed(lambda: stage(t, W, N_IMG, S, (src, dst, r)), a.iters)
        rec["ratios"].append(row)
    rec["stage_tome_off_again"] = timed(lambda: stage(t, W, N_IMG, S, None), a.iters)
    if not a.no_step:
        rec["cfg_step"] = step_times(dev, a.iters)
    text = json.dumps(rec)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
