#!/usr/bin/env python3
"""Time masked video-to-video's kernels (csrc/inpaint.hip), medians of 20 after a warm-up, at the headline latent
(1, 4, 24, 72, 128) with a mask that keeps frames 0-7:

  * `mask_renoise` in place, and the same expression as torch-GPU ops (`scheduler.add_noise` + `torch.where`); the two results
    are compared;
  * `mask_paste_f32` at that latent and `mask_composite_u8` at 24 x 576 x 1024 frames, each against `torch.where`;
  * the whole CFG step (cfg_input, UNet, CFG + DDIM) on seeded synthetic Zeroscope weights without the select, with it, and
    without it again, each timed by this tool in one process.

Measured numbers only; no ratio is claimed in advance.

    python tools/inpaint_bench.py [--out profiles/inpaint_bench.json] [--iters 20] [--no_step]"""
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

SHAPE, KEEP = (1, 4, 24, 72, 128), 8
SA, S1 = 0.83984375, 0.54296875


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


def step_times(dev, iters, x0, base, m):
    from vdx.scheduler import DDIMScheduler
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    from vdx.weights import synthetic_state_dict
    cfg = UNet3DConfig.zeroscope()
    unet = UNet3DConditionModel(cfg).load_diffusers_state_dict(synthetic_state_dict(cfg, 1234, dev), device=dev)
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(*SHAPE, generator=g).half().to(dev)
    emb = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).half().to(dev)
    sched = DDIMScheduler()
    sched.set_timesteps(50, device=dev)
    t = sched._host_timesteps[10]

    def step(masked):
        noise = unet(ops.cfg_input(lat, None, 0.0), t, encoder_hidden_states=emb).sample
        new = sched.step_cfg(noise, t, lat, 7.5)
        return ops.mask_renoise(new, x0, base, m, SA, S1, False, 0) if masked else new
    out = {"latent": list(SHAPE), "weights": "synthetic Zeroscope, seed 1234", "timestep": int(t)}
    out["mask_off"] = timed(lambda: step(False), iters)
    out["mask_on"] = timed(lambda: step(True), iters)
    out["mask_off_again"] = timed(lambda: step(False), iters)
    out["on_minus_off_ms"] = round(out["mask_on"]["median_ms"] - (out["mask_off"]["median_ms"] + out["mask_off_again"]["median_ms"]) / 2, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no_step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = {"job": f"masked video-to-video kernels at {SHAPE}, the mask keeps frames 0-{KEEP - 1}",
           "device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha()}
    g = torch.Generator().manual_seed(0)
    x0, base, z = (torch.randn(*SHAPE, generator=g).half().to(dev) for _ in range(3))
    _, C, T, h, w = SHAPE
    m = torch.ones(T, h, w, dtype=torch.uint8, device=dev)
    m[:KEEP] = 0
    ops.check_latent_mask(m, T, h, w)
    mb = m.bool()[None, None]
    work = z.clone()
    row = {"bytes_fp16_latent": z.numel() * 2}
    row["kernel_in_place"] = timed(lambda: ops.mask_renoise(work, x0, base, m, SA, S1, False, 0), a.iters)
    row["kernel_in_place_last"] = timed(lambda: ops.mask_renoise(work, x0, base, m, SA, S1, True, 0), a.iters)
    row["torch_add_noise_where"] = timed(lambda: torch.where(mb, z, SA * x0 + S1 * base), a.iters)
    row["torch_over_kernel"] = round(row["torch_add_noise_where"]["median_ms"] / row["kernel_in_place"]["median_ms"], 2)
    row["equal_values"] = bool(torch.equal(ops.mask_renoise(z.clone(), x0, base, m, SA, S1, False, 0),
                                           torch.where(mb, z, SA * x0 + S1 * base)))
    rec["mask_renoise"] = row
    z32 = z.float()
    rec["mask_paste_f32"] = {"kernel_in_place": timed(lambda: ops.mask_paste_f32(z32, x0, m), a.iters),
                             "torch_where": timed(lambda: torch.where(mb, z32, x0.float()), a.iters)}
    F, H, W = 24, 576, 1024
    gen, orig = (torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(2))
    pm = torch.ones(F, H, W, dtype=torch.uint8, device=dev)
    pm[:KEEP] = 0
    out = torch.empty_like(gen)
    rec["mask_composite_u8"] = {"frames": [F, H, W, 3], "bytes_moved": 3 * gen.numel() + pm.numel(),
                                "kernel": timed(lambda: ops.mask_composite_u8(gen, orig, pm, out=out), a.iters),
                                "torch_where": timed(lambda: torch.where(pm.bool()[..., None], gen, orig), a.iters),
                                "equal_values": bool(torch.equal(ops.mask_composite_u8(gen, orig, pm),
                                                                 torch.where(pm.bool()[..., None], gen, orig)))}
    rec["mask_to_latent"] = {r: timed(lambda r=r: ops.mask_to_latent(pm, r), a.iters) for r in ops.MASK_RULES}
    del gen, orig, out
    if not a.no_step:
        rec["cfg_step"] = step_times(dev, a.iters, x0, base, m)
    text = json.dumps(rec)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
