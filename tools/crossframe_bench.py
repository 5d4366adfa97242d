#!/usr/bin/env python3
"""Time cross-frame attention (csrc/flash_frames.hip), medians of 20 taken in alternating rounds in one process after a warm-up
of every shape:

  * `ops.flash_attn_frames` at 2 samples x 16 frames of 72 x 128 tokens with 5 heads (level 0) and of 36 x 64 tokens with 10 heads
    (level 1), for R = 1 ("first") and R = 2 ("sparse_causal") — each beside the only way to get the same values without the
    kernel: a gather + concat of the reference frames' K | V rows per image, then `ops.flash_attn` with skv = R S; and beside
    the plain `ops.flash_attn` on the frames' own tokens (the floor: S keys per query), with the time per key relative to it;
  * the whole CFG step (cfg_input, UNet, CFG + DDIM) at the headline latent (1, 4, 24, 72, 128) on seeded synthetic Zeroscope
    weights with the switch off, on ("sparse_causal", every level), off again, the difference beside the spread of the two off
    readings.

Measured numbers only.

    python tools/crossframe_bench.py [--out profiles/crossframe_bench.json] [--iters 20] [--no_step]"""
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
from vdx.crossframe import ref_table  # noqa: E402

#         (n_samples, F, hh, ww, heads, mode)
KERNELS = [(2, 16, 72, 128, 5, "first"), (2, 16, 72, 128, 5, "sparse_causal"),
           (2, 16, 36, 64, 10, "first"), (2, 16, 36, 64, 10, "sparse_causal")]


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternating(fns, iters, warmup=3):
    """{name: {"median_ms", "min_ms", "iters"}}: every round times each of `fns` once, in order."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            ms[k].append(once(fn))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "iters": iters} for k, v in ms.items()}


def kernel_rows(dev, iters):
    rows = []
    for n, F, hh, ww, heads, mode in KERNELS:
        C, S, n_img = heads * 64, hh * ww, n * F
        M = n_img * S
        qkv = torch.randn(M, 3 * C, generator=torch.Generator().manual_seed(0)).half().to(dev)
        out = torch.empty(M, C, dtype=torch.float16, device=dev)
        table = ref_table(mode, F)
        R = table.shape[1]
        refs = table.to(dev)
        img = torch.tensor([[b * F + r for r in row] for b in range(n) for row in table.tolist()], device=dev)     # [n_img][R]
        kw = dict(heads=heads, seq_per_kv=1, scale=0.125, v_rows=True, out=out)

        def frames():
            ops.flash_attn_frames(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], n_samples=n, F=F, S=S, heads=heads, refs=refs, scale=0.125, out=out)

        def gathered():
            kv = qkv.view(n_img, S, 3 * C)[:, :, C:][img].reshape(n_img * R * S, 2 * C)
            ops.flash_attn(qkv[:, :C], kv[:, :C], kv[:, C:], n_seq=n_img, sq=S, skv=R * S, skv_pad=R * S, **kw)

        def plain():
            ops.flash_attn(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], n_seq=n_img, sq=S, skv=S, skv_pad=S, **kw)

        row = {"n_samples": n, "F": F, "hh": hh, "ww": ww, "heads": heads, "mode": mode, "R": R}
        row.update(alternating({"flash_attn_frames": frames, "gather_concat_flash_attn": gathered, "flash_attn_own_frame": plain}, iters))
        flops = 4.0 * n_img * heads * S * R * S * 64
        t, tg, tp = (row[k]["median_ms"] for k in ("flash_attn_frames", "gather_concat_flash_attn", "flash_attn_own_frame"))
        row["flash_attn_frames"]["tflops"] = round(flops / t / 1e9, 1)
        row["flash_attn_own_frame"]["tflops"] = round(flops / R / tp / 1e9, 1)
        row["gather_over_frames"] = round(tg / t, 3)
        row["time_per_key_over_own_frame"] = round(t / R / tp, 3)
        rows.append(row)
        del qkv, out
    return rows


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

    def reading():
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        ms = [once(step) for _ in range(iters)]
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "iters": iters,
                "steps_per_s": round(1000.0 / statistics.median(ms), 4)}
    out = {"latent": [1, 4, 24, 72, 128], "weights": "synthetic Zeroscope, seed 1234", "timestep": int(t), "mode": "sparse_causal",
           "max_downsample": 8}
    out["cross_frame_off"] = reading()
    unet.enable_cross_frame("sparse_causal")
    out["cross_frame_on"] = reading()
    unet.disable_cross_frame()
    out["cross_frame_off_again"] = reading()
    a, b, on = out["cross_frame_off"]["median_ms"], out["cross_frame_off_again"]["median_ms"], out["cross_frame_on"]["median_ms"]
    out["gap_between_off_readings_ms"] = round(abs(a - b), 4)
    out["on_minus_slower_off_ms"] = round(on - max(a, b), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no_step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = {"job": "cross-frame attention: keys and values from reference frames, read where they lie", "device": torch.cuda.get_device_name(0),
           "source_sha": vdx._lib.source_sha(), "kernels": kernel_rows(dev, a.iters)}
    if not a.no_step:
        rec["cfg_step"] = step_times(dev, a.iters)
    text = json.dumps(rec)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
