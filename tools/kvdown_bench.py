#!/usr/bin/env python3
"""Time token downsampling's attention (csrc/flash_kvdown.hip), medians of 20 taken in alternating rounds in one process after a
warm-up of every shape:

  * `ops.flash_attn_kvdown` at 48 images x 72 x 128 tokens with 5 heads for s = 2 and s = 4, and at 48 x 36 x 64 with 10 heads
    for s = 2 — each beside `ops.flash_attn` on the same rows over all S keys (the plain attention) and beside the only way to
    downsample without the kernel: a gather copy of the key rows of k|v, then `ops.flash_attn` with skv = Tk; achieved FLOP/s
    on the downsampled problem's own count 4 n_img heads S Tk 64;
  * the whole CFG step (cfg_input, UNet, CFG + DDIM) at the headline latent (1, 4, 24, 72, 128) on seeded synthetic Zeroscope
    weights with the option off, on (factor 2, level 0), off again, the difference beside the spread of the two off readings.

Measured numbers only.

    python tools/kvdown_bench.py [--out profiles/kvdown_bench.json] [--iters 20] [--no_step]"""
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
from vdx.kvdown import key_rows  # noqa: E402

#         (n_img, hh, ww, heads, s)
KERNELS = [(48, 72, 128, 5, 2), (48, 72, 128, 5, 4), (48, 36, 64, 10, 2)]


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
    for n_img, hh, ww, heads, s in KERNELS:
        C, S = heads * 64, hh * ww
        M = n_img * S
        qkv = torch.randn(M, 3 * C, generator=torch.Generator().manual_seed(0)).half().to(dev)
        out = torch.empty(M, C, dtype=torch.float16, device=dev)
        idx = key_rows(n_img, hh, ww, s)
        Tk = idx.shape[1]
        idx = idx.flatten().to(dev)
        kw = dict(n_seq=n_img, sq=S, heads=heads, seq_per_kv=1, scale=0.125, v_rows=True, out=out)

        def kvdown():
            ops.flash_attn_kvdown(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], n_img=n_img, hh=hh, ww=ww, s=s, heads=heads, scale=0.125, out=out)

        def plain():
            ops.flash_attn(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], skv=S, skv_pad=S, **kw)

        def gathered():
            g = qkv[:, C:].index_select(0, idx)
            ops.flash_attn(qkv[:, :C], g[:, :C], g[:, C:], skv=Tk, skv_pad=Tk, **kw)

        row = {"n_img": n_img, "hh": hh, "ww": ww, "heads": heads, "s": s, "Tk": Tk}
        row.update(alternating({"flash_attn_kvdown": kvdown, "flash_attn_all_keys": plain, "gather_flash_attn": gathered}, iters))
        flops = 4.0 * n_img * heads * S * Tk * 64
        row["flash_attn_kvdown"]["tflops"] = round(flops / row["flash_attn_kvdown"]["median_ms"] / 1e9, 1)
        row["flash_attn_all_keys"]["tflops"] = round(flops * S / Tk / row["flash_attn_all_keys"]["median_ms"] / 1e9, 1)
        rows.append(row)
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
    out = {"latent": [1, 4, 24, 72, 128], "weights": "synthetic Zeroscope, seed 1234", "timestep": int(t), "factor": 2, "max_downsample": 1}
    out["kv_downsample_off"] = reading()
    unet.enable_kv_downsample()
    out["kv_downsample_on"] = reading()
    unet.disable_kv_downsample()
    out["kv_downsample_off_again"] = reading()
    a, b, on = out["kv_downsample_off"]["median_ms"], out["kv_downsample_off_again"]["median_ms"], out["kv_downsample_on"]["median_ms"]
    out["gap_between_off_readings_ms"] = round(abs(a - b), 4)
    out["on_minus_faster_off_ms"] = round(on - min(a, b), 4)
    out["faster_than_both_by_more_than_their_gap"] = bool(min(a, b) - on > abs(a - b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no_step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = {"job": "token downsampling: all queries against the strided key grid, read in place", "device": torch.cuda.get_device_name(0),
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
