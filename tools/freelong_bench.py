#!/usr/bin/env python3
"""Time FreeLong's blended temporal attention (csrc/freelong.hip), medians taken in alternating rounds in one process after a
warm-up of every shape, each reading a batch of launches between two device events:

  * `ops.temporal_attn_blend` at the temporal shapes of a (2, 4, F, 72, 128) UNet call, levels 0 to 3 (HW = 9216, 2304, 576, 144
    pixels with 5, 10, 20, 20 heads), for F = 48, 96 and 128 frames with window 24 —
  * beside `ops.temporal_attn` on the same rows, the floor: one attention, no band, no blend;
  * beside the composition the kernel replaces: `ops.temporal_attn` for Zg, a banded attention for Zl (no kernel of the library
    takes a band mask: torch's bmm, masked_fill, softmax, bmm on (item, F, 64) operands that were permuted BEFORE the clock
    starts, so the composition is not charged for its layout change), and Zl + Lp (Zg - Zl) as a torch subtraction and
    `baddbmm` over the frame axis on row-layout tensors;
  * the whole CFG step (cfg_input, UNet, CFG + DDIM) at (1, 4, 48, 72, 128) on seeded synthetic Zeroscope weights with the option
    off, on (window 24, d_t 0.25), off again.

Measured numbers only.

    python tools/freelong_bench.py [--out profiles/freelong_bench.json] [--iters 10] [--no_step]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vdx  # noqa: E402,F401
from vdx import freelong, ops  # noqa: E402

LEVELS = [(72 * 128, 5), (36 * 64, 10), (18 * 32, 20), (9 * 16, 20)]          # (HW, heads) of levels 0..3
FRAMES = (48, 96, 128)
WINDOW, D_T, B = 24, 0.25, 2


def batch_ms(fn, launches):
    """Milliseconds per call of `fn`, from `launches` calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


def alternating(fns, iters, launches, warmup=2):
    """{name: {"median_ms", "min_ms", "iters", "launches"}}: every round takes one reading of each of `fns`, in order."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            ms[k].append(batch_ms(fn, launches))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "iters": iters, "launches": launches}
            for k, v in ms.items()}


def kernel_rows(dev, iters):
    rows = []
    for level, (HW, heads) in enumerate(LEVELS):
        for F in FRAMES:
            inner, r = heads * 64, freelong.radius_of(WINDOW)
            M = B * F * HW
            qkv = torch.randn(M, 3 * inner, generator=torch.Generator(device=dev).manual_seed(0), dtype=torch.float16, device=dev)
            out = torch.empty(M, inner, dtype=torch.float16, device=dev)
            lp = freelong.blend_matrix(F, "gaussian", D_T).to(torch.float16).to(dev)
            kw = dict(B=B, F=F, HW=HW, heads=heads, scale=0.125)
            # the composition's operands, laid out before the clock starts: (item, F, 64) for torch's attention
            q, k, v = (t.reshape(B, F, HW, heads, 64).permute(0, 2, 3, 1, 4).reshape(-1, F, 64).contiguous()
                       for t in qkv.split(inner, dim=1))
            idx = torch.arange(F, device=dev)
            bias = torch.zeros(F, F, dtype=torch.float16, device=dev).masked_fill((idx[:, None] - idx[None, :]).abs() > r, float("-inf"))
            zg, zl = torch.empty_like(out), torch.empty_like(out)
            lpb = lp.expand(B, F, F)

            def fused():
                ops.temporal_attn_blend(qkv, lp, radius=r, out=out, **kw)

            def floor():
                ops.temporal_attn(qkv, out=zg, **kw)

            def composition():
                ops.temporal_attn(qkv, out=zg, **kw)
                torch.bmm(torch.baddbmm(bias, q, k.transpose(1, 2), alpha=0.125).softmax(dim=-1), v)
                torch.baddbmm(zl.view(B, F, -1), lpb, (zg - zl).view(B, F, -1))

            launches = max(2, min(50, int(2e9 // (M * inner))))       # enough work per reading at the small levels
            row = {"level": level, "B": B, "F": F, "HW": HW, "heads": heads, "window": WINDOW, "radius": r}
            row.update(alternating({"temporal_attn_blend": fused, "temporal_attn": floor, "composition": composition}, iters, launches))
            row["blend_over_floor"] = round(row["temporal_attn_blend"]["median_ms"] / row["temporal_attn"]["median_ms"], 3)
            row["composition_over_blend"] = round(row["composition"]["median_ms"] / row["temporal_attn_blend"]["median_ms"], 3)
            row["hbm_gb_per_s"] = round(M * inner * 2 * 4 / row["temporal_attn_blend"]["median_ms"] / 1e6, 1)     # q, k, v read once, out written once
            rows.append(row)
            print(json.dumps(row), flush=True)
            del qkv, out, q, k, v, zg, zl
            torch.cuda.empty_cache()
    return rows


def step_times(dev, iters):
    from vdx.scheduler import DDIMScheduler
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    from vdx.weights import synthetic_state_dict
    cfg = UNet3DConfig.zeroscope()
    unet = UNet3DConditionModel(cfg).load_diffusers_state_dict(synthetic_state_dict(cfg, 1234, dev), device=dev)
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(1, 4, 48, 72, 128, generator=g).half().to(dev)
    emb = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).half().to(dev)
    sched = DDIMScheduler()
    sched.set_timesteps(50, device=dev)
    t = sched._host_timesteps[10]

    def step():
        noise = unet(ops.cfg_input(lat, None, 0.0), t, encoder_hidden_states=emb).sample
        return sched.step_cfg(noise, t, lat, 7.5)

    def reading():
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        ms = [batch_ms(step, 1) for _ in range(iters)]
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "iters": iters}
    out = {"latent": [1, 4, 48, 72, 128], "weights": "synthetic Zeroscope, seed 1234", "timestep": int(t), "window": WINDOW, "d_t": D_T}
    out["free_long_off"] = reading()
    unet.enable_free_long(WINDOW, D_T)
    out["free_long_on"] = reading()
    unet.disable_free_long()
    out["free_long_off_again"] = reading()
    a, b, on = out["free_long_off"]["median_ms"], out["free_long_off_again"]["median_ms"], out["free_long_on"]["median_ms"]
    out["gap_between_off_readings_ms"] = round(abs(a - b), 4)
    out["on_minus_faster_off_ms"] = round(on - min(a, b), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no_step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = {"job": "FreeLong: global and banded temporal attention from one set of scores, blended along time by a circulant",
           "device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(), "kernels": kernel_rows(dev, a.iters)}
    if not a.no_step:
        rec["cfg_step"] = step_times(dev, a.iters)
    text = json.dumps(rec)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
