#!/usr/bin/env python3
"""Time FreeU (csrc/freeu.hip), medians of 20 after a warm-up:

  * the skip filter in place at (48 images, 9 x 16, 1280 channels) and (48, 18 x 32, 1280 and 640), and the same expression as
    an fp32 `torch.fft` chain on the GPU (rows -> planes, fft2, fftshift, mask, ifftshift, ifft2, real, half, planes -> rows);
    the chain's result is compared with the kernel's;
  * the backbone scale at those rows, and `x[:, :C // 2] *= b` in torch;
  * the whole CFG step (cfg_input, UNet, CFG + DDIM) at the headline latent (1, 4, 24, 72, 128) on seeded synthetic Zeroscope
    weights, FreeU off and on (1.2, 1.4, 0.9, 0.2), each timed by this tool in one process.

Measured numbers only; no ratio is claimed in advance.

    python tools/freeu_bench.py [--out profiles/freeu_bench.json] [--iters 20] [--no_step]"""
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

DIMS = (-2, -1)
SHAPES = [(48, 9, 16, 1280), (48, 18, 32, 1280), (48, 18, 32, 640)]
SETTING = dict(s1=0.9, s2=0.2, b1=1.2, b2=1.4)


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


def fft_chain(rows, n, H, W, s):
    x = rows.view(n, H, W, -1).permute(0, 3, 1, 2).float()
    f = torch.fft.fftshift(torch.fft.fft2(x, dim=DIMS), dim=DIMS)
    mask = torch.ones((H, W), dtype=torch.float32, device=rows.device)
    mask[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = s
    y = torch.fft.ifft2(torch.fft.ifftshift(f * mask, dim=DIMS), dim=DIMS).real.half()
    return y.permute(0, 2, 3, 1).reshape(rows.shape)


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
    out = {"latent": [1, 4, 24, 72, 128], "weights": "synthetic Zeroscope, seed 1234", "timestep": int(t)}
    out["freeu_off"] = timed(step, iters)
    unet.enable_freeu(**SETTING)
    out["freeu_on"] = timed(step, iters)
    unet.disable_freeu()
    out["freeu_off_again"] = timed(step, iters)
    out["on_minus_off_ms"] = round(out["freeu_on"]["median_ms"] - (out["freeu_off"]["median_ms"] + out["freeu_off_again"]["median_ms"]) / 2, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no_step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = {"job": "FreeU skip filter and backbone scale on the UNet's rows; setting b1 1.2, b2 1.4, s1 0.9, s2 0.2",
           "device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(), "kernels": []}
    g = torch.Generator().manual_seed(0)
    for n, H, W, C in SHAPES:
        rows = (torch.randn(n * H * W, C, generator=g) + 1.0).half().to(dev)
        s = 0.9 if (H, W) == (9, 16) else 0.2
        row = {"n_img": n, "plane": [H, W], "C": C, "s": s, "bytes_fp16": rows.numel() * 2}
        got = ops.freeu_filter(rows, n_img=n, h=H, w=W, s=s)
        work = rows.clone()
        row["filter_in_place"] = timed(lambda: ops.freeu_filter(work, n_img=n, h=H, w=W, s=s, out=work), a.iters)
        try:
            ref = fft_chain(rows, n, H, W, s)
            torch.cuda.synchronize()
            row["torch_fft_chain"] = timed(lambda: fft_chain(rows, n, H, W, s), a.iters)
            row["torch_over_filter"] = round(row["torch_fft_chain"]["median_ms"] / row["filter_in_place"]["median_ms"], 2)
            d = (got.float() - ref.float()).abs()
            row["agreement_with_chain"] = {"max_abs_difference": float(d.max()),
                                           "share_of_elements_that_differ": float((got != ref).float().mean())}
        except Exception as e:                                             # noqa: BLE001 (rocFFT missing or failing on this box)
            row["torch_fft_error"] = f"{type(e).__name__}: {e}"[:300]
        work = rows.clone()
        row["scale_in_place"] = timed(lambda: ops.freeu_scale(work, 1.0), a.iters)
        row["torch_scale_in_place"] = timed(lambda: work[:, :C // 2].mul_(1.0), a.iters)
        rec["kernels"].append(row)
        del rows, work, got
    if not a.no_step:
        rec["cfg_step"] = step_times(dev, a.iters)
    text = json.dumps(rec)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
