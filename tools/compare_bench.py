#!/usr/bin/env python3
"""Time the clip comparison (vdx/compare.py, csrc/compare.hip) of one video against another: 24 uint8 frames at 576x1024, both
clips already on the GPU.  HIP events around PSNR + SSIM (one scale) and around the full PSNR + SSIM + MS-SSIM call, per
kernel (ssim_scale per scale, down2 per step, finalize), and around `compare_frames` itself (which adds the copy of 30 means
per frame to the host); next to them the same expression as a chain of torch ops on the GPU in fp32, as one would write it
(`torch_chain` below: conv2d with the Gaussian as two separable passes over the planes as a batch, avg_pool2d between the
scales).  Before any time is printed the two paths must agree to 1e-3 in every mean (the chain's fp32 moments cancel; its
content is noisy enough for that bound) and exactly in sse.  Warm-up, repeated runs, medians.  Measured numbers only.  Prints one JSON line;
`--out FILE` also writes it.

    python tools/compare_bench.py [--frames 24] [--iters 20] [--out profiles/compare_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vdx  # noqa: E402,F401
from vdx import compare, ops  # noqa: E402


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
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "iters": iters}


def torch_chain(a, b, scales):
    """tests/compare_ref.py's expression in fp32 torch ops on the clips' device -> (means (F, 3, scales, 2), sse int64 [F])."""
    F = a.shape[0]
    w = torch.from_numpy(compare.window()).float().to(a.device)
    wv, wh = w.view(1, 1, 11, 1), w.view(1, 1, 1, 11)
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    d = a.to(torch.int64) - b.to(torch.int64)
    sse = (d * d).sum(dim=(1, 2, 3))
    x = a.permute(0, 3, 1, 2).reshape(F * 3, 1, *a.shape[1:3]).float()
    y = b.permute(0, 3, 1, 2).reshape(F * 3, 1, *a.shape[1:3]).float()
    out = []

    def filt(p):
        return torch.nn.functional.conv2d(torch.nn.functional.conv2d(p, wv), wh)
    for s in range(scales):
        if s:
            x, y = torch.nn.functional.avg_pool2d(x, 2), torch.nn.functional.avg_pool2d(y, 2)
        mx, my = filt(x), filt(y)
        sx2, sy2, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
        cs = (2 * sxy + C2) / (sx2 + sy2 + C2)
        ssim = (2 * (mx * my) + C1) / (mx * mx + my * my + C1) * cs
        out.append(torch.stack([ssim.mean(dim=(1, 2, 3)), cs.mean(dim=(1, 2, 3))], -1))
    return torch.stack(out, 1).view(F, 3, scales, 2), sse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import lpips_ref as L
    dev = torch.device("cuda:0")
    F, H, W = args.frames, 576, 1024
    a = torch.from_numpy(L.frames_like_video(F, H, W, seed=0)).to(dev)
    g = torch.Generator(device="cpu").manual_seed(1)
    b = (a.cpu().to(torch.int16) + torch.randint(-6, 7, a.shape, generator=g, dtype=torch.int16)).clamp(0, 255).to(torch.uint8).to(dev)
    res = {"job": f"PSNR / SSIM / MS-SSIM between two clips of {F} frames {H}x{W} uint8, both on the GPU",
           "device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1)},
           "torch_chain": "fp32 conv2d (11x1 then 1x11) per moment, avg_pool2d between scales, mean per plane"}
    for scales, name in ((1, "psnr_ssim"), (5, "psnr_ssim_ms_ssim")):
        got, sse = compare.plane_means(a, b, scales)
        want, wsse = torch_chain(a, b, scales)
        worst = float((got[:, :, :scales] - want.double()).abs().max())
        if worst > 1e-3 or not torch.equal(sse, wsse):
            raise SystemExit(f"{name}: kernels and torch chain disagree: means {worst:.3e}, sse equal {torch.equal(sse, wsse)}; no time printed")
        row = {"agreement": {"max_abs_mean_difference": worst, "sse_equal": True},
               "kernels": timed(lambda: compare.plane_means(a, b, scales), args.iters),
               "torch_chain": timed(lambda: torch_chain(a, b, scales), max(args.iters // 4, 3), warmup=1),
               "whole_compare_frames": timed(lambda: compare.compare_frames(a, b, ms_ssim=scales > 1), args.iters)}
        row["torch_over_kernels"] = round(row["torch_chain"]["median_ms"] / row["kernels"]["median_ms"], 1)
        res[name] = row
    # per kernel, at the sizes of the five scales
    taps = compare.window()
    per, x, y = {}, a, b
    means = torch.zeros((F, 3, 5, 2), dtype=torch.float64, device=dev)
    sse = torch.empty((F,), dtype=torch.int64, device=dev)
    for s in range(5):
        if s:
            per[f"down2_to_scale_{s}"] = timed(lambda: ops.compare_down2(x, y), args.iters)
            x, y = ops.compare_down2(x, y)
        h, w = (int(v) for v in (x.shape[1:3] if s == 0 else x.shape[1:]))
        per[f"ssim_scale_{s}"] = dict(timed(lambda: ops.compare_ssim_scale(x, y, taps), args.iters), height=h, width=w)
        part, sp = ops.compare_ssim_scale(x, y, taps)
        per[f"finalize_{s}"] = timed(lambda: ops.compare_finalize(part, sp, (h - 10) * (w - 10), s, means, sse if sp is not None else None),
                                     args.iters)
    res["per_kernel"] = per
    # what scale 0 has to move at least: both clips once
    least = 2 * F * H * W * 3
    res["scale_0_least_bytes"] = least
    res["scale_0_least_bytes_per_s"] = round(least / (per["ssim_scale_0"]["median_ms"] * 1e-3), 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
