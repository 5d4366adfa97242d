#!/usr/bin/env python3
"""Time the temporal filter (vdx/deflicker.py, csrc/deflicker.hip) of one video: 24 uint8 frames at 576x1024 already on the GPU,
strength 0.5, sigma 10.  HIP events around the kernel alone on given flows (one pass), around the whole `filter_frames` (both
flow passes included; one and two filter passes), and around the same expression as a chain of torch ops on the GPU in fp32
(`torch_chain` below: `grid_sample` with align_corners and border padding for the warp, `avg_pool2d` over a replicate-padded
plane for the patch mean).  The chain is the only yardstick there is: the parent commit has no counterpart.  grid_sample forms
its weights from normalised coordinates, so the two paths round differently near x.5; before any time is printed they must agree
within one grey level everywhere, and the share of differing bytes is recorded.  Medians of 20 after a warm-up, measured numbers
only.  Prints one JSON line; `--out FILE` also writes it.

    python tools/deflicker_bench.py [--frames 24] [--iters 20] [--out profiles/deflicker_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vdx  # noqa: E402,F401
from vdx import deflicker, ops  # noqa: E402


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
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4),
            "iters": iters}


def _warp(img, flow):
    """img (P, 3, H, W) fp32 sampled at q + flow(q), flow (P, H, W, 2) -> (P, 3, H, W)."""
    P, _, H, W = img.shape
    ys, xs = torch.meshgrid(torch.arange(H, device=img.device, dtype=torch.float32), torch.arange(W, device=img.device, dtype=torch.float32),
                            indexing="ij")
    gx = (xs + flow[..., 0]) / max(W - 1, 1) * 2 - 1
    gy = (ys + flow[..., 1]) / max(H - 1, 1) * 2 - 1
    return TF.grid_sample(img, torch.stack([gx, gy], -1), mode="bilinear", padding_mode="border", align_corners=True)


def torch_chain(frames, fab, fba, strength, sigma):
    """One pass of tests/deflicker_ref.py's expression for an open clip in fp32 torch ops on the frames' device."""
    I = frames.permute(0, 3, 1, 2).float()
    acc, wsum = torch.zeros_like(I), torch.zeros_like(I[:, :1])
    for sl, nb, flow in ((slice(1, None), I[:-1], fba), (slice(None, -1), I[1:], fab)):
        Wn = _warp(nb, flow)
        e = ((I[sl] - Wn) ** 2).sum(1, keepdim=True)
        d = TF.avg_pool2d(TF.pad(e, (1, 1, 1, 1), mode="replicate"), 3, 1) / 3
        w = 1 / (1 + d / (sigma * sigma))
        acc[sl] += w * Wn
        wsum[sl] += w
    out = (I + strength * acc) / (1 + strength * wsum)
    return torch.floor(out + 0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import lpips_ref as L
    dev = torch.device("cuda:0")
    F, H, W, lam, sig = a.frames, 576, 1024, 0.5, 10.0
    frames = torch.from_numpy(L.frames_like_video(F, H, W, seed=0)).to(dev)
    res = {"job": f"temporal filter of {F} frames {H}x{W} uint8 on the GPU, strength {lam}, sigma {sig}: Farneback flows both ways + one kernel per pass",
           "device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "torch_chain": "fp32 grid_sample (align_corners, border) + avg_pool2d over a replicate-padded plane, one pass"}
    fab, fba = deflicker.clip_flows(frames)
    got, want = ops.deflicker_frames(frames, fab, fba, lam, sig), torch_chain(frames, fab, fba, lam, sig)
    d = (got.to(torch.int16) - want.to(torch.int16)).abs()
    worst, share = int(d.max()), float((d > 0).float().mean())
    if worst > 1:
        raise SystemExit(f"kernel and torch chain disagree: largest difference {worst}, share {share:.2e}; no time printed")
    res["agreement"] = {"largest_difference": worst, "share": share, "bytes_changed_by_the_filter": float((got != frames).float().mean())}
    out = torch.empty_like(got)
    res["kernel_one_pass"] = timed(lambda: ops.deflicker_frames(frames, fab, fba, lam, sig, out=out), a.iters)
    res["torch_chain_one_pass"] = timed(lambda: torch_chain(frames, fab, fba, lam, sig), a.iters)
    res["flows_both_ways"] = timed(lambda: deflicker.clip_flows(frames), a.iters)
    res["whole_filter_frames_1_pass"] = timed(lambda: deflicker.filter_frames(frames, lam, sig, 1), a.iters)
    res["whole_filter_frames_2_passes"] = timed(lambda: deflicker.filter_frames(frames, lam, sig, 2), a.iters)
    # bytes the kernel has to move at least: frames in and out once, both flows in once
    least = 2 * F * H * W * 3 + 2 * (F - 1) * H * W * 8
    res["kernel_least_bytes"] = least
    res["kernel_least_bytes_per_s"] = round(least / (res["kernel_one_pass"]["median_ms"] * 1e-3), 1)
    res["torch_over_kernel"] = round(res["torch_chain_one_pass"]["median_ms"] / res["kernel_one_pass"]["median_ms"], 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
