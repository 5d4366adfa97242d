#!/usr/bin/env python3
"""Time the frame interpolation (vdx/interp.py, csrc/interp.hip) of one video: 24 uint8 frames at 576x1024 already on the GPU,
factors 2, 3 and 4.  HIP events around the two flow passes (forward and frame-reversed), around the kernel alone on those
flows, and around the whole `interpolate_frames`; next to the kernel, the same expression as a chain of torch ops on the GPU in
fp32 (`torch_chain` below: index arithmetic and advanced indexing, no grid_sample, whose border handling and weights are not the
stated ones).  Before any time is printed the two paths must agree within the stage bound of tests/test_interp_gpu.py: at most
one grey level, in at most 1e-3 of the bytes.  Measured numbers only.  Prints one JSON line; `--out FILE` also writes it.

    python tools/interp_bench.py [--frames 24] [--iters 10] [--out profiles/interp_bench.json]"""
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
from vdx import flow, interp, ops  # noqa: E402


def timed(fn, iters, warmup=2):
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


def _clamp(v, hi):
    return torch.fmin(torch.fmax(v, torch.zeros_like(v)), torch.full_like(v, float(hi)))


def _sample(img, cx, cy):
    """img (P, H, W, C) fp32 sampled at clamped (cx, cy) (P, H, W) -> (P, H, W, C), tests/interp_ref.py's grouping."""
    P, H, W, _ = img.shape
    flx, fly = torch.floor(cx), torch.floor(cy)
    x0, y0 = flx.long().clamp(0, W - 1), fly.long().clamp(0, H - 1)
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    fx, fy = (cx - flx)[..., None], (cy - fly)[..., None]
    p = torch.arange(P, device=img.device)[:, None, None]
    gx, gy = 1 - fx, 1 - fy
    return (img[p, y0, x0] * gx + img[p, y0, x1] * fx) * gy + (img[p, y1, x0] * gx + img[p, y1, x1] * fx) * fy


def _side(img, own, other, g):
    P, H, W, _ = img.shape
    fin = torch.isfinite(g[..., 0]) & torch.isfinite(g[..., 1])
    ys, xs = torch.meshgrid(torch.arange(H, device=g.device, dtype=g.dtype), torch.arange(W, device=g.device, dtype=g.dtype),
                            indexing="ij")
    zero = torch.zeros_like(g[..., 0])
    px, py = xs + torch.where(fin, g[..., 0], zero), ys + torch.where(fin, g[..., 1], zero)
    inside = fin & (px >= -0.5) & (px <= W - 0.5) & (py >= -0.5) & (py <= H - 0.5)
    cx, cy = _clamp(px, W - 1), _clamp(py, H - 1)
    S, cf = _sample(img, cx, cy), _sample(own, cx, cy)
    back = _sample(other, _clamp(cx + cf[..., 0], W - 1), _clamp(cy + cf[..., 1], H - 1))
    r = cf + back
    n2 = r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]
    v = torch.where(torch.isfinite(n2), 1 / (1 + n2), zero)
    return S, torch.where(inside, v, v * 1e-6)


def torch_chain(frames, fab, fba, N):
    """tests/interp_ref.py's expression for a whole clip in fp32 torch ops on the frames' device."""
    F, H, W, _ = frames.shape
    out = torch.empty(((F - 1) * N + 1, H, W, 3), dtype=torch.uint8, device=frames.device)
    out[::N] = frames
    A, B = frames[:-1].float(), frames[1:].float()
    for k in range(1, N):
        t, a = np.float32(k) / np.float32(N), np.float32(N - k) / np.float32(N)
        tt, aa, at = float(t * t), float(a * a), float(a * t)
        SA, vA = _side(A, fab, fba, tt * fba - at * fab)
        SB, vB = _side(B, fba, fab, aa * fab - at * fba)
        wA, wB = float(a) * vA, float(t) * vB
        dead = ~(wA + wB > 0)
        wA, wB = torch.where(dead, torch.full_like(wA, float(a)), wA), torch.where(dead, torch.full_like(wB, float(t)), wB)
        o = (wA[..., None] * SA + wB[..., None] * SB) / (wA + wB)[..., None]
        out[k::N] = torch.floor(o + 0.5).clamp(0, 255).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import lpips_ref as L
    dev = torch.device("cuda:0")
    F, H, W = a.frames, 576, 1024
    frames = torch.from_numpy(L.frames_like_video(F, H, W, seed=0)).to(dev)
    res = {"job": f"frame interpolation of {F} frames {H}x{W} uint8 on the GPU, Farneback flows both ways + one kernel",
           "device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1)},
           "torch_chain": "fp32 index arithmetic + advanced indexing (no grid_sample), the restatement's grouping"}
    fab = flow.farneback_flows(frames)
    fba = flow.farneback_flows(frames.flip(0)).flip(0).contiguous()
    res["flows_both_ways"] = timed(lambda: (flow.farneback_flows(frames), flow.farneback_flows(frames.flip(0)).flip(0).contiguous()),
                                   a.iters)
    for N in (2, 3, 4):
        got, want = ops.interp_frames(frames, fab, fba, N), torch_chain(frames, fab, fba, N)
        d = (got.to(torch.int16) - want.to(torch.int16)).abs()
        worst, share = int(d.max()), float((d > 0).float().mean())
        if worst > 1 or share > 1e-3:
            raise SystemExit(f"factor {N}: kernel and torch chain disagree: largest difference {worst}, share {share:.2e}; no time printed")
        out = torch.empty_like(got)
        n_new = (F - 1) * (N - 1)
        row = {"frames_out": int(got.shape[0]), "agreement": {"largest_difference": worst, "share": share},
               "kernel": timed(lambda: ops.interp_frames(frames, fab, fba, N, out=out), a.iters),
               "torch_chain": timed(lambda: torch_chain(frames, fab, fba, N), max(a.iters // 2, 3), warmup=1),
               "whole_interpolate_frames": timed(lambda: interp.interpolate_frames(frames, N), a.iters)}
        # bytes the kernel has to move at least: frames in and out once, both flows in once
        least = F * H * W * 3 + int(got.numel()) + 2 * (F - 1) * H * W * 8
        row["kernel_least_bytes"] = least
        row["kernel_least_bytes_per_s"] = round(least / (row["kernel"]["median_ms"] * 1e-3), 1)
        row["kernel_us_per_new_frame"] = round(row["kernel"]["median_ms"] * 1e3 / n_new, 2)
        row["torch_over_kernel"] = round(row["torch_chain"]["median_ms"] / row["kernel"]["median_ms"], 1)
        res[f"factor_{N}"] = row
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
