#!/usr/bin/env python3
"""Time the co-denoising kernels (csrc/codenoise.hip) at the headline latent (1,4,24,72,128) with two 16-frame windows that
overlap by 8.  Measured numbers only: medians of `--iters` (default 20) event-timed calls; all of these are launch-bound.

  * the fused whole-clip DDIM step (`vdx_cofuse_cfg_ddim_step_f16`) and DPM-Solver++ second-order step;
  * for scale, the plain `vdx_cfg_ddim_step_f16` at that latent (one window's worth of noise, no fuse);
  * the same fuse + DDIM expression as a chain of torch-GPU ops (fp32 weighted sums per window, then the fp16 chain);
  * `cfg_input_window` against slice-copy + `cfg_input` for one 16-frame window.
Prints one JSON line; `--out FILE` also writes it.

    python tools/codenoise_bench.py [--iters 20] [--out profiles/codenoise_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vdx  # noqa: E402,F401
from vdx import ops  # noqa: E402
from vdx.codenoise import window_table  # noqa: E402
from vdx.planner import ChunkPlan  # noqa: E402
from vdx.scheduler import DDIMScheduler, DPMSolverMultistepScheduler  # noqa: E402


def timed(fn, iters, warmup=5):
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


def torch_chain(z, wins, ranges, wn, gs, coeffs):
    """Fuse + CFG + DDIM as torch ops on GPU tensors: fp32 accumulators per frame range, then fp16 tensors with host scalars."""
    s1, sa, sp, s1p = coeffs
    acc = torch.zeros((2,) + tuple(z.shape[1:]), dtype=torch.float32, device=z.device)
    for k, ((s, e), w) in enumerate(zip(ranges, wins)):
        acc[:, :, s:e] += w.float() * wn[k, s:e].view(1, 1, -1, 1, 1)
    u, c = acc.half().chunk(2)
    eps = u + gs * (c - u)
    x0 = (z - s1 * eps) * (1.0 / sa)
    return sp * x0 + s1p * eps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1)}}
    shape, ranges, ov = (1, 4, 24, 72, 128), ((0, 16), (8, 24)), 8
    _, C, T, H, W = shape
    g = torch.Generator().manual_seed(0)
    z = torch.randn(shape, generator=g).half().to(dev)
    prev = torch.randn(shape, generator=g).half().to(dev)
    wins = [torch.randn(2, C, e - s, H, W, generator=g).half().to(dev) for s, e in ranges]
    packed = torch.cat([w.reshape(-1) for w in wins])
    tab = window_table(ChunkPlan(16, ov, ranges, 1), T)
    rows, wn = tab.rows(1, 2, wins[0].numel()), tab.wn.to(dev)
    d = DDIMScheduler()
    d.set_timesteps(50)
    cd = d.coefficients(d._host_timesteps[25])
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(25)
    cp = s.coefficients(12, True)
    out, x0 = torch.empty_like(z), torch.empty_like(z)
    eps2 = torch.randn(2, *shape[1:], generator=g).half().to(dev)
    n = z.numel()
    win_halves = sum(w.numel() for w in wins)
    got = ops.cofuse_cfg_ddim_step(z, packed, rows, wn, 7.5, cd)
    want = torch_chain(z, wins, ranges, wn, 7.5, cd)
    step = {"latent": list(shape), "windows": [list(r) for r in ranges], "halves_read": win_halves + n, "halves_written": n,
            "max_abs_diff_to_torch_chain": float((got.float() - want.float()).abs().max()),
            "fused_cofuse_cfg_ddim_step": timed(lambda: ops.cofuse_cfg_ddim_step(z, packed, rows, wn, 7.5, cd, out=out), a.iters),
            "fused_cofuse_cfg_dpm_step": timed(lambda: ops.cofuse_cfg_dpm_step(z, packed, rows, wn, 7.5, cp, x0_prev=prev, x0_out=x0,
                                                                                 out=out), a.iters),
            "plain_cfg_ddim_step": timed(lambda: ops.cfg_ddim_step(eps2, z, 7.5, cd, out=out), a.iters),
            "torch_chain": timed(lambda: torch_chain(z, wins, ranges, wn, 7.5, cd), a.iters)}
    step["torch_chain_over_fused"] = round(step["torch_chain"]["median_ms"] / step["fused_cofuse_cfg_ddim_step"]["median_ms"], 2)
    step["fused_over_plain"] = round(step["fused_cofuse_cfg_ddim_step"]["median_ms"] / step["plain_cfg_ddim_step"]["median_ms"], 2)
    step["fused_gb_per_s"] = round((win_halves + 2 * n) * 2 / (step["fused_cofuse_cfg_ddim_step"]["median_ms"] * 1e-3) / 1e9, 1)
    res["step"] = step
    ctx = torch.randn(1, C, 1, H, W, generator=g).half().to(dev)
    s0, e0 = ranges[1]
    x2 = torch.empty((2, C, e0 - s0, H, W), dtype=torch.float16, device=dev)
    a_ = ops.cfg_input_window(z, ctx, 0.35, s0, e0)
    b_ = ops.cfg_input(z[:, :, s0:e0].contiguous(), ctx, 0.35)
    res["input"] = {"window": [s0, e0], "equal": bool(torch.equal(a_, b_)),
                    "cfg_input_window": timed(lambda: ops.cfg_input_window(z, ctx, 0.35, s0, e0, out=x2), a.iters),
                    "slice_copy_plus_cfg_input": timed(lambda: ops.cfg_input(z[:, :, s0:e0].contiguous(), ctx, 0.35, out=x2), a.iters)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
