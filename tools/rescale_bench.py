#!/usr/bin/env python3
"""Time the CFG-rescale kernels (csrc/rescale.hip) at the headline latent (1,4,24,72,128).  Measured numbers only: medians of
`--iters` (default 20) event-timed calls; all of these are launch-bound.

  * statistics + step for DDIM and for DPM-Solver++ (second order), and each launch on its own;
  * the co-fused pair with two 16-frame windows that overlap by 8;
  * baselines in the same process: the plain fused steps without rescale, and the same expression (combine, two `std`, the
    rescale, the DDIM chain) as a chain of torch-GPU ops.
Prints one JSON line; `--out FILE` also writes it.

    python tools/rescale_bench.py [--iters 20] [--out profiles/rescale_bench.json]"""
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


def torch_chain(eps2, z, gs, phi, coeffs):
    """CFG + rescale + DDIM as torch ops on fp16 GPU tensors with host scalars (diffusers' `rescale_noise_cfg`, then the step)."""
    s1, sa, sp, s1p = coeffs
    u, c = eps2.chunk(2)
    g = u + gs * (c - u)
    g = phi * (g * (c.std() / g.std())) + (1.0 - phi) * g
    x0 = (z - s1 * g) * (1.0 / sa)
    return sp * x0 + s1p * g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1)}}
    shape, ranges, ov, gs, phi = (1, 4, 24, 72, 128), ((0, 16), (8, 24)), 8, 7.5, 0.7
    _, C, T, H, W = shape
    g = torch.Generator().manual_seed(0)
    z = torch.randn(shape, generator=g).half().to(dev)
    prev = torch.randn(shape, generator=g).half().to(dev)
    eps2 = torch.randn(2, *shape[1:], generator=g).half().to(dev)
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
    fac = ops.rescale_factors(phi)
    part = ops.cfg_rescale_stats(eps2, gs).clone()
    copart = ops.cofuse_cfg_rescale_stats(z, packed, rows, wn, gs).clone()
    got = ops.cfg_rescale_ddim_step(eps2, z, gs, fac, cd, part)
    want = torch_chain(eps2, z, gs, phi, cd)
    it = a.iters

    def pair_ddim():
        ops.cfg_rescale_ddim_step(eps2, z, gs, fac, cd, ops.cfg_rescale_stats(eps2, gs), out=out)

    def pair_dpm():
        ops.cfg_rescale_dpm_step(eps2, z, gs, fac, cp, ops.cfg_rescale_stats(eps2, gs), x0_prev=prev, x0_out=x0, out=out)

    def pair_co_ddim():
        ops.cofuse_cfg_rescale_ddim_step(z, packed, rows, wn, gs, fac, cd, ops.cofuse_cfg_rescale_stats(z, packed, rows, wn, gs), out=out)

    def pair_co_dpm():
        ops.cofuse_cfg_rescale_dpm_step(z, packed, rows, wn, gs, fac, cp, ops.cofuse_cfg_rescale_stats(z, packed, rows, wn, gs),
                                        x0_prev=prev, x0_out=x0, out=out)
    r = {"latent": list(shape), "windows": [list(w) for w in ranges], "guidance_scale": gs, "guidance_rescale": phi,
         "partial_rows": int(part.shape[0]), "cofuse_partial_rows": int(copart.shape[0]),
         "max_abs_diff_to_torch_chain": float((got.float() - want.float()).abs().max()),
         "stats": timed(lambda: ops.cfg_rescale_stats(eps2, gs), it),
         "rescale_ddim_step_alone": timed(lambda: ops.cfg_rescale_ddim_step(eps2, z, gs, fac, cd, part, out=out), it),
         "stats_plus_ddim_step": timed(pair_ddim, it),
         "stats_plus_dpm_step": timed(pair_dpm, it),
         "cofuse_stats": timed(lambda: ops.cofuse_cfg_rescale_stats(z, packed, rows, wn, gs), it),
         "cofuse_stats_plus_ddim_step": timed(pair_co_ddim, it),
         "cofuse_stats_plus_dpm_step": timed(pair_co_dpm, it),
         "plain_cfg_ddim_step": timed(lambda: ops.cfg_ddim_step(eps2, z, gs, cd, out=out), it),
         "plain_cfg_dpm_step": timed(lambda: ops.cfg_dpm_step(eps2, z, gs, cp, x0_prev=prev, x0_out=x0, out=out), it),
         "plain_cofuse_cfg_ddim_step": timed(lambda: ops.cofuse_cfg_ddim_step(z, packed, rows, wn, gs, cd, out=out), it),
         "plain_cofuse_cfg_dpm_step": timed(lambda: ops.cofuse_cfg_dpm_step(z, packed, rows, wn, gs, cp, x0_prev=prev, x0_out=x0, out=out), it),
         "torch_chain": timed(lambda: torch_chain(eps2, z, gs, phi, cd), it)}
    for new, old in (("stats_plus_ddim_step", "plain_cfg_ddim_step"), ("stats_plus_dpm_step", "plain_cfg_dpm_step"),
                     ("cofuse_stats_plus_ddim_step", "plain_cofuse_cfg_ddim_step"), ("cofuse_stats_plus_dpm_step", "plain_cofuse_cfg_dpm_step")):
        r[new + "_over_plain"] = round(r[new]["median_ms"] / r[old]["median_ms"], 2)
    r["torch_chain_over_stats_plus_ddim_step"] = round(r["torch_chain"]["median_ms"] / r["stats_plus_ddim_step"]["median_ms"], 2)
    res["rescale"] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
