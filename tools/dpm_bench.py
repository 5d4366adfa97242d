#!/usr/bin/env python3
"""Time the DPM-Solver++ (2M) sampler (vdx/scheduler.py `DPMSolverMultistepScheduler`, csrc/dpm.hip).  Measured numbers only.

  * the fused CFG + second-order step (`vdx_cfg_dpm_step_f16`) at the headline latent (1,4,24,72,128) against the same
    expression as a chain of torch-GPU elementwise ops on fp16 tensors (what a scheduler written in torch launches per step),
    and, for scale, the fused CFG + DDIM step (`vdx_cfg_ddim_step_f16`) at the same latent;
  * one 25-step `dpmpp_2m` denoise against one 50-step DDIM denoise of the same chunk through `DistributedVideoDiffuser.denoise`
    at the tiny golden UNet config (widths 64/128/128/128, 4 frames, 16x32 latent): the point is the number of UNet forwards,
    not the UNet.
Prints one JSON line; `--out FILE` also writes it.

    python tools/dpm_bench.py [--iters 50] [--out profiles/dpm_step_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vdx  # noqa: E402,F401
from vdx import ops  # noqa: E402
from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser  # noqa: E402
from vdx.scheduler import DDIMScheduler, DPMSolverMultistepScheduler  # noqa: E402

TINY = dict(ch=(64, 128, 128, 128), cross=128, in_heads=2)


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


def torch_chain(eps2, x, x0_prev, gs, c):
    """The step's expression as torch ops on fp16 GPU tensors with host scalars (coefficients as `coefficients()` gives them)."""
    s0, inv_a0, cx, c_d0, c_d1, inv_r0 = c
    u, cc = eps2.chunk(2)
    e = u + gs * (cc - u)
    x0 = (x - s0 * e) * inv_a0
    d1 = inv_r0 * (x0 - x0_prev)
    return cx * x - (-c_d0) * x0 - (-c_d1) * d1, x0


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(out)), 3), "min_ms": round(float(np.min(out)), 3), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3, help="repetitions of each whole denoise")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1)}}

    # ---- the step at the headline latent ----------------------------------------------------------------------------------
    shape = (1, 4, 24, 72, 128)
    g = torch.Generator().manual_seed(0)
    eps2 = torch.randn(2, *shape[1:], generator=g).half().to(dev)
    x = torch.randn(shape, generator=g).half().to(dev)
    prev = torch.randn(shape, generator=g).half().to(dev)
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(25)
    c = s.coefficients(12, True)
    out, x0 = torch.empty_like(x), torch.empty_like(x)
    got = ops.cfg_dpm_step(eps2, x, 7.5, c, x0_prev=prev, x0_out=x0, out=out)
    want = torch_chain(eps2, x, prev, 7.5, c)
    d = DDIMScheduler()
    d.set_timesteps(50)
    cd = d.coefficients(d._host_timesteps[25])
    n = x.numel()
    step = {"latent": list(shape), "halves_read": 4 * n, "halves_written": 2 * n,
            "equal_to_torch_chain": bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])),
            "fused_cfg_dpm_step": timed(lambda: ops.cfg_dpm_step(eps2, x, 7.5, c, x0_prev=prev, x0_out=x0, out=out), a.iters),
            "torch_chain": timed(lambda: torch_chain(eps2, x, prev, 7.5, c), a.iters),
            "fused_cfg_ddim_step": timed(lambda: ops.cfg_ddim_step(eps2, x, 7.5, cd, out=out), a.iters)}
    step["torch_chain_over_fused"] = round(step["torch_chain"]["median_ms"] / step["fused_cfg_dpm_step"]["median_ms"], 2)
    step["fused_gb_per_s"] = round(6 * n * 2 / (step["fused_cfg_dpm_step"]["median_ms"] * 1e-3) / 1e9, 1)
    res["step"] = step

    # ---- 25 steps of dpmpp_2m against 50 steps of DDIM, tiny UNet ------------------------------------------------------------
    from oracle.unet3d_ref import UNet3DConfig as RefCfg, synthetic_state_dict
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    sd = synthetic_state_dict(RefCfg.tiny(**TINY), seed=1234)
    unet = UNet3DConditionModel(UNet3DConfig(block_out_channels=TINY["ch"], cross_attention_dim=TINY["cross"],
                                             transformer_in_heads=TINY["in_heads"])).load_diffusers_state_dict(sd, device=dev)
    emb = torch.randn(2, 77, TINY["cross"], generator=g).half().to(dev)
    lat = torch.randn(1, 4, 4, 16, 32, generator=g).half().to(dev)
    den = {"unet": "tiny golden config " + str(TINY["ch"]), "latent": list(lat.shape)}
    for name, sched, steps in (("ddim_50", DDIMScheduler(), 50), ("dpmpp_2m_25", DPMSolverMultistepScheduler(), 25)):
        cfg = DiffuserConfig(num_frames=4, steps=steps, height=128, width=256, mode="hybrid", device="cuda",
                             scheduler="ddim" if name == "ddim_50" else "dpmpp_2m")
        dd = DistributedVideoDiffuser(cfg, unet, sched, emb[:1], emb[1:])
        den[name] = wall(lambda: dd.denoise(lat), a.reps)
        den[name]["steps"] = steps
    den["ddim_50_over_dpmpp_2m_25"] = round(den["ddim_50"]["median_ms"] / den["dpmpp_2m_25"]["median_ms"], 2)
    res["denoise"] = den
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
