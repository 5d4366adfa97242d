#!/usr/bin/env python3
"""Time the dynamic-thresholding kernels (csrc/dynthresh.hip) at the headline latent (1,4,24,72,128).  Measured numbers only:
medians of `--iters` (default 20) event-timed calls taken in alternating rounds (every round times every candidate once, so a
drift of the box falls on all of them alike).

  * each of the four launches on its own (sums, histogram, select, step);
  * statistics + step for DDIM and for DPM-Solver++ (second order), against the plain fused steps timed in the same process;
  * the same expression as a chain of torch-GPU ops (`torch.sort` for the quantile), its values asserted equal first;
  * the co-fused pair with two 16-frame windows that overlap by 8.
One histogram layout is built and measured: global bins with a lane's runs of equal bins merged into one add.
Prints one JSON line; `--out FILE` also writes it.

    python tools/dynthresh_bench.py [--iters 20] [--out profiles/dynthresh_bench.json]"""
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


def timed_rounds(cands, iters, warmup=5):
    """{name: fn} -> {name: {"median_ms", "min_ms", "iters"}}: `iters` rounds, each timing every candidate once, in order."""
    for _ in range(warmup):
        for fn in cands.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in cands}
    for _ in range(iters):
        for name, fn in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {name: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "iters": iters}
            for name, v in ms.items()}


def torch_chain(eps2, z, gs, ms, k, f, coeffs):
    """The definition as torch ops on fp16 GPU tensors with host scalars: every fp16 tensor op rounds once, as the kernels' lines do."""
    s1, sa, sp, s1p = coeffs
    u, c = eps2.chunk(2)
    C = u.shape[1]
    g = (u + gs * (c - u)).reshape(C, -1)
    l = (u + ms * (c - u)).reshape(C, -1)
    M = g.shape[1]
    mg = (g.double().sum(1, keepdim=True) / M).cpu().numpy().astype(np.float16)       # ONE rounding: numpy converts directly
    ml = (l.double().sum(1, keepdim=True) / M).cpu().numpy().astype(np.float16)
    mg, ml = torch.from_numpy(mg).to(g.device), torch.from_numpy(ml).to(g.device)
    d, e = g - mg, l - ml
    ref_lo = (e.view(torch.int16) & 0x7fff).max(dim=1, keepdim=True).values
    a = torch.sort(d.view(torch.int16) & 0x7fff, dim=1).values
    lo, hi = a[:, k:k + 1], a[:, min(k + 1, M - 1):min(k + 1, M - 1) + 1]
    if f == 0.0:
        ref_hi = lo
    else:
        lof, hif = lo.view(torch.float16).float(), hi.view(torch.float16).float()
        ref_hi = (lof + f * (hif - lof)).half().view(torch.int16)
    s = torch.maximum(ref_lo, ref_hi).view(torch.float16)
    ref_lo = ref_lo.contiguous().view(torch.float16)
    dc = torch.where(d > s, s.expand_as(d), torch.where(d < -s, (-s).expand_as(d), d))
    g2 = (((dc / s) * ref_lo) + mg).reshape(z.shape)
    x0 = (z - s1 * g2) * (1.0 / sa)
    return sp * x0 + s1p * g2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1)}}
    shape, ranges, ov, gs, ms, q = (1, 4, 24, 72, 128), ((0, 16), (8, 24)), 8, 15.0, 7.0, 0.995
    _, C, T, H, W = shape
    M = T * H * W
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
    fac = ops.mimic_factors(ms, q, M)
    ws = ops.cfg_mimic_stats(eps2, gs, fac).clone()
    cows = ops.cofuse_cfg_mimic_stats(z, packed, rows, wn, gs, fac).clone()
    got = ops.cfg_mimic_ddim_step(eps2, z, gs, cd, ws)
    want = torch_chain(eps2, z, gs, fac[0], fac[1], fac[2], cd)
    differ = int((got.view(torch.int16) != want.view(torch.int16)).sum())
    assert differ == 0, f"{differ} of {got.numel()} elements differ from the torch chain"
    hist = ops.mimic_ws_views(ws, C)["hist"]
    it = a.iters

    def stats(stages):
        return lambda: ops.cfg_mimic_stats(eps2, gs, fac, ws=ws, stages=stages)

    def co_stats(stages):
        return lambda: ops.cofuse_cfg_mimic_stats(z, packed, rows, wn, gs, fac, ws=cows, stages=stages)
    cands = {
        "sums": stats(1), "histogram_global_bins": stats(2), "select": stats(4), "stats": stats(7),
        "mimic_ddim_step_alone": lambda: ops.cfg_mimic_ddim_step(eps2, z, gs, cd, ws, out=out),
        "stats_plus_ddim_step": lambda: ops.cfg_mimic_ddim_step(eps2, z, gs, cd, ops.cfg_mimic_stats(eps2, gs, fac, ws=ws), out=out),
        "stats_plus_dpm_step": lambda: ops.cfg_mimic_dpm_step(eps2, z, gs, cp, ops.cfg_mimic_stats(eps2, gs, fac, ws=ws), x0_prev=prev,
                                                              x0_out=x0, out=out),
        "plain_cfg_ddim_step": lambda: ops.cfg_ddim_step(eps2, z, gs, cd, out=out),
        "plain_cfg_dpm_step": lambda: ops.cfg_dpm_step(eps2, z, gs, cp, x0_prev=prev, x0_out=x0, out=out),
        "cofuse_sums": co_stats(1), "cofuse_histogram_global_bins": co_stats(2), "cofuse_stats": co_stats(7),
        "cofuse_stats_plus_ddim_step": lambda: ops.cofuse_cfg_mimic_ddim_step(z, packed, rows, wn, gs, cd, co_stats(7)(), out=out),
        "cofuse_stats_plus_dpm_step": lambda: ops.cofuse_cfg_mimic_dpm_step(z, packed, rows, wn, gs, cp, co_stats(7)(), x0_prev=prev,
                                                                            x0_out=x0, out=out),
        "plain_cofuse_cfg_ddim_step": lambda: ops.cofuse_cfg_ddim_step(z, packed, rows, wn, gs, cd, out=out),
        "plain_cofuse_cfg_dpm_step": lambda: ops.cofuse_cfg_dpm_step(z, packed, rows, wn, gs, cp, x0_prev=prev, x0_out=x0, out=out),
        "torch_chain": lambda: torch_chain(eps2, z, gs, fac[0], fac[1], fac[2], cd),
    }
    r = {"latent": list(shape), "windows": [list(w) for w in ranges], "guidance_scale": gs, "cfg_mimic": ms, "cfg_mimic_percentile": q,
         "rank": [fac[1], fac[2]], "elements_per_channel": M, "workspace_bytes": int(ws.numel()),
         "occupied_bins_per_channel": [int(v) for v in (hist != 0).sum(1).cpu()],
         "largest_bin_per_channel": [int(v) for v in hist.max(1).values.cpu()],
         "elements_equal_to_torch_chain": int(got.numel()), "histogram_layouts_measured": ["global bins, runs of equal bins merged"]}
    r.update(timed_rounds(cands, it))
    for new, old in (("stats_plus_ddim_step", "plain_cfg_ddim_step"), ("stats_plus_dpm_step", "plain_cfg_dpm_step"),
                     ("cofuse_stats_plus_ddim_step", "plain_cofuse_cfg_ddim_step"), ("cofuse_stats_plus_dpm_step", "plain_cofuse_cfg_dpm_step")):
        r[new + "_over_plain"] = round(r[new]["median_ms"] / r[old]["median_ms"], 2)
    r["torch_chain_over_stats_plus_ddim_step"] = round(r["torch_chain"]["median_ms"] / r["stats_plus_ddim_step"]["median_ms"], 2)
    res["dynthresh"] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
