#!/usr/bin/env python3
"""Time the ring-window kernels (csrc/codenoise.hip, its RING flag) at the headline latent (1,4,24,72,128) with the looping job's default plan:
two ring windows of 16 frames, (0, 16) and (12, 28), the second wrapping into frames 0..3.  Measured numbers only: medians of
`--iters` (default 20) event-timed calls, each taken in `--rounds` (default 3) rounds that alternate between a ring kernel and
its sibling, so that the spread between a kernel's own rounds stands beside the difference between the two.

  * the ring DDIM step (`vdx_coloop_cfg_ddim_step_f16`) and the ring DPM-Solver++ second-order step;
  * in the same process, `cofuse_cfg_ddim_step` / `cofuse_cfg_dpm_step` on the non-wrapping plan of that shape, (0, 16), (12, 24);
  * the same ring expression as a chain of torch-GPU ops (`index_select` per window, fp32 weighted sums, then the fp16 chain);
  * `cfg_input_loop` for the wrapping window against `cfg_input_window` for (8, 24) and against `torch.roll` + slice-copy +
    `cfg_input`.
Prints one JSON line; `--out FILE` also writes it.

    python tools/coloop_bench.py [--iters 20] [--rounds 3] [--out profiles/coloop_bench.json]"""
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
from vdx.codenoise import loop_plan, loop_table, window_table  # noqa: E402
from vdx.planner import plan  # noqa: E402
from vdx.scheduler import DDIMScheduler, DPMSolverMultistepScheduler  # noqa: E402


def median_ms(fn, iters, warmup=5):
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
    return float(np.median(ms))


def rounds(fns, iters, n):
    """{name: fn} timed in n alternating rounds -> {name: {"median_ms": median of the rounds' medians, "rounds_ms": [...],
    "spread_ms": max - min of the rounds}}."""
    got = {k: [] for k in fns}
    for _ in range(n):
        for k, fn in fns.items():
            got[k].append(median_ms(fn, iters))
    return {k: {"median_ms": round(float(np.median(v)), 4), "rounds_ms": [round(x, 4) for x in v],
                "spread_ms": round(max(v) - min(v), 4), "iters": iters} for k, v in got.items()}


def torch_ring_chain(z, wins, table, wn, gs, coeffs):
    """Ring fuse + CFG + DDIM as torch ops on GPU tensors: per window an index of its frames on the ring, fp32 accumulators, then
    fp16 tensors with host scalars."""
    s1, sa, sp, s1p = coeffs
    T = z.shape[2]
    acc = torch.zeros((2,) + tuple(z.shape[1:]), dtype=torch.float32, device=z.device)
    for k, ((s, n), w) in enumerate(zip(table, wins)):
        idx = (s + torch.arange(n, device=z.device)) % T
        acc.index_add_(2, idx, w.float() * wn[k].index_select(0, idx).view(1, 1, -1, 1, 1))
    u, c = acc.half().chunk(2)
    eps = u + gs * (c - u)
    x0 = (z - s1 * eps) * (1.0 / sa)
    return sp * x0 + s1p * eps


def ratio(res, a, b):
    return round(res[a]["median_ms"] / res[b]["median_ms"], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1)}}
    shape = (1, 4, 24, 72, 128)
    _, C, T, H, W = shape
    ring, flat = loop_plan(T, 1, 16, 4), plan(T, 1, 16, 4)
    assert ring.ranges == ((0, 16), (12, 28)) and flat.ranges == ((0, 16), (12, 24))
    g = torch.Generator().manual_seed(0)
    z = torch.randn(shape, generator=g).half().to(dev)
    prev = torch.randn(shape, generator=g).half().to(dev)
    slot = 2 * C * 16 * H * W
    packed = torch.randn(2 * slot, generator=g).half().to(dev)       # both plans read their windows out of the same two slots
    rtab, ftab = loop_table(ring, T), window_table(flat, T)
    rrows, rwn = rtab.rows(1, 2, slot), rtab.wn.to(dev)
    frows, fwn = ftab.rows(1, 2, slot), ftab.wn.to(dev)
    table = [(s, n) for _, s, n in rrows]
    wins = [packed[off:off + 2 * C * n * H * W].view(2, C, n, H, W) for off, _, n in rrows]
    d = DDIMScheduler()
    d.set_timesteps(50)
    cd = d.coefficients(d._host_timesteps[25])
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(25)
    cp = s.coefficients(12, True)
    out, x0 = torch.empty_like(z), torch.empty_like(z)
    n = z.numel()
    got = ops.coloop_cfg_ddim_step(z, packed, rrows, rwn, 7.5, cd)
    want = torch_ring_chain(z, wins, table, rwn, 7.5, cd)
    step = {"latent": list(shape), "ring_windows": [[s_, n_] for s_, n_ in table], "flat_windows": [list(r) for r in flat.ranges],
            "ring_halves_read": sum(w.numel() for w in wins) + n, "halves_written": n,
            "max_abs_diff_to_torch_chain": float((got.float() - want.float()).abs().max())}
    step.update(rounds({
        "coloop_cfg_ddim_step": lambda: ops.coloop_cfg_ddim_step(z, packed, rrows, rwn, 7.5, cd, out=out),
        "cofuse_cfg_ddim_step": lambda: ops.cofuse_cfg_ddim_step(z, packed, frows, fwn, 7.5, cd, out=out),
        "coloop_cfg_dpm_step": lambda: ops.coloop_cfg_dpm_step(z, packed, rrows, rwn, 7.5, cp, x0_prev=prev, x0_out=x0, out=out),
        "cofuse_cfg_dpm_step": lambda: ops.cofuse_cfg_dpm_step(z, packed, frows, fwn, 7.5, cp, x0_prev=prev, x0_out=x0, out=out),
        "torch_ring_chain": lambda: torch_ring_chain(z, wins, table, rwn, 7.5, cd)}, a.iters, a.rounds))
    step["coloop_over_cofuse_ddim"] = ratio(step, "coloop_cfg_ddim_step", "cofuse_cfg_ddim_step")
    step["coloop_over_cofuse_dpm"] = ratio(step, "coloop_cfg_dpm_step", "cofuse_cfg_dpm_step")
    step["torch_chain_over_coloop_ddim"] = ratio(step, "torch_ring_chain", "coloop_cfg_ddim_step")
    res["step"] = step
    ctx = torch.randn(1, C, 1, H, W, generator=g).half().to(dev)
    s0, n0 = table[1]
    x2 = torch.empty((2, C, n0, H, W), dtype=torch.float16, device=dev)
    a_ = ops.cfg_input_loop(z, ctx, 0.35, s0, n0)
    b_ = ops.cfg_input(z.roll(-s0, 2)[:, :, :n0].contiguous(), ctx, 0.35)
    inp = {"ring_window": [s0, n0], "flat_window": [T - n0, T], "equal": bool(torch.equal(a_, b_))}
    inp.update(rounds({
        "cfg_input_loop": lambda: ops.cfg_input_loop(z, ctx, 0.35, s0, n0, out=x2),
        "cfg_input_window": lambda: ops.cfg_input_window(z, ctx, 0.35, T - n0, T, out=x2),
        "roll_slice_copy_plus_cfg_input": lambda: ops.cfg_input(z.roll(-s0, 2)[:, :, :n0].contiguous(), ctx, 0.35, out=x2)},
        a.iters, a.rounds))
    inp["loop_over_window"] = ratio(inp, "cfg_input_loop", "cfg_input_window")
    res["input"] = inp
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
