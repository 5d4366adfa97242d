#!/usr/bin/env python3
"""Time the strided-window kernels (csrc/codenoise.hip, its `costride_tab`) at the headline latent (1,4,24,72,128) with the
two-level plan of the default two-rank job: 24 frames, chunk 16, overlap 8 -> level 0 (0, 20, 1), (12, 12, 1) and level 1
(0, 12, 2), (1, 12, 2): 56 window-frames per step instead of 32.  Measured numbers only: medians of `--iters` (default 20)
event-timed calls, each taken in `--rounds` (default 3) rounds that alternate between a strided kernel and its sibling, so that
the spread between a kernel's own rounds stands beside the difference between the two.

  * the strided DDIM step (`vdx_costride_cfg_ddim_step_f16`) and the strided DPM-Solver++ second-order step;
  * in the same process, `cofuse_cfg_ddim_step` / `cofuse_cfg_dpm_step` on the level-0 plan (32 window-frames);
  * the same strided expressions as chains of torch-GPU ops (per window an `index_add_` of its fp32 products in ascending order,
    then the fp16 chain, one rounding per operation), whose values are ASSERTED equal to the kernels';
  * `cfg_input_stride` for (0, 12, 2) against `cfg_input_window` for (0, 12) and against `index_select` + `cfg_input`.
`--merge FILE...`: instead of timing, copy the "step" sections of `tools/codenoise_bench.py` / `tools/coloop_bench.py` outputs
taken on the parent commit and on this one into the record (`--out`), under "shared_kernel": the readings and the tools' own
round-to-round spread, the margin by which the flat and ring steps may differ.
Prints one JSON line; `--out FILE` also writes it.

    python tools/costride_bench.py [--iters 20] [--rounds 3] [--out profiles/costride_bench.json]"""
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
from vdx.codenoise import stride_plan, stride_table, window_table  # noqa: E402
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


def r16(x):
    return x.half().float()


def torch_fuse(z, wins, table, wn, gs):
    """The strided fuse and the CFG combine as torch ops on GPU tensors -> the guided noise, fp32 holding fp16 values.  The
    accumulator starts at zero and the windows are added in ascending order: 0 + p is p, so the sums are the kernel's."""
    acc = torch.zeros((2,) + tuple(z.shape[1:]), dtype=torch.float32, device=z.device)
    for k, ((s, n, d), w) in enumerate(zip(table, wins)):
        idx = s + d * torch.arange(n, device=z.device)
        acc.index_add_(2, idx, w.float() * wn[k].index_select(0, idx).view(1, 1, -1, 1, 1))
    u, c = r16(acc).chunk(2)
    return r16(u + r16(gs * r16(c - u)))


def torch_ddim_chain(z, wins, table, wn, gs, coeffs):
    s1, sa, sp, s1p = (float(np.float32(c)) for c in coeffs)
    e, x = torch_fuse(z, wins, table, wn, gs), z.float()
    x0 = r16(r16(x - r16(s1 * e)) * float(np.float32(1.0) / np.float32(sa)))
    return r16(r16(sp * x0) + r16(s1p * e)).half()


def torch_dpm_chain(z, wins, table, wn, gs, coeffs, prev):
    """DPM-Solver++ second order from the kernel's six coefficients (include/vdx.h) -> (z', x0)."""
    s0, inv_a0, cx, d0, d1, inv_r0 = (float(np.float32(c)) for c in coeffs)
    e, x = torch_fuse(z, wins, table, wn, gs), z.float()
    x0 = r16(r16(x - r16(s0 * e)) * inv_a0)
    new = r16(r16(cx * x) - r16(-d0 * x0))
    diff = r16(inv_r0 * r16(x0 - prev.float()))
    return r16(new - r16(-d1 * diff)).half(), x0.half()


def ratio(res, a, b):
    return round(res[a]["median_ms"] / res[b]["median_ms"], 3)


def merge(paths):
    """{label: the "step" section's timed entries} of codenoise_bench / coloop_bench outputs named LABEL=FILE."""
    out = {}
    for item in paths:
        label, path = item.split("=", 1)
        with open(path) as f:
            rec = json.loads(f.readline())
        out[label] = {"source_sha": rec.get("source_sha"), "device": rec.get("device"),
                      **{k: v for k, v in rec["step"].items() if isinstance(v, dict) and "median_ms" in v}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="*", default=None, metavar="LABEL=FILE")
    a = ap.parse_args()
    if a.merge is not None:
        with open(a.out) as f:
            res = json.loads(f.readline())
        res["shared_kernel"] = merge(a.merge)
        line = json.dumps(res)
        print(line)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        return
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1)}}
    shape = (1, 4, 24, 72, 128)
    _, C, T, H, W = shape
    sp = stride_plan(T, 2, 16, 8, "coherent", 2)
    assert sp.windows == ((0, 20, 1), (12, 12, 1), (0, 12, 2), (1, 12, 2))
    g = torch.Generator().manual_seed(0)
    z = torch.randn(shape, generator=g).half().to(dev)
    prev = torch.randn(shape, generator=g).half().to(dev)
    slot = 2 * C * sp.chunk * H * W
    packed = torch.randn(4 * slot, generator=g).half().to(dev)       # both plans read their windows out of the same slots
    stab, ftab = stride_table(sp, T), window_table(sp.base, T)
    srows, swn = stab.rows(1, 4, slot), stab.wn.to(dev)
    frows, fwn = ftab.rows(1, 4, slot), ftab.wn.to(dev)
    table = [r[1:] for r in srows]
    wins = [packed[off:off + 2 * C * n * H * W].view(2, C, n, H, W) for off, _, n, _ in srows]
    d = DDIMScheduler()
    d.set_timesteps(50)
    cd = d.coefficients(d._host_timesteps[25])
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(25)
    cp = s.coefficients(12, True)
    out, x0 = torch.empty_like(z), torch.empty_like(z)
    n = z.numel()
    assert torch.equal(ops.costride_cfg_ddim_step(z, packed, srows, swn, 7.5, cd), torch_ddim_chain(z, wins, table, swn, 7.5, cd))
    got, got_x0 = ops.costride_cfg_dpm_step(z, packed, srows, swn, 7.5, cp, x0_prev=prev)
    want, want_x0 = torch_dpm_chain(z, wins, table, swn, 7.5, cp, prev)
    assert torch.equal(got, want) and torch.equal(got_x0, want_x0)
    step = {"latent": list(shape), "strided_windows": [list(w) for w in table], "flat_windows": [list(r) for r in sp.base.ranges],
            "window_table_bytes_by_value": 64 * (8 + 4 + 4 + 4),
            "strided_halves_read": sum(w.numel() for w in wins) + n, "flat_halves_read": sum(2 * C * (e - s_) * H * W for s_, e in sp.base.ranges) + n,
            "halves_written": n, "equal_to_torch_chains": True}
    step.update(rounds({
        "costride_cfg_ddim_step": lambda: ops.costride_cfg_ddim_step(z, packed, srows, swn, 7.5, cd, out=out),
        "cofuse_cfg_ddim_step": lambda: ops.cofuse_cfg_ddim_step(z, packed, frows, fwn, 7.5, cd, out=out),
        "costride_cfg_dpm_step": lambda: ops.costride_cfg_dpm_step(z, packed, srows, swn, 7.5, cp, x0_prev=prev, x0_out=x0, out=out),
        "cofuse_cfg_dpm_step": lambda: ops.cofuse_cfg_dpm_step(z, packed, frows, fwn, 7.5, cp, x0_prev=prev, x0_out=x0, out=out),
        "torch_ddim_chain": lambda: torch_ddim_chain(z, wins, table, swn, 7.5, cd),
        "torch_dpm_chain": lambda: torch_dpm_chain(z, wins, table, swn, 7.5, cp, prev)}, a.iters, a.rounds))
    step["costride_over_cofuse_ddim"] = ratio(step, "costride_cfg_ddim_step", "cofuse_cfg_ddim_step")
    step["costride_over_cofuse_dpm"] = ratio(step, "costride_cfg_dpm_step", "cofuse_cfg_dpm_step")
    step["torch_chain_over_costride_ddim"] = ratio(step, "torch_ddim_chain", "costride_cfg_ddim_step")
    step["torch_chain_over_costride_dpm"] = ratio(step, "torch_dpm_chain", "costride_cfg_dpm_step")
    res["step"] = step
    ctx = torch.randn(1, C, 1, H, W, generator=g).half().to(dev)
    s0, n0, d0 = table[2]
    x2 = torch.empty((2, C, n0, H, W), dtype=torch.float16, device=dev)
    idx = (s0 + d0 * torch.arange(n0)).to(dev)
    a_ = ops.cfg_input_stride(z, ctx, 0.35, s0, n0, d0)
    b_ = ops.cfg_input(z.index_select(2, idx).contiguous(), ctx, 0.35)
    assert torch.equal(a_, b_)
    inp = {"strided_window": [s0, n0, d0], "flat_window": [s0, s0 + n0], "equal": True}
    inp.update(rounds({
        "cfg_input_stride": lambda: ops.cfg_input_stride(z, ctx, 0.35, s0, n0, d0, out=x2),
        "cfg_input_window": lambda: ops.cfg_input_window(z, ctx, 0.35, s0, s0 + n0, out=x2),
        "index_select_plus_cfg_input": lambda: ops.cfg_input(z.index_select(2, idx).contiguous(), ctx, 0.35, out=x2)},
        a.iters, a.rounds))
    inp["stride_over_window"] = ratio(inp, "cfg_input_stride", "cfg_input_window")
    inp["index_select_over_stride"] = ratio(inp, "index_select_plus_cfg_input", "cfg_input_stride")
    res["input"] = inp
    res["note"] = "kernel times only; no whole-video figure was taken"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
