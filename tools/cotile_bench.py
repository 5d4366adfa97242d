#!/usr/bin/env python3
"""Time the tiled co-denoising kernels (csrc/cotile.hip) at a (1,4,24,144,256) latent (1152 x 2048 pixels) with two 16-frame
windows that overlap by 8, times the 3 x 3 grid a 72 x 128 tile gives with the default overlap (18, 32): 18 windows.  Measured
numbers only: medians of `--iters` (default 20) event-timed calls.

  * the fused whole-clip DDIM step (`vdx_cotile_cfg_ddim_step_f16`) and DPM-Solver++ second-order step;
  * the same fuse + DDIM expression as a chain of torch-GPU ops (fp32 weighted sums per window, then the fp16 chain);
  * for scale per element, the existing temporal `vdx_cofuse_cfg_*_step_f16` at (1,4,24,72,128), the same two time windows;
  * `cfg_input_tile` against slice-copy + `cfg_input` for one tile of one 16-frame window.
Prints one JSON line; `--out FILE` also writes it.

    python tools/cotile_bench.py [--iters 20] [--out profiles/cotile_bench.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import vdx  # noqa: E402,F401
from codenoise_bench import timed  # noqa: E402
from vdx import ops  # noqa: E402
from vdx.codenoise import tile_plan, window_table  # noqa: E402
from vdx.planner import ChunkPlan  # noqa: E402
from vdx.scheduler import DDIMScheduler, DPMSolverMultistepScheduler  # noqa: E402


def torch_chain(z, wins, ranges, wn, tp, wyn, wxn, gs, coeffs):
    """Fuse + CFG + DDIM as torch ops on GPU tensors: one fp32 accumulator, a weighted add per window, then the fp16 chain."""
    s1, sa, sp, s1p = coeffs
    acc = torch.zeros((2,) + tuple(z.shape[1:]), dtype=torch.float32, device=z.device)
    for kt, (s, e) in enumerate(ranges):
        for ky, y0 in enumerate(tp.ys):
            wty = wn[kt, s:e].view(-1, 1, 1) * wyn[ky, y0:y0 + tp.th].view(1, -1, 1)
            for kx, x0 in enumerate(tp.xs):
                w = wty * wxn[kx, x0:x0 + tp.tw].view(1, 1, -1)
                acc[:, :, s:e, y0:y0 + tp.th, x0:x0 + tp.tw] += wins[kt][ky * len(tp.xs) + kx].float() * w
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
    shape, ranges, ov = (1, 4, 24, 144, 256), ((0, 16), (8, 24)), 8
    _, C, T, H, W = shape
    tp = tile_plan(H, W, 72, 128, 18, 32)
    g = torch.Generator().manual_seed(0)
    z = torch.randn(shape, generator=g).half().to(dev)
    prev = torch.randn(shape, generator=g).half().to(dev)
    wins = [[torch.randn(2, C, e - s, tp.th, tp.tw, generator=g).half().to(dev) for _ in range(tp.count)] for s, e in ranges]
    slot = wins[0][0].numel()
    packed = torch.cat([w.reshape(-1) for per in wins for w in per])
    tab = window_table(ChunkPlan(16, ov, ranges, 1), T)
    rows, wn = tab.rows(1, 2, tp.count * slot), tab.wn.to(dev)
    grid = tp.grid(slot, dev)
    d = DDIMScheduler()
    d.set_timesteps(50)
    cd = d.coefficients(d._host_timesteps[25])
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(25)
    cp = s.coefficients(12, True)
    out, x0 = torch.empty_like(z), torch.empty_like(z)
    n = z.numel()
    got = ops.cotile_cfg_ddim_step(z, packed, rows, wn, grid, 7.5, cd)
    want = torch_chain(z, wins, ranges, wn, tp, grid.wyn, grid.wxn, 7.5, cd)
    step = {"latent": list(shape), "time_windows": [list(r) for r in ranges], "tile": [tp.th, tp.tw], "rows": list(tp.ys),
            "columns": list(tp.xs), "windows": len(ranges) * tp.count, "halves_read": packed.numel() + n, "halves_written": n,
            "max_abs_diff_to_torch_chain": float((got.float() - want.float()).abs().max()),
            "fused_cotile_cfg_ddim_step": timed(lambda: ops.cotile_cfg_ddim_step(z, packed, rows, wn, grid, 7.5, cd, out=out), a.iters),
            "fused_cotile_cfg_dpm_step": timed(lambda: ops.cotile_cfg_dpm_step(z, packed, rows, wn, grid, 7.5, cp, x0_prev=prev,
                                                                                 x0_out=x0, out=out), a.iters),
            "torch_chain": timed(lambda: torch_chain(z, wins, ranges, wn, tp, grid.wyn, grid.wxn, 7.5, cd), a.iters)}
    step["torch_chain_over_fused"] = round(step["torch_chain"]["median_ms"] / step["fused_cotile_cfg_ddim_step"]["median_ms"], 2)
    step["fused_gb_per_s"] = round((packed.numel() + 2 * n) * 2 / (step["fused_cotile_cfg_ddim_step"]["median_ms"] * 1e-3) / 1e9, 1)
    res["step"] = step
    # the existing temporal step at the headline latent, the same two time windows: per element of the latent
    hs = (1, 4, 24, 72, 128)
    zh, ph = (torch.randn(hs, generator=g).half().to(dev) for _ in range(2))
    hw = [torch.randn(2, C, e - s, 72, 128, generator=g).half().to(dev) for s, e in ranges]
    hp = torch.cat([w.reshape(-1) for w in hw])
    hrows = tab.rows(1, 2, hw[0].numel())
    oh, xh = torch.empty_like(zh), torch.empty_like(zh)
    co = {"latent": list(hs),
          "cofuse_cfg_ddim_step": timed(lambda: ops.cofuse_cfg_ddim_step(zh, hp, hrows, wn, 7.5, cd, out=oh), a.iters),
          "cofuse_cfg_dpm_step": timed(lambda: ops.cofuse_cfg_dpm_step(zh, hp, hrows, wn, 7.5, cp, x0_prev=ph, x0_out=xh, out=oh), a.iters)}
    for name, tiled in (("ddim", "fused_cotile_cfg_ddim_step"), ("dpm", "fused_cotile_cfg_dpm_step")):
        co[f"{name}_ns_per_kilo_element"] = {"cotile": round(step[tiled]["median_ms"] * 1e6 / (n / 1e3), 3),
                                            "cofuse": round(co[f"cofuse_cfg_{name}_step"]["median_ms"] * 1e6 / (zh.numel() / 1e3), 3)}
    res["against_cofuse"] = co
    ctx = torch.randn(1, C, 1, H, W, generator=g).half().to(dev)
    s0, e0 = ranges[1]
    box = tp.boxes[4]                                                # the middle tile: rows 54.., columns 96..
    y0, th, x0_, tw = box
    x2 = torch.empty((2, C, e0 - s0, th, tw), dtype=torch.float16, device=dev)
    a_ = ops.cfg_input_tile(z, ctx, 0.35, s0, e0, *box)

    def slice_copy():
        return ops.cfg_input(z[:, :, s0:e0, y0:y0 + th, x0_:x0_ + tw].contiguous(), ctx[:, :, :, y0:y0 + th, x0_:x0_ + tw].contiguous(),
                             0.35, out=x2)
    res["input"] = {"window": [s0, e0], "box": list(box), "equal": bool(torch.equal(a_, slice_copy())),
                    "cfg_input_tile": timed(lambda: ops.cfg_input_tile(z, ctx, 0.35, s0, e0, *box, out=x2), a.iters),
                    "slice_copy_plus_cfg_input": timed(slice_copy, a.iters)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
