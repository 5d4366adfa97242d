#!/usr/bin/env python3
"""Time regional prompts (csrc/region.hip, the UNet's `regions=` path) on synthetic Zeroscope weights.  Measured numbers only:
medians of `--iters` (default 20) event-timed calls, each taken in `--rounds` (default 3) rounds that alternate between the
entries of a group, so that the spread between an entry's own rounds stands beside the difference between two entries.

  * the blend kernel at (16 frames, 72 x 128 pixels, C = 320) with R = 3 regions, hard masks (every cell one owner) and soft masks
    (overlapping ramps), against the same expression as a torch-GPU chain (equal values asserted); time and achieved GB/s of the
    bytes each form has to move: the kernel reads the non-zero-weight inputs of a row only, the chain reads every input;
  * one UNet call on the 16-frame window of the headline latent with 0, 1 and 3 regions, the 0-region call read before and after:
    that spread is the noise floor against which the regional cost stands.
No whole-video figure is taken.  Prints one JSON line; `--out FILE` also writes it.

    python tools/region_bench.py [--iters 20] [--rounds 3] [--out profiles/region_bench.json]"""
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
from vdx.region import region_plan  # noqa: E402
from vdx.unet3d import UNet3DConditionModel, UNet3DConfig  # noqa: E402
from vdx.weights import synthetic_state_dict  # noqa: E402


def median_ms(fn, iters, warmup=3):
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
    got = {k: [] for k in fns}
    for _ in range(n):
        for k, fn in fns.items():
            got[k].append(median_ms(fn, iters))
    return {k: {"median_ms": round(float(np.median(v)), 4), "rounds_ms": [round(x, 4) for x in v],
                "spread_ms": round(max(v) - min(v), 4), "iters": iters} for k, v in got.items()}


def masks(kind, T, H, W):
    """Three regions in pixels.  hard: three 0 / 255 quarters on 64-pixel blocks (the base keeps the fourth); soft: three
    overlapping ramps, one of them moving with the frames."""
    x = np.arange(W, dtype=np.float64)[None, :].repeat(H, 0)
    y = np.arange(H, dtype=np.float64)[:, None].repeat(W, 1)
    if kind == "hard":
        q = [np.zeros((H, W), np.uint8) for _ in range(3)]
        q[0][:H // 2 // 64 * 64, :W // 2] = 255
        q[1][:H // 2 // 64 * 64, W // 2:] = 255
        q[2][H // 2 // 64 * 64:, :W // 2] = 255
        return q
    ramp = lambda v: np.round(255 * np.clip(v, 0, 1)).astype(np.uint8)      # noqa: E731
    return [ramp((W / 2 - x) / (W / 4)), ramp((H / 2 - y) / (H / 4)),
            np.stack([ramp((W / 8 - np.hypot(x - W * (t + 1) / (T + 1), y - H / 2)) / (W / 16)) for t in range(T)])]


def torch_chain(subs, table, L):
    """The kernel's expression with torch ops on the GPU: fp32 products and sums in ascending j, zero weights skipped through
    `where`, exact ones selected."""
    w = table[:L].reshape(-1, table.shape[2])
    acc = torch.zeros(subs[0].shape, dtype=torch.float32, device=subs[0].device)
    started = torch.zeros(w.shape[0], dtype=torch.bool, device=w.device)
    for j, x in enumerate(subs):
        use = w[:, j] != 0
        term = w[:, j:j + 1] * x.float()
        acc = torch.where((use & ~started)[:, None], term, torch.where(use[:, None], acc + term, acc))
        started |= use
    out = acc.half()
    for j in reversed(range(len(subs))):
        out = torch.where((w[:, j] == 1.0)[:, None], subs[j], out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1)}, "whole_video": "not measured"}
    L, h, w, C, N, D = 16, 72, 128, 320, 77, 1024
    g = torch.Generator().manual_seed(0)
    M = L * h * w
    subs = [torch.randn(M, C, generator=g).half().to(dev) for _ in range(4)]
    blend = {"rows": M, "C": C, "inputs": 4}
    plans = {}
    for kind in ("hard", "soft"):
        plan = plans[kind] = region_plan([(m, "") for m in masks(kind, L, 8 * h, 8 * w)], L, h, w, 4).to(dev)
        table = plan.tables[0]
        out = torch.empty_like(subs[0])
        want = torch_chain(subs, table, L)
        got = ops.region_blend(subs, table, 0, L, out=out)
        nonzero = int((table != 0).sum())                          # (row, input) pairs the kernel reads
        r = rounds({"kernel": lambda: ops.region_blend(subs, table, 0, L, out=out), "torch_chain": lambda: torch_chain(subs, table, L)},
                   a.iters, a.rounds)
        moved = (nonzero + M) * C * 2 + table.numel() * 4
        moved_chain = (4 + 1) * M * C * 2 + table.numel() * 4       # the least a chain that cannot skip must move: every input once
        r["kernel"]["bytes"], r["kernel"]["GBps"] = moved, round(moved / r["kernel"]["median_ms"] / 1e6, 1)
        r["torch_chain"]["bytes_at_least"], r["torch_chain"]["GBps_of_that"] = moved_chain, round(moved_chain / r["torch_chain"]["median_ms"] / 1e6, 1)
        r["equal"] = bool(torch.equal(got, want))
        r["nonzero_weights_per_row"] = round(nonzero / M, 3)
        r["chain_over_kernel"] = round(r["torch_chain"]["median_ms"] / r["kernel"]["median_ms"], 2)
        assert r["equal"], kind
        blend[kind] = r
    res["blend"] = blend
    del subs
    cfg = UNet3DConfig.zeroscope()
    m = UNet3DConditionModel(cfg).load_diffusers_state_dict(synthetic_state_dict(cfg, 1234, dev), device=dev)
    lat = torch.randn(1, 4, L, h, w, generator=g).half().to(dev)
    x = ops.cfg_input(lat, None, 0.0)
    text = torch.randn(2, N, D, generator=g).half().to(dev)
    rtext = torch.randn(3, N, D, generator=g).half().to(dev)
    soft = masks("soft", L, 8 * h, 8 * w)
    one = (rtext[:1].contiguous(), region_plan([(soft[0], "")], L, h, w, 4).to(dev), (0, L, 1, False))
    three = (rtext, plans["soft"], (0, L, 1, False))
    m.text_cache_slots = 3                                           # every timed call below is a cache hit
    call = lambda regions: m(x, 500, encoder_hidden_states=text, regions=regions).sample      # noqa: E731
    unet = {"window": [2, 4, L, h, w]}
    unet.update(rounds({"regions_0_before": lambda: call(None), "regions_1": lambda: call(one), "regions_3": lambda: call(three),
                        "regions_0_after": lambda: call(None)}, a.iters, a.rounds))
    r0 = [unet["regions_0_before"]["median_ms"], unet["regions_0_after"]["median_ms"]]
    unet["regions_0_spread_ms"] = round(abs(r0[0] - r0[1]), 4)
    unet["regions_1_minus_0_ms"] = round(unet["regions_1"]["median_ms"] - float(np.mean(r0)), 4)
    unet["regions_3_minus_0_ms"] = round(unet["regions_3"]["median_ms"] - float(np.mean(r0)), 4)
    res["unet_call"] = unet
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
