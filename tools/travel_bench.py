#!/usr/bin/env python3
"""Time prompt travel (csrc/travel.hip, the UNet's per-frame text path) on synthetic Zeroscope weights, for one UNet call on the
16-frame window of the headline latent (1,4,24,72,128).  Measured numbers only: medians of `--iters` (default 20) event-timed
calls, each taken in `--rounds` (default 3) rounds that alternate between the entries of a group, so that the spread between an
entry's own rounds stands beside the difference between two entries.

  * the UNet call with one text per sample (2, 77, 1024) before and after, and with a text per frame (2, 16, 77, 1024) between them,
    all cache hits (the job's steady state);
  * the per-frame call as a cache hit against a miss (a fresh tensor every call: 32 K / V projections at 32 items and the packs);
  * `ops.text_travel` for one window;
  * the pack kernel against `packing.pack_k5_kv`'s torch chain at 32 items.
Prints one JSON line; `--out FILE` also writes it.

    python tools/travel_bench.py [--iters 20] [--rounds 3] [--out profiles/travel_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vdx  # noqa: E402,F401
from vdx import ops, packing  # noqa: E402
from vdx.travel import travel_plan  # noqa: E402
from vdx.unet3d import TEXT_PAD, UNet3DConditionModel, UNet3DConfig  # noqa: E402
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
    """{name: fn} timed in n alternating rounds -> {name: {"median_ms": median of the rounds' medians, "rounds_ms": [...],
    "spread_ms": max - min of the rounds}}."""
    got = {k: [] for k in fns}
    for _ in range(n):
        for k, fn in fns.items():
            got[k].append(median_ms(fn, iters))
    return {k: {"median_ms": round(float(np.median(v)), 4), "rounds_ms": [round(x, 4) for x in v],
                "spread_ms": round(max(v) - min(v), 4), "iters": iters} for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1)}}
    T, L, H, W, N, D = 24, 16, 72, 128, 77, 1024
    cfg = UNet3DConfig.zeroscope()
    m = UNet3DConditionModel(cfg).load_diffusers_state_dict(synthetic_state_dict(cfg, 1234, dev), device=dev)
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(1, 4, L, H, W, generator=g).half().to(dev)
    x = ops.cfg_input(lat, None, 0.0)
    keys = torch.randn(3, N, D, generator=g).half().to(dev)
    uncond = torch.randn(N, D, generator=g).half().to(dev)
    lo, hi, w = travel_plan([(0, ""), (11, ""), (23, "")], T).to(dev)
    text4 = ops.text_travel(keys, uncond, lo, hi, w, 0, L)
    text3 = torch.stack([uncond, keys[0]]).contiguous()
    m.text_cache_slots = 2                                           # both texts stay: every timed call below is a hit
    call = lambda e: m(x, 500, encoder_hidden_states=e).sample      # noqa: E731
    unet = {"window": [2, 4, L, H, W], "text_rank3": list(text3.shape), "text_per_frame": list(text4.shape)}
    unet.update(rounds({"rank3_before": lambda: call(text3), "per_frame": lambda: call(text4), "rank3_after": lambda: call(text3)},
                       a.iters, a.rounds))
    r3 = [unet["rank3_before"]["median_ms"], unet["rank3_after"]["median_ms"]]
    unet["rank3_spread_ms"] = round(abs(r3[0] - r3[1]), 4)
    unet["per_frame_minus_rank3_ms"] = round(unet["per_frame"]["median_ms"] - float(np.mean(r3)), 4)
    res["unet_call"] = unet
    m.text_cache_slots = 1

    def miss():
        return call(text4.clone())                                   # a new tensor: identity differs, the K / V are projected again
    cache = rounds({"hit": lambda: call(text4), "miss": miss}, a.iters, a.rounds)
    cache["miss_minus_hit_ms"] = round(cache["miss"]["median_ms"] - cache["hit"]["median_ms"], 4)
    kv = sum(t.numel() * 2 for ent in m._text_kv.values() for t in ent if t is not None) + m._text_ref[3].numel() * 2
    cache["entry_bytes"] = int(kv)
    res["cache"] = cache
    out4 = torch.empty_like(text4)
    tt = rounds({"text_travel": lambda: ops.text_travel(keys, uncond, lo, hi, w, 0, L, out=out4)}, a.iters, a.rounds)
    tt["bytes_written"] = out4.numel() * 2
    res["text_travel"] = tt
    n_items, inner = 2 * L, 320
    k_rows = torch.randn(n_items * TEXT_PAD, inner, generator=g).half().to(dev)
    vt = torch.randn(inner, n_items * TEXT_PAD, generator=g).half().to(dev)
    blob = torch.empty((n_items, inner // 64, 3 * 4096), dtype=torch.float16, device=dev)
    pack = {"n_items": n_items, "equal": bool(torch.equal(ops.cross_attn_block_pack_kv(k_rows, vt, n_items, TEXT_PAD),
                                                             packing.pack_k5_kv(k_rows, vt, n_items, TEXT_PAD)))}
    pack.update(rounds({"pack_kernel": lambda: ops.cross_attn_block_pack_kv(k_rows, vt, n_items, TEXT_PAD, out=blob),
                        "pack_k5_kv_torch": lambda: packing.pack_k5_kv(k_rows, vt, n_items, TEXT_PAD)}, a.iters, a.rounds))
    pack["torch_over_kernel"] = round(pack["pack_k5_kv_torch"]["median_ms"] / pack["pack_kernel"]["median_ms"], 2)
    res["pack"] = pack
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
