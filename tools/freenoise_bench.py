#!/usr/bin/env python
"""Time FreeNoise's window-fused temporal attention (csrc/freenoise.hip) at level 0 of the headline latent extended to F = 64
frames: B = 2, HW = 72 x 128, 5 heads, L = 16, S = 4.  Three variants in ONE process, timed in alternating rounds after a
warm-up, medians of --iters rounds:

  windows  `ops.temporal_attn_windows`, one launch
  loop     the same result as a loop of `ops.temporal_attn` over slice copies of each window's rows plus a torch weighted sum
  full     plain `ops.temporal_attn` over all 64 frames (another result: the un-windowed attention, for scale)

GB/s are against the one-read-one-write byte count of the fused kernel: qkv read once, out written once.

    python tools/freenoise_bench.py [--out profiles/freenoise_bench.json] [--iters 20]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vdx  # noqa: E402,F401
from vdx import _lib, freenoise, ops  # noqa: E402

B, F, HW, HEADS, L, S = 2, 64, 72 * 128, 5, 16, 4
SCALE = 64 ** -0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freenoise_bench.json"))
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    inner = HEADS * 64
    qkv = torch.randn(B * F * HW, 3 * inner, generator=torch.Generator(device=dev).manual_seed(0), device=dev, dtype=torch.float16)
    starts = freenoise.window_starts(F, L, S)
    wn = freenoise.window_weights(F, L, S).to(dev)
    out = torch.empty((B * F * HW, inner), dtype=torch.float16, device=dev)

    def windows():
        return ops.temporal_attn_windows(qkv, wn, B=B, F=F, HW=HW, heads=HEADS, scale=SCALE, L=L, S=S, out=out)

    def loop():
        q5 = qkv.view(B, F, HW, 3 * inner)
        acc = torch.zeros((B, F, HW, inner), dtype=torch.float32, device=dev)
        for i, s in enumerate(starts):
            o = ops.temporal_attn(q5[:, s:s + L].reshape(B * L * HW, 3 * inner), B=B, F=L, HW=HW, heads=HEADS, scale=SCALE)
            acc[:, s:s + L] += wn[i].view(1, L, 1, 1) * o.view(B, L, HW, inner).float()
        return acc.half().view(B * F * HW, inner)

    def full():
        return ops.temporal_attn(qkv, B=B, F=F, HW=HW, heads=HEADS, scale=SCALE, out=out)

    variants = {"windows": windows, "loop": loop, "full": full}
    got, want = windows().clone(), loop()
    err = float((got.float() - want.float()).abs().max())
    for fn in variants.values():            # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.iters):                # alternating rounds: every variant once per round
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    nbytes = qkv.numel() * 2 + out.numel() * 2
    rec = {"job": f"window-fused temporal attention, B={B} F={F} HW={HW} heads={HEADS} L={L} S={S} ({len(starts)} windows)",
           "device": torch.cuda.get_device_name(0), "source_sha": _lib.source_sha(), "iters": a.iters,
           "one_read_one_write_bytes": nbytes, "max_abs_diff_windows_vs_loop": err}
    for k, v in ms.items():
        med = statistics.median(v)
        rec[k] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "gb_per_s_of_fused_bytes": round(nbytes / med / 1e6, 1)}
    rec["loop_over_windows"] = round(rec["loop"]["median_ms"] / rec["windows"]["median_ms"], 3)
    rec["windows_over_full"] = round(rec["windows"]["median_ms"] / rec["full"]["median_ms"], 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
