#!/usr/bin/env python3
"""Time weighted and long prompts (csrc/prompt.hip, the UNet at text of more than 128 rows) on synthetic Zeroscope weights.  Measured
numbers only: medians of `--iters` (default 20) event-timed calls, each taken in `--rounds` (default 3) rounds that alternate
between the entries of a group, so that the spread between an entry's own rounds stands beside the difference between two entries.

  * the weighting kernel at (2 x 4 sequences, 77, 1024) against the same expression as torch-GPU ops (equal values asserted: the
    inputs keep |z| <= 64, so the fp64 sums are exact in any order);
  * one UNet call on the 16-frame window of the (1, 4, 24, 72, 128) latent at text 77, read before and after the others in every
    round (that spread is the noise floor), at text 154, 231 and 308, and at text 77 with the fused level-0 cross-attention (K5)
    switched off: K5 declines above 80 keys, so that last difference is what level 0 pays for leaving K5 at any longer text, and
    the rest of a longer text's added milliseconds is the longer keys themselves;
  * with `--parent_tree DIR` (a checkout of the parent commit with its library built): `bench.py --gpus 1` of this tree and of that
    one, alternating, each run a fresh process.  Without it: "not measured".
No whole-video figure is taken.  Prints one JSON line; `--out FILE` also writes it.

    python tools/prompt_bench.py [--iters 20] [--rounds 3] [--parent_tree DIR] [--out profiles/prompt_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vdx  # noqa: E402,F401
from vdx import ops  # noqa: E402
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


def torch_expression(z, w):
    """csrc/prompt.hip's lines with torch ops on the GPU."""
    y = (z.float() * w[:, :, None]).half()
    r = (z.double().sum(dim=(1, 2)) / y.double().sum(dim=(1, 2))).float()
    return (y.float() * r[:, None, None]).half()


def bench_py(tree, steps, warmup):
    """One fresh `bench.py --gpus 1` of `tree` -> its steps/s."""
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                         cwd=tree, check=True, capture_output=True, text=True, timeout=900).stdout
    return float(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])["value"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent_tree", default=None)
    ap.add_argument("--bench_steps", type=int, default=10)
    ap.add_argument("--bench_warmup", type=int, default=3)
    ap.add_argument("--bench_rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1)}, "whole_video": "not measured"}
    g = torch.Generator().manual_seed(0)
    n_seq, n_tok, D = 8, 77, 1024
    z = (torch.randn(n_seq, n_tok, D, generator=g) * 8).clamp(-64, 64).half().to(dev)
    w = torch.tensor([0.55, 1.0, 1.1 ** 3, 1.3], dtype=torch.float32)[torch.randint(0, 4, (n_seq, n_tok), generator=g)]
    w[:, 1] = 1.3
    wd = w.to(dev)
    out = torch.empty_like(z)
    equal = bool(torch.equal(ops.prompt_weight(z, w, out=out).view(torch.int16), torch_expression(z, wd).view(torch.int16)))
    assert equal
    kern = rounds({"op": lambda: ops.prompt_weight(z, w, out=out), "torch_expression": lambda: torch_expression(z, wd)}, a.iters, a.rounds)
    moved = 2 * z.numel() * 2 + w.numel() * 4                       # z read (the second pass hits cache), out written, w read
    kern.update(shape=[n_seq, n_tok, D], equal=equal, bytes=moved, op_GBps=round(moved / kern["op"]["median_ms"] / 1e6, 1),
                torch_over_op=round(kern["torch_expression"]["median_ms"] / kern["op"]["median_ms"], 2),
                note="op: ops.prompt_weight, host checks and the weights' upload included; one block per sequence, 8 blocks on the chip")
    res["kernel"] = kern

    cfg = UNet3DConfig.zeroscope()
    m = UNet3DConditionModel(cfg).load_diffusers_state_dict(synthetic_state_dict(cfg, 1234, dev), device=dev)
    L, h, wl = 16, 72, 128
    lat = torch.randn(1, 4, L, h, wl, generator=g).half().to(dev)
    x = ops.cfg_input(lat, None, 0.0)
    full = torch.randn(2, 308, cfg.cross_attention_dim, generator=g).half().to(dev)
    texts = {n: full[:, :n].contiguous() for n in (77, 154, 231, 308)}
    m.text_cache_slots = 4                                           # every timed call below is a cache hit

    def call(n, k5=True):
        m.fuse_cross_attn = k5
        try:
            return m(x, 500, encoder_hidden_states=texts[n]).sample
        finally:
            m.fuse_cross_attn = True

    unet = {"window": [2, 4, L, h, wl]}
    unet.update(rounds({"text_77_before": lambda: call(77), "text_154": lambda: call(154), "text_231": lambda: call(231),
                        "text_308": lambda: call(308), "text_77_k5_off": lambda: call(77, False), "text_77_after": lambda: call(77)},
                       a.iters, a.rounds))
    r0 = [unet["text_77_before"]["median_ms"], unet["text_77_after"]["median_ms"]]
    base = float(np.mean(r0))
    unet["text_77_spread_ms"] = round(abs(r0[0] - r0[1]), 4)
    unet["level0_leaving_k5_ms"] = round(unet["text_77_k5_off"]["median_ms"] - base, 4)
    for n in (154, 231, 308):
        unet[f"text_{n}_minus_77_ms"] = round(unet[f"text_{n}"]["median_ms"] - base, 4)
        unet[f"text_{n}_beyond_leaving_k5_ms"] = round(unet[f"text_{n}"]["median_ms"] - unet["text_77_k5_off"]["median_ms"], 4)
    res["unet_call"] = unet
    del m, x, lat
    torch.cuda.empty_cache()

    if a.parent_tree:
        trees = {"this": ROOT, "parent": os.path.abspath(a.parent_tree)}
        got = {k: [] for k in trees}
        for _ in range(a.bench_rounds):
            for k, tree in trees.items():
                got[k].append(round(bench_py(tree, a.bench_steps, a.bench_warmup), 4))
        res["bench_py"] = {"steps": a.bench_steps, "warmup": a.bench_warmup, "steps_per_s": got,
                           "spread": {k: round(max(v) - min(v), 4) for k, v in got.items()}}
    else:
        res["bench_py"] = "not measured"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
