#!/usr/bin/env python3
"""Time the LoRA merge (csrc/lora.hip, vdx/lora.py) on one GPU.  Measured numbers only: medians of `--iters` (default 20).

  * the kernel at (1280 x 1280, R 16), (10240 x 1280, R 16) and (1280 x 11520, a 3x3 conv flattened, R 16) against the same
    expression as torch-GPU ops, `W.float().addmm(up, down, alpha=s).half()` (equal within one fp16 ulp, asserted: the torch form
    sums in an order of its own); time and achieved GB/s of the bytes the merge has to move (W read and written, up and down read);
  * a whole-XL merge: a rank-16 adapter on every attention and feed-forward projection of the synthetic Zeroscope state dict,
    from `set_adapters` to loaded weights, split into the merge (`lora.merge_state_dict`, uploads and downloads included) and the
    re-packing (`load_diffusers_state_dict`), with the time to re-obtain the synthetic base beside them.
Prints one JSON line; `--out FILE` also writes it.

    python tools/lora_bench.py [--iters 20] [--out profiles/lora_bench.json] [--skip-xl]"""
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
from vdx import _lib, lora, ops  # noqa: E402
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


def kernel_case(n_out, n_in, R, iters, dev):
    g = torch.Generator().manual_seed(n_out + n_in)
    W = (torch.randn(n_out, n_in, generator=g) / n_in ** 0.5).half().to(dev)
    up, down, s = torch.randn(n_out, R, generator=g).to(dev), (torch.randn(R, n_in, generator=g) / (R * n_in) ** 0.5).to(dev), 0.75
    out = torch.empty_like(W)
    ours = ops.lora_merge(W, [(up, down, s)], out=out).clone()
    theirs = W.float().addmm(up, down, alpha=s).half()
    diff = (ours.float() - theirs.float()).abs()
    assert bool((diff <= 2.0 ** -10 * theirs.float().abs() + 2.0 ** -24).all()), float(diff.max())     # one fp16 ulp at most
    nbytes = 2 * W.numel() * 2 + (up.numel() + down.numel()) * 4
    k = median_ms(lambda: ops.lora_merge(W, [(up, down, s)], out=out), iters)
    t = median_ms(lambda: W.float().addmm(up, down, alpha=s).half(), iters)
    return {"shape": [n_out, n_in], "rank": R, "iters": iters, "kernel_ms": round(k, 4), "torch_ms": round(t, 4),
            "kernel_gbps": round(nbytes / k / 1e6, 1), "torch_gbps_same_bytes": round(nbytes / t / 1e6, 1), "bytes": nbytes,
            "max_abs_diff_vs_torch": float(diff.max())}


def xl_case(iters, dev):
    cfg = UNet3DConfig.zeroscope()
    shapes = lora.targets("unet", cfg)
    ends = (".to_q", ".to_k", ".to_v", ".to_out.0", ".ff.net.0.proj", ".ff.net.2")
    mods = [m for m in shapes if m.endswith(ends)]
    g = torch.Generator().manual_seed(1)
    sd = {}
    for m in mods:
        co, ci = shapes[m]
        sd[f"unet.{m}.lora_A.weight"] = torch.randn(16, ci, generator=g) / ci ** 0.5
        sd[f"unet.{m}.lora_B.weight"] = 0.05 * torch.randn(co, 16, generator=g)
    ad = lora.read_lora(sd, "xl", unet_cfg=cfg)
    unet = UNet3DConditionModel(cfg)
    base_s, merge_s, pack_s = [], [], []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        base = synthetic_state_dict(cfg, 1234, "cpu")
        t1 = time.perf_counter()
        merged = lora.merge_state_dict(base, "unet", [ad], [1.0], dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        unet.load_diffusers_state_dict(merged, device=dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        base_s.append(t1 - t0); merge_s.append(t2 - t1); pack_s.append(t3 - t2)
        del base, merged
    med = lambda v: round(float(np.median(v)), 4)      # noqa: E731
    return {"modules": len(mods), "rank": 16, "iters": iters, "base_s": med(base_s), "merge_s": med(merge_s), "repack_s": med(pack_s),
            "merged_weight_bytes": int(sum(2 * int(np.prod(shapes[m])) for m in mods)),
            "note": "base_s: the synthetic base generated on the CPU; merge_s: upload, kernel and download of every targeted weight; "
                    "repack_s: load_diffusers_state_dict from CPU tensors to the GPU"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--xl-iters", type=int, default=3)
    ap.add_argument("--skip-xl", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "source_sha": _lib.source_sha(),
           "kernel": [kernel_case(1280, 1280, 16, a.iters, dev), kernel_case(10240, 1280, 16, a.iters, dev),
                      kernel_case(1280, 11520, 16, a.iters, dev)]}
    if not a.skip_xl:
        rec["xl_merge"] = xl_case(a.xl_iters, dev)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
