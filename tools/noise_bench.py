#!/usr/bin/env python3
"""Time the seeded noise generator (csrc/noise.hip) at the headline latent (1,4,24,72,128).  Measured numbers only: medians of
`--iters` (default 20) event-timed calls taken in alternating rounds (every round times every candidate once, so a drift of the box
falls on all of them alike).

  * the kernel over the whole tensor, fp16 and fp32 (the fast form: a lane per Philox block);
  * the kernel over a 16-frame box (one merged row, the fast form) and over a box that starts inside a block (the general form);
  * `torch.randn` on the GPU (what the job does without `--seed`);
  * `torch.randn` on the CPU plus the upload (what `--noise_device cpu` costs), wall-clocked, since its work is the host's.
All of these are launch-bound at 884 736 elements; no ratio is promised.  The kernel's bits are checked against tests/noise_ref.py
first.  Prints one JSON line; `--out FILE` also writes it.

    python tools/noise_bench.py [--iters 20] [--out profiles/noise_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import vdx  # noqa: E402,F401
from vdx import ops  # noqa: E402


def timed_rounds(cands, iters, warmup=5):
    """{name: fn} -> {name: {"median_ms", "min_ms", "iters"}}: `iters` rounds, each timing every candidate once, in order.  GPU
    time by events; a name that starts with "host_" by the wall clock around the call and a synchronize."""
    for _ in range(warmup):
        for fn in cands.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in cands}
    for _ in range(iters):
        for name, fn in cands.items():
            if name.startswith("host_"):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {name: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "iters": iters}
            for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import noise_ref
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1)}}
    shape, seed = (1, 4, 24, 72, 128), 5
    frames16 = ((0, 0, 4, 0, 0), (1, 4, 16, 72, 128))
    ragged = ((0, 0, 0, 0, 1), (1, 4, 24, 72, 124))
    got = ops.philox_normal(shape, seed, device=dev).cpu().numpy()
    differ = int((got.view(np.uint16) != noise_ref.normal(shape, seed).view(np.uint16)).sum())
    assert differ == 0, f"{differ} of {got.size} elements differ from the restatement"
    assert ops.philox_form(shape) and ops.philox_form(shape, frames16) and not ops.philox_form(shape, ragged)
    o16, o32 = torch.empty(shape, dtype=torch.float16, device=dev), torch.empty(shape, dtype=torch.float32, device=dev)
    b16, r16 = torch.empty(frames16[1], dtype=torch.float16, device=dev), torch.empty(ragged[1], dtype=torch.float16, device=dev)

    def torch_gpu():
        torch.manual_seed(0)
        return torch.randn(*shape, device=dev, dtype=torch.float16)

    def torch_cpu_upload():
        torch.manual_seed(0)
        return torch.randn(*shape, device="cpu", dtype=torch.float16).to(dev)
    cands = {
        "philox_f16_whole": lambda: ops.philox_normal(shape, seed, device=dev, out=o16),
        "philox_f32_whole": lambda: ops.philox_normal(shape, seed, dtype=torch.float32, device=dev, out=o32),
        "philox_f16_16_frame_box": lambda: ops.philox_normal(shape, seed, box=frames16, device=dev, out=b16),
        "philox_f16_general_form_box": lambda: ops.philox_normal(shape, seed, box=ragged, device=dev, out=r16),
        "torch_randn_gpu_f16": torch_gpu,
        "host_torch_randn_cpu_f16_plus_upload": torch_cpu_upload,
    }
    r = {"latent": list(shape), "elements": int(np.prod(shape)), "elements_equal_to_restatement": int(got.size),
         "boxes": {"16_frame": [list(v) for v in frames16], "general_form": [list(v) for v in ragged]},
         "timing": "GPU events, except host_*: wall clock around the call and a synchronize"}
    r.update(timed_rounds(cands, a.iters))
    res["noise"] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
