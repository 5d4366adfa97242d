#!/usr/bin/env python3
"""Time the GPU Farneback flow (vdx/flow.py, csrc/flow.hip; scoring.py:311-339, fsdp_chunked_coherent.py:236-246) of one
video: 24 uint8 frames at 576x1024 already on the GPU, 23 pairs in one batch.  HIP events around each stage at every
pyramid level (grey, blur + resize, polynomial expansion, the flow's upsampling, one update iteration), around the whole
`farneback_flows`, `temporal_consistency` and a four-boundary `flow_warp_error`; next to them the wall time of the float64
shim (vdx.compat.cv2_shim) for ONE pair on the same box.  Measured numbers only.  Prints one JSON line; `--out FILE` also
writes it.

    python tools/flow_bench.py [--frames 24] [--iters 10] [--no-cpu] [--out profiles/flow_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vdx  # noqa: E402,F401
from vdx import flow, ops  # noqa: E402
from vdx.compat import cv2_shim  # noqa: E402


def timed(fn, iters, warmup=2):
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
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true", help="skip the shim's one pair")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import lpips_ref as R
    dev = torch.device("cuda:0")
    F, H, W = a.frames, 576, 1024
    host = R.frames_like_video(F, H, W, seed=0)
    frames = torch.from_numpy(host).to(dev)
    res = {"job": f"Farneback flow (0.5, 3, 15, 3, 5, 1.2, 0) over {F - 1} consecutive pairs, {F} frames {H}x{W} uint8 on the GPU",
           "device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1)}}
    plan = flow.level_plan(H, W, flow.LEVELS)
    taps, inv_g = flow.poly_tables()
    st = {}
    grey = ops.flow_grey(frames)
    st["grey"] = timed(lambda: ops.flow_grey(frames), a.iters)
    fl = None
    for k in range(len(plan) - 1, -1, -1):
        h, w, sigma, radius = plan[k]
        if k > 0:
            t = flow._taps_on(dev, sigma, radius)
            pyr = lambda: ops.flow_resize(ops.flow_corr1d(ops.flow_corr1d(grey, t, 0), t, 1), h, w)   # noqa: E731
            img = pyr()
            st[f"level{k}_blur_resize"] = timed(pyr, a.iters)
        else:
            img = grey
        Rk = ops.flow_polyexp(img, taps, inv_g)
        st[f"level{k}_polyexp"] = timed(lambda: ops.flow_polyexp(img, taps, inv_g), a.iters)
        if fl is None:
            fl = torch.zeros((F - 1, h, w, 2), dtype=torch.float32, device=dev)
        else:
            prev = fl
            fl = ops.flow_resize(prev, h, w, mul=2.0)
            st[f"level{k}_flow_upsample"] = timed(lambda: ops.flow_resize(prev, h, w, mul=2.0), a.iters)
        other = torch.empty_like(fl)
        for _ in range(flow.ITERATIONS):
            fl, other = ops.flow_update(Rk, fl, out=other), fl
        st[f"level{k}_update_one_iteration"] = timed(lambda: ops.flow_update(Rk, fl, out=other), a.iters)
        del Rk, other
    st["abs_sum"] = timed(lambda: ops.flow_abs_sum(fl), a.iters)
    st["remap_absdiff"] = timed(lambda: ops.flow_remap_absdiff(frames, fl), a.iters)
    res["stages"] = st
    res["stages_sum_ms"] = round(sum(v["median_ms"] * (flow.ITERATIONS if k.endswith("one_iteration") else 1)
                                     for k, v in st.items() if k != "remap_absdiff"), 4)
    del fl, grey
    res["flows_whole"] = timed(lambda: flow.farneback_flows(frames), a.iters)
    res["tc_whole"] = timed(lambda: flow.temporal_consistency(frames), a.iters)
    res["tc_whole"]["tc"] = flow.temporal_consistency(frames)
    ranges = [(i * F // 5, (i + 1) * F // 5) for i in range(5)]
    res["flow_err_whole"] = timed(lambda: flow.flow_warp_error(frames, ranges), a.iters)
    res["flow_err_whole"].update(boundaries=len(flow.boundary_pairs(F, ranges)), flow_err=flow.flow_warp_error(frames, ranges))
    if not a.no_cpu:
        g0, g1 = (cv2_shim.cvtColor(host[i], cv2_shim.COLOR_RGB2GRAY) for i in (0, 1))
        t0 = time.time()
        want = cv2_shim.calcOpticalFlowFarneback(g0, g1, None, *flow_args())
        wall = time.time() - t0
        got = flow.farneback_flows(frames[:2])[0].cpu().numpy()
        res["cpu_shim"] = {"one_pair_wall_s": round(wall, 3), "mean_abs_flow": float(np.mean(np.abs(want))),
                           "gpu_mean_abs_flow": float(np.mean(np.abs(got)))}
        per_pair_ms = res["flows_whole"]["median_ms"] / (F - 1)
        res["gpu_ms_per_pair"] = round(per_pair_ms, 4)
        res["shim_over_gpu_per_pair"] = round(wall * 1e3 / per_pair_ms, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def flow_args():
    return (flow.PYR_SCALE, flow.LEVELS, flow.WINSIZE, flow.ITERATIONS, flow.POLY_N, flow.POLY_SIGMA, flow.FLAGS)


if __name__ == "__main__":
    main()
