#!/usr/bin/env python3
"""Measure the GPU Farneback flow (vdx/flow.py) against the float64 shim (vdx.compat.cv2_shim) on the inputs of
tests/test_flow_gpu.py (tests/flow_inputs.py): per row the max-abs and rel-L2 difference of the flow, the interior median,
and for the remap kernel the share of bytes that differ from `cv2_shim.remap` fed the GPU's own flow; then the content rows
(edges, flat areas, noise: `flow_inputs.content_clip`) with their own worst figures.  The test bounds are 4x the worst flow
figures this prints, per group of rows (tests/test_flow_gpu.py).  Measured numbers only.

    python tools/flow_parity.py [--out profiles/flow_parity.txt] [--no-large]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vdx  # noqa: E402,F401
from vdx import flow  # noqa: E402
from vdx.compat import cv2_shim  # noqa: E402
import flow_inputs as FI  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-large", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"GPU Farneback flow against the float64 shim; device {torch.cuda.get_device_name(0)}, source_sha {vdx._lib.source_sha()}",
             "row (H, W) (dx, dy): flow max-abs px, rel-L2, interior median (x, y) [shim's]; remap bytes differing from cv2_shim.remap"]
    worst_abs = worst_rel = 0.0
    for hw, sh in FI.SMALL_ROWS + ([] if a.no_large else [FI.LARGE_ROW]):
        fr = FI.pair(hw, sh)
        want = FI.shim_flow(2, hw[0], hw[1], sh[0], sh[1])[0].astype(np.float64)
        got = flow.farneback_flows(torch.from_numpy(fr.copy()).to(dev))[0].cpu().numpy().astype(np.float64)
        e_abs = float(np.abs(got - want).max())
        e_rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        worst_abs, worst_rel = max(worst_abs, e_abs), max(worst_rel, e_rel)
        med, smed = (np.median(f[10:-10, 10:-10].reshape(-1, 2), 0) for f in (got, want))
        flows, sums, warped = flow.warp_pairs(fr, [1], device=dev, want_warped=True)
        fl = flows[0].cpu().numpy()
        mx = (np.arange(hw[1])[None, :] + fl[:, :, 0]).astype(np.float32)
        my = (np.arange(hw[0])[:, None] + fl[:, :, 1]).astype(np.float32)
        ref = cv2_shim.remap(fr[0], mx, my, cv2_shim.INTER_LINEAR).astype(np.int32)
        d = np.abs(warped[0].cpu().numpy().astype(np.int32) - ref)
        lines.append(f"{hw} {sh}: {e_abs:.3e} px, {e_rel:.3e}, median ({med[0]:.4f}, {med[1]:.4f}) [({smed[0]:.4f}, {smed[1]:.4f})]; "
                     f"remap {int((d > 0).sum())} of {d.size} bytes differ (share {float((d > 0).mean()):.2e}), largest difference {int(d.max())}")
    lines.append(f"worst flow max-abs {worst_abs:.3e} px, worst rel-L2 {worst_rel:.3e}; test bounds = 4x these")
    lines.append("content rows (72, 104), integer pixel values: flow max-abs px, rel-L2 (n/a where the shim's flow is ~0), "
                 "largest |shim flow| px, TC gpu / shim")
    worst_abs = worst_rel = 0.0
    for name in FI.CONTENT_ROWS + FI.ZERO_ROWS:
        fr = FI.content_clip(name)
        want = FI.content_shim_flow(name)[0].astype(np.float64)
        got = flow.farneback_flows(torch.from_numpy(fr.copy()).to(dev))[0].cpu().numpy().astype(np.float64)
        e_abs = float(np.abs(got - want).max())
        worst_abs = max(worst_abs, e_abs)
        if name in FI.CONTENT_ROWS:
            e_rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
            worst_rel = max(worst_rel, e_rel)
        tc, tc_shim = flow.temporal_consistency(fr, device=dev), float(np.mean(np.abs(want)))
        lines.append(f"{name}: {e_abs:.3e} px, {f'{e_rel:.3e}' if name in FI.CONTENT_ROWS else 'n/a'}, {float(np.abs(want).max()):.3e}, "
                     f"TC {tc!r} / {tc_shim!r}")
    lines.append(f"worst content max-abs {worst_abs:.3e} px, worst rel-L2 {worst_rel:.3e}; STRUCT bounds = 4x these, max-abs <= 2e-3 px")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
