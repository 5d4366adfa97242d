#!/usr/bin/env python3
"""Measure the frame interpolation (vdx/interp.py, csrc/interp.hip) on the inputs of its tests (tests/interp_inputs.py):

  * on the CPU, from the float64 restatement (tests/interp_ref.py) with the float64 shim's flows: the interior mean absolute
    error of the interpolated middle frame of the moving pair against the true middle frame, that of the plain blend, and their
    ratio (tests/test_interp_host.py asserts it with a 2x margin);
  * on the GPU: per stage case and size the share of bytes in which the kernel differs from the float64 restatement on the same
    fp32 flows and the largest difference, next to the same figures of the restatement evaluated in float32 numpy; per case the
    worst share (tests/test_interp_gpu.py bounds it by 4x that, capped at 1e-3); and the moving pair's ratio with the GPU's own flows.

Measured numbers only.

    python tools/interp_parity.py [--out profiles/interp_parity.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vdx  # noqa: E402,F401
from vdx import interp, ops  # noqa: E402
from vdx.compat import cv2_shim  # noqa: E402
import interp_inputs as I  # noqa: E402
import interp_ref as R  # noqa: E402


def diff(got, want):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    return int(d.max()), int(np.count_nonzero(d)), d.size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    A, B, truth = I.moving_pair()
    ga, gb = (cv2_shim.cvtColor(f, cv2_shim.COLOR_RGB2GRAY) for f in (A, B))
    args = (None, 0.5, 3, 15, 3, 5, 1.2, 0)
    fab, fba = cv2_shim.calcOpticalFlowFarneback(ga, gb, *args), cv2_shim.calcOpticalFlowFarneback(gb, ga, *args)
    e_i, e_b = I.interior_mae(R.interp_pair(A, B, fab, fba, 1, 2), truth), I.interior_mae(R.blend_pair(A, B, 1, 2), truth)
    lines = [f"frame interpolation; device {torch.cuda.get_device_name(0)}, source_sha {vdx._lib.source_sha()}",
             f"CPU, float64 restatement, float64 shim flows: moving pair {I.QUALITY_HW} moved by {I.MOVE}, interior (border "
             f"{I.QUALITY_BORDER}) MAE interpolated {e_i:.4f}, plain blend {e_b:.4f}, ratio {e_i / e_b:.4f}",
             f"  largest flow error there: {float(np.abs(fab[24:-24, 24:-24] - np.array(I.MOVE)).max()):.2e} px; steepest canvas step "
             f"{float(max(np.abs(np.diff(A.astype(float), axis=ax)).max() for ax in (0, 1))):.0f} grey levels per px"]
    out = interp.interpolate_frames(np.stack([A, B]), 2, device=dev).cpu().numpy()
    g_i = I.interior_mae(out[1], truth)
    lines.append(f"GPU, its own flows: MAE interpolated {g_i:.4f}, ratio {g_i / e_b:.4f}")
    lines.append("stage cases, kernel against the float64 restatement on the same fp32 flows: (H, W) case factors: largest "
                 "difference, bytes differing of all (share) [the restatement in float32 numpy: the same figures]")
    worst = {}
    for name in I.STAGE_CASES:
        for size in I.STAGE_SIZES:
            frames, ab, ba = I.stage_case(size, name)
            f, tab, tba = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (frames, ab, ba))
            Ns = I.stage_factors(name)
            got = np.concatenate([ops.interp_frames(f, tab, tba, N).cpu().numpy() for N in Ns])
            want = np.concatenate([R.interp_clip(frames, ab, ba, N) for N in Ns])
            f32 = np.concatenate([R.interp_clip(frames, ab, ba, N, dtype=np.float32) for N in Ns])
            (m, n, tot), (m32, n32, _) = diff(got, want), diff(f32, want)
            worst[name] = max(worst.get(name, 0.0), n / tot)
            lines.append(f"{size} {name} {Ns}: {m}, {n} of {tot} ({n / tot:.2e}) [{m32}, {n32} ({n32 / tot:.2e}); kernel == float32 "
                         f"numpy: {bool(np.array_equal(got, f32))}]")
    lines.append("worst share per case: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + "; test bound = 4x, capped at 1e-3")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
