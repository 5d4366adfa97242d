#!/usr/bin/env python3
"""Measure the clip comparison kernels (vdx/compare.py, csrc/compare.hip) against the float64 restatement (tests/compare_ref.py)
on the inputs of tests/test_compare_gpu.py:

  * sse: equal to numpy's integer sum or not, per size;
  * per input kind, the worst over the sizes of max |mean - restatement's mean| over frames, planes and (ssim, cs) at scale 0,
    and of |frame SSIM - restatement's|;
  * the same for the five scales of MS-SSIM and for MS-SSIM itself;
  * on the CPU, what fp32 moments would cost: the restatement with float32 moments on the flat-bright input.

tests/test_compare_gpu.py bounds each kind by 4x the larger of its two figures.  Measured numbers only.

    python tools/compare_parity.py [--out profiles/compare_parity.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vdx  # noqa: E402,F401
from vdx import compare  # noqa: E402
import compare_ref as R  # noqa: E402


def fp32_moment_error(size=(61, 117)) -> float:
    """max |ssim map with float32 moments - float64 map| on one flat-bright plane pair."""
    a, b = R.pair("flat_bright", size, frames=1)
    x, y = a[0, ..., 0].astype(np.float32), b[0, ..., 0].astype(np.float32)
    w = R.window().astype(np.float32)

    def valid(p):
        H, W = p.shape
        v = np.zeros((H - 10, W), np.float32)
        for k in range(11):
            v += w[k] * p[k:k + H - 10, :]
        o = np.zeros((H - 10, W - 10), np.float32)
        for k in range(11):
            o += w[k] * v[:, k:k + W - 10]
        return o
    mx, my = valid(x), valid(y)
    sx2, sy2, sxy = valid(x * x) - mx * mx, valid(y * y) - my * my, valid(x * y) - mx * my
    c1, c2 = np.float32(R.C1), np.float32(R.C2)
    m32 = (2 * (mx * my) + c1) / (mx * mx + my * my + c1) * ((2 * sxy + c2) / (sx2 + sy2 + c2))
    m64, _ = R.ssim_maps(x, y)
    return float(np.abs(m32.astype(np.float64) - m64).max())


def measure(kind, size, scales, dev):
    a, b = R.pair(kind, size)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    means, sse = compare.plane_means(ta, tb, scales)
    means, sse = means.cpu().numpy()[:, :, :scales], sse.cpu().tolist()
    want = R.clip_means(a, b, scales)
    exact = sse == [R.sse(fa, fb) for fa, fb in zip(a, b)]
    d_means = float(np.abs(means - want).max())
    if scales == 1:
        d_val = max(abs(compare._ssim_of(means[f]) - R.ssim_from_means(want[f])) for f in range(len(a)))
    else:
        d_val = max(abs(compare._ms_ssim_of(means[f]) - R.ms_ssim_from_means(want[f])) for f in range(len(a)))
    return exact, d_means, d_val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"clip comparison against the float64 restatement; device {torch.cuda.get_device_name(0)}, source_sha {vdx._lib.source_sha()}",
             "row: kind (H, W): sse exact, max |plane mean - restatement| over frames, planes, (ssim, cs), max |frame value - restatement|"]
    worst = {}
    lines.append("scale 0 (SSIM):")
    for kind in R.SSIM_KINDS:
        for size in R.SSIM_SIZES:
            exact, dm, dv = measure(kind, size, 1, dev)
            w = worst.setdefault(kind, [0.0, 0.0])
            w[0], w[1] = max(w[0], dm), max(w[1], dv)
            lines.append(f"{kind} {size}: sse exact {exact}, means {dm:.3e}, ssim {dv:.3e}")
    lines.append("SSIM worst per kind (the larger of the two): " + ", ".join(f"{k} {max(v):.3e}" for k, v in worst.items())
                 + "; test bound = 4x each")
    nz = worst["noise"][0]
    lines.append(f"flat_bright / noise = {worst['flat_bright'][0] / nz if nz else float('inf'):.2f} (above 100 the moments would be "
                 "lost to cancellation)")
    lines.append(f"CPU, the restatement with float32 moments, flat_bright (61, 117): max |ssim map - float64 map| {fp32_moment_error():.3e}")
    worst_ms = {}
    lines.append("five scales (MS-SSIM):")
    for kind in R.MS_KINDS:
        for size in R.MS_SIZES:
            exact, dm, dv = measure(kind, size, 5, dev)
            w = worst_ms.setdefault(kind, [0.0, 0.0])
            w[0], w[1] = max(w[0], dm), max(w[1], dv)
            lines.append(f"{kind} {size}: sse exact {exact}, means {dm:.3e}, ms_ssim {dv:.3e}")
    lines.append("MS-SSIM worst per kind (the larger of the two): " + ", ".join(f"{k} {max(v):.3e}" for k, v in worst_ms.items())
                 + "; test bound = 4x each")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
