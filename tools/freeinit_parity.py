#!/usr/bin/env python3
"""Measure FreeInit's frequency mix (vdx/freeinit.py, csrc/freeinit.hip) against the float64 restatement (tests/freeinit_ref.py)
on the inputs of tests/test_freeinit_gpu.py: per volume and filter, the largest difference from the restatement's fp16 rounding
in fp16 ulps, the number and share of elements whose bits differ, and the largest |kernel - restatement| of the fp16 result.
tests/test_freeinit_gpu.py allows 4x the share at the headline extent, as a count.  Measured numbers only.

    python tools/freeinit_parity.py [--out profiles/freeinit_parity.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vdx  # noqa: E402,F401
from vdx.freeinit import freq_mix, lowpass_filter  # noqa: E402
import freeinit_ref as R  # noqa: E402
import test_freeinit_gpu as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"FreeInit frequency mix against the float64 restatement; device {torch.cuda.get_device_name(0)}, "
             f"source_sha {vdx._lib.source_sha()}",
             "stop frequencies 0.5 / 0.5; row: volume filter: largest difference in fp16 ulps, elements that differ of all "
             "(share), largest |fp16 result - float64 restatement|"]
    rows = [(v, m) for v in cases.SMALL for m in cases.METHODS] + [(cases.HEADLINE, m) for m in cases.METHODS] \
        + [(v, "butterworth") for v in cases.TILE_EDGES]
    headline = {}
    for vol, method in rows:
        z, eta = cases._inputs(vol)
        filt = lowpass_filter(vol[2:], method, 0.5, 0.5)
        got = freq_mix(z.to(dev), eta.to(dev), filt).cpu()
        want = R.mix(z, eta, filt)
        ulps, share = R.compare_fp16(got, want)
        n = got.numel()
        if vol == cases.HEADLINE:
            headline[method] = share
        lines.append(f"{vol} {method}: {ulps:.2f} ulp, {round(share * n)} of {n} ({share:.3e}), "
                     f"{float((got.double() - want).abs().max()):.3e}")
    lines.append("share at the headline extent: " + ", ".join(f"{m} {s:.3e}" for m, s in headline.items())
                 + f"; the largest, {max(headline.values()):.3e}, is tests/test_freeinit_gpu.py's MEASURED_SHARE; test bound = 4x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
