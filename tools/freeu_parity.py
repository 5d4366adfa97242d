#!/usr/bin/env python3
"""Count the fp16 elements at which FreeU's skip filter (csrc/freeu.hip) differs from the float64 restatement
(tests/freeu_ref.py) on every case of tests/test_freeu_gpu.py::test_filter_matches_the_restatement, and on the two headline
planes (9 x 16 and 18 x 32, 1280 channels) at the full 48 images; and the backbone scale against torch's CPU half multiply over
all 65 536 inputs.  Measured numbers only.

    python tools/freeu_parity.py [--out profiles/freeu_parity.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vdx  # noqa: E402,F401
from vdx import ops  # noqa: E402
import freeu_ref as R  # noqa: E402
import test_freeu_gpu as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"FreeU skip filter against the float64 restatement; device {torch.cuda.get_device_name(0)}, "
             f"source_sha {vdx._lib.source_sha()}",
             "row: plane, channels, images, s: elements that differ of all, largest |fp16 result - float64 restatement|"]
    total = bad_total = 0
    for H, W in R.PLANES:
        for C in cases.CHANNELS:
            for s in cases.SCALES:
                x, want16, want64 = R.make_case(H, W, C, 3, s)
                for n_img in (1, 2, 3):
                    got = cases.run_filter(dev, x, s, n_img)
                    bad = R.differing(got, want16[:n_img])
                    total, bad_total = total + got.numel(), bad_total + bad
                    lines.append(f"{H}x{W} C={C} n_img={n_img} s={s}: {bad} of {got.numel()}, "
                                 f"{float((got.double() - want64[:n_img]).abs().max()):.3e}")
    lines.append(f"all test cases: {bad_total} of {total} elements differ")
    for (H, W), s in (((9, 16), 0.9), ((18, 32), 0.2)):
        x, want16, want64 = R.make_case(H, W, 1280, 48, s)
        got = cases.run_filter(dev, x, s)
        lines.append(f"headline {H}x{W} C=1280 n_img=48 s={s}: {R.differing(got, want16)} of {got.numel()}, "
                     f"{float((got.double() - want64).abs().max()):.3e}")
    every = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16).reshape(-1, 8)
    x = torch.cat([every, every.flip(0)], dim=1).contiguous()
    for b in (1.2, 1.4, 1.0):
        got, want = ops.freeu_scale(x.to(dev), b).cpu(), R.scale_ref(x, b)
        wrong = int(((cases.bits(got) != cases.bits(want)) & ~(got.isnan() & want.isnan())).sum())
        lines.append(f"scale b={b}: {wrong} of {got.numel()} elements differ from torch's CPU half multiply (all 65536 inputs)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
