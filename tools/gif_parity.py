#!/usr/bin/env python
"""Write profiles/gif_parity.txt: the figures tests/gif_ref.py computes about the GIF writer's palette and strips, from the
numpy restatement (no GPU): the PSNR of `vdx.gif.median_cut`'s palette on a gradient clip beside a uniform 6x7x6 palette and
Pillow's own median cut, and the file size at the default strips against one strip per frame at 576 x 1024.

    python tools/gif_parity.py [--out profiles/gif_parity.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gif_parity.txt"))
    a = ap.parse_args()
    import PIL

    import gif_ref as R
    from vdx import gif
    ours, uniform, lines = R.parity_figures(gif.median_cut)
    lines = [f"tools/gif_parity.py (tests/gif_ref.py parity_figures, strip_cost_figures), Pillow {PIL.__version__}",
             "", "Palette (asserted: median_cut >= uniform; parity with Pillow's palette is not claimed):"] + lines
    lines += ["", "Cost of independent strips (recorded, not asserted): file bytes, one frame, from the restatement:"] + R.strip_cost_figures(gif.median_cut)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
