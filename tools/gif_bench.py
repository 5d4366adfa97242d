#!/usr/bin/env python
"""Time the animated-GIF writer (vdx/gif.py `encode_gif`, csrc/gif.hip) on 24 frames of 576 x 1024 that are on the device, and the
only other route beside it on the same box: a copy to the host plus Pillow's `save(save_all=True)`.

Per configuration (both dithers; the default strips, strip_rows=1 and one strip per frame): the median of `--iters` runs of
`encode_gif` as a whole, frames on the device to file bytes in host memory, in three rounds that alternate over the
configurations, and each stage's kernel time from HIP events on the stream (median over the same runs); the host's median cut
and file assembly are timed on their own.  Pillow is timed
`--pillow-iters` times (it takes seconds per run).

    python tools/gif_bench.py [--frames 24] [--iters 20] [--out profiles/gif_bench.json]"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clip(T, H, W, seed=0):
    """A gradient that moves, a noisy third, a flat band: smooth, busy and flat regions in every frame"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    f = np.stack([np.stack([(x * 255 // (W - 1) + 8 * t) % 256, y * 255 // (H - 1), (x + y + 16 * t) // 4 % 256], axis=-1)
                  for t in range(T)]).astype(np.uint8)
    f[:, :H // 3, :W // 3] = rng.integers(0, 256, (T, H // 3, W // 3, 3))
    f[:, 2 * H // 3:] = (40, 90, 200)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--height", type=int, default=576)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pillow-iters", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gif_bench.json"))
    a = ap.parse_args()
    from PIL import Image
    import PIL

    from vdx import _lib, gif
    dev = torch.device("cuda:0")
    T, H, W = a.frames, a.height, a.width
    host = clip(T, H, W)
    frames = torch.from_numpy(host).to(dev)
    configs = [(d, name, sr) for d in ("bayer", "none") for name, sr in (("default", None), ("rows1", 1), ("one_strip", H))]
    wall = {c[:2]: [] for c in configs}
    stages = {c[:2]: {} for c in configs}
    sizes = {}
    for d, name, sr in configs:                                             # warm-up, and the sizes
        blob, info = gif.encode_gif(frames, 8, dither=d, strip_rows=sr)
        sizes[d, name] = {"bytes": len(blob), "colors": info["colors"], "strip_rows": info["strip_rows"]}
    per_round = -(-a.iters // 3)
    for _round in range(3):
        for d, name, sr in configs:
            for _ in range(per_round):
                ev = []
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gif.encode_gif(frames, 8, dither=d, strip_rows=sr, _events=ev)
                wall[d, name].append((time.perf_counter() - t0) * 1e3)
                torch.cuda.synchronize()
                for stage, e0, e1 in ev:
                    stages[d, name].setdefault(stage, []).append(e0.elapsed_time(e1))
    # the host's share of `encode_gif`, each part on its own: the median cut of this clip's histogram, and the file assembly
    from vdx import ops
    hist = ops.gif_hist(frames).cpu().numpy()
    cut_ms, asm_ms = [], []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        pal = gif.median_cut(hist)
        cut_ms.append((time.perf_counter() - t0) * 1e3)
    blocks = [bytes(len(blob) // T)] * T
    for _ in range(a.iters):
        t0 = time.perf_counter()
        gif.file_bytes(W, H, pal, blocks, 13, 0)
        asm_ms.append((time.perf_counter() - t0) * 1e3)
    host = {"occupied_bins": int((hist != 0).sum()), "median_cut_median_ms": statistics.median(cut_ms),
            "file_bytes_median_ms": statistics.median(asm_ms)}
    pil = []
    for _ in range(a.pillow_iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        imgs = [Image.fromarray(f) for f in frames.cpu().numpy()]
        buf = io.BytesIO()
        imgs[0].save(buf, format="GIF", save_all=True, append_images=imgs[1:], duration=130, loop=0)
        pil.append((time.perf_counter() - t0) * 1e3)
        pil_bytes = len(buf.getvalue())
    rec = {"tool": "tools/gif_bench.py", "source_sha": _lib.source_sha(), "device": torch.cuda.get_device_name(0), "frames": T, "height": H,
           "width": W, "fps": 8, "runs_per_config": 3 * per_round, "rounds": 3,
           "content": "moving gradient, a noisy third, a flat band (tools/gif_bench.py clip)",
           "encode_gif_ms": {f"{d}/{name}": {"median_ms": statistics.median(wall[d, name]), "min_ms": min(wall[d, name]),
                                             "max_ms": max(wall[d, name]), **sizes[d, name],
                                             "stage_kernel_ms": {s: statistics.median(v) for s, v in stages[d, name].items()}}
                             for d, name, _sr in configs},
           "host_parts_ms": host,
           "host_copy_plus_pillow": {"pillow": PIL.__version__, "runs": a.pillow_iters, "median_ms": statistics.median(pil), "bytes": pil_bytes}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
