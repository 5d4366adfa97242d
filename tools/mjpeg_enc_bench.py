#!/usr/bin/env python3
"""Time the Motion-JPEG write side (vdx/video.py `encode_frames`, csrc/mjpeg_enc.hip; fsdp_chunked_coherent.py:250-253
`cv2.VideoWriter`) of one video: 24 uint8 frames of 576x1024 on the GPU to the file's bytes in host memory, wall time, for three
paths in one process on one box:

    (a) `encode_frames` + the container, the writer's default stream (one segment per frame);
    (b) the same with `restart_rows=1` (one segment per MCU row);
    (c) the yardstick, today's path: one copy of the frames to the host, then `Image.save(format="JPEG", quality=92)` per frame
        and the same container.

For (a) and (b) also the per-stage kernel times from HIP events inside `encode_frames` (colour, forward DCT, entropy up to the
per-frame lengths, the copy of the lengths + allocation, packing).  Every path's file is checked byte-equal to (c)'s before
anything is timed.  Measured numbers only.  Prints one JSON line; `--out FILE` also writes it.

    python tools/mjpeg_enc_bench.py [--frames 24] [--iters 10] [--out profiles/mjpeg_enc_bench.json]"""
import argparse
import io
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
from vdx import ops, video  # noqa: E402
from vdx.compat import cv2_shim  # noqa: E402


def wall(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(np.min(ms)), 3), "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import lpips_ref as R
    from PIL import Image
    dev = torch.device("cuda:0")
    F, H, W = a.frames, 576, 1024
    frames = torch.from_numpy(np.stack(list(R.frames_like_video(F, H, W, seed=0)))).to(dev)
    res = {"job": f"{F} uint8 frames {H}x{W} on the GPU -> Motion-JPEG mp4 bytes in host memory, quality 92, 4:2:0",
           "device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1), "host_cpus_usable": len(os.sched_getaffinity(0))}}

    def pillow_path(rows):
        host = frames.cpu().numpy()
        jpegs = []
        for f in host:
            buf = io.BytesIO()
            Image.fromarray(f).save(buf, format="JPEG", quality=92, **({"restart_marker_rows": rows} if rows else {}))
            jpegs.append(buf.getvalue())
        return cv2_shim.mp4_bytes(jpegs, 8, W, H)

    def gpu_path(rows):
        return cv2_shim.mp4_bytes(video.encode_frames(frames, restart_rows=rows), 8, W, H)

    names = ("color", "fdct", "entropy", "lengths_to_host", "pack")
    for name, rows in (("a_default_stream", 0), ("b_restart_rows_1", 1)):
        data = gpu_path(rows)
        entry = {"file_bytes": len(data), "byte_equal_to_pillow": data == pillow_path(rows)}
        if not entry["byte_equal_to_pillow"]:
            raise SystemExit(f"{name}: the file differs from Pillow's; nothing timed")
        entry["whole"] = wall(lambda: gpu_path(rows), a.iters)
        stages = {k: [] for k in names}
        for _ in range(a.iters):
            ev = []
            video.encode_frames(frames, restart_rows=rows, _events=ev)
            torch.cuda.synchronize()
            for k, (e0, e1) in zip(names, zip(ev[:-1], ev[1:])):
                stages[k].append(e0.elapsed_time(e1))
        entry["stage_ms"] = {k: round(float(np.median(v)), 4) for k, v in stages.items()}
        res[name] = entry
    res["c_copy_to_host_plus_pillow_loop"] = {"whole": wall(lambda: pillow_path(0), max(a.iters // 2, 3), warmup=1)}
    c = res["c_copy_to_host_plus_pillow_loop"]["whole"]["median_ms"]
    for name in ("a_default_stream", "b_restart_rows_1"):
        res[name]["pillow_over_this"] = round(c / res[name]["whole"]["median_ms"], 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
