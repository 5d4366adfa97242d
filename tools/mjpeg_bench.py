#!/usr/bin/env python3
"""Time the Motion-JPEG read side (vdx/video.py, csrc/mjpeg.hip; scoring.py:16, :110 `cv2.VideoCapture(video_path)`) of one
video: 24 frames at 576x1024 written at quality 92 by the shim's VideoWriter, from the file's bytes in host memory to uint8
frames on the GPU, wall time with a synchronisation at the end, for three paths in one process on one box:

    (a) `read_frames` of the writer's default stream: one segment per frame, 24 busy lanes in the entropy stage;
    (b) `read_frames` of the `restart_rows=1` stream: one segment per MCU row, 864 segments;
    (c) the yardstick: a Pillow decode loop over the same samples plus one upload of the stacked frames.

For (a) and (b) also the host part alone (demux + marker walk + building the upload) and the per-stage kernel times from HIP
events inside `read_frames`.  Every path's frames are checked bit-equal to (c)'s before anything is timed.  Measured numbers
only.  Prints one JSON line; `--out FILE` also writes it.

    python tools/mjpeg_bench.py [--frames 24] [--iters 10] [--out profiles/mjpeg_bench.json]"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vdx  # noqa: E402,F401
from vdx import metrics, ops, video  # noqa: E402


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
    clip = list(R.frames_like_video(F, H, W, seed=0))
    res = {"job": f"Motion-JPEG mp4 bytes in host memory -> {F} uint8 frames {H}x{W} on the GPU, quality 92, 4:2:0",
           "device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1), "host_cpus_usable": len(os.sched_getaffinity(0))}}
    files = {}
    with tempfile.TemporaryDirectory() as d:
        for name, rows in (("a_default_stream", 0), ("b_restart_rows_1", 1)):
            p = os.path.join(d, name + ".mp4")
            metrics.write_video(clip, p, 8, **({"restart_rows": rows} if rows else {}))
            files[name] = open(p, "rb").read()

    def pillow_path(data):
        jpegs = video.demux(data)[0]
        host = np.stack([np.asarray(Image.open(io.BytesIO(j)).convert("RGB")) for j in jpegs])
        return torch.from_numpy(host).to(dev)

    want = pillow_path(files["a_default_stream"])
    for name, data in files.items():
        got, info = video.read_frames(data, device=dev)
        entry = {"file_bytes": len(data), "n_segments": info["n_segments"], "restart_interval": info["restart_interval"],
                 "bit_equal_to_pillow": bool(torch.equal(got, pillow_path(data)))}
        if not entry["bit_equal_to_pillow"]:
            raise SystemExit(f"{name}: the decode differs from Pillow's; nothing timed")
        entry["whole"] = wall(lambda: video.read_frames(data, device=dev), a.iters)
        t = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            video.plan(video.demux(data)[0])
            t.append((time.perf_counter() - t0) * 1e3)
        entry["host_parse_ms"] = round(float(np.median(t)), 3)
        stages = {"entropy": [], "idct": [], "color": []}
        for _ in range(a.iters):
            ev = []
            video.read_frames(data, device=dev, _events=ev)
            torch.cuda.synchronize()
            for k, (e0, e1) in zip(stages, zip(ev[:-1], ev[1:])):
                stages[k].append(e0.elapsed_time(e1))
        entry["stage_kernel_ms"] = {k: round(float(np.median(v)), 4) for k, v in stages.items()}
        res[name] = entry
    del want
    res["c_pillow_loop_plus_upload"] = {"whole": wall(lambda: pillow_path(files["a_default_stream"]), max(a.iters // 2, 3), warmup=1)}
    c = res["c_pillow_loop_plus_upload"]["whole"]["median_ms"]
    for name in files:
        res[name]["pillow_over_this"] = round(c / res[name]["whole"]["median_ms"], 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
