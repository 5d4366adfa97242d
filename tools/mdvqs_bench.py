#!/usr/bin/env python3
"""Time the MD-VQS video-quality term and the authenticity gate (vdx/lpips.py, vdx/mdvqs.py;
InferNet/template/validator/scoring.py:13-67, :269-309) of one video: 24 uint8 frames at 576x1024 already on the GPU, with HIP
events around each stage of LPIPS-AlexNet (resize, stem, the five convolutions with their ReLU / pooling, the five distance
taps), around the whole `LPIPSAlex` call and around `verify_video_authenticity`.  Next to them, the wall time of the fp32
CPU restatement (tests/lpips_ref.py: Pillow + torch-CPU; numpy for the gate) on the same frames, and the box's MFMA probe.
Measured numbers only.  Prints one JSON line; `--out FILE` also writes it.

    python tools/mdvqs_bench.py [--frames 24] [--iters 20] [--no-cpu] [--out profiles/mdvqs_bench.json]"""
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
from vdx import ops  # noqa: E402
from vdx.lpips import TAP_SIZES, LPIPSAlex  # noqa: E402
from vdx.mdvqs import verify_video_authenticity  # noqa: E402


def timed(fn, iters, warmup=3):
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true", help="skip the fp32 CPU restatement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import lpips_ref as R
    dev = torch.device("cuda:0")
    F = a.frames
    host = R.frames_like_video(F, 576, 1024, seed=0)
    frames = torch.from_numpy(host).to(dev)
    m = LPIPSAlex.synthetic(seed=0, device=dev)
    res = {"job": f"LPIPS-AlexNet over {F - 1} consecutive pairs + authenticity gate, {F} frames 576x1024 uint8 on the GPU",
           "device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "box": {"mfma_probe_tflops": round(ops.probe_mfma(dev), 1)}}
    conv = (F, 13, 13, 13, 13, 1, 0)
    st = {}
    u8 = ops.resize_u8(frames, 224, 224, "bilinear")
    st["resize_224"] = timed(lambda: ops.resize_u8(frames, 224, 224, "bilinear"), a.iters)
    cols = ops.lpips_stem(u8, m.lut)
    st["stem_im2col"] = timed(lambda: ops.lpips_stem(u8, m.lut, out=cols), a.iters)
    c1 = ops.gemm(cols, m.w[0], M=F * 3025, bias=m.b[0])
    st["conv1_gemm"] = timed(lambda: ops.gemm(cols, m.w[0], M=F * 3025, bias=m.b[0], out=c1), a.iters)
    p1 = ops.relu_maxpool(c1, n_img=F, H=55, W=55)
    st["relu_maxpool_55"] = timed(lambda: ops.relu_maxpool(c1, n_img=F, H=55, W=55, out=p1), a.iters)
    cols2 = ops.im2col(p1, n_img=F, H=27, W=27, k=5, pad=2)
    st["conv2_im2col"] = timed(lambda: ops.im2col(p1, n_img=F, H=27, W=27, k=5, pad=2, out=cols2), a.iters)
    c2 = ops.gemm(cols2, m.w[1], M=F * 729, bias=m.b[1])
    st["conv2_gemm"] = timed(lambda: ops.gemm(cols2, m.w[1], M=F * 729, bias=m.b[1], out=c2), a.iters)
    x = ops.relu_maxpool(c2, n_img=F, H=27, W=27)
    st["relu_maxpool_27"] = timed(lambda: ops.relu_maxpool(c2, n_img=F, H=27, W=27, out=x), a.iters)
    taps = [c1, c2]
    for i in (2, 3, 4):
        src = x
        x = ops.gemm(src, m.w[i], M=F * 169, mode=ops.CONV3X3, conv=conv, bias=m.b[i])
        st[f"conv{i + 1}_gemm"] = timed(lambda: ops.gemm(src, m.w[i], M=F * 169, mode=ops.CONV3X3, conv=conv, bias=m.b[i], out=x), a.iters)
        st[f"conv{i + 1}_relu"] = timed(lambda: ops.relu(x, out=x), a.iters)
        taps.append(x)
    out = torch.zeros(F - 1, dtype=torch.float32, device=dev)
    for i, (t, s) in enumerate(zip(taps, TAP_SIZES)):
        st[f"distance_tap{i + 1}"] = timed(lambda: ops.lpips_distance(t, m.lin[i], F=F, HW=s * s, out=out), a.iters)
    st["frame_stats"] = timed(lambda: ops.frame_stats(frames), a.iters)
    res["stages"] = st
    res["stages_sum_ms"] = round(sum(v["median_ms"] for k, v in st.items() if k != "frame_stats"), 4)
    res["lpips_whole"] = timed(lambda: m(frames), a.iters)
    res["lpips_whole"]["per_pair"] = m(frames).tolist()
    res["authenticity_whole"] = timed(lambda: verify_video_authenticity(frames, device=dev), a.iters)
    res["authenticity_whole"]["verdict"], res["authenticity_whole"]["stats"] = verify_video_authenticity(frames, device=dev)
    if not a.no_cpu:
        sd = R.synthetic_state_dict(0)
        t0 = time.time()
        want, _ = R.lpips_pairs(host, sd)
        res["cpu_fp32_restatement"] = {"lpips_wall_s": round(time.time() - t0, 3), "threads": torch.get_num_threads(),
                                       "per_pair": want.tolist()}
        t0 = time.time()
        ok, ent, dif = R.authenticity(host)
        res["cpu_fp32_restatement"].update(authenticity_wall_s=round(time.time() - t0, 3), verdict=bool(ok))
        got = torch.tensor(res["lpips_whole"]["per_pair"], dtype=torch.float64)
        res["lpips_worst_rel_err_vs_cpu"] = float(((got - want.double()).abs() / want.double()).max())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
