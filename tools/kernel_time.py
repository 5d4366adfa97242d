#!/usr/bin/env python3
"""Dev tool: wall time of one fused transformer kernel alone, median of 9 launches after 3 warm-up launches.  The library
comes from VDX_LIB_PATH: the product, or a stamps / timing-only -D..._ABL_* build (tools/k8_abl.sh makes K8's).

    tools/kernel_time.py k7     temporal attention, first design (csrc/tattn_fused.hip): level 0 and transformer_in, F = 24
    tools/kernel_time.py k7b    temporal attention, second design (csrc/tattn2.hip): level 0, F = 24 and 16
    tools/kernel_time.py k8     feed-forward (csrc/ff_fused.hip): level 0, F = 24 and 16
"""
import os
os.environ.setdefault("VDX_ALLOW_LAB_BUILD", "1")      # lab tool: may load a stamps / ablation build
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vdx  # noqa: E402,F401
from vdx import ops, packing  # noqa: E402

dev = torch.device("cuda:0")
B, HW = 2, 72 * 128


def r(*s, k=1.0):
    return (torch.randn(*s, device=dev) * k).half()


def k7(inner, F=24):
    t = r(B * F * HW, inner)
    w = [r(inner, inner, k=0.06) for _ in range(4)]
    pq, po = packing.pack_k7_qkv(*w[:3]).contiguous(), packing.pack_k7_out(w[3]).contiguous()
    out = torch.empty_like(t)
    g, b_, bo = r(inner, k=0.1) + 1, r(inner, k=0.1), r(inner, k=0.1)
    return lambda: ops.temporal_attn_block(t, g, b_, pq, po, bo, B=B, F=F, HW=HW, scale=0.125, out=out)


def k7b(F, inner=320):
    t = r(B * F * HW, inner)
    w = [r(inner, inner, k=0.06) for _ in range(4)]
    blob = packing.pack_k7b(*w, r(inner, k=0.1) + 1, r(inner, k=0.1), r(inner, k=0.1), 0.125).contiguous()
    out = torch.empty_like(t)
    return lambda: ops.temporal_attn_block2(t, blob, B=B, F=F, HW=HW, out=out)


def k8(F, inner=320):
    blob = packing.pack_k8(r(8 * inner, inner, k=0.06), r(8 * inner, k=0.1), r(inner, 4 * inner, k=0.03), r(inner, k=0.1),
                           r(inner, k=0.2) + 1, r(inner, k=0.1))
    M = B * F * HW
    t = r(M, inner)
    out = torch.empty_like(t)
    return lambda: ops.ff_block(t, blob, M=M, out=out)


# kernel -> (what varies, its values, launch maker)
KERNELS = {"k7": ("inner", (320, 512), k7), "k7b": ("F", (24, 16), k7b), "k8": ("F", (24, 16), k8)}


def median_ms(launch):
    ts = []
    for i in range(12):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


if len(sys.argv) != 2 or sys.argv[1] not in KERNELS:
    sys.exit("usage: kernel_time.py " + "|".join(KERNELS))
label, values, make = KERNELS[sys.argv[1]]
res = [f"{label} {v}: {median_ms(make(v)):.3f} ms" for v in values]
print(os.path.basename(os.environ.get("VDX_LIB_PATH", "libvdx_hip.so")), " | ".join(res))
