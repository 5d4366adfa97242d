"""Prompt travel restated (not a test): the schedule and the blend in plain Python / torch-CPU, every operation a correctly rounded
fp32 operation in the stated order, and a per-frame-text forward of the fp32 oracle.  tests/test_travel_*.py pin vdx/travel.py,
csrc/travel.hip and the UNet's rank-4 text path to these."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def plan(frames, T, loop=False):
    """`frames`: the keys' frames, ascending and distinct, inside [0, T) -> (lo, hi, w): int32, int32, fp32 arrays of length T.
    Frame t lies between the keys a = the last one at or before t and b = the next one: w = (t - f_a) / (f_b - f_a) in float64,
    rounded once to fp32.  Before the first key the first key holds, after the last the last; with `loop` (and more than one key)
    both ranges lie between the last key and the first key one clip length later.  On a key frame, and wherever one key holds,
    lo == hi and w == 0."""
    frames = list(frames)
    assert frames == sorted(set(frames)) and frames and 0 <= frames[0] and frames[-1] < T
    lo, hi, w = np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T, np.float32)
    n = len(frames)
    for t in range(T):
        before = [i for i, f in enumerate(frames) if f <= t]
        after = [i for i, f in enumerate(frames) if f > t]
        if before and after:
            a, b, fa, fb = before[-1], after[0], frames[before[-1]], frames[after[0]]
        elif loop and n > 1:
            a, b = n - 1, 0
            fa, fb = (frames[-1], frames[0] + T) if before else (frames[-1] - T, frames[0])
        else:
            a = b = before[-1] if before else 0
            fa, fb = t, t + 1
        weight = np.float32(np.float64(t - fa) / np.float64(fb - fa)) if a != b else np.float32(0)
        lo[t], hi[t], w[t] = a, (b if weight != 0 else a), weight
    return lo, hi, w


def text_travel(keys, uncond, lo, hi, w, s, L, d=1, ring=False):
    """keys fp16 (n_keys, N, D), uncond fp16 (N, D) -> fp16 (2, L, N, D): item 0 uncond on every frame; item 1, frame f, for the clip
    frame t = s + f d (`ring`: mod T): keys[lo[t]]'s bits where w[t] == 0 or lo[t] == hi[t], else
    fp16(fp32(fp32(1 - w) fp32(a)) + fp32(w fp32(b)))."""
    T = len(lo)
    out = torch.empty((2, L) + tuple(keys.shape[1:]), dtype=torch.float16)
    out[0] = uncond.reshape(keys.shape[1:])
    one = torch.tensor(1.0, dtype=torch.float32)
    for f in range(L):
        t = s + f * d
        if ring and t >= T:
            t -= T
        assert 0 <= t < T
        a, b, wt = keys[int(lo[t])], keys[int(hi[t])], torch.tensor(float(w[t]), dtype=torch.float32)
        if float(wt) == 0.0 or int(lo[t]) == int(hi[t]):
            out[1, f] = a
        else:
            pa = (one - wt) * a.float()
            pb = wt * b.float()
            out[1, f] = (pa + pb).half()
    return out


def oracle_forward_per_frame(model, sample, timestep, text):
    """`oracle/unet3d_ref.py`'s `UNet3DConditionModelRef.forward`, module for module, with text already shaped (B F, N, D): the
    `repeat_interleave` of the text is skipped, nothing else differs."""
    from oracle.unet3d_ref import timestep_embedding
    b, _, nf, h, w = sample.shape
    assert text.dim() == 3 and text.shape[0] == b * nf
    t = torch.as_tensor(timestep)
    if t.dim() == 0:
        t = t[None]
    t = t.expand(b)
    emb = model.time_embedding(timestep_embedding(t, model.cfg.block_out_channels[0]).to(sample.dtype))
    emb = emb.repeat_interleave(nf, dim=0)
    ehs = text
    x = sample.permute(0, 2, 1, 3, 4).reshape(b * nf, -1, h, w)
    x = model.conv_in(x)
    x = model.transformer_in(x, nf)
    skips = [x]
    for blk in model.down_blocks:
        x, outs = blk(x, emb, ehs, nf)
        skips += outs
    x = model.mid_block(x, emb, ehs, nf)
    nup = 2 ** (len(model.cfg.block_out_channels) - 1)
    forward_size = (h % nup != 0) or (w % nup != 0)
    for blk in model.up_blocks:
        size = None
        if forward_size and blk.upsamplers is not None:
            size = skips[-len(blk.resnets) - 1].shape[2:]
        x = blk(x, skips, emb, ehs, nf, size)
    x = model.conv_out(F.silu(model.conv_norm_out(x)))
    return x.reshape(b, nf, -1, h, w).permute(0, 2, 1, 3, 4)


# ---- the parity case of tests/test_travel_gpu.py: tiny UNet, F = 3, three different texts ------------------------------------------
TINY = dict(ch=(64, 128, 128, 128), cross=128, in_heads=2)
PARITY_F, PARITY_H, PARITY_W, PARITY_T, PARITY_BOUND = 3, 16, 16, 501, 4e-3
TEXT_SCALE = 1.0     # unit-scale texts, as every UNet test draws them: swapping two frames' texts moves the oracle 19x the bound (profiles/travel_parity.txt)


def parity_inputs():
    """-> sample fp16 (2, 4, F, H, W), text fp16 (2, F, 77, cross): three different texts per item."""
    g = torch.Generator().manual_seed(77)
    sample = torch.randn(2, 4, PARITY_F, PARITY_H, PARITY_W, generator=g).half()
    text = (TEXT_SCALE * torch.randn(2, PARITY_F, 77, TINY["cross"], generator=g)).half()
    return sample, text


def parity_oracle():
    """-> (the fp32 oracle model on fp16-rounded tiny weights, its state dict)."""
    from oracle.unet3d_ref import UNet3DConditionModelRef, UNet3DConfig as RefCfg, synthetic_state_dict
    sd = synthetic_state_dict(RefCfg.tiny(**TINY), seed=1234)
    ref = UNet3DConditionModelRef(RefCfg.tiny(**TINY)).eval()
    ref.load_state_dict({k: v.half().float() for k, v in sd.items()})
    return ref, sd


def swap_sensitivity(ref=None):
    """rel-L2 by which the oracle's output moves when frames 0 and 2 of the parity case swap their texts (CPU, the oracle alone)."""
    ref = ref or parity_oracle()[0]
    sample, text = parity_inputs()
    swapped = text[:, [2, 1, 0]]
    with torch.no_grad():
        a = oracle_forward_per_frame(ref, sample.float(), torch.tensor(PARITY_T), text.float().reshape(-1, *text.shape[2:]))
        b = oracle_forward_per_frame(ref, sample.float(), torch.tensor(PARITY_T), swapped.float().reshape(-1, *text.shape[2:]))
    return float((a.double() - b.double()).norm() / a.double().norm()), a
