"""Regional prompts restated (the yardstick of tests/test_region_*.py; vdx/region.py and csrc/region.hip are what it measures).

A job has the base prompt (text 0) and R regions (mask, text), 1 <= R <= 7; a mask is uint8 (H, W) or (T, H, W), 0..255.

Weights (float64, `weights`): `a_r` of a latent cell is the mean of mask / 255 over its 8x8 pixels; the level with downsample
factor `down` has the grid (ceil(h / down), ceil(w / down)) and its cell (y, x) the mean of `a_r` over the latent cells
[y down, min((y+1) down, h)) x [x down, min((x+1) down, w)); a_0 = max(0, 1 - sum_r a_r); w_j = a_j / sum_j a_j, rounded once to
fp32.  Written with plain loops over the cells.

Blend (`blend`, torch-CPU): row (f, p) of a window is the clip frame tau = s + f d (`ring`: mod T);
out = fp16(sum_j fp32(w_j[tau, p]) fp32(sub_j[row])) in ascending j, every product and every add an fp32 operation of its own, the
terms with w_j == 0 (and the inputs that are None) skipped, the first remaining term starting the sum; where some w_j == 1.0f the
row is sub_j's bits (the first such j); no term at all gives +0.

Oracle (`couple`): the fp32 oracle UNet with the `attn2` of every spatial transformer wrapped in the attention-couple form,
`sum_j w_j attn2(x, text_j)` on the conditional item's frames — equal to blending the sub-blocks in exact arithmetic, because
the weights of a cell sum to 1.  oracle/ itself is unchanged."""
import contextlib

import numpy as np
import torch


def level_grid(h, w, down):
    return -(-h // down), -(-w // down)


def weights(masks, T, h, w, levels):
    """masks: uint8 arrays (8h, 8w) or (T, 8h, 8w) -> [fp32 (T, hh ww, R + 1) per level], by the definition, cell by cell."""
    lat = []
    for m in masks:
        m = np.asarray(m)
        m = np.broadcast_to(m if m.ndim == 3 else m[None], (T, 8 * h, 8 * w)).astype(np.float64) / 255.0
        a = np.zeros((T, h, w))
        for y in range(h):
            for x in range(w):
                a[:, y, x] = m[:, 8 * y:8 * y + 8, 8 * x:8 * x + 8].reshape(T, 64).sum(axis=1) / 64.0
        lat.append(a)
    out = []
    for lev in range(levels):
        down = 1 << lev
        hh, ww = level_grid(h, w, down)
        tab = np.zeros((T, hh * ww, len(masks) + 1), np.float32)
        for y in range(hh):
            for x in range(ww):
                y1, x1 = min((y + 1) * down, h), min((x + 1) * down, w)
                n = (y1 - y * down) * (x1 - x * down)
                a = np.stack([l[:, y * down:y1, x * down:x1].reshape(T, n).sum(axis=1) / n for l in lat], axis=1)      # (T, R)
                a = np.concatenate([np.maximum(0.0, 1.0 - a.sum(axis=1, keepdims=True)), a], axis=1)
                tab[:, y * ww + x] = (a / a.sum(axis=1, keepdims=True)).astype(np.float32)
        out.append(tab)
    return out


def window_frames(T, s, L, d=1, ring=False):
    return [(s + f * d) - T if ring and s + f * d >= T else s + f * d for f in range(L)]


def blend(inputs, table, s, L, d=1, ring=False):
    """inputs: fp16 CPU tensors (L S, C) or None; table: fp32 (T, S, n) numpy or tensor -> fp16 (L S, C)."""
    table = torch.as_tensor(np.asarray(table), dtype=torch.float32)
    T, S, n = table.shape
    assert len(inputs) == n
    w = torch.cat([table[tau] for tau in window_frames(T, s, L, d, ring)])               # (L S, n)
    for j in range(n):
        if inputs[j] is None:
            w[:, j] = 0.0
    first = next(t for t in inputs if t is not None)
    M, C = first.shape
    assert M == L * S
    acc = torch.zeros(M, C, dtype=torch.float32)
    started = torch.zeros(M, dtype=torch.bool)
    for j in range(n):
        if inputs[j] is None:
            continue
        use = w[:, j] != 0
        term = w[:, j:j + 1] * inputs[j].float()                                        # one fp32 product
        acc = torch.where((use & ~started)[:, None], term, torch.where(use[:, None], acc + term, acc))
        started |= use
    out = acc.half()
    chosen = torch.zeros(M, dtype=torch.bool)
    for j in range(n):
        if inputs[j] is None:
            continue
        one = (w[:, j] == 1.0) & ~chosen
        out = torch.where(one[:, None], inputs[j], out)
        chosen |= one
    return out


@contextlib.contextmanager
def couple(model, texts, tables, grids, window, B, F):
    """Inside: `model` (oracle/unet3d_ref.py `UNet3DConditionModelRef`) runs every spatial transformer's `attn2` as
    `sum_j w_j attn2(x, texts[j])` on the LAST of its B items' F frames; the other items keep the text they are called with.
    texts: fp32 (R + 1, N, D), text 0 the base; tables: [(T, S_l, R + 1)] per level, grids: [(hh, ww)]; window: (s, L, d, ring)."""
    from oracle.unet3d_ref import Transformer2DModel
    s, L, d, ring = window
    assert L == F
    cells = [hh * ww for hh, ww in grids]
    assert len(set(cells)) == len(cells), "the levels are told apart by their cell counts"
    taus = window_frames(tables[0].shape[0], s, L, d, ring)
    patched = []
    for mod in model.modules():
        if not isinstance(mod, Transformer2DModel):
            continue
        attn = mod.transformer_blocks[0].attn2

        def forward(x, ctx=None, attn=attn, plain=attn.forward):
            n, S, _ = x.shape
            assert n == B * F
            tab = torch.as_tensor(np.asarray(tables[cells.index(S)]), dtype=torch.float64)[taus]          # (F, S, R + 1)
            out = plain(x, ctx).clone()
            xc = x[(B - 1) * F:]
            acc = torch.zeros_like(xc, dtype=torch.float64)
            for j in range(texts.shape[0]):
                acc += tab[:, :, j:j + 1] * plain(xc, texts[j][None].expand(F, -1, -1).to(x.dtype)).double()
            out[(B - 1) * F:] = acc.to(x.dtype)
            return out

        attn.forward = forward
        patched.append(attn)
    try:
        yield
    finally:
        for attn in patched:
            del attn.forward


# ---- the parity case of tests/test_region_gpu.py: tiny UNet, F = 3, base + two soft-edged regions (one per-frame) -----------------
TINY = dict(ch=(64, 128, 128, 128), cross=128, in_heads=2)
PARITY_F, PARITY_H, PARITY_W, PARITY_T, PARITY_BOUND = 3, 16, 16, 501, 4e-3
TEXT_SCALE = 1.0


def parity_masks():
    """Region 1: static, the left part of the frame with a soft edge (a ramp 255 -> 0 over 32 pixels); region 2: per-frame, a soft
    disc that moves right with the frames.  Together they leave the base some of the frame and overlap in part of it."""
    H, W = 8 * PARITY_H, 8 * PARITY_W
    x = np.arange(W)[None, :].repeat(H, 0).astype(np.float64)
    y = np.arange(H)[:, None].repeat(W, 1).astype(np.float64)
    left = np.clip((56.0 - x) / 32.0, 0.0, 1.0)
    m1 = np.round(255 * left).astype(np.uint8)
    m2 = np.stack([np.round(255 * np.clip((40.0 - np.hypot(x - (60 + 20 * f), y - 80)) / 16.0, 0.0, 1.0)).astype(np.uint8)
                   for f in range(PARITY_F)])
    return m1, m2


def parity_inputs():
    """-> sample fp16 (2, 4, F, H, W), text fp16 (2, 77, cross) [uncond, base], region texts fp16 (2, 77, cross)."""
    g = torch.Generator().manual_seed(91)
    sample = torch.randn(2, 4, PARITY_F, PARITY_H, PARITY_W, generator=g).half()
    text = (TEXT_SCALE * torch.randn(2, 77, TINY["cross"], generator=g)).half()
    rtext = (TEXT_SCALE * torch.randn(2, 77, TINY["cross"], generator=g)).half()
    return sample, text, rtext


def parity_oracle():
    from oracle.unet3d_ref import UNet3DConditionModelRef, UNet3DConfig as RefCfg, synthetic_state_dict
    sd = synthetic_state_dict(RefCfg.tiny(**TINY), seed=1234)
    ref = UNet3DConditionModelRef(RefCfg.tiny(**TINY)).eval()
    ref.load_state_dict({k: v.half().float() for k, v in sd.items()})
    return ref, sd


def oracle_regional(ref, sample, text, rtext, tables, grids, window):
    """The oracle's output fp32 for the batch `sample` with regional prompts on its last item."""
    B, F = sample.shape[0], sample.shape[2]
    texts = torch.cat([text[B - 1:].float(), rtext.float()])
    with torch.no_grad(), couple(ref, texts, tables, grids, window, B, F):
        return ref(sample.float(), torch.tensor(PARITY_T), text.float()).sample


def parity_case(ref=None):
    """-> (moved, want, tables, grids): the oracle's regional output `want`, and the rel-L2 `moved` by which it changes when the
    two regions swap their texts (CPU, the oracle alone): the power of the parity test."""
    ref = ref or parity_oracle()[0]
    sample, text, rtext = parity_inputs()
    levels = len(TINY["ch"])
    tables = weights(parity_masks(), PARITY_F, PARITY_H, PARITY_W, levels)
    grids = [level_grid(PARITY_H, PARITY_W, 1 << l) for l in range(levels)]
    window = (0, PARITY_F, 1, False)
    want = oracle_regional(ref, sample, text, rtext, tables, grids, window)
    other = oracle_regional(ref, sample, text, rtext.flip(0), tables, grids, window)
    return float((want.double() - other.double()).norm() / want.double().norm()), want, tables, grids
