"""Inputs and CPU yardsticks of tests/test_vae_blocks_gpu.py: the AutoencoderKL mid-block attention (`vdx.vae.AutoencoderKL.
_attention`) alone, in regimes where its softmax is peaked.

  * `state_dicts(C)`: diffusers-shaped decoder and encoder tables of a small VAE whose mid block is C wide (so that the
    product's own loaders pack them; the loaders' folds are not restated here), seeded once per C;
  * `attention_params(C, regime)`: the attention's weights in one of the regimes below, as fp16 values;
  * `reference(C, hw, n, regime)`: the block's input rows, `oracle.vae_ref.VaeAttentionRef` in fp64 on them, and the
    rel-L2 of `diffusers_fp16` against it: the floor of fp16 execution that the product's error is measured against.
    The caller computes it once per case and shares it between the decoder-table and the encoder-table test.

Regimes (gain g on to_q / to_k; the scaled logits have a standard deviation of about g^2):
    a     g = 1: softmax close to uniform (what `synthetic_state_dict` gives)
    b     g = 2.83: logit std about 8, largest probability of a row about 0.75
    c     g = 6
    d12   to_k = to_q, g = 12: every token attends to itself; raw q.k reaches 9e4 at C = 512 (above fp16's 65504)
    d23   to_k = to_q, g = 23: raw q.k reaches 3.4e5; the scaled logits (<= 1.6e4) are well inside fp16
    e     g = 1 and a value bias of magnitude 5: the b_v fold behind to_out decides the output
"""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import vae_ref

GROUPS = 32
REGIMES = {"a": 1.0, "b": 2.83, "c": 6.0, "d12": 12.0, "d23": 23.0, "e": 1.0}
ATT = "mid_block.attentions.0"


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def r16(t):
    """One fp16 rounding of an exactly (fp64) computed result, as an fp64 tensor."""
    return t.half().double()


@functools.lru_cache(maxsize=None)
def state_dicts(C):
    """(decoder table, encoder table, block_out_channels, layers_per_block) of a VAE with a C-wide mid block, fp16 values."""
    from vdx.vae import VaeConfig
    from vdx.weights import synthetic_vae_encoder_state_dict
    ch, layers = (64, 64, 64, C), 1
    dec = vae_ref.synthetic_state_dict(vae_ref.VaeConfig(block_out_channels=ch, layers_per_block=layers), seed=100 + C)
    enc = synthetic_vae_encoder_state_dict(VaeConfig(block_out_channels=ch, layers_per_block=layers), seed=200 + C)
    return {k: v.half() for k, v in dec.items()}, {k: v.half() for k, v in enc.items()}, ch, layers


@functools.lru_cache(maxsize=None)
def attention_params(C, regime):
    """The attention's parameters under their diffusers names (`group_norm.weight`, `to_q.weight`, ... `to_out.0.bias`)."""
    g = torch.Generator().manual_seed(31 * C + sorted(REGIMES).index(regime))
    p = {"group_norm.weight": 1.0 + 0.05 * torch.randn(C, generator=g), "group_norm.bias": 0.02 * torch.randn(C, generator=g)}
    for name in ("to_q", "to_k", "to_v", "to_out.0"):
        p[name + ".weight"] = torch.randn(C, C, generator=g) / math.sqrt(C)
        p[name + ".bias"] = 0.02 * torch.randn(C, generator=g)
    gain = REGIMES[regime]
    p["to_q.weight"] = p["to_q.weight"] * gain
    if regime.startswith("d"):
        p["to_k.weight"], p["to_k.bias"] = p["to_q.weight"], p["to_q.bias"]
    else:
        p["to_k.weight"] = p["to_k.weight"] * gain
    if regime == "e":
        p["to_v.bias"] = 5.0 * torch.sign(torch.randn(C, generator=g))
    return {k: v.half() for k, v in p.items()}


def tables(C, regime):
    """The decoder and encoder state dicts of `state_dicts(C)` with the attention of `attention_params(C, regime)`."""
    dec, enc, ch, layers = state_dicts(C)
    dec, enc = dict(dec), dict(enc)
    for k, v in attention_params(C, regime).items():
        dec[f"decoder.{ATT}.{k}"] = v
        enc[f"encoder.{ATT}.{k}"] = v
    return dec, enc, ch, layers


def rows_to_nchw(rows, n, hh, ww):
    return rows.reshape(n, hh, ww, -1).permute(0, 3, 1, 2).contiguous()


def nchw_to_rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def diffusers_fp16(p, x, n, hh, ww):
    """The block as diffusers runs it in fp16, every op exact and its output rounded to fp16 once: GroupNorm, to_q / to_k /
    to_v, baddbmm(alpha = 1/sqrt(C)) (the SCALED scores are what is stored), the upcast softmax cast back, P.V, to_out, the
    residual add.  x: rows [n*hh*ww][C] (fp16 values) -> rows, fp64."""
    C, S = x.shape[1], hh * ww
    d = {k: v.double() for k, v in p.items()}
    x = x.double()
    t = F.group_norm(x.reshape(n, S, C).transpose(1, 2), GROUPS, d["group_norm.weight"], d["group_norm.bias"], 1e-6)
    t = r16(t.transpose(1, 2))                                                       # (n, S, C)
    q, k, v = (r16(t @ d[f"to_{m}.weight"].t() + d[f"to_{m}.bias"]) for m in "qkv")
    s = r16((q @ k.transpose(1, 2)) * (1.0 / math.sqrt(C)))
    pr = r16(torch.softmax(s, dim=-1))
    o = r16(pr @ v)
    o = r16(o @ d["to_out.0.weight"].t() + d["to_out.0.bias"])
    return r16(o.reshape(n * S, C) + x)


def reference(C, hw, n, regime):
    """(x rows fp16 [n*S][C], fp64 reference rows, floor): floor = rel-L2 of `diffusers_fp16` against the fp64 reference."""
    hh, ww = hw
    S = hh * ww
    g = torch.Generator().manual_seed(C + 7 * S + n)
    x = (torch.randn(n * S, C, generator=g) + 0.5 * torch.randn(1, C, generator=g)).half()
    p = attention_params(C, regime)
    ref = vae_ref.VaeAttentionRef(C, GROUPS).double().eval()
    ref.load_state_dict({k: v.double() for k, v in p.items()})
    with torch.no_grad():
        want = nchw_to_rows(ref(rows_to_nchw(x.double(), n, hh, ww)))
        floor = rel_l2(diffusers_fp16(p, x, n, hh, ww), want)
    return x, want, floor
