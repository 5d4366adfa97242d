"""INT8 score product for the spatial self-attention (SageAttention: Zhang et al., "SageAttention: Accurate 8-Bit Attention
for Plug-and-play Inference Acceleration", ICLR 2025; unpinned): Q.K^T runs on the int8 matrix instruction with the keys
smoothed by their per-image mean and one scale per block of 64 tokens; softmax and P.V stay as the fp16 kernel has them.  The
kernels are `ops.attn_quant_i8` and `ops.flash_attn_i8` (csrc/flash_i8.hip; include/vdx.h states the
definition).  The host side lives here: the parameters' check, the per-level rule and the record; the switch is
`UNet3DConditionModel.enable_quant_attn` (vdx/unet3d.py).

The method is restated, not ported: the `sageattention` package is not pinned against.  tests/quantattn_ref.py restates the
quantiser and the attention on the quantised operands."""
from typing import List

MODE = "qk_int8"    # the one mode: int8 Q.K^T, fp16 P.V
BLOCK = 64          # tokens per quantisation block


def check_params(max_downsample=1) -> dict:
    """The parameters as the record {"mode", "max_downsample"}; `ValueError` for a max_downsample outside {1, 2, 4, 8}."""
    if isinstance(max_downsample, bool) or not isinstance(max_downsample, int):
        raise ValueError(f"quant_attn: max_downsample must be an integer, got {max_downsample!r}")
    if max_downsample not in (1, 2, 4, 8):
        raise ValueError(f"quant_attn: max_downsample must be 1, 2, 4 or 8, got {max_downsample!r}")
    return {"mode": MODE, "max_downsample": max_downsample}


def applies(params: dict, down: int) -> bool:
    """Does a level with downsample factor `down` take the int8 path?"""
    return down <= params["max_downsample"]


def levels(params: dict, hh: int, ww: int, n_levels: int = 4) -> List[dict]:
    """The levels of a UNet on an (hh, ww) level-0 frame whose self-attention takes the int8 path:
    [{"down", "tokens", "blocks"}], `blocks` being the quantisation blocks of a frame."""
    out = []
    for lvl in range(n_levels):
        if applies(params, 1 << lvl):
            out.append({"down": 1 << lvl, "tokens": hh * ww, "blocks": (hh * ww + BLOCK - 1) // BLOCK})
        hh, ww = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
    return out
