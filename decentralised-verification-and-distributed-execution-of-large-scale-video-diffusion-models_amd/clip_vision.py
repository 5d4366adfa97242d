"""`CLIPVisionModel` (ViT-B/32) on libvdx_hip.so — the image tower of the validator's quality score:

    InferNet/template/validator/scoring.py:119-124
        frame = self.transform(Image.fromarray(frame)).unsqueeze(0)      # Resize((224, 224)), ToTensor, Normalize
        image_features = self.clip_model.get_image_features(frame)         # openai/clip-vit-base-patch32

`get_image_features` is `visual_projection(post_layernorm(ViT(pixels)[:, 0]))`; this module computes everything up to
`post_layernorm` (the pooled class token), and vdx/clip_score.py applies the projection.  The arithmetic is
`transformers.CLIPVisionModel`: a 32x32/32 patch convolution 3 -> 768 without bias, the class token, 50 position
embeddings, `pre_layrnorm`, 12 pre-LN encoder layers (12 heads of 64, MLP 3072 with `quick_gelu`), eps 1e-5.
tests/test_clip_score_gpu.py checks it against the real dependency (a seeded `transformers.CLIPModel` on the CPU).

Rows are [F*64][768]: each frame's 50 tokens padded to 64 rows (one key tile of the attention kernel).  The front end
(`ops.clip_preprocess`) writes the patch GEMM's operand directly from uint8 frames, so the patch convolution is one GEMM
against `patch_embedding.weight.reshape(768, 3072)`; `ops.clip_vision_embed` adds the class token and the positions and
applies `pre_layrnorm`; LayerNorm / GEMM / `vdx_flash_attn_rows_f16` (q, k, v as column blocks of one projection) /
`vdx_quick_gelu_f16` do the layers.  There is no CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import ops
from ._lib import VdxError

SEQ_PAD = 64       # rows per frame (50 tokens + zero rows)


@dataclass
class CLIPVisionConfig:
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    image_size: int = 224
    patch_size: int = 32
    num_channels: int = 3
    layer_norm_eps: float = 1e-5
    hidden_act: str = "quick_gelu"

    @property
    def num_patches(self) -> int:
        return (self.image_size // self.patch_size) ** 2


class CLIPVisionModel(nn.Module):
    def __init__(self, cfg: Optional[CLIPVisionConfig] = None):
        super().__init__()
        self.cfg = c = cfg or CLIPVisionConfig()
        if (c.image_size, c.patch_size, c.num_channels) != (224, 32, 3):
            raise VdxError("CLIPVisionModel: the front end is built for 224x224 RGB images in 32x32 patches (ViT-B/32)")
        if c.hidden_size != 64 * c.num_attention_heads or c.intermediate_size % 64 or c.hidden_size > 1024:
            raise VdxError("CLIPVisionModel: the kernels need 64-wide heads, hidden <= 1024 and widths that are multiples of 64")
        if c.hidden_act not in ("quick_gelu", "gelu"):
            raise VdxError(f"CLIPVisionModel: hidden_act {c.hidden_act!r} is not built")
        self.W: Dict[str, torch.Tensor] = {}
        self._device = torch.device("cpu")

    @torch.no_grad()
    def load_transformers_state_dict(self, sd: Dict[str, torch.Tensor], device=None):
        """`CLIPVisionModel.state_dict()` keys, with or without the `vision_model.` prefix."""
        dev = torch.device(device) if device is not None else self._device
        c = self.cfg
        sd = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in sd.items()}
        W: Dict[str, torch.Tensor] = {}
        used = set()

        def get(k):
            used.add(k)
            if k not in sd:
                raise VdxError(f"missing key in state dict: {k}")
            return sd[k]

        def put(name, t):
            W[name] = t.to(device=dev, dtype=torch.float16).contiguous()

        D = c.hidden_size
        put("patch", get("embeddings.patch_embedding.weight").reshape(D, -1))      # [D][3*32*32], column c*1024 + ky*32 + kx
        put("cls", get("embeddings.class_embedding"))
        put("pos", get("embeddings.position_embedding.weight"))
        if W["pos"].shape != (c.num_patches + 1, D):
            raise VdxError(f"CLIPVisionModel: position embedding {tuple(W['pos'].shape)} != ({c.num_patches + 1}, {D})")
        for n in ("pre_layrnorm", "post_layernorm"):
            put(n + ".weight", get(n + ".weight"))
            put(n + ".bias", get(n + ".bias"))
        for i in range(c.num_hidden_layers):
            p = f"encoder.layers.{i}"
            for n in ("layer_norm1", "layer_norm2"):
                put(f"{p}.{n}.weight", get(f"{p}.{n}.weight"))
                put(f"{p}.{n}.bias", get(f"{p}.{n}.bias"))
            a = p + ".self_attn"
            put(a + ".qkv.weight", torch.cat([get(a + f".{x}_proj.weight") for x in "qkv"], 0))
            put(a + ".qkv.bias", torch.cat([get(a + f".{x}_proj.bias") for x in "qkv"], 0))
            put(a + ".out.weight", get(a + ".out_proj.weight"))
            put(a + ".out.bias", get(a + ".out_proj.bias"))
            for n in ("fc1", "fc2"):
                put(f"{p}.mlp.{n}.weight", get(f"{p}.mlp.{n}.weight"))
                put(f"{p}.mlp.{n}.bias", get(f"{p}.mlp.{n}.bias"))
        extra = {k for k in sd if k not in used and not k.endswith("position_ids")}
        if extra:
            raise VdxError(f"unexpected keys in state dict: {sorted(extra)[:5]} ... ({len(extra)})")
        self.W, self._device = W, dev
        return self

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        if self.W:
            probe = fn(torch.empty(0, dtype=torch.float16, device=self._device))
            self.W = {k: v.to(probe.device) for k, v in self.W.items()}
            self._device = probe.device
        return out

    def num_parameters(self) -> int:
        return sum(v.numel() for v in self.W.values())

    def _weights(self):
        if not self.W:
            raise VdxError("CLIPVisionModel: no weights loaded")
        if self.W["patch"].device.type != "cuda":
            raise VdxError("CLIPVisionModel: weights are not on a GPU (the encoder has no CPU fallback)")
        return self.W

    @torch.no_grad()
    def forward_patches(self, patches: torch.Tensor, F: int) -> torch.Tensor:
        """Patch-GEMM operand rows fp16 [F*49][3072] (`ops.clip_preprocess`) -> pooled output fp16 [F][768]
        (`post_layernorm` of each frame's class token: `CLIPVisionModel(...).pooler_output`)."""
        c, W = self.cfg, self._weights()
        D, H, P = c.hidden_size, c.num_attention_heads, c.num_patches
        M = F * SEQ_PAD
        emb = ops.gemm(patches, W["patch"], M=F * P)                                   # patch_embedding (no bias)
        x = ops.clip_vision_embed(emb, W["cls"], W["pos"], W["pre_layrnorm.weight"], W["pre_layrnorm.bias"], F=F,
                                  seq_pad=SEQ_PAD, eps=c.layer_norm_eps)
        act = ops.quick_gelu if c.hidden_act == "quick_gelu" else ops.gelu
        for i in range(c.num_hidden_layers):
            p = f"encoder.layers.{i}"
            a = p + ".self_attn"
            ln = ops.layernorm(x, W[p + ".layer_norm1.weight"], W[p + ".layer_norm1.bias"], M=M, eps=c.layer_norm_eps)
            qkv = ops.gemm(ln, W[a + ".qkv.weight"], M=M, bias=W[a + ".qkv.bias"])
            o = ops.flash_attn(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], n_seq=F, sq=SEQ_PAD, skv=P + 1, skv_pad=SEQ_PAD,
                               heads=H, seq_per_kv=1, scale=64 ** -0.5, v_rows=True)
            x = ops.gemm(o, W[a + ".out.weight"], M=M, bias=W[a + ".out.bias"], residual=x)
            ln = ops.layernorm(x, W[p + ".layer_norm2.weight"], W[p + ".layer_norm2.bias"], M=M, eps=c.layer_norm_eps)
            hid = ops.gemm(ln, W[p + ".mlp.fc1.weight"], M=M, bias=W[p + ".mlp.fc1.bias"])
            act(hid, out=hid)
            x = ops.gemm(hid, W[p + ".mlp.fc2.weight"], M=M, bias=W[p + ".mlp.fc2.bias"], residual=x)
        cls_rows = x.view(F, SEQ_PAD, D)[:, 0]                                        # [F][D], row stride 64*D
        return ops.layernorm(cls_rows, W["post_layernorm.weight"], W["post_layernorm.bias"], M=F, eps=c.layer_norm_eps)

    @torch.no_grad()
    def forward(self, frames: torch.Tensor) -> torch.Tensor:
        """uint8 RGB frames (F, H, W, 3) on the GPU -> pooled output fp16 [F][768]."""
        self._weights()
        return self.forward_patches(ops.clip_preprocess(frames), frames.shape[0])
