"""The validator's CLIP quality score of a generated video on libvdx_hip.so:

    InferNet/neurons/validator.py:277,898    compute_quality_score_clip(video, prompt)
    InferNet/template/validator/scoring.py:87-147   CLIPScorer.compute_quality_score
        Q = 1/F * sum_i cos(E_text, E_frame_i)        under openai/clip-vit-base-patch32

What it computes, step by step (the same as the reference unless stated):
  * frames: a decoded uint8 RGB clip in any form vdx/frames.py takes.  DEVIATION: the reference re-reads the mp4
    with OpenCV and converts BGR->RGB (:110-121); here the frames the pipeline decoded are scored directly — no lossy
    codec round trip, and OpenCV is not a dependency;
  * Resize((224, 224)) + ToTensor + Normalize (:81-85): Pillow's antialiased bilinear resize, bit for bit, then
    ((u / 255) - mean) / std in fp32 with the ImageNet statistics (0.485, 0.456, 0.406) / (0.229, 0.224, 0.225) —
    the reference's choice, not CLIP's own statistics (`ops.clip_preprocess`); the pixels then enter the tower in fp16;
  * image features: `visual_projection(post_layernorm(ViT(pixels)[:, 0]))` (vdx/clip_vision.py + the projection here).
    transformers >= 5 returns a `BaseModelOutputWithPooling` from `get_image_features`; its `.pooler_output` is this
    vector (the reference's `F.normalize(get_image_features(...))` assumes the 4.x tensor return);
  * text features: the prompt tokenized with `padding=True` (one prompt: no padding, the mask is all ones), an empty
    prompt replaced by "a video" (:97-99), the 12-layer causal text tower with `quick_gelu` (vdx/clip_text.py), pooled
    at the first EOS token (49407, also the largest id, so the legacy argmax rule agrees), then `text_projection`;
  * F.normalize on both sides, per-frame dot products, the mean over frames (:137-140, `ops.clip_cosine_score`);
    zero frames score 0.0 (:133-135).
  DEVIATION: the reference turns every exception into a score of 0.0 (:145-147); here errors raise `VdxError` (a prompt
  longer than 77 tokens, for one, which the reference's model rejects and scores 0.0).

Weights come from a local directory in transformers layout (`from_local`) or from a seeded `transformers.CLIPModel`
(`synthetic`); nothing is downloaded.  `logit_scale` is not part of the score and is ignored.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Optional, Tuple

import torch

from . import frames as _frames, ops
from ._lib import VdxError
from .clip_text import CLIPTextConfig, CLIPTextModel
from .clip_vision import CLIPVisionConfig, CLIPVisionModel

DEFAULT_PROMPT = "a video"
_TEXT_KEYS = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
              "max_position_embeddings", "layer_norm_eps", "hidden_act")
_VISION_KEYS = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size",
                "num_channels", "layer_norm_eps", "hidden_act")
_TOKENIZER_FILES = ("tokenizer.json", "vocab.json")


def prompt_or_default(prompt: Optional[str]) -> str:
    """scoring.py:97-99: an empty or blank prompt is scored as "a video"."""
    return DEFAULT_PROMPT if not prompt or prompt.strip() == "" else prompt


def configs_from_dict(d: dict):
    """A transformers `CLIPConfig` dict (config.json) -> (CLIPTextConfig, CLIPVisionConfig, projection_dim, eos_token_id)."""
    t, v = d.get("text_config") or {}, d.get("vision_config") or {}
    vit_b32_text = dict(hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8,
                        hidden_act="quick_gelu")                                   # transformers' CLIPTextConfig defaults
    tc = CLIPTextConfig(**{**vit_b32_text, **{k: t[k] for k in _TEXT_KEYS if k in t}})
    vc = CLIPVisionConfig(**{k: v[k] for k in _VISION_KEYS if k in v})
    return tc, vc, int(d.get("projection_dim", 512)), int(t.get("eos_token_id", 49407))


def split_state_dict(sd: Dict[str, torch.Tensor]):
    """`CLIPModel.state_dict()` -> (text tower keys, vision tower keys, {visual_projection, text_projection}).
    `logit_scale` is ignored on purpose (it scales logits, not the score); any other key is an error."""
    text, vision, proj = {}, {}, {}
    for k, t in sd.items():
        if k.startswith("text_model."):
            text[k] = t
        elif k.startswith("vision_model."):
            vision[k] = t
        elif k in ("visual_projection.weight", "text_projection.weight"):
            proj[k] = t
        elif k != "logit_scale":
            raise VdxError(f"CLIPScorer: unexpected key in the CLIPModel state dict: {k}")
    for k in ("visual_projection.weight", "text_projection.weight"):
        if k not in proj:
            raise VdxError(f"CLIPScorer: missing key in state dict: {k}")
    return text, vision, proj


class CLIPScorer:
    """`CLIPScorer.compute_quality_score` (scoring.py:87-147) on the HIP path; see the module docstring."""

    def __init__(self, text_cfg: CLIPTextConfig, vision_cfg: CLIPVisionConfig, projection_dim: int = 512,
                 eos_token_id: int = 49407):
        self.text = CLIPTextModel(text_cfg)
        self.vision = CLIPVisionModel(vision_cfg)
        self.projection_dim, self.eos_token_id = projection_dim, eos_token_id
        self.W: Dict[str, torch.Tensor] = {}
        self.tokenizer = None
        self.synthetic_weights = False
        self.device = torch.device("cpu")

    # ---- construction ------------------------------------------------------------------------
    @torch.no_grad()
    def load_transformers_state_dict(self, sd: Dict[str, torch.Tensor], device="cuda"):
        dev = torch.device(device)
        text, vision, proj = split_state_dict(sd)
        self.text.load_transformers_state_dict(text, device=dev)
        self.vision.load_transformers_state_dict(vision, device=dev)
        self.W = {"visual_projection": proj["visual_projection.weight"].to(dev, torch.float16).contiguous(),
                  "text_projection": proj["text_projection.weight"].to(dev, torch.float16).contiguous()}
        self.device = dev
        return self

    @classmethod
    def from_local(cls, path: str, device="cuda") -> "CLIPScorer":
        """A local directory in transformers layout: config.json + model.safetensors or pytorch_model.bin (and the
        tokenizer files, when present).  Only a directory that exists is read; nothing is fetched."""
        if not os.path.isdir(path):
            raise VdxError(f"CLIPScorer.from_local: {path!r} is not a directory (weights are read from disk only)")
        cfgp = os.path.join(path, "config.json")
        if not os.path.exists(cfgp):
            raise VdxError(f"CLIPScorer.from_local: {cfgp} is missing")
        with open(cfgp) as f:
            tc, vc, pd, eos = configs_from_dict(json.load(f))
        from .compat.diffusers_shim import _load_file
        sd = _load_file([os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")])
        if sd is None:
            raise VdxError(f"CLIPScorer.from_local: no model.safetensors or pytorch_model.bin in {path}")
        s = cls(tc, vc, pd, eos).load_transformers_state_dict(sd, device=device)
        if any(os.path.exists(os.path.join(path, f)) for f in _TOKENIZER_FILES):
            import transformers
            s.tokenizer = transformers.CLIPTokenizer.from_pretrained(path, local_files_only=True)
        return s

    @classmethod
    def synthetic(cls, seed: int = 0, device="cuda") -> "CLIPScorer":
        """`transformers.CLIPModel(CLIPConfig())` (ViT-B/32 shapes) with weights drawn under `seed`: the score of a run
        without a checkpoint.  `synthetic_weights` is then True."""
        import transformers
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            model = transformers.CLIPModel(transformers.CLIPConfig())
        tc, vc, pd, eos = configs_from_dict(model.config.to_dict())
        s = cls(tc, vc, pd, eos).load_transformers_state_dict(model.state_dict(), device=device)
        s.synthetic_weights = True
        return s

    # ---- features ----------------------------------------------------------------------------
    @torch.no_grad()
    def image_features(self, frames) -> torch.Tensor:
        """uint8 RGB frames (F, H, W, 3) -> `get_image_features(...).pooler_output` fp16 [F][projection_dim]."""
        if _frames.check(frames, "CLIPScorer")[0] == 0:
            raise VdxError("CLIPScorer.image_features: no frames")
        t = _frames.on_device(frames, self.device)
        pooled = self.vision(t)
        return ops.gemm(pooled, self.W["visual_projection"], M=t.shape[0])

    @torch.no_grad()
    def text_features(self, input_ids: torch.Tensor) -> torch.Tensor:
        """input_ids (B, S <= 77) -> `get_text_features(...).pooler_output` fp16 [B][projection_dim]."""
        ids = input_ids if input_ids.dim() == 2 else input_ids.view(1, -1)
        ids = ids.cpu()
        hid = self.text(ids)[0]                                                     # final_layer_norm output (B, S, D)
        if self.eos_token_id == 2:                                                  # transformers' legacy rule: argmax id
            pos = ids.to(torch.int32).argmax(dim=-1)
        else:                                                                       # the first EOS token
            pos = (ids == self.eos_token_id).to(torch.int32).argmax(dim=-1)
        pooled = hid[torch.arange(ids.shape[0]), pos.to(hid.device)].contiguous()
        return ops.gemm(pooled, self.W["text_projection"], M=ids.shape[0])

    def tokenize(self, prompt: Optional[str], tokenizer=None) -> torch.Tensor:
        tok = tokenizer or self.tokenizer
        if tok is None:
            raise VdxError("CLIPScorer: a prompt string needs a tokenizer (none was given and the weights came without one)")
        return tok(prompt_or_default(prompt), return_tensors="pt", padding=True).input_ids

    @torch.no_grad()
    def score(self, frames, prompt_or_ids, tokenizer=None) -> Tuple[float, torch.Tensor]:
        """-> (Q, per-frame cosines fp32 [F] on the host).  Zero frames -> (0.0, empty) before anything else (:133-135)."""
        if _frames.check(frames, "CLIPScorer")[0] == 0:
            return 0.0, torch.empty(0, dtype=torch.float32)
        t = _frames.on_device(frames, self.device)
        ids = prompt_or_ids if isinstance(prompt_or_ids, torch.Tensor) else self.tokenize(prompt_or_ids, tokenizer)
        if ids.dim() == 2 and ids.shape[0] != 1:
            raise VdxError("CLIPScorer.score: one prompt per video")
        img = self.image_features(t)
        txt = self.text_features(ids)
        mean, per = ops.clip_cosine_score(img, txt[0])
        return float(mean.item()), per.cpu()

    def score_file(self, src, prompt_or_ids, tokenizer=None) -> Tuple[float, torch.Tensor]:
        """`compute_quality_score(video_path, prompt)` (scoring.py:87-147) starting from the FILE like the reference
        (`cv2.VideoCapture(video_path)`, :110): `src` (a path, the file's bytes, or a list of JPEG byte strings) is decoded on the
        GPU (vdx/video.py `read_frames`, bit for bit Pillow's decode) and `score` takes the frames where they are."""
        from .video import read_frames
        return self.score(read_frames(src, device=self.device)[0], prompt_or_ids, tokenizer=tokenizer)
