"""CPU suite: the host half of the CLIP quality score (vdx/clip_score.py; InferNet/template/validator/scoring.py:87-147) —
Pillow's bilinear resize tables and pass order against Pillow itself, the CLIPModel state-dict split, the empty-prompt rule,
the pipeline's new flags (off by default) and the C-ABI struct of vdx_clip_preprocess_u8."""
import os
import re

import numpy as np
import pytest
import torch

import vdx  # noqa: F401
from vdx import _lib, ops
from vdx._lib import VdxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(576, 1024), (320, 576), (72, 128), (100, 150), (224, 224)]


def _pass(img, axis, bounds, coeffs):
    """One Pillow 8-bpc resample pass in integers: clip8((2^21 + sum px * k) >> 22) along `axis`."""
    src = np.moveaxis(img, axis, -1).astype(np.int64)
    out = np.empty(src.shape[:-1] + (len(bounds),), np.int64)
    for i, (x0, n) in enumerate(bounds):
        out[..., i] = (1 << 21) + (src[..., x0:x0 + n] * coeffs[i, :n]).sum(-1)
    return np.moveaxis(np.clip(out >> 22, 0, 255).astype(np.uint8), -1, axis)


def emulate_resize(frame, order="hv"):
    H, W = frame.shape[:2]
    xb, xk = ops.clip_resize_coeffs(W)
    yb, yk = ops.clip_resize_coeffs(H)
    if order == "hv":
        return _pass(_pass(frame, 1, xb, xk), 0, yb, yk)
    return _pass(_pass(frame, 0, yb, yk), 1, xb, xk)


def _frame(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("H,W", SIZES)
def test_resize_tables_reproduce_pillow_bit_for_bit(H, W):
    Image = pytest.importorskip("PIL.Image")
    fr = _frame(H, W, H * 7 + W)
    want = np.asarray(Image.fromarray(fr).resize((224, 224), Image.BILINEAR))
    assert np.array_equal(emulate_resize(fr), want)


def test_resize_pass_order_matters():
    """Vertical-then-horizontal is off by 1 LSB at 576x1024: the kernel's horizontal-first order is the one Pillow runs."""
    Image = pytest.importorskip("PIL.Image")
    fr = _frame(576, 1024, 3)
    want = np.asarray(Image.fromarray(fr).resize((224, 224), Image.BILINEAR))
    assert not np.array_equal(emulate_resize(fr, "vh"), want)
    assert np.array_equal(emulate_resize(fr, "hv"), want)


def test_resize_tables_shape_and_lds_band():
    xb, xk = ops.clip_resize_coeffs(1024)
    assert xb.dtype == np.int32 and xk.dtype == np.int32 and xk.shape == (224, 11)
    assert (xb[:, 1] <= xk.shape[1]).all() and (xb.sum(1) <= 1024).all() and (xb[:, 0] >= 0).all()
    assert (np.abs(xk.sum(1) - (1 << 22)) <= xk.shape[1]).all()          # each window's weights sum to 1 in 22-bit
    yb, _ = ops.clip_resize_coeffs(576)
    assert ops.clip_band_span(yb, ops.CLIP_BAND) * 224 * 3 <= ops.CLIP_LDS_MAX


def test_state_dict_split_covers_every_key_and_rejects_extras():
    transformers = pytest.importorskip("transformers")
    from vdx.clip_score import configs_from_dict, split_state_dict
    from vdx.clip_text import CLIPTextModel
    from vdx.clip_vision import CLIPVisionModel
    torch.manual_seed(0)
    m = transformers.CLIPModel(transformers.CLIPConfig())
    sd = m.state_dict()
    text, vision, proj = split_state_dict(sd)
    assert len(text) + len(vision) + len(proj) + 1 == len(sd)              # + logit_scale, ignored on purpose
    tc, vc, pd, eos = configs_from_dict(m.config.to_dict())
    assert (tc.hidden_size, tc.num_hidden_layers, tc.hidden_act, vc.hidden_size, vc.num_hidden_layers, pd, eos) == \
        (512, 12, "quick_gelu", 768, 12, 512, 49407)
    CLIPTextModel(tc).load_transformers_state_dict(text, device="cpu")    # every tower key used (extras raise)
    CLIPVisionModel(vc).load_transformers_state_dict(vision, device="cpu")
    with pytest.raises(VdxError):
        split_state_dict({**sd, "bogus.weight": torch.zeros(1)})
    with pytest.raises(VdxError):
        CLIPVisionModel(vc).load_transformers_state_dict({**vision, "vision_model.extra": torch.zeros(1)}, device="cpu")


def test_empty_prompt_becomes_a_video():
    from vdx.clip_score import prompt_or_default
    assert prompt_or_default("") == prompt_or_default("   ") == prompt_or_default(None) == "a video"
    assert prompt_or_default("a red panda") == "a red panda"


def test_zero_frames_score_zero_before_tokenizing():
    """scoring.py:133-135: no frames -> 0.0, even for a prompt string with no tokenizer at hand (nothing else is looked at)."""
    from vdx.clip_score import CLIPScorer
    from vdx.clip_text import CLIPTextConfig
    from vdx.clip_vision import CLIPVisionConfig
    s = CLIPScorer(CLIPTextConfig(hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8,
                                  hidden_act="quick_gelu"), CLIPVisionConfig())
    q, per = s.score([], "a red panda")
    assert q == 0.0 and per.numel() == 0 and per.dtype == torch.float32
    q, per = s.score(np.zeros((0, 576, 1024, 3), np.uint8), "")
    assert q == 0.0 and per.numel() == 0


def test_text_config_default_activation_is_unchanged():
    from vdx.clip_text import CLIPTextConfig, CLIPTextModel
    assert CLIPTextConfig().hidden_act == "gelu" and CLIPTextConfig.sd2().hidden_act == "gelu"
    with pytest.raises(VdxError):
        CLIPTextModel(CLIPTextConfig(hidden_act="relu"))


def test_clip_flags_default_off_and_old_argv_parses_the_same():
    from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args
    old = ["--num_frames", "24", "--steps", "5", "--mode", "chunk", "--chunk_size", "8", "--prompt", "a cat"]
    a = build_arg_parser().parse_args(old)
    assert a.clip_json is None and a.clip_model is None
    assert config_from_args(a) == DiffuserConfig(num_frames=24, steps=5, mode="chunk", chunk_size=8, prompt="a cat")
    b = build_arg_parser().parse_args(old + ["--clip_json", "s.json", "--clip_model", "/m"])
    assert (b.clip_json, b.clip_model) == ("s.json", "/m") and config_from_args(b) == config_from_args(a)


def test_from_local_refuses_a_missing_directory(tmp_path):
    from vdx.clip_score import CLIPScorer
    with pytest.raises(VdxError):
        CLIPScorer.from_local(str(tmp_path / "nope"))
    with pytest.raises(VdxError):
        CLIPScorer.from_local(str(tmp_path))                                # no config.json


def test_clip_preprocess_args_struct_matches_header_field_order():
    hdr = open(os.path.join(ROOT, "include", "vdx.h")).read()
    body = re.search(r"typedef struct vdx_clip_preprocess_args \{(.*?)\} vdx_clip_preprocess_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        decl = re.sub(r"^(const\s+)?(void\s*\*|int32_t\s*\*|int32_t|size_t)\s*", "", decl)
        names += [n.strip().lstrip("*") for n in decl.split(",")]
    assert names == [f[0] for f in _lib.ClipPreprocessArgs._fields_]
