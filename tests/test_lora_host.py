"""Host side of the LoRA adapters (vdx/lora.py, vdx/options.py `check_lora`; no GPU): both key conventions parse to the same
adapter, the kohya table resolves every Zeroscope module name uniquely, every refusal names the key, alpha present and absent, the
restatement of the merge (tests/lora_ref.py) against float64 within a derived bound, `check_lora`'s refusals, and the job's
options and record without the flag."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import vdx  # noqa: E402,F401
import lora_ref as L  # noqa: E402
from vdx import lora  # noqa: E402
from vdx.clip_text import CLIPTextConfig  # noqa: E402
from vdx.pipeline import FLAG_OF_FIELD, DiffuserConfig, build_arg_parser, config_from_args  # noqa: E402
from vdx.unet3d import UNet3DConfig  # noqa: E402
from vdx.weights import state_dict_spec, synthetic_clip_state_dict  # noqa: E402

TINY = UNet3DConfig(block_out_channels=(64, 128, 128, 128), cross_attention_dim=128, transformer_in_heads=2)
TINY_CLIP = CLIPTextConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2)
B = "down_blocks.0.attentions.0.transformer_blocks.0"
UNET_MODS = [f"{B}.attn1.to_q", f"{B}.attn2.to_k", f"{B}.ff.net.0.proj", "down_blocks.0.attentions.0.proj_in", "down_blocks.0.resnets.0.conv1",
             "down_blocks.0.temp_convs.0.conv1.2", "down_blocks.1.resnets.0.conv_shortcut", "time_embedding.linear_1"]
TEXT_MODS = ["encoder.layers.0.self_attn.q_proj", "encoder.layers.1.mlp.fc1"]


def _parts(rank=4, alpha=None, seed=1):
    us, ts = lora.targets("unet", TINY), lora.targets("text_encoder", TINY_CLIP)
    parts = {("unet", m): v for m, v in L.seeded_adapter(us, UNET_MODS, rank, seed, alpha=alpha).items()}
    parts.update({("text_encoder", m): v for m, v in L.seeded_adapter(ts, TEXT_MODS, rank, seed + 1, alpha=alpha).items()})
    return parts


def _read(sd, **kw):
    return lora.read_lora(sd, "t", unet_cfg=TINY, text_cfg=TINY_CLIP, **kw)


def _same(a, b):
    assert set(a.modules) == set(b.modules)
    for k in a.modules:
        (da, ua, aa), (db, ub, ab) = a.modules[k], b.modules[k]
        assert da.dtype == ua.dtype == torch.float32 and torch.equal(da, db) and torch.equal(ua, ub) and aa == ab, k


def test_clip_spec_is_the_synthetic_table():
    sd = synthetic_clip_state_dict(TINY_CLIP, 11, "cpu")
    assert {k: tuple(v.shape) for k, v in sd.items()} == lora.clip_state_dict_spec(TINY_CLIP)


@pytest.mark.parametrize("alpha", [None, 2.0])
def test_both_conventions_parse_to_identical_adapters(alpha):
    parts = _parts(alpha=alpha)
    peft = _read(L.adapter_file_dict(parts, "peft"))
    _same(peft, _read(L.adapter_file_dict(parts, "kohya")))
    _same(peft, _read(L.adapter_file_dict(parts, "diffusers_old")))
    _same(peft, _read(L.adapter_file_dict(parts, "peft", text_model_prefix=True)))
    _same(peft, _read(L.adapter_file_dict(parts, "kohya", text_model_prefix=True)))
    assert len(peft.of("unet")) == len(UNET_MODS) and len(peft.of("text_encoder")) == len(TEXT_MODS)
    assert peft.record(0.5) == {"name": "t", "scale": 0.5, "rank": 4, "unet_modules": len(UNET_MODS), "text_modules": len(TEXT_MODS)}
    for (comp, m), (down, up, a) in peft.modules.items():
        shape = lora.targets(comp, TINY if comp == "unet" else TINY_CLIP)[m]
        assert tuple(down.shape) == (4, torch.Size(shape[1:]).numel()) and tuple(up.shape) == (shape[0], 4)
        assert a == (4.0 if alpha is None else alpha)                      # absent: alpha = R
        src = parts[(comp, m)]
        assert torch.equal(down, src[0].reshape(4, -1)) and torch.equal(up, src[1].reshape(shape[0], 4))


def test_files_round_trip(tmp_path):
    from safetensors.torch import save_file
    parts = _parts()
    sd = L.adapter_file_dict(parts, "kohya")
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "style.safetensors"))
    torch.save(sd, tmp_path / "style.pt")
    a = lora.read_lora(str(tmp_path / "style.safetensors"), unet_cfg=TINY, text_cfg=TINY_CLIP)
    b = lora.read_lora(tmp_path / "style.pt", unet_cfg=TINY, text_cfg=TINY_CLIP)
    assert a.name == b.name == "style"
    _same(a, b)
    _same(a, _read(sd))
    half = {k: (v.half() if v.dim() else v) for k, v in sd.items()}        # fp16 / bf16 files widen exactly
    h = _read(half)
    assert all(torch.equal(h.modules[k][0], half_d.float()) for k, half_d in
               ((k, half[L.kohya_name(*k) + ".lora_down.weight"].reshape(4, -1)) for k in h.modules))
    _read({k: (v.bfloat16() if v.dim() else v) for k, v in sd.items()})
    for bad in ("https://example.invalid/x.safetensors", str(tmp_path / "missing.safetensors")):
        with pytest.raises(ValueError, match="not a local file"):
            lora.read_lora(bad, unet_cfg=TINY, text_cfg=TINY_CLIP)


def test_kohya_table_resolves_every_zeroscope_name_uniquely():
    cfg = UNet3DConfig.zeroscope()
    mods = lora.targets("unet", cfg)
    spec = state_dict_spec(cfg)
    assert set(mods) == {k[:-7] for k, s in spec.items() if k.endswith(".weight") and len(s) >= 2}
    table = lora.kohya_table(mods)
    assert len(table) == len(mods) and set(table.values()) == set(mods)
    assert all(table[m.replace(".", "_")] == m for m in mods)
    text = lora.targets("text_encoder", CLIPTextConfig.sd2())
    assert len(lora.kohya_table(text)) == len(text) == 23 * 6
    with pytest.raises(ValueError, match="share the kohya name"):
        lora.kohya_table(["a.b_c", "a_b.c"])


def _peft(parts):
    return L.adapter_file_dict(parts, "peft")


def test_every_refusal_names_the_key():
    parts = _parts()
    q = f"unet.{B}.attn1.to_q"

    def refused(sd, match):
        with pytest.raises(ValueError, match=match) as e:
            _read(sd)
        return str(e.value)

    sd = _peft(parts)
    refused({**sd, "unet.down_blocks.9.attentions.0.proj_in.lora_A.weight": torch.zeros(4, 64),
             "unet.down_blocks.9.attentions.0.proj_in.lora_B.weight": torch.zeros(64, 4)}, "down_blocks.9.*does not have")
    refused({**L.adapter_file_dict(parts, "kohya"), "lora_unet_down_blocks_0_attentions_0_proj.lora_down.weight": torch.zeros(4, 64)},
            "lora_unet_down_blocks_0_attentions_0_proj.lora_down.weight.*does not have")
    refused({k: v for k, v in sd.items() if k != q + ".lora_B.weight"}, "attn1.to_q.lora_A.weight.*half")
    refused({k: v for k, v in sd.items() if k != q + ".lora_A.weight"}, "attn1.to_q.lora_B.weight.*half")
    refused({**sd, f"unet.{B}.attn1.to_v.alpha": torch.tensor(1.0)}, "attn1.to_v.alpha.*half")
    refused({**sd, q + ".lora_A.weight": torch.zeros(4, 65)}, "attn1.to_q.lora_A.weight.*does not fit")
    refused({**sd, q + ".lora_B.weight": torch.zeros(65, 4)}, "attn1.to_q.lora_B.weight.*does not fit")
    refused({**sd, q + ".lora_B.weight": torch.zeros(64, 5)}, "attn1.to_q.lora_B.weight.*does not fit")
    conv = "unet.down_blocks.0.resnets.0.conv1"
    refused({**sd, conv + ".lora_A.weight": torch.zeros(4, 64, 1, 9)}, "conv1.lora_A.weight.*does not fit")
    refused({**sd, q + ".lora_A.weight": torch.zeros(513, 64), q + ".lora_B.weight": torch.zeros(64, 513)}, "attn1.to_q.lora_A.weight.*rank 513")
    refused({**sd, q + ".lora_A.weight": torch.zeros(0, 64), q + ".lora_B.weight": torch.zeros(64, 0)}, "attn1.to_q.lora_A.weight.*rank 0")
    for v in (float("nan"), float("inf")):
        refused({**sd, q + ".alpha": torch.tensor(v)}, "attn1.to_q.alpha.*not finite")
        poisoned = sd[q + ".lora_A.weight"].clone()
        poisoned[1, 3] = v
        refused({**sd, q + ".lora_A.weight": poisoned}, "attn1.to_q.lora_A.weight.*non-finite")
        poisoned = sd[q + ".lora_B.weight"].clone()
        poisoned[0, 0] = v
        refused({**sd, q + ".lora_B.weight": poisoned}, "attn1.to_q.lora_B.weight.*non-finite")
    for key in ("lora_unet_x.hada_w1_a", "lora_unet_x.lokr_w1", f"lora_unet_{B.replace('.', '_')}_attn1_to_q.lora_mid.weight",
                q + ".lora_magnitude_vector", "lora_unet_x.dora_scale", q + ".lora_embedding_A"):
        refused({**sd, key: torch.zeros(2, 2)}, key.replace(".", r"\.") + ".*variant")
    refused({**sd, "something.else": torch.zeros(2)}, "something.else.*neither")
    refused({**sd, "vae.decoder.conv_in.lora_A.weight": torch.zeros(2, 2)}, "vae.decoder.*neither")
    refused({**sd, "unet.conv_norm_out.lora_A.weight": torch.zeros(2, 64), "unet.conv_norm_out.lora_B.weight": torch.zeros(64, 2)},
            "conv_norm_out.*does not have")                                # a norm is no target
    refused({**sd, q + ".lora_A.weight": torch.zeros(4, 64, dtype=torch.int32)}, "attn1.to_q.lora_A.weight.*fp16, bf16 or fp32")
    refused({}, "empty")
    refused({**sd, q + ".lora.down.weight": torch.zeros(4, 64)}, "both give down")


def test_linear_adapter_on_a_1x1_conv_and_conv_adapters():
    us = lora.targets("unet", TINY)
    sc = "down_blocks.1.resnets.0.conv_shortcut"
    assert len(us[sc]) == 4 and us[sc][2:] == (1, 1)
    co, ci = us[sc][:2]
    flat = _read({f"unet.{sc}.lora_A.weight": torch.ones(2, ci), f"unet.{sc}.lora_B.weight": torch.ones(co, 2)})
    conv = _read({f"unet.{sc}.lora_A.weight": torch.ones(2, ci, 1, 1), f"unet.{sc}.lora_B.weight": torch.ones(co, 2, 1, 1)})
    _same(flat, conv)
    t = "down_blocks.0.temp_convs.0.conv1.2"
    assert us[t] == (64, 64, 3, 1, 1)
    tc = _read({f"unet.{t}.lora_A.weight": torch.ones(2, 64, 3, 1, 1), f"unet.{t}.lora_B.weight": torch.ones(64, 2, 1, 1, 1)})
    assert tuple(tc.modules[("unet", t)][0].shape) == (2, 192)


def test_merge_scale_is_one_rounding_of_the_float64_quotient():
    import numpy as np
    for scale, alpha, R in ((0.8, 16.0, 16), (0.3, 7.0, 3), (1.0, 1.0, 512), (-0.1, 32.0, 24)):
        assert lora.merge_scale(scale, alpha, R) == float(np.float32(np.float64(scale) * np.float64(alpha) / R)) == L.merge_scale(scale, alpha, R)
    with pytest.raises(ValueError, match="finite"):
        lora.merge_scale(1e30, 1e30, 1)


@pytest.mark.parametrize("n_out,n_in,ranks", [(7, 9, (1,)), (16, 24, (5, 3)), (4, 4, (64,)), (12, 20, (2,) * 8)])
def test_restatement_lies_within_the_derived_bound_of_float64(n_out, n_in, ranks):
    """fp32 sums of R products, A scaled sums and one last sum: before the fp16 rounding an element carries at most
    (R_max + A + 2) roundings of relative size 2^-24 each on partial results no larger than |w| + sum_a |s_a| sum_r |u d| (the
    standard bound for recursive summation, first order; the products' own roundings are among the R_max + 1 of a term)."""
    g = torch.Generator().manual_seed(n_out + n_in)
    W = torch.randn(n_out, n_in, generator=g).half()
    ads = [(torch.randn(n_out, R, generator=g), torch.randn(R, n_in, generator=g), 0.3 + 0.2 * a) for a, R in enumerate(ranks)]
    got = W.float() + L.delta(ads, n_out, n_in)
    exact = W.double()
    mag = W.double().abs()
    for up, down, s in ads:
        s64 = float(L.f32(s))
        exact = exact + s64 * (up.double() @ down.double())
        mag = mag + abs(s64) * (up.double().abs() @ down.double().abs())
    bound = (max(ranks) + len(ranks) + 2) * 2.0 ** -24 * mag
    err = (got.double() - exact).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert torch.equal(L.merge(W, ads), got.half())


# ---- the job's option ----------------------------------------------------------------------------------------------------------
def test_check_lora_refusals(tmp_path):
    from vdx.options import check_lora, resolve
    f = tmp_path / "a.safetensors"
    f.write_bytes(b"x")
    g = tmp_path / "b.pt"
    g.write_bytes(b"x")
    assert check_lora(DiffuserConfig()) is None
    assert check_lora(DiffuserConfig(lora=((str(f), 1), (g, "0.5")))) == ((str(f), 1.0), (str(g), 0.5))
    for bad, match in ((((str(tmp_path / "missing.pt"), 1.0),), "not a local file"),
                       ((("http://example.invalid/a.safetensors", 1.0),), "not a local file"),
                       (((str(f), float("nan")),), "finite"), (((str(f), float("inf")),), "finite"), (((str(f), "much"),), "number"),
                       (((str(f), True),), "finite"),
                       (((str(f), 1.0), (str(tmp_path / "." / "a.safetensors"), 0.5)), "twice"),
                       (tuple((str(f), 1.0) for _ in range(9)), "at most 8"), ((), "non-empty"), (((str(f),),), "pair"), (((5, 1.0),), "string")):
        with pytest.raises(ValueError, match=match):
            check_lora(DiffuserConfig(lora=bad))
    with pytest.raises(ValueError, match="not a local file"):                # inside resolve, before anything loads
        resolve(DiffuserConfig(lora=((str(tmp_path / "missing.pt"), 1.0),)), job=True, world=1)
    opts = resolve(DiffuserConfig(lora=((str(f), 0.5),)), job=True, world=1)
    assert opts.lora == ((str(f), 0.5),) and opts.lora_found is None


def test_flag_and_field():
    from dataclasses import fields
    assert DiffuserConfig().lora is None and "lora" in {x.name for x in fields(DiffuserConfig)}
    assert FLAG_OF_FIELD.get("lora", "lora") == "lora"
    parse = lambda argv: config_from_args(build_arg_parser().parse_args(argv))     # noqa: E731
    assert parse([]).lora is None
    assert parse(["--lora", "a.safetensors", "0.8", "--lora", "b.pt", "-1"]).lora == (("a.safetensors", 0.8), ("b.pt", -1.0))
    assert parse(["--lora", "a.safetensors", "much"]).lora == (("a.safetensors", "much"),)         # for the check to refuse


def test_without_the_flag_options_and_record_are_unchanged():
    from vdx import options
    from vdx.options import RECORD_KEYS, info_options, lora_record, resolve
    assert RECORD_KEYS == ("freeu", "tome", "co_denoise", "tile", "loop", "context_stride", "mask", "negative_prompt", "guidance_rescale")
    for job in (False, True):
        opts = resolve(DiffuserConfig(), job=job, world=1)
        assert opts.lora is None and opts.lora_found is None
        assert lora_record(opts) == {} and info_options(opts, None) == {}
    assert lora_record({"a": 1}) == {} and lora_record({"lora": [1]}) == {"lora": [1]}
    import dataclasses
    opts = dataclasses.replace(resolve(DiffuserConfig(), world=1), lora_found=({"name": "a", "scale": 0.5, "rank": 4, "unet_modules": 2,
                                                                               "text_modules": 0},))
    assert info_options(opts, None) == {"lora": [{"name": "a", "scale": 0.5, "rank": 4, "unet_modules": 2, "text_modules": 0}]}
    assert "lora" not in options.RULES and all("lora" not in str(r) for r in options.RULES.values())     # excluded by none
