"""CPU suite: the AutoencoderKL-decode oracle (structural pins — the diffusers boundary is parity-unpinned,
oracle/__init__.py) and the product's weight ingest for it."""
import math

import numpy as np
import pytest
import torch

import vdx  # noqa: F401
from vdx._lib import VdxError
from vdx.vae import AutoencoderKL, VaeConfig, qk_fold

from oracle import vae_ref

import vae_blocks_ref as blocks


def test_vae_oracle_structure_matches_published_decoder():
    with torch.device("meta"):
        m = vae_ref.AutoencoderKLRef(vae_ref.VaeConfig.sd())
    # Stable-Diffusion AutoencoderKL: 83 653 863 parameters = encoder 34 163 592 + quant_conv 72
    # + post_quant_conv 20 + decoder 49 490 179
    assert sum(p.numel() for p in m.decoder.parameters()) == 49_490_179
    assert sum(p.numel() for p in m.post_quant_conv.parameters()) == 20
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert len(sd) == 140
    assert sd["post_quant_conv.weight"] == (4, 4, 1, 1)
    assert sd["decoder.conv_in.weight"] == (512, 4, 3, 3)
    assert sd["decoder.mid_block.attentions.0.to_q.weight"] == (512, 512)
    assert sd["decoder.mid_block.attentions.0.group_norm.weight"] == (512,)
    assert sd["decoder.up_blocks.2.resnets.0.conv_shortcut.weight"] == (256, 512, 1, 1)
    assert sd["decoder.up_blocks.3.resnets.0.conv_shortcut.weight"] == (128, 256, 1, 1)
    assert "decoder.up_blocks.3.upsamplers.0.conv.weight" not in sd
    assert sd["decoder.up_blocks.2.upsamplers.0.conv.weight"] == (256, 256, 3, 3)
    assert sd["decoder.conv_out.weight"] == (3, 128, 3, 3)


def test_vae_oracle_decodes_8x_and_maps_frames_like_the_reference():
    cfg = vae_ref.VaeConfig.tiny()
    m = vae_ref.AutoencoderKLRef(cfg).eval()
    m.load_state_dict(vae_ref.synthetic_state_dict(cfg))
    lat = torch.randn(1, 4, 2, 4, 8, generator=torch.Generator().manual_seed(3))
    frames = vae_ref.frames_from_latents(m, lat)
    assert len(frames) == 2 and frames[0].shape == (32, 64, 3) and frames[0].dtype == np.uint8
    with torch.no_grad():
        x = m.decode(lat[:, :, 1] / 0.18215).sample[0].permute(1, 2, 0)
    want = ((x * 0.5 + 0.5).clamp(0, 1) * 255).byte().numpy()      # .byte() truncates
    assert np.array_equal(frames[1], want)
    assert frames[1].min() >= 0 and frames[1].max() <= 255 and frames[1].std() > 1


def test_vae_weight_ingest_covers_every_decoder_key():
    with torch.device("meta"):
        ref = vae_ref.AutoencoderKLRef(vae_ref.VaeConfig.sd())
    sd = dict(ref.state_dict())
    m = AutoencoderKL(VaeConfig.sd()).load_diffusers_state_dict(sd, device="meta")
    # packed = decoder + post_quant_conv folded into conv_in, conv_in K 45 -> 64, conv_out rows 3 -> 64, no value bias
    assert m.num_parameters() == 49_490_179 - 512 * 36 + 512 * 64 - 512 + 61 * (9 * 128 + 1)
    assert m.config.scaling_factor == 0.18215 and m.config.latent_channels == 4
    # a full AutoencoderKL checkpoint also carries the encoder half: accepted and dropped
    sd["encoder.conv_in.weight"] = torch.empty(128, 3, 3, 3, device="meta")
    sd["quant_conv.weight"] = torch.empty(8, 8, 1, 1, device="meta")
    AutoencoderKL(VaeConfig.sd()).load_diffusers_state_dict(sd, device="meta")
    sd["decoder.bogus.weight"] = torch.empty(1, device="meta")
    with pytest.raises(VdxError):
        AutoencoderKL(VaeConfig.sd()).load_diffusers_state_dict(sd, device="meta")


def test_vae_decode_has_no_cpu_path():
    cfg = vae_ref.VaeConfig.tiny()
    m = AutoencoderKL(VaeConfig(block_out_channels=cfg.block_out_channels))
    m.load_diffusers_state_dict({k: v.half() for k, v in vae_ref.synthetic_state_dict(cfg).items()})
    with pytest.raises(VdxError):
        m.decode(torch.zeros(1, 4, 8, 8, dtype=torch.float16))


def _loaded_attention(C, regime):
    """Both loaders on the CPU on the tables of tests/vae_blocks_ref.py -> [(packed table, key prefix)], the raw parameters."""
    dec, enc, ch, layers = blocks.tables(C, regime)
    m = AutoencoderKL(VaeConfig(block_out_channels=ch, layers_per_block=layers))
    m.load_diffusers_state_dict(dec).load_diffusers_encoder_state_dict(enc)
    return [(m.W, f"decoder.{blocks.ATT}."), (m.E, f"encoder.{blocks.ATT}.")], blocks.attention_params(C, regime)


@pytest.mark.parametrize("C", [128, 512])
def test_vae_value_bias_is_folded_behind_to_out(C):
    """P.(V + 1 b_v^T) = P.V + b_v: the packed to_out bias is b_out + W_out.b_v (fp64) to one fp16 rounding, with a value bias
    of magnitude 5 that dominates it, and no to_v.bias is kept."""
    tabs, p = _loaded_attention(C, "e")
    want = p["to_out.0.bias"].double() + p["to_out.0.weight"].double() @ p["to_v.bias"].double()
    assert float(want.abs().max()) > 1.0
    for T, a in tabs:
        assert a + "to_v.bias" not in T and T[a + "to_out.0.bias"].dtype == torch.float16
        err = (T[a + "to_out.0.bias"].double() - want).abs()
        ulp = 2.0 ** torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -14))) * 2.0 ** -10
        assert (err <= 0.5 * ulp * (1 + 2.0 ** -8)).all(), float((err / ulp).max())   # 2^-8: the loader forms it in fp32
        assert torch.equal(T[a + "to_out.0.weight"], p["to_out.0.weight"])


@pytest.mark.parametrize("C,regime", [(128, "a"), (512, "a"), (512, "d23")])
def test_vae_to_q_carries_a_power_of_two_of_the_softmax_scale(C, regime):
    """The fp16 scores stay finite wherever diffusers' scaled ones do: packed to_q = to_q * pre with pre a power of two
    <= 1/sqrt(C), and the scale handed to the softmax restores to_q / sqrt(C) - exactly for every weight whose packed value
    is a normal fp16 number, to half a subnormal step below that."""
    pre, scale = qk_fold(C)
    assert math.frexp(pre)[0] == 0.5 and pre * math.sqrt(C) <= 1.0 < 2 * pre * math.sqrt(C)
    assert 1.0 <= scale < 2.0 and math.isclose(pre * scale, 1.0 / math.sqrt(C), rel_tol=2.0 ** -52)
    assert qk_fold(512)[0] == 2.0 ** -5
    tabs, p = _loaded_attention(C, regime)
    for T, a in tabs:
        for kind in ("weight", "bias"):
            raw, packed = p[f"to_q.{kind}"].double(), T[a + f"to_q.{kind}"].double()
            normal = (raw * pre).abs() >= 2.0 ** -14
            assert normal.float().mean() > 0.9 or kind == "bias"
            assert torch.equal(packed[normal] / pre, raw[normal])
            assert torch.equal(packed[normal] * scale, raw[normal] * (pre * scale))               # pre * scale: 1/sqrt(C) as fp64 has it
            assert torch.allclose(packed[normal] * scale, raw[normal] / math.sqrt(C), rtol=2.0 ** -50, atol=0.0)
            assert ((packed / pre - raw).abs() <= 2.0 ** -25 / pre).all()
            assert torch.equal(T[a + f"to_k.{kind}"], p[f"to_k.{kind}"])                      # to_k is packed as it is
