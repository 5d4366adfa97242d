"""CPU suite of video-to-video refinement: the encoder's structure and ingest, the truncated schedule, Pillow's bicubic
coefficients (emulated in numpy against PIL itself), and the CLI's unchanged text-to-video configuration."""
import numpy as np
import pytest
import torch

import vdx  # noqa: F401
from vdx import ops
from vdx._lib import VdxError
from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args, vid2vid_timesteps
from vdx.scheduler import DDIMScheduler
from vdx.vae import AutoencoderKL, VaeConfig
from vdx.weights import synthetic_vae_encoder_state_dict, synthetic_vae_state_dict

import vae_encoder_ref as ref

TINY = VaeConfig(block_out_channels=(64, 64, 128, 128))      # the synthetic:tiny VAE widths


def test_encoder_restatement_structure():
    with torch.device("meta"):
        m = ref.AutoencoderKLEncoderRef(VaeConfig.sd())
    assert sum(p.numel() for p in m.encoder.parameters()) == 34_163_592     # tests/test_vae_host.py: the published split
    assert sum(p.numel() for p in m.quant_conv.parameters()) == 72
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert len(sd) == 108
    assert sd["encoder.conv_in.weight"] == (128, 3, 3, 3)
    assert sd["encoder.down_blocks.0.downsamplers.0.conv.weight"] == (128, 128, 3, 3)
    assert sd["encoder.down_blocks.1.resnets.0.conv_shortcut.weight"] == (256, 128, 1, 1)
    assert sd["encoder.down_blocks.2.resnets.0.conv_shortcut.weight"] == (512, 256, 1, 1)
    assert "encoder.down_blocks.3.downsamplers.0.conv.weight" not in sd
    assert sd["encoder.mid_block.attentions.0.to_q.weight"] == (512, 512)
    assert sd["encoder.conv_out.weight"] == (8, 512, 3, 3)
    assert sd["quant_conv.weight"] == (8, 8, 1, 1)
    syn = synthetic_vae_encoder_state_dict(VaeConfig.sd())
    assert {k: tuple(v.shape) for k, v in syn.items()} == sd


def test_encoder_ingest_covers_every_key_and_refuses_unknown():
    cfg = TINY
    sd = synthetic_vae_encoder_state_dict(cfg, seed=8)
    vae = AutoencoderKL(cfg).load_diffusers_encoder_state_dict(sd, device="cpu")
    assert vae.W == {} and vae.num_parameters() == 0            # the decoder's table and its meaning are untouched
    E = vae.E
    assert E["encoder.conv_in.weight"].shape == (64, 64)        # K = 27 padded to 64
    assert E["encoder.conv_out.weight"].shape == (64, 9 * 128) and E["encoder.conv_out.bias"].shape == (64,)
    # quant_conv folded exactly: W' = Wq . Wout, b' = Wq . bout + bq
    wq = sd["quant_conv.weight"].float().reshape(8, 8)
    want_b = wq @ sd["encoder.conv_out.bias"].float() + sd["quant_conv.bias"].float()
    assert torch.equal(E["encoder.conv_out.bias"][:8], want_b.half())
    assert not E["encoder.conv_out.bias"][8:].any()
    with pytest.raises(VdxError, match="unexpected encoder keys"):
        AutoencoderKL(cfg).load_diffusers_encoder_state_dict(dict(sd, **{"encoder.extra.weight": torch.zeros(1)}), device="cpu")
    # a whole VAE table: decoder keys are ignored here, encoder keys are still dropped by the decoder ingest
    both = dict(sd, **synthetic_vae_state_dict(cfg, 7))
    AutoencoderKL(cfg).load_diffusers_encoder_state_dict(both, device="cpu")
    d = AutoencoderKL(cfg).load_diffusers_state_dict(both, device="cpu")
    assert d.E == {} and not any(k.startswith("encoder.") for k in d.W)


def test_encoder_ingest_missing_keys_each_refused():
    cfg = TINY
    sd = synthetic_vae_encoder_state_dict(cfg, seed=8)
    for k in ("encoder.down_blocks.2.downsamplers.0.conv.bias", "quant_conv.weight", "encoder.mid_block.attentions.0.to_v.bias"):
        bad = {kk: v for kk, v in sd.items() if kk != k}
        with pytest.raises(VdxError, match="missing key"):
            AutoencoderKL(cfg).load_diffusers_encoder_state_dict(bad, device="cpu")


def test_synthetic_decoder_table_unchanged_by_the_encoder_one():
    a = synthetic_vae_state_dict(TINY, 7)
    synthetic_vae_encoder_state_dict(TINY, 8)
    b = synthetic_vae_state_dict(TINY, 7)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert not any(k.startswith(("encoder.", "quant_conv.")) for k in a)


@pytest.mark.parametrize("steps", [1, 20, 25, 50])
def test_vid2vid_timesteps_table(steps):
    s = DDIMScheduler()
    s.set_timesteps(steps)
    full = s._host_timesteps
    for strength in (0.01, 0.1, 0.25, 0.3, 0.5, 0.6, 0.61, 0.75, 0.99, 1.0):
        init = min(int(steps * strength), steps)
        ts = vid2vid_timesteps(s, steps, strength)
        assert ts == full[max(steps - init, 0):]
        assert len(ts) == init
    if steps == 50:
        ts = vid2vid_timesteps(s, 50, 0.6)
        assert len(ts) == 30 and ts[0] == 581 and ts[-1] == 1
        # the DDIM step keeps the full schedule's spacing: from 581 to prev_t 561 (1000 // 50), not to 581 - 1000 // 30
        a = s.alphas_cumprod
        want = tuple(float(v) for v in ((1 - a[581]) ** 0.5, a[581] ** 0.5, a[561] ** 0.5, (1 - a[561]) ** 0.5))
        assert s.coefficients(ts[0]) == want
        assert ts[1] == 561


def test_vid2vid_timesteps_errors():
    s = DDIMScheduler()
    s.set_timesteps(20)
    for bad in (0.0, -0.1, 1.01, 2.0):
        with pytest.raises(ValueError, match="strength"):
            vid2vid_timesteps(s, 20, bad)
    with pytest.raises(ValueError, match="steps"):
        vid2vid_timesteps(s, 0, 0.5)
    with pytest.raises(ValueError, match="set for"):
        vid2vid_timesteps(s, 25, 0.5)


def _pass(img, bounds, coeffs, axis):
    """One integer pass of Pillow's resample along `axis` (uint8 intermediate)."""
    src = np.moveaxis(img, axis, -1).astype(np.int64)
    out = np.empty(src.shape[:-1] + (len(bounds),), np.int64)
    for o, (x0, n) in enumerate(bounds):
        out[..., o] = (1 << 21) + (src[..., x0:x0 + n] * coeffs[o, :n]).sum(-1)
    return np.moveaxis(np.clip(out >> 22, 0, 255).astype(np.uint8), -1, axis)


def emulate_bicubic(img, W, H):
    Hi, Wi = img.shape[:2]
    if Wi != W:
        b, k = ops.clip_resize_coeffs(Wi, W, "bicubic")
        img = _pass(img, b, k, 1)
    if Hi != H:
        b, k = ops.clip_resize_coeffs(Hi, H, "bicubic")
        img = _pass(img, b, k, 0)
    return img


@pytest.mark.parametrize("src,dst", [((576, 320), (1024, 576)), ((64, 40), (100, 70)), ((97, 53), (40, 31)),
                                     ((50, 37), (50, 81)), ((77, 30), (33, 30)), ((31, 29), (31, 29))])
def test_bicubic_coefficients_match_pillow(src, dst):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(sum(src) + sum(dst))
    img = rng.integers(0, 256, (src[1], src[0], 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(img).resize(dst))                      # default filter: BICUBIC
    assert np.array_equal(emulate_bicubic(img, *dst), want)


def test_bilinear_coefficients_unchanged():
    b0, k0 = ops.clip_resize_coeffs(333)
    b1, k1 = ops.clip_resize_coeffs(333, 224, "bilinear")
    assert np.array_equal(b0, b1) and np.array_equal(k0, k1) and k0.shape[1] == 5


def test_unit_lut_is_diffusers_map():
    lut = ops.u8_to_unit_lut()
    u = torch.arange(256, dtype=torch.uint8)
    want = (2.0 * (u.float() / 255.0) - 1.0).half()
    assert lut.dtype == torch.float16 and torch.equal(lut, want)
    assert lut[0] == -1 and lut[255] == 1


def test_cli_without_init_video_keeps_config():
    a = build_arg_parser().parse_args(["--num_frames", "8", "--steps", "3"])
    cfg = config_from_args(a)
    d = DiffuserConfig(num_frames=8, steps=3)
    assert cfg.init_video is None and cfg.strength == 0.6 and cfg.posterior == "sample"
    for k in vars(d):
        if k not in ("device", "noise_device"):
            assert getattr(cfg, k) == getattr(d, k), k
    a2 = build_arg_parser().parse_args(["--init_video", "x.npy", "--strength", "0.5", "--posterior", "mode"])
    c2 = config_from_args(a2)
    assert (c2.init_video, c2.strength, c2.posterior) == ("x.npy", 0.5, "mode")


def test_encode_shape_rules():
    vae = AutoencoderKL(TINY).load_diffusers_encoder_state_dict(synthetic_vae_encoder_state_dict(TINY),
                                                                            device="cpu")
    with pytest.raises(VdxError, match="multiples of 8"):
        vae._check_encode_size(60, 64)
    with pytest.raises(VdxError, match="% 64"):
        vae._check_encode_size(64, 72)
    vae._check_encode_size(64, 64)
    with pytest.raises(VdxError, match="no encoder weights"):
        AutoencoderKL(TINY)._check_encode_size(64, 64)
