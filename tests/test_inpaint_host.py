"""-m "not gpu": masked video-to-video's host side (vdx/inpaint.py): the mask intake, the `--keep_frames` specs, every refusal of
`check_mask` with its message, the two pixel -> latent rules of the restatement, and the parser's defaults."""
import numpy as np
import pytest
import torch

import inpaint_ref as R
import vdx  # noqa: F401
from vdx import inpaint
from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args, run_job

T, H, W = 5, 16, 24


def test_load_mask_takes_the_three_shapes_and_nothing_else(tmp_path):
    rng = np.random.default_rng(0)
    full = (rng.random((T, H, W)) < 0.5).astype(np.uint8) * 7                     # nonzero = regenerate, whatever the value
    plane = rng.random((H, W)) < 0.5                                              # bool
    per_frame = np.array([1, 0, 0, 255, 0], dtype=np.uint8)
    for name, arr, want in (("full", full, full != 0), ("plane", plane, np.broadcast_to(plane, (T, H, W))),
                            ("frames", per_frame, np.broadcast_to((per_frame != 0)[:, None, None], (T, H, W)))):
        np.save(tmp_path / f"{name}.npy", arr)
        got = inpaint.load_mask(str(tmp_path / f"{name}.npy"), T, H, W)
        assert got.dtype == np.uint8 and got.shape == (T, H, W) and got.flags["C_CONTIGUOUS"] and got.max() <= 1
        assert np.array_equal(got, want.astype(np.uint8)), name
    for bad in (np.zeros((T, H, W + 8), np.uint8), np.zeros((H // 8, W // 8), np.uint8), np.zeros((T + 1,), np.uint8),
                np.zeros((T, H, W, 1), np.uint8)):
        np.save(tmp_path / "bad.npy", bad)
        with pytest.raises(ValueError, match="shape"):
            inpaint.load_mask(str(tmp_path / "bad.npy"), T, H, W)
    np.save(tmp_path / "float.npy", np.zeros((T, H, W), np.float32))
    with pytest.raises(ValueError, match="uint8 or bool"):
        inpaint.load_mask(str(tmp_path / "float.npy"), T, H, W)


def test_keep_frames_specs():
    k = inpaint.keep_frames_mask
    assert k("0:3", 8).tolist() == [0, 0, 0, 1, 1, 1, 1, 1]
    assert k("0:2,6:8", 8).tolist() == [0, 0, 1, 1, 1, 1, 0, 0]
    assert k("3", 8).tolist() == [1, 1, 1, 0, 1, 1, 1, 1] and k("-1", 8).tolist() == [1] * 7 + [0]
    assert k(":2", 8).tolist() == [0, 0] + [1] * 6 and k("6:", 8).tolist() == [1] * 6 + [0, 0]
    assert k("::2", 8).tolist() == [0, 1] * 4 and k(" 1 , 4:6 ", 8).tolist() == [1, 0, 1, 1, 0, 0, 1, 1]
    assert k("-2:", 8).tolist() == [1] * 6 + [0, 0] and k("0:8", 8).tolist() == [0] * 8 and k("4:4", 8).tolist() == [1] * 8
    assert k("0:3", 8).dtype == np.uint8
    for bad in ("8", "-9", "0:9", "-9:2", "a", "1:b", "1:2:3:4", "", "1,,2", "::0", "1.5", None):
        with pytest.raises(ValueError):
            k(bad, 8)


def test_check_mask_refusals_and_messages(tmp_path):
    clip = str(tmp_path / "clip.npy")
    base = dict(num_frames=T, height=H, width=W, init_video=clip)
    assert inpaint.check_mask(DiffuserConfig()) is None and inpaint.check_mask(DiffuserConfig(), "halo") is None
    px = inpaint.check_mask(DiffuserConfig(keep_frames="0:2", **base))
    assert px.shape == (T, H, W) and px[:2].max() == 0 and px[2:].min() == 1
    with pytest.raises(ValueError, match="init_video"):
        inpaint.check_mask(DiffuserConfig(keep_frames="0:2", num_frames=T, height=H, width=W))
    np.save(tmp_path / "m.npy", np.ones((T, H, W), np.uint8))
    with pytest.raises(ValueError, match="exclude each other"):
        inpaint.check_mask(DiffuserConfig(keep_frames="0:2", mask=str(tmp_path / "m.npy"), **base))
    with pytest.raises(ValueError, match="allgather"):
        inpaint.check_mask(DiffuserConfig(keep_frames="0:2", **base), "halo")
    with pytest.raises(ValueError, match="keeps everything"):
        inpaint.check_mask(DiffuserConfig(keep_frames=":", **base))
    np.save(tmp_path / "z.npy", np.zeros((H, W), np.uint8))
    with pytest.raises(ValueError, match="keeps everything"):
        inpaint.check_mask(DiffuserConfig(mask=str(tmp_path / "z.npy"), **base))
    lone = np.zeros((H, W), np.uint8)
    lone[7, 7] = 1                                                 # no pixel (8y, 8x) is set: "nearest" regenerates nothing
    np.save(tmp_path / "lone.npy", lone)
    with pytest.raises(ValueError, match="keeps everything"):
        inpaint.check_mask(DiffuserConfig(mask=str(tmp_path / "lone.npy"), **base))
    assert inpaint.check_mask(DiffuserConfig(mask=str(tmp_path / "lone.npy"), mask_rule="any", **base)).sum() == T
    with pytest.raises(ValueError, match="mask_rule"):
        inpaint.check_mask(DiffuserConfig(keep_frames="0:2", mask_rule="bilinear", **base))
    with pytest.raises(ValueError, match="mask_rule"):
        inpaint.check_mask(DiffuserConfig(mask_rule="bilinear"))
    with pytest.raises(ValueError, match="shape"):
        inpaint.check_mask(DiffuserConfig(mask=str(tmp_path / "m.npy"), num_frames=T, height=H, width=W + 8, init_video=clip))
    # an all-ones mask is allowed: plain video-to-video
    assert inpaint.check_mask(DiffuserConfig(mask=str(tmp_path / "m.npy"), **base)).min() == 1
    # the job refuses before any model is loaded (needs no GPU), and FreeInit stays refused with --init_video
    with pytest.raises(ValueError, match="init_video"):
        run_job(DiffuserConfig(keep_frames="0:2"), out_video=None)
    with pytest.raises(ValueError, match="allgather"):
        run_job(DiffuserConfig(keep_frames="0:2", **base), exchange="halo", out_video=None)
    with pytest.raises(ValueError, match="keeps everything"):
        run_job(DiffuserConfig(keep_frames=":", **base), out_video=None)
    with pytest.raises(ValueError, match="init_video"):
        run_job(DiffuserConfig(keep_frames="0:2", free_init_iters=2, **base), out_video=None)


def test_latent_mask_rules():
    px = torch.zeros(2, H, W, dtype=torch.uint8)
    px[0, 7, 7] = 1                                                # the last pixel of cell (0, 0): dropped by nearest, kept by any
    px[1, 8, 16] = 200                                             # pixel (8y, 8x) of cell (1, 2): both rules
    near, anyr = R.latent_mask_ref(px, "nearest"), R.latent_mask_ref(px, "any")
    assert near.shape == anyr.shape == (2, H // 8, W // 8) and near.dtype == anyr.dtype == torch.uint8
    assert near[0].sum() == 0 and anyr[0, 0, 0] == 1 and anyr[0].sum() == 1
    assert near[1, 1, 2] == 1 and near[1].sum() == 1 and torch.equal(near[1], anyr[1])
    # "nearest" is what F.interpolate takes at the exact factor 8
    rnd = (torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)) < 0.3).to(torch.uint8)
    want = torch.nn.functional.interpolate(rnd[None].float(), size=(H // 8, W // 8), mode="nearest")[0].to(torch.uint8)
    assert torch.equal(R.latent_mask_ref(rnd, "nearest"), want)
    # the product's host copy (the refusals use it before a device is touched) agrees with the restatement
    for rule in ("nearest", "any"):
        assert np.array_equal(inpaint.latent_mask_host(rnd.numpy(), rule), R.latent_mask_ref(rnd, rule).numpy())
        assert np.array_equal(inpaint.latent_mask_host(px.numpy(), rule), R.latent_mask_ref(px, rule).numpy())
    rec = inpaint.mask_record(torch.tensor([[[0, 0]], [[0, 1]], [[1, 1]], [[0, 0]]], dtype=torch.uint8), "any", False)
    assert rec == {"rule": "any", "paste": False, "kept_fraction": 5 / 8, "kept_frames": 2}


def test_renoise_ref_is_a_select():
    g = torch.Generator().manual_seed(2)
    x0, base = (torch.randn(1, 2, 4, 2, 3, generator=g).half() for _ in range(2))
    z = torch.randn(1, 2, 2, 2, 3, generator=g).half()
    z[0, 0, 0, 0, 0], z[0, 1, 1, 1, 2] = float("nan"), -0.0
    m = (torch.rand(4, 2, 3, generator=g) < 0.5).to(torch.uint8)
    got = R.renoise_ref(z, x0, base, m, 0.75, 0.5, False, 1)
    known = (0.75 * x0 + 0.5 * base)[:, :, 1:3]                    # fp16 tensor ops: torch's own add_noise expression
    mm = m[1:3].bool()[None, None].expand_as(z)
    assert torch.equal(got.view(torch.int16)[mm], z.view(torch.int16)[mm])
    assert torch.equal(got.view(torch.int16)[~mm], known.view(torch.int16)[~mm])
    last = R.renoise_ref(z, x0, base, m, 0.0, 0.0, True, 2)
    mm = m[2:4].bool()[None, None].expand_as(z)
    assert torch.equal(last.view(torch.int16)[~mm], x0[:, :, 2:4].view(torch.int16)[~mm])


def test_parser_defaults_leave_the_config_as_it_was():
    p = build_arg_parser()
    cfg = config_from_args(p.parse_args([]))
    assert cfg == DiffuserConfig()
    assert (cfg.mask, cfg.keep_frames, cfg.mask_rule, cfg.mask_paste) == (None, None, "nearest", True)
    a = p.parse_args(["--keep_frames", "0:8", "--mask_rule", "any", "--mask_paste", "off"])
    cfg = config_from_args(a)
    assert (cfg.mask, cfg.keep_frames, cfg.mask_rule, cfg.mask_paste) == (None, "0:8", "any", False)
    assert config_from_args(p.parse_args(["--mask", "m.npy"])).mask == "m.npy"
    with pytest.raises(SystemExit):
        p.parse_args(["--mask_rule", "bilinear"])
