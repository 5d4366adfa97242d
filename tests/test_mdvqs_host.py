"""CPU suite: the host half of the MD-VQS score and authenticity gate (vdx/mdvqs.py, vdx/lpips.py;
InferNet/template/validator/scoring.py:13-67, :154-343) — properties of the fp32 restatement the GPU tests are measured
against (tests/lpips_ref.py), the gate's finishing math from integer counts, the recalled `lpips` key map, the pipeline's
new flags (off by default), and the refusal of CPU tensors on the product path."""
import numpy as np
import pytest
import torch

import vdx  # noqa: F401
from vdx._lib import VdxError

import lpips_ref as R


@pytest.fixture(scope="module")
def sd():
    return R.synthetic_state_dict(0)


def test_reference_distance_is_zero_for_equal_frames_and_symmetric(sd):
    pytest.importorskip("PIL.Image")
    fr = R.frames_like_video(2, 100, 150, seed=1)
    with torch.no_grad():
        taps = R.alex_taps(R.scaled_pixels(fr, sd), sd)
        fwd, per_tap = R.lpips_pairs_from_taps(taps, sd)
        bwd, _ = R.lpips_pairs_from_taps([t.flip(0) for t in taps], sd)
        same, _ = R.lpips_pairs_from_taps([t[[0, 0]] for t in taps], sd)
    assert [tuple(t.shape[1:]) for t in taps] == [(64, 55, 55), (192, 27, 27), (384, 13, 13), (256, 13, 13), (256, 13, 13)]
    assert float(same) == 0.0 and torch.equal(fwd, bwd)
    assert 0.05 < float(fwd) < 1.0 and float(per_tap.min()) > 0.01                 # non-degenerate: every tap contributes


def test_reference_all_zero_pixels_are_finite():
    a = torch.zeros(1, 8, 2, 2)
    b = torch.zeros(1, 8, 2, 2)
    b[0, :, 0, 0] = 1.0
    d = R.tap_distance(a, b, torch.ones(8))
    assert torch.isfinite(d).all() and abs(float(d) - 0.25) < 1e-6                 # one of four pixels differs by a unit vector


def test_stem_lut_is_the_reference_transform(sd):
    from vdx.lpips import stem_lut
    lut = stem_lut(sd["scaling_layer.shift"], sd["scaling_layer.scale"])
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 256, 1, 1).expand(1, 256, 1, 3).contiguous().numpy()
    want = R.scaled_pixels_u8(u8, sd)[0, :, :, 0].half()                           # (3, 256)
    assert lut.shape == (3, 256) and lut.dtype == torch.float16 and torch.equal(lut, want)


def test_authenticity_finishing_math_from_integer_counts():
    """`authenticity_from_counts` on exact integers equals the restatement of scoring.py:13-67 on the frames, bit for bit."""
    from vdx.mdvqs import authenticity_from_counts
    fr = R.frames_like_video(4, 40, 56, seed=2)
    hist = np.stack([R.grey_hist(f).reshape(256).astype(np.uint32) for f in fr])
    diff = np.array([np.abs(fr[i + 1].astype(np.int64) - fr[i].astype(np.int64)).sum() for i in range(3)], np.uint64)
    ok, st = authenticity_from_counts(hist, diff, 40 * 56 * 3)
    want_ok, ent, dif = R.authenticity(fr)
    assert ok is True and want_ok is True
    assert st == {"entropy_mean": float(np.mean(ent)), "entropy_std": float(np.std(ent)), "diff_mean": float(np.mean(dif)),
                  "diff_std": float(np.std(dif))}
    # each threshold on its own: repeated frames (no difference), a constant image (no entropy), a single frame (no pairs)
    assert authenticity_from_counts(hist[[0, 0, 0]], np.zeros(2, np.uint64), 40 * 56 * 3)[0] is False
    flat = np.zeros((3, 256), np.uint32)
    flat[:, 128] = 40 * 56
    assert authenticity_from_counts(flat, diff[:2], 40 * 56 * 3)[0] is False
    ok1, st1 = authenticity_from_counts(hist[:1], diff[:0], 40 * 56 * 3)
    assert ok1 is False and st1["diff_mean"] is None and st1["entropy_mean"] == float(np.mean(ent[:1]))
    assert authenticity_from_counts(hist[:0], diff[:0], 1)[0] is False
    # the same entropy with equal differences: diff_std < 0.01 alone rejects
    assert authenticity_from_counts(hist[:3], np.array([900, 900], np.uint64), 40 * 56 * 3)[0] is False


def test_from_local_reads_the_recalled_lpips_layout(tmp_path, sd):
    from vdx.lpips import LPIPSAlex, expected_shapes
    assert set(sd) == set(expected_shapes()) and len(sd) == 17
    path = str(tmp_path / "alex.pth")
    torch.save(R.lpips_state_dict_file_layout(sd), path)                            # + the `lins.N` aliases of a full state_dict()
    a, b = LPIPSAlex.from_local(path, device="cpu"), LPIPSAlex.synthetic(seed=0, device="cpu")
    assert a.synthetic_weights is False and b.synthetic_weights is True
    for x, y in zip(a.w + a.b + a.lin + [a.lut], b.w + b.b + b.lin + [b.lut]):
        assert x.dtype == y.dtype and torch.equal(x, y)
    assert [tuple(w.shape) for w in b.w] == [(64, 384), (192, 1600), (384, 1728), (256, 3456), (256, 2304)]
    assert all(v.dtype == torch.float32 for v in b.lin) and not b.w[0][:, 363:].any()
    with pytest.raises(VdxError, match="unexpected key"):
        LPIPSAlex().load_lpips_state_dict({**sd, "net.slice1.1.weight": torch.zeros(1)}, device="cpu")
    for k in ("net.slice3.6.bias", "lin4.model.1.weight", "scaling_layer.scale"):
        with pytest.raises(VdxError, match="missing key"):
            LPIPSAlex().load_lpips_state_dict({q: v for q, v in sd.items() if q != k}, device="cpu")
    with pytest.raises(VdxError):
        LPIPSAlex().load_lpips_state_dict({**sd, "lin0.model.1.weight": -sd["lin0.model.1.weight"]}, device="cpu")
    with pytest.raises(VdxError):
        LPIPSAlex.from_local(str(tmp_path / "nope.pth"))


def test_conv_weights_are_laid_out_for_the_gathers(sd):
    """conv1 / conv2 weights follow the stem's and im2col's column order, K = (ky*k + kx)*Cin + c."""
    from vdx.lpips import LPIPSAlex
    m = LPIPSAlex.synthetic(seed=0, device="cpu")
    w1 = sd["net.slice1.0.weight"].half()
    assert m.w[0][5, (3 * 11 + 7) * 3 + 2] == w1[5, 2, 3, 7]
    w2 = sd["net.slice2.3.weight"].half()
    assert m.w[1][17, (4 * 5 + 1) * 64 + 33] == w2[17, 33, 4, 1]


def test_mdvqs_flags_default_off_and_old_argv_parses_the_same():
    from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args
    old = ["--num_frames", "24", "--steps", "5", "--mode", "chunk", "--chunk_size", "8", "--prompt", "a cat"]
    a = build_arg_parser().parse_args(old)
    assert a.mdvqs_json is None and a.lpips_model is None and a.clip_json is None
    assert config_from_args(a) == DiffuserConfig(num_frames=24, steps=5, mode="chunk", chunk_size=8, prompt="a cat")
    b = build_arg_parser().parse_args(old + ["--mdvqs_json", "m.json", "--lpips_model", "/w/alex.pth", "--clip_model", "/m"])
    assert (b.mdvqs_json, b.lpips_model, b.clip_model) == ("m.json", "/w/alex.pth", "/m")
    assert config_from_args(b) == config_from_args(a)


def test_product_path_refuses_cpu_tensors():
    """No CPU fallback: models held on the CPU raise at the first kernel, as the rest of the package does."""
    from vdx.lpips import LPIPSAlex
    from vdx.mdvqs import MDVQS, verify_video_authenticity
    fr = R.frames_like_video(2, 32, 48, seed=3)
    lp = LPIPSAlex.synthetic(seed=0, device="cpu")
    with pytest.raises(VdxError):
        lp(fr)
    with pytest.raises(VdxError):
        lp.features(torch.from_numpy(fr))
    with pytest.raises(VdxError):
        MDVQS(lpips=lp).compute_video_quality(fr)
    with pytest.raises(VdxError):
        verify_video_authenticity(torch.from_numpy(fr), device="cpu")
    with pytest.raises(VdxError):
        MDVQS().compute_video_quality(fr)                                           # no model at all
    with pytest.raises(VdxError):
        MDVQS(lpips=lp).compute_prompt_fidelity(fr, "a cat")


def test_video_quality_and_flow_edge_cases_without_a_gpu():
    """scoring.py:295-297, :336-337: fewer than two frames -> 0.0 before any kernel; TC is the mean |flow| over the pairs."""
    from vdx.lpips import LPIPSAlex
    from vdx.mdvqs import MDVQS
    m = MDVQS(lpips=LPIPSAlex.synthetic(seed=0, device="cpu"))
    fr = R.frames_like_video(3, 32, 48, seed=4)
    assert m.compute_video_quality(fr[:1]) [0] == 0.0 and m.compute_video_quality(fr[:0])[1].numel() == 0
    assert m.compute_temporal_consistency(fr[:1]) == 0.0 and m.compute_temporal_consistency([]) == 0.0
    tc = m.compute_temporal_consistency(fr)
    assert tc > 0.0 and tc == m.compute_temporal_consistency(torch.from_numpy(fr))
    with pytest.raises(VdxError):
        m.compute_temporal_consistency(fr.astype(np.float32))
