"""-m gpu: the validator's MD-VQS score and authenticity gate (vdx/mdvqs.py, vdx/lpips.py, csrc/mdvqs.hip;
InferNet/template/validator/scoring.py:13-67, :154-343) on libvdx_hip.so against tests/lpips_ref.py: Pillow's resize and an
fp32 torch-CPU restatement of LPIPS-AlexNet, and a numpy restatement of the gate.  The network's shapes are fixed by the
224x224 resize, so small means few frames (F = 3: two pairs) from small sources.

The bounds marked "Measured on MI355X" are twice the measured value rounded up to two significant digits (the margin the
project uses for box-to-box and seed variation); everything called bit-equal has no tolerance."""
import csv
import json

import numpy as np
import pytest
import torch

import lpips_ref as R

pytestmark = pytest.mark.gpu
pytest.importorskip("PIL.Image")

SOURCES = [(100, 150, 1), (320, 576, 2)]            # (H, W, seed) of the F = 3 source clips
TAP_SIZES = (55, 27, 13, 13, 13)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def hard_state_dict(sd):
    """The hard variant: the biases of conv3..5 lowered, one layer after the other, until 40 % of the pixels of the 100x150
    clip have no positive channel at that tap (all-zero feature vectors: the 0 / (0 + 1e-10) path), and `lin` log-uniform
    over [1e-3, 1]."""
    hd = {k: v.clone() for k, v in sd.items()}
    g = torch.Generator().manual_seed(5)
    for i in range(5):
        hd[f"lin{i}.model.1.weight"] = 10 ** (-3 * torch.rand(hd[f"lin{i}.model.1.weight"].shape, generator=g))
    x = R.scaled_pixels(R.frames_like_video(3, 100, 150, 1), hd)
    with torch.no_grad():
        for i in (2, 3, 4):
            taps = R.alex_taps(x, hd)                                               # taps before i are final
            src = torch.nn.functional.max_pool2d(taps[1], 3, 2) if i == 2 else taps[i - 1]
            key = R.conv_key(i) + ".bias"
            raw = torch.nn.functional.conv2d(src, hd[R.conv_key(i) + ".weight"], hd[key], padding=1)
            hd[key] = hd[key] - torch.quantile(raw.amax(1).flatten(), 0.4)
    return hd


@pytest.fixture(scope="module")
def sd():
    return R.synthetic_state_dict(0)


@pytest.fixture(scope="module")
def hard_sd(sd):
    return hard_state_dict(sd)


@pytest.fixture(scope="module")
def clips():
    return {(H, W): R.frames_like_video(3, H, W, seed) for H, W, seed in SOURCES}


@pytest.fixture(scope="module")
def reference(sd, hard_sd, clips):
    """{(variant, H, W): (taps NCHW fp32, per-pair distances, per-tap contributions)}: computed once, never changed."""
    out = {}
    with torch.no_grad():
        for name, w in (("synthetic", sd), ("hard", hard_sd)):
            for key, fr in clips.items():
                taps = R.alex_taps(R.scaled_pixels(fr, w), w)
                out[(name,) + key] = (taps,) + R.lpips_pairs_from_taps(taps, w)
    return out


@pytest.fixture(scope="module")
def models(gpu, sd, hard_sd):
    import vdx  # noqa: F401
    from vdx.lpips import LPIPSAlex
    return {"synthetic": LPIPSAlex.synthetic(seed=0, device=gpu), "hard": LPIPSAlex().load_lpips_state_dict(hard_sd, device=gpu)}


# ---- stem -----------------------------------------------------------------------------------------------------------
def _want_stem(u8_224, sd):
    px = R.scaled_pixels_u8(u8_224, sd).half().float()
    cols = torch.nn.functional.unfold(px, 11, padding=2, stride=4)                   # (F, 3*121, 3025), K = c*121 + tap
    F = px.shape[0]
    cols = cols.view(F, 3, 121, 3025).permute(0, 3, 2, 1).reshape(F * 3025, 363)    # K = tap*3 + c
    return torch.nn.functional.pad(cols, (0, 21)).half()


@pytest.mark.parametrize("pitched", [False, True])
def test_stem_rows_are_the_unfolded_reference_pixels(gpu, sd, models, pitched):
    """Resize (Pillow's bits) + both affine maps in fp32 + one rounding to fp16 + the k11 s4 p2 gather: bit-equal to `unfold`
    of the reference pixels rounded to fp16; padding columns and out-of-image taps exactly 0.  `pitched`: a cropped view."""
    from vdx import ops
    if pitched:
        big = torch.from_numpy(R.frames_like_video(2, 120, 170, seed=9)).to(gpu)
        fr = big[:, 7:107, 11:161]
        assert not fr.is_contiguous()
    else:
        fr = torch.from_numpy(R.frames_like_video(2, 100, 150, seed=8)).to(gpu)
    u8 = ops.resize_u8(fr, 224, 224, "bilinear")
    assert torch.equal(u8.cpu(), torch.from_numpy(R.pil_resize(fr.cpu().numpy())))
    rows = ops.lpips_stem(u8, models["synthetic"].lut).cpu()
    want = _want_stem(u8.cpu().numpy(), sd)
    assert rows.shape == (2 * 3025, 384) and torch.equal(rows, want)
    assert not rows[:, 363:].any()
    corner = rows[0].view(-1)[:363].view(11, 11, 3)                                  # output pixel (0, 0): taps with ky < 2 or kx < 2 lie outside
    assert not corner[:2].any() and not corner[:, :2].any() and corner[2:, 2:].ne(0).any()


# ---- relu + maxpool, im2col ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C", [(55, 64), (27, 192)])
def test_relu_maxpool_is_torch_bit_for_bit(gpu, S, C):
    """In-place ReLU and MaxPool2d(3, 2) of the ReLU'd rows, including the last window (55 -> 27, 27 -> 13) and the corners."""
    from vdx import ops
    n = 2
    x = torch.randn(n * S * S, C, generator=torch.Generator().manual_seed(S)).half()
    d = x.to(gpu)
    pooled = ops.relu_maxpool(d, n_img=n, H=S, W=S)
    nchw = R.rows_to_nchw(x, n, S)
    want_relu = torch.relu(nchw)
    want_pool = torch.nn.functional.max_pool2d(want_relu, 3, 2)
    So = (S - 3) // 2 + 1
    assert want_pool.shape[-1] == So and pooled.shape == (n * So * So, C)
    assert torch.equal(R.rows_to_nchw(d.cpu(), n, S), want_relu)
    got = R.rows_to_nchw(pooled.cpu(), n, So)
    assert torch.equal(got, want_pool)
    assert torch.equal(got[:, :, -1, -1], want_relu[:, :, 2 * So - 2:2 * So + 1, 2 * So - 2:2 * So + 1].amax((2, 3)))


@pytest.mark.parametrize("k,pad,S,C", [(5, 2, 27, 64), (3, 1, 13, 192), (5, 2, 6, 64)])
def test_im2col_is_unfold_bit_for_bit(gpu, k, pad, S, C):
    from vdx import ops
    n = 2
    x = torch.randn(n * S * S, C, generator=torch.Generator().manual_seed(k * S)).half()
    got = ops.im2col(x.to(gpu), n_img=n, H=S, W=S, k=k, pad=pad).cpu()
    cols = torch.nn.functional.unfold(R.rows_to_nchw(x, n, S), k, padding=pad)      # (n, C*k*k, S*S), K = c*k*k + tap
    want = cols.view(n, C, k * k, S * S).permute(0, 3, 2, 1).reshape(n * S * S, k * k * C).half()
    assert torch.equal(got, want)
    first = got[0].view(k, k, C)                                                    # image corner: taps above / left are padding
    assert not first[:pad].any() and not first[:, :pad].any()
    assert torch.equal(first[pad, pad], x[0]) and torch.equal(got[-1].view(k, k, C)[pad, pad], x[-1])


def test_relu_over_every_fp16_pattern(gpu):
    """All 65 536 bit patterns: == torch.relu on the CPU, NaN where torch gives NaN; in place the same.  (The sign of zero
    is not asserted.)"""
    from vdx import ops
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    want = torch.relu(x.float()).half()
    d = x.to(gpu)
    got = ops.relu(d).cpu()
    nan = torch.isnan(want)
    assert nan.sum() == 2046 and torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan], want[~nan])
    again = ops.relu(d, out=d).cpu()
    assert torch.equal(torch.isnan(again), nan) and torch.equal(again[~nan], want[~nan])
    odd = ops.relu(d[:65529]).cpu()                                                  # a length that is no multiple of 8: the scalar tail
    assert torch.equal(odd[~nan[:65529]], want[:65529][~nan[:65529]])


# ---- the distance kernel ------------------------------------------------------------------------------------------
DIST_REL = 4.0e-7      # see test_distance_kernel_matches_the_fp64_formula


def _distance_features(F, HW, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(F, HW, C, generator=g)).half()
    x[0, :7] = 0                                     # pixels all zero in the first frame of a pair only
    x[1, 5:12] = 0                                   # ... in both frames (5, 6), and in the second only
    x[1, 20:30] *= 60000 / x[1, 20:30].max()         # features near the fp16 maximum
    x[2, 25] = 65504.0
    lin = torch.rand(C, generator=g)
    return x, lin


@pytest.mark.parametrize("HW,C", [(3025, 64), (729, 192), (169, 384), (169, 256)])
def test_distance_kernel_matches_the_fp64_formula(gpu, HW, C):
    """The kernel on given fp16 features against the formula in fp64 on the same features: all-zero pixels in one or both
    frames of a pair come out finite and equal to the reference, as do features at the fp16 maximum.  Measured on MI355X:
    worst relative error 1.96e-7 (HW 3025, C 64), 9.82e-8, 9.01e-8, 3.87e-8
    over the four tap shapes."""
    from vdx import ops
    F = 4
    x, lin = _distance_features(F, HW, C, seed=HW + C)
    got = ops.lpips_distance(x.view(F * HW, C).to(gpu), lin.to(gpu), F=F, HW=HW).cpu()
    nchw = x.double().permute(0, 2, 1).reshape(F, C, HW, 1)
    want = R.tap_distance(nchw[:-1], nchw[1:], lin, dtype=torch.float64)
    err = float(((got.double() - want).abs() / want).max())
    print(f"distance kernel HW={HW} C={C}: {got.tolist()} vs {want.tolist()}, worst relative error {err:.2e}")
    assert torch.isfinite(got).all() and err <= DIST_REL


def test_distance_kernel_is_deterministic_accumulates_and_is_zero_for_equal_frames(gpu):
    from vdx import ops
    F, HW, C = 3, 729, 192
    x, lin = _distance_features(F, HW, C, seed=3)
    d, l = x.view(F * HW, C).to(gpu), lin.to(gpu)
    a, b = ops.lpips_distance(d, l, F=F, HW=HW), ops.lpips_distance(d, l, F=F, HW=HW)
    assert torch.equal(a, b)
    twice = ops.lpips_distance(d, l, F=F, HW=HW, out=a.clone())
    assert torch.equal(twice, a + a)
    same = x[:1].expand(3, HW, C).reshape(3 * HW, C).contiguous().to(gpu)
    assert torch.equal(ops.lpips_distance(same, l, F=3, HW=HW).cpu(), torch.zeros(2))


# ---- taps and end to end --------------------------------------------------------------------------------------------
TAP_REL_L2 = {"synthetic": 1.4e-3, "hard": 3.7e-3}     # see test_taps_match_the_fp32_reference
PAIR_REL = {"synthetic": 9.6e-5, "hard": 6.5e-4}       # see test_lpips_end_to_end


@pytest.mark.parametrize("variant", ["synthetic", "hard"])
@pytest.mark.parametrize("H,W", [s[:2] for s in SOURCES])
def test_taps_match_the_fp32_reference(models, reference, clips, variant, H, W):
    """Each of the five ReLU taps against the fp32 CPU network, rel-L2.  Measured on MI355X, taps 1..5: synthetic
    3.50e-4 4.77e-4 5.09e-4 5.62e-4 6.51e-4 (100x150), 3.67e-4 4.90e-4 5.27e-4 5.69e-4 6.57e-4 (320x576); hard
    3.50e-4 4.77e-4 1.58e-3 1.82e-3 1.84e-3 (100x150), 3.67e-4 4.90e-4 1.29e-3 1.46e-3 1.60e-3 (320x576).  The hard variant's
    taps 3-5 keep only the upper tail of each pre-activation (bias lowered to the 40 % quantile of the per-pixel maximum): the
    fp16 rounding of the inputs is relative to the whole sum, the surviving value is what exceeds the cut, so its relative
    error grows; the distances these taps give agree to 3.2e-4 (test_lpips_end_to_end)."""
    taps = models[variant].features(clips[(H, W)])
    want = reference[(variant, H, W)][0]
    errs = [rel_l2(R.rows_to_nchw(t.cpu(), 3, s), w) for t, s, w in zip(taps, TAP_SIZES, want)]
    print(f"{variant} {H}x{W}: tap rel-L2 " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= TAP_REL_L2[variant]


@pytest.mark.parametrize("variant", ["synthetic", "hard"])
def test_lpips_end_to_end(models, reference, clips, variant):
    """Per-pair LPIPS and vq against the fp32 reference, relative error; `hard`: conv3..5 biases lowered until 40 % of the
    pixels are all-zero feature vectors at taps 3-5 and lin log-uniform over [1e-3, 1].  Measured on MI355X: worst per-pair
    relative error 4.80e-5 (synthetic: 4.80e-5 at 100x150, 9.77e-6 at 320x576), 3.22e-4 (hard: 3.22e-4, 3.19e-5); the
    reference's per-pair distances are 0.19 .. 0.46 (synthetic), 0.75 .. 1.33 (hard)."""
    from vdx.mdvqs import MDVQS
    worst = 0.0
    for (H, W), fr in clips.items():
        taps, want, per_tap = reference[(variant, H, W)]
        if variant == "hard":
            share = [float((t.sum(1) == 0).float().mean()) for t in taps[2:]]
            assert (H, W) != (100, 150) or min(share) >= 0.3, share
        assert float(per_tap.min()) > 0.01                                          # every tap contributes: not degenerate
        vq, per = MDVQS(lpips=models[variant]).compute_video_quality(fr)
        err = float(((per.double() - want.double()).abs() / want.double()).max())
        want_vq = max(0.0, 1.0 - float(want.double().mean()))
        print(f"{variant} {H}x{W}: per-pair {per.tolist()} vs {want.tolist()} (worst rel {err:.2e}); vq {vq:.6f} vs {want_vq:.6f}")
        assert per.shape == (2,) and per.dtype == torch.float32
        assert abs(vq - want_vq) <= PAIR_REL[variant] * float(want.double().mean())
        worst = max(worst, err)
    assert worst <= PAIR_REL[variant]


def test_lpips_is_deterministic_and_takes_device_frames(models, clips, gpu):
    fr = clips[(100, 150)]
    a = models["synthetic"](fr)
    b = models["synthetic"](torch.from_numpy(fr).to(gpu))
    assert torch.equal(a, b)
    assert models["synthetic"](fr[:1]).numel() == 0
    same = models["synthetic"](np.stack([fr[0], fr[0]]))
    assert torch.equal(same, torch.zeros(1))


# ---- the authenticity gate ----------------------------------------------------------------------------------------------
def _want_counts(fr):
    hist = np.stack([R.grey_hist(f).reshape(256) for f in fr]).astype(np.int64)
    diff = np.array([np.abs(fr[i + 1].astype(np.int64) - fr[i].astype(np.int64)).sum() for i in range(len(fr) - 1)], np.int64)
    return hist, diff


@pytest.mark.parametrize("case", ["100x150", "576x1024", "pitched", "one row"])
def test_frame_stats_are_numpy_integers(gpu, case):
    from vdx import ops
    if case == "pitched":
        big = torch.from_numpy(R.frames_like_video(3, 120, 170, seed=4)).to(gpu)
        d = big[:, 3:113, 9:160]
        fr = d.cpu().numpy()
    else:
        F, H, W = {"100x150": (3, 100, 150), "576x1024": (2, 576, 1024), "one row": (2, 1, 37)}[case]
        fr = R.frames_like_video(F, H, W, seed=H)
        d = torch.from_numpy(fr).to(gpu)
    hist, diff = ops.frame_stats(d)
    want_h, want_d = _want_counts(fr)
    assert np.array_equal(hist.cpu().numpy().astype(np.int64), want_h)
    assert np.array_equal(diff.cpu().numpy(), want_d)
    assert int(hist.sum()) == fr.shape[0] * fr.shape[1] * fr.shape[2]


def test_authenticity_matches_the_restatement_bit_for_bit(gpu):
    from vdx.mdvqs import verify_video_authenticity
    for H, W, seed in [(100, 150, 1), (320, 576, 2)]:
        fr = R.frames_like_video(3, H, W, seed)
        ok, st = verify_video_authenticity(torch.from_numpy(fr).to(gpu))
        want_ok, ent, dif = R.authenticity(fr)
        assert ok is True and want_ok is True
        assert st == {"entropy_mean": float(np.mean(ent)), "entropy_std": float(np.std(ent)),
                      "diff_mean": float(np.mean(dif)), "diff_std": float(np.std(dif))}


def test_authenticity_rejects_repeated_constant_and_single_frames(gpu):
    from vdx.mdvqs import verify_video_authenticity
    fr = R.frames_like_video(3, 64, 96, seed=6)
    repeated = np.stack([fr[0]] * 3)
    constant = np.full((3, 64, 96, 3), 128, np.uint8)
    for clip in (repeated, constant, fr[:1]):
        ok, st = verify_video_authenticity(clip, device=gpu)
        want_ok, ent, dif = R.authenticity(clip)
        assert ok is False and want_ok is False
        assert st["entropy_mean"] == float(np.mean(ent)) and st["entropy_std"] == float(np.std(ent))
        assert st["diff_mean"] == (float(np.mean(dif)) if dif else None)
    assert verify_video_authenticity(fr[:0], device=gpu)[0] is False
    assert verify_video_authenticity(fr, device=gpu)[0] is True


# ---- MD-VQS ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mdvqs(gpu, models):
    from vdx.clip_score import CLIPScorer
    from vdx.mdvqs import MDVQS
    pytest.importorskip("transformers")
    return MDVQS(CLIPScorer.synthetic(seed=0, device=gpu), models["synthetic"])


def test_md_vqs_is_the_weighted_sum_of_its_parts(mdvqs, gpu):
    """total == alpha pf + beta vq + gamma tc of the parts computed on their own; pf == CLIPScorer.score bit for bit.  TC runs
    on 64x96 frames so the CPU flow stays short."""
    from vdx.compat.diffusers_shim import HashTokenizer
    fr = R.frames_like_video(3, 64, 96, seed=7)
    tok = HashTokenizer()
    pf, vq, tc, total = mdvqs.compute_md_vqs(fr, "a rocket in space, 4k", tokenizer=tok)
    assert pf == mdvqs.clip.score(fr, "a rocket in space, 4k", tokenizer=tok)[0]
    assert pf == mdvqs.compute_prompt_fidelity(torch.from_numpy(fr).to(gpu), "a rocket in space, 4k", tokenizer=tok)
    assert vq == mdvqs.compute_video_quality(fr)[0] and tc == mdvqs.compute_temporal_consistency(fr)
    assert total == 0.4 * pf + 0.3 * vq + 0.3 * tc == mdvqs.compute_quality_score(fr, "a rocket in space, 4k", tokenizer=tok)
    assert 0.0 < vq < 1.0 and tc > 0.0 and np.isfinite(total)
    assert vq == max(0.0, 1.0 - float(np.mean([float(d) for d in mdvqs.lpips(fr)])))


def test_md_vqs_edge_cases_zero_and_one_frame(mdvqs):
    """scoring.py:133-135, :295-297, :336-337: no frames -> every term 0.0; one frame -> PF alone."""
    from vdx.compat.diffusers_shim import HashTokenizer
    fr = R.frames_like_video(1, 64, 96, seed=8)
    assert mdvqs.compute_md_vqs(fr[:0], "x", tokenizer=HashTokenizer()) == (0.0, 0.0, 0.0, 0.0)
    pf, vq, tc, total = mdvqs.compute_md_vqs(fr, "x", tokenizer=HashTokenizer())
    assert vq == 0.0 and tc == 0.0 and pf != 0.0 and total == 0.4 * pf + 0.3 * 0.0 + 0.3 * 0.0
    v, per = mdvqs.compute_video_quality(fr)
    assert v == 0.0 and per.numel() == 0


# ---- pipeline -----------------------------------------------------------------------------------------------------
BASE = ["--model_id", "synthetic:tiny", "--num_frames", "8", "--steps", "2", "--height", "128", "--width", "256",
        "--chunk_size", "6", "--overlap", "2", "--mode", "chunk", "--out_video", "", "--noise_device", "cpu"]
KEYS = {"pf", "vq", "tc", "total", "weights", "lpips_per_pair", "authentic", "authenticity", "synthetic_weights", "n_frames"}


def test_pipeline_writes_mdvqs_json_and_keeps_the_csv_row(gpu, tmp_path):
    """`python -m vdx.pipeline ... --mdvqs_json` on tiny synthetic weights: the record has the documented keys, and the CSV
    row's columns that measure neither time nor memory equal those of the same run without the flag."""
    import vdx  # noqa: F401
    from vdx.pipeline import main
    out_csv, js = str(tmp_path / "r.csv"), str(tmp_path / "m.json")
    base = BASE + ["--out_csv", out_csv]
    assert main(base) == 0
    assert main(base + ["--mdvqs_json", js]) == 0
    rec = json.load(open(js))
    assert set(rec) == KEYS
    assert rec["weights"] == {"alpha": 0.4, "beta": 0.3, "gamma": 0.3} and rec["n_frames"] == 8
    assert len(rec["lpips_per_pair"]) == 7 and rec["synthetic_weights"] is True and isinstance(rec["authentic"], bool)
    assert set(rec["authenticity"]) == {"entropy_mean", "entropy_std", "diff_mean", "diff_std"}
    assert rec["total"] == 0.4 * rec["pf"] + 0.3 * rec["vq"] + 0.3 * rec["tc"]
    assert rec["vq"] == max(0.0, 1.0 - float(np.mean(rec["lpips_per_pair"])))
    rows = list(csv.DictReader(open(out_csv)))
    timed = {"timestamp", "latency_s", "throughput_fps", "net_gather_s", "net_reduce_s", "peak_vram_mb", "end_vram_mb"}
    assert len(rows) == 2 and rows[0].keys() == rows[1].keys()
    assert {k: v for k, v in rows[0].items() if k not in timed} == {k: v for k, v in rows[1].items() if k not in timed}


def test_pipeline_scores_md_vqs_after_the_row_is_written(gpu, tmp_path, monkeypatch):
    """--mdvqs_json scores after the row took its latency (the pattern of test_pipeline_latency_does_not_include_the_score,
    without the sleep: the order of the two events is what keeps the scorer out of `latency_s`)."""
    import vdx  # noqa: F401
    from vdx import metrics, pipeline
    events = []
    append = metrics.append_csv

    def appended(path, row):
        events.append("row")
        append(path, row)

    def record(frames, prompt, lpips_model, clip_model, tok, device):
        events.append("score")
        return {"n_frames": len(frames)}

    monkeypatch.setattr(metrics, "append_csv", appended)
    monkeypatch.setattr(pipeline, "mdvqs_record", record)
    js = tmp_path / "m.json"
    assert pipeline.main(BASE + ["--out_csv", str(tmp_path / "r.csv"), "--mdvqs_json", str(js)]) == 0
    assert events == ["row", "score"] and json.load(open(js)) == {"n_frames": 8}
