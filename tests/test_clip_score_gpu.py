"""-m gpu: the validator's CLIP quality score (vdx/clip_score.py; InferNet/template/validator/scoring.py:87-147) on
libvdx_hip.so against the REAL dependencies: Pillow for Resize((224, 224)) and `transformers.CLIPModel(CLIPConfig())`
(ViT-B/32 shapes, seeded weights) in fp32 on the CPU for the towers and the score."""
import csv

import pytest
import torch

from clip_stage_ref import frames_like_video, pil_resize, reference_pixels, unfold_patches

pytestmark = pytest.mark.gpu
transformers = pytest.importorskip("transformers")
Image = pytest.importorskip("PIL.Image")

SIZES = [(576, 1024), (320, 576), (72, 128), (100, 150), (224, 224)]


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def clip_model():
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        return transformers.CLIPModel(transformers.CLIPConfig()).eval()


@pytest.fixture(scope="module")
def scorer(gpu, clip_model):
    import vdx  # noqa: F401
    from vdx.clip_score import CLIPScorer
    return CLIPScorer.synthetic(seed=0, device=gpu)


def test_synthetic_scorer_is_the_seeded_clipmodel(scorer, clip_model):
    assert scorer.synthetic_weights
    w = clip_model.visual_projection.weight.detach()
    assert torch.equal(scorer.W["visual_projection"].cpu(), w.half())


@pytest.mark.parametrize("H,W", SIZES)
def test_resize_is_pillow_bit_for_bit(gpu, H, W):
    from vdx import ops
    F = 24 if (H, W) == (576, 1024) else 3
    fr = frames_like_video(F, H, W, seed=H + W)
    rows, u8 = ops.clip_preprocess(torch.from_numpy(fr).to(gpu), return_u8=True)
    assert torch.equal(u8.cpu(), torch.from_numpy(pil_resize(fr)))
    assert rows.shape == (F * 49, 3072)


def test_resize_reads_pitched_frames(gpu):
    """A crop of wider frames (row pitch > 3*W, frame pitch > rows): the same bits as the packed copy."""
    from vdx import ops
    big = torch.from_numpy(frames_like_video(2, 330, 600, seed=9)).to(gpu)
    view = big[:, 5:325, 10:586]
    _, u8 = ops.clip_preprocess(view, return_u8=True)
    assert torch.equal(u8.cpu(), torch.from_numpy(pil_resize(view.cpu().numpy())))


@pytest.mark.parametrize("H,W", [(576, 1024), (100, 150)])
def test_normalized_patch_rows_are_torch_cpu_bits(gpu, H, W):
    from vdx import ops
    fr = frames_like_video(4, H, W, seed=3)
    rows = ops.clip_preprocess(torch.from_numpy(fr).to(gpu))
    want = unfold_patches(reference_pixels(fr)).half()
    assert torch.equal(rows.cpu(), want)


def _image_errs(scorer, model, fr):
    got = scorer.image_features(fr).float().cpu()
    with torch.no_grad():
        want = model.get_image_features(pixel_values=reference_pixels(fr)).pooler_output
    per = [rel_l2(got[i], want[i]) for i in range(len(fr))]
    return rel_l2(got, want), max(per)


def test_image_features_match_clipmodel(scorer, clip_model):
    """get_image_features(...).pooler_output in fp32 on the CPU from the reference's pixels.  Measured on MI355X:
    rel-L2 1.14e-3 overall, 1.19e-3 worst frame."""
    fr = frames_like_video(8, 576, 1024, seed=11)
    tot, worst = _image_errs(scorer, clip_model, fr)
    print(f"image features rel-L2 {tot:.3e} (worst frame {worst:.3e})")
    assert tot <= 2.5e-3 and worst <= 2.5e-3


def test_image_features_match_clipmodel_peaked_attention(gpu, clip_model):
    """Position embeddings and q/k weights x4, so attention is far from uniform.  Measured: rel-L2 1.07e-3 overall,
    1.11e-3 worst frame."""
    import copy
    from vdx.clip_score import CLIPScorer, configs_from_dict
    m = copy.deepcopy(clip_model)
    with torch.no_grad():
        m.vision_model.embeddings.position_embedding.weight.mul_(4)
        for layer in m.vision_model.encoder.layers:
            layer.self_attn.q_proj.weight.mul_(4)
            layer.self_attn.k_proj.weight.mul_(4)
    s = CLIPScorer(*configs_from_dict(m.config.to_dict()))
    s.load_transformers_state_dict(m.state_dict(), device=gpu)
    tot, worst = _image_errs(s, m, frames_like_video(4, 320, 576, seed=12))
    print(f"peaked image features rel-L2 {tot:.3e} (worst frame {worst:.3e})")
    assert tot <= 2.5e-3 and worst <= 2.5e-3


def _ids(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.tensor([49406]), torch.randint(1000, 49000, (n - 2,), generator=g), torch.tensor([49407])]).view(1, -1)


@pytest.mark.parametrize("n", [7, 77])
def test_text_features_match_clipmodel(scorer, clip_model, n):
    """get_text_features(...).pooler_output, fp32 on the CPU; 77 tokens is the longest prompt.  Measured: rel-L2 1.23e-3
    (7 tokens), 1.20e-3 (77)."""
    ids = _ids(n, seed=n)
    got = scorer.text_features(ids).float().cpu()
    with torch.no_grad():
        want = clip_model.get_text_features(input_ids=ids).pooler_output
    err = rel_l2(got, want)
    print(f"text features ({n} tokens) rel-L2 {err:.3e}")
    assert err <= 2.5e-3


def test_prompt_longer_than_77_tokens_raises(scorer):
    from vdx._lib import VdxError
    with pytest.raises(VdxError):
        scorer.text_features(_ids(78, seed=1))


@pytest.mark.parametrize("F", [1, 24])
def test_score_matches_the_reference_formula(scorer, clip_model, F):
    """PIL -> ImageNet normalize -> fp32 CLIPModel -> F.normalize -> dot -> mean, composed on the CPU (scoring.py:106-140).
    Measured: |d score| 6.8e-5 (F=1), 5.7e-5 (F=24); per-frame |d cos| at most 1.6e-4."""
    fr = frames_like_video(F, 576, 1024, seed=20 + F)
    ids = _ids(12, seed=F)
    score, per = scorer.score(fr, ids)
    with torch.no_grad():
        t = torch.nn.functional.normalize(clip_model.get_text_features(input_ids=ids).pooler_output, dim=-1)
        i = torch.nn.functional.normalize(clip_model.get_image_features(pixel_values=reference_pixels(fr)).pooler_output, dim=-1)
    want_per = (i @ t.T).view(-1)
    want = float(want_per.mean())
    d_per = float((per.double() - want_per.double()).abs().max())
    print(f"F={F}: score {score:.6f} vs {want:.6f} (|d| {abs(score - want):.2e}), per-frame max |d| {d_per:.2e}")
    assert per.shape == (F,) and d_per <= 1e-3 and abs(score - want) <= 5e-4


def test_score_is_deterministic_and_zero_frames_score_zero(scorer, gpu):
    from vdx.compat.diffusers_shim import HashTokenizer
    fr = torch.from_numpy(frames_like_video(6, 320, 576, seed=5)).to(gpu)
    a = scorer.score(fr, "a rocket in space, 4k", tokenizer=HashTokenizer())
    b = scorer.score(fr, "a rocket in space, 4k", tokenizer=HashTokenizer())
    assert a[0] == b[0] and torch.equal(a[1], b[1])
    s0, p0 = scorer.score(fr[:0], "x", tokenizer=HashTokenizer())
    assert s0 == 0.0 and p0.numel() == 0
    # an empty prompt is scored as "a video" (scoring.py:97-99)
    assert scorer.score(fr, "", tokenizer=HashTokenizer())[0] == scorer.score(fr, "a video", tokenizer=HashTokenizer())[0]


def test_quick_gelu_matches_torch(gpu):
    from vdx import ops
    x = (torch.randn(4096, 64, generator=torch.Generator().manual_seed(1)) * 4).half()
    got = ops.quick_gelu(x.to(gpu)).float().cpu()
    want = (x.float() * torch.sigmoid(1.702 * x.float())).half().float()
    assert float((got - want).abs().max()) <= 2 ** -10 * float(want.abs().max())


def test_pipeline_writes_clip_json_and_keeps_the_csv_row(gpu, tmp_path):
    """`python -m vdx.pipeline ... --clip_json` on tiny synthetic weights: the JSON is written, and the CSV row's columns
    that measure neither time nor memory equal those of the same run without the flag."""
    import json
    import vdx  # noqa: F401
    from vdx.pipeline import main
    out_csv = str(tmp_path / "r.csv")
    base = ["--model_id", "synthetic:tiny", "--num_frames", "8", "--steps", "2", "--height", "128", "--width", "256",
            "--chunk_size", "6", "--overlap", "2", "--mode", "chunk", "--out_csv", out_csv, "--out_video", "",
            "--noise_device", "cpu"]
    js = str(tmp_path / "clip.json")
    assert main(base) == 0
    assert main(base + ["--clip_json", js]) == 0
    rec = json.load(open(js))
    assert set(rec) == {"clip_score", "per_frame", "synthetic_weights", "tokenizer", "n_frames"}
    assert rec["n_frames"] == 8 and len(rec["per_frame"]) == 8 and rec["synthetic_weights"] is True
    assert rec["tokenizer"] == "pipeline:HashTokenizer" and -1.0 <= rec["clip_score"] <= 1.0
    assert abs(rec["clip_score"] - sum(rec["per_frame"]) / 8) < 1e-6
    rows = list(csv.DictReader(open(out_csv)))
    timed = {"timestamp", "latency_s", "throughput_fps", "net_gather_s", "net_reduce_s", "peak_vram_mb", "end_vram_mb"}
    assert len(rows) == 2 and rows[0].keys() == rows[1].keys()
    assert {k: v for k, v in rows[0].items() if k not in timed} == {k: v for k, v in rows[1].items() if k not in timed}


def test_pipeline_latency_does_not_include_the_score(gpu, tmp_path, monkeypatch):
    """--clip_json scores after the row took its latency: a scorer that takes 3 s leaves `latency_s` where a run without the
    flag has it, and runs only after the row is written."""
    import time
    import vdx  # noqa: F401
    from vdx import metrics, pipeline
    out_csv = str(tmp_path / "r.csv")
    base = ["--model_id", "synthetic:tiny", "--num_frames", "8", "--steps", "2", "--height", "128", "--width", "256",
            "--chunk_size", "6", "--overlap", "2", "--mode", "chunk", "--out_csv", out_csv, "--out_video", "",
            "--noise_device", "cpu"]
    events = []
    append = metrics.append_csv

    def appended(path, row):
        events.append("row")
        append(path, row)

    def slow_record(frames, prompt, clip_model, tok, device):
        events.append("score")
        time.sleep(3.0)
        return {"clip_score": 0.0, "per_frame": [], "synthetic_weights": True, "tokenizer": "stub", "n_frames": len(frames)}

    monkeypatch.setattr(metrics, "append_csv", appended)
    monkeypatch.setattr(pipeline, "clip_score_record", slow_record)
    assert pipeline.main(base) == 0
    assert pipeline.main(base + ["--clip_json", str(tmp_path / "c.json")]) == 0
    assert events == ["row", "row", "score"]
    rows = list(csv.DictReader(open(out_csv)))
    plain, flagged = float(rows[0]["latency_s"]), float(rows[1]["latency_s"])
    print(f"latency_s without the flag {plain:.2f}, with it {flagged:.2f} (scorer stub: 3 s)")
    assert flagged < plain + 1.5
