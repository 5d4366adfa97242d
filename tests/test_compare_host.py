"""Host tests of the full-reference clip comparison: the float64 definition (tests/compare_ref.py) in its closed forms, and the
argument handling of vdx/compare.py and of the job's --compare_to / --compare_json.  No GPU."""
import json
import math

import numpy as np
import pytest

import compare_ref as R


# ---- 1. closed forms -------------------------------------------------------------------------------------------------------
def test_identical_frames_give_ssim_one_exactly_and_infinite_psnr():
    g = np.random.default_rng(0)
    a = g.integers(0, 256, (180, 190, 3)).astype(np.uint8)
    assert R.ssim(a, a.copy()) == 1.0
    assert R.ms_ssim(a, a.copy()) == 1.0
    assert R.sse(a, a) == 0 and R.psnr(a, a) == math.inf


def test_white_against_black():
    a, b = np.full((20, 30, 3), 255, np.uint8), np.zeros((20, 30, 3), np.uint8)
    # the means are 255 and 0, every (co)variance is 0 up to the rounding of the window's sum: ssim = C1 / (255^2 + C1) * 1
    assert R.ssim(a, b) == pytest.approx(R.C1 / (255.0 ** 2 + R.C1), rel=1e-12)
    assert R.psnr(a, b) == 0.0
    assert R.sse(a, b) == 3 * 20 * 30 * 255 ** 2


def test_a_against_a_plus_one():
    g = np.random.default_rng(1)
    a = g.integers(0, 255, (23, 37, 3)).astype(np.uint8)             # below 255: a + 1 does not saturate
    assert R.sse(a, a + 1) == 3 * 23 * 37
    assert R.psnr(a, a + 1) == 10.0 * math.log10(255.0 ** 2)


# ---- 2. window and domain --------------------------------------------------------------------------------------------------
def test_window_is_the_normalised_gaussian():
    from vdx import compare
    w = R.window()
    d = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-d * d / 4.5)
    assert w.shape == (11,) and abs(w.sum() - 1.0) < 1e-15
    np.testing.assert_allclose(w, g / g.sum(), rtol=1e-15)
    assert np.array_equal(w, w[::-1])
    assert np.array_equal(compare.window(), w)                          # the kernels' taps are the definition's, bit for bit


def test_ms_ssim_clamps_a_negative_mean_to_zero():
    g = np.random.default_rng(2)
    x = g.integers(0, 256, (176, 180, 3)).astype(np.uint8)
    m = R.frame_means(x, 255 - x, 5)
    assert (m[:, 0, 1] < 0).all()                                       # cs at scale 0 is negative on every plane
    v = R.ms_ssim(x, 255 - x)
    assert v == 0.0 and not math.isnan(v)
    assert R.ssim(x, 255 - x) < 0


def test_size_refusals():
    from vdx import compare
    from vdx._lib import VdxError
    small = np.zeros((2, 10, 40, 3), np.uint8)
    for ms in (True, False):
        with pytest.raises(VdxError, match="too small for SSIM"):
            compare.compare_frames(small, small, ms_ssim=ms)
    with pytest.raises(ValueError):
        R.ssim(small[0], small[0])
    mid = np.zeros((1, 175, 300, 3), np.uint8)
    with pytest.raises(VdxError, match="too small for MS-SSIM"):
        compare.compare_frames(mid, mid)
    assert compare.check_pair(mid, mid, ms_ssim=False) == (1, 175, 300)
    with pytest.raises(ValueError):
        R.ms_ssim(mid[0], mid[0])
    assert R.ssim(mid[0], mid[0]) == 1.0


@pytest.mark.parametrize("a, b, what", [
    (np.zeros((2, 20, 20, 3), np.uint8), np.zeros((3, 20, 20, 3), np.uint8), "differ in shape"),
    (np.zeros((2, 20, 20, 3), np.uint8), np.zeros((2, 20, 21, 3), np.uint8), "differ in shape"),
    (np.zeros((2, 20, 20, 3), np.float32), np.zeros((2, 20, 20, 3), np.float32), "uint8"),
    (np.zeros((2, 20, 20), np.uint8), np.zeros((2, 20, 20), np.uint8), "uint8 RGB"),
    (np.zeros((0, 20, 20, 3), np.uint8), np.zeros((0, 20, 20, 3), np.uint8), "no frames"),
])
def test_bad_pairs_are_refused_before_any_upload(a, b, what, monkeypatch):
    from vdx import compare, frames
    from vdx._lib import VdxError
    monkeypatch.setattr(frames, "on_device", lambda *a, **k: pytest.fail("uploaded"))
    with pytest.raises(VdxError, match=what):
        compare.compare_frames(a, b, ms_ssim=False)


# ---- 3. seam frames --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, ranges, ends", [
    (8, [(0, 8)], []),
    (8, [], []),
    (8, [(0, 6), (4, 8)], [6]),
    (8, [(4, 8), (0, 6)], [6]),                                         # start order, not list order
    (12, [(0, 5), (3, 8), (6, 12)], [5, 8]),
    (6, [(0, 6), (4, 6)], []),                                          # an end at n is no boundary
    (10, [(0, 4), (4, 4 + 10), (8, 10)], [4]),                          # an end past the clip is skipped
])
def test_seam_frames_are_boundary_l1s_ends(n, ranges, ends):
    from vdx import compare, metrics
    assert compare.seam_frames(n, ranges) == sorted({i for e in ends for i in (e - 1, e)})
    # boundary_l1 on frames whose neighbour differences name their position: |f[e] - f[e-1]| = 2^(e-1)
    frames = [np.full((1, 1, 3), 2.0 ** i, np.float32) for i in range(n)]
    got = metrics.boundary_l1(frames, ranges)
    assert got == (float(np.mean([2.0 ** (e - 1) for e in ends])) if ends else None)


# ---- 4. argument handling --------------------------------------------------------------------------------------------------
BASE = ["--model_id", "synthetic:tiny", "--num_frames", "8", "--steps", "2", "--height", "128", "--width", "256", "--out_video", ""]


@pytest.fixture
def no_loading(monkeypatch):
    """The job's loader raises if it is reached."""
    from vdx.compat import diffusers_shim

    def reached(*a, **k):
        raise AssertionError("the model loader was reached")
    monkeypatch.setattr(diffusers_shim.DiffusionPipeline, "from_pretrained", reached)


def test_compare_to_and_compare_json_go_together(no_loading, tmp_path):
    from vdx import pipeline
    from vdx._lib import VdxError
    clip = tmp_path / "c.npy"
    np.save(clip, np.zeros((8, 128, 256, 3), np.uint8))
    for flags in (["--compare_to", str(clip)], ["--compare_json", str(tmp_path / "o.json")]):
        with pytest.raises(VdxError, match="together"):
            pipeline.main(BASE + ["--out_csv", str(tmp_path / "r.csv")] + flags)
    assert not (tmp_path / "r.csv").exists() and not (tmp_path / "o.json").exists()


def test_missing_and_mismatched_targets_are_refused_before_any_model_load(no_loading, tmp_path):
    from vdx import pipeline
    from vdx._lib import VdxError
    tail = ["--out_csv", str(tmp_path / "r.csv"), "--compare_json", str(tmp_path / "o.json")]
    with pytest.raises(VdxError, match="is not a file"):
        pipeline.main(BASE + tail + ["--compare_to", str(tmp_path / "nothing.npy")])
    for shape, dtype in (((7, 128, 256, 3), np.uint8), ((8, 128, 128, 3), np.uint8), ((8, 128, 256), np.uint8),
                         ((8, 128, 256, 3), np.float32)):
        clip = tmp_path / "c.npy"
        np.save(clip, np.zeros(shape, dtype))
        with pytest.raises(VdxError, match="holds"):
            pipeline.main(BASE + tail + ["--compare_to", str(clip)])
    bad = tmp_path / "bad.npy"
    bad.write_bytes(b"not numpy at all")
    with pytest.raises(VdxError, match="cannot read"):
        pipeline.main(BASE + tail + ["--compare_to", str(bad)])
    assert not (tmp_path / "r.csv").exists() and not (tmp_path / "o.json").exists()


def test_the_flags_default_to_off():
    from vdx import pipeline
    a = pipeline.build_arg_parser().parse_args([])
    assert a.compare_to is None and a.compare_json is None
    pipeline.check_compare_args(a)


def test_cli_json_writes_null_for_an_infinite_psnr(tmp_path, monkeypatch, capsys):
    from vdx import compare
    rec = {"n_frames": 2, "height": 16, "width": 16, "sse": [0, 12], "psnr": [math.inf, 40.5], "ssim": [1.0, 0.9],
           "mean": {"psnr": math.inf, "ssim": 0.95}, "identical": False}
    seen = {}

    def fake(path_a, path_b, **kw):
        seen.update(a=path_a, b=path_b, **kw)
        return dict(rec)
    monkeypatch.setattr(compare, "compare_files", fake)
    pa, pb = tmp_path / "a.npy", tmp_path / "b.npy"
    for p in (pa, pb):
        np.save(p, np.zeros((2, 16, 16, 3), np.uint8))
    out = tmp_path / "o.json"
    assert compare.main([str(pa), str(pb), "--json", str(out), "--no_ms_ssim"]) == 0
    assert seen["ms_ssim"] is False and seen["lpips"] is None
    text = out.read_text()
    assert "Infinity" not in text and "NaN" not in text
    back = json.loads(text)
    assert back == json.loads(capsys.readouterr().out)
    assert back["psnr"] == [None, 40.5] and back["mean"]["psnr"] is None and back["sse"] == [0, 12]
    assert back["identical"] is False and back["a"] == str(pa) and back["b"] == str(pb)
    with pytest.raises(ValueError):
        json.dumps(rec, allow_nan=False)                                # what the conversion is for


def test_cli_refuses_a_missing_file(tmp_path):
    from vdx import compare
    from vdx._lib import VdxError
    with pytest.raises(VdxError, match="is not a file"):
        compare.main([str(tmp_path / "a.npy"), str(tmp_path / "b.npy")])
