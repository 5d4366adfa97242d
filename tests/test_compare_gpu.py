"""GPU tests of the full-reference clip comparison (vdx/compare.py, vdx.ops.compare_*, csrc/compare.hip): the kernels against
the float64 restatement (tests/compare_ref.py), the properties that are equalities, and the feature up to the job."""
import csv
import json
import math

import numpy as np
import pytest
import torch

import compare_ref as R

pytestmark = pytest.mark.gpu

# profiles/compare_parity.txt (tools/compare_parity.py on the MI355X): per input kind the largest absolute difference from the
# float64 restatement over the sizes, frames, planes, the (ssim, cs) means of every scale and the frame's value.  The bounds
# are 4x these.  They are one to three units in the last place of a float64 near 1 (near 0.01 for independent noise): the
# kernel and numpy sum the same float64 products in different orders, nothing else differs.
MEASURED_SSIM = {"noise": 2.776e-17, "perturbed": 2.220e-16, "flat_bright": 2.220e-16, "step": 3.331e-16, "anticorrelated": 2.220e-16}
MEASURED_MS = {"perturbed": 2.220e-16, "flat_bright": 2.220e-16, "anticorrelated": 2.220e-16}


def _dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)


# ---- 1. PSNR is exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", R.PSNR_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sse_is_numpys_integer_sum_and_psnr_its_float64(gpu, size):
    from vdx import compare
    a, b = R.pair("noise", size, frames=3)
    a[2], b[2] = 255, 0                                                 # the largest sum a frame can hold
    rec = compare.compare_frames(_dev(a, gpu), _dev(b, gpu), ms_ssim=False)
    want = [R.sse(fa, fb) for fa, fb in zip(a, b)]
    assert rec["sse"] == want and all(isinstance(v, int) for v in rec["sse"])
    assert want[2] == 3 * size[0] * size[1] * 255 ** 2
    assert rec["psnr"] == [R.psnr(fa, fb) for fa, fb in zip(a, b)] and rec["psnr"][2] == 0.0
    assert rec["identical"] is False and "ms_ssim" not in rec


# ---- 2. SSIM and the scale-0 means ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.SSIM_KINDS)
@pytest.mark.parametrize("size", R.SSIM_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ssim_matches_the_float64_restatement(gpu, size, kind):
    from vdx import compare
    a, b = R.pair(kind, size)
    ta, tb = _dev(a, gpu), _dev(b, gpu)
    means, sse = compare.plane_means(ta, tb, 1)
    means = means.cpu().numpy()
    want = R.clip_means(a, b, 1)
    rec = compare.compare_frames(ta, tb, ms_ssim=False)
    d_means = float(np.abs(means[:, :, :1] - want).max())
    d_ssim = max(abs(rec["ssim"][f] - R.ssim_from_means(want[f])) for f in range(len(a)))
    print(f"{size} {kind}: means {d_means:.3e}, ssim {d_ssim:.3e}; ssim {rec['ssim']}")
    assert not means[:, :, 1:].any()                                    # the scales that were not asked for stay zero
    assert sse.cpu().tolist() == [R.sse(fa, fb) for fa, fb in zip(a, b)]
    assert max(d_means, d_ssim) <= 4 * MEASURED_SSIM[kind]
    if kind == "anticorrelated":
        assert max(rec["ssim"]) < 0
    assert torch.equal(ta.cpu(), torch.from_numpy(a)) and torch.equal(tb.cpu(), torch.from_numpy(b))


# ---- 3. MS-SSIM --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.MS_KINDS)
@pytest.mark.parametrize("size", R.MS_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ms_ssim_matches_the_float64_restatement(gpu, size, kind):
    from vdx import compare
    a, b = R.pair(kind, size)
    rec = compare.compare_frames(_dev(a, gpu), _dev(b, gpu))
    means = compare.plane_means(_dev(a, gpu), _dev(b, gpu), 5)[0].cpu().numpy()
    want = R.clip_means(a, b, 5)
    d_means = float(np.abs(means - want).max())
    d_ms = max(abs(rec["ms_ssim"][f] - R.ms_ssim_from_means(want[f])) for f in range(len(a)))
    print(f"{size} {kind}: means {d_means:.3e}, ms_ssim {d_ms:.3e}; ms_ssim {rec['ms_ssim']}")
    assert max(d_means, d_ms) <= 4 * MEASURED_MS[kind]
    if kind == "anticorrelated":                                        # the clamp: exactly 0, not NaN
        assert rec["ms_ssim"] == [0.0, 0.0] and (means[:, :, 0, 1] < 0).all()


# ---- 4. exact properties -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip5(gpu):
    a, b = R.pair("perturbed", (176, 177), frames=5)
    return a, b, _dev(a, gpu), _dev(b, gpu)


def test_a_clip_against_itself(gpu, clip5):
    from vdx import compare
    _a, _b, ta, _tb = clip5
    rec = compare.compare_frames(ta, ta.clone())
    assert rec["ssim"] == [1.0] * 5 and rec["ms_ssim"] == [1.0] * 5
    assert rec["sse"] == [0] * 5 and rec["psnr"] == [math.inf] * 5 and rec["identical"] is True
    assert rec["mean"] == {"psnr": math.inf, "ssim": 1.0, "ms_ssim": 1.0}


def test_swap_symmetry_bit_for_bit(gpu, clip5):
    from vdx import compare
    for kind in ("perturbed", "noise", "flat_bright"):
        a, b = R.pair(kind, (176, 177), frames=2)
        ta, tb = _dev(a, gpu), _dev(b, gpu)
        assert compare.compare_frames(ta, tb) == compare.compare_frames(tb, ta)
        m_ab, m_ba = compare.plane_means(ta, tb, 5)[0], compare.plane_means(tb, ta, 5)[0]
        assert torch.equal(m_ab.view(torch.int64), m_ba.view(torch.int64))


def test_batch_independence_and_repeatability_bit_for_bit(gpu, clip5):
    from vdx import compare
    _a, _b, ta, tb = clip5
    whole = compare.compare_frames(ta, tb)
    assert compare.compare_frames(ta, tb) == whole
    for i in range(5):
        one = compare.compare_frames(ta[i:i + 1], tb[i:i + 1])
        for k in ("sse", "psnr", "ssim", "ms_ssim"):
            assert one[k] == [whole[k][i]], (k, i)
    m5 = compare.plane_means(ta, tb, 5)[0]
    m1 = compare.plane_means(ta[3:4], tb[3:4], 5)[0]
    assert torch.equal(m5[3].view(torch.int64), m1[0].view(torch.int64))


def test_frames_on_the_gpu_are_used_where_they_are(gpu, clip5, monkeypatch):
    from vdx import compare, ops
    _a, _b, ta, tb = clip5
    seen = []
    real = ops.compare_ssim_scale

    def spy(x, y, taps):
        seen.append((x.data_ptr(), y.data_ptr(), x.dtype))
        return real(x, y, taps)
    monkeypatch.setattr(ops, "compare_ssim_scale", spy)
    compare.compare_frames(ta, tb, ms_ssim=False)
    assert seen == [(ta.data_ptr(), tb.data_ptr(), torch.uint8)]


def test_seams_and_means(gpu, clip5):
    from vdx import compare
    _a, _b, ta, tb = clip5
    rec = compare.compare_frames(ta, tb, ranges=[(0, 3), (2, 5)])
    assert rec["seam_frames"] == [2, 3]
    for k in ("psnr", "ssim", "ms_ssim"):
        assert rec["seam"][k] == (rec[k][2] + rec[k][3]) / 2
        assert rec["interior"][k] == (rec[k][0] + rec[k][1] + rec[k][4]) / 3
        assert rec["mean"][k] == sum(rec[k]) / 5
    plain = compare.compare_frames(ta, tb, ranges=[(0, 5)])
    assert "seam_frames" not in plain and "seam" not in plain and "interior" not in plain
    assert plain == compare.compare_frames(ta, tb)


def test_host_arrays_sequences_and_pitched_frames(gpu, clip5):
    from vdx import compare
    a, b, ta, tb = clip5
    want = compare.compare_frames(ta[:2], tb[:2], ms_ssim=False)
    assert compare.compare_frames(a[:2], b[:2], ms_ssim=False, device=gpu) == want
    assert compare.compare_frames(list(a[:2]), [tb[0], tb[1]], ms_ssim=False, device=gpu) == want
    wide = torch.zeros((2, 176, 200, 3), dtype=torch.uint8, device=gpu)
    wide[:, :, :177] = ta[:2]
    assert compare.compare_frames(wide[:, :, :177], tb[:2], ms_ssim=False) == want


def test_kernels_refuse_what_they_do_not_take(gpu):
    from vdx import ops
    from vdx._lib import VdxError
    small = torch.zeros((1, 10, 40, 3), dtype=torch.uint8, device=gpu)
    with pytest.raises(VdxError):
        ops.compare_ssim_scale(small, small, R.window())
    ok = torch.zeros((1, 12, 12, 3), dtype=torch.uint8, device=gpu)
    with pytest.raises(VdxError):
        ops.compare_ssim_scale(ok, ok, R.window()[:10])
    with pytest.raises(VdxError):
        ops.compare_ssim_scale(ok, ok.float(), R.window())
    with pytest.raises(VdxError):
        ops.compare_ssim_scale(ok, ok[:, :11], R.window())


# ---- 5. down2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(13, 17), (12, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_down2_against_numpy(gpu, size):
    from vdx import ops
    H, W = size
    g = np.random.default_rng(H * 100 + W)
    u8 = g.integers(0, 256, (2, H, W, 3)).astype(np.uint8)
    other = g.integers(0, 256, (2, H, W, 3)).astype(np.uint8)
    got_a, got_b = (t.cpu().numpy() for t in ops.compare_down2(_dev(u8, gpu), _dev(other, gpu)))
    for got, src in ((got_a, u8), (got_b, other)):
        assert got.shape == (6, H // 2, W // 2) and got.dtype == np.float32
        for f in range(2):
            for c in range(3):
                want = R.down2(src[f, :, :, c])                          # sums of four bytes over 4 are exact in fp32
                assert np.array_equal(got[3 * f + c].astype(np.float64), want)
    assert np.array_equal(ops.compare_down2(_dev(u8, gpu)).cpu().numpy(), got_a)
    f32 = (g.standard_normal((5, H, W)) * 100).astype(np.float32)
    got = ops.compare_down2(_dev(f32, gpu)).cpu().numpy()
    p = f32[:, :2 * (H // 2), :2 * (W // 2)]
    want = ((p[:, 0::2, 0::2] + p[:, 0::2, 1::2]) + (p[:, 1::2, 0::2] + p[:, 1::2, 1::2])) * np.float32(0.25)
    assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- 6. files --------------------------------------------------------------------------------------------------------------------
def test_compare_files(gpu, tmp_path):
    from vdx import compare, video
    from vdx._lib import VdxError
    import lpips_ref as L
    frames = L.frames_like_video(3, 48, 64, seed=3)
    mp4, npy = tmp_path / "c.mp4", tmp_path / "c.npy"
    video.write_frames(mp4, _dev(frames, gpu), 8)
    np.save(npy, frames)
    rec = compare.compare_files(mp4, npy, ms_ssim=False)
    assert rec == compare.compare_frames(video.read_frames(mp4, device=gpu)[0], frames, ms_ssim=False)
    assert rec["identical"] is False and all(20 < p < math.inf for p in rec["psnr"])      # JPEG is lossy, but close
    assert compare.compare_files(npy, npy, ms_ssim=False)["identical"] is True
    grey = np.full((2, 48, 64, 3), 128, np.uint8)                       # a constant grey clip survives JPEG
    gmp4, gnpy = tmp_path / "g.mp4", tmp_path / "g.npy"
    video.write_frames(gmp4, _dev(grey, gpu), 8)
    np.save(gnpy, grey)
    assert compare.compare_files(gmp4, gnpy, ms_ssim=False)["identical"] is True
    bad = tmp_path / "bad.mp4"
    bad.write_bytes(b"\x00\x00\x00\x18ftypisom" + b"\x00" * 64)
    with pytest.raises(VdxError, match="mp4"):
        compare.compare_files(bad, npy, ms_ssim=False)
    out = tmp_path / "o.json"
    assert compare.main([str(mp4), str(npy), "--no_ms_ssim", "--json", str(out)]) == 0
    back = json.loads(out.read_text())
    assert back["ssim"] == rec["ssim"] and back["sse"] == rec["sse"] and back["a"] == str(mp4)


# ---- 7. the job ------------------------------------------------------------------------------------------------------------------
BASE = ["--model_id", "synthetic:tiny", "--num_frames", "8", "--steps", "2", "--height", "128", "--width", "256",
        "--chunk_size", "6", "--overlap", "2", "--mode", "chunk", "--out_video", "", "--noise_device", "cpu"]


def test_pipeline_compares_with_an_earlier_run(gpu, tmp_path, monkeypatch):
    from vdx import pipeline
    got = {}
    res = pipeline.run_job(pipeline.config_from_args(pipeline.build_arg_parser().parse_args(BASE)), out_video=None, clip_inputs=got)
    first = tmp_path / "first.npy"
    np.save(first, np.stack(got["frames"]))
    assert len(got["ranges"]) > 1
    out_csv, js = str(tmp_path / "r.csv"), tmp_path / "cmp.json"
    assert pipeline.main(BASE + ["--out_csv", out_csv]) == 0
    assert pipeline.main(BASE + ["--out_csv", out_csv, "--compare_to", str(first), "--compare_json", str(js)]) == 0
    rec = json.loads(js.read_text())
    assert rec["identical"] is True and rec["compare_to"] == str(first) and rec["n_frames"] == 8
    assert rec["sse"] == [0] * 8 and rec["psnr"] == [None] * 8 and rec["ssim"] == [1.0] * 8
    assert "ms_ssim" not in rec                                         # 128 x 256 is below 176
    rows = list(csv.DictReader(open(out_csv)))
    timed = {"timestamp", "latency_s", "throughput_fps", "net_gather_s", "net_reduce_s", "peak_vram_mb", "end_vram_mb"}
    assert len(rows) == 2 and rows[0].keys() == rows[1].keys()
    assert {k: v for k, v in rows[0].items() if k not in timed} == {k: v for k, v in rows[1].items() if k not in timed}
    assert res["temp_instab"] is not None

    real = pipeline.seeded_noise

    def other_seed(shape, sigma, device, noise_device=None, dtype=torch.float16):
        base = real(shape, sigma, device, noise_device, dtype)          # the job's own call, then the draw after it
        nd = torch.device(noise_device) if noise_device is not None else torch.device(device)
        return (torch.randn(*shape, device=nd, dtype=dtype) * sigma).to(base.device)
    monkeypatch.setattr(pipeline, "seeded_noise", other_seed)
    assert pipeline.main(BASE + ["--out_csv", out_csv, "--compare_to", str(first), "--compare_json", str(js)]) == 0
    rec = json.loads(js.read_text())
    ends = [e for _s, e in sorted(got["ranges"])[:-1] if 0 < e < 8]
    assert rec["identical"] is False and any(rec["sse"])
    assert rec["seam_frames"] == sorted({i for e in ends for i in (e - 1, e)})
    assert set(rec["seam"]) == set(rec["interior"]) == {"psnr", "ssim"} and rec["seam"]["ssim"] < 1.0


# ---- 8. lpips= ---------------------------------------------------------------------------------------------------------------------
def test_lpips_values_are_vdx_lpips_called_directly(gpu):
    from vdx import compare
    from vdx.lpips import LPIPSAlex
    from vdx._lib import VdxError
    import lpips_ref as L
    lp = LPIPSAlex.synthetic(seed=0, device=gpu)
    a = L.frames_like_video(3, 100, 150, seed=1)
    b = L.frames_like_video(3, 100, 150, seed=2)
    rec = compare.compare_frames(a, b, ms_ssim=False, lpips=lp, device=gpu)
    want = [float(lp(np.stack([a[i], b[i]]))[0]) for i in range(3)]
    assert rec["lpips"] == want and all(v > 0 for v in want)
    assert rec["mean"]["lpips"] == sum(want) / 3
    assert "lpips" not in compare.compare_frames(a, b, ms_ssim=False, device=gpu)
    with pytest.raises(VdxError):
        compare.compare_frames(a, b, ms_ssim=False, lpips="alex", device=gpu)
