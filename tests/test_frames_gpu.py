"""-m gpu: every consumer of a uint8 RGB clip takes it in each form vdx/frames.py accepts, gives the same bits for each, and
reads a clip that is already on the GPU where it lies.  One 3-frame clip of 24 x 40 noise: the smallest size every consumer
takes (the flow needs min(H, W) >= 16, SSIM >= 11; MS-SSIM is off)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F, H, W, WIDE, X0 = 3, 24, 40, 47, 3


@pytest.fixture(scope="module")
def forms(gpu):
    """name -> the same clip as a packed GPU tensor, a host array, a list of host frames and a pitched crop of a 47-wide one."""
    a = np.random.default_rng(0).integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    wide = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (F, H, WIDE, 3), dtype=np.uint8)).to(gpu)
    wide[:, :, X0:X0 + W] = torch.from_numpy(a).to(gpu)
    pitched = wide[:, :, X0:X0 + W]
    assert not pitched.is_contiguous() and pitched.data_ptr() % 2 == 1
    return {"packed": torch.from_numpy(a).to(gpu), "array": a, "list": list(a), "pitched": pitched}


@pytest.fixture(scope="module")
def consumers(gpu):
    """name -> (the call, the name of the first `ops` launcher the clip reaches)."""
    from vdx import compare, flow, interp, mdvqs
    from vdx.lpips import LPIPSAlex
    other = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (F, H, W, 3), dtype=np.uint8)).to(gpu)
    lp = LPIPSAlex.synthetic(seed=0, device=gpu)
    out = {"compare_frames": (lambda fr: compare.compare_frames(fr, other, ms_ssim=False, device=gpu), "compare_ssim_scale"),
           "interpolate_frames": (lambda fr: interp.interpolate_frames(fr, 2, device=gpu), "flow_grey"),
           "farneback_flows": (lambda fr: flow.farneback_flows(fr, device=gpu), "flow_grey"),
           "temporal_consistency": (lambda fr: flow.temporal_consistency(fr, device=gpu), "flow_grey"),
           "verify_video_authenticity": (lambda fr: mdvqs.verify_video_authenticity(fr, device=gpu), "frame_stats"),
           "LPIPSAlex": (lp, "resize_u8")}
    return out


@pytest.fixture(scope="module")
def clip_scorer(gpu):
    pytest.importorskip("transformers")
    from vdx.clip_score import CLIPScorer
    return CLIPScorer.synthetic(seed=0, device=gpu)


def _same(x, y):
    if isinstance(x, torch.Tensor):
        return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    if isinstance(x, tuple):
        return len(x) == len(y) and all(_same(p, q) for p, q in zip(x, y))
    return type(x) is type(y) and x == y                                 # floats, dicts and lists of floats, bools


def _check(call, launcher, forms, monkeypatch):
    from vdx import ops
    seen = []
    real = getattr(ops, launcher)

    def spy(clip, *a, **k):
        seen.append(clip.data_ptr())
        return real(clip, *a, **k)
    monkeypatch.setattr(ops, launcher, spy)
    want = call(forms["packed"])
    assert seen[0] == forms["packed"].data_ptr()                        # used where it lies
    for name in ("array", "list", "pitched"):
        del seen[:]
        got = call(forms[name])
        assert _same(got, want), name
        assert seen and (seen[0] == forms["pitched"].data_ptr()) == (name == "pitched")
    return want


@pytest.mark.parametrize("name", ["compare_frames", "interpolate_frames", "farneback_flows", "temporal_consistency",
                                  "verify_video_authenticity", "LPIPSAlex"])
def test_every_form_gives_the_same_bits_and_gpu_clips_are_read_in_place(name, consumers, forms, monkeypatch):
    call, launcher = consumers[name]
    want = _check(call, launcher, forms, monkeypatch)
    if name == "compare_frames":
        assert want["n_frames"] == F and not want["identical"]
    elif name == "interpolate_frames":
        assert tuple(want.shape) == (2 * F - 1, H, W, 3) and torch.equal(want[::2], forms["packed"])
    elif name == "farneback_flows":
        assert tuple(want.shape) == (F - 1, H, W, 2) and bool(want.abs().sum() > 0)
    elif name == "temporal_consistency":
        assert want > 0.0
    elif name == "verify_video_authenticity":
        assert want[1]["diff_mean"] > 0 and want[1]["entropy_mean"] > 7     # noise: nearly 8 bits per pixel
    else:
        assert tuple(want.shape) == (F - 1,) and bool((want > 0).all())


def test_clip_score_takes_every_form(clip_scorer, forms, monkeypatch):
    ids = torch.tensor([[49406, 320, 1125, 49407]])
    q, per = _check(lambda fr: clip_scorer.score(fr, ids), "clip_preprocess", forms, monkeypatch)
    assert per.shape == (F,) and abs(q - float(per.mean())) < 1e-6


def test_the_intake_on_the_gpu(gpu, forms):
    """`on_device` itself: no copy of what is in place, one packed copy of anything else, a list of GPU frames included."""
    from vdx import frames
    packed, pitched = forms["packed"], forms["pitched"]
    for t in (packed, pitched):
        for dev in (gpu, "cuda", torch.device("cuda")):
            assert frames.on_device(t, dev).data_ptr() == t.data_ptr()
    sub = frames.on_device(pitched, gpu, [2, 0])
    assert sub.is_contiguous() and torch.equal(sub, packed[[2, 0]])
    rgba = torch.zeros((F, H, W, 4), dtype=torch.uint8, device=gpu)
    rgba[..., :3] = packed
    for clip in (rgba[..., :3], [packed[0], packed[1], packed[2]], forms["array"], packed.cpu()):
        got = frames.on_device(clip, gpu)
        assert got.device == gpu and got.is_contiguous() and torch.equal(got, packed)
    assert frames.device_for(pitched) == gpu and frames.device_for(forms["array"]) == torch.device("cuda")
