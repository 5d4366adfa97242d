"""Host tests of the one intake of uint8 RGB clips (vdx/frames.py) and of the entry points that go through it.  The device
is "cpu" throughout, which takes every branch of the intake; no GPU."""
import warnings

import numpy as np
import pytest
import torch

import vdx  # noqa: F401
from vdx import _lib
from vdx._lib import VdxError

F, H, W = 3, 16, 20


def _clip(f=F, h=H, w=W, c=3, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (f, h, w, c), dtype=np.uint8)


def _refused():
    """name -> (a malformed clip, the words its refusal carries)."""
    ok = _clip()
    four, one = "uint8 RGB frames (F, H, W, 3), got ", "uint8 RGB frames (H, W, 3) of one size, got "
    return {"float32": (ok.astype(np.float32), four + "float32 (3, 16, 20, 3)"),
            "float32 tensor": (torch.from_numpy(ok).float(), four + "torch.float32 (3, 16, 20, 3)"),
            "no channels": (ok[..., 0], four + "uint8 (3, 16, 20)"),
            "rgba": (_clip(c=4), four + "uint8 (3, 16, 20, 4)"),
            "ragged list": ([ok[0], ok[1, :15], ok[2]], one + "uint8 (15, 20, 3)"),
            "float frame in a list": ([ok[0], ok[1], ok[2].astype(np.float32)], one + "float32 (16, 20, 3)")}


REFUSED = sorted(_refused())


# ---- 1. check ----------------------------------------------------------------------------------------------------------
def test_check_accepts_every_form_and_returns_the_shape():
    from vdx import frames
    a = _clip()
    t = torch.from_numpy(a.copy())
    for clip in (a, t, list(a), list(t), [a[0], t[1], a[2]], tuple(a)):
        assert frames.check(clip, "x") == (F, H, W)
    assert frames.check([], "x") == (0, 0, 0)
    assert frames.check(a[:0], "x") == (0, H, W) and frames.check(t[:0], "x") == (0, H, W)
    wide = torch.zeros((F, H, W + 7, 3), dtype=torch.uint8)
    assert frames.check(wide[:, :, :W], "x") == (F, H, W)               # layout is not `check`'s business


@pytest.mark.parametrize("name", REFUSED)
def test_check_refuses_under_the_callers_name(name):
    from vdx import frames
    bad, words = _refused()[name]
    with pytest.raises(VdxError) as e:
        frames.check(bad, "somebody")
    assert str(e.value) == "somebody: expected " + words


# ---- 2. on_device ------------------------------------------------------------------------------------------------------
def test_a_packed_tensor_already_there_is_not_copied():
    from vdx import frames
    t = torch.from_numpy(_clip())
    for index in (None, range(F), [0, 1, 2]):
        assert frames.on_device(t, "cpu", index).data_ptr() == t.data_ptr()
    wide = torch.from_numpy(_clip(w=W + 7, f=F + 1))
    view = wide[:F, :, 3:3 + W]                                         # row and frame pitch, an odd byte offset
    got = frames.on_device(view, torch.device("cpu"))
    assert not view.is_contiguous() and got.data_ptr() == view.data_ptr() and got.stride() == view.stride()


def test_anything_else_becomes_one_packed_copy_of_the_same_bytes():
    from vdx import frames
    rgba = _clip(c=4)
    views = [(torch.from_numpy(rgba)[..., :3], rgba[..., :3]),                               # pixel stride 4
             (rgba[..., :3], rgba[..., :3]),
             (rgba[..., 2::-1], rgba[..., 2::-1]),                                           # channels flipped: stride -1
             (torch.from_numpy(_clip()).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1), _clip()),   # planar
             (torch.from_numpy(_clip())[:, :, ::2], _clip()[:, :, ::2]),
             (list(_clip()), _clip()), ([torch.from_numpy(f) for f in _clip()], _clip()),
             ([_clip()[0], torch.from_numpy(_clip()[1])], _clip()[:2])]
    for clip, want in views:
        got = frames.on_device(clip, "cpu")
        assert got.dtype == torch.uint8 and got.is_contiguous() and frames.is_packed(got)
        assert np.array_equal(got.numpy(), want)


def test_an_index_touches_only_the_frames_it_names():
    from vdx import frames

    class Untouchable:
        def __array__(self, *a, **k):
            raise AssertionError("a frame outside the index was converted")

    a = _clip(f=5)
    clip = [Untouchable(), a[1], a[2], Untouchable(), Untouchable()]
    got = frames.on_device(clip, "cpu", index=[1, 2])
    assert np.array_equal(got.numpy(), a[1:3])
    with pytest.raises(AssertionError):
        frames.on_device(clip, "cpu")
    assert np.array_equal(frames.on_device(a, "cpu", [4, 4, 0]).numpy(), a[[4, 4, 0]])       # repeats and any order
    t = torch.from_numpy(a)
    got = frames.on_device(t, "cpu", [1, 2])
    assert torch.equal(got, t[1:3]) and got.is_contiguous()


def test_a_read_only_array_converts_without_a_warning():
    from vdx import frames
    a = _clip()
    ro = np.frombuffer(a.tobytes(), np.uint8).reshape(a.shape)
    assert not ro.flags.writeable
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for clip in (ro, list(ro), ro[:, :, ::2]):
            got = frames.on_device(clip, "cpu")
            assert np.array_equal(got.numpy(), np.stack(list(clip)))
        assert np.array_equal(frames.on_device(ro, "cpu", [2, 0]).numpy(), a[[2, 0]])


def test_device_for():
    from vdx import frames
    assert frames.device_for(_clip(), None) == torch.device("cuda")
    assert frames.device_for(torch.from_numpy(_clip()), None) == torch.device("cuda")
    assert frames.device_for(_clip(), "cuda:1") == torch.device("cuda", 1) and frames.device_for([], "cpu") == torch.device("cpu")


# ---- 3. is_packed is the launchers' verdict ----------------------------------------------------------------------------
class _AsIfOnTheGpu:
    """A host tensor that says it is on the GPU: `ops.check_u8_frames` past its device test, with no GPU."""
    is_cuda = True

    def __init__(self, t):
        self._t = t

    def __getattr__(self, name):
        return getattr(self._t, name)


def _layouts():
    x = torch.from_numpy(_clip(f=4, h=6, w=8))
    wide = torch.from_numpy(_clip(f=4, h=6, w=13))
    rgba = torch.from_numpy(_clip(f=4, h=6, w=8, c=4))
    return [("contiguous", x, True), ("row pitch", wide[:, :, :8], True), ("row pitch and offset", wide[:, :, 3:11], True),
            ("frame pitch", x[::2], True), ("row and frame pitch", wide[1::2, :, 2:10], True), ("every other row", x[:, ::2], True),
            ("one frame", x[1:2], True), ("every other column", x[:, :, ::2], False), ("rgba", rgba[..., :3], False),
            ("planar", x.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1), False),
            ("rows and columns swapped", x.transpose(1, 2), False), ("one frame repeated", x[:1].expand(4, 6, 8, 3), False),
            ("one row repeated", x[:, :1].expand(4, 6, 8, 3), False),
            ("rows that overlap", wide.as_strided((4, 6, 8, 3), (6 * 13 * 3, 12, 3, 1)), False),
            ("frames that overlap", wide.as_strided((4, 6, 8, 3), (39, 39, 3, 1)), False)]


@pytest.mark.parametrize("name, t, packed", _layouts(), ids=[r[0] for r in _layouts()])
def test_is_packed_agrees_with_the_launchers_check(name, t, packed):
    from vdx import frames, ops
    assert frames.is_packed(t) is packed
    if packed:
        assert ops.check_u8_frames(_AsIfOnTheGpu(t), "k") == tuple(t.shape[:3])
    else:
        with pytest.raises(VdxError, match="k: pixels must be packed"):
            ops.check_u8_frames(_AsIfOnTheGpu(t), "k")
    assert not frames.is_packed(t[..., 0])                               # not a clip at all: no, not an IndexError


# ---- 4. the entry points: a malformed clip is refused before anything is uploaded or launched -----------------------------
def _entry_points():
    """name -> the call, built on the host the way tests/test_mdvqs_host.py and tests/test_clip_score_host.py build the models."""
    from vdx import compare, flow, interp, mdvqs
    from vdx.clip_score import CLIPScorer
    from vdx.clip_text import CLIPTextConfig
    from vdx.clip_vision import CLIPVisionConfig
    from vdx.lpips import LPIPSAlex
    lp = LPIPSAlex.synthetic(seed=0, device="cpu")
    cs = CLIPScorer(CLIPTextConfig(hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8,
                                   hidden_act="quick_gelu"), CLIPVisionConfig())
    ids = torch.tensor([[49406, 320, 49407]])
    good = _clip()
    return {"compare.check_pair": lambda fr: compare.check_pair(fr, good, ms_ssim=False),
            "compare.check_pair (second clip)": lambda fr: compare.check_pair(good, fr, ms_ssim=False),
            "compare.compare_frames": lambda fr: compare.compare_frames(fr, good, ms_ssim=False),
            "interp.check_frames": interp.check_frames,
            "interp.interpolate_frames": lambda fr: interp.interpolate_frames(fr, 2),
            "flow.farneback_flows": flow.farneback_flows,
            "flow.temporal_consistency": flow.temporal_consistency,
            "flow.flow_warp_error": lambda fr: flow.flow_warp_error(fr, [(0, 2), (2, 3)]),
            "mdvqs.verify_video_authenticity": mdvqs.verify_video_authenticity,
            "LPIPSAlex": lp, "LPIPSAlex.features": lp.features,
            "CLIPScorer.score": lambda fr: cs.score(fr, ids), "CLIPScorer.image_features": cs.image_features}


@pytest.fixture(scope="module")
def entry_points():
    return _entry_points()


ENTRY_POINTS = ["compare.check_pair", "compare.check_pair (second clip)", "compare.compare_frames", "interp.check_frames",
                "interp.interpolate_frames", "flow.farneback_flows", "flow.temporal_consistency", "flow.flow_warp_error",
                "mdvqs.verify_video_authenticity", "LPIPSAlex", "LPIPSAlex.features", "CLIPScorer.score", "CLIPScorer.image_features"]


@pytest.fixture
def no_gpu_work(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a launch was attempted"))
    monkeypatch.setattr(torch.Tensor, "to", lambda *a, **k: pytest.fail("uploaded"))
    monkeypatch.setattr(torch.Tensor, "cuda", lambda *a, **k: pytest.fail("uploaded"))


@pytest.mark.parametrize("bad", REFUSED)
@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_entry_points_refuse_a_malformed_clip_before_any_upload_or_launch(entry, bad, entry_points, no_gpu_work):
    with pytest.raises(VdxError, match="expected uint8 RGB frames"):
        entry_points[entry](_refused()[bad][0])


def test_a_read_only_clip_reaches_the_first_kernel_without_a_warning(entry_points):
    """Up to `ops.frame_stats`, which refuses host tensors: the intake itself has nothing to warn about."""
    a = _clip()
    ro = np.frombuffer(a.tobytes(), np.uint8).reshape(a.shape)
    from vdx import mdvqs
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(VdxError, match="frame_stats: expected uint8 .* on the GPU"):
            mdvqs.verify_video_authenticity(ro, device="cpu")
