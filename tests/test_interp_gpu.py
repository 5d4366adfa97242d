"""GPU tests of the frame interpolation (vdx/interp.py, vdx.ops.interp_frames, csrc/interp.hip): the kernel against the
float64 restatement (tests/interp_ref.py) on the same fp32 flows, its properties, and the feature end to end up to the job."""
import numpy as np
import pytest
import torch

import interp_inputs as I
import interp_ref as R

pytestmark = pytest.mark.gpu

# Stage bound: at most one grey level anywhere, in at most a share of a case's bytes.  profiles/interp_parity.txt has the shares
# measured on the MI355X against the float64 restatement, per flow case the worst over the five sizes; the bound is 4x that,
# capped at 1e-3 (the remap test's cap).  Every difference measured is an exact tie of the stated expression at a penalised
# border pixel; the cases without one are byte-equal, and stay so: the kernel is one fixed sequence of IEEE operations.
MEASURED_SHARE = {"zero": 0.0, "const_int": 5.79e-4, "const_half": 0.0, "smooth": 0.0, "outside": 0.0, "wild": 0.0}
SHARE_CAP = 1e-3
# tests/test_interp_host.py's bound on interior MAE(interpolated) / MAE(plain blend): the measured 0.0 with a 2x margin (the GPU's
# own flows measure 0.0 as well: profiles/interp_parity.txt)
QUALITY_BOUND = min(2 * 0.0, 1.0)


def _dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)                        # a copy: the shared inputs are read-only


@pytest.mark.parametrize("name", I.STAGE_CASES)
@pytest.mark.parametrize("size", I.STAGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stage_parity_with_the_float64_restatement(gpu, size, name):
    from vdx import ops
    frames, fab, fba = I.stage_case(size, name)
    f, ab, ba = _dev(frames, gpu), _dev(fab, gpu), _dev(fba, gpu)
    before = [t.clone() for t in (f, ab, ba)]
    got = np.concatenate([ops.interp_frames(f, ab, ba, N).cpu().numpy() for N in I.stage_factors(name)])
    want = np.concatenate([R.interp_clip(frames, fab, fba, N) for N in I.stage_factors(name)])
    assert got.shape == want.shape
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    share = float(np.count_nonzero(d)) / d.size
    print(f"{size} {name}: max |d| {int(d.max())}, {int(np.count_nonzero(d))} of {d.size} bytes differ (share {share:.2e})")
    assert d.max() <= 1
    assert share <= min(4 * MEASURED_SHARE[name], SHARE_CAP)
    if name == "zero":                                                  # byte-equal to the copy
        assert np.array_equal(got, np.broadcast_to(frames[0], got.shape))
    for t, b in zip((f, ab, ba), before):                               # inputs are read only (NaN entries compare as bits)
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))


@pytest.fixture(scope="module")
def clip5(gpu):
    """Five 24 x 40 frames of the canvas moving by (1, 1) per frame, and their GPU flows both ways."""
    from vdx import flow
    frames = np.stack([I.crop(24, 40, -i, -i, seed=3) for i in range(5)])
    f = _dev(frames, gpu)
    fab = flow.farneback_flows(f)
    fba = flow.farneback_flows(f.flip(0)).flip(0).contiguous()
    return frames, f, fab, fba


@pytest.mark.parametrize("F", [2, 5])
@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_properties(gpu, clip5, F, N):
    from vdx import interp, ops
    frames, f, fab, fba = clip5
    out = interp.interpolate_frames(f[:F], N)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == ((F - 1) * N + 1, 24, 40, 3)
    assert torch.equal(out[::N], f[:F])                                 # the originals, byte for byte
    assert torch.equal(interp.interpolate_frames(f[:F], N), out)        # run to run
    assert torch.equal(interp.interpolate_frames(frames[:F], N, device=gpu), out)      # host frames: uploaded, the same bytes
    if N == 1:
        assert out.data_ptr() == f.data_ptr()                           # the input itself, not a copy
        return
    # the flows of a pair do not depend on the batch (tests/test_flow_gpu.py), nor does the kernel: a clip against its pairs
    assert torch.equal(ops.interp_frames(f[:F], fab[:F - 1], fba[:F - 1], N), out)
    for i in range(F - 1):
        pair = ops.interp_frames(f[i:i + 2], fab[i:i + 1], fba[i:i + 1], N)
        assert torch.equal(pair, out[i * N:(i + 1) * N + 1])
    # the symmetry of the expression, on the device: the reversed clip gives the reversed result
    rev = ops.interp_frames(f[:F].flip(0).contiguous(), fba[:F - 1].flip(0).contiguous(), fab[:F - 1].flip(0).contiguous(), N)
    assert torch.equal(rev.flip(0), out)


def test_single_frame_and_pitched_input(gpu, clip5):
    from vdx import interp, ops
    frames, f, fab, fba = clip5
    one = interp.interpolate_frames(f[:1], 3)
    assert tuple(one.shape) == (1, 24, 40, 3) and torch.equal(one, f[:1])
    wide = torch.zeros((5, 24, 47, 3), dtype=torch.uint8, device=gpu)   # rows and frames with a pitch, odd byte offsets
    wide[:, :, 3:43] = f
    view = wide[:, :, 3:43]
    assert not view.is_contiguous()
    assert torch.equal(ops.interp_frames(view, fab, fba, 2), ops.interp_frames(f, fab, fba, 2))


def test_refusals(gpu, clip5):
    from vdx import interp, ops
    from vdx._lib import VdxError, load
    frames, f, fab, fba = clip5
    for bad in (lambda: ops.interp_frames(f, fab, fba, 0), lambda: ops.interp_frames(f, fab, fba, 2.0),
                lambda: ops.interp_frames(f, fab[:3], fba, 2), lambda: ops.interp_frames(f, fab, fba.double(), 2),
                lambda: ops.interp_frames(f, fab.cpu(), fba, 2), lambda: ops.interp_frames(f[:1], fab[:0], fba[:0], 2),
                lambda: ops.interp_frames(f.cpu(), fab, fba, 2), lambda: ops.interp_frames(f, fab[..., :1], fba, 2),
                lambda: ops.interp_frames(f, fab, fba, 2, out=torch.empty((8, 24, 40, 3), dtype=torch.uint8, device=gpu)),
                lambda: interp.interpolate_frames(f.float(), 2), lambda: interp.interpolate_frames(f[:, :15], 2),
                lambda: interp.interpolate_frames(f, 1.5)):
        with pytest.raises(VdxError):
            bad()
    # the entry point's own refusals: null or misaligned flows, N < 1, F < 1 (nothing is launched)
    lib, out = load(), torch.empty((9, 24, 40, 3), dtype=torch.uint8, device=gpu)
    args = lambda **kw: [kw.get("frames", f.data_ptr()), f.stride(0), f.stride(1), kw.get("fab", fab.data_ptr()),
                         kw.get("fba", fba.data_ptr()), kw.get("F", 5), 24, 40, kw.get("N", 2), out.data_ptr(), out.stride(0), None]
    for kw, word in ((dict(fab=None), "null"), (dict(fba=None), "null"), (dict(fab=fab.data_ptr() + 4), "aligned"),
                     (dict(N=0), "N=0"), (dict(F=0), "F=0"), (dict(frames=None), "null")):
        assert lib.vdx_interp_frames_u8(*args(**kw)) != 0
        assert word in lib.vdx_last_error().decode()


def test_beats_the_plain_blend_with_the_gpus_own_flows(gpu):
    from vdx import interp
    A, B, truth = I.moving_pair()
    out = interp.interpolate_frames(np.stack([A, B]), 2, device=gpu).cpu().numpy()
    assert np.array_equal(out[0], A) and np.array_equal(out[2], B)
    e_interp, e_blend = I.interior_mae(out[1], truth), I.interior_mae(R.blend_pair(A, B, 1, 2), truth)
    print(f"interior MAE: interpolated {e_interp:.4f}, plain blend {e_blend:.4f}, ratio {e_interp / e_blend:.4f}")
    assert e_blend > 2.0 and e_interp / e_blend <= QUALITY_BOUND and e_interp / e_blend < 1


def test_written_file_has_the_interpolated_frames_and_rate(gpu, clip5, tmp_path):
    from vdx import interp, video
    _frames, f, _fab, _fba = clip5
    for N in (2, 3):
        out = interp.interpolate_frames(f, N)
        path = tmp_path / f"i{N}.mp4"
        video.write_frames(path, out, 8 * N)
        got, info = video.read_frames(path, device=gpu)
        assert info["n_frames"] == 4 * N + 1 == got.shape[0] and info["fps"] == 8.0 * N
        assert tuple(got.shape[1:]) == (24, 40, 3)


BASE = ["--model_id", "synthetic:tiny", "--num_frames", "8", "--steps", "2", "--height", "128", "--width", "256",
        "--chunk_size", "6", "--overlap", "2", "--mode", "chunk", "--noise_device", "cpu"]


def test_run_job_interpolates_what_it_writes_and_nothing_else(gpu, tmp_path):
    from vdx import interp, video
    from vdx.compat.diffusers_shim import DiffusionPipeline
    from vdx.pipeline import build_arg_parser, config_from_args, run_job
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    res, files, taken = {}, {}, {}
    for name, extra, kw in (("none", [], {}), ("one", ["--interpolate", "1"], {}), ("two", ["--interpolate", "2"], {}),
                            ("two_gpu", ["--interpolate", "2"], {"gpu_video_write": True})):
        mp4, got = tmp_path / f"{name}.mp4", {}
        res[name] = run_job(config_from_args(build_arg_parser().parse_args(BASE + extra)), out_video=str(mp4), pipe=pipe,
                            clip_inputs=got, **kw)
        files[name], taken[name] = mp4.read_bytes(), np.stack(got["frames"])
    assert files["one"] == files["none"]                                # --interpolate 1 is the run that never names it
    assert (res["none"]["interpolate"], res["none"]["frames_written"]) == (1, 8)
    assert (res["two"]["interpolate"], res["two"]["frames_written"]) == (2, 15) == (2, res["two_gpu"]["frames_written"])
    assert files["two_gpu"] == files["two"]                             # host writer and GPU writer alike
    for name in ("one", "two", "two_gpu"):                              # the numbers and the scored frames are the generated ones'
        assert np.array_equal(taken[name], taken["none"])
        assert all(res[name][k] == res["none"][k] for k in ("temp_instab", "flow_err", "num_frames"))
    assert res["none"]["temp_instab"] is not None
    _, info = video.read_frames(files["none"], device=gpu)
    assert info["n_frames"] == 8 and info["fps"] == 8.0
    _, info = video.read_frames(files["two"], device=gpu)
    assert info["n_frames"] == 15 and info["fps"] == 16.0
    # the file holds the encoder's rendering of exactly the interpolated clip
    want = tmp_path / "want.mp4"
    video.write_frames(want, interp.interpolate_frames(taken["none"], 2, device=gpu), 16)
    assert want.read_bytes() == files["two"]
    with pytest.raises(interp.VdxError):
        run_job(config_from_args(build_arg_parser().parse_args(BASE + ["--interpolate", "0"])), out_video=None, pipe=pipe)
