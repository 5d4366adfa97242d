"""The frame interpolation's restatement (tests/interp_ref.py) on the CPU: its symmetries, what it reproduces exactly, that
it beats the plain blend on a moving texture, that float32 evaluates it like float64 on the stage-test inputs (which is what
admits them to tests/test_interp_gpu.py), and the refusals of vdx/interp.py that need no library."""
import numpy as np
import pytest

import interp_inputs as I
import interp_ref as R

# profiles/interp_parity.txt: interior MAE of the interpolated middle frame over that of the plain blend, measured with the
# float64 shim's flows on the moving pair: 0.0 (the true middle frame is reproduced exactly; the blend is off by 10.2 grey
# levels).  Asserted with a 2x margin, which leaves 0, and never looser than < 1.  The 0 is no accident of rounding: the
# largest flow error there is 3.8e-3 px and the canvas' steepest step 43 grey levels per px, so a sample is within 0.17 of the
# integer it rounds to.
QUALITY_RATIO = 0.0
QUALITY_BOUND = min(2 * QUALITY_RATIO, 1.0)
# the stage bound of tests/test_interp_gpu.py: at most one grey level, in at most this share of a case's bytes (the cap; the
# remap test's)
SHARE_CAP = 1e-3


def _shim_flows(A, B):
    from vdx.compat import cv2_shim
    ga, gb = cv2_shim.cvtColor(A, cv2_shim.COLOR_RGB2GRAY), cv2_shim.cvtColor(B, cv2_shim.COLOR_RGB2GRAY)
    args = (None, 0.5, 3, 15, 3, 5, 1.2, 0)
    return cv2_shim.calcOpticalFlowFarneback(ga, gb, *args), cv2_shim.calcOpticalFlowFarneback(gb, ga, *args)


@pytest.fixture(scope="module")
def moving():
    A, B, truth = I.moving_pair()
    fab, fba = _shim_flows(A, B)
    return A, B, truth, fab, fba


def test_swap_symmetry_is_exact(moving):
    A, B, _truth, fab, fba = moving
    for k, N in ((1, 2), (1, 3), (2, 3), (1, 4), (3, 7)):
        assert np.array_equal(R.interp_pair(A, B, fab, fba, k, N), R.interp_pair(B, A, fba, fab, N - k, N))
    frames, fab, fba = I.stage_case((17, 19), "wild")                   # NaN and inf entries follow the same rule
    assert np.array_equal(R.interp_pair(frames[0], frames[1], fab[0], fba[0], 1, 3),
                          R.interp_pair(frames[1], frames[0], fba[0], fab[0], 2, 3))


def test_zero_flows_on_equal_frames_give_the_frame(moving):
    A = moving[0]
    z = np.zeros(A.shape[:2] + (2,), np.float32)
    for k, N in ((1, 2), (1, 3), (3, 4)):
        assert np.array_equal(R.interp_pair(A, A, z, z, k, N), A)


def test_constant_integer_flow_gives_the_half_way_crop():
    H, W = I.QUALITY_HW
    for dx, dy in ((4, 2), (-6, 2), (2, -8), (0, 4)):
        A, B, M = I.crop(H, W, 0, 0), I.crop(H, W, -dx, -dy), I.crop(H, W, -dx // 2, -dy // 2)
        fab = np.broadcast_to(np.array([dx, dy], np.float32), (H, W, 2))
        got = R.interp_pair(A, B, fab, -fab, 1, 2)
        b = 8                                                           # |d| / 2 <= 4 < 8: no clamped position inside
        assert np.array_equal(got[b:-b, b:-b], M[b:-b, b:-b])


def test_clip_layout():
    frames = np.stack([I.crop(16, 20, i, 0) for i in range(3)])
    z = np.zeros((2, 16, 20, 2), np.float32)
    out = R.interp_clip(frames, z, z, 3)
    assert out.shape == (7, 16, 20, 3) and np.array_equal(out[::3], frames)
    assert np.array_equal(out[1], R.interp_pair(frames[0], frames[1], z[0], z[0], 1, 3))
    assert np.array_equal(R.interp_clip(frames, z, z, 1), frames)


def test_beats_the_plain_blend_on_a_moving_texture(moving):
    A, B, truth, fab, fba = moving
    e_interp = I.interior_mae(R.interp_pair(A, B, fab, fba, 1, 2), truth)
    e_blend = I.interior_mae(R.blend_pair(A, B, 1, 2), truth)
    print(f"interior MAE: interpolated {e_interp:.4f}, plain blend {e_blend:.4f}, ratio {e_interp / e_blend:.4f}")
    assert e_blend > 2.0                                                # the texture does move: the blend is visibly wrong
    assert e_interp / e_blend <= QUALITY_BOUND and e_interp / e_blend < 1


@pytest.mark.parametrize("name", I.STAGE_CASES)
@pytest.mark.parametrize("size", I.STAGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_float32_evaluates_the_stage_inputs_like_float64(size, name):
    """What admits an input to the GPU stage test: the expression in float32 (the kernel's type) is within one grey level of
    float64 everywhere, and differs in at most SHARE_CAP of the case's bytes."""
    frames, fab, fba = I.stage_case(size, name)
    want = np.concatenate([R.interp_clip(frames, fab, fba, N) for N in I.stage_factors(name)])
    got = np.concatenate([R.interp_clip(frames, fab, fba, N, dtype=np.float32) for N in I.stage_factors(name)])
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    share = float(np.count_nonzero(d)) / d.size
    print(f"{size} {name}: max |d| {int(d.max())}, share {share:.2e} of {d.size} bytes")
    assert d.max() <= 1 and share <= SHARE_CAP
    if name == "zero":
        assert np.array_equal(want, np.broadcast_to(frames[0], want.shape))


def test_refusals_that_need_no_library():
    from vdx import interp
    from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args
    ok = np.zeros((2, 16, 16, 3), np.uint8)
    for bad in (ok.astype(np.float32), ok.astype(np.int8), ok[0], ok[..., :2], ok[..., 0], np.zeros((2, 15, 40, 3), np.uint8),
                np.zeros((2, 40, 15, 3), np.uint8), [ok[0], np.zeros((16, 17, 3), np.uint8)]):
        with pytest.raises(interp.VdxError):
            interp.interpolate_frames(bad, 2)
    for factor in (0, -1, 2.0, 1.5, "2", None, True, interp.MAX_FACTOR + 1):
        with pytest.raises(interp.VdxError):
            interp.interpolate_frames(ok, factor)
    assert interp.n_output_frames(24, 2) == 47 and interp.n_output_frames(24, 1) == 24 and interp.n_output_frames(1, 4) == 1
    assert DiffuserConfig().interpolate == 1
    assert config_from_args(build_arg_parser().parse_args([])).interpolate == 1
    assert config_from_args(build_arg_parser().parse_args(["--interpolate", "3"])).interpolate == 3
