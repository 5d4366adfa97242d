"""Host side of the GPU Farneback flow (vdx/flow.py): the level plan against the shim's rule, the tap tables against scipy,
argument checks that must raise before any launch, and the opt-in wiring.  Needs no GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

import vdx  # noqa: F401
from vdx import _lib, flow
from vdx._lib import VdxError
from vdx.compat import cv2_shim

import flow_inputs as FI


def _shim_levels(H, W, levels, pyr_scale=0.5):
    """cv2_shim.py:161-168 restated: the level count it keeps and the sizes it resizes to."""
    levels = max(int(levels), 1)
    while levels > 1 and min(H, W) * pyr_scale ** (levels - 1) < 16:
        levels -= 1
    return [(max(int(round(H * pyr_scale ** k)), 1), max(int(round(W * pyr_scale ** k)), 1)) for k in range(levels)]


def test_level_plan_of_the_test_rows():
    sizes = lambda H, W: [(h, w) for h, w, _s, _r in flow.level_plan(H, W, 3)]   # noqa: E731
    assert sizes(24, 40) == [(24, 40)]
    assert sizes(72, 104) == [(72, 104), (36, 52), (18, 26)]
    assert sizes(97, 131) == [(97, 131), (48, 66), (24, 33)]                    # half to even: 48.5 -> 48, 65.5 -> 66
    assert sizes(576, 1024) == [(576, 1024), (288, 512), (144, 256)]
    assert [(s, r) for _h, _w, s, r in flow.level_plan(576, 1024, 3)] == [(0.0, 0), (0.5, 2), (1.5, 6)]


def test_level_plan_matches_the_shims_rule_sweep():
    for H in range(16, 131, 3):
        for W in range(16, 131):
            for levels in (1, 2, 3, 5):
                assert [(h, w) for h, w, _s, _r in flow.level_plan(H, W, levels)] == _shim_levels(H, W, levels), (H, W, levels)


def test_level_plan_level_count_is_what_the_shim_runs(monkeypatch):
    """Count the shim's own `_poly_exp` calls (two per level) on real frames: the plan has that many levels."""
    calls = []
    real = cv2_shim._poly_exp
    monkeypatch.setattr(cv2_shim, "_poly_exp", lambda img, n, s: calls.append(img.shape) or real(img, n, s))
    for H, W in ((16, 40), (31, 33), (32, 40), (63, 70), (64, 64)):
        calls.clear()
        g = np.zeros((H, W), np.uint8)
        cv2_shim.calcOpticalFlowFarneback(g, g, None, 0.5, 3, 15, 1, 5, 1.2, 0)
        assert calls[::2] == [(h, w) for h, w, _s, _r in flow.level_plan(H, W, 3)][::-1]


@pytest.mark.parametrize("sigma,radius", [(0.5, 2), (1.5, 6), (3.5, 14)])
def test_gaussian_taps_equal_scipys(sigma, radius):
    imp = np.zeros(4 * radius + 1)
    imp[2 * radius] = 1.0
    want = ndimage.gaussian_filter(imp, sigma, mode="mirror")[radius:3 * radius + 1]
    got = flow.gaussian_taps(sigma, radius)
    assert got.shape == (2 * radius + 1,) and np.abs(got - want).max() <= 1e-7
    assert np.abs(got.astype(np.float32) - want).max() <= 1e-7                   # as the kernel receives them
    assert want[0] > 0 and ndimage.gaussian_filter(imp, sigma, mode="mirror")[radius - 1] == 0   # scipy's radius is this one


def test_poly_tables_reproduce_the_shims_expansion():
    """The six moments through the host tables equal `_poly_exp` on a random image (float64, 1e-9)."""
    taps, inv_g = flow.poly_tables()
    assert taps.shape == (3, 11) and inv_g.shape == (5, 6)
    x = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-x * x / (2 * 1.2 * 1.2))
    g /= g.sum()
    assert np.abs(taps - np.stack([g, g * x, g * x * x])).max() <= 1e-15
    img = np.random.default_rng(0).standard_normal((40, 56)) * 50
    sep = lambda ky, kx: ndimage.correlate1d(ndimage.correlate1d(img, kx, axis=1, mode="mirror"), ky, axis=0, mode="mirror")  # noqa: E731
    k0, k1, k2 = taps
    m = np.stack([sep(k0, k0), sep(k0, k1), sep(k1, k0), sep(k0, k2), sep(k2, k0), sep(k1, k1)], -1)
    got = m @ inv_g.T
    for j, want in enumerate(cv2_shim._poly_exp(img, 5, 1.2)):
        assert np.abs(got[..., j] - want).max() <= 1e-9


@pytest.mark.parametrize("kw", [{"pyr_scale": 0.8}, {"winsize": 13}, {"poly_n": 7}, {"poly_sigma": 1.5},
                                {"flags": cv2_shim.OPTFLOW_FARNEBACK_GAUSSIAN}, {"flags": cv2_shim.OPTFLOW_USE_INITIAL_FLOW},
                                {"levels": 2.5}, {"iterations": "3"}])
def test_unsupported_parameters_raise_before_any_launch(kw, monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a launch was attempted"))
    with pytest.raises(VdxError):
        flow.farneback_flows(FI.pair((24, 40), (1.0, 0.5)), **kw)


def test_bad_frames_raise_before_any_launch(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a launch was attempted"))
    ok = FI.pair((24, 40), (1.0, 0.5))
    bad = [ok.astype(np.float32), ok.astype(np.int16), ok[..., :1], np.concatenate([ok, ok[..., :1]], -1), ok[0],
           torch.from_numpy(ok.copy()).float(), [ok[0], ok[1, :20]], ok[:, :15], ok[:, :, :15], ok[:1]]
    for fr in bad:
        with pytest.raises(VdxError):
            flow.farneback_flows(fr)
    for fr in bad[:8]:
        with pytest.raises(VdxError):
            flow.temporal_consistency(fr)
        with pytest.raises(VdxError):
            flow.flow_warp_error(fr, [(0, 1), (1, 2)])
    with pytest.raises(VdxError):
        flow.level_plan(15, 64, 3)


def test_no_pairs_need_no_gpu(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a launch was attempted"))
    fr = FI.clip(6, 72, 104, 1.5, -0.75)
    assert flow.temporal_consistency(fr[:1]) == 0.0 and flow.temporal_consistency(fr[:0]) == 0.0
    assert flow.flow_warp_error(fr, [(0, 6)]) is None and flow.flow_warp_error(fr[:1], [(0, 1)]) is None
    assert flow.flow_warp_error(fr, [(0, 6), (6, 12)]) is None                   # the only boundary lies past the clip
    assert flow.boundary_pairs(6, [(3, 6), (0, 3)]) == [3] and flow.boundary_pairs(8, [(0, 4), (2, 6), (4, 8)]) == [4, 6]


def test_opt_in_wiring_keeps_the_defaults():
    from vdx import metrics
    from vdx.mdvqs import MDVQS
    from vdx.pipeline import build_arg_parser, config_from_args
    p = build_arg_parser()
    assert p.parse_args([]).gpu_flow is False and config_from_args(p.parse_args([])).gpu_flow is False
    assert p.parse_args(["--gpu_flow"]).gpu_flow is True and config_from_args(p.parse_args(["--gpu_flow"])).gpu_flow is True
    assert MDVQS().flow == "cpu" and MDVQS(flow="gpu").flow == "gpu"
    with pytest.raises(VdxError):
        MDVQS(flow="opencl")
    # without a device the metric is the host path, value for value (cv2_shim through metrics._cv2)
    fr = list(FI.clip(6, 72, 104, 1.5, -0.75))
    want = metrics.flow_warp_error(fr, [(0, 3), (3, 6)])
    assert metrics.flow_warp_error(fr, [(0, 3), (3, 6)], device=None) == want and want > 0


def test_flow_symbols_are_bound_with_the_headers_argument_counts():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vdx.h")).read()
    names = [n for n in _lib.SIGNATURES if n.startswith("vdx_flow_")]
    assert len(names) == 7
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n) and f"int {n}(" in hdr
