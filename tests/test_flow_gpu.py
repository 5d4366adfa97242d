"""The GPU Farneback flow (vdx/flow.py, csrc/flow.hip) against the project's own float64 shim (`vdx.compat.cv2_shim`, imported
explicitly in tests/flow_inputs.py), and the two numbers built on it: MD-VQS temporal consistency and `flow_err`.

Rows (tests/flow_inputs.py), the smallest inputs at which each part can go wrong:
    (24, 40)    (1.0, 0.5)     the level rule collapses to one level
    (72, 104)   (1.5, -0.75)   three levels 72x104 / 36x52 / 18x26, no size a multiple of a tile
    (72, 104)   (6.0, -3.0)    the coarse levels carry the motion; clamped sampling at the border
    (97, 131)   (-2.25, 1.5)   odd sizes, half-to-even level sizes 48x66 / 24x33
    (64, 200)   (3.0, 3.0)     wide aspect, many tiles in x
    (576, 1024) (1.5, -0.75)   the real extent, one pair

Content rows (tests/flow_inputs.py `content_clip`), all (72, 104) with integer pixel values, frame i moved by i x the shift:
    diagonal    edge x + y < 90 + 3 i, grey 245 / 10: every window sees one straight edge, the 2 x 2 system is nearly singular
    square      white 24 x 32 square on black, +3 px: flat inside and outside, edges in both directions, corners
    noise_roll  uniform noise rolled by 2 px: texture at the pixel scale, above the pyramid's pass band at level 0
    noise_pair  noise against unrelated noise: no motion to find, large flows that clamp at every border
    mixed       left half the textured clip, right half the diagonal edge: well and badly conditioned windows side by side
    step        vertical step, +2 px        \
    bars        8-px bars, +1 px             | one-dimensional or flat: g12 = g22 = 0, the regularised solve gives a flow of ~0
    ramp        2 grey levels per px, +2 px  | (the shim's is asserted < 1e-6 px); max-abs only, rel-L2 is undefined
    constant    128 everywhere              /

Bounds.  FLOW_MAX_ABS / FLOW_REL_L2 are 4x the worst figures measured on an MI355X over all six rows with the all-fp32
kernels (tools/flow_parity.py; 4x is the project's head-room for fp32 summation-order differences
between boxes; measured then: max-abs 8.9e-7 .. 1.7e-5 px, rel-L2 1.9e-7 .. 1.0e-6, remap bytes differing from the shim's at
most 5.3e-5 of a frame, each by one grey level), and FLOW_MAX_ABS may not exceed 1e-3 px: a wrong tap, border mode, level size or off-by-one moves these
fields by 1e-2 px or more, fp32 rounding sits near 1e-5 px.  The content rows have their own pair, STRUCT_MAX_ABS / STRUCT_REL_L2,
4x the worst figures measured over those rows (same file, same tool), and STRUCT_MAX_ABS may not exceed 2e-3 px, a fifth of
that 1e-2 px (profiles/flow_parity.txt holds the current figures of every row).  FLOW_MAX_ABS / FLOW_REL_L2 are kept as they were; since polyexp and update compute in fp64
the six rows measure max-abs 1.2e-7 .. 4.8e-7 px and rel-L2 9.2e-9 .. 2.1e-8.  With the all-fp32 kernels the content rows measured,
on the same device: diagonal max-abs 0.97 px (23 % of the values off by more than 1e-3 px, TC 5.0 % off), mixed 0.94 px, bars
8.7e-3 px, step 3.1e-3 px, square 2.4e-4 px, noise_pair 2.1e-4 px: det = g0 g2 - g1^2 + 1e-3 cancels in fp32 where a window sees one
straight edge."""
import json

import numpy as np
import pytest
import torch

import vdx  # noqa: F401
from vdx import flow, metrics
from vdx.compat import cv2_shim

import flow_inputs as FI

pytestmark = pytest.mark.gpu

FLOW_MAX_ABS = 4 * 1.729e-5  # px; worst row measured: (72, 104) (6.0, -3.0)
FLOW_REL_L2 = 4 * 1.005e-6   # worst row measured: (576, 1024)
assert FLOW_MAX_ABS <= 1e-3
REMAP_SHARE = 1e-3           # share of warped bytes that may differ from cv2_shim.remap (by one grey level at most)

STRUCT_MAX_ABS = 4 * 4.005e-4  # px; worst content row measured: mixed
STRUCT_REL_L2 = 4 * 1.333e-5   # worst content row measured: diagonal
assert STRUCT_MAX_ABS <= 2e-3

ROWS = FI.SMALL_ROWS + [FI.LARGE_ROW]
IDS = [f"{h}x{w}_{dx}_{dy}" for (h, w), (dx, dy) in ROWS]


def _gpu_flow(gpu, hw, sh):
    return flow.farneback_flows(torch.from_numpy(FI.pair(hw, sh).copy()).to(gpu))


@pytest.mark.parametrize("hw,sh", ROWS, ids=IDS)
def test_flow_matches_the_shim(gpu, hw, sh):
    got = _gpu_flow(gpu, hw, sh)
    assert got.shape == (1, hw[0], hw[1], 2) and got.dtype == torch.float32 and got.is_cuda
    got = got[0].cpu().numpy().astype(np.float64)
    want = FI.shim_flow(2, hw[0], hw[1], sh[0], sh[1])[0].astype(np.float64)
    e_abs = float(np.abs(got - want).max())
    e_rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"flow {hw} {sh}: max-abs {e_abs:.3e} px (bound {FLOW_MAX_ABS:.1e}), rel-L2 {e_rel:.3e} (bound {FLOW_REL_L2:.1e})")
    assert np.isfinite(got).all()
    assert e_abs <= FLOW_MAX_ABS and e_rel <= FLOW_REL_L2


@pytest.mark.parametrize("name", FI.CONTENT_ROWS + FI.ZERO_ROWS)
def test_content_flow_matches_the_shim(gpu, name):
    """Edges, flat areas and noise: every pixel of the flow against the shim's, and TC against mean |shim flow|."""
    fr = FI.content_clip(name)
    got = flow.farneback_flows(torch.from_numpy(fr.copy()).to(gpu))[0].cpu().numpy().astype(np.float64)
    want = FI.content_shim_flow(name)[0].astype(np.float64)
    assert got.shape == want.shape == FI.CONTENT_HW + (2,)
    e_abs = float(np.abs(got - want).max())
    if name in FI.ZERO_ROWS:
        e_rel = 0.0
        assert float(np.abs(want).max()) < 1e-6                                    # the row is still of the ~0 kind
    else:
        e_rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        assert float(np.abs(want).max()) > 1.0                                     # ... and this one still moves
    print(f"flow {name}: max-abs {e_abs:.3e} px (bound {STRUCT_MAX_ABS:.1e}), rel-L2 {e_rel:.3e} (bound {STRUCT_REL_L2:.1e})")
    assert np.isfinite(got).all()
    assert e_abs <= STRUCT_MAX_ABS and e_rel <= STRUCT_REL_L2
    tc, tc_shim = flow.temporal_consistency(fr, device=gpu), float(np.mean(np.abs(want)))
    # as in test_temporal_consistency_matches_the_cpu_path: every |flow| within STRUCT_MAX_ABS, so is their mean; the fixed
    # order fp32 sum adds at most ~140 roundings on a value's path
    margin = STRUCT_MAX_ABS + 140 * 2.0 ** -24 * tc_shim
    print(f"TC {name}: gpu {tc!r} shim {tc_shim!r}: difference {abs(tc - tc_shim):.3e} (margin {margin:.3e})")
    assert np.isfinite(tc) and abs(tc - tc_shim) <= margin


@pytest.mark.parametrize("name", FI.CONTENT_ROWS + FI.ZERO_ROWS)
def test_content_flow_warp_error_matches_the_host_metric(gpu, name):
    """Four frames, one boundary: frame 1 warped by the flow 1 -> 2 against frame 2, on the GPU and through the shim."""
    fr = FI.content_clip(name, 4)
    ranges = [(0, 2), (2, 4)]
    want = metrics.flow_warp_error(list(fr), ranges)
    got = flow.flow_warp_error(torch.from_numpy(fr.copy()).to(gpu), ranges)
    # the margin of test_flow_warp_error_matches_the_host_metric with this row's flow bound and this frame's largest step
    f1 = fr[1].astype(np.int32)
    G = max(int(np.abs(np.diff(f1, axis=0)).max()), int(np.abs(np.diff(f1, axis=1)).max()))
    margin = REMAP_SHARE * 1.0 + 4 * G * STRUCT_MAX_ABS
    print(f"flow_err {name}: gpu {got!r} host {want!r}: difference {abs(got - want):.3e} (margin {margin:.3e}, G = {G})")
    assert np.isfinite(got) and abs(got - want) <= margin


@pytest.mark.parametrize("hw,sh", FI.SMALL_ROWS, ids=IDS[:-1])
def test_interior_flow_recovers_the_shift(gpu, hw, sh):
    got = _gpu_flow(gpu, hw, sh)[0].cpu().numpy()
    med = np.median(got[10:-10, 10:-10].reshape(-1, 2), axis=0)                   # (24, 40) keeps 4 x 20 pixels
    print(f"interior median {hw} {sh}: ({med[0]:.4f}, {med[1]:.4f})")
    assert abs(med[0] - sh[0]) <= 0.05 and abs(med[1] - sh[1]) <= 0.05


def test_once_per_frame_and_batch_independence(gpu):
    """Five frames: every pair's flow out of the batch is bit-equal to the flow of that pair alone, and to a second run."""
    fr = torch.from_numpy(FI.clip(5, 72, 104, 1.5, -0.75).copy()).to(gpu)
    whole = flow.farneback_flows(fr)
    assert whole.shape == (4, 72, 104, 2)
    assert torch.equal(whole, flow.farneback_flows(fr))
    for i in range(4):
        assert torch.equal(whole[i], flow.farneback_flows(fr[i:i + 2])[0]), i
    host = flow.farneback_flows(FI.clip(5, 72, 104, 1.5, -0.75), device=gpu)       # host frames: the same bits
    assert torch.equal(whole, host)
    assert float((whole[0] - whole[3]).abs().max()) > 0                           # the pairs are not copies of one another
    tc = flow.temporal_consistency(fr)
    assert tc == flow.temporal_consistency(fr) and tc == flow.temporal_consistency(list(FI.clip(5, 72, 104, 1.5, -0.75)), device=gpu)


def test_runtime_levels_and_iterations(gpu):
    """`levels` and `iterations` are run-time integers: each (levels, iterations) matches the shim called with the same."""
    fr = FI.pair((72, 104), (1.5, -0.75))
    grey = [cv2_shim.cvtColor(f, cv2_shim.COLOR_RGB2GRAY) for f in fr]
    for levels, iters in ((1, 1), (2, 4), (5, 2)):                                 # 5 collapses to 3 by the level rule
        want = cv2_shim.calcOpticalFlowFarneback(grey[0], grey[1], None, 0.5, levels, 15, iters, 5, 1.2, 0).astype(np.float64)
        got = flow.farneback_flows(fr, levels, iters, device=gpu)[0].cpu().numpy().astype(np.float64)
        e = float(np.abs(got - want).max())
        print(f"levels {levels}, iterations {iters}: max-abs {e:.3e} px")
        assert e <= FLOW_MAX_ABS


# ---- TC ----------------------------------------------------------------------------------------------------------------
def test_temporal_consistency_matches_the_cpu_path(gpu):
    from vdx.mdvqs import MDVQS
    fr = FI.clip(4, 72, 104, 1.5, -0.75)
    cpu = MDVQS(flow="cpu").compute_temporal_consistency(fr)
    want = float(np.mean([np.mean(np.abs(f)) for f in FI.shim_flow(4, 72, 104, 1.5, -0.75)]))
    assert cpu == want                                                             # the CPU path IS the shim here (no cv2)
    got = flow.temporal_consistency(torch.from_numpy(fr.copy()).to(gpu))
    # Every flow value is within FLOW_MAX_ABS of the shim's, so is every |flow| and so is their mean: relative to TC = mean
    # |flow| that is FLOW_MAX_ABS / TC.  The GPU's fixed-order fp32 sum adds at most ~140 roundings per value's path (72
    # sequential adds per lane at the largest frame, 6 butterfly steps, 3 wave adds, 64 partials): 140 * 2^-24 relative.
    rel = FLOW_MAX_ABS / cpu + 140 * 2.0 ** -24
    print(f"TC gpu {got!r} cpu {cpu!r}: relative difference {abs(got - cpu) / cpu:.3e} (margin {rel:.3e})")
    assert abs(got - cpu) <= rel * cpu
    assert 0.5 < cpu < 1.5                                                         # mean of |1.5| and |-0.75| is 1.125


def test_mdvqs_with_gpu_flow(gpu):
    from vdx.compat.diffusers_shim import HashTokenizer
    from vdx.mdvqs import MDVQS
    fr = FI.clip(4, 72, 104, 1.5, -0.75)
    m = MDVQS.synthetic(seed=0, device=gpu, flow="gpu")
    tc = m.compute_temporal_consistency(fr)
    assert isinstance(tc, float) and tc == flow.temporal_consistency(fr, device=gpu)
    assert tc == m.compute_temporal_consistency(torch.from_numpy(fr.copy()).to(gpu))
    pf, vq, tc2, total = m.compute_md_vqs(fr, "a rocket in space, 4k", tokenizer=HashTokenizer())
    assert tc2 == tc and total == 0.4 * pf + 0.3 * vq + 0.3 * tc
    assert m.compute_temporal_consistency(fr[:1]) == 0.0 and m.compute_temporal_consistency(fr[:0]) == 0.0
    assert MDVQS(flow="gpu").compute_temporal_consistency(fr) == tc               # no models: frames go to "cuda"


# ---- remap and flow_err --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,sh", FI.SMALL_ROWS, ids=IDS[:-1])
def test_remap_kernel_against_the_shims_remap(gpu, hw, sh):
    """The GPU's own flow, downloaded, through `cv2_shim.remap` (metrics.py:61-64) against the GPU's warped frame."""
    fr = FI.pair(hw, sh)
    flows, sums, warped = flow.warp_pairs(fr, [1], device=gpu, want_warped=True)
    assert flows.shape == (1, hw[0], hw[1], 2) and warped.shape == (1, hw[0], hw[1], 3) and warped.dtype == torch.uint8
    fl = flows[0].cpu().numpy()
    mx = (np.arange(hw[1])[None, :] + fl[:, :, 0]).astype(np.float32)
    my = (np.arange(hw[0])[:, None] + fl[:, :, 1]).astype(np.float32)
    want = cv2_shim.remap(fr[0], mx, my, cv2_shim.INTER_LINEAR).astype(np.int32)
    got = warped[0].cpu().numpy().astype(np.int32)
    d = np.abs(got - want)
    print(f"remap {hw} {sh}: {int((d > 0).sum())} of {d.size} bytes differ (share {float((d > 0).mean()):.2e}), largest {int(d.max())}")
    assert d.max() <= 1 and float((d > 0).mean()) <= REMAP_SHARE
    assert int(sums[0]) == int(np.abs(got - fr[1].astype(np.int32)).sum())         # the integer sum is exact
    _f, sums2, none = flow.warp_pairs(fr, [1], device=gpu)
    assert none is None and torch.equal(sums, sums2)


def test_remap_border_is_constant_zero(gpu):
    """A flow that points outside the image: taps there read 0 (cv2.remap's constant border), partly outside taps blend."""
    from vdx import ops
    rng = np.random.default_rng(3)
    fr = rng.integers(0, 256, (2, 16, 24, 3), dtype=np.uint8)
    fl = np.zeros((1, 16, 24, 2), np.float32)
    fl[0, :, :12, 0], fl[0, :, 12:, 0] = -30.25, 7.5
    fl[0, :8, :, 1], fl[0, 8:, :, 1] = -4.75, 9.5
    sums, warped = ops.flow_remap_absdiff(torch.from_numpy(fr).to(gpu), torch.from_numpy(fl).to(gpu), want_warped=True)
    mx = (np.arange(24)[None, :] + fl[0, :, :, 0]).astype(np.float32)
    my = (np.arange(16)[:, None] + fl[0, :, :, 1]).astype(np.float32)
    want = cv2_shim.remap(fr[0], mx, my, cv2_shim.INTER_LINEAR)
    assert (want == 0).mean() > 0.5 and (want != 0).any()
    # quarter / half weights on byte values are exact in fp32; ties (x.5) round half to even in both
    assert np.array_equal(warped[0].cpu().numpy(), want)
    assert int(sums[0]) == int(np.abs(want.astype(np.int32) - fr[1].astype(np.int32)).sum())


def test_flow_warp_error_matches_the_host_metric(gpu):
    fr = FI.clip(6, 72, 104, 1.5, -0.75)
    ranges = [(0, 3), (3, 6)]
    want = metrics.flow_warp_error(list(fr), ranges)
    got = flow.flow_warp_error(torch.from_numpy(fr.copy()).to(gpu), ranges)
    assert got == metrics.flow_warp_error(list(fr), ranges, device=gpu) == flow.flow_warp_error(list(fr), ranges, device=gpu)
    # One boundary: frame 2 warped by the flow 2 -> 3 against frame 3 (metrics.py:58-65), grey by COLOR_BGR2GRAY of the RGB bytes.
    # Margin: (a) the remap kernel may differ from the shim's remap in a share REMAP_SHARE of bytes by one grey level;
    # (b) the flow differs by at most FLOW_MAX_ABS px per component, which moves a bilinearly warped value by at most
    # (|d/dx| + |d/dy|) FLOW_MAX_ABS <= 2 G FLOW_MAX_ABS with G the largest difference of neighbouring bytes of the frame;
    # rounding to uint8 turns a move of m < 1 into a step of 1 for a share m of the bytes: the mean moves by at most
    # another 2 G FLOW_MAX_ABS.
    f2 = fr[2].astype(np.int32)
    G = max(int(np.abs(np.diff(f2, axis=0)).max()), int(np.abs(np.diff(f2, axis=1)).max()))
    margin = REMAP_SHARE * 1.0 + 4 * G * FLOW_MAX_ABS
    print(f"flow_err gpu {got!r} host {want!r}: difference {abs(got - want):.3e} (margin {margin:.3e}, G = {G})")
    assert abs(got - want) <= margin


def test_flow_warp_error_direction_and_boundaries(gpu):
    """Frame e-1 is sampled at x + flow(e-1 -> e) and compared with frame e, grey by COLOR_BGR2GRAY of the RGB bytes
    (metrics.py:58-65), and only the inner chunk ends count."""
    fr = FI.clip(6, 72, 104, 1.5, -0.75)
    flows, sums, warped = flow.warp_pairs(fr, [3], device=gpu, want_warped=True)
    shim = FI.shim_flow(6, 72, 104, 1.5, -0.75, 0, True)[2].astype(np.float64)    # frames 2 -> 3, COLOR_BGR2GRAY
    assert float(np.abs(flows[0].cpu().numpy() - shim).max()) <= FLOW_MAX_ABS
    rgb = FI.shim_flow(6, 72, 104, 1.5, -0.75)[2].astype(np.float64)              # what COLOR_RGB2GRAY would have given
    assert float(np.abs(rgb - shim).max()) > 10 * FLOW_MAX_ABS                    # ... is told apart by the bound above
    w = warped[0].cpu().numpy()
    mx = (np.arange(104)[None, :] + shim[:, :, 0]).astype(np.float32)
    my = (np.arange(72)[:, None] + shim[:, :, 1]).astype(np.float32)
    moved = np.abs(cv2_shim.remap(fr[2], mx, my, cv2_shim.INTER_LINEAR).astype(np.int32) - w.astype(np.int32))
    # frame 2 (not 3) is the one sampled at x + flow; a flow within FLOW_MAX_ABS moves few bytes across a rounding step
    G = max(int(np.abs(np.diff(fr[2].astype(np.int32), axis=0)).max()), int(np.abs(np.diff(fr[2].astype(np.int32), axis=1)).max()))
    assert moved.max() <= 1 and float((moved > 0).mean()) <= REMAP_SHARE + 4 * G * FLOW_MAX_ABS
    assert int(sums[0]) == int(np.abs(w.astype(np.int64) - fr[3].astype(np.int64)).sum())
    three = flow.flow_warp_error(fr, [(4, 6), (0, 2), (2, 4)], device=gpu)         # unsorted: boundaries 2 and 4
    parts = [flow.flow_warp_error(fr, [(0, e), (e, 6)], device=gpu) for e in (2, 4)]
    assert three == float(np.mean(parts))
    assert flow.flow_warp_error(fr, [(0, 6)], device=gpu) is None and flow.flow_warp_error(fr[:1], [(0, 1)], device=gpu) is None
    assert flow.flow_warp_error(np.stack([fr[0]] * 6), [(0, 3), (3, 6)], device=gpu) == 0.0


# ---- pipeline ------------------------------------------------------------------------------------------------------------
BASE = ["--model_id", "synthetic:tiny", "--num_frames", "8", "--steps", "2", "--height", "128", "--width", "256",
        "--chunk_size", "6", "--overlap", "2", "--mode", "chunk", "--out_video", "", "--noise_device", "cpu"]
KEYS = {"pf", "vq", "tc", "total", "weights", "lpips_per_pair", "authentic", "authenticity", "synthetic_weights", "n_frames"}


def test_pipeline_gpu_flow_flag(gpu, tmp_path):
    """`--gpu_flow` puts both numbers on the GPU path and marks the record; without it the record's keys are the old ones."""
    import csv
    from vdx.pipeline import main
    out_csv, js0, js1 = str(tmp_path / "r.csv"), str(tmp_path / "m0.json"), str(tmp_path / "m1.json")
    assert main(BASE + ["--out_csv", out_csv, "--mdvqs_json", js0]) == 0
    assert main(BASE + ["--out_csv", out_csv, "--mdvqs_json", js1, "--gpu_flow"]) == 0
    rec0, rec1 = json.load(open(js0)), json.load(open(js1))
    assert set(rec0) == KEYS and set(rec1) == KEYS | {"flow"} and rec1["flow"] == "gpu"
    assert {k: rec0[k] for k in KEYS - {"tc", "total"}} == {k: rec1[k] for k in KEYS - {"tc", "total"}}
    assert rec1["total"] == 0.4 * rec1["pf"] + 0.3 * rec1["vq"] + 0.3 * rec1["tc"]
    rows = list(csv.DictReader(open(out_csv)))
    assert len(rows) == 2 and rows[0]["flow_err"] != "" and rows[1]["flow_err"] != ""
    for v in (rec0["tc"], rec1["tc"], float(rows[0]["flow_err"]), float(rows[1]["flow_err"])):
        assert np.isfinite(v) and v >= 0.0
    timed = {"timestamp", "latency_s", "throughput_fps", "net_gather_s", "net_reduce_s", "peak_vram_mb", "end_vram_mb", "flow_err"}
    assert {k: v for k, v in rows[0].items() if k not in timed} == {k: v for k, v in rows[1].items() if k not in timed}
