"""GPU tests of the temporal filter (vdx/deflicker.py, vdx.ops.deflicker_frames, csrc/deflicker.hip): the kernel against the
float64 restatement (tests/deflicker_ref.py) on seeded synthetic flows, its exact properties, its effect, and `filter_frames`
on the real Farneback flows."""
import numpy as np
import pytest
import torch

import deflicker_ref as R
import interp_inputs as I

pytestmark = pytest.mark.gpu

# (F, H, W).  The kernel's tile is 32 x 16: (33, 65) and (17, 33) cross a tile edge by one pixel on both axes, (16, 40) fills
# one tile row exactly, (1, 1) and (5, 7) are all halo.
SHAPES = [(1, 4, 4), (2, 1, 1), (2, 5, 7), (3, 33, 65), (4, 16, 40), (2, 17, 33)]
PARAMS = [(lam, sig) for lam in (0.25, 1.0) for sig in (2.0, 10.0)]
# Parity bound: at most one grey level anywhere, in at most a share of a case's bytes.  profiles/deflicker_parity.txt has the
# shares measured on the MI355X against the float64 restatement, per shape the worst over strength, sigma and loop; the bound is
# 4x that, capped at 1e-3 (the margin convention of profiles/flow_parity.txt).  A difference is a value within fp32 rounding of
# x.5: the kernel is one fixed sequence of IEEE operations, so the cases stay what was measured.
MEASURED_SHARE = {(1, 4, 4): 0.0, (2, 1, 1): 0.0, (2, 5, 7): 0.0, (3, 33, 65): 5.18e-5,(4, 16, 40): 0.0, (2, 17, 33): 0.0}
SHARE_CAP = 1e-3


def case(shape, loop, seed=0):
    """Seeded frames and flows uniform in +-3 px -> (frames uint8, fab, fba fp32 (F - 1 + loop, H, W, 2))."""
    F, H, W = shape
    rng = np.random.default_rng([seed, F, H, W])
    frames = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    fab, fba = (rng.uniform(-3, 3, (F - 1 + loop, H, W, 2)).astype(np.float32) for _ in range(2))
    return frames, fab, fba


def run(gpu, frames, fab, fba, lam, sig, loop=False):
    from vdx import ops
    return ops.deflicker_frames(*(torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (frames, fab, fba)), lam, sig, loop=loop)


@pytest.mark.parametrize("loop", [False, True], ids=["open", "loop"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_float64_restatement(gpu, shape, loop):
    frames, fab, fba = case(shape, loop)
    worst = 0.0
    for lam, sig in PARAMS:
        got = run(gpu, frames, fab, fba, lam, sig, loop).cpu().numpy()
        d = np.abs(got.astype(np.int16) - R.deflicker_pass(frames, fab, fba, lam, sig, loop).astype(np.int16))
        share = float(np.count_nonzero(d)) / d.size
        print(f"parity {shape} loop={int(loop)} strength={lam} sigma={sig}: max |d| {int(d.max())}, {int(np.count_nonzero(d))} of {d.size} bytes differ (share {share:.2e})")
        assert d.max() <= 1
        worst = max(worst, share)
    assert worst <= min(4 * MEASURED_SHARE[shape], SHARE_CAP)


def test_non_finite_and_huge_flows_stay_in_their_patch(gpu):
    shape = (3, 33, 65)
    frames, fab, fba = case(shape, False, seed=1)
    rng = np.random.default_rng(7)
    for fl in (fab, fba):
        for v in (np.nan, np.inf, -np.inf, 1e4, -1e4):
            p, y, x, c = (rng.integers(0, n, 12) for n in fl.shape)
            fl[p, y, x, c] = v
    got = run(gpu, frames, fab, fba, 1.0, 10.0).cpu().numpy()
    torch.cuda.synchronize()                                            # a clean run
    want = R.deflicker_pass(frames, fab, fba, 1.0, 10.0)

    def wild(fl):                                                       # (H, W): a pixel with a wild entry in its 3 x 3 patch
        bad = np.pad(~(np.abs(fl) < 1e3).all(-1), 1)
        return sum(bad[dy:dy + shape[1], dx:dx + shape[2]] for dy in range(3) for dx in range(3)) > 0
    none = np.zeros(shape[1:], bool)
    clean = np.stack([~((wild(fba[t - 1]) if t > 0 else none) | (wild(fab[t]) if t < 2 else none)) for t in range(3)])
    assert clean.mean() > 0.5
    assert np.abs(got.astype(np.int16) - want.astype(np.int16))[clean].max() <= 1


def test_exact_cases(gpu):
    from vdx import ops
    frames, fab, fba = case((5, 17, 33), True)                          # five flows each: the loop's; the open clip uses four
    f, ab, ba = (torch.from_numpy(a).to(gpu) for a in (frames, fab, fba))
    # identical frames, zero flows: the bytes; one frame: the bytes
    same = f[:1].expand(3, -1, -1, -1).contiguous()
    zero = torch.zeros((3, 17, 33, 2), device=gpu)
    for lam in (0.25, 0.5, 1.0):
        assert torch.equal(ops.deflicker_frames(same, zero, zero, lam, 10.0, loop=True), same)
        assert torch.equal(ops.deflicker_frames(same, zero[:2], zero[:2], lam, 10.0), same)
    assert torch.equal(ops.deflicker_frames(f[:1], ab[:0], ba[:0], 1.0, 2.0), f[:1])
    # frame t depends on frames t-1, t, t+1 alone, and on nothing else in the batch; run to run
    full = ops.deflicker_frames(f, ab[:4], ba[:4], 0.5, 10.0)
    sub = ops.deflicker_frames(f[1:].contiguous(), ab[1:4].contiguous(), ba[1:4].contiguous(), 0.5, 10.0)
    assert torch.equal(sub[1:-1], full[2:-1]) and not torch.equal(sub[0], full[1])
    assert torch.equal(ops.deflicker_frames(f, ab[:4], ba[:4], 0.5, 10.0), full)
    # the loop has no first frame: rotating the clip and its flows rotates the result
    ring = ops.deflicker_frames(f, ab, ba, 0.5, 10.0, loop=True)
    rolled = ops.deflicker_frames(*(torch.roll(t, 2, 0) for t in (f, ab, ba)), 0.5, 10.0, loop=True)
    assert torch.equal(rolled, torch.roll(ring, 2, 0)) and not torch.equal(ring[0], full[0])
    # out may not be the input: the kernel refuses instead of reading what it has written
    with pytest.raises(ops.VdxError, match="overlaps"):
        ops.deflicker_frames(f, ab[:4], ba[:4], 0.5, 10.0, out=f)


def test_effect_on_a_translating_texture_with_flickering_brightness(gpu):
    from vdx import deflicker
    F, H, W, (dx, dy) = 6, 48, 64, (2, 1)
    clean = np.stack([I.crop(H, W, -dx * t, -dy * t, seed=5) for t in range(F)]).astype(np.int16) * 7 // 8 + 16   # 16..239: no clipping
    noisy = (clean + np.array([6, -6] * 3, np.int16)[:, None, None, None]).astype(np.uint8)
    flow = torch.tensor([dx, dy], dtype=torch.float32, device=gpu).expand(F - 1, H, W, 2).contiguous()
    f = torch.from_numpy(noisy).to(gpu)
    mae = [float(np.abs(noisy.astype(np.int16) - clean).mean())]
    for passes in (1, 2):
        out = deflicker.run_passes(f, flow, -flow, 1.0, 10.0, passes).cpu().numpy()
        mae.append(float(np.abs(out.astype(np.int16) - clean).mean()))
    print(f"effect: MAE against the clean clip {mae[0]:.3f} (input), {mae[1]:.3f} (1 pass), {mae[2]:.3f} (2 passes)")
    assert mae[0] == 6.0 and mae[2] < mae[1] < mae[0]


@pytest.mark.parametrize("loop", [False, True], ids=["open", "loop"])
def test_filter_frames_on_the_real_flows(gpu, loop):
    from vdx import deflicker, flow
    frames = np.stack([I.crop(64, 96, -i, -i, seed=3) for i in range(4)])
    f = torch.from_numpy(frames).to(gpu)
    out = deflicker.filter_frames(f, 0.5, 10.0, passes=2, loop=loop)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape == f.shape and not torch.equal(out, f)
    ext = torch.cat([f, f[:1]]) if loop else f                          # the flows `interpolate_frames` computes
    fab, fba = flow.farneback_flows(ext), flow.farneback_flows(ext.flip(0)).flip(0).contiguous()
    assert torch.equal(out, two_passes(f, fab, fba, loop))
    assert torch.equal(deflicker.filter_frames(list(frames), 0.5, 10.0, passes=2, device=gpu, loop=loop), out)     # host frames
    assert deflicker.filter_frames(f[:1], loop=loop).data_ptr() == f.data_ptr()                                      # one frame: the input


def two_passes(f, fab, fba, loop):
    from vdx import ops
    return ops.deflicker_frames(ops.deflicker_frames(f, fab, fba, 0.5, 10.0, loop=loop), fab, fba, 0.5, 10.0, loop=loop)
