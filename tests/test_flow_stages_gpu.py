"""Every stage of the GPU Farneback flow (csrc/flow.hip through vdx/ops.py) on its own against its float64 definition in
`vdx.compat.cv2_shim` / scipy, at the sizes where a kernel goes wrong: extents smaller than a halo (the mirror wraps more than
once), one tile and one more than a tile, pitched frames, more than 64 pairs, displacements that clamp on every border,
non-finite flows.  Each stage is fed what its reference is fed (the GPU's upstream output, downloaded), so errors do not
compound.  Integer stages are compared for equality; floating-point bounds are derived in each test's docstring from the
arithmetic the kernel uses: a number of roundings times the unit roundoff (u32 = 2^-24, u64 = 2^-53) times the sum of the
absolute terms, first order, never read off the kernel's output."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import vdx  # noqa: F401
from vdx import flow, ops
from vdx.compat import cv2_shim

pytestmark = pytest.mark.gpu

U32, U64 = 2.0 ** -24, 2.0 ** -53


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _host(t):
    return t.cpu().numpy()


def _pitched(frames, gpu):
    """The frames as a view of a wider, longer buffer of another value: row pitch 3 (W + 5), frame pitch (H + 3) rows."""
    F, H, W, _ = frames.shape
    big = torch.full((F + 1, H + 3, W + 5, 3), 0xA5, dtype=torch.uint8, device=gpu)
    big[:F, :H, :W] = _dev(frames, gpu)
    view = big[:F, :H, :W]
    assert not view.is_contiguous() or H * W == 1
    return view


# ---- grey ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(5, 7), (1, 1)])
def test_grey_equals_cvtcolor(gpu, hw):
    """Integers: (4899 R + 9617 G + 1868 B + 8192) >> 14 fits in 32 bits and is exact in fp32; equality, both channel orders,
    packed and pitched."""
    rng = np.random.default_rng(11)
    fr = rng.integers(0, 256, (10,) + hw + (3,), dtype=np.uint8)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    fr[:8, 0, 0] = corners                                                         # the eight corner triples, one per frame
    for bgr, code in ((False, cv2_shim.COLOR_RGB2GRAY), (True, cv2_shim.COLOR_BGR2GRAY)):
        want = np.stack([cv2_shim.cvtColor(f, code) for f in fr]).astype(np.float32)
        for frames in (_dev(fr, gpu), _pitched(fr, gpu)):
            got = ops.flow_grey(frames, bgr=bgr)
            assert got.shape == (10,) + hw and got.dtype == torch.float32
            assert np.array_equal(_host(got), want), (bgr, frames.stride())
    assert set(want[:8, 0, 0]) >= {0.0, 255.0}


# ---- corr1d --------------------------------------------------------------------------------------------------------------
def test_corr1d_against_scipy_mirror(gpu):
    """fp32: acc = 0; acc += t_k v_k for the n = 2 r + 1 taps in order.  The first product and every later product and addition
    round once (a fused multiply-add rounds less), so the term entered first passes n roundings: |error| <= ((1 + u32)^n - 1) S
    <= (n + 1) u32 S for n <= 29, with S = sum |t_k| |v_k| = correlate1d(|img|, |taps|).  The float64 reference's own n u64 S is
    below the slack of that (n + 1).  Radius 14 on an extent of 2, 3 or 5 wraps the mirror several times; extent 1 repeats
    its only sample."""
    rng = np.random.default_rng(12)
    for (H, W) in ((1, 9), (9, 1), (2, 5), (5, 3), (16, 70)):
        img = rng.uniform(-255, 255, (2, H, W)).astype(np.float32)
        for sigma, radius in ((0.5, 0), (0.5, 2), (1.5, 6), (3.5, 14)):
            taps = flow.gaussian_taps(sigma, radius).astype(np.float32)
            n = 2 * radius + 1
            for axis in (0, 1):
                got = _host(ops.flow_corr1d(_dev(img, gpu), _dev(taps, gpu), axis)).astype(np.float64)
                want = ndimage.correlate1d(img.astype(np.float64), taps.astype(np.float64), axis=axis + 1, mode="mirror")
                S = ndimage.correlate1d(np.abs(img).astype(np.float64), np.abs(taps).astype(np.float64), axis=axis + 1, mode="mirror")
                excess = np.abs(got - want) - (n + 1) * U32 * S
                assert excess.max() <= 0, (H, W, radius, axis, float(np.abs(got - want).max()))
                if radius == 0:
                    assert np.array_equal(got, img)                                # one tap of 1: a copy


# ---- resize --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2])
def test_resize_against_resize_linear(gpu, C):
    """fp32: out = ((a wx0 + b wx1) wy0 + (c wx0 + d wx1) wy1) mul with wx1 = fx, wx0 = 1 - fx.  The source position is exact
    integer arithmetic; fx is one rounded division and 1 - fx one more rounding, so each of wx0, wx1, wy0, wy1 is off by at
    most 2 u32 absolutely, and the four tap weights wx wy together by 2 u32 (sum wy + sum wx) = 8 u32.  The arithmetic adds at
    most 6 roundings on a tap's path (product, sum, product, sum, mul, and one spare for an unfused multiply-add), relative to
    sum w |v| <= M, the largest |input|.  |error| <= (8 + 6) u32 M |mul|; 16 is asserted.  The reference's float64 coordinate
    error (~1e-13 M) is inside the slack.  Same size in and out: fx = fy = 0 exactly, so the output is the input times mul, bit for bit."""
    rng = np.random.default_rng(13)
    for (Hi, Wi), (Ho, Wo), mul in (((97, 131), (48, 66), 1.0), ((48, 66), (97, 131), 2.0), ((16, 26), (36, 52), 2.0),
                                    ((1, 1), (4, 4), 1.0), ((5, 1), (3, 7), 1.0)):
        x = rng.uniform(-255, 255, (2, Hi, Wi) + ((2,) if C == 2 else ())).astype(np.float32)
        got = _host(ops.flow_resize(_dev(x, gpu), Ho, Wo, mul=mul)).astype(np.float64)
        want = np.stack([cv2_shim._resize_linear(i.astype(np.float64), Wo, Ho) * mul for i in x])
        assert got.shape == want.shape == (2, Ho, Wo) + x.shape[3:]
        bound = 16 * U32 * float(np.abs(x).max()) * abs(mul)
        e = float(np.abs(got - want).max())
        assert e <= bound, ((Hi, Wi), (Ho, Wo), e, bound)
        if (Hi, Wi) == (1, 1):
            assert np.array_equal(got, np.broadcast_to(x.astype(np.float64), got.shape) * mul)
    x = _dev(rng.uniform(-255, 255, (2, 17, 23) + ((2,) if C == 2 else ())).astype(np.float32), gpu)
    for mul in (1.0, 2.0):
        assert torch.equal(ops.flow_resize(x, 17, 23, mul=mul), x * mul)


# ---- polyexp -------------------------------------------------------------------------------------------------------------
def _polyexp_reference(img):
    """`_poly_exp` of a float64 image -> planes (5, H, W), and A (5, H, W): for plane j the sum of the absolute terms of its
    evaluation, sum_q |ig[j][q]| (|ky_q| x |kx_q| correlated with |img|)."""
    want = np.stack(cv2_shim._poly_exp(img, 5, 1.2))
    (k0, k1, k2), ig = (np.abs(t) for t in flow.poly_tables())
    a = np.abs(img)

    def sep(ky, kx):
        return ndimage.correlate1d(ndimage.correlate1d(a, kx, axis=1, mode="mirror"), ky, axis=0, mode="mirror")

    m = np.stack([sep(k0, k0), sep(k0, k1), sep(k1, k0), sep(k0, k2), sep(k2, k0), sep(k1, k1)])      # 1, x, y, xx, yy, xy
    return want, np.einsum("jq,qhw->jhw", ig, m)


def _check_polyexp(gpu, imgs):
    got = _host(ops.flow_polyexp(_dev(imgs, gpu), *flow.poly_tables())).astype(np.float64)
    assert got.shape == (imgs.shape[0], 5) + imgs.shape[1:]
    for g, img in zip(got, imgs):
        want, A = _polyexp_reference(img.astype(np.float64))
        excess = np.abs(g - want) - (U32 * np.abs(want) + 2 * 30 * U64 * A)
        assert excess.max() <= 0, (imgs.shape, float(np.abs(g - want).max()))
    return got


@pytest.mark.parametrize("hw", [(16, 64), (17, 65), (2, 2), (3, 11), (6, 5), (40, 130)])
def test_polyexp_against_poly_exp(gpu, hw):
    """fp64 arithmetic on the fp32 image with float64 tables: a term passes at most 11 roundings in the column pass, 11 in the row
    pass and 6 in the product with inv(G) (a product and a sum per tap, fewer when fused: at most 28; 30 is used), relative to
    A = the sum of the absolute terms (`_polyexp_reference`); the float64 reference, which sums in another order, may be as far
    from the exact value: 2 x 30 u64 A.  The result is rounded once to fp32: u32 |r|.  fp32 sums would miss this bound by
    five orders of magnitude.  Sizes: one 16 x 64 tile, one more in both directions, extents below the halo of 5 (the mirror
    wraps up to five times), several tiles.  Contents: uniform 0..255, and an impulse in each corner."""
    H, W = hw
    rng = np.random.default_rng(14)
    imgs = np.zeros((6, H, W), np.float32)
    imgs[:2] = rng.uniform(0, 255, (2, H, W))
    for i, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        imgs[2 + i, y, x] = 255.0
    got = _check_polyexp(gpu, imgs)
    assert float(np.abs(got[0] - got[1]).max()) > 1e-3                             # the images are not read as one


def test_polyexp_of_a_constant_image_is_zero(gpu):
    """No gradient, no curvature: all five planes are 0 within the bound above (here 60 u64 A ~ 1e-11 against |img| = 128; an fp32
    evaluation leaves ~1e-5)."""
    got = _check_polyexp(gpu, np.full((1, 19, 70), 128.0, np.float32))
    assert float(np.abs(got).max()) <= 1e-10


# ---- update --------------------------------------------------------------------------------------------------------------
N_UPDATE = 56


def _update_reference(R0, R1, fl):
    """`_update_flow(R0, R1, fl, 15, False)` in float64 -> (new flow (H, W, 2), its first-order error bound (H, W, 2)) for an
    evaluation in which every term passes at most N_UPDATE roundings of u64 and the result is rounded once to fp32.
    Capitals are the sums of absolute terms of the lower-case quantities (`_sample` of |plane|: the weights are >= 0)."""
    H, W = fl.shape[:2]
    want = cv2_shim._update_flow(tuple(R0), tuple(R1), fl, 15, False)
    gx, gy = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    xs, ys = gx + fl[..., 0], gy + fl[..., 1]
    s1 = [cv2_shim._sample(c, xs, ys) for c in R1]
    S1 = [cv2_shim._sample(np.abs(c), xs, ys) for c in R1]
    r0, A0 = R0, np.abs(R0)
    a11, a22, a12 = 0.5 * (r0[2] + s1[2]), 0.5 * (r0[3] + s1[3]), 0.25 * (r0[4] + s1[4])
    A11, A22, A12 = 0.5 * (A0[2] + S1[2]), 0.5 * (A0[3] + S1[3]), 0.25 * (A0[4] + S1[4])
    dx, dy = fl[..., 0], fl[..., 1]
    dbx = -0.5 * (s1[0] - r0[0]) + a11 * dx + a12 * dy
    dby = -0.5 * (s1[1] - r0[1]) + a12 * dx + a22 * dy
    DBX = 0.5 * (S1[0] + A0[0]) + A11 * np.abs(dx) + A12 * np.abs(dy)
    DBY = 0.5 * (S1[1] + A0[1]) + A12 * np.abs(dx) + A22 * np.abs(dy)
    box = lambda c: ndimage.uniform_filter(c, 15, mode="mirror")   # noqa: E731
    g = [box(c) for c in (a11 * a11 + a12 * a12, a11 * a12 + a12 * a22, a12 * a12 + a22 * a22, a11 * dbx + a12 * dby,
                          a12 * dbx + a22 * dby)]
    G = [box(c) for c in (A11 * A11 + A12 * A12, A11 * A12 + A12 * A22, A12 * A12 + A22 * A22, A11 * DBX + A12 * DBY,
                          A12 * DBX + A22 * DBY)]
    det = g[0] * g[2] - g[1] * g[1] + 1e-3
    e = N_UPDATE * U64
    d_det = 2 * e * (G[0] * G[2] + G[1] * G[1])
    d_nx = 2 * e * (G[2] * G[3] + G[1] * G[4])
    d_ny = 2 * e * (G[0] * G[4] + G[1] * G[3])
    bound = np.stack([(d_nx + np.abs(want[..., 0]) * d_det) / np.abs(det), (d_ny + np.abs(want[..., 1]) * d_det) / np.abs(det)], -1)
    return want, 2 * bound + U32 * np.abs(want)


def _expansions(gpu, n, H, W, seed):
    rng = np.random.default_rng(seed)
    R = ops.flow_polyexp(_dev(rng.uniform(0, 255, (n, H, W)).astype(np.float32), gpu), *flow.poly_tables())
    return R, _host(R).astype(np.float64)


def _flows_for(P, H, W, rng):
    """name -> fp32 (P, H, W, 2): zero; uniform +-3; uniform +-40 (clamps on every border); exactly onto column W-1 and row H-1."""
    y, x = np.mgrid[:H, :W]
    last = np.broadcast_to(np.stack([W - 1 - x, H - 1 - y], -1), (P, H, W, 2))
    return {"zero": np.zeros((P, H, W, 2), np.float32), "pm3": rng.uniform(-3, 3, (P, H, W, 2)).astype(np.float32),
            "pm40": rng.uniform(-40, 40, (P, H, W, 2)).astype(np.float32), "last": last.astype(np.float32)}


@pytest.mark.parametrize("hw", [(2, 2), (5, 9), (32, 32), (33, 33), (46, 47), (16, 26)])
def test_update_against_update_flow(gpu, hw):
    """fp64 arithmetic on fp32 planes.  Roundings on a term's path to a window mean g: the sample (coordinate, fraction and
    1 - fraction, two products and a sum per axis: 8), A = (A0 + A1) / 2 (1; the halving is exact), db (5), the product
    A^T A or A^T db (3), 14 additions and a division per box pass (30): 47.  Then numerator and determinant (3 and 4) and the
    quotient (1): N_UPDATE = 56 covers every path.  First order, with capitals the sums of absolute terms: |d g_q| <= N u64 G_q,
    |d (g_a g_b)| <= 2 N u64 G_a G_b, so |d num_x| <= 2 N u64 (G2 G3 + G1 G4), |d det| <= 2 N u64 (G0 G2 + G1^2) and
    |d flow_x| <= (|d num_x| + |flow_x| |d det|) / |det|, likewise y (`_update_reference`).  The float64 reference sums in
    another order and may be as far from the exact value: twice that; the stored flow is rounded once: + u32 |flow|.
    Sizes: below the halo of 7 (the mirror wraps up to four times), one 32 x 32 tile, one more, the staged 46 x 46 extent,
    a level size of the plan.  step 1: 3 pairs from 4 expansions; step 2: 3 pairs from 6.  Every expansion differs, so a wrong
    R0 / R1 index shows."""
    H, W = hw
    rng = np.random.default_rng(15)
    for step, n in ((1, 4), (2, 6)):
        R, Rh = _expansions(gpu, n, H, W, 150 + step)
        for name, fl in _flows_for(3, H, W, rng).items():
            got = _host(ops.flow_update(R, _dev(fl, gpu), step=step)).astype(np.float64)
            assert np.isfinite(got).all()
            for p in range(3):
                want, bound = _update_reference(Rh[p * step], Rh[p * step + 1], fl[p].astype(np.float64))
                excess = np.abs(got[p] - want) - bound
                assert excess.max() <= 0, (hw, step, name, p, float(np.abs(got[p] - want).max()), float(bound.max()))
            assert float(np.abs(got[0] - got[1]).max()) > 0 and float(np.abs(got[1] - got[2]).max()) > 0


def test_update_contains_non_finite_flows(gpu):
    """NaN, +inf and -inf in a few input flow pixels: their sampling position clamps into the image, their products poison only
    the windows that hold them.  Every output pixel whose window holds none of them (more than 7 px away in x or in y; a
    mirrored window reaches no farther than a direct one) meets the bound of the test above against the reference run with those
    pixels' flow set to 0 (it cannot read them), and the next launch is fine."""
    H, W = 46, 47
    rng = np.random.default_rng(16)
    R, Rh = _expansions(gpu, 2, H, W, 160)
    clean = rng.uniform(-3, 3, (1, H, W, 2)).astype(np.float32)
    bad = [((5, 6), (np.nan, 1.0)), ((20, 40), (np.inf, np.nan)), ((40, 10), (-np.inf, np.inf)), ((45, 46), (0.5, -np.inf))]
    fl, far = clean.copy(), np.ones((H, W), bool)
    y, x = np.mgrid[:H, :W]
    for (by, bx), v in bad:
        fl[0, by, bx], clean[0, by, bx] = v, 0.0
        far &= (np.abs(y - by) > 7) | (np.abs(x - bx) > 7)                        # the 15 x 15 window does not hold it
    assert far.sum() > 1000
    got = _host(ops.flow_update(R, _dev(fl, gpu))).astype(np.float64)[0]
    want, bound = _update_reference(Rh[0], Rh[1], clean[0].astype(np.float64))
    assert np.isfinite(got[far]).all() and not np.isfinite(got).all()
    assert (np.abs(got - want)[far] - bound[far]).max() <= 0
    again = _host(ops.flow_update(R, _dev(clean, gpu))).astype(np.float64)[0]      # the device goes on
    assert (np.abs(again - want) - bound).max() <= 0


# ---- abs_sum -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 65, 130])
def test_abs_sum_against_a_float64_sum(gpu, P):
    """fp32, fixed order: a value is added into its lane's sum (ceil(chunk / 256) = 1 addition at these sizes), passes 6
    butterfly steps, at most 3 additions of wave sums and at most 64 of block partials: 74 roundings relative to sum |x|.
    P = 65 and 130 reach the second and third block of the final kernel; n = 126 and 270 are no multiples of the 64 chunks.
    A pair's sum is bit-equal alone and inside the batch."""
    rng = np.random.default_rng(17)
    for (H, W) in ((1, 1), (3, 21), (9, 15)):
        fl = rng.uniform(-8, 8, (P, H, W, 2)).astype(np.float32)
        d = _dev(fl, gpu)
        got = ops.flow_abs_sum(d)
        assert got.shape == (P,) and got.dtype == torch.float32
        want = np.abs(fl.astype(np.float64)).reshape(P, -1).sum(1)
        assert (np.abs(_host(got).astype(np.float64) - want) - 74 * U32 * want).max() <= 0, (P, H, W)
        for p in sorted({0, P // 2, min(63, P - 1), min(64, P - 1), P - 1}):
            assert torch.equal(ops.flow_abs_sum(d[p:p + 1].contiguous())[0], got[p]), (P, H, W, p)


# ---- remap ---------------------------------------------------------------------------------------------------------------
def test_remap_edges_pitch_and_non_finite_flows(gpu):
    """Flows that are multiples of 1/4: the weights are multiples of 1/16 and every product and sum of byte values is exact in
    fp32, ties round half to even in both, so the bytes equal `cv2_shim.remap`'s and the integer sums are exact.  Map
    coordinates in (-1, 0) and (W-1, W), likewise y: one tap inside, one on the constant-0 border.  NaN, +-inf and +-2e9
    give 0 (the shim is handed 2e9 for the non-finite ones: it cannot read them).  step 2 with 3 pairs, packed and pitched."""
    H, W, P = 9, 13, 3
    rng = np.random.default_rng(18)
    fr = rng.integers(0, 256, (2 * P, H, W, 3), dtype=np.uint8)
    fl = (rng.integers(-12, 13, (P, H, W, 2)) * 0.25).astype(np.float32)
    fl[:, :, 0, 0], fl[:, :, W - 1, 0] = -0.5, 0.25                                # x in (-1, 0) and (W-1, W)
    fl[:, 0, :, 1], fl[:, H - 1, :, 1] = -0.75, 0.5
    special = [((4, 3), (np.nan, 0.0)), ((4, 5), (0.0, np.inf)), ((4, 7), (-np.inf, 1.0)), ((5, 3), (2e9, 0.0)), ((5, 5), (0.25, -2e9)),
               ((5, 7), (np.nan, np.nan))]
    shim_fl = fl.copy()
    for (y, x), v in special:
        fl[:, y, x] = v
        shim_fl[:, y, x] = 2e9
    want = np.empty((P, H, W, 3), np.uint8)
    for p in range(P):
        mx = (np.arange(W)[None, :] + shim_fl[p, :, :, 0]).astype(np.float32)
        my = (np.arange(H)[:, None] + shim_fl[p, :, :, 1]).astype(np.float32)
        want[p] = cv2_shim.remap(fr[2 * p], mx, my, cv2_shim.INTER_LINEAR)
    for (y, x), _v in special:
        assert (want[:, y, x] == 0).all()
    assert (want[:, :, 0] != 0).any() and (want[:, 1:-1, 1:-1] != 0).mean() > 0.5
    sums_want = np.abs(want.astype(np.int64) - fr[1::2].astype(np.int64)).reshape(P, -1).sum(1)
    for frames in (_dev(fr, gpu), _pitched(fr, gpu)):
        sums, warped = ops.flow_remap_absdiff(frames, _dev(fl, gpu), step=2, want_warped=True)
        assert np.array_equal(_host(warped), want), frames.stride()
        assert np.array_equal(_host(sums), sums_want)
        assert torch.equal(ops.flow_remap_absdiff(frames, _dev(fl, gpu), step=2)[0], sums)
