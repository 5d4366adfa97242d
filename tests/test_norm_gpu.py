"""-m gpu: csrc/norm.hip against float64 — the GroupNorm STATISTICS themselves (per-slab (n, mean, M2) triples and the
per-(sample, channel) scale / shift table, read back through `ops.groupnorm_stats`), the apply pass against its own
table, the fold's two claims (`ops.groupnorm_fold`), and LayerNorm at every dispatch — at the partition edges listed in
tests/norm_ref.py (`GN_SHAPES`; tests/test_norm_host.py asserts which edge each shape reaches).

BOUNDS ON THE STATISTICS.  Not taken from the GPU: tests/norm_ref.py `emulate_stats` redoes the statistics pass in float32
in the kernel's order on the CPU, and `stat_errors` measures it against float64 in four figures (definitions there):
pmean (slab means, in standard deviations of the slab), pm2 (slab M2, relative), scale (relative), shift (relative to
sqrt(var + eps) |scale|, net of the rounding of the final fp32 subtraction).  RECORDED below holds, per (shape, regime),
the emulator's own figures rounded up to two digits; `python tests/norm_ref.py --record` prints the table.  pm2, scale
and shift, which are relative, are floored at 2^-24 (one fp32 rounding), so that a case the emulator happens to get
exactly does not demand bits.  pmean has no floor in the table (the emulator gets the slab means of constant groups,
and of the integer-valued large-mean data at power-of-two group sizes, exactly: figure 0); instead every slab mean may
be off by what storing THAT slab's mean in fp32 costs: |err_i| <= GPU_FACTOR max(pmean sd_i, 2^-24 |mean_i|)
(norm_ref.pmean_ratio).  tests/test_norm_host.py asserts the emulator stays inside RECORDED and RECORDED within 12 % of
the emulator; the GPU must stay inside GPU_FACTOR = 8 times RECORDED (FMA contraction and reassociation the emulator
does not model).  Slab counts are compared as integers.  Where the arithmetic is exact by construction (regime e: a
constant group) the triples are compared exactly.

OTHER BOUNDS (derived, fixed):
  apply      |y - (x a + b)| <= 0.5 ulp16 + 2^-22 (|x a| + |b|) with the kernel's OWN (a, b): one fp32 multiply-add, fused
             or not, and one fp16 rounding; with SiLU the comparator of tests/test_activations_gpu.py for silu_f
             (0.5 ulp16 (1 + 2^-8) + 2^-21 |exact|) plus the pre-activation bound times |silu'| <= 1.1.
  fold       w_s bit-equal to fp16(fp32(w) * a); bias_s within (C / 64 + 12) 2^-24 sum(|w beta| + |w16 mean|).
  LayerNorm  0.5 ulp16 + c 2^-24 (|x - mean| rstd |gamma| + |beta|), c = 16 + C / 64; in the large-mean regime plus
             2^-24 |mean| rstd |gamma| (three times that at a row mean of 1, see test_layernorm_against_float64): the
             two-pass form rounds the mean itself to fp32.
             A constant row gives beta exactly.

LayerNorm dispatch, from vdx_layernorm_f16: the row-group kernel takes every C / 8 = LPR * NL with LPR in 8, 16, 32, 64 and
NL <= 5 (64, 320, 640, 1280, 512, 1024, 2048, and also 768 = <32, 3> and 1536 = <64, 3>); the one-row-per-wave kernel
the rest: 96 and 32 (NV 1), 576 (NV 2), 1088 (NV 3) and 1600 (NV 4: C / 8 = 200 is divisible by 8 but 25 > 5 vectors per
lane, so layernorm_kernel<4> IS reachable).

RECORDED: case -> (pmean, pm2, scale, shift), measured on the CPU (numpy float32), see above."""
import numpy as np
import pytest
import torch

import norm_ref as R

pytestmark = pytest.mark.gpu

GPU_FACTOR = 8.0
RECORDED = {
    "1-1-64-0-32-0-a": (0.0e+00, 6.0e-08, 7.4e-08, 6.0e-06),
    "1-1-64-0-32-0-e": (0.0e+00, 6.0e-08, 9.3e-08, 1.3e-04),
    "1-5-320-0-32-0-a": (3.1e-08, 1.6e-07, 1.3e-07, 6.0e-08),
    "1-5-320-0-32-0-d": (0.0e+00, 6.0e-08, 9.3e-08, 2.2e-07),
    "1-5-320-0-32-0-g": (2.8e-08, 2.0e-07, 1.3e-07, 6.0e-08),
    "6-35-64-0-32-0-a": (8.8e-08, 2.0e-07, 1.2e-07, 6.0e-08),
    "6-35-64-0-32-0-c": (7.2e-07, 2.5e-07, 1.3e-07, 1.8e-07),
    "6-35-64-0-32-0-f": (9.6e-08, 2.7e-07, 1.1e-07, 6.0e-08),
    "3-300-320-0-32-0-a": (6.5e-08, 2.4e-07, 8.7e-08, 6.0e-08),
    "3-300-320-0-32-0-b1": (5.6e-05, 1.4e-05, 1.1e-06, 4.0e-04),
    "3-300-320-0-32-0-b2": (6.6e-05, 1.4e-05, 8.7e-07, 3.0e-04),
    "3-300-320-0-32-0-c": (6.9e-06, 2.0e-06, 1.3e-07, 2.2e-07),
    "3-300-320-0-32-0-d": (0.0e+00, 6.0e-08, 9.7e-08, 3.1e-07),
    "3-300-320-0-32-0-e": (0.0e+00, 6.0e-08, 9.8e-08, 3.0e-04),
    "3-300-320-0-32-0-f": (1.2e-07, 2.8e-07, 1.0e-07, 6.0e-08),
    "3-300-320-0-32-0-g": (5.8e-08, 2.6e-07, 8.8e-08, 6.0e-08),
    "1-300-320-0-32-48-a": (3.5e-08, 2.0e-07, 9.8e-08, 6.0e-08),
    "1-300-320-0-32-48-c": (5.1e-06, 7.8e-07, 1.2e-07, 1.7e-07),
    "2-130-64-128-32-0-a": (7.4e-08, 2.4e-07, 8.3e-08, 6.0e-08),
    "2-130-64-128-32-0-d": (0.0e+00, 6.0e-08, 9.3e-08, 2.7e-07),
    "2-130-64-128-32-0-g": (8.6e-08, 2.2e-07, 9.5e-08, 6.0e-08),
    "2-513-1280-640-32-0-a": (2.4e-08, 3.2e-07, 9.8e-08, 6.0e-08),
    "2-513-1280-640-32-0-c": (4.3e-06, 5.6e-07, 9.5e-08, 2.0e-07),
    "2-513-1280-640-32-0-f": (1.6e-06, 4.3e-07, 9.7e-08, 6.0e-08),
    "2-257-2560-0-32-0-a": (2.4e-08, 3.7e-07, 1.3e-07, 6.0e-08),
    "2-257-2560-0-32-0-d": (0.0e+00, 6.0e-08, 8.5e-08, 1.8e-07),
    "2-257-2560-0-32-0-e": (0.0e+00, 6.0e-08, 1.0e-07, 2.8e-04),
    "2-257-2560-0-32-0-g": (2.1e-08, 3.8e-07, 1.1e-07, 6.0e-08),
    "2-40-320-0-1-0-a": (4.1e-09, 2.2e-07, 7.3e-08, 6.0e-08),
    "2-40-320-0-1-0-d": (0.0e+00, 6.0e-08, 6.4e-08, 6.0e-08),
    "2-40-320-0-1-0-g": (4.0e-09, 2.3e-07, 6.5e-08, 6.0e-08),
    "3-1000-2048-0-32-0-a": (2.7e-08, 3.7e-07, 1.1e-07, 6.0e-08),
    "3-1000-2048-0-32-0-b1": (0.0e+00, 2.4e-07, 1.2e-07, 3.9e-05),
    "3-1000-2048-0-32-0-b2": (0.0e+00, 2.4e-07, 1.2e-07, 4.0e-05),
    "3-1000-2048-0-32-0-c": (2.8e-07, 5.0e-07, 8.7e-08, 1.8e-07),
    "3-1000-2048-0-32-0-f": (1.6e-07, 5.1e-07, 9.7e-08, 6.0e-08),
    "2-16389-320-0-32-0-a": (5.3e-08, 3.3e-07, 1.2e-07, 6.0e-08),
    "2-16389-320-0-32-0-b1": (6.8e-05, 1.1e-05, 2.2e-07, 8.3e-05),
    "2-16389-320-0-32-0-b2": (6.3e-05, 1.3e-05, 2.6e-07, 7.5e-05),
    "2-16389-320-0-32-0-c": (2.1e-04, 5.6e-05, 9.0e-08, 1.9e-07),
    "2-16389-320-0-32-0-f": (8.7e-08, 2.1e-06, 1.6e-07, 6.0e-08),
    "1-2049-128-0-32-0-a": (1.3e-07, 2.5e-07, 8.7e-08, 6.0e-08),
    "1-2049-128-0-32-0-c": (2.3e-05, 8.0e-06, 8.0e-08, 1.3e-07),
    "1-8065-64-0-32-0-a": (2.8e-07, 3.6e-07, 6.9e-08, 6.0e-08),
    "1-8065-64-0-32-0-b1": (9.5e-05, 4.2e-05, 3.7e-07, 1.3e-04),
    "1-8065-64-0-32-0-b2": (9.9e-05, 3.7e-05, 6.1e-07, 2.1e-04),
    "1-8065-64-0-32-0-c": (1.6e-04, 9.7e-05, 6.9e-08, 1.6e-07),
    "1-24705-64-0-32-0-a": (2.0e-07, 5.3e-07, 7.6e-08, 6.0e-08),
    "1-24705-64-0-32-0-c": (3.1e-04, 1.7e-04, 9.1e-08, 1.4e-07),
    "1-32897-64-0-32-0-a": (2.1e-07, 6.0e-07, 8.4e-08, 6.0e-08),
    "1-32897-64-0-32-0-b1": (1.2e-04, 1.6e-05, 3.6e-07, 1.3e-04),
    "1-32897-64-0-32-0-b2": (1.1e-04, 1.5e-05, 3.5e-07, 1.1e-04),
    "1-32897-64-0-32-0-c": (2.1e-04, 5.5e-05, 8.9e-08, 1.6e-07),
    "1-32897-64-0-32-0-e": (0.0e+00, 6.0e-08, 9.8e-08, 2.3e-04),
    "1-497-64-0-32-0-a": (2.5e-07, 2.3e-07, 8.6e-08, 6.0e-08),
    "1-497-64-0-32-0-c": (7.1e-06, 2.3e-06, 7.6e-08, 6.0e-08),
    "1-505-64-0-32-0-a": (2.5e-07, 2.4e-07, 9.1e-08, 6.0e-08),
    "1-505-64-0-32-0-c": (6.3e-06, 2.4e-06, 7.2e-08, 7.8e-08),
    "1-1529-64-0-32-0-a": (1.6e-07, 3.0e-07, 9.1e-08, 6.0e-08),
    "1-1529-64-0-32-0-c": (2.9e-05, 1.3e-05, 9.0e-08, 8.5e-08),
    "1-1537-64-0-32-0-a": (1.9e-07, 2.4e-07, 7.1e-08, 6.0e-08),
    "1-1537-64-0-32-0-c": (3.6e-05, 1.2e-05, 8.3e-08, 1.9e-07),
    "2-129-512-0-32-8-a": (2.6e-08, 1.9e-07, 8.9e-08, 6.0e-08),
    "2-129-512-0-32-8-b1": (0.0e+00, 2.4e-06, 2.6e-07, 9.7e-05),
    "2-129-512-0-32-8-b2": (0.0e+00, 2.4e-06, 2.2e-07, 8.0e-05),
    "2-129-512-0-32-8-f": (5.8e-08, 2.0e-07, 9.5e-08, 6.0e-08),
}
RATIOS = {}                     # figure -> (largest GPU error / bound, case): printed at the end of the module
SENTINEL = -1234.0


def _ops():
    import vdx  # noqa: F401
    from vdx import ops
    return ops


def dev16(a, gpu):
    """fp16 numpy array -> device tensor with the same bits."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16).copy()).to(gpu).view(torch.float16).reshape(a.shape)


def host16(t):
    """fp16 tensor -> float64 numpy."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.float16).astype(np.float64).reshape(tuple(t.shape))


def host32(t):
    return t.detach().cpu().contiguous().numpy().copy()


def window(rows, cols, left, right, gpu):
    """A [rows][cols] view into a sentinel-filled buffer `left` + cols + `right` wide -> (buffer, view)."""
    buf = torch.full((rows, left + cols + right), SENTINEL, dtype=torch.float16, device=gpu)
    return buf, buf[:, left:left + cols]


def untouched(buf, left, cols):
    return bool((buf[:, :left] == SENTINEL).all()) and bool((buf[:, left + cols:] == SENTINEL).all())


def note(figure, ratio, case):
    if ratio > RATIOS.get(figure, (-1.0, None))[0]:
        RATIOS[figure] = (ratio, case)


@pytest.fixture(scope="module", autouse=True)
def ratio_table():
    yield
    print("\n==== largest GPU error / bound per figure ====")
    for k in sorted(RATIOS):
        print(f"    {k}: {RATIOS[k][0]:.3f} of its bound at {RATIOS[k][1]}")


def _sources(shape, x, gpu):
    """Device sources of a case: contiguous, except the two-source shape whose sources are views into wider buffers."""
    ns, rps, c1, c2, G, part = shape
    M = ns * rps
    xd = dev16(x.reshape(M, c1 + c2), gpu)
    if not c2:
        return xd, None
    _, x1 = window(M, c1, 8, 16, gpu)
    _, x2 = window(M, c2, 16, 8, gpu)
    x1.copy_(xd[:, :c1])
    x2.copy_(xd[:, c1:])
    return x1, x2


def _stats(ops, shape, x1, x2, gamma, beta, **kw):
    ns, rps, c1, c2, G, part = shape
    ab, partial = ops.groupnorm_stats(x1, gamma, beta, groups=G, n_samples=ns, rows_per_sample=rps, eps=R.GN_EPS, x2=x2,
                                      partition_samples=part, **kw)
    return host32(ab), host32(partial)


def apply_bound(xa, b, ref):
    d = 2.0 ** -22 * (np.abs(xa) + np.abs(b))
    return 0.5 * R.ulp16(np.abs(ref) + d) + d, d


# ---- GroupNorm: triples, table, apply, run to run ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,regime", R.GN_CASES, ids=[R.case_id(s, r) for s, r in R.GN_CASES])
def test_groupnorm_statistics_and_apply(gpu, shape, regime):
    ops = _ops()
    ns, rps, c1, c2, G, part = shape
    C, M, case = c1 + c2, ns * rps, R.case_id(shape, regime)
    x, gamma, beta = R.gn_inputs(shape, regime)
    x1, x2 = _sources(shape, x, gpu)
    gd, bd = dev16(gamma, gpu), dev16(beta, gpu)
    sr = R.stat_rows(ns, rps, part)
    ab, partial = _stats(ops, shape, x1, x2, gd, bd)
    assert partial.shape == (ns, R.nslabs(ns, rps, part), G, 3) and ab.shape == (ns, C, 2)
    # 6. run to run, in a workspace of the test's own
    ws = torch.full((R.workspace_bytes(ns, rps, C, G, part),), 0xA5, dtype=torch.uint8, device=gpu)
    ab2, partial2 = _stats(ops, shape, x1, x2, gd, bd, workspace=ws)
    assert ab.tobytes() == ab2.tobytes() and partial.tobytes() == partial2.tobytes(), "two launches differ in their bits"
    # 1. + 2. triples and table against float64 (counts exactly: inside stat_errors)
    got = dict(n=partial[..., 0], mean=partial[..., 1], m2=partial[..., 2], scale=ab[..., 0], shift=ab[..., 1])
    assert np.isfinite(partial).all() and np.isfinite(ab).all()
    err = R.stat_errors(got, x, gamma, beta, G, R.GN_EPS, sr)
    line = []
    ratios = {}
    for fig, rec in zip(R.FIGURES, RECORDED[case]):
        ratios[fig] = R.pmean_ratio(err, rec, GPU_FACTOR) if fig == "pmean" else err[fig] / (GPU_FACTOR * rec)
        note(fig, ratios[fig], case)
        line.append(f"{fig} {err[fig]:.3g} / {GPU_FACTOR * rec:.3g} ({ratios[fig]:.3f})")
    print(f"{case}: " + ", ".join(line))
    for fig, rec in zip(R.FIGURES, RECORDED[case]):
        assert ratios[fig] <= 1.0, f"{case}: {fig} {err[fig]:.4g} is {ratios[fig]:.3f} of {GPU_FACTOR:g} x {rec:.3g} (pmean: slab by slab)"
    x64 = x.astype(np.float64)
    if regime == "e":               # every operation is exact: mean = the constant, M2 = 0, scale = gamma / sqrt(eps)
        assert np.array_equal(got["m2"], np.zeros_like(got["m2"]))
        assert np.array_equal(got["mean"].astype(np.float64), np.broadcast_to(x64[:, :1, ::C // G], got["mean"].shape))
        want = (gamma.astype(np.float64) / np.sqrt(R.eps64(R.GN_EPS))).astype(np.float32)
        assert (np.abs(got["scale"] - want[None, :]) <= 2 * np.spacing(np.abs(want))[None, :]).all()
    # 3. apply against the kernel's own table, every element
    a, b = ab[..., 0].astype(np.float64)[:, None, :], ab[..., 1].astype(np.float64)[:, None, :]
    xa = x64 * a
    pre = (xa + b).reshape(M, C)
    bound, d = apply_bound(xa, b, xa + b)
    for silu in (False, True) if regime in "agf" else (False,):
        strided = c2 != 0
        buf, out = window(M, C, 8 if strided else 0, 8 if strided else 0, gpu)
        ops.groupnorm(x1, gd, bd, groups=G, n_samples=ns, rows_per_sample=rps, eps=R.GN_EPS, silu_act=silu, x2=x2, out=out,
                      partition_samples=part)
        y = host16(out)
        assert untouched(buf, 8 if strided else 0, C), "the apply pass wrote outside its columns"
        if silu:
            ref = R.silu64(pre)
            d1 = 1.1 * d.reshape(M, C)
            bnd = 0.5 * R.ulp16(np.abs(ref) + d1) * (1 + 2.0 ** -8) + 2.0 ** -21 * np.abs(ref) + d1
        else:
            ref, bnd = pre, bound.reshape(M, C)
        e = np.abs(y - ref)
        assert np.isfinite(y).all()
        worst = float((e / bnd).max())
        note("apply+silu" if silu else "apply", worst, case)
        assert worst <= 1.0, f"{case}: silu={silu}: {int((e > bnd).sum())} of {e.size} outside, worst {worst:.3f} of the bound at row {int(np.argmax((e / bnd).max(axis=1)))}"


# ---- 4. marker rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rps,C,part", [(16389, 320, 2), (1000, 2048, 3)])
def test_marker_rows(gpu, rps, C, part):
    """One launch, sample i all zero but for row markers[i] = 8.0: every group of every sample must come out with
    mean 8 / rps and var 64 (1 / rps)(1 - 1 / rps).  A row dropped or read twice moves the mean by 100 %; the tolerance,
    2^-18 relative, is sixty-four fp32 roundings and more than the few dozen operations on these exact inputs can spend."""
    ops = _ops()
    rows = R.marker_rows(rps, C, part)
    ns, G, tol = len(rows), 32, 2.0 ** -18
    assert R.stat_rows(part, rps) == R.stat_rows(ns, rps, part) and ns >= 8
    x = torch.zeros((ns, rps, C), dtype=torch.float16, device=gpu)
    for i, r in enumerate(rows):
        x[i, r] = 8.0
    one, zero = torch.ones(C, dtype=torch.float16, device=gpu), torch.zeros(C, dtype=torch.float16, device=gpu)
    ab, partial = ops.groupnorm_stats(x.view(ns * rps, C), one, zero, groups=G, n_samples=ns, rows_per_sample=rps, eps=R.GN_EPS,
                                      partition_samples=part)
    ab, partial = host32(ab).astype(np.float64), host32(partial).astype(np.float64)
    mean, var = 8.0 / rps, 64.0 * (1.0 / rps) * (1.0 - 1.0 / rps)
    scale = 1.0 / np.sqrt(var + R.eps64(R.GN_EPS))
    for i, r in enumerate(rows):
        assert np.abs(ab[i, :, 0] - scale).max() <= tol * scale, f"marker row {r}: scale {ab[i, 0, 0]} for {scale}"
        assert np.abs(ab[i, :, 1] + mean * scale).max() <= tol * mean * scale, f"marker row {r}: shift {ab[i, 0, 1]} for {-mean * scale}"
    sr = R.stat_rows(part, rps)
    for i, r in enumerate(rows):
        s = r // sr
        n = min(rps, (s + 1) * sr) - s * sr
        others = np.delete(partial[i], s, axis=0)
        assert np.array_equal(others[..., 1:], np.zeros_like(others[..., 1:])), f"marker row {r} shows in another slab"
        assert np.abs(partial[i, s, :, 1] - 8.0 / n).max() <= tol * 8.0 / n, f"marker row {r}: slab mean"
        m2 = 64.0 * (C // G) * (1.0 - 1.0 / n)
        assert np.abs(partial[i, s, :, 2] - m2).max() <= tol * m2, f"marker row {r}: slab M2"


# ---- 5. partition_samples ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,rps,C,part", [(4, 300, 320, 48), (4, 129, 512, 8), (2, 16389, 320, 2), (4, 35, 64, 6)])
def test_partition_samples_pins_the_bits(gpu, ns, rps, C, part):
    """The table and the triples of sample s are bit-identical whether it is computed alone, in half the batch or in the
    whole batch under the same partition_samples; against partition_samples = 0 they are identical wherever the restated
    geometry gives the same slab size, and otherwise the slab count differs as restated."""
    ops = _ops()
    G = 32
    x, gamma, beta = R.gn_inputs((ns, rps, C, 0, G, part), "a")
    xd, gd, bd = dev16(x.reshape(ns * rps, C), gpu), dev16(gamma, gpu), dev16(beta, gpu)

    def run(s0, n, p):
        ab, partial = ops.groupnorm_stats(xd[s0 * rps:(s0 + n) * rps], gd, bd, groups=G, n_samples=n, rows_per_sample=rps,
                                          eps=R.GN_EPS, partition_samples=p)
        return host32(ab), host32(partial)

    whole_ab, whole_p = run(0, ns, part)
    assert whole_p.shape[1] == R.nslabs(ns, rps, part)
    for s in range(ns):
        ab1, p1 = run(s, 1, part)
        assert ab1[0].tobytes() == whole_ab[s].tobytes() and p1[0].tobytes() == whole_p[s].tobytes(), f"sample {s} alone"
    half = ns // 2
    for s0 in (0, half):
        abh, ph = run(s0, half, part)
        assert abh.tobytes() == whole_ab[s0:s0 + half].tobytes() and ph.tobytes() == whole_p[s0:s0 + half].tobytes()
    for s0, n in ((0, ns), (0, 1), (half, half)):
        ab0, p0 = run(s0, n, 0)
        if R.stat_rows(n, rps) == R.stat_rows(n, rps, part):
            assert ab0.tobytes() == whole_ab[s0:s0 + n].tobytes() and p0.tobytes() == whole_p[s0:s0 + n].tobytes()
        else:
            assert p0.shape[1] == R.nslabs(n, rps) != whole_p.shape[1]


@pytest.mark.parametrize("rps", [20, 32])
def test_groupnorm_stats_one_sample_one_group(gpu, rps):
    """n_samples = G = 1: a slab is three floats, so the table's offset (rounded up to 4 floats) is the same for 3 and
    for 4 slabs — rps 20 and 32 at slab 8.  `groupnorm_stats` must hand back the slab count of the geometry; bounds as
    for every case, from the emulator run here."""
    ops = _ops()
    shape, C = (1, rps, 64, 0, 1, 0), 64
    assert R.nslabs(1, rps) == {20: 3, 32: 4}[rps] and R.round_up4(3 * 3) == R.round_up4(3 * 4)
    x, gamma, beta = R.gn_inputs(shape, "a")
    ab, partial = _stats(ops, shape, dev16(x.reshape(rps, C), gpu), None, dev16(gamma, gpu), dev16(beta, gpu))
    assert partial.shape == (1, R.nslabs(1, rps), 1, 3) and ab.shape == (1, C, 2)
    got = dict(n=partial[..., 0], mean=partial[..., 1], m2=partial[..., 2], scale=ab[..., 0], shift=ab[..., 1])
    err = R.stat_errors(got, x, gamma, beta, 1, R.GN_EPS, 8)                       # counts exactly, inside
    emu = R.emulator_figures(shape, "a")
    for fig in R.FIGURES:
        rec = R.round_up2(max(emu[fig], R.FIGURE_FLOORS[fig]))
        ratio = R.pmean_ratio(err, rec, GPU_FACTOR) if fig == "pmean" else err[fig] / (GPU_FACTOR * rec)
        assert ratio <= 1.0, f"rps {rps}: {fig} {err[fig]:.4g} is {ratio:.3f} of {GPU_FACTOR:g} x {rec:.3g}"


# ---- the fold -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", R.FOLD_REGIMES)
@pytest.mark.parametrize("fshape", R.FOLD_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_groupnorm_fold(gpu, fshape, regime):
    ops = _ops()
    C, N, ns, rps = fshape
    G, case = 32, "fold-" + "-".join(map(str, fshape)) + "-" + regime
    x, gamma, beta, w, bias = R.fold_inputs(fshape, regime)
    xd, gd, bd, wd, biasd = (dev16(v, gpu) for v in (x.reshape(ns * rps, C), gamma, beta, w, bias))
    ws = torch.zeros((R.workspace_bytes(ns, rps, C, G),), dtype=torch.uint8, device=gpu)
    w_s, b_s = ops.groupnorm_fold(xd, gd, bd, wd, biasd, groups=G, n_samples=ns, rows_per_sample=rps, eps=R.FOLD_EPS, workspace=ws)
    off = R.workspace_bytes(ns, rps, C, G) // 4 - ns * C * 2
    ab = host32(ws.view(torch.float32)[off:].view(ns, C, 2))                       # the table this very launch left
    ab_again, _ = ops.groupnorm_stats(xd, gd, bd, groups=G, n_samples=ns, rows_per_sample=rps, eps=R.FOLD_EPS)
    assert ab.tobytes() == host32(ab_again).tobytes()
    a = ab[..., 0]
    got_w = w_s.detach().cpu().view(torch.int16).numpy().view(np.float16).reshape(ns, N, C)
    want_w = (w.astype(np.float32)[None, :, :] * a[:, None, :]).astype(np.float16)
    assert got_w.tobytes() == want_w.tobytes(), f"{case}: {int((got_w.view(np.int16) != want_w.view(np.int16)).sum())} weights differ from fp16(w * a)"
    zero = gamma == 0
    if regime == "g":
        assert zero.sum() >= 2 and not got_w[:, :, zero].any()
    mean_c = R.ref_table(x, gamma, beta, G, R.FOLD_EPS)[2]
    ref_b, mag = R.ref_fold(w, bias, beta, got_w, mean_c)
    bound = (C / 64 + 12) * 2.0 ** -24 * mag
    e = np.abs(host32(b_s).astype(np.float64) - ref_b)
    note("fold bias", float((e / bound).max()), case)
    assert (e <= bound).all(), f"{case}: bias_s worst {float((e / bound).max()):.3f} of its bound"


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------
LN_CASES = [(M, C) for C in R.LN_WIDTHS for M in R.ln_rows(C)] + R.LN_BIG


@pytest.mark.parametrize("M,C", LN_CASES)
def test_layernorm_against_float64(gpu, M, C):
    """Strided rows and output (views into wider sentinel-filled buffers), all four regimes per shape (the two large row
    counts: regime a and the constant rows).  The bound is in the module docstring; the large-mean term
    2^-24 |mean| rstd |gamma| is added in the large-mean regime: the two-pass form rounds the mean to fp32.  Regimes a and
    g (a row mean of about 0.06) get the bound without it.  Regime "mid" (a row mean of 1, at 3 standard deviations) gets
    three times the term: the fp32 mean is fl(fl(sum) fl(1 / C)), three roundings of a number of the mean's size (the
    last addition of the sum, the constant, the product), and where |x - mean| rstd and |beta| are both near 0 the rest
    of the slack is smaller than one of them, so that an output within it of an fp16 tie may not land on either side."""
    ops = _ops()
    c = 16 + C / 64
    failures = []
    for regime in (R.LN_REGIMES if M < 1000 else ["a", "mid", "const"]):
        x, gamma, beta = R.ln_inputs(M, C, regime)
        _, xv = window(M, C, 8, 8, gpu)
        xv.copy_(dev16(x, gpu))
        buf, out = window(M, C, 16, 8, gpu)
        ops.layernorm(xv, dev16(gamma, gpu), dev16(beta, gpu), M=M, eps=R.LN_EPS, out=out)
        y = host16(out)
        assert untouched(buf, 16, C), "layernorm wrote outside its columns"
        assert np.isfinite(y).all()
        ref, mean, rstd = R.ref_layernorm(x, gamma, beta, R.LN_EPS)
        g64, b64 = np.abs(gamma.astype(np.float64)), beta.astype(np.float64)
        if regime == "const":
            if not np.array_equal(y, np.broadcast_to(b64, y.shape)):
                failures.append(f"M={M} C={C}: a constant row must give beta exactly")
            continue
        slack = c * 2.0 ** -24 * (np.abs(x.astype(np.float64) - mean) * rstd * g64 + np.abs(b64))
        if regime in ("mean", "mid"):
            slack = slack + (3.0 if regime == "mid" else 1.0) * 2.0 ** -24 * np.abs(mean) * rstd * g64
        bound = 0.5 * R.ulp16(np.abs(ref) + slack) + slack
        e = np.abs(y - ref)
        worst = float((e / bound).max())
        note(f"layernorm {regime}", worst, f"M={M} C={C}")
        print(f"layernorm M={M} C={C} {regime}: {int((e > bound).sum())} of {e.size} outside, worst {worst:.3f} of the bound")
        if worst > 1.0:
            failures.append(f"M={M} C={C} {regime}: {int((e > bound).sum())} of {e.size} outside, worst {worst:.3f} of the bound")
    assert not failures, "; ".join(failures)
