"""The activation comparator of tests/test_activations_gpu.py, float32 emulations of the library's approximate
nonlinearities, and canaries that prove the comparator rejects the mistakes it exists for.  No GPU is needed here.

The comparator (`compare`): input x exactly as the kernel sees it, multiplier c, exact = c * f(x) in float64,

    |got - exact| <= 0.5 * ulp16(exact) * (1 + 2^-8)  +  2^-21 * |exact|  +  |c| * |x| * eps_site

ulp16(v) is the fp16 spacing at v, floored at the subnormal spacing 2^-24.  The first term is the one fp16 rounding every
site performs, the second an fp32 evaluation built from a handful of <= 1-ulp fp32 operations, eps_site the approximation
error of Phi that the site's own header documents (0 for SiLU / QuickGELU / exp).  An exact value beyond 65504 must come
out as inf of the right sign; as fp16 rounds to inf from 65520 on, an exact value between 65504 and 65520 plus the last two
terms may come out either way (3 * 21840 * Phi is such a tie: a Phi of 1 - 1e-7 decides it).

The emulations mirror csrc/vdx_common.h (`erf_fast`, `gelu_tab_init`, `gelu_tab`), csrc/ff_fused.hip (`gelu_poly`) and
csrc/conv_fused.hip (`silu8`) operation for operation in float32; a fused multiply-add is formed in float64 and rounded once.
They predict, they do not measure: the measured envelopes are in the docstring of tests/test_activations_gpu.py."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

F32 = np.float32
SQRT1_2 = 0.70710678118654752
PHI_M45 = 3.4e-6                      # Phi(-4.5), rounded up (3.398e-6)

# eps_site: what each header documents for its approximation of Phi
EPS_ERF_FAST = 0.75e-7                # erf_fast: |erf error| <= 1.5e-7, Phi = (1 + erf) / 2
EPS_GELU_TAB = 3e-6 + 0.75e-7         # linear interpolation of a table that erf_fast fills
EPS_GELU_POLY = 2.1e-5                # on the clamp interval and the right tail (the header said 2e-5; measured 2.01e-5)
EPS_GELU_POLY_LEFT_TAIL = PHI_M45 + EPS_GELU_POLY     # x < -4.5: Phi stays at the polynomial's Phi(-4.5) while the exact one goes to 0


def eps_gelu_poly(x):
    """eps_site of K8's polynomial as a function of the gate."""
    return np.where(np.asarray(x, dtype=np.float64) < -4.5, EPS_GELU_POLY_LEFT_TAIL, EPS_GELU_POLY)


# ---- inputs -------------------------------------------------------------------------------------------------------------
def all_fp16_bits():
    return np.arange(65536, dtype=np.uint32).astype(np.uint16)


def finite_fp16():
    """All 63 488 finite fp16 values (both zeros, all subnormals), in bit-pattern order."""
    b = all_fp16_bits()
    return b[(b & 0x7C00) != 0x7C00].view(np.float16)


def coverage_fp16():
    """The coverage rule of the sites that take few values per launch: every fp16 value with |x| <= 8, every 16th bit
    pattern beyond, and the largest finite values of both signs."""
    v = finite_fp16()
    bits = v.view(np.uint16)
    keep = (np.abs(v.astype(np.float64)) <= 8.0) | (bits % 16 == 0) | ((bits & 0x7FFF) == 0x7BFF)
    return v[keep]


def k8_fp32_grid():
    """fp32 gate values finer than fp16: 64 fp32 steps either side of both clamp points of `gelu_poly`, and around 0 in
    steps of 2^-27 (an eighth of the smallest fp16 subnormal) plus the 64 smallest fp32 values of both signs."""
    out = []
    for centre in (4.5, -4.5):
        b = np.array([centre], dtype=F32).view(np.int32)[0]
        out.append((b + np.arange(-64, 65, dtype=np.int32)).astype(np.int32).view(F32))
    k = np.arange(-64, 65, dtype=np.float64)
    out.append((k * 2.0 ** -27).astype(F32))
    tiny = np.arange(1, 65, dtype=np.int32).view(F32)
    out += [tiny, -tiny]
    return np.concatenate(out)


# ---- exact functions (float64) ------------------------------------------------------------------------------------------
_erfc = np.frompyfunc(math.erfc, 1, 1)


def phi64(x):
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * _erfc(-x * math.sqrt(0.5)).astype(np.float64)


def gelu64(x):
    x = np.asarray(x, dtype=np.float64)
    return x * phi64(x)


def _sigmoid_mul64(x, k):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-k * x))


def silu64(x):
    return _sigmoid_mul64(x, 1.0)


def quick_gelu64(x):
    return _sigmoid_mul64(x, 1.702)


# ---- the comparator -----------------------------------------------------------------------------------------------------
def ulp16(v):
    """fp16 spacing at v (float64), floored at the subnormal spacing 2^-24; 32 from 32768 up."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return np.exp2(np.minimum(e, 15.0) - 10.0)


class Envelope:
    """Worst figures of one site: `eps` = the largest (err - rounding terms) / (|c| |x|), what eps_site has to cover; `ulps`
    = the largest error in fp16 ulps of the exact value; each with the input where it occurred."""

    def __init__(self, site, claimed):
        self.site, self.claimed = site, claimed
        self.eps, self.eps_x, self.ulps, self.ulps_x, self.n = 0.0, None, 0.0, None, 0

    def merge(self, o):
        if o.eps > self.eps or self.eps_x is None:
            self.eps, self.eps_x = o.eps, o.eps_x
        if o.ulps > self.ulps or self.ulps_x is None:
            self.ulps, self.ulps_x = o.ulps, o.ulps_x
        self.n += o.n
        return self

    def row(self):
        return (f"{self.site:<44s} claimed {self.claimed:<9.3g} needed {self.eps:<9.3g} at x = {self.eps_x!r:<22}"
                f" worst {self.ulps:.3f} ulp at x = {self.ulps_x!r}  ({self.n} values)")


def compare(site, x, got, exact, c=1.0, eps_site=0.0):
    """Checks every element; -> Envelope.  x: inputs as the kernel saw them; got: the kernel's fp16 outputs; exact = c * f(x)
    in float64; c and eps_site scalars or arrays.  Nothing is masked out: an exact value beyond 65504 must be inf of its sign,
    every other output finite and inside the bound."""
    x = np.asarray(x, dtype=np.float64).ravel()
    got = np.asarray(got, dtype=np.float64).ravel()
    exact = np.asarray(exact, dtype=np.float64).ravel()
    c = np.broadcast_to(np.asarray(c, dtype=np.float64), x.shape)
    eps_arr = np.broadcast_to(np.asarray(eps_site, dtype=np.float64), x.shape)
    assert x.shape == got.shape == exact.shape and x.size > 0, (site, x.shape, got.shape, exact.shape)
    assert np.isfinite(x).all() and np.isfinite(exact).all(), f"{site}: the comparator takes finite inputs"
    u = ulp16(exact)
    rounding = 0.5 * u * (1.0 + 2.0 ** -8) + 2.0 ** -21 * np.abs(exact)
    cx = np.abs(c) * np.abs(x)
    bound = rounding + cx * eps_arr
    slack = 2.0 ** -21 * np.abs(exact) + cx * eps_arr
    over = (np.abs(exact) > 65504.0) & (np.abs(exact) - slack >= 65520.0)       # must be inf
    either = (np.abs(exact) > 65504.0) & ~over                                   # the tie region of the last finite value
    with np.errstate(invalid="ignore"):
        err = np.abs(got - exact)
    ok_over = np.isinf(got) & (np.sign(got) == np.sign(exact))
    ok_in = np.isfinite(got) & (err <= bound)
    ok = np.where(over, ok_over, np.where(either, ok_over | ok_in, ok_in))
    err_f = np.where(over | ~np.isfinite(got), 0.0, err)
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.where(cx > 0, np.maximum(err_f - rounding, 0.0) / cx, 0.0)
    ulps = err_f / u
    env = Envelope(site, float(np.max(eps_arr)))
    i, j = int(np.argmax(need)), int(np.argmax(ulps))
    env.eps, env.eps_x, env.ulps, env.ulps_x, env.n = float(need[i]), float(x[i]), float(ulps[j]), float(x[j]), x.size
    if not ok.all():
        bad = np.flatnonzero(~ok)
        excess = np.where(over, np.inf, err / bound)[bad]
        worst = bad[np.argsort(-np.nan_to_num(excess, nan=np.inf, posinf=np.inf))[:10]]
        lines = [f"  x = {float(x[k])!r}  c = {float(c[k])!r}  got = {float(got[k])!r}  exact = {float(exact[k])!r}  error = "
                 f"{(err[k] / u[k]) if np.isfinite(got[k]) else float('nan'):.3f} ulp  bound = {bound[k] / u[k]:.3f} ulp"
                 for k in worst]
        raise AssertionError(f"{site}: {bad.size} of {x.size} outputs outside the bound; the worst:\n" + "\n".join(lines))
    return env


# ---- float32 emulations of the device functions ---------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(F32)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _mul(a, b):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64)).astype(F32)


def _exp2(a):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(np.asarray(a, np.float64)).astype(F32)


def _rcp(a):
    with np.errstate(divide="ignore"):
        return (1.0 / np.asarray(a, np.float64)).astype(F32)


def emu_erf_fast(x):
    x = _f32(x)
    ax = np.abs(x)
    t = _rcp(_fma(F32(0.3275911), ax, F32(1.0)))
    p = F32(1.061405429)
    p = _fma(p, t, F32(-1.453152027))
    p = _fma(p, t, F32(1.421413741))
    p = _fma(p, t, F32(-0.284496736))
    p = _fma(p, t, F32(0.254829592))
    e = _exp2(_mul(_mul(F32(-1.44269504088896341), ax), ax))
    r = _fma(-_mul(p, t), e, F32(1.0))
    return np.copysign(r, x)


def emu_gelu_erf(x):
    """gelu_erf_f: 0.5f * x * (1.0f + erf_fast(x * 0.70710678f))."""
    x = _f32(x)
    e = emu_erf_fast(_mul(x, F32(SQRT1_2)))
    return _mul(_mul(F32(0.5), x), (F32(1.0) + e).astype(F32))


GELU_TAB_N = 1024


def emu_gelu_tab_init(zero_left_end=True):
    """-> (p0, dp): gelu_tab_init's table.  `zero_left_end`: cell 0 starts at Phi = 0 (so the clamped index gives 0 * x)."""
    h = F32(10.0) / F32(GELU_TAB_N)
    i = np.arange(GELU_TAB_N, dtype=np.float64)
    x0 = _fma(_f32(i), h, F32(-5.0))
    p0 = _fma(F32(0.5), emu_erf_fast(_mul(x0, F32(SQRT1_2))), F32(0.5))
    p1 = _fma(F32(0.5), emu_erf_fast(_mul((x0 + h).astype(F32), F32(SQRT1_2))), F32(0.5))
    if zero_left_end:
        p0 = p0.copy()
        p0[0] = F32(0.0)
    return p0, (p1 - p0).astype(F32)


def emu_gelu_tab(x, tab):
    x = _f32(x)
    p0, dp = tab
    u = _fma(x, F32(GELU_TAB_N / 10.0), F32(GELU_TAB_N / 2.0))
    u = np.minimum(np.maximum(u, F32(0.0)), F32(GELU_TAB_N - 0.001))
    fi = np.floor(u)
    k = fi.astype(np.int64)
    return _mul(x, _fma((u - fi).astype(F32), dp[k], p0[k]))


K8_COEFFS = (3.988662064e-01, -6.624013931e-02, 9.729332291e-03, -1.076692832e-03, 8.726890519e-05, -4.958988029e-06,
             1.845751427e-07, -4.001098564e-09, 3.804222562e-11)


def emu_gelu_poly(x, coeffs=K8_COEFFS):
    x = _f32(x)
    xc = np.clip(x, F32(-4.5), F32(4.5))
    u = _mul(xc, xc)
    p = F32(coeffs[8])
    for k in range(7, -1, -1):
        p = _fma(p, u, F32(coeffs[k]))
    return _mul(x, _fma(xc, p, F32(0.5)))


def emu_silu8(y, log2e=-1.44269504088896341):
    """K1 / K3: y * rcp(1 + exp2(-log2(e) * y))."""
    y = _f32(y)
    d = (_exp2(_mul(y, F32(log2e))) + F32(1.0)).astype(F32)
    return _mul(y, _rcp(d))


def emu_silu_f(x):
    """silu_f: x / (1 + __expf(-x)), __expf(v) = exp2(v * log2 e)."""
    x = _f32(x)
    d = (_exp2(_mul(-x, F32(1.44269504088896341))) + F32(1.0)).astype(F32)
    with np.errstate(invalid="ignore"):
        return (x.astype(np.float64) / d.astype(np.float64)).astype(F32)


def to16(a):
    """One fp16 rounding (round to nearest even; overflow gives inf), back as float64."""
    with np.errstate(over="ignore"):
        return np.asarray(a).astype(np.float16).astype(np.float64)


# ---- tests: the comparator's own pieces ----------------------------------------------------------------------------------
def test_input_sets():
    v = finite_fp16()
    assert v.size == 63488 and np.isfinite(v.astype(np.float64)).all()
    bits = set(v.view(np.uint16).tolist())
    assert {0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x7BFF, 0xFBFF} <= bits
    cov = coverage_fp16()
    cb = set(cov.view(np.uint16).tolist())
    assert {b for b in bits if (b & 0x7FFF) <= 0x4800} <= cb and {0x7BFF, 0xFBFF, 0x7BF0, 0x4810} <= cb
    assert cov.size == 2 * (0x4801 + (0x7C00 - 0x4810) // 16 + 1)


def test_ulp16_is_the_fp16_spacing():
    v = finite_fp16().astype(np.float64)
    pos = np.sort(v[v > 0])
    gap = np.diff(pos)
    assert np.array_equal(ulp16(pos[:-1]), gap)
    assert ulp16(0.0) == 2.0 ** -24 and ulp16(65504.0) == 32.0 and ulp16(-1.0) == 2.0 ** -10 and ulp16(1e-9) == 2.0 ** -24


def test_comparator_accepts_correct_rounding_and_overflow_to_inf():
    x = finite_fp16().astype(np.float64)
    for c in (1.0, -1.0, 0.37109375, 3.0, 1024.0):
        exact = c * gelu64(x)
        env = compare("rounded exact", x, to16(exact), exact, c, 0.0)
        assert env.ulps <= 0.5 and env.eps == 0.0
    exact = 1024.0 * gelu64(x)
    got = to16(exact)
    assert np.isinf(got).sum() > 1000
    # an overflow that saturates instead of giving inf, an inf of the wrong sign, a NaN: each is rejected
    for wrong in (np.where(np.isinf(got), np.sign(got) * 65504.0, got), np.where(np.isinf(got), -got, got),
                  np.where(np.isinf(got), np.nan, got)):
        with pytest.raises(AssertionError, match="outside the bound"):
            compare("overflow", x, wrong, exact, 1024.0, 0.0)


def test_comparator_rejects_one_ulp_and_reports_the_input():
    x = finite_fp16().astype(np.float64)
    exact = silu64(x)
    got = to16(exact)
    k = int(np.flatnonzero(x == 3.0)[0])
    got[k] += ulp16(exact[k])
    with pytest.raises(AssertionError) as e:
        compare("silu one ulp off", x, got, exact)
    assert "silu one ulp off" in str(e.value) and "x = 3.0" in str(e.value) and "1 of 63488" in str(e.value)


# ---- tests: torch's own fp32 functions pass with eps_site = 0 -------------------------------------------------------------
def test_torch_silu_passes_without_allowance_and_torch_gelu_at_the_table_allowance():
    v = finite_fp16()
    x = v.astype(np.float64)
    xt = torch.from_numpy(v.astype(np.float32))
    compare("torch F.silu fp32", x, F.silu(xt).half().double().numpy(), silu64(x), 1.0, 0.0)
    compare("torch F.gelu fp64", x, F.gelu(xt.double()).half().double().numpy(), gelu64(x), 1.0, 0.0)
    # torch's fp32 erf GELU does NOT pass without an allowance: its erf is 3.5e-7 off near -2.8 (x = -3.98: 5.8 fp16 ulps,
    # Phi 1.75e-7 off), more than `erf_fast` claims.  It is a correct erf GELU all the same, so it passes at the table's.
    env = compare("torch F.gelu fp32", x, F.gelu(xt).half().double().numpy(), gelu64(x), 1.0, EPS_GELU_TAB)
    assert env.eps < 2.5e-7


# ---- tests: the canaries ---------------------------------------------------------------------------------------------------
def test_canary_tanh_gelu_is_rejected_at_every_gelu_site():
    v = finite_fp16()
    x = v.astype(np.float64)
    got = F.gelu(torch.from_numpy(v.astype(np.float32)), approximate="tanh").half().double().numpy()
    for eps in (EPS_ERF_FAST, EPS_GELU_TAB, eps_gelu_poly(x)):
        with pytest.raises(AssertionError, match="outside the bound"):
            compare("tanh GELU", x, got, gelu64(x), 1.0, eps)


def test_emulated_erf_fast_gelu_passes_its_claim():
    x = finite_fp16().astype(np.float64)
    env = compare("emulated gelu_erf_f", x, to16(emu_gelu_erf(x)), gelu64(x), 1.0, EPS_ERF_FAST)
    print(env.row())


def test_emulated_gelu_tab_passes_and_a_perturbed_cell_is_rejected():
    x = finite_fp16().astype(np.float64)
    tab = emu_gelu_tab_init()
    for c in (1.0, -1.0, 0.37109375, 3.0, 1024.0):
        env = compare("emulated gelu_tab", x, to16(_mul(F32(c), emu_gelu_tab(x, tab))), c * gelu64(x), c, EPS_GELU_TAB)
    print(env.row())
    # the clamped index of the left tail gives exactly 0 * x
    left = x[x < -5.0]
    assert np.all(emu_gelu_tab(left, tab) == 0.0)
    # (cells of the positive side are no canaries: 1e-5 of an output near x is below the fp16 spacing there, 4.9e-4 x)
    for cell in (0, 100, 300, 511, 512):
        p0, dp = (a.copy() for a in tab)
        p0[cell] += F32(1e-5)
        with pytest.raises(AssertionError, match="outside the bound"):
            compare(f"gelu_tab, cell {cell} + 1e-5", x, to16(emu_gelu_tab(x, (p0, dp))), gelu64(x), 1.0, EPS_GELU_TAB)


def test_emulated_gelu_tab_left_tail_before_the_zero_cell():
    """With Phi(-5) ~ 3e-7 as the left end of cell 0 the left tail is 3e-7 * |x| away from the exact -0: inside the
    documented 3e-6 (the comparator accepts it), but never 0; with Phi = 0 stored there it is exact."""
    x = finite_fp16().astype(np.float64)
    old = emu_gelu_tab_init(zero_left_end=False)
    compare("emulated gelu_tab, Phi(-5) in cell 0", x, to16(emu_gelu_tab(x, old)), gelu64(x), 1.0, EPS_GELU_TAB)
    left = x[x < -5.0]
    env = compare("emulated gelu_tab, Phi(-5) in cell 0, left tail", left, to16(emu_gelu_tab(left, old)), gelu64(left), 1.0, EPS_GELU_TAB)
    assert 2e-7 < env.eps < 4e-7
    assert to16(emu_gelu_tab(np.array([-65504.0]), old))[0] < -0.015


def test_emulated_gelu_poly_passes_and_a_coefficient_typo_is_rejected():
    g = coverage_fp16().astype(np.float64)
    grid = k8_fp32_grid().astype(np.float64)
    x = np.concatenate([g, grid])
    env = compare("emulated gelu_poly", x, to16(emu_gelu_poly(x)), gelu64(x), 1.0, eps_gelu_poly(x))
    print(env.row())
    typo = list(K8_COEFFS)
    typo[3] = -1.077692832e-03                      # C3 off in its 4th digit
    with pytest.raises(AssertionError, match="outside the bound"):
        compare("gelu_poly, C3 typo", x, to16(emu_gelu_poly(x, typo)), gelu64(x), 1.0, eps_gelu_poly(x))
    # the left tail needs its linear bound: against the interval's 2e-5 alone it is rejected only where the polynomial's
    # Phi(-4.5) exceeds it, so check the tail bound is the one in force
    tail = x[x < -4.5]
    env_t = compare("emulated gelu_poly, left tail", tail, to16(emu_gelu_poly(tail)), gelu64(tail), 1.0, EPS_GELU_POLY_LEFT_TAIL)
    assert env_t.eps <= EPS_GELU_POLY_LEFT_TAIL


def test_canary_silu_with_a_short_exp2_constant_is_rejected():
    x = finite_fp16().astype(np.float64)
    compare("emulated silu8", x, to16(emu_silu8(x)), silu64(x))
    compare("emulated silu_f", x, to16(emu_silu_f(x)), silu64(x))
    with pytest.raises(AssertionError, match="outside the bound"):
        compare("silu8, log2(e) = 1.4427", x, to16(emu_silu8(x, -1.4427)), silu64(x))


def test_k8_fp32_grid():
    g = k8_fp32_grid()
    assert g.dtype == F32 and g.size == 129 * 3 + 128
    assert (g > F32(4.5)).sum() == 64 and ((g < F32(4.5)) & (g > 4.4)).sum() == 64 and (g < F32(-4.5)).sum() == 64
    assert np.unique(g).size >= g.size - 1          # only +0 / -0 coincide
