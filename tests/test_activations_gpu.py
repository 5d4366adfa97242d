"""-m gpu: every nonlinearity the library evaluates, swept over all fp16 inputs IN EACH KERNEL THAT EMBEDS ONE, against the
function in float64 through the one comparator of tests/test_activations_host.py:

    |got - c f(x)| <= 0.5 ulp16(exact) (1 + 2^-8)  +  2^-21 |exact|  +  |c| |x| eps_site

Fused sites are driven with selector weights so that the pre-activation is chosen, not computed: the output is fp16(c * f(x)).

site -> test
    silu_f            vdx_silu_f16                      test_direct_ops[silu]
    silu_f            vdx_groupnorm_part_f16, silu = 1  test_silu_behind_groupnorm
    silu8 (K1)        vdx_conv3x3_gn_f16                test_silu_in_conv3x3_gn[one source | two sources]
    silu8 (K3)        vdx_tconv_gn_f16, F = 8, 12, 16   test_silu_in_tconv_gn
    erf_fast          vdx_gelu_f16                      test_direct_ops[gelu]
    gelu_tab          gemm_kernel / gemm_ring_kernel / gemm_ws_kernel, GEGLU   test_geglu_epilogue (every instantiation:
                                                        test_geglu_cases_cover_every_geglu_instantiation)
    gelu_poly (K8)    vdx_ff_block_f16 / _proj_f16      test_ff_block_gelu[plain | proj]
    QuickGELU         vdx_quick_gelu_f16                test_direct_ops[quick_gelu]
    exp               vdx_vae_posterior_f16             test_vae_posterior_exp
    sin / cos / exp   vdx_timestep_embedding_f16        test_timestep_embedding_all_timesteps

MEASURED ENVELOPES (printed by every run, `pytest -s`).  MI355X (gfx950), 2026-10-16, on the tree of the commit that added
this file (parent 7139045).  "needed" = worst (err - the two rounding terms) / (|c| |x|): what eps_site has to cover.
"worst": the largest error in fp16 ulps of the exact value, over all multipliers (2046 ulp at x = -5.35 is c = 1024: the exact
-2.4e-4 against the left tail's 0, inside 1024 * 5.35 * 3e-6), each with the input where it occurred.  As printed:

    QuickGELU: vdx_quick_gelu_f16  claimed 0  needed 0  at x = 0.0  worst 0.500 ulp at x = -3.935546875  (63488 values)
    erf_fast: vdx_gelu_f16  claimed 7.5e-08  needed 6.7e-08  at x = -3.05078125  worst 2.043 ulp at x = -4.08984375  (63488 values)
    exp: vdx_vae_posterior_f16  claimed 0  needed 0  at x = 0.0  worst 0.500 ulp at x = 0.0226898193359375  (63488 values)
    gelu_poly: ff_fused_kernel<320, false>  claimed 2.1e-05  needed 2.01e-05  at x = -4.499995231628418  worst 16031744.000 ulp at x = -65504.0  (39360 values)
    gelu_poly: ff_fused_kernel<320, true>  claimed 2.1e-05  needed 2.01e-05  at x = -4.499995231628418  worst 16031744.000 ulp at x = -65504.0  (39360 values)
    gelu_tab: gemm_kernel<128, 128, 2, 2, 0, true, false, 0> claimed 3.08e-06  needed 2.23e-06  at x = -1.17578125  worst 2046.461 ulp at x = -5.34765625  (317440 values)
    gelu_tab: gemm_kernel<128, 128, 2, 2, 0, true, false, 0> (gate in bias) claimed 3.08e-06  needed 2.85e-07  at x = -5.0  worst 735.311 ulp at x = -5.66015625  (640 values)
    gelu_tab: gemm_kernel<128, 128, 4, 2, 0, true, false, 0> (gate in bias) claimed 3.08e-06  needed 2.85e-07  at x = -5.0  worst 735.311 ulp at x = -5.66015625  (640 values)
    gelu_tab: gemm_kernel<256, 320, 4, 2, 0, true, false, 0> claimed 3.08e-06  needed 2.23e-06  at x = -1.17578125  worst 2046.461 ulp at x = -5.34765625  (952320 values)
    gelu_tab: gemm_kernel<256, 320, 4, 2, 0, true, false, 0> (gate in bias) claimed 3.08e-06  needed 2.85e-07  at x = -5.0  worst 735.311 ulp at x = -5.66015625  (1920 values)
    gelu_tab: gemm_kernel<256, 64, 4, 1, 0, true, false, 0> (gate in bias) claimed 3.08e-06  needed 2.85e-07  at x = -5.0  worst 735.311 ulp at x = -5.66015625  (640 values)
    gelu_tab: gemm_ring_kernel<2, 64, 2, 0, true> (gate in bias) claimed 3.08e-06  needed 2.85e-07  at x = -5.0  worst 735.311 ulp at x = -5.66015625  (640 values)
    gelu_tab: gemm_ring_kernel<4, 32, 4, 0, true> (gate in bias) claimed 3.08e-06  needed 2.85e-07  at x = -5.0  worst 735.311 ulp at x = -5.66015625  (640 values)
    gelu_tab: gemm_ring_kernel<4, 64, 4, 0, true> (gate in bias) claimed 3.08e-06  needed 2.85e-07  at x = -5.0  worst 735.311 ulp at x = -5.66015625  (640 values)
    gelu_tab: gemm_ws_kernel<320, 10, 64, true, false, false, false> (gate in bias) claimed 3.08e-06  needed 2.85e-07  at x = -5.0  worst 673.092 ulp at x = -5.67578125  (800 values)
    gelu_tab: gemm_ws_kernel<320, 8, 64, true, false, true, false> (gate in bias) claimed 3.08e-06  needed 5.93e-07  at x = -0.564453125  worst 576.266 ulp at x = -5.703125  (1280 values)
    gelu_tab: gemm_ws_kernel<512, 8, 32, true, false, true, false> (gate in bias) claimed 3.08e-06  needed 1.58e-06  at x = -1.7333984375  worst 1738.300 ulp at x = -5.11328125  (2048 values)
    gelu_tab: gemm_ws_kernel<640, 8, 32, true, false, true, false> (gate in bias) claimed 3.08e-06  needed 2.85e-07  at x = -5.0  worst 1823.246 ulp at x = -5.23828125  (2560 values)
    silu8: conv3x3_gn_kernel (256 + 64)  claimed 0  needed 0  at x = 0.0  worst 0.500 ulp at x = -2.724609375  (38720 values)
    silu8: conv3x3_gn_kernel (320 + 0)  claimed 0  needed 0  at x = 0.0  worst 0.500 ulp at x = -2.724609375  (38720 values)
    silu8: tconv_gn_kernel<12>  claimed 0  needed 0  at x = 0.0  worst 0.500 ulp at x = -2.724609375  (38720 values)
    silu8: tconv_gn_kernel<16>  claimed 0  needed 0  at x = 0.0  worst 0.500 ulp at x = -2.724609375  (38720 values)
    silu8: tconv_gn_kernel<8>  claimed 0  needed 0  at x = 0.0  worst 0.500 ulp at x = -2.724609375  (38720 values)
    silu_f: groupnorm(silu_act)  claimed 0  needed 0  at x = 0.0  worst 0.500 ulp at x = -0.7138671875  (38720 values)
    silu_f: vdx_silu_f16  claimed 0  needed 0  at x = 0.0  worst 0.500 ulp at x = -0.7138671875  (63488 values)
    sin / cos / exp: vdx_timestep_embedding_f16  claimed 5.96e-08  needed 0  at x = 0.0  worst 0.500 ulp at x = 465.0  (320000 values)
    (a GEGLU instantiation without a row of its own printed the figures of gemm_kernel<128, 128, 2, 2, ...>; <256, 320, ...>
    is reached by variants 0, 2 and 6: three launches in one row)

Before this file the table's left tail was Phi(-5) = 2.9e-7 times x (-0.0195 at x = -65472, c = 1: inside the 3e-6 |x| the
header allows, so the comparator accepted it; it is now exactly -0), K8's header claimed 2e-5 (2.01e-5 is needed), and the
timestep embedding's frequencies came from expf, one fp32 ulp off the correctly rounded value in a few columns (44 of 320 000
outputs outside the bound: t = 601, got -2.372e-4 for -2.983e-4, 256 fp16 ulps against 151 allowed).  On a library with the parent's table every test_geglu_epilogue case fails its exact-zero assertion (70 395 outputs each).  The whole module takes 3.5 s."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_activations_host as H
from test_activations_host import compare

pytestmark = pytest.mark.gpu

MULTIPLIERS = (1.0, -1.0, 0.37109375, 3.0, 1024.0)
ENVELOPES = {}


def _ops():
    import vdx  # noqa: F401
    from vdx import ops, packing
    return ops, packing


def record(env):
    ENVELOPES[env.site] = ENVELOPES[env.site].merge(env) if env.site in ENVELOPES else env
    print(env.row())
    return env


@pytest.fixture(scope="module", autouse=True)
def envelope_table():
    yield
    print("\n==== activation envelopes (site, claimed eps, eps needed = worst (err - rounding) / |c x|, worst error) ====")
    for k in sorted(ENVELOPES):
        print(ENVELOPES[k].row())


def dev16(values, gpu):
    """fp16 numpy array -> device tensor with the same bits."""
    return torch.from_numpy(np.ascontiguousarray(values).view(np.int16).copy()).to(gpu).view(torch.float16)


def host64(t):
    return t.detach().cpu().view(torch.int16).numpy().view(np.float16).astype(np.float64)


def all_rows_equal(out):
    """Every row has the values of row 0 (no NaN; the sign of a zero is free: x * 0 + beta keeps x's sign for beta = -0)."""
    return bool((out == out[:1]).all())


# ---- (a) the direct ops --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["silu", "gelu", "quick_gelu"])
def test_direct_ops(gpu, name):
    """All 65 536 bit patterns in one tensor.  Finite -> comparator; NaN -> NaN; +inf -> +inf; -inf -> NaN, which is what
    torch's fp32 functions give on the CPU (-inf * 0)."""
    ops, _ = _ops()
    bits = H.all_fp16_bits()
    v = bits.view(np.float16)
    out = host64(getattr(ops, name)(dev16(v, gpu)))
    x = v.astype(np.float64)
    fin = np.isfinite(x)
    exact, eps = {"silu": (H.silu64, 0.0), "gelu": (H.gelu64, H.EPS_ERF_FAST), "quick_gelu": (H.quick_gelu64, 0.0)}[name]
    site = {"silu": "silu_f: vdx_silu_f16", "gelu": "erf_fast: vdx_gelu_f16", "quick_gelu": "QuickGELU: vdx_quick_gelu_f16"}[name]
    record(compare(site, x[fin], out[fin], exact(x[fin]), 1.0, eps))
    assert np.isnan(out[np.isnan(x)]).all() and np.isnan(x).sum() == 2046
    assert out[bits == 0x7C00][0] == np.inf
    xt = torch.tensor([float("-inf")])
    want = {"silu": F.silu(xt), "gelu": F.gelu(xt), "quick_gelu": xt * torch.sigmoid(1.702 * xt)}[name].item()
    got = out[bits == 0xFC00][0]
    assert np.isnan(want) and np.isnan(got), (name, want, got)


# ---- (b) the GEGLU epilogue of every GEMM instantiation ------------------------------------------------------------------
GEGLU_CASES = [(v, 1280, 64) for v in (1, 2, 3, 4, 5, 6, 8, 9, 0)] + [(7, 1600, 320), (7, 2560, 320), (7, 4096, 512), (7, 5120, 640)]
GEGLU_M = 63488


def test_geglu_cases_cover_every_geglu_instantiation():
    ops, _ = _ops()
    rows = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_kernel_names.json")))
    want = {r[-1] for r in rows if r[4]}
    assert len(want) >= 11 and all("true" in n for n in want)
    have = {ops.gemm_kernel_name(GEGLU_M, N, K, ops.PLAIN, True, v) for v, N, K in GEGLU_CASES}
    have |= {ops.gemm_kernel_name(704, N, K, ops.PLAIN, True, v) for v, N, K in GEGLU_CASES}
    assert want <= have, sorted(want - have)


def _geglu_weights(packing, N, K, gpu):
    """Logical [value | gate] weight: value row j = c_j e_0, gate row j = e_1; -> packed weight, zero bias, c per column."""
    n_out = N // 2
    c = np.array([MULTIPLIERS[j % len(MULTIPLIERS)] for j in range(n_out)])
    w = torch.zeros(N, K, dtype=torch.float16)
    w[:n_out, 0] = torch.from_numpy(c).half()
    w[n_out:, 1] = 1.0
    wp, bp = packing.pack_geglu(w, torch.zeros(N, dtype=torch.float16))
    return wp.to(gpu), bp.to(gpu), c


@pytest.mark.parametrize("variant,N,K", GEGLU_CASES)
def test_geglu_epilogue(gpu, variant, N, K):
    """One launch of 63 488 rows: row r carries the r-th finite fp16 value as its gate, column j the multiplier c_j.  Then
    the gate in the bias (a = 0): the bias add in front of the GELU."""
    ops, packing = _ops()
    name = ops.gemm_kernel_name(GEGLU_M, N, K, ops.PLAIN, True, variant)
    assert ("gemm_ws_kernel" in name) == (variant == 7 or K > 64), name
    site = f"gelu_tab: {name}"
    g = H.finite_fp16()
    x = g.astype(np.float64)
    n_out, nc = N // 2, len(MULTIPLIERS)
    wp, bp, c = _geglu_weights(packing, N, K, gpu)
    a = torch.zeros(GEGLU_M, K, dtype=torch.float16, device=gpu)
    a[:, 0] = 1.0
    a[:, 1] = dev16(g, gpu)
    out = ops.gemm(a, wp, M=GEGLU_M, bias=bp, geglu=True, variant=variant)
    assert tuple(out.shape) == (GEGLU_M, n_out)
    ob = out.view(torch.int16)
    assert torch.equal(ob[:, nc:], ob[:, :-nc]), f"{site}: columns of one multiplier differ"
    first = host64(out[:, :nc].contiguous()).reshape(GEGLU_M, nc)
    gx = H.gelu64(x)
    for j, cj in enumerate(MULTIPLIERS):
        record(compare(site, x, first[:, j], cj * gx, cj, H.EPS_GELU_TAB))
    # the left tail is exactly zero (the clamped index reads Phi = 0), for every multiplier, 1024 included
    tail = x < -5.0
    assert tail.sum() == 14079
    bad = np.flatnonzero(tail[:, None] & (first != 0.0))
    assert bad.size == 0, (f"{site}: {bad.size} outputs with gate < -5 are not zero; the first: gate {float(x[bad[0] // nc])!r}, "
                           f"c {MULTIPLIERS[bad[0] % nc]!r}, got {float(first.ravel()[bad[0]])!r}")
    del a, out, ob
    # the gate in the bias: n_out gate values spread over all finite fp16 values, the edges included
    Mb = 704
    pick = np.linspace(0, g.size - 1, n_out).astype(np.int64)
    gb = g[pick].copy()
    gb[1:9] = np.array([65504.0, -0.0, -5.0, 5.0, -4.9921875, 2.0 ** -24, -(2.0 ** -24), -5.00390625], dtype=np.float16)
    b = torch.zeros(N, dtype=torch.float16)
    b[:n_out] = torch.from_numpy(c).half()
    b[n_out:] = torch.from_numpy(gb.view(np.int16).copy()).view(torch.float16)
    wz, bpk = packing.pack_geglu(torch.zeros(N, K, dtype=torch.float16), b)
    outb = ops.gemm(torch.zeros(Mb, K, dtype=torch.float16, device=gpu), wz.to(gpu), M=Mb, bias=bpk.to(gpu), geglu=True, variant=variant)
    assert all_rows_equal(outb), f"{site}: rows differ with the gate in the bias"
    xb = gb.astype(np.float64)
    gotb = host64(outb[0])
    record(compare(site + " (gate in bias)", xb, gotb, c * H.gelu64(xb), c, H.EPS_GELU_TAB))
    assert (xb < -5.0).sum() > n_out // 8 and np.all(gotb[xb < -5.0] == 0.0), \
        f"{site}: gate < -5 in the bias: not zero at {xb[(xb < -5.0) & (gotb != 0.0)][:5]!r}"


# ---- (c) K8 ----------------------------------------------------------------------------------------------------------------
K8_M = 192 * 3 + 40


def _batches(values, n=320):
    """values (1-D) in batches of n; the last one is filled up with its own first values."""
    for i in range(0, values.size, n):
        b = values[i:i + n]
        if b.size < n:
            b = np.concatenate([b, values[:n - b.size]])
        yield b


@pytest.mark.parametrize("proj", [False, True], ids=["plain", "proj"])
def test_ff_block_gelu(gpu, proj):
    """w1 = 0 makes the gate b1[gate j] and the value b1[value j] = c whatever LayerNorm does; w2 selects hidden unit j(i) for
    output i; t = 0, b2 = 0: out[r][i] = fp16(c_i * gelu(g_i)) in every row (a partial last group of rows included).  b1 is
    fp32, so besides the fp16 coverage set the gate sweeps fp32 values finer than fp16 around the clamp points and around 0."""
    ops, packing = _ops()
    inner, hid = 320, 1280
    hidden_of = 4 * np.arange(inner) + (np.arange(inner) % 4)              # hidden unit of output i: every chunk, mixed lanes
    w2 = torch.zeros(inner, hid)
    w2[torch.arange(inner), torch.from_numpy(hidden_of)] = 1.0
    z = lambda *s: torch.zeros(*s, device=gpu)       # noqa: E731
    w1, w2, ones = z(2 * hid, inner), w2.to(gpu), torch.ones(inner, device=gpu)
    val_at = torch.from_numpy(hidden_of).to(gpu)                          # rows of diffusers' GEGLU.proj: value | gate
    gate_at = val_at + hid
    t = torch.zeros(K8_M, inner, dtype=torch.float16, device=gpu)
    kw = {}
    if proj:
        tail = packing.pack_k8_proj(torch.eye(inner, device=gpu), z(inner))
        kw = dict(proj=(tail, torch.zeros(K8_M, inner, dtype=torch.float16, device=gpu), K8_M))
    gates = np.concatenate([H.coverage_fp16().astype(np.float32), H.k8_fp32_grid()])
    site = f"gelu_poly: ff_fused_kernel<320, {'true' if proj else 'false'}>"
    cs = np.array(MULTIPLIERS[:4])
    total = None
    for gb in _batches(gates):
        c = cs[np.arange(inner) % 4]
        c = np.where(np.abs(gb) * 3.0 < 60000.0, c, np.sign(c))            # no inf in the hidden row: 0 * inf in W2's product
        b1 = z(2 * hid)                                                   # fp32: pack_k8 keeps it as it is (beta = 0)
        b1[val_at] = torch.from_numpy(c.astype(np.float32)).to(gpu)
        b1[gate_at] = torch.from_numpy(gb.copy()).to(gpu)
        blob = packing.pack_k8(w1, b1, w2, z(inner), ones, z(inner))
        out = ops.ff_block(t, blob, M=K8_M, **kw)
        assert all_rows_equal(out), f"{site}: rows differ"
        x = gb.astype(np.float64)
        env = compare(site, x, host64(out[0]), c * H.gelu64(x), c, H.eps_gelu_poly(x))
        total = env if total is None else total.merge(env)
    record(total)


# ---- (d) SiLU behind a GroupNorm ---------------------------------------------------------------------------------------------
def _silu_sweep(site, gpu, launch):
    """`launch(beta fp16 device [320]) -> out [rows][320]`: gamma = 0, so every row must be silu(beta)."""
    total = None
    for vb in _batches(H.coverage_fp16()):
        out = launch(dev16(vb, gpu))
        assert all_rows_equal(out), f"{site}: rows differ"
        x = vb.astype(np.float64)
        env = compare(site, x, host64(out[0]), H.silu64(x))
        total = env if total is None else total.merge(env)
    record(total)


def test_silu_behind_groupnorm(gpu):
    ops, _ = _ops()
    C, ns, rps = 320, 2, 77
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(ns * rps, C, generator=g) * 3).half().to(gpu)
    gamma = torch.zeros(C, dtype=torch.float16, device=gpu)
    _silu_sweep("silu_f: groupnorm(silu_act)", gpu,
                lambda beta: ops.groupnorm(x, gamma, beta, groups=32, n_samples=ns, rows_per_sample=rps, eps=1e-5, silu_act=True))


@pytest.mark.parametrize("c1,c2", [(320, 0), (256, 64)], ids=["one source", "two sources"])
def test_silu_in_conv3x3_gn(gpu, c1, c2):
    """K1: the weight selects channel i at the centre tap, so out[pixel][i] = fp16(silu(beta_i)) at border pixels too."""
    ops, packing = _ops()
    C, n, hh, ww = c1 + c2, 2, 5, 9
    g = torch.Generator().manual_seed(2)
    rows = (torch.randn(n * hh * ww, C, generator=g) * 3).half().to(gpu)
    xa = rows[:, :c1].contiguous()
    xb = rows[:, c1:].contiguous() if c2 else None
    w = torch.zeros(C, C, 3, 3, dtype=torch.float16)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    wp = packing.pack_conv3x3(w).to(gpu)
    gamma = torch.zeros(C, dtype=torch.float16, device=gpu)
    assert ops.conv3x3_gn_supported(c1, c2, C)
    _silu_sweep(f"silu8: conv3x3_gn_kernel ({c1} + {c2})", gpu,
                lambda beta: ops.conv3x3_gn(xa, gamma, beta, wp, x2=xb, groups=32, n_img=n, h=hh, wd=ww, eps=1e-5))


@pytest.mark.parametrize("Fr", [8, 12, 16])
def test_silu_in_tconv_gn(gpu, Fr):
    """K3, its three frame-tile instantiations: the weight selects channel i at the centre tap in time."""
    ops, packing = _ops()
    C, B, S = 320, 1, 20
    g = torch.Generator().manual_seed(3)
    rows = (torch.randn(B * Fr * S, C, generator=g) * 3).half().to(gpu)
    w = torch.zeros(C, C, 3, 1, 1, dtype=torch.float16)
    w[torch.arange(C), torch.arange(C), 1] = 1.0
    wp = packing.pack_tconv3(w).to(gpu)
    gamma = torch.zeros(C, dtype=torch.float16, device=gpu)
    assert ops.tconv_gn_supported(C, C, Fr)
    _silu_sweep(f"silu8: tconv_gn_kernel<{Fr}>", gpu,
                lambda beta: ops.tconv_gn(rows, gamma, beta, wp, groups=32, B=B, F=Fr, S=S, eps=1e-5))


# ---- (e) the VAE posterior's exp ---------------------------------------------------------------------------------------------
def test_vae_posterior_exp(gpu):
    """mean 0, eps 1, scale 1, log-variance = every finite fp16 value: out = fp16(exp(h)), h = fp16(0.5 * clamp(lv, -30, 20))
    (the kernel's "fp16 after every op"), h known exactly on the host.  The mode path returns the mean's bits."""
    ops, _ = _ops()
    lv = H.finite_fp16()
    hw = lv.size // 4
    mom = np.zeros((hw, 8), dtype=np.float16)
    mom[:, 4:] = lv.reshape(hw, 4)
    mom[:, :4] = 0.0
    md = dev16(mom, gpu)
    ones = torch.ones(1, 4, hw, dtype=torch.float16, device=gpu)
    out = host64(ops.vae_posterior(md, 1, hw, eps=ones)).reshape(4, hw).T.reshape(-1)      # out[c][p] -> order of lv
    hh = (np.clip(lv.astype(np.float32), -30.0, 20.0) * np.float32(0.5)).astype(np.float16).astype(np.float64)
    record(compare("exp: vdx_vae_posterior_f16", hh, out, np.exp(hh)))
    mom[:, :4] = lv[::-1].reshape(hw, 4)
    md = dev16(mom, gpu)
    mode = ops.vae_posterior(md, 1, hw).cpu().view(torch.int16).numpy().reshape(4, hw).T
    assert np.array_equal(mode, mom[:, :4].view(np.int16))


# ---- (f) the timestep embedding ------------------------------------------------------------------------------------------------
def test_timestep_embedding_all_timesteps(gpu):
    """All 1000 integer timesteps x dim 320, B = 2, against float64 cos / sin of the argument formed in fp32 as diffusers'
    `get_timestep_embedding` forms it.  Bound: the comparator's rounding terms + 2^-24 t for the fp32 argument."""
    ops, _ = _ops()
    T, B, dim = 1000, 2, 320
    half = dim // 2
    ts = torch.zeros(T, 4, dtype=torch.float32)
    ts[:, 0] = torch.arange(T, dtype=torch.float32)
    td = ts.to(gpu)
    buf = torch.full((T, B, dim), float("nan"), dtype=torch.float16, device=gpu)
    for i in range(T):
        ops.timestep_embedding(td[i, :1], B, dim, out=buf[i])
    got = host64(buf).reshape(T, B, dim)
    assert np.array_equal(got[:, 0], got[:, 1])
    exponent = -np.log(10000.0) * torch.arange(half, dtype=torch.float32) / half
    # fp32 exponent and fp32 product, as diffusers; exp correctly rounded to fp32 (torch's own fp32 exp is one ulp off that at
    # j = 2 and j = 55 on the CPU, and differently so elsewhere: no kernel can follow it)
    f32 = torch.from_numpy(np.exp(exponent.double().numpy()).astype(np.float32))
    arg = (ts[:, :1] * f32[None, :]).double().numpy()
    exact = np.concatenate([np.cos(arg), np.sin(arg)], axis=1)
    tt = np.broadcast_to(ts[:, :1].double().numpy(), exact.shape)
    # the comparator with c = 1, "x" = t and eps_site = 2^-24: the third term is then 2^-24 * t
    record(compare("sin / cos / exp: vdx_timestep_embedding_f16", tt, got[:, 0], exact, 1.0, 2.0 ** -24))
