"""No GPU: the float64 reference of tests/gemm_exact_ref.py against torch's own operators, the exactness condition of its
case table, and the table's coverage of every instantiation vdx_gemm_f16 can launch (vdx_gemm_kernel_name is host-only).

Adding a kernel family.  A new instantiation in pick_tile, vdx_gemm_ring_launch or vdx_gemm_ws_launch shows up in
`probed_names` (a sweep of the pinned variants, modes, epilogues and weights-stationary shapes through the library's own
route) and fails `test_every_reachable_instantiation_is_listed` until it is (1) spelled in `listed_names` below and (2) given
cases in gemm_exact_ref.py (`VARIANTS` / `WS_FAMILIES` and the case builders) that hit its M-below-tile, M-tail, N-tail and
shortest-K edges, which `test_every_instantiation_has_cases_at_its_edges` derives from the cases' shapes."""
import pytest
import torch
import torch.nn.functional as F

import gemm_exact_ref as R


def _ops():
    import vdx  # noqa: F401
    from vdx import ops
    return ops


def tf(b):
    return "true" if b else "false"


# ---- the explicit list of instantiations (as rocprofv3 prints them), the phase form apart -----------------------------------
def tiled_name(v, mode, geglu, var=0):
    BM, BN = R.VARIANTS[v]
    if v in (3, 4, 8):
        wmb, rpw, ns = {3: (4, 64, 4), 4: (2, 64, 2), 8: (4, 32, 4)}[v]
        assert (wmb * rpw, 320) == (BM, BN)
        return f"gemm_ring_kernel<{wmb}, {rpw}, {ns}, {mode}, {tf(geglu)}>"
    wm, wn = {1: (4, 2), 9: (2, 2), 5: (4, 1), 2: (4, 2), 6: (4, 2)}[v]
    if var == 2 and v == 1:
        wm = 2                       # the nearest-to-size gather runs the four-wave 128x128 form
    split = mode != 0 and v == 2     # split staging roles: the gathers of variant 2
    return f"gemm_kernel<{BM}, {BN}, {wm}, {wn}, {mode}, {tf(geglu)}, {tf(split)}, {var}>"


def ksplit_name(mode):
    return f"gemm_kernel<256, 320, 4, 2, {mode}, false, {tf(mode != 0)}, 1> split-K + reduce"


def ws_name(fam, geglu=False, res=False, wset=False):
    K, nw, rows, pipe = R.WS_FAMILIES[fam]
    return f"gemm_ws_kernel<{K}, {nw}, {rows}, {tf(geglu)}, {tf(res)}, {tf(pipe)}, {tf(wset)}>"


def listed_names():
    names = {tiled_name(v, m, False) for v in R.VARIANTS for m in (0, 1, 2)}           # {variants} x {plain, conv3x3, tconv3}
    names |= {tiled_name(v, 0, True) for v in R.VARIANTS}                              # x GEGLU
    names |= {tiled_name(v, 1, False, 2) for v in R.UPS2_VARIANTS}                     # the two upsample-to-size kernels
    names |= {ksplit_name(m) for m in (0, 1, 2)}                                       # the three split-K kernels
    for fam in R.WS_FAMILIES:                                                          # every weights-stationary family
        names |= {ws_name(fam), ws_name(fam, res=True), ws_name(fam, geglu=True)}
        if fam != 3:
            names.add(ws_name(fam, wset=True))
    # (variants 2 and 6 differ in the staging roles of the gathers only: plain and GEGLU are one instantiation each)
    assert len(names) == 8 * 4 - 2 + 2 + 3 + 4 * 3 + 3
    return names


def expected_name(c):
    mode = R.MODE[c["kind"]]
    geglu = c["kind"] == "geglu"
    if c["ksplit"]:
        return ksplit_name(mode)
    if c["variant"] == 7:
        return ws_name(R.ws_family(c["M"], c["N"], c["K"], geglu), geglu, c["epi"] in ("all", "bias_res"), bool(c["wset_rows"]))
    return tiled_name(c["variant"], mode, geglu, 2 if c["conv"] and c["conv"][6] == 2 else 0)


def name_of(c):
    return _ops().gemm_kernel_name(**R.name_kwargs(c))


def probed_names():
    """Every name the library's route can give: all 16 values of the variant field x modes x epilogues x gathers x split-K,
    and for the weights-stationary route every K up to 2048 x N x epilogue x weight sets.  Refused calls have no name."""
    ops = _ops()
    from vdx._lib import VdxError
    names = set()

    def ask(**kw):
        try:
            names.add(ops.gemm_kernel_name(**kw))
        except VdxError:
            pass

    for v in range(16):
        for M in (64, 300, 20000):
            for N in (64, 256, 320, 640):
                ask(M=M, N=N, K=64, mode=0, geglu=False, variant=v)
                ask(M=M, N=N, K=64, mode=0, geglu=True, variant=v)
                ask(M=M, N=N, K=64, mode=0, geglu=False, variant=v, single_source=False, residual=True)
                ask(M=M, N=N, K=192, mode=2, geglu=False, variant=v)
                for ups, pm, st in ((0, 0, 1), (1, 0, 1), (2, 0, 1), (0, 1, 2), (0, 0, 2)):
                    hi, ho = (M, M) if st == 1 and ups == 0 else (M, M // 2) if st == 2 else (M // 2, M)
                    wi, wo = (1, 1) if st == 1 and ups != 1 else (2, 1) if st == 2 else (1, 2)
                    ask(M=ho * wo, N=N, K=576, mode=1, geglu=False, variant=v, conv=(1, hi, wi, ho, wo, st, ups), pad_mode=pm)
                for ks in (2, 4):
                    ask(M=M, N=N, K=1024, mode=0, geglu=False, variant=v, ksplit=ks)
                    ask(M=M, N=N, K=9 * 128, mode=1, geglu=False, variant=v, ksplit=ks)
                    ask(M=M, N=N, K=3 * 256, mode=2, geglu=False, variant=v, ksplit=ks)
    for K in range(64, 2049, 64):
        for M in (64, 20032):
            for N in (64, 128, 256, 320, 384, 512, 640, 1280):
                for v in (0, 7):
                    for geglu, res, wset in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 64)):
                        ask(M=M, N=N, K=K, mode=0, geglu=bool(geglu), variant=v, residual=bool(res), wset_rows=wset)
    return names


# ---- 1: the reference is the operator ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,stride,pad_mode,ups,size", [
    (5, 7, 1, 0, 0, None), (1, 9, 1, 0, 0, None), (9, 1, 1, 0, 0, None), (1, 1, 1, 0, 0, None), (5, 7, 2, 0, 0, None),
    (6, 8, 2, 0, 0, None), (1, 1, 2, 0, 0, None), (6, 8, 2, 1, 0, None), (7, 9, 2, 1, 0, None), (2, 3, 2, 1, 0, None),
    (3, 5, 1, 0, 1, None), (3, 3, 1, 0, 2, (5, 6)), (7, 2, 1, 0, 2, (7, 3)), (9, 6, 1, 0, 2, (11, 9))])
def test_conv_reference_is_torch_conv2d(h, w, stride, pad_mode, ups, size):
    g = torch.Generator().manual_seed(h * 31 + w)
    x = torch.randint(-2, 3, (3, 8, h, w), generator=g).double()
    wt = torch.randint(-2, 3, (5, 8, 3, 3), generator=g).double()
    y = x
    if ups == 1:
        y = F.interpolate(y, scale_factor=2.0, mode="nearest")
    elif ups == 2:
        y = F.interpolate(y, size=size, mode="nearest")
    want = F.conv2d(F.pad(y, (0, 1, 0, 1)), wt, stride=2) if pad_mode == 1 else F.conv2d(y, wt, stride=stride, padding=1)
    got = R.conv3x3_ref(x, wt, stride, pad_mode, ups, size)
    assert got.shape == want.shape == (3, 5) + R._conv_out(h, w, stride, pad_mode, ups, size)
    assert torch.equal(got, want)


@pytest.mark.parametrize("frames,hw", [(1, 1), (2, 7), (3, 16), (5, 33)])
def test_tconv_reference_is_torch_conv3d(frames, hw):
    g = torch.Generator().manual_seed(frames + hw)
    x = torch.randint(-2, 3, (2, frames, hw, 8), generator=g).double()
    wt = torch.randint(-2, 3, (5, 8, 3), generator=g).double()
    want = F.conv3d(x.permute(0, 3, 1, 2)[..., None], wt[..., None, None], padding=(1, 0, 0))[..., 0].permute(0, 2, 3, 1)
    assert torch.equal(R.tconv3_ref(x, wt), want)


def test_reference_of_whole_cases_is_torch():
    """build(): packed weights, operand slices and the epilogue of a few table rows, against torch's operators on the operands
    as the kernel will read them (the packed table unpacked by its documented K order)."""
    by_id = {c["id"]: c for c in R.cases()}
    picked = [c for c in R.cases() if c["variant"] == 2 and not c["refused"] and c["exact"]
              and (c["c2"] or c["rows"] or c["pad_mode"] or (c["conv"] and c["conv"][6]) or (c["tconv"] and c["tconv"][1] == 5 and c["epi"] == "all"))]
    assert len(picked) >= 8 and by_id
    for c in picked:
        t, ref, kw = R.build(c)
        cut = lambda k: t[k][0][:, t[k][1]:t[k][1] + t[k][2]].double()
        M, N, c1 = c["M"], c["N"], c["c1"]
        w = t["w"].double()
        if c["kind"] == "plain":
            a = torch.cat([cut("a"), cut("a2")], 1) if c["c2"] else cut("a")
            y = F.linear(a, w)
        elif c["kind"] == "conv":
            n, h, wd, ho, wo, stride, ups = c["conv"]
            w4 = w.reshape(N, c1 // 64, 9, 64).permute(0, 1, 3, 2).reshape(N, c1, 3, 3)       # K = (slice, tap, channel)
            x = cut("a").reshape(n, h, wd, c1).permute(0, 3, 1, 2)
            if ups:
                x = F.interpolate(x, size=(ho, wo) if ups == 2 else (2 * h, 2 * wd), mode="nearest")
            y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w4, stride=2) if c["pad_mode"] else F.conv2d(x, w4, stride=stride, padding=1)
            y = y.permute(0, 2, 3, 1).reshape(M, N)
        else:
            B, fr, hw = c["tconv"]
            w5 = w.reshape(N, c1 // 64, 3, 64).permute(0, 1, 3, 2).reshape(N, c1, 3, 1, 1)
            y = F.conv3d(cut("a").reshape(B, fr, hw, c1).permute(0, 3, 1, 2)[..., None], w5, padding=(1, 0, 0))
            y = y[..., 0].permute(0, 2, 3, 1).reshape(M, N)
        if "bias" in t:
            y = y + t["bias"].double()
        if "bias2" in t:
            y = y + cut("bias2")[torch.arange(M) // kw["rows_per_bias2"]]
        if "residual" in t:
            y = y + cut("residual")
        assert torch.equal(y, ref), c["id"]


# ---- 2: the exactness condition ---------------------------------------------------------------------------------------------
def test_exact_cases_are_fp16_exact_integers():
    n = 0
    for c in R.cases():
        if not c["exact"] or c["refused"]:
            continue
        t, ref, _ = R.build(c)
        assert ref.shape == (c["M"], c["N"]) and ref.abs().max() < 2048, (c["id"], float(ref.abs().max()))
        assert torch.equal(ref, ref.round()) and torch.equal(ref.half().double(), ref), c["id"]
        for k, v in t.items():                       # the operands too: integers in their ranges, fp16-exact
            v = v[0] if isinstance(v, tuple) else v
            assert torch.equal(v.double(), v.double().round()) and v.abs().max() <= (2 if k in ("a", "a2", "w") else 8), (c["id"], k)
        n += 1
    assert n > 300


# ---- 3: coverage ------------------------------------------------------------------------------------------------------------
def test_every_reachable_instantiation_is_listed():
    """The list is exactly what the route can reach (the phase form apart: tests/test_upconv_phase_gpu.py)."""
    probed, listed = probed_names(), listed_names()
    assert probed == listed, f"reachable but not listed: {sorted(probed - listed)}; listed but not reached: {sorted(listed - probed)}"


def test_every_case_reaches_the_family_it_names():
    from vdx._lib import VdxError
    for c in R.cases():
        if c["refused"]:
            with pytest.raises(VdxError):
                name_of(c)
        else:
            assert name_of(c) == expected_name(c), c["id"]


def test_every_instantiation_has_cases_at_its_edges():
    seen = {}
    for c in R.cases():
        if not c["refused"]:
            seen.setdefault(name_of(c), set()).update(R.edges_of(c))
    assert set(seen) == listed_names(), f"without a case: {sorted(listed_names() - set(seen))}; unlisted: {sorted(set(seen) - listed_names())}"
    want = {"m_below", "m_tail", "n_tail", "k_short"}
    missing = {n: sorted(want - e) for n, e in seen.items() if want - e}
    assert not missing, missing


def test_every_group_has_the_full_epilogue_and_the_listed_edges():
    """Per pinned tile variant: every listed M, N and K of the plain table, two sources, a row range inside tiles, the
    rows_per_bias2 values, and bias + bias2 + residual in every exact mode."""
    for v, (BM, BN) in R.VARIANTS.items():
        mine = [c for c in R.cases() if c["variant"] == v and not c["ksplit"]]
        plain = [c for c in mine if c["kind"] == "plain"]
        assert {1, 15, BM - 1, BM, BM + 1, 2 * BM + 17} <= {c["M"] for c in plain}
        assert {64, BN, BN + 64} | ({BN - 64} if BN > 64 else set()) <= {c["N"] for c in plain}
        assert {64, 128, 192, 320} <= {c["K"] for c in plain}
        assert {1, 37} <= {c["rpb2"] for c in plain} and any(c["rpb2"] == c["M"] for c in plain)
        assert any(c["c2"] == 128 and c["c1"] == 64 and c["pad"] for c in plain)
        assert any(c["rows"] and c["rows"][0] % 16 and c["rows"][1] % 16 and c["rows"][1] < c["M"] for c in plain)
        for kind in ("plain", "conv", "tconv"):
            assert any(c["epi"] == "all" for c in mine if c["kind"] == kind), (v, kind)
        assert {(c["M"], c["c1"]) for c in mine if c["kind"] == "geglu"} >= {(m, k) for m in (1, BM + 1) for k in (64, 320)}
