"""-m gpu: every instantiation of vdx_gemm_f16 at its tile edges against the float64 reference of tests/gemm_exact_ref.py.

Integer inputs make every sum exact (see gemm_exact_ref.py), so a case passes only if the kernel returns the reference
rounded to fp16 BIT FOR BIT: one dropped, doubled or misplaced element changes an output by at least 1.  Per case:
  1 the rows [row_begin, row_end) x [0, N) equal ref.half()
  2 `out` is a column slice of a wider NaN-filled buffer with rows below it: everything outside the product is still NaN
  3 a second call leaves the same bits
  4 every other tile family that takes the shape returns the same tensor (what the row-split callers rely on)
GEGLU cases go through the erf table: they keep the bound of tests/test_ops_gpu.py (`close`, 3e-3) and checks 2 and 3.
Cases the library refuses by design assert the VdxError."""
import pytest
import torch

import gemm_exact_ref as R
from test_ops_gpu import close

pytestmark = pytest.mark.gpu

GROUPS = sorted({R.group_of(c) for c in R.cases()})


def _ops():
    import vdx  # noqa: F401
    from vdx import ops
    return ops


def _call(ops, gpu, c, t, kw, n_out, **over):
    """One launch into a fresh NaN-filled buffer -> (buffer, the out slice)."""
    M = c["M"]
    buf = torch.full((M + 3, n_out + 24), float("nan"), dtype=torch.float16, device=gpu)
    out = buf[:M, 8:8 + n_out]
    args = dict(kw, **over)
    ops.gemm(t["a"], t["w"], a2=t.get("a2"), bias=t.get("bias"), bias2=t.get("bias2"), residual=t.get("residual"),
             wset_bias=t.get("wset_bias"), out=out, **args)
    return buf, out


def _where(c, bad):
    """The first wrong element and where it sits in its tile."""
    f = R.family_of(c)
    r, col = (int(v) for v in bad.nonzero()[0])
    rb = c["rows"][0] if c["rows"] else 0
    return (f"{int(bad.sum())} / {bad.numel()} wrong; first at row {r + rb}, column {col} = tile ({r // f['BM']}, {col // f['BN']}) "
            f"+ ({r % f['BM']}, {col % f['BN']}) of {f['BM']}x{f['BN']}, K = {c['K']}")


def others_of(c):
    """The other routes that take the case's shape: (variant, ksplit) pairs."""
    if c["wset_rows"]:
        return []                                           # weight sets run on the weights-stationary kernels only
    if c["ksplit"] or c["variant"] == 7:
        return [(2, 0), (1, 0)]
    vs = R.UPS2_VARIANTS if c["conv"] and c["conv"][6] == 2 else R.VARIANTS
    return [(v, 0) for v in vs if v != c["variant"]]


def run_case(ops, gpu, c):
    from vdx._lib import VdxError
    t, ref, kw = R.build(c)
    t = {k: (v[0].to(gpu)[:, v[1]:v[1] + v[2]] if isinstance(v, tuple) else v.to(gpu)) for k, v in t.items()}
    n_out = ref.shape[1]
    if c["refused"]:
        with pytest.raises(VdxError):
            _call(ops, gpu, c, t, kw, n_out)
        return
    rb, re_ = c["rows"] if c["rows"] else (0, c["M"])
    buf, out = _call(ops, gpu, c, t, kw, n_out)
    got = out[rb:re_]
    if c["exact"]:
        want = ref.half().to(gpu)[rb:re_]
        bad = got != want                                   # (a NaN left in the product is wrong too)
        assert not bad.any(), f"{c['id']}: {_where(c, bad)}"
        assert torch.equal(got, want)
    else:
        close(got, ref.float()[rb:re_])
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[rb:re_, 8:8 + n_out] = False
    assert torch.isnan(buf[outside]).all(), f"{c['id']}: {int((~torch.isnan(buf[outside])).sum())} elements written outside the product"
    again, _ = _call(ops, gpu, c, t, kw, n_out)
    assert torch.equal(again.view(torch.int16), buf.view(torch.int16)), f"{c['id']}: a second call gives other bits"
    if c["exact"]:
        for v, ks in others_of(c):
            _, o = _call(ops, gpu, c, t, kw, n_out, variant=v, ksplit=ks)
            assert torch.equal(o[rb:re_], got), f"{c['id']}: variant {v} differs: {_where(c, o[rb:re_] != got)}"


@pytest.mark.parametrize("label,kind", GROUPS, ids=[f"{a}-{b}" for a, b in GROUPS])
def test_gemm_family_at_its_edges(gpu, label, kind):
    ops = _ops()
    mine = [c for c in R.cases() if R.group_of(c) == (label, kind)]
    assert mine
    for c in mine:
        if c["reserve"]:
            ops.set_reserved_cus(c["reserve"])
        try:
            run_case(ops, gpu, c)
        finally:
            if c["reserve"]:
                ops.set_reserved_cus(0)
