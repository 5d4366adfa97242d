"""-m gpu: the AutoencoderKL mid block's kernels at the edges the whole-model comparisons average away (their seeded weights
give a near-uniform softmax over ~100 keys): `_attention` alone in peaked-softmax regimes on the decoder and the encoder
table, `softmax_rows` at every instantiation and with extreme rows, `groupnorm` as the VAE calls it (eps 1e-6, 4 / 8 / 16
channels per group, partition_samples = 8).  References: fp64 torch on the CPU from the same fp16-rounded inputs and weights.

ATTENTION.  Cases and yardsticks: tests/vae_blocks_ref.py.  floor = rel-L2 against fp64 of the block with fp16 roundings where
diffusers has them (q, k, v, the SCALED scores, P, P.V, to_out, the residual add); the product (another, equally valid order:
scores pre-scaled by a power of two through the packed to_q, value bias folded behind to_out, one rounding after to_out + bias +
residual) may be at most 2 x floor, the margin test_vae_tiny_matches_golden grants.  Regimes d12 / d23 must also be finite.

MEASURED (printed by every run, `pytest -s`).  MI355X (gfx950), 2026-10-18, on the tree of the commit that added this file.
Per case: the floor, and the product's rel-L2 (its ratio to the floor) with the attention loaded through the decoder and
through the encoder loader (the same attention parameters in both tables):

    C    S     n  regime  floor      decoder table      encoder table
    512  64    1  a       2.650e-04  2.417e-04 (0.91 x)  2.417e-04 (0.91 x)
    512  64    3  a       2.645e-04  2.395e-04 (0.91 x)  2.395e-04 (0.91 x)
    512  192   1  a       2.521e-04  2.288e-04 (0.91 x)  2.288e-04 (0.91 x)
    512  192   3  a       2.499e-04  2.279e-04 (0.91 x)  2.279e-04 (0.91 x)
    512  1088  1  a       2.426e-04  2.217e-04 (0.91 x)  2.217e-04 (0.91 x)
    512  1088  3  a       2.455e-04  2.226e-04 (0.91 x)  2.226e-04 (0.91 x)
    512  64    1  b       7.669e-04  7.263e-04 (0.95 x)  7.263e-04 (0.95 x)
    512  64    3  b       8.203e-04  7.799e-04 (0.95 x)  7.799e-04 (0.95 x)
    512  192   1  b       9.641e-04  8.877e-04 (0.92 x)  8.877e-04 (0.92 x)
    512  192   3  b       1.006e-03  9.113e-04 (0.91 x)  9.113e-04 (0.91 x)
    512  1088  1  b       1.103e-03  1.050e-03 (0.95 x)  1.050e-03 (0.95 x)
    512  1088  3  b       1.082e-03  1.114e-03 (1.03 x)  1.114e-03 (1.03 x)
    512  64    1  c       2.019e-03  1.676e-03 (0.83 x)  1.676e-03 (0.83 x)
    512  64    3  c       1.370e-03  1.279e-03 (0.93 x)  1.279e-03 (0.93 x)
    512  192   1  c       1.929e-03  2.431e-03 (1.26 x)  2.431e-03 (1.26 x)
    512  192   3  c       1.924e-03  1.977e-03 (1.03 x)  1.977e-03 (1.03 x)
    512  1088  1  c       2.285e-03  2.539e-03 (1.11 x)  2.539e-03 (1.11 x)
    512  1088  3  c       2.580e-03  2.868e-03 (1.11 x)  2.868e-03 (1.11 x)
    512  64    1  d12     3.258e-04  2.859e-04 (0.88 x)  2.859e-04 (0.88 x)
    512  64    3  d12     3.292e-04  2.851e-04 (0.87 x)  2.851e-04 (0.87 x)
    512  192   1  d12     3.297e-04  2.857e-04 (0.87 x)  2.857e-04 (0.87 x)
    512  192   3  d12     3.297e-04  2.847e-04 (0.86 x)  2.847e-04 (0.86 x)
    512  1088  1  d12     3.288e-04  2.836e-04 (0.86 x)  2.836e-04 (0.86 x)
    512  1088  3  d12     3.280e-04  2.847e-04 (0.87 x)  2.847e-04 (0.87 x)
    512  64    1  d23     3.286e-04  2.852e-04 (0.87 x)  2.852e-04 (0.87 x)
    512  64    3  d23     3.279e-04  2.840e-04 (0.87 x)  2.840e-04 (0.87 x)
    512  192   1  d23     3.291e-04  2.861e-04 (0.87 x)  2.861e-04 (0.87 x)
    512  192   3  d23     3.295e-04  2.854e-04 (0.87 x)  2.854e-04 (0.87 x)
    512  1088  1  d23     3.289e-04  2.849e-04 (0.87 x)  2.849e-04 (0.87 x)
    512  1088  3  d23     3.289e-04  2.847e-04 (0.87 x)  2.847e-04 (0.87 x)
    512  64    1  e       3.765e-04  2.981e-04 (0.79 x)  2.981e-04 (0.79 x)
    512  64    3  e       3.758e-04  2.976e-04 (0.79 x)  2.976e-04 (0.79 x)
    512  192   1  e       3.726e-04  2.969e-04 (0.80 x)  2.969e-04 (0.80 x)
    512  192   3  e       3.743e-04  2.958e-04 (0.79 x)  2.958e-04 (0.79 x)
    512  1088  1  e       3.729e-04  2.964e-04 (0.79 x)  2.964e-04 (0.79 x)
    512  1088  3  e       3.717e-04  2.942e-04 (0.79 x)  2.942e-04 (0.79 x)
    128  64    1  a       2.671e-04  2.434e-04 (0.91 x)  2.434e-04 (0.91 x)
    128  64    3  a       2.591e-04  2.407e-04 (0.93 x)  2.407e-04 (0.93 x)
    128  192   1  a       2.441e-04  2.257e-04 (0.92 x)  2.257e-04 (0.92 x)
    128  192   3  a       2.487e-04  2.292e-04 (0.92 x)  2.292e-04 (0.92 x)
    128  1088  1  a       2.420e-04  2.236e-04 (0.92 x)  2.236e-04 (0.92 x)
    128  1088  3  a       2.419e-04  2.215e-04 (0.92 x)  2.215e-04 (0.92 x)
    128  64    1  b       9.765e-04  7.585e-04 (0.78 x)  7.585e-04 (0.78 x)
    128  64    3  b       8.952e-04  8.431e-04 (0.94 x)  8.431e-04 (0.94 x)
    128  192   1  b       1.078e-03  9.870e-04 (0.92 x)  9.870e-04 (0.92 x)
    128  192   3  b       9.931e-04  9.603e-04 (0.97 x)  9.603e-04 (0.97 x)
    128  1088  1  b       1.154e-03  1.284e-03 (1.11 x)  1.284e-03 (1.11 x)
    128  1088  3  b       1.093e-03  1.152e-03 (1.05 x)  1.152e-03 (1.05 x)
    128  64    1  c       2.317e-03  2.029e-03 (0.88 x)  2.029e-03 (0.88 x)
    128  64    3  c       2.420e-03  1.786e-03 (0.74 x)  1.786e-03 (0.74 x)
    128  192   1  c       2.193e-03  2.815e-03 (1.28 x)  2.815e-03 (1.28 x)
    128  192   3  c       2.384e-03  2.666e-03 (1.12 x)  2.666e-03 (1.12 x)
    128  1088  1  c       2.356e-03  2.621e-03 (1.11 x)  2.621e-03 (1.11 x)
    128  1088  3  c       2.550e-03  2.767e-03 (1.09 x)  2.767e-03 (1.09 x)
    128  64    1  d12     3.353e-04  2.905e-04 (0.87 x)  2.905e-04 (0.87 x)
    128  64    3  d12     3.352e-04  2.864e-04 (0.85 x)  2.864e-04 (0.85 x)
    128  192   1  d12     3.346e-04  2.895e-04 (0.87 x)  2.895e-04 (0.87 x)
    128  192   3  d12     3.310e-04  2.876e-04 (0.87 x)  2.876e-04 (0.87 x)
    128  1088  1  d12     3.321e-04  2.869e-04 (0.86 x)  2.869e-04 (0.86 x)
    128  1088  3  d12     3.282e-04  2.851e-04 (0.87 x)  2.851e-04 (0.87 x)
    128  64    1  d23     3.358e-04  2.939e-04 (0.88 x)  2.939e-04 (0.88 x)
    128  64    3  d23     3.300e-04  2.829e-04 (0.86 x)  2.829e-04 (0.86 x)
    128  192   1  d23     3.269e-04  2.825e-04 (0.86 x)  2.825e-04 (0.86 x)
    128  192   3  d23     3.267e-04  2.830e-04 (0.87 x)  2.830e-04 (0.87 x)
    128  1088  1  d23     3.277e-04  2.851e-04 (0.87 x)  2.851e-04 (0.87 x)
    128  1088  3  d23     3.253e-04  2.835e-04 (0.87 x)  2.835e-04 (0.87 x)
    128  64    1  e       3.548e-04  2.771e-04 (0.78 x)  2.771e-04 (0.78 x)
    128  64    3  e       3.558e-04  2.726e-04 (0.77 x)  2.726e-04 (0.77 x)
    128  192   1  e       3.507e-04  2.763e-04 (0.79 x)  2.763e-04 (0.79 x)
    128  192   3  e       3.500e-04  2.736e-04 (0.78 x)  2.736e-04 (0.78 x)
    128  1088  1  e       3.484e-04  2.718e-04 (0.78 x)  2.718e-04 (0.78 x)
    128  1088  3  e       3.517e-04  2.724e-04 (0.77 x)  2.724e-04 (0.77 x)
    worst product / floor: 1.28 x (bound 2 x); every d12 / d23 output finite

Before `vdx.vae.qk_fold` (to_q packed unscaled, all of 1/sqrt(C) applied by the softmax kernel) regimes a, b, c and e gave the
figures above to within 3 % and the d regimes NaN wherever a raw q.k exceeds 65504: the GEMM epilogue's fp32 -> fp16
conversion gives +-inf (it does not saturate: 64 products of 40 * 40 are stored as inf, of 40 * -40 as -inf), and
softmax_rows turns a row holding +inf into (inf - inf) * c = NaN.  Decoder table, the same inputs:

    C=512 S=64 n=1       d12  product nan        NaN in 30208 of 32768 outputs
    C=512 S=192 n=3      d12  product nan        NaN in 274944 of 294912 outputs
    C=512 S=1088 n=1     d12  product nan        NaN in 512000 of 557056 outputs
    C=512 S=64 n=1       d23  product nan        NaN in 32768 of 32768 outputs
    C=512 S=192 n=3      d23  product nan        NaN in 294912 of 294912 outputs
    C=512 S=1088 n=1     d23  product nan        NaN in 557056 of 557056 outputs
    C=128 S=64 n=1       d12  product 2.905e-04  NaN in 0 of 8192 outputs
    C=128 S=192 n=3      d12  product 2.876e-04  NaN in 0 of 73728 outputs
    C=128 S=1088 n=1     d12  product 2.869e-04  NaN in 0 of 139264 outputs
    C=128 S=64 n=1       d23  product nan        NaN in 4736 of 8192 outputs
    C=128 S=192 n=3      d23  product nan        NaN in 39296 of 73728 outputs
    C=128 S=1088 n=1     d23  product nan        NaN in 66048 of 139264 outputs

SOFTMAX_ROWS against fp64 torch.softmax within 2^-11 ref + 2^-24 (the fp16 rounding of the result plus half a subnormal step):
every case inside, the closest 3.0e-8 below the bound (rows with one dominant entry, the others in the subnormal range).
GROUPNORM: every case inside `close(tol=4e-3)`, batched samples bit-equal to themselves alone.  The whole module takes 9 s."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

import vae_blocks_ref as R
from test_ops_gpu import close, h

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# 1. _attention alone
ATT_CASES = [(C, regime, hw, n, table) for C, regime, hw, n, table in itertools.product(
    (512, 128), R.REGIMES, ((8, 8), (12, 16), (32, 34)), (1, 3), ("decoder", "encoder"))]      # S = 64, 192, 1088

_MODEL = {}


def _model(gpu, C, regime):
    """The product with both tables of `R.tables(C, regime)` loaded by its own loaders (one model alive at a time)."""
    import vdx  # noqa: F401
    from vdx.vae import AutoencoderKL, VaeConfig
    if (C, regime) not in _MODEL:
        _MODEL.clear()
        dec, enc, ch, layers = R.tables(C, regime)
        m = AutoencoderKL(VaeConfig(block_out_channels=ch, layers_per_block=layers))
        m.load_diffusers_state_dict(dec, device=gpu)
        m.load_diffusers_encoder_state_dict(enc, device=gpu)
        _MODEL[(C, regime)] = m
    return _MODEL[(C, regime)]


_REF = {}


def _reference(C, hw, n, regime):
    """One reference per case, shared by the two tables (they are adjacent in ATT_CASES) and then dropped."""
    key = (C, hw, n, regime)
    if key not in _REF:
        _REF.clear()
        _REF[key] = R.reference(C, hw, n, regime)
    return _REF[key]


@pytest.mark.parametrize("C,regime,hw,n,table", ATT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_attention_alone(gpu, C, regime, hw, n, table):
    m = _model(gpu, C, regime)
    x, want, floor = _reference(C, hw, n, regime)
    W = m.W if table == "decoder" else m.E
    xd = x.to(gpu)
    got = m._attention(f"{table}.{R.ATT}", xd, n, hw[0], hw[1], W).cpu()
    assert torch.equal(xd.cpu(), x)                                              # the input (also the residual) is not written
    err = R.rel_l2(got, want)
    print(f"attention {table} C={C} S={hw[0] * hw[1]} n={n} regime {regime}: floor {floor:.3e}  product {err:.3e}  "
          f"({err / floor:.2f} x)  finite {bool(torch.isfinite(got).all())}")
    assert got.shape == want.shape and got.dtype == torch.float16
    if regime.startswith("d"):
        assert torch.isfinite(got).all()
    assert err <= 2 * floor


# ---------------------------------------------------------------------------------------------------------------------
# 3. softmax_rows
SM_KINDS = ("equal", "dominant", "all_lowest", "mixed_extremes", "minus_inf", "underflow")


def _softmax_rows_input(kind, rows, cols, g):
    """(x [rows][cols] fp16 values as fp32, scale)."""
    if kind == "equal":
        return torch.full((rows, cols), 3.0), 0.5
    if kind == "dominant":                                   # the others land in fp16's subnormal range or below it
        x = torch.randn(rows, cols, generator=g)
        x[torch.arange(rows), torch.randint(cols, (rows,), generator=g)] = 16.0
        return x, 1.0
    if kind == "all_lowest":
        return torch.full((rows, cols), -65504.0), 1.0
    if kind == "mixed_extremes":
        return torch.where(torch.rand(rows, cols, generator=g) < 0.25, 65504.0, -65504.0), 1.0
    if kind == "minus_inf":
        x = torch.randn(rows, cols, generator=g) * 3
        x[torch.rand(rows, cols, generator=g) < 0.5] = float("-inf")
        x[:, cols // 2] = 1.0                                # at least one finite entry per row
        return x, 1.0 / math.sqrt(512)
    x = torch.randn(rows, cols, generator=g) * 6             # "underflow": adjacent fp16 values are >= 2^-14 * 2^20 apart
    return x, 2.0 ** 20


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("cols", [8, 64, 2048, 2056, 10240, 10248, 16384])       # NV = 1, 1, 1 | 2, 5 | 8, 8
def test_softmax_rows_edges(gpu, rows, cols):
    import vdx  # noqa: F401
    from vdx import ops
    g = torch.Generator().manual_seed(cols + rows)
    for kind in SM_KINDS:
        x, scale = _softmax_rows_input(kind, rows, cols, g)
        x = torch.cat([x, torch.full((rows, 8), 7.0)], 1).half()                 # ld = cols + 8
        scale = float(torch.tensor(scale, dtype=torch.float32))                  # what the C ABI receives
        ref = torch.softmax(x[:, :cols].double() * scale, dim=-1)
        d = x.to(gpu)
        ops.softmax_rows(d, rows=rows, cols=cols, scale=scale)
        out = d.cpu()
        assert torch.equal(out[:, cols:], x[:, cols:]), kind                     # columns past `cols` untouched
        got = out[:, :cols].double()
        assert torch.isfinite(got).all(), kind
        excess = (got - ref).abs() - (2.0 ** -11 * ref + 2.0 ** -24)
        print(f"softmax_rows {rows}x{cols} {kind}: worst err - bound {float(excess.max()):.3e}, row sums "
              f"{float(got.sum(1).min()):.6f}..{float(got.sum(1).max()):.6f}")
        assert excess.max() <= 0, (kind, float(excess.max()))
        if kind == "minus_inf":
            assert (got[x[:, :cols] == float("-inf")] == 0).all()
        if kind == "underflow":                                                  # the largest entries share 1, the rest is 0
            top = x[:, :cols] == x[:, :cols].max(1, keepdim=True).values
            assert (got[~top] == 0).all() and torch.equal(got[top], ref[top].half().double())


def test_softmax_rows_refusals(gpu):
    import vdx  # noqa: F401
    from vdx import ops
    from vdx._lib import VdxError
    x = torch.zeros(2, 16400, dtype=torch.float16, device=gpu)
    for cols, scale in ((12, 1.0), (16392, 1.0), (64, 0.0), (64, -1.0)):
        with pytest.raises(VdxError):
            ops.softmax_rows(x, rows=2, cols=cols, scale=scale)
    assert not x.any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. groupnorm as the VAE calls it
def _gn_ref(x, gamma, beta, ns, rps, silu, eps=1e-6):
    x3 = x.double().reshape(ns, rps, -1).permute(0, 2, 1)
    ref = F.group_norm(x3, 32, gamma.double(), beta.double(), eps)
    if silu:
        ref = F.silu(ref)
    return ref.permute(0, 2, 1).reshape(ns * rps, -1).float()


@pytest.mark.parametrize("rps", [64, 200, 4104])
@pytest.mark.parametrize("ns", [1, 3, 8, 9])
@pytest.mark.parametrize("C", [128, 256, 512])
def test_groupnorm_as_the_vae_calls_it(gpu, C, ns, rps):
    import vdx  # noqa: F401
    from vdx import ops
    g = torch.Generator().manual_seed(C + 3 * ns + rps)
    x = h(torch.randn(ns * rps, C, generator=g) * 2 + torch.randn(1, C, generator=g))
    gamma, beta = h(1 + 0.2 * torch.randn(C, generator=g)), h(0.3 * torch.randn(C, generator=g))
    xd, gd, bd = x.half().to(gpu), gamma.half().to(gpu), beta.half().to(gpu)
    for silu in (False, True):
        out = ops.groupnorm(xd, gd, bd, groups=32, n_samples=ns, rows_per_sample=rps, eps=1e-6, silu_act=silu, partition_samples=8)
        close(out, _gn_ref(x, gamma, beta, ns, rps, silu), tol=4e-3)
        for i in {0, ns - 1}:                                # a sample alone has the bits of its batched self
            one = ops.groupnorm(xd[i * rps:(i + 1) * rps], gd, bd, groups=32, n_samples=1, rows_per_sample=rps, eps=1e-6,
                                silu_act=silu, partition_samples=8)
            assert torch.equal(one, out[i * rps:(i + 1) * rps]), (silu, i)


def test_groupnorm_variance_below_eps(gpu):
    """Every group alternates (three rows at a time, and from channel to channel) between 1 and 1 + 2^-10, adjacent fp16
    values: its variance of about 2^-22 = 2.4e-7 is below the VAE's eps = 1e-6, so the normalised values are +-0.44 and a
    kernel that used 1e-5 (+-0.15) or dropped eps (+-1) is far out."""
    import vdx  # noqa: F401
    from vdx import ops
    g = torch.Generator().manual_seed(12)
    C, ns, rps = 512, 2, 200
    r, c = torch.arange(ns * rps)[:, None], torch.arange(C)[None, :]
    x = 1.0 + 2.0 ** -10 * ((r // 3 + c) % 2).float()
    gamma, beta = h(1 + 0.2 * torch.randn(C, generator=g)), h(0.3 * torch.randn(C, generator=g))
    ref = _gn_ref(x, gamma, beta, ns, rps, False)
    assert 0.40 < float(_gn_ref(x, torch.ones(C), torch.zeros(C), ns, rps, False).abs().max()) < 0.48
    out = ops.groupnorm(x.half().to(gpu), gamma.half().to(gpu), beta.half().to(gpu), groups=32, n_samples=ns, rows_per_sample=rps,
                        eps=1e-6, silu_act=False, partition_samples=8)
    close(out, ref, tol=4e-3)
