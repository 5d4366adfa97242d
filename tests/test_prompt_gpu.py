"""-m gpu: `ops.prompt_weight` (csrc/prompt.hip) against tests/prompt_ref.py, bit for bit, at every lane width (D % 8, D % 4, odd D, an
unaligned base), every n_tok edge (1, 76, 77) and one, three and nine sequences (more blocks than one), with weights drawn from
{0, 0.55, 1.0, 1.1^3, -1}; in place; a canary behind `out`; run to run; a sequence of NaN / inf / -0 beside clean ones; all-ones
weights launch nothing.  Inputs keep |z| <= 64, so the fp64 sums of at most 77 x 1024 fp16 values are exact (checked on the CPU for
every input, `prompt_ref.sums_are_exact`) and the reference does not depend on the order of summation: no tolerance.  A NaN has no
one bit pattern (the CPU and the GPU sign their default NaN differently): where the expression gives a NaN both must hold one,
everything else is compared as bits."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prompt_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
WEIGHTS = (0.0, 0.55, 1.0, 1.1 * 1.1 * 1.1, -1.0)


def make(n_seq, n_tok, D, seed):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(n_seq, n_tok, D, generator=g) * 8).clamp(-64, 64).half()
    w = torch.tensor(WEIGHTS, dtype=torch.float32)[torch.randint(0, len(WEIGHTS), (n_seq, n_tok), generator=g)]
    w[:, 0] = WEIGHTS[1 + seed % 2 * 2]                                           # every sequence carries a weight other than 1.0 (and 0)
    assert bool(R.sums_are_exact(z, w).all())
    return z, w


def same(got, want):
    """Bit for bit; where the expression gives a NaN, a NaN."""
    got, want = got.cpu(), want.cpu()
    nan = torch.isnan(want)
    return bool(torch.equal(torch.isnan(got), nan)) and bool(torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]))


@pytest.mark.parametrize("D", [1, 2, 4, 8, 120, 128, 1024])
def test_kernel_equals_the_restatement_bit_for_bit(gpu, D):
    from vdx import ops
    for n_tok in (1, 76, 77):
        for n_seq in (1, 3, 9):
            z, w = make(n_seq, n_tok, D, seed=D + 7 * n_tok + n_seq)
            got = ops.prompt_weight(z.to(gpu), w)
            assert got.dtype == torch.float16 and tuple(got.shape) == (n_seq, n_tok, D)
            assert same(got, R.weight(z, w)), (D, n_tok, n_seq)
            assert same(ops.prompt_weight(z.to(gpu), w.to(gpu)), got)             # weights handed over on the device


@pytest.mark.parametrize("D,offset", [(1024, 1), (1024, 4), (120, 1), (120, 4), (4, 2)])
def test_unaligned_base_takes_the_narrower_lanes(gpu, D, offset):
    """z and out `offset` elements into their buffers: 2 bytes off takes the one-element lanes, 8 bytes off the 8-byte ones."""
    from vdx import ops
    z, w = make(3, 77, D, seed=offset)
    buf = torch.zeros(z.numel() + 16, dtype=torch.float16, device=gpu)
    zin = buf[offset:offset + z.numel()].view(z.shape)
    zin.copy_(z)
    obuf = torch.full((z.numel() + 16,), 7.0, dtype=torch.float16, device=gpu)
    out = obuf[offset:offset + z.numel()].view(z.shape)
    assert zin.data_ptr() % 16 == 2 * offset and zin.is_contiguous()
    assert ops.prompt_weight(zin, w, out=out) is out and same(out, R.weight(z, w))
    assert bool((obuf[:offset] == 7.0).all()) and bool((obuf[offset + z.numel():] == 7.0).all())       # the canary, both sides


def test_in_place_canary_and_run_to_run(gpu):
    from vdx import ops
    z, w = make(9, 77, 1024, seed=5)
    want = R.weight(z, w)
    buf = torch.full((z.numel() + 4096,), -3.0, dtype=torch.float16, device=gpu)
    zin = buf[:z.numel()].view(z.shape)
    zin.copy_(z)
    first = ops.prompt_weight(zin, w)
    second = ops.prompt_weight(zin, w)
    assert same(first, want) and torch.equal(first.view(torch.int16), second.view(torch.int16))
    assert ops.prompt_weight(zin, w, out=zin) is zin and same(zin, want)          # out may be z
    assert bool((buf[z.numel():] == -3.0).all())


def test_a_sequence_of_nan_inf_and_minus_zero_stays_in_its_sequence(gpu):
    from vdx import ops
    z, w = make(3, 77, 128, seed=11)
    clean = R.weight(z, w)
    z[1, 3, 5], z[1, 10, 0], z[1, 20, 7] = float("nan"), float("inf"), -0.0
    got = ops.prompt_weight(z.to(gpu), w)
    assert same(got[0], clean[0]) and same(got[2], clean[2])
    assert same(got[1], R.weight(z, w)[1]) and bool(torch.isnan(got[1]).any())
    # m1 = 0: the only token at weight 0 gives y = 0 and r = m0 / 0, what the lines give, with no branch
    z1, w1 = torch.full((2, 1, 8), 2.0).half(), torch.tensor([[0.0], [0.55]])
    assert same(ops.prompt_weight(z1.to(gpu), w1), R.weight(z1, w1))


def test_all_ones_launch_nothing_and_mixed_batches_keep_the_encoders_bits(gpu, monkeypatch):
    from vdx import ops
    launched = []
    launch = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda sym, *a: (launched.append((sym, a[3])), launch(sym, *a))[1])
    z, w = make(4, 77, 128, seed=2)
    zg = z.to(gpu)
    ones = torch.ones_like(w)
    assert ops.prompt_weight(zg, ones) is zg and launched == []
    out = torch.empty_like(zg)
    assert ops.prompt_weight(zg, ones, out=out) is out and torch.equal(out, zg) and launched == []
    w[1] = 1.0
    w[3] = 1.0
    got = ops.prompt_weight(zg, w)
    assert launched == [("vdx_prompt_weight_f16", 2)]                             # one launch, the two weighted sequences
    want = R.weight(z, w)
    assert torch.equal(got[1].view(torch.int16), zg[1].view(torch.int16)) and torch.equal(got[3].view(torch.int16), zg[3].view(torch.int16))
    assert same(got[0], want[0]) and same(got[2], want[2])
    assert torch.equal(zg.cpu().view(torch.int16), z.view(torch.int16))           # the input is left alone


def test_host_refusals(gpu):
    from vdx import ops
    from vdx._lib import VdxError
    z = torch.zeros(2, 77, 8, dtype=torch.float16, device=gpu)
    w = torch.full((2, 77), 1.1)
    for bad_z in (torch.zeros(2, 78, 8, dtype=torch.float16, device=gpu), torch.zeros(2, 0, 8, dtype=torch.float16, device=gpu),
                  torch.zeros(2, 77, 0, dtype=torch.float16, device=gpu), z.float(), z.cpu(), z.transpose(0, 1)):
        with pytest.raises(VdxError):
            ops.prompt_weight(bad_z, torch.full((bad_z.shape[0], bad_z.shape[1]), 1.1))
    for bad in (float("nan"), float("inf"), -float("inf")):
        wb = w.clone()
        wb[1, 5] = bad
        with pytest.raises(VdxError, match="not finite"):
            ops.prompt_weight(z, wb)
    with pytest.raises(VdxError):
        ops.prompt_weight(z, w[:, :76])
    with pytest.raises(VdxError):
        ops.prompt_weight(z, w.double())
    with pytest.raises(VdxError):
        ops.prompt_weight(z, w, out=torch.empty(2, 77, 4, dtype=torch.float16, device=gpu))
