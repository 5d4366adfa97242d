"""Test infrastructure for tests/test_attn_regimes_gpu.py and tests/test_attn_regimes_host.py: seeded inputs that put the
attention sub-block kernels (csrc/attn.hip core, csrc/tattn_fused.hip K7, csrc/tattn2.hip K7b, csrc/xattn.hip K5) into the
regimes their sibling tests in tests/test_ops_gpu.py never reach, and two references of each sub-block.  Not product code.

`exact_*`    float64 statements of `s + attn(LN(s))` over the frames of a pixel and of
             `t + attn2(norm2(t), text)`, evaluated from the fp16-rounded inputs: the math of
             `_temporal_block_ref` / `_cross_block_ref` of tests/test_ops_gpu.py.
`rounded_*`  the same math in fp32 with an fp16 rounding wherever the kernel rounds:
             K7b / K5  x^ = h(x.rstd - mean.rstd);  W_q' = h(c.W_q.diag(gamma)), c = scale.log2 e, W_k' = h(W_k.diag(gamma)),
                       W_v' = h(W_v.diag(gamma));  q = h(x^.W_q'^T + c.W_q.beta), k = h(x^.W_k'^T), v = h(x^.W_v'^T)
                       (K5: k, v = h(text.W^T));  P = h(exp2(s - max) / sum);  o = h(P.v);
                       out = h(h(o.W_o^T + b_o') + t), b_o' = b_o + W_o.W_v.beta (K5: b_o).
             K7        ln = h((x - mean).rstd.gamma + beta);  q, k, v = h(ln.W^T);  P = h(exp2(c.s - c.max) / sum);
                       o = h(P.v);  out = h(o.W_o^T + b_o + t).
             core      the K7 softmax on given fp16 q|k|v rows;  out = h(P.v).

Regimes (weights: the sibling test's seeded draw, multiplied where stated):
  ordinary      the sibling test's inputs (t = randn * 1.5 + 0.3).
  one_hot       W_q * 32, W_k * 32: powers of two, so the weights stay exact in fp16; scores then spread over thousands of
                nats.  The factors alone cannot make the regime fair: both the gap between a pair's two top scores and
                the error the fp16 roundings of LayerNorm's output, q and k leave in a score grow with the factors, so at
                any factor a share of the (query, head) pairs of a plain draw has its winner moved or flipped by the
                roundings, and `rounded` itself misses the bound by a factor of 2 to 24 (measured with W_q * 8, W_k * 32: 97
                to 99 % one-hot, every fused kernel over the bound at most shapes).  So the rows are SELECTED: seeded candidates — whole
                pixels for the temporal kernels, query rows for K5 — are drawn as the sibling test draws them and kept only
                if every (query, head) pair of theirs has a margin >= MARGIN = 10 nats in float64.  In `exact` every pair
                (at least the 90 % asked for) then carries a top weight >= 0.999 with that margin.
  two_way_tie   one_hot with every frame row (temporal: frame f + F/2 = frame f) or text token (K5: token j + kv_len // 2 =
                token j) appearing twice, bit for bit: the two top weights of every (query, head) pair are equal, and the
                margin is the pair's over the third.  An odd kv_len leaves one last token; it is all zeros (key 0, value 0:
                a real key whose score is exactly 0).  Note what the regime can and cannot see: the two keys of a pair carry
                the same v, so it checks that equal scores give equal weights through max / exp2 / sum / rounding, not
                that both keys are counted — that is what flat and the bit-for-bit mask tests are for.
  outlier_rows  sibling weights; t = randn * 0.5 + 20 with four channels of every row at +-300.
  flat          W_q = 0: every weight is exactly 1 / (number of real keys).

`err_over_bound(out, ref, tol)` is the `close()` formula of tests/test_ops_gpu.py as a ratio: max of
|out - ref| / (tol.max|ref| + tol.|ref|).  The kernels are held to ratio <= 1 against `exact` at the sibling tests' tol
(4e-3 temporal, 5e-3 K5); tests/test_attn_regimes_host.py holds `rounded` to <= 0.5, which is what makes that bound fair in
the peaked regimes.  Measured `rounded`-vs-`exact` ratios (max over the shapes of the regime; pytest -s
tests/test_attn_regimes_host.py prints every case):

  kernel          ordinary       one_hot   two_way_tie  outlier_rows          flat
  core               0.071         0.017         0.002         0.065         0.071
  k7-320             0.112         0.062         0.057         0.052         0.059
  k7-512             0.188         0.100         0.125         0.052         0.057
  k7b                0.139         0.082         0.075         0.053         0.064
  k5                 0.066         0.053         0.051         0.042         0.039
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

LOG2E = 1.4426950408889634
SCALE = 0.125
EPS = 1e-5
REGIMES = ("one_hot", "two_way_tie", "outlier_rows", "flat")
TEMPORAL_SHAPES = [(2, 24, 5), (1, 16, 7), (2, 4, 9), (1, 2, 13), (1, 48, 3)]          # (B, F, HW)
CROSS_SHAPES = [(2, 50, 77), (1, 200, 16), (2, 70, 17)]                                 # (n_items, rows, kv_len)
TOL = {"core": 4e-3, "k7": 4e-3, "k7b": 4e-3, "k5": 5e-3}                              # the sibling tests' close() tol
ONE_HOT_FACTORS = {"temporal": (32.0, 32.0), "cross": (32.0, 32.0)}                    # (W_q, W_k)
MARGIN = 10.0                                                                           # nats
CROSS, PAD = 128, 128                                                                   # text width, padded text length


def h(x):
    """fp16-rounded fp32 tensor."""
    return x.half().float()


def err_over_bound(out, ref, tol):
    out, ref = out.double().cpu(), ref.double()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    scale = ref.abs().max().item() + 1e-6
    return float(((out - ref).abs() / (tol * scale + tol * ref.abs())).max())


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _outlier_rows(M, inner, g):
    t = torch.randn(M, inner, generator=g) * 0.5 + 20.0
    for r in range(M):
        ch = torch.randperm(inner, generator=g)[:4]
        sign = torch.randint(0, 2, (4,), generator=g).float() * 2 - 1
        t[r, ch] = 300.0 * sign
    return h(t)


def _margin(s, tie):
    """Scores [..][k] -> the winner's lead over the runner-up; two_way_tie: the lead of the second best over the third, which
    is the winning pair's lead (and 0 where a single key, the zero token an odd text ends in, beats a pair)."""
    rank = 2 if tie else 1
    if s.shape[-1] <= rank:
        return torch.full(s.shape[:-1], float("inf"), dtype=s.dtype)
    v = s.topk(rank + 1, dim=-1).values
    return v[..., rank - 1] - v[..., rank]


def _accept(g, n, draw, margins):
    """The first n of the seeded candidates `draw(g)` [batch][...] whose every (query, head) margin is >= MARGIN."""
    got = []
    for _ in range(400):
        cand = draw(g)
        ok = (margins(cand) >= MARGIN).flatten(1).all(1)
        got.extend(cand[ok])
        if len(got) >= n:
            return torch.stack(got[:n])
    raise AssertionError("the regime's factors leave too few candidates with the margin")


@functools.lru_cache(maxsize=None)
def temporal_case(regime, inner, B, Fr, HW):
    """The sibling tests' draw (seed inner + F + HW, same order) put into `regime`."""
    g = torch.Generator().manual_seed(inner + Fr + HW)
    M, heads = B * Fr * HW, inner // 64
    t = h(torch.randn(M, inner, generator=g) * 1.5 + 0.3)
    gamma, beta = h(1 + 0.2 * torch.randn(inner, generator=g)), h(0.1 * torch.randn(inner, generator=g))
    wq, wk, wv, wo = (h(torch.randn(inner, inner, generator=g) * s_) for s_ in (0.09, 0.09, 0.06, 0.05))
    bo = h(0.1 * torch.randn(inner, generator=g))
    if regime in ("one_hot", "two_way_tie"):
        tie = regime == "two_way_tie"
        assert Fr % 2 == 0 or not tie
        fq, fk = ONE_HOT_FACTORS["temporal"]
        wq, wk = wq * fq, wk * fk
        d = lambda x: x.double()   # noqa: E731

        def draw(g):               # 16 candidate pixels [F][inner]; two_way_tie: frame f + F/2 = frame f
            x = h(torch.randn(16, Fr // 2 if tie else Fr, inner, generator=g) * 1.5 + 0.3)
            return torch.cat([x, x], 1) if tie else x

        def margins(x):
            ln = F.layer_norm(d(x), (inner,), d(gamma), d(beta), EPS)
            s = _split(ln @ d(wq).t(), heads) @ _split(ln @ d(wk).t(), heads).transpose(-1, -2) * SCALE
            return _margin(s, tie)

        t = _unseq(_accept(g, B * HW, draw, margins), B, Fr, HW).contiguous()
    elif regime == "outlier_rows":
        t = _outlier_rows(M, inner, g)
    elif regime == "flat":
        wq = torch.zeros_like(wq)
    else:
        assert regime == "ordinary", regime
    return SimpleNamespace(regime=regime, inner=inner, heads=heads, B=B, F=Fr, HW=HW, M=M, t=t, gamma=gamma, beta=beta,
                           wq=wq, wk=wk, wv=wv, wo=wo, bo=bo)


@functools.lru_cache(maxsize=None)
def cross_case(regime, n_items, rows, kv_len):
    """The sibling test's draw (seed n_items + rows + kv_len, same order) put into `regime`."""
    inner, heads = 320, 5
    g = torch.Generator().manual_seed(n_items + rows + kv_len)
    M = n_items * rows
    t = h(torch.randn(M, inner, generator=g) * 1.5 + 0.3)
    gamma, beta = h(1 + 0.2 * torch.randn(inner, generator=g)), h(0.1 * torch.randn(inner, generator=g))
    wq, wo = h(torch.randn(inner, inner, generator=g) * 0.09), h(torch.randn(inner, inner, generator=g) * 0.05)
    wk, wv = h(torch.randn(inner, CROSS, generator=g) * 0.12), h(torch.randn(inner, CROSS, generator=g) * 0.09)
    bo = h(0.1 * torch.randn(inner, generator=g))
    ehs = h(torch.randn(n_items, kv_len, CROSS, generator=g))
    if regime in ("one_hot", "two_way_tie"):
        tie = regime == "two_way_tie"
        fq, fk = ONE_HOT_FACTORS["cross"]
        wq, wk = wq * fq, wk * fk
        if tie:
            half = kv_len // 2
            ehs[:, half:2 * half] = ehs[:, :half]
            ehs[:, 2 * half:] = 0.0
        d = lambda x: x.double()   # noqa: E731
        items = []
        for i in range(n_items):
            k = _split((d(ehs[i]) @ d(wk).t())[None], heads)                    # [1][heads][kv][64]

            def margins(x):        # x: candidate rows [64][inner]
                ln = F.layer_norm(d(x), (inner,), d(gamma), d(beta), EPS)
                q = _split((ln @ d(wq).t())[None], heads)
                return _margin(q @ k.transpose(-1, -2) * SCALE, tie)[0].t()    # [row][head]

            items.append(_accept(g, rows, lambda g: h(torch.randn(64, inner, generator=g) * 1.5 + 0.3), margins))
        t = torch.cat(items)
    elif regime == "outlier_rows":
        t = _outlier_rows(M, inner, g)
    elif regime == "flat":
        wq = torch.zeros_like(wq)
    else:
        assert regime == "ordinary", regime
    return SimpleNamespace(regime=regime, inner=inner, heads=heads, n_items=n_items, rows=rows, kv_len=kv_len, M=M, t=t,
                           gamma=gamma, beta=beta, wq=wq, wk=wk, wv=wv, wo=wo, bo=bo, ehs=ehs)


def padded_text(c):
    """The text zero-padded to PAD slots per item, [n_items * PAD][CROSS]: what the un-fused path multiplies by W_k / W_v."""
    p = torch.zeros(c.n_items * PAD, CROSS)
    p.view(c.n_items, PAD, CROSS)[:, :c.kv_len] = c.ehs
    return p


def fill_padding(k_rows, vt, n_items, kv_len, seed):
    """Copies of k_rows [n_items*PAD][inner] and vt [inner][n_items*PAD] with every slot at or past kv_len holding seeded
    finite values of magnitude 50 .. 100 and the real slots untouched."""
    g = torch.Generator().manual_seed(seed)
    inner = k_rows.shape[1]

    def junk(*shape):
        mag = 50.0 + 50.0 * torch.rand(*shape, generator=g)
        sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
        return (mag * sign).to(dtype=k_rows.dtype, device=k_rows.device)

    k2, v2 = k_rows.clone(), vt.clone()
    k2.view(n_items, PAD, inner)[:, kv_len:] = junk(n_items, PAD - kv_len, inner)
    v2.view(inner, n_items, PAD)[:, :, kv_len:] = junk(inner, n_items, PAD - kv_len)
    return k2, v2


def redraw_except(t, keep_rows, seed, gain=4.0):
    """t with every row outside `keep_rows` replaced by another seeded draw scaled by `gain` (fp16 values)."""
    g = torch.Generator().manual_seed(seed)
    t2 = h(torch.randn(t.shape, generator=g) * gain)
    t2[keep_rows] = t[keep_rows]
    return t2


def pixel_rows(B, Fr, HW, b, pixels):
    """Row indices (b * F + f) * HW + p of the given pixels of item b, frame-major."""
    return torch.tensor([(b * Fr + f) * HW + p for f in range(Fr) for p in pixels])


# ---------------------------------------------------------------------------------------------
# float64 statements
# ---------------------------------------------------------------------------------------------
def _seq(x, B, Fr, HW):
    return x.reshape(B, Fr, HW, -1).permute(0, 2, 1, 3).reshape(B * HW, Fr, -1)


def _unseq(o, B, Fr, HW):
    return o.reshape(B, HW, Fr, -1).permute(0, 2, 1, 3).reshape(B * Fr * HW, -1)


def _split(x, heads):                      # [n][s][heads * 64] -> [n][heads][s][64]
    return x.reshape(x.shape[0], x.shape[1], heads, 64).permute(0, 2, 1, 3)


def _merge(o):                             # [n][heads][s][64] -> [n][s][heads * 64]
    return o.permute(0, 2, 1, 3).reshape(o.shape[0], o.shape[2], -1)


def _scores(q, k):
    """q.k^T summed element by element: every score is the same sequence of operations on its own q and k rows, so equal
    key rows give equal bits (a blocked matrix product promises no such thing)."""
    return (q.unsqueeze(-2) * k.unsqueeze(-3)).sum(-1)


def _linear(x, w):
    """x.w^T one row at a time (a batch of equal-shaped products): equal rows of x give equal bits wherever they sit."""
    lead = x.shape[:-1]
    x = x.reshape(-1, 1, x.shape[-1])
    return torch.bmm(x, w.t().expand(x.shape[0], -1, -1)).reshape(*lead, w.shape[0])


def _attn64(q, k, v, heads):
    s = _scores(_split(q, heads), _split(k, heads)) * SCALE
    p = torch.softmax(s, dim=-1)
    return _merge(p @ _split(v, heads)), p, s


def core_qkv(c):
    """fp16 q|k|v rows [M][3 * inner] of a temporal case: what the un-fused chain hands to ops.temporal_attn."""
    d = lambda x: x.double()   # noqa: E731
    ln = F.layer_norm(d(c.t), (c.inner,), d(c.gamma), d(c.beta), EPS)
    return h(_linear(ln, d(torch.cat([c.wq, c.wk, c.wv], 0))).float())


def exact_core(qkv, B, Fr, HW, heads):
    """-> (out [M][inner], P [B*HW][heads][F][F], scores in nats)."""
    inner = heads * 64
    x = _seq(qkv.double(), B, Fr, HW)
    o, p, s = _attn64(x[..., :inner], x[..., inner:2 * inner], x[..., 2 * inner:], heads)
    return _unseq(o, B, Fr, HW), p, s


def exact_temporal(c):
    """-> (out [M][inner], P [B*HW][heads][F][F], scores in nats)."""
    d = lambda x: x.double()   # noqa: E731
    t = d(c.t)
    ln = F.layer_norm(t, (c.inner,), d(c.gamma), d(c.beta), EPS)
    sq = lambda w: _seq(_linear(ln, d(w)), c.B, c.F, c.HW)   # noqa: E731
    o, p, s = _attn64(sq(c.wq), sq(c.wk), sq(c.wv), c.heads)
    return t + _unseq(o, c.B, c.F, c.HW) @ d(c.wo).t() + d(c.bo), p, s


def exact_cross(c):
    """-> (out [M][inner], P [n_items][heads][rows][kv_len], scores in nats)."""
    d = lambda x: x.double()   # noqa: E731
    t = d(c.t)
    ln = F.layer_norm(t, (c.inner,), d(c.gamma), d(c.beta), EPS)
    q = _linear(ln, d(c.wq)).reshape(c.n_items, c.rows, c.inner)
    o, p, s = _attn64(q, _linear(d(c.ehs), d(c.wk)), _linear(d(c.ehs), d(c.wv)), c.heads)
    return t + o.reshape(c.M, c.inner) @ d(c.wo).t() + d(c.bo), p, s


# ---------------------------------------------------------------------------------------------
# fp32 with the kernels' roundings
# ---------------------------------------------------------------------------------------------
def _centred(t):
    mean = t.mean(1, keepdim=True)
    rstd = torch.rsqrt(((t - mean) ** 2).mean(1, keepdim=True) + EPS)
    return mean, rstd


def _softmax_pv(s2, v):
    """s2: scores in log2 units [..][q][k]; v [..][k][64] -> h(P.v) with P = h(exp2(s - max) / sum)."""
    e = torch.exp2(s2 - s2.max(-1, keepdim=True).values)
    return h(h(e / e.sum(-1, keepdim=True)) @ v)


def rounded_core(qkv, B, Fr, HW, heads):
    inner = heads * 64
    x = _seq(qkv.float(), B, Fr, HW)
    q, k, v = (_split(x[..., i * inner:(i + 1) * inner], heads) for i in range(3))
    o = _softmax_pv((q @ k.transpose(-1, -2)) * (SCALE * LOG2E), v)
    return _unseq(_merge(o), B, Fr, HW)


def rounded_k7(c):
    mean, rstd = _centred(c.t)
    ln = h((c.t - mean) * rstd * c.gamma + c.beta)
    sq = lambda w: _split(_seq(h(ln @ w.t()), c.B, c.F, c.HW), c.heads)   # noqa: E731
    o = _softmax_pv((sq(c.wq) @ sq(c.wk).transpose(-1, -2)) * (SCALE * LOG2E), sq(c.wv))
    return h(_unseq(_merge(o), c.B, c.F, c.HW) @ c.wo.t() + c.bo + c.t)


def _folded_q(c, xn):
    cc = SCALE * LOG2E
    return h(xn @ h(c.wq * c.gamma[None, :] * cc).t() + cc * (c.wq @ c.beta))


def rounded_k7b(c):
    mean, rstd = _centred(c.t)
    xn = h(c.t * rstd - mean * rstd)
    sq = lambda x: _split(_seq(x, c.B, c.F, c.HW), c.heads)   # noqa: E731
    q = sq(_folded_q(c, xn))
    k = sq(h(xn @ h(c.wk * c.gamma[None, :]).t()))
    v = sq(h(xn @ h(c.wv * c.gamma[None, :]).t()))
    o = _unseq(_merge(_softmax_pv(q @ k.transpose(-1, -2), v)), c.B, c.F, c.HW)
    bo2 = c.bo + c.wo @ (c.wv @ c.beta)
    return h(h(o @ c.wo.t() + bo2) + c.t)


def rounded_k5(c):
    mean, rstd = _centred(c.t)
    xn = h(c.t * rstd - mean * rstd)
    q = _split(_folded_q(c, xn).reshape(c.n_items, c.rows, c.inner), c.heads)
    k = _split(h(c.ehs @ c.wk.t()), c.heads)
    v = _split(h(c.ehs @ c.wv.t()), c.heads)
    o = _merge(_softmax_pv(q @ k.transpose(-1, -2), v)).reshape(c.M, c.inner)
    return h(h(o @ c.wo.t() + c.bo) + c.t)


def top_two(p):
    """Softmax weights [..][k] -> (largest, second largest, index of the largest); k = 1 has second largest 0."""
    if p.shape[-1] == 1:
        return p[..., 0], torch.zeros_like(p[..., 0]), torch.zeros(p.shape[:-1], dtype=torch.long)
    v, i = p.topk(2, dim=-1)
    return v[..., 0], v[..., 1], i[..., 0]


def one_hot_share(p, s):
    """Share of (query, head) pairs whose top weight is >= 0.999 with a margin to the runner-up score of >= 10 nats."""
    w1, _, _ = top_two(p)
    sv = s.topk(2, dim=-1).values
    return float(((w1 >= 0.999) & (sv[..., 0] - sv[..., 1] >= 10.0)).double().mean())


