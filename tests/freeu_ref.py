"""FreeU (Si et al. 2023; diffusers' `apply_freeu` / `fourier_filter`) restated on the CPU (not a test): the skip filter in
float64 with torch.fft, literally in the SHIFT form of the published definition, the backbone scale as torch's half-by-scalar
multiply, and the oracle's up blocks 0 and 1 with the two FreeU lines inserted.  The kernels (csrc/freeu.hip) run the
projection form below, so the literal form is an independent route to the same numbers."""
import math
import types

import numpy as np
import torch

DIMS = (-2, -1)


def fourier_filter_ref(x, s):
    """Re ifft2(ifftshift(fftshift(fft2(x)) M)) over the last two axes in float64, M = 1 except
    M[cr - 1 : cr + 1, cc - 1 : cc + 1] = s with cr = H // 2, cc = W // 2 and Python's slice semantics (threshold = 1)."""
    x = x.double()
    H, W = x.shape[-2:]
    f = torch.fft.fftshift(torch.fft.fft2(x, dim=DIMS), dim=DIMS)
    mask = torch.ones((H, W), dtype=torch.float64)
    cr, cc = H // 2, W // 2
    mask[cr - 1:cr + 1, cc - 1:cc + 1] = s
    return torch.fft.ifft2(torch.fft.ifftshift(f * mask, dim=DIMS), dim=DIMS).real


def masked_frequencies(n):
    """K_N: the frequencies of an axis of length n that the 2-wide centre of the shifted mask covers: 0 and -1 mod n."""
    return sorted({0, (n - 1) % n})


def unit_roots(n):
    """e^{-2 pi i j / n} for j < n, complex128, with the multiples of a quarter turn exact (math.sin(math.pi) is 1.2e-16)."""
    j = torch.arange(n, dtype=torch.float64)
    w = torch.complex(torch.cos(2.0 * math.pi * j / n), -torch.sin(2.0 * math.pi * j / n))
    for q in range(n):
        if 4 * q % n == 0:
            w[q] = (1.0, -1j, -1.0, 1j)[4 * q // n]
    return w


def fourier_filter_projection(x, s):
    """x + (s - 1) / (H W) Re sum_{ky in K_H, kx in K_W} X(ky, kx) e^{+2 pi i (ky y / H + kx x / W)}, float64: what the
    kernel computes, written with explicit sums; the roots of unity are indexed by (k n) mod N."""
    x = x.double()
    H, W = x.shape[-2:]
    wh, ww = unit_roots(H), unit_roots(W)
    corr = torch.zeros_like(x)
    for ky in masked_frequencies(H):
        for kx in masked_frequencies(W):
            f = wh[(ky * torch.arange(H)) % H][:, None] * ww[(kx * torch.arange(W)) % W][None, :]
            X = (x * f).sum(dim=DIMS, keepdim=True)
            corr = corr + (X * f.conj()).real
    return x + (s - 1.0) / (H * W) * corr


def scale_ref(x16, b):
    """The backbone scale: channels [0, C // 2) of fp16 rows [M][C] times b, fp16(fp32(x) fp32(b)) as torch's CPU half multiply
    forms it; the other channels unchanged.  -> a new tensor."""
    out = x16.clone()
    half = x16.shape[-1] // 2
    out[..., :half] = x16[..., :half] * b
    return out


def to_fp16(x64):
    """float64 -> fp16 with ONE rounding (numpy's; torch would go through fp32 for some paths)."""
    return torch.from_numpy(x64.numpy().astype(np.float16))


# float64 routes to the same plane (torch.fft, the explicit sums, the kernels' order) differ by at most 2e-14 on the planes used
# here (values up to about 8, at most 576 positions: tests/test_freeu_host.py measures the first two); a restated value this
# far from an fp16 rounding boundary rounds the same way on every route
TIE_DISTANCE = 1e-12


def tie_distance(x64):
    """Per element, the absolute distance between a float64 value and the nearest boundary between two fp16 roundings."""
    a = x64.double().abs()
    ulp = torch.exp2(torch.floor(torch.log2(a.clamp_min(2.0 ** -14))) - 10)
    return (torch.remainder(a / ulp, 1.0) - 0.5).abs() * ulp


PLANES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (2, 4), (4, 8), (5, 9), (9, 16), (18, 32)]
_CASES = {}


def make_case(H, W, C, n_img, s, seed=0):
    """-> (x fp16 (n_img, C, H, W), want fp16, want float64), computed once per argument set and shared (do not write to them).
    x is seeded N(0, 1) plus a per-plane offset in [-4, 4], so the DC term matters.  A plane the mask covers whole (N <= 2 on
    both axes) is s x, and s x of an fp16 x can be an exact tie (0.9 x 1145 = 1030.5), which the last bit of each float64 route
    would decide: where the restatement lies within TIE_DISTANCE of a rounding boundary the INPUT element there is moved by
    one fp16 step and the restatement taken again, until no such element is left.  With s = 0 (dyadic, and every term of a
    small plane dyadic too) a tie can be exact on every route and then rounds half-to-even on all of them: a tie at which the
    two float64 routes give the same double is kept, any other is moved away like the rest."""
    key = (H, W, C, n_img, s, seed)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(1000 * H + 10 * W + C + seed)
    x = (torch.randn(n_img, C, H, W, generator=g) + (torch.rand(n_img, C, 1, 1, generator=g) * 8 - 4)).half()
    for _ in range(64):
        want64 = fourier_filter_ref(x, s)
        near = tie_distance(want64) < TIE_DISTANCE
        if s == 0.0:                                           # an exact tie is one both float64 routes hit with the same double
            near &= want64 != fourier_filter_projection(x, s)
        if not near.any():
            break
        bits = x.view(torch.int16)
        bits[near] += 1                                        # the next fp16 away from zero
    else:
        raise AssertionError(f"make_case{key}: ties left after 64 rounds")
    assert torch.isfinite(x.float()).all()
    _CASES[key] = (x, to_fp16(want64), want64)
    return _CASES[key]


def differing(got16, want16):
    """Elements whose fp16 values differ: NaN equals NaN, and the two zeros are one value (the exact expression has no signed
    zero: where it is 0 the restatement's sign is whatever its FFT's arithmetic left, -0 for some 2 x 2 planes at s = 0)."""
    return int(((got16 != want16) & ~(got16.isnan() & want16.isnan())).sum())


def rows_to_planes(rows, n_img, H, W):
    """[n_img H W][C] -> (n_img, C, H, W)"""
    return rows.reshape(n_img, H, W, -1).permute(0, 3, 1, 2)


def planes_to_rows(planes):
    n, C, H, W = planes.shape
    return planes.permute(0, 2, 3, 1).reshape(n * H * W, C)


def with_freeu(ref_model, b1, b2, s1, s2):
    """Installs on `ref_model.up_blocks[0]` and `[1]` (an oracle.unet3d_ref.UNet3DConditionModelRef) per-instance `forward`s that
    restate the block's loop with FreeU's two lines in front of the concatenation (diffusers' `apply_freeu`, resolution_idx 0
    and 1; the model computes in fp32, so the filter is diffusers' own fp32 expression around the float64 restatement).
    -> ref_model."""
    def make(b, s):
        def forward(self, x, skips, emb, ehs, nf, upsample_size=None):
            for i, (res, tc) in enumerate(zip(self.resnets, self.temp_convs)):
                skip = skips.pop()
                x = torch.cat([x[:, :x.shape[1] // 2] * b, x[:, x.shape[1] // 2:]], dim=1)
                skip = fourier_filter_ref(skip, s).to(skip.dtype)
                x = torch.cat([x, skip], dim=1)
                x = tc(res(x, emb), nf)
                if self.cross_attn:
                    x = self.temp_attentions[i](self.attentions[i](x, ehs), nf)
            if self.upsamplers is not None:
                x = self.upsamplers[0](x, upsample_size)
            return x
        return forward
    for blk, (b, s) in zip(ref_model.up_blocks[:2], ((b1, s1), (b2, s2))):
        blk.forward = types.MethodType(make(b, s), blk)
    return ref_model
