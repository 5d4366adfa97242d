"""Reference of the upsampler convolution in phase form, written from the statement of packing.pack_upconv_phase's table
(not from the kernel): output (2i+a, 2j+b) = sum over ty, tx in {0, 1} of T[2a+b][ty][tx] . x[i+a-1+ty][j+b-1+tx], zero
outside the image."""
import torch
import torch.nn.functional as F


def unpack_phase_table(table: torch.Tensor, N: int) -> torch.Tensor:
    """[4*N][4*C] in the kernels' K order (64-channel slice, tap, channel) -> [phase][N][C][ty][tx]."""
    C = table.shape[1] // 4
    assert table.shape == (4 * N, 4 * C) and C % 64 == 0
    t = table.reshape(4, N, C // 64, 2, 2, 64)                 # phase, n, slice, ty, tx, channel
    return t.permute(0, 1, 2, 5, 3, 4).reshape(4, N, C, 2, 2)


def phase_reference(x: torch.Tensor, table: torch.Tensor, N: int) -> torch.Tensor:
    """x [n][C][h][w], table [4*N][4*C] (same dtype) -> [n][N][2h][2w]: the four 2x2 convolutions, interleaved."""
    n, _, h, w = x.shape
    wp = unpack_phase_table(table, N)
    xp = F.pad(x, (1, 1, 1, 1))
    out = x.new_zeros((n, N, 2 * h, 2 * w))
    for a in range(2):
        for b in range(2):
            out[:, :, a::2, b::2] = F.conv2d(xp[:, :, a:a + h + 1, b:b + w + 1], wp[2 * a + b])
    return out
