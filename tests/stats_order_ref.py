"""The ORDER in which the statistics passes (csrc/rescale.hip, csrc/dynthresh.hip) add their fp64 terms, restated on the host with
numpy float64, so a block's partial row can be compared bit for bit:

  a lane starts at 0.0 and adds its elements in the order its noise source hands them over;
  a wave's 64 lanes are added by a shuffle tree: for off = 32, 16, .., 1 lane l takes a[l] + a[l + off] (lane 0 holds the sum);
  the block's four waves are added in ascending order: ((w0 + w1) + w2) + w3.

The one-buffer source (`direct_order`): block x of nx grid-strides over the channel's vectors of E elements, v = x * 256 + lane +
j * nx * 256.  The co-fused source (`line_order`): block x of nx takes the channel's lines x, x + nx, ..., and in a line of HW
elements a lane the vectors at p = (lane + 256 j) * E."""
import numpy as np


def width(M):
    return 8 if M % 8 == 0 else 4 if M % 4 == 0 else 1


def direct_order(M, E, x, nx):
    """-> the trips of block x: int arrays (256, E) of element indices inside the channel, -1 where a lane has none."""
    lane, nv, trips, j = np.arange(256), M // E, [], 0
    while x * 256 + j * nx * 256 < nv:
        v = x * 256 + lane + j * nx * 256
        trips.append(np.where((v < nv)[:, None], v[:, None] * E + np.arange(E)[None, :], -1))
        j += 1
    return trips


def line_order(lines, HW, E, x, nx):
    lane, trips = np.arange(256), []
    for line in range(x, lines, nx):
        j = 0
        while 256 * j * E < HW:
            p = (lane + 256 * j) * E
            trips.append(np.where((p < HW)[:, None], line * HW + p[:, None] + np.arange(E)[None, :], -1))
            j += 1
    return trips


def block_row(terms, trips):
    """terms float64 (n, Q), a block's trips -> its row float64 (Q,)."""
    terms = np.asarray(terms, dtype=np.float64)
    acc = np.zeros((256, terms.shape[1]), dtype=np.float64)
    with np.errstate(all="ignore"):
        for idx in trips:
            for e in range(idx.shape[1]):
                col = idx[:, e]
                has = col >= 0
                acc[has] = acc[has] + terms[col[has]]
        w = acc.reshape(4, 64, -1)
        for off in (32, 16, 8, 4, 2, 1):
            nxt = w + w                                             # a lane without a partner gets its own value back
            nxt[:, :64 - off] = w[:, :64 - off] + w[:, off:]
            w = nxt
        t = w[:, 0]
        return ((t[0] + t[1]) + t[2]) + t[3]


def rows(terms, order, nx):
    """`order(x, nx)` -> block x's trips; -> float64 (nx, Q)."""
    return np.stack([block_row(terms, order(x, nx)) for x in range(nx)])


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and bool((got.view(np.uint64) == want.view(np.uint64)).all())
