"""-m "not gpu": the host side of the GroupNorm / LayerNorm tests (tests/norm_ref.py, tests/test_norm_gpu.py): the restated
launch geometry against the built library's own workspace size, the float32 emulator of the statistics pass against
float64 inside the figures recorded in tests/test_norm_gpu.py, and WHICH EDGE EACH GPU SHAPE REACHES — a later change of the
slab policy that moves a case off its edge fails here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_ref as R  # noqa: E402
import test_norm_gpu as T  # noqa: E402

import vdx  # noqa: E402,F401
from vdx import _lib  # noqa: E402

# (ns, rps, C, G, partition_samples) -> slab rows: every halving, partition_samples below, equal to and above n_samples
HALVINGS = [((2, 16384, 320, 32, 0), 128), ((1, 16384, 320, 32, 0), 64), ((2, 4096, 320, 32, 0), 32),
            ((2, 2304, 640, 32, 0), 16), ((2, 576, 1280, 32, 0), 8), ((48, 9216, 320, 32, 0), 128),
            ((8, 300, 320, 32, 4), 8), ((8, 300, 320, 32, 8), 8), ((8, 300, 320, 32, 48), 32), ((1, 300, 320, 32, 100), 128), ((1, 300, 320, 32, 60), 64),
            ((4, 16389, 320, 32, 2), 128), ((2, 16389, 320, 32, 1), 64), ((3, 1, 8, 1, 0), 8), ((1, 100000, 64, 2, 0), 128)]


def test_geometry_against_the_library():
    lib = _lib.load()
    table = [g for g, _ in HALVINGS] + [(ns, rps, c1 + c2, G, part) for ns, rps, c1, c2, G, part in R.GN_SHAPES]
    table += [(ns, rps, C, 32, 0) for C, _, ns, rps in R.FOLD_SHAPES] + [(9, 16389, 320, 32, 2), (9, 1000, 2048, 32, 3)]
    table += [(1, 20, 64, 1, 0), (1, 32, 64, 1, 0)]        # n_samples = G = 1: 3 and 4 slabs, the same table offset
    for ns, rps, C, G, part in table:
        want = (R.round_up4(ns * R.nslabs(ns, rps, part) * G * 3) + ns * C * 2) * 4
        assert lib.vdx_groupnorm_workspace_part(ns, rps, C, G, part) == want == R.workspace_bytes(ns, rps, C, G, part), (ns, rps, C, G, part)
    for (ns, rps, C, G, part), rows in HALVINGS:
        assert R.stat_rows(ns, rps, part) == rows, (ns, rps, part)
    assert {rows for _, rows in HALVINGS} == {128, 64, 32, 16, 8}
    assert lib.vdx_groupnorm_workspace(3, 300, 320, 32) == R.workspace_bytes(3, 300, 320, 32)


def test_row_walk_is_a_partition():
    """Every row of a sample is read by exactly one (slab, row subset), in ascending order per thread."""
    for ns, rps, c1, c2, G, part in R.GN_SHAPES:
        if rps > 3000:
            continue
        sr, (kr, nt) = R.stat_rows(ns, rps, part), R.krows_threads(c1 + c2)
        seen = []
        for s in range((rps + sr - 1) // sr):
            for rsub in range(kr):
                first, trips, tail = R.rows_of_thread(s, rsub, sr, kr, rps)
                walk = first + [r for t in trips for r in t] + tail
                assert walk == sorted(walk) and (not trips or first)
                seen += walk
        assert sorted(seen) == list(range(rps))


# the edges of the issue's list -> which shapes must reach them
EDGES = {
    "unrolled_then_tail": [(3, 1000, 2048, 0, 32, 0), (2, 16389, 320, 0, 32, 0), (2, 257, 2560, 0, 32, 0)],
    "idle_threads": [(1, 1, 64, 0, 32, 0), (1, 5, 320, 0, 32, 0), (6, 35, 64, 0, 32, 0), (2, 130, 64, 128, 32, 0)],
    "last_slab_one_row": [(2, 513, 1280, 640, 32, 0), (1, 2049, 128, 0, 32, 0), (1, 8065, 64, 0, 32, 0), (1, 24705, 64, 0, 32, 0),
                          (1, 32897, 64, 0, 32, 0), (2, 129, 512, 0, 32, 8)],
    "cpg_over_64": [(2, 257, 2560, 0, 32, 0), (2, 40, 320, 0, 1, 0)],
    "block_not_wave_multiple": [(1, 5, 320, 0, 32, 0), (3, 300, 320, 0, 32, 0), (2, 130, 64, 128, 32, 0), (2, 16389, 320, 0, 32, 0)],
}
# shape -> (slab rows, krows, threads, slabs, rows of the last slab, most rows per thread)
GEOMETRY = {
    (1, 1, 64, 0, 32, 0): (8, 32, 256, 1, 1, 1), (1, 5, 320, 0, 32, 0): (8, 7, 280, 1, 5, 1),
    (6, 35, 64, 0, 32, 0): (8, 32, 256, 5, 3, 1), (3, 300, 320, 0, 32, 0): (8, 7, 280, 38, 4, 2),
    (1, 300, 320, 0, 32, 48): (32, 7, 280, 10, 12, 5), (2, 130, 64, 128, 32, 0): (8, 11, 264, 17, 2, 1),
    (2, 513, 1280, 640, 32, 0): (8, 2, 480, 65, 1, 4), (2, 257, 2560, 0, 32, 0): (8, 1, 320, 33, 1, 8),
    (2, 40, 320, 0, 1, 0): (8, 7, 280, 5, 8, 2), (3, 1000, 2048, 0, 32, 0): (8, 1, 256, 125, 8, 8),
    (2, 16389, 320, 0, 32, 0): (128, 7, 280, 129, 5, 19), (1, 2049, 128, 0, 32, 0): (8, 16, 256, 257, 1, 1),
    (1, 8065, 64, 0, 32, 0): (16, 32, 256, 505, 1, 1), (1, 24705, 64, 0, 32, 0): (64, 32, 256, 387, 1, 2),
    (1, 32897, 64, 0, 32, 0): (128, 32, 256, 258, 1, 4), (1, 497, 64, 0, 32, 0): (8, 32, 256, 63, 1, 1),
    (1, 505, 64, 0, 32, 0): (8, 32, 256, 64, 1, 1), (1, 1529, 64, 0, 32, 0): (8, 32, 256, 192, 1, 1),
    (1, 1537, 64, 0, 32, 0): (8, 32, 256, 193, 1, 1), (2, 129, 512, 0, 32, 8): (8, 4, 256, 17, 1, 2),
}


def test_shape_table_reaches_what_it_claims(capsys):
    feats = {s: R.features(s[0], s[1], s[2] + s[3], s[4], s[5]) for s in R.GN_SHAPES}
    assert set(GEOMETRY) == set(R.GN_SHAPES) == set(R.GN_REGIMES)
    with capsys.disabled():
        print()
        for s, f in feats.items():
            print(f"    {s}: slab {f['slab_rows']} x {f['nslabs']}, krows {f['krows']}, {f['threads']} threads, cpg {f['cpg']}, "
                  f"<= {f['rows_per_thread']} rows per thread, last slab {f['last_slab_rows']}: "
                  + ", ".join(k for k in EDGES if f[k]))
    for s, f in feats.items():
        got = (f["slab_rows"], f["krows"], f["threads"], f["nslabs"], f["last_slab_rows"], f["rows_per_thread"])
        assert got == GEOMETRY[s], (s, got)
    for edge, shapes in EDGES.items():
        for s in shapes:
            assert feats[s][edge], f"{s} no longer reaches {edge}"
    # the finalize: lanes without a slab, one slab per lane, the tail alone at its longest, one unrolled trip on one lane,
    # an unrolled trip and a tail
    assert {1, 63, 64, 65, 192, 193, 257} <= {f["nslabs"] for f in feats.values()}
    assert any(f["nslabs"] > 128 and f["last_slab_rows"] < f["slab_rows"] for f in feats.values())
    # the four-rows-per-trip loop on the level-0 path: slab 128, 18-19 rows per thread
    f = feats[(2, 16389, 320, 0, 32, 0)]
    assert f["slab_rows"] == 128 and f["rows_per_thread"] == 19 and f["apply_rows"] == 32
    # every shape gets regime (a); the pair at rps 300 differs in its slab size only
    assert all("a" in r for r in R.GN_REGIMES.values())
    assert feats[(3, 300, 320, 0, 32, 0)]["slab_rows"] == 8 and feats[(1, 300, 320, 0, 32, 48)]["slab_rows"] == 32
    # the strided two-source case: groups straddle the 8-channel vectors and the seam between the sources
    assert feats[(2, 130, 64, 128, 32, 0)]["cpg"] == 6 and 64 % 6 != 0
    # the marker rows of test_marker_rows, pinned: slab edges, the first unrolled row, the trip / tail seam, the last row
    assert R.marker_rows(1000, 2048, 3) == [0, 1, 4, 5, 7, 8, 15, 992, 999]
    assert R.marker_rows(16389, 320, 2) == [0, 7, 112, 119, 127, 128, 255, 16384, 16388]
    # regime (f) plants its outliers on the first row of every slab of the case's own geometry, and nowhere else
    for s in R.GN_SHAPES:
        if "f" in R.GN_REGIMES[s]:
            x = R.gn_inputs(s, "f")[0].astype(np.float32)
            hot = np.flatnonzero((x > 30).any(axis=(0, 2)))
            assert np.array_equal(hot, np.arange(0, s[1], feats[s]["slab_rows"])), s


@pytest.mark.parametrize("shape,regime", R.GN_CASES, ids=[R.case_id(s, r) for s, r in R.GN_CASES])
def test_emulator_inside_the_recorded_figures(shape, regime):
    ns, rps, c1, c2, G, part = shape
    x, gamma, beta = R.gn_inputs(shape, regime)
    assert x.dtype == np.float16 and np.isfinite(x.astype(np.float32)).all()
    sr, (kr, _) = R.stat_rows(ns, rps, part), R.krows_threads(c1 + c2)
    emu = R.emulate_stats(x, gamma, beta, G, R.GN_EPS, sr, kr)
    err = R.stat_errors(emu, x, gamma, beta, G, R.GN_EPS, sr)
    for fig, rec in zip(R.FIGURES, T.RECORDED[R.case_id(shape, regime)]):
        assert err[fig] <= rec, f"{fig}: {err[fig]:.4g} > recorded {rec:.3g}"
        # ... and the table is the emulator's own figure, not a looser one: an emulator (or a table) that drifts fails here
        assert rec <= max(R.RECORD_SLACK * err[fig], R.round_up2(R.FIGURE_FLOORS[fig])), f"{fig}: recorded {rec:.3g} for {err[fig]:.4g}"
        if fig in ("pm2", "scale"):                 # far inside a one-row error: 1 / 128 of a full slab's M2
            assert T.GPU_FACTOR * rec < 2e-3
    assert R.pmean_ratio(err, T.RECORDED[R.case_id(shape, regime)][0], 1.0) <= 1.0
    if regime in "de":                              # constant over rows: a thread's own M2 is exactly 0
        assert emu["thread_m2_max"] == 0.0
    if regime == "e":
        assert not emu["m2"].any()
    if regime == "g":
        g32 = gamma.astype(np.float32)
        assert (g32 == 0).sum() >= 2 and ((g32 != 0) & (np.abs(g32) < 2.0 ** -14)).sum() >= 2 and g32.max() == 30 and g32.min() == -30


def test_recorded_table_is_the_case_table():
    assert set(T.RECORDED) == {R.case_id(s, r) for s, r in R.GN_CASES}
    assert T.GPU_FACTOR == 8.0


def test_emulator_notices_what_the_mutants_do():
    """The figures separate an honest fp32 pass from a wrong one: a merge without its between-subset term and a slab that
    drops its last row both land far outside 8 x the recorded figure."""
    shape = (3, 300, 320, 0, 32, 0)
    x, gamma, beta = R.gn_inputs(shape, "c")
    sr, (kr, _) = R.stat_rows(3, 300), R.krows_threads(320)
    rec = dict(zip(R.FIGURES, T.RECORDED[R.case_id(shape, "c")]))
    short = x.copy()
    short[:, sr - 1::sr] = short[:, sr - 2::sr][:, :short[:, sr - 1::sr].shape[1]]      # every slab reads a row twice
    emu = R.emulate_stats(short, gamma, beta, 32, R.GN_EPS, sr, kr)
    emu["n"] = R.ref_partial(x, 32, sr)[0].astype(np.float32)
    err = R.stat_errors(emu, x, gamma, beta, 32, R.GN_EPS, sr)
    assert err["pmean"] > 100 * T.GPU_FACTOR * rec["pmean"] and err["pm2"] > 100 * T.GPU_FACTOR * rec["pm2"]


def test_layernorm_dispatch_restated():
    for C, want in R.LN_WIDTHS.items():
        assert R.ln_dispatch(C) == want, C
    assert {R.ln_dispatch(C) for C in R.LN_WIDTHS if R.ln_dispatch(C)[0] == "wave"} == {("wave", 1), ("wave", 2), ("wave", 3), ("wave", 4)}
    assert {d[1] for d in R.LN_WIDTHS.values() if d[0] == "rows"} == {8, 16, 32, 64}
    assert R.ln_rows(320) == [1, 7, 8, 9, 33] and R.ln_rows(2048) == [1, 2, 5] and R.ln_rows(96) == [1, 3, 4, 5, 17]
    for M, C in R.LN_BIG:                           # groups per wave on the 2048-block grid
        rw = 64 // R.ln_dispatch(C)[1]
        groups = -(-M // rw)
        assert groups > 8192 and (C != 64 or groups > 16384)


def test_float64_reference_is_group_norm():
    """The reference against torch's float64 GroupNorm / LayerNorm on one small case."""
    import torch
    import torch.nn.functional as F
    shape = (2, 130, 64, 128, 32, 0)
    x, gamma, beta = R.gn_inputs(shape, "a")
    scale, shift, _, _ = R.ref_table(x, gamma, beta, 32, R.GN_EPS)
    mine = x.astype(np.float64) * scale[:, None, :] + shift[:, None, :]
    t = lambda a: torch.from_numpy(a.astype(np.float64))  # noqa: E731
    ref = F.group_norm(t(x).permute(0, 2, 1), 32, t(gamma), t(beta), float(R.eps64(R.GN_EPS))).permute(0, 2, 1).numpy()
    assert np.abs(mine - ref).max() < 1e-12
    xl, gl, bl = R.ln_inputs(9, 320, "a")
    ln = F.layer_norm(t(xl), (320,), t(gl), t(bl), float(R.eps64(R.LN_EPS))).numpy()
    assert np.abs(R.ref_layernorm(xl, gl, bl, R.LN_EPS)[0] - ln).max() < 1e-12
