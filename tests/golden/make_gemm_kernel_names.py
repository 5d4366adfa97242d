"""Writes tests/golden/gemm_kernel_names.json: the names `ops.gemm_kernel_name` gave while it was a Python restatement of the
C dispatch, recorded from a checkout of the last commit that had it (the parent of the commit that added this file):
    python tests/golden/make_gemm_kernel_names.py /path/to/parent/checkout
Pure Python there (no GPU, no library).  Rows [M, N, K, mode, geglu, variant, single_source, residual, whole, wset, name];
tests/test_host.py asks the library for every one of them.  Axis values:
  M   B*F*S for B in {1, 2}, F in {2, 12, 16, 24}, S in {9216, 2304, 576, 144}, and 154, 1024, 16320, 16384
  N   64 320 512 640 960 1280 1536 1920 2560 4096 5120 10240
  K   plain: 320 512 640 1280 2560 5120 (with and without GEGLU); conv3x3: 9 C, temporal conv: 3 C, C in {320, 640, 1280}
The full product of these with ten variants is ~50 000 rows (4 MB); even the automatic choice alone is 0.5 MB of fixture
nobody can read.  The table is therefore cut along what the decision depends on (csrc/gemm.hip at that commit), so that every
value of every axis occurs and every input of every predicate takes each of its outcomes:
  tile choice (choose_tile) is a function of (rows, N) alone: EVERY (M, N) pair, automatic, plain K = 1280;
  weights-stationary choice depends on M >= 16384, M % 64 / % 32, K in {320, 512, 640}, N % 320 / % 256, GEGLU: every N x
      K <= 640 x GEGLU at M in {1024, 16320, 16384, 442368}, automatic; pinned 7 at M in {288, 1024, 16384} on seven N;
  MODE / GEGLU / SPLIT of the name depend on mode and flags, not on the size: every other (K, mode, GEGLU) at every N with
      M = 110592, at N in {640, 1280} with M = 6912, and the first K of conv3x3 / temporal conv / plain GEGLU at every M, N = 640;
  pinned variants 1 2 3 4 5 6 8 9: each mode (plain, plain GEGLU, conv3x3, temporal conv) at (16384, 1280) and (154, 64);
  residual / a row range / a second source (automatic) and weight sets (pinned 7, as ops.gemm passed them): M in {1024, 16384,
      442368}, N in {320, 512, 1280}, K in {320, 640}, plain, where the library accepts the combination (no residual with
      GEGLU, weight sets on whole weights-stationary products of a multiple of 64 rows only: include/vdx.h `wset_rows`).
Flags are written 0 / 1."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

MS = sorted({b * f * s for b in (1, 2) for f in (2, 12, 16, 24) for s in (9216, 2304, 576, 144)} | {154, 1024, 16320, 16384})
NS = (64, 320, 512, 640, 960, 1280, 1536, 1920, 2560, 4096, 5120, 10240)
PLAIN_K = (320, 512, 640, 1280, 2560, 5120)
WIDTHS = (320, 640, 1280)
FORCED = (1, 2, 3, 4, 5, 6, 8, 9)


def main(parent):
    sys.path.insert(0, parent)
    from vdx import ops
    assert "WS_MIN_ROWS" in vars(ops), "not a checkout with the Python restatement of the dispatch"
    kinds = [(k, 0, g) for k in PLAIN_K for g in (False, True)] + [(9 * c, 1, False) for c in WIDTHS] + [(3 * c, 2, False) for c in WIDTHS]
    rows = []

    def add(M, N, K, mode, geglu, variant=0, single_source=True, residual=False, whole=True, wset=False, only_ws=False):
        try:
            name = ops.gemm_kernel_name(M, N, K, mode, geglu, variant, single_source, residual, whole, wset)
        except KeyError:          # variant 7 on a shape without a weights-stationary kernel: the old function had no name
            return
        if only_ws and "gemm_ws_kernel" not in name:
            return
        rows.append([M, N, K, mode, int(geglu), variant, int(single_source), int(residual), int(whole), int(wset), name])

    first = {(0, False): 320, (0, True): 320, (1, False): 2880, (2, False): 960}     # first K of each (mode, GEGLU)
    for M in MS:
        for N in NS:
            add(M, N, 1280, 0, False)
            for K, mode, geglu in kinds:
                short = mode == 0 and K <= 640
                if short and M in (1024, 16320, 16384, 442368):
                    add(M, N, K, mode, geglu)
                if short and M in (288, 1024, 16384) and N in (64, 320, 512, 640, 960, 1280, 4096):
                    add(M, N, K, mode, geglu, 7, only_ws=True)
                if not short and (K, mode, geglu) != (1280, 0, False):
                    if M == 110592 or (M == 6912 and N in (640, 1280)) or (N == 640 and K == first.get((mode, geglu), 1280)):
                        add(M, N, K, mode, geglu)
                if (M, N) in ((16384, 1280), (154, 64)) and K == first.get((mode, geglu)):
                    for v in FORCED:
                        add(M, N, K, mode, geglu, v)
            for K in (320, 640) if N in (320, 512, 1280) and M in (1024, 16384, 442368) else ():
                add(M, N, K, 0, False, residual=True)
                add(M, N, K, 0, False, whole=False)
                add(M, N, K, 0, False, single_source=False)
                add(M, N, K, 0, True, single_source=False)
                add(M, N, K, 0, False, 7, wset=True, only_ws=True)
    out = os.path.join(HERE, "gemm_kernel_names.json")
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
    print(len(rows), "rows,", len({r[-1] for r in rows}), "names,", os.path.getsize(out), "bytes ->", out)


if __name__ == "__main__":
    main(sys.argv[1])
