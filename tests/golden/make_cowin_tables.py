"""Records tests/golden/cowin_tables.json: what the three fuse-table builders of vdx/codenoise.py (`window_table`, `loop_table`,
`stride_table`) give over a sweep of plans, and what the whole-clip fused steps of vdx/ops.py hand to `ops._launch`.

  * "tables": for T in {5, 8, 13, 24} x world in {1, 2, 3} x chunk in {0 (auto), 4, 6, 16} x overlap in {1, 2, 4} and the kinds
    flat (`plan`), ring (`loop_plan`) and strided with 2 and 3 levels (`stride_plan`), every case the planner and the builder
    accept: the plan's arguments, `fused`, `rows(world, per_rank, 1000)` and the SHA-256 of `wn.numpy().tobytes()`.
  * "launches": one flat, one ring, one strided and one tiled step, the DDIM and the DPM-Solver++ form of each, on host tensors
    with `ops._p` answering an argument's NAME instead of its pointer and `ops._launch` recording: [symbol, arguments], host
    arrays as lists.  Nothing launches and no device is needed.

The fixture pins bits and argument order, so it is recorded from the commit BEFORE a change to that code, never from the code
under test:

    git worktree add DIR <parent commit>  &&  cp tests/golden/make_cowin_tables.py DIR/tests/golden/
    python DIR/tests/golden/make_cowin_tables.py tests/golden/cowin_tables.json

tests/test_cowin_tables_host.py imports `table_case` and `launches` from here and replays what was recorded.
"""
import ctypes
import hashlib
import itertools
import json
import os
import sys
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

KINDS = {"flat": 1, "ring": 1, "stride2": 2, "stride3": 3}       # kind -> stride levels
SWEEP = list(itertools.product((5, 8, 13, 24), (1, 2, 3), (0, 4, 6, 16), (1, 2, 4), KINDS))


def table_case(T, world, chunk, overlap, kind):
    """One case of the sweep -> {"args", "fused", "rows", "sha256"}; the planner's or the builder's `ValueError` passes through."""
    from vdx import codenoise as cn
    from vdx.planner import plan
    if kind == "flat":
        p = plan(T, world, chunk, overlap)
        tab = cn.window_table(p, T)
    elif kind == "ring":
        p = cn.loop_plan(T, world, chunk, overlap)
        tab = cn.loop_table(p, T)
    else:
        p = cn.stride_plan(T, world, chunk, overlap, levels=KINDS[kind])
        tab = cn.stride_table(p, T)
    return {"args": [T, world, chunk, overlap, kind], "fused": [list(r) for r in tab.fused],
            "rows": [list(r) for r in tab.rows(world, p.per_rank, 1000)],
            "sha256": hashlib.sha256(tab.wn.numpy().tobytes()).hexdigest()}


def launches():
    """-> {wrapper name: [symbol, arguments]} of the eight plain whole-clip steps on a (1,4,8,8,8) host latent."""
    import torch
    from vdx import codenoise as cn
    from vdx import ops
    from vdx.planner import ChunkPlan
    T, C, h, w = 8, 4, 8, 8
    z = torch.zeros(1, C, T, h, w, dtype=torch.float16)
    prev, x0 = torch.zeros_like(z), torch.zeros_like(z)
    flat = ChunkPlan(6, 2, ((0, 6), (4, 8)), 1)
    ring = cn.loop_plan(T, 1, 4, 1)
    strided = cn.stride_plan(T, 1, 4, 1, levels=2)
    tiles = cn.tile_plan(h, w, 6, 6, 2, 2)
    ddim, dpm = (0.5, 0.25, 0.125, 2.0), (0.5, 0.25, 0.125, 2.0, 4.0, 8.0)
    seen = []

    def plainly(v):
        return list(v) if isinstance(v, ctypes.Array) else v

    def record(symbol, *args):
        seen.append([symbol, [plainly(v) for v in args]])

    def cases():
        for stem, plan_, tab, slot in (("cofuse", flat, cn.window_table(flat, T), 2 * C * flat.chunk * h * w),
                                       ("coloop", ring, cn.loop_table(ring, T), 2 * C * ring.chunk * h * w),
                                       ("costride", strided, cn.stride_table(strided, T), 2 * C * strided.chunk * h * w)):
            rows = tab.rows(1, plan_.per_rank, slot)
            yield stem, (z, torch.zeros(plan_.per_rank * slot, dtype=torch.float16), rows, tab.wn)
        tab, slot = cn.window_table(flat, T), 2 * C * flat.chunk * tiles.th * tiles.tw
        rows = tab.rows(1, flat.per_rank, tiles.count * slot)
        yield "cotile", (z, torch.zeros(flat.per_rank * tiles.count * slot, dtype=torch.float16), rows, tab.wn, tiles.grid(slot, "cpu"))

    with mock.patch.object(ops, "_p", lambda t, name, dtype=None: None if t is None else name), mock.patch.object(ops, "_launch", record):
        got = {}
        for stem, head in cases():
            for name, call in ((f"{stem}_cfg_ddim_step", lambda f: f(*head, 7.5, ddim)),
                               (f"{stem}_cfg_dpm_step", lambda f: f(*head, 7.5, dpm, x0_prev=prev, x0_out=x0))):
                call(getattr(ops, name))
                got[name] = seen.pop()
                assert not seen
    return got


def main(path):
    import vdx  # noqa: F401
    tables = []
    for case in SWEEP:
        try:
            tables.append(table_case(*case))
        except ValueError:      # PlannerError is one: a case the planner or the builder refuses is not recorded
            pass
    with open(path, "w") as f:
        f.write('{"tables": [\n' + ",\n".join(json.dumps(t) for t in tables) + '\n],\n"launches": {\n'
                + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in launches().items()) + "\n}}\n")
    kinds = [t["args"][4] for t in tables]
    print(f"{path}: {len(tables)} tables ({ {k: kinds.count(k) for k in KINDS} }), {len(launches())} launches")


if __name__ == "__main__":
    main(sys.argv[1])
