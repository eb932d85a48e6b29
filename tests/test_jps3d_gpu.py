"""HIP 3D Jump Point Search (jps3d.hip via the C-ABI) vs the reference JPS3D runs of
tests/golden/jps3d_runs.npz.

Bar: bit-exact status, cost, path, CLOSED order, every CLOSED node's final parent and g, and the
number of expansions."""
import math
from decimal import Decimal, localcontext

import numpy as np
import pytest

import jps3d_checks as J

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return J.cases()


def run_group(group, **kw):
    """One jps3d_batch call over fixture cases of one grid size and heuristic, as per-query grids."""
    from python_motion_planning_amd import batch

    occ = np.stack([c["occ"] for c in group])
    S = np.stack([c["start"] for c in group]).astype(np.int32)
    G = np.stack([c["goal"] for c in group]).astype(np.int32)
    r = batch.jps3d_batch(occ, S, G, group[0]["heuristic"], expand_cap=int(np.prod(occ.shape[1:])), counters=True, **kw)
    return {k: v.cpu().numpy() for k, v in r.items() if k != "dims" and v is not None}


def compare(group, r):
    """Every output of the batch against the reference's records; returns the number of cases compared."""
    for q, c in enumerate(group):
        tag = (c["i"], c["occ"].shape)
        assert r["status"][q] == (0 if len(c["path"]) else 1), tag
        assert r["cost"][q] == c["cost"], tag  # inf == inf when unreachable
        assert np.array_equal(r["path"][q, : r["path_len"][q]], c["path"]), tag
        ne = int(r["n_expanded"][q])
        assert ne == len(c["closed"]), tag
        assert np.array_equal(r["expand"][q, :ne], c["closed"]), tag
        assert np.array_equal(r["expand_parent"][q, :ne], c["closed_parent"]), tag
        assert np.array_equal(r["expand_g"][q, :ne].view(np.int64), c["closed_g"].view(np.int64)), tag
        assert r["counters"][q, 2] == c["expansions"], tag
    return len(group)


def groups_of(cases):
    groups = {}
    for c in cases:
        groups.setdefault((c["occ"].shape, c["heuristic"]), []).append(c)
    return groups


def test_jps3d_against_reference(cases):
    n = 0
    for group in groups_of(cases).values():
        n += compare(group, run_group(group))
    assert n == len(cases) == 220


def test_jps3d_dropin_class(cases):
    """JPS3D(...).plan() on six fixture cases (a failed search and a re-expansion among them) and on
    numpy-integer endpoints: cost, path tuples and (current, parent, g, h) of every expand node."""
    import python_motion_planning_amd as pmp

    small = [c for c in cases if c["occ"].size <= 21 * 15 * 11]
    picks = [next(c for c in small if len(c["path"]) == 0 and len(c["closed"]) > 1),
             next(c for c in small if c["expansions"] > len(c["closed"])),
             next(c for c in small if c["heuristic"] == "manhattan" and len(c["path"]) > 2),
             next(c for c in small if c["expansions"] == len(c["closed"]) and len(c["path"]) > 3), cases[-6], cases[-3]]
    assert len({c["i"] for c in picks}) == 6
    for k, c in enumerate(picks + [picks[3]]):
        X, Y, Z = c["occ"].shape
        env = pmp.Grid3D(X, Y, Z)
        env.update({(int(a), int(b), int(d)) for a, b, d in np.argwhere(c["occ"])})
        ints = k < len(picks)  # the last run passes numpy integers
        s = tuple(int(v) for v in c["start"]) if ints else tuple(c["start"])
        g = tuple(int(v) for v in c["goal"]) if ints else tuple(c["goal"])
        assert ints or isinstance(s[0], np.integer)
        cost, path, expand = pmp.JPS3D(s, g, env, c["heuristic"]).plan()
        assert cost == c["cost"], c["i"]
        assert path == [J.decode(v, c["occ"].shape) for v in c["path"]], c["i"]
        assert len(expand) == len(c["closed"]), c["i"]
        for node, cell, par, gv in zip(expand, c["closed"], c["closed_parent"], c["closed_g"]):
            cur = J.decode(cell, c["occ"].shape)
            d = [abs(int(c["goal"][a]) - cur[a]) for a in range(3)]
            h = sum(d) if c["heuristic"] == "manhattan" else math.sqrt(sum(v * v for v in d))
            assert (node.current, node.parent, node.g, node.h) == (cur, J.decode(par, c["occ"].shape), float(gv), h), c["i"]


def exact_length(cells, dims):
    """A path's length as a Decimal of a + b sqrt(2) + c sqrt(3) from its unit-step counts: free of the
    rounding that the planners' float sums carry."""
    pts = [J.decode(v, dims) for v in cells]
    n = [0, 0, 0, 0]
    for p, q in zip(pts[:-1], pts[1:]):
        delta = [abs(q[k] - p[k]) for k in range(3)]
        n[sum(v != 0 for v in delta)] += max(delta)
    with localcontext() as ctx:
        ctx.prec = 50
        return n[1] + n[2] * Decimal(2).sqrt() + n[3] * Decimal(3).sqrt()


def test_jps3d_shared_grid_invariants():
    """512 C5 queries on the shared door grid.  (a) the per-query form, the input-order schedule and 4
    workers per CU give identical results; (b) every found path is valid and its cost is the sum along
    it; (c) what JPS3D finds AStar3D finds, at no greater length.

    (c) compares exact lengths (unit-step counts times 1, sqrt 2, sqrt 3), not the float costs: a jump of
    k diagonal steps costs sqrt(2 k^2) in one rounding where A* adds sqrt(2) k times, and on these
    queries 33 of the 354 found JPS costs lie 1-4 ulp below A*'s float cost for paths of equal length."""
    from python_motion_planning_amd import AStar3D, _lib, batch, workloads as wl

    _, S, G = wl.c5_workload(512)
    occ = wl.SCENARIOS_3D["door"](26, 20, 16)
    keys = ("status", "cost", "path_len", "path", "n_expanded", "expand", "expand_parent", "expand_g", "counters")

    def run(o):
        r = batch.jps3d_batch(o, S, G, expand_cap=512, counters=True)
        r = {k: r[k].cpu().numpy() for k in keys}
        for q in range(len(S)):  # compare only what the kernel wrote
            r["path"][q, r["path_len"][q]:] = 0
            for k in ("expand", "expand_parent", "expand_g"):
                r[k][q, min(r["n_expanded"][q], 512):] = 0
        return r

    base = run(occ)
    assert base["n_expanded"].max() <= 512
    L, ctx = _lib.load_library(), _lib.context()
    variants = {"per-query": run(np.broadcast_to(occ, (len(S),) + occ.shape))}
    _lib.check(ctx, L.pmp_astar2d_set_schedule(ctx, 0), "schedule")
    try:
        variants["input order"] = run(occ)
    finally:
        _lib.check(ctx, L.pmp_astar2d_set_schedule(ctx, 1), "schedule")
    _lib.check(ctx, L.pmp_set_workers_per_cu(ctx, 4), "workers")
    try:
        variants["4 workers per CU"] = run(occ)
    finally:
        _lib.check(ctx, L.pmp_set_workers_per_cu(ctx, 0), "workers")
    for name, v in variants.items():
        for k in keys:
            assert np.array_equal(base[k], v[k]), (name, k)
    a = AStar3D.plan_batch(occ, S, G)
    a_st, a_pl, a_path = a["status"].cpu().numpy(), a["path_len"].cpu().numpy(), a["path"].cpu().numpy()
    found = 0
    for q in range(len(S)):
        assert base["status"][q] in (0, 1), q
        if base["status"][q] != 0:
            continue
        found += 1
        path = base["path"][q, : base["path_len"][q]]
        assert J.path_cost(occ, path) == base["cost"][q], q
        assert a_st[q] == 0, q
        assert exact_length(path, occ.shape) >= exact_length(a_path[q, : a_pl[q]], occ.shape), q
    assert found >= 300


def test_jps3d_small_heap_spill(cases):
    """The 40x30x30 runs with the smallest LDS heap share (32 workers per CU configured and resident:
    192 entries of 24 B), so most of each heap lives in its HBM spill."""
    from python_motion_planning_amd import _lib

    group = [c for c in cases if c["occ"].shape == (40, 30, 30)]
    assert len(group) == 4
    L, ctx = _lib.load_library(), _lib.context()
    _lib.check(ctx, L.pmp_set_workers_per_cu(ctx, 32), "workers")
    _lib.check(ctx, L.pmp_set_resident_per_cu(ctx, 32), "resident")
    try:
        r = run_group(group)
    finally:
        _lib.check(ctx, L.pmp_set_resident_per_cu(ctx, 0), "resident")
        _lib.check(ctx, L.pmp_set_workers_per_cu(ctx, 0), "workers")
    assert compare(group, r) == 4
    assert r["counters"][:, 3].min() > ((160 * 1024 // 32 - 256) // 24 & ~15)
