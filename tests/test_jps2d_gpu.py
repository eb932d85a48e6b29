"""HIP 2D Jump Point Search (jps2d.hip via the C-ABI) vs the reference JPS runs of
tests/golden/jps2d_runs.npz.

Bar: exact status, cost bits, path, len(CLOSED), pushes, pops, expansions and max heap size, and the
CLOSED cells, parents and g in insertion order (by SHA-1 on the 1024^2 grid).  Everything compared is
an integer or a correctly rounded f64, so there is no tolerance."""
import math

import numpy as np
import pytest

import jps2d_checks as J

pytestmark = pytest.mark.gpu

KEYS = ("status", "cost", "path_len", "path", "n_expanded", "expand", "expand_parent", "expand_g", "counters")


@pytest.fixture(scope="module")
def grids():
    return J.grids()


def run_grid(g, cases=None, **kw):
    """One jps2d_batch call per heuristic over the cases of one grid; returns per-case numpy outputs."""
    from python_motion_planning_amd import batch

    cases = g["cases"] if cases is None else cases
    out = [None] * len(cases)
    for heur in ("euclidean", "manhattan"):
        idx = [k for k, c in enumerate(cases) if c["heuristic"] == heur]
        if not idx:
            continue
        S = np.stack([cases[k]["start"] for k in idx]).astype(np.int32)
        G = np.stack([cases[k]["goal"] for k in idx]).astype(np.int32)
        ecap = max(cases[k]["n_closed"] for k in idx) + 1
        pcap = max(len(cases[k]["path"]) for k in idx) + 1
        kw2 = dict(path_cap=pcap, expand_cap=ecap, counters=True)
        kw2.update(kw)
        r = batch.jps2d_batch(g["occ"], S, G, heur, **kw2)
        r = {k: r[k].cpu().numpy() for k in KEYS}
        for j, k in enumerate(idx):
            out[k] = {key: r[key][j] for key in KEYS}
    return out


def compare(g, c, r):
    tag = (g["name"], c["i"])
    assert r["status"] == (0 if c["found"] else 1), tag
    assert r["cost"].view(np.int64) == c["cost"].view(np.int64), tag
    assert np.array_equal(r["path"][: r["path_len"]], c["path"]), tag
    ne = int(r["n_expanded"])
    assert ne == c["n_closed"], tag
    assert tuple(int(v) for v in r["counters"]) == (c["pushes"], c["pops"], c["n_closed"], c["max_heap"]), tag
    if c["closed"] is not None:
        assert np.array_equal(r["expand"][:ne], c["closed"]), tag
        assert np.array_equal(r["expand_parent"][:ne], c["closed_parent"]), tag
        assert np.array_equal(r["expand_g"][:ne].view(np.int64), c["closed_g"].view(np.int64)), tag
    assert J.closed_digest(r["expand"][:ne], r["expand_parent"][:ne], r["expand_g"][:ne]) == c["digest"], tag


def test_jps2d_against_reference(grids):
    """Every fixture case; the 1024^2 cases with a push capacity above their largest push count."""
    n = 0
    for g in grids:
        kw = {} if g["stored"] else dict(push_cap=max(c["pushes"] for c in g["cases"]) + 8)
        for c, r in zip(g["cases"], run_grid(g, **kw)):
            compare(g, c, r)
            n += 1
    assert n == 382


def test_jps2d_dropin_class(grids):
    """JPS((5, 5), (45, 25), README grid).plan(): the reference's cost, the 10 path tuples goal first, and
    10 Nodes with the fixture's current, parent, g and h; a no-path query returns ([], [], [])."""
    import python_motion_planning_amd as pmp

    g = next(g for g in grids if g["name"] == "readme")
    W, H = g["occ"].shape
    env = pmp.Grid(W, H)
    env.update({(int(x), int(y)) for x, y in np.argwhere(g["occ"])})
    dec = lambda c: (int(c) // H, int(c) % H)  # noqa: E731
    for c in g["cases"]:
        planner = pmp.JPS((5, 5), (45, 25), env, c["heuristic"])
        cost, path, expand = planner.run()
        assert cost == c["cost"] and (c["heuristic"] != "euclidean" or cost == 53.45584412271572)
        assert path == [dec(v) for v in c["path"]] and len(path) == 10 and path[0] == (45, 25) and path[-1] == (5, 5)
        assert len(expand) == c["n_closed"] == 10
        for k, (node, cell, par, gv) in enumerate(zip(expand, c["closed"], c["closed_parent"], c["closed_g"])):
            cur = dec(cell)
            dx, dy = 45 - cur[0], 25 - cur[1]
            h = 0 if k == 0 else (abs(dx) + abs(dy) if c["heuristic"] == "manhattan" else math.hypot(dx, dy))
            assert isinstance(node, pmp.Node)
            assert (node.current, node.parent, node.g, node.h) == (cur, dec(par), float(gv), h), (c["i"], k)
    sq = next(g for g in grids if g["name"] == "squeeze")
    c = sq["cases"][3]
    assert not c["found"]
    env = pmp.Grid(*sq["occ"].shape)
    env.update({(int(x), int(y)) for x, y in np.argwhere(sq["occ"])})
    assert pmp.JPS(tuple(c["start"]), tuple(c["goal"]), env).plan() == ([], [], [])


def test_jps2d_spill_and_capacity(grids):
    """(a) The shortest 1024^2 query with the smallest LDS heap share (32 workers per CU resident: 304
    entries of 16 B), so most of its heap lives in the HBM spill: identical outputs.  (b) A push capacity
    below one query's recorded push count: that query reports status 3, the others of the batch still
    equal the fixture."""
    from python_motion_planning_amd import _lib

    c2 = next(g for g in grids if not g["stored"])
    c = min(c2["cases"], key=lambda c: c["pushes"])
    L, ctx = _lib.load_library(), _lib.context()
    _lib.check(ctx, L.pmp_set_workers_per_cu(ctx, 32), "workers")
    _lib.check(ctx, L.pmp_set_resident_per_cu(ctx, 32), "resident")
    try:
        r = run_grid(c2, [c], push_cap=c["pushes"] + 8)[0]
    finally:
        _lib.check(ctx, L.pmp_set_resident_per_cu(ctx, 0), "resident")
        _lib.check(ctx, L.pmp_set_workers_per_cu(ctx, 0), "workers")
    compare(c2, c, r)
    assert c["max_heap"] > ((160 * 1024 // 32 - 256) // 16 & ~15)

    g = next(g for g in grids if g["name"] == "random00")
    cases = [c for c in g["cases"] if c["heuristic"] == "euclidean"]
    pushes = sorted(c["pushes"] for c in cases)
    cap = pushes[-1] - 1  # below the largest push count only
    assert cap >= 16 and pushes[0] <= cap
    res = run_grid(g, cases, push_cap=cap)
    over = 0
    for c, r in zip(cases, res):
        if c["pushes"] > cap:
            assert r["status"] == 3 and r["path_len"] == 0, c["i"]
            over += 1
        else:
            compare(g, c, r)
    assert 1 <= over < len(cases)


def test_jps2d_scheduling(grids):
    """The 40 pairs of the 64x45 grid, short and long queries together, sixteen times over (320 queries per
    heuristic on 256 workers, so the schedule matters): input order, then longest-first.  Identical, and
    the fixture's."""
    from python_motion_planning_amd import _lib

    g = next(g for g in grids if g["name"] == "random00")
    assert g["occ"].shape == (64, 45)
    cases = g["cases"] * 16
    L, ctx = _lib.load_library(), _lib.context()
    _lib.check(ctx, L.pmp_set_workers_per_cu(ctx, 1), "workers")
    try:
        _lib.check(ctx, L.pmp_astar2d_set_schedule(ctx, 0), "schedule")
        try:
            plain = run_grid(g, cases)
        finally:
            _lib.check(ctx, L.pmp_astar2d_set_schedule(ctx, 1), "schedule")
        lpt = run_grid(g, cases)
    finally:
        _lib.check(ctx, L.pmp_set_workers_per_cu(ctx, 0), "workers")
    for c, a, b in zip(cases, plain, lpt):
        compare(g, c, a)
        compare(g, c, b)
        ne, pl = int(a["n_expanded"]), int(a["path_len"])
        for k in KEYS:
            va, vb = a[k], b[k]
            if k == "path":
                va, vb = va[:pl], vb[:pl]
            elif k.startswith("expand"):
                va, vb = va[:ne], vb[:ne]
            assert np.array_equal(va, vb), (c["i"], k)


def test_jps2d_unwalled_grids_match_restatement():
    """Grids without border walls, where the kernel counts cells outside the grid as obstacles and the
    reference walks off: the yardstick is the restatement (pinned to the reference on walled grids by
    test_jps2d_fixture.py), which pads the grid the same way.  Sides of 1 and 2 cells, one word, exact
    multiples of the word and one past them; endpoints drawn from all cells, obstacles included."""
    rng = np.random.default_rng(7)
    sides = [(1, 1), (1, 9), (2, 2), (3, 40), (31, 33), (32, 32), (33, 32), (64, 33), (33, 64), (65, 31), (40, 96)]
    sides += [(int(rng.integers(3, 71)), int(rng.integers(3, 71))) for _ in range(13)]
    n = 0
    for k, (W, H) in enumerate(sides):
        occ = (rng.random((W, H)) < rng.uniform(0.0, 0.35)).astype(np.uint8)
        rs = J.Restated(occ)
        cases = []
        for j in range(6):
            s, g = (int(rng.integers(W)), int(rng.integers(H))), (int(rng.integers(W)), int(rng.integers(H)))
            heur = "manhattan" if (k + j) % 2 else "euclidean"
            r = rs.plan(s, g, heur)
            closed, parent, gv = (np.array(r[key], dt) for key, dt in (("closed", np.int32), ("parent", np.int32),
                                                                       ("g", np.float64)))
            cases.append(dict(i=(k, j), start=np.array(s), goal=np.array(g), heuristic=heur, found=r["found"],
                              cost=np.float64(r["cost"]), path=np.array(r["path"], np.int32), n_closed=len(closed),
                              digest=J.closed_digest(closed, parent, gv), pushes=r["pushes"], pops=r["pops"],
                              max_heap=r["max_heap"], closed=closed, closed_parent=parent, closed_g=gv))
        g = dict(name="unwalled%dx%d" % (W, H), occ=occ, cases=cases)
        for c, r in zip(cases, run_grid(g)):
            compare(g, c, r)
            n += 1
    assert n == 24 * 6
