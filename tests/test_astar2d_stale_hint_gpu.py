"""The stale hint of the multi-query 2D engine (astar2d_mq.hip): a pop whose cell is known to be
CLOSED one step ahead skips the 3x3 round, G[pusher] and the parent prefetch.  Only a wrong "stale"
could change a result, so every case runs on engine 2 with both tier-2 placements and every query is
compared with the oracle on status, cost bits, path, n_expanded, the four counters (pushes, pops,
expansions, largest heap) and the closure order.  The shapes are the smallest at which each change of
the root occurs: duplicates of the cell just closed, pushes that reach the root, heaps of 1-3 entries,
an exhausted OPEN, a slot's next query, the 15-query cell-state clear."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_REF = {}  # case name -> (occ, starts, goals, [oracle result per query]); computed once, read only


@pytest.fixture(params=[(2, 0), (2, 1)], ids=["mq", "mq_t2lds"])
def engine(request):
    from python_motion_planning_amd import _lib

    L, ctx = _lib.load_library(), _lib.context()
    _lib.check(ctx, L.pmp_astar2d_set_engine(ctx, *request.param), "engine")
    yield request.param
    _lib.check(ctx, L.pmp_astar2d_set_engine(ctx, 1, 0), "engine")
    _lib.check(ctx, L.pmp_astar2d_reserve_auto(ctx), "reserve_auto")


def _walled(W, H):
    occ = np.zeros((W, H), np.uint8)
    occ[0, :] = occ[-1, :] = occ[:, 0] = occ[:, -1] = 1
    return occ


def _case(name, build, algo="astar"):
    key = (name, algo)
    if key not in _REF:
        from oracle import oracle as O

        occ, S, G = build()
        S, G = np.asarray(S, np.int32).reshape(-1, 2), np.asarray(G, np.int32).reshape(-1, 2)
        _REF[key] = (occ, S, G, [O.astar2d(occ, S[q], G[q], algo=algo) for q in range(len(S))])
    return _REF[key]


def _check(case, algo="astar", copies=1, reserve_slots=None):
    """Run the case's queries (`copies` times over, in one launch) and compare every query."""
    from python_motion_planning_amd import batch

    occ, S, G, ref = case
    W, H = occ.shape
    nq = len(S)
    r = batch.astar2d_batch(occ, np.tile(S, (copies, 1)), np.tile(G, (copies, 1)), path_cap=W * H + 1,
                            expand_cap=W * H, counters=True, algo=algo, reserve_slots=reserve_slots)
    st, cost = r["status"].cpu().numpy(), r["cost"].cpu().numpy()
    ne, pl = r["n_expanded"].cpu().numpy(), r["path_len"].cpu().numpy()
    P, ctr = r["path"].cpu().numpy(), r["counters"].cpu().numpy()
    E = r["expand"].cpu().numpy().astype(np.uint32) & (0x03FFFFFF if "theta" in algo else 0x0FFFFFFF)
    stale = 0
    for k in range(copies * nq):
        o = ref[k % nq]
        at = (algo, k, S[k % nq].tolist(), G[k % nq].tolist())
        assert st[k] == o["status"], at
        assert cost[k].tobytes() == np.float64(o["cost"]).tobytes(), at
        assert ne[k] == o["n_expanded"], at
        assert ctr[k].tolist() == [o["n_push"], o["n_pop"], o["n_expanded"], o["max_heap"]], at
        assert np.array_equal(P[k, : pl[k]], o["path_cells"]), at
        assert np.array_equal(E[k, : ne[k]].astype(np.int32), o["expand_cells"]), at
        stale += o["n_pop"] - o["n_expanded"]
    return stale, sum(o["n_pop"] for o in ref) * copies


def _duplicates(W, H):
    """Open ground: 16 directions (axis, diagonal, knight offsets) from two starts, as far as each goes."""
    occ = _walled(W, H)
    dirs = [(1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1),
            (1, 2), (2, 1), (-1, 2), (-2, 1), (1, -2), (2, -1), (-1, -2), (-2, -1)]

    def free(x, y):
        return 0 <= x < W and 0 <= y < H and occ[x, y] == 0

    S, G = [], []
    for sx, sy in ((W // 2, H // 2), (2, H - 3)):
        for dx, dy in dirs:
            k = 0
            while free(sx + (k + 1) * dx, sy + (k + 1) * dy):
                k += 1
            S.append((sx, sy))
            G.append((sx + k * dx, sy + k * dy))
    return occ, S, G


def _dup_both():
    return [("dup24", lambda: _duplicates(24, 24)), ("dup40x17", lambda: _duplicates(40, 17))]


def _tiny():
    """Heaps of 1-3 entries: start == goal, adjacent cells, a one-cell-wide corridor of length 30."""
    occ = np.ones((32, 3), np.uint8)
    occ[1:31, 1] = 0
    S = [(5, 1), (5, 1), (6, 1), (1, 1), (30, 1), (1, 1)]
    G = [(5, 1), (6, 1), (5, 1), (30, 1), (1, 1), (16, 1)]
    return occ, S, G


def _tiny_diag():
    """start == goal and neighbours (axis and diagonal) on open ground"""
    occ = _walled(8, 8)
    S = [(3, 3), (3, 3), (3, 3), (3, 3), (4, 4)]
    G = [(3, 3), (4, 3), (4, 4), (2, 4), (3, 3)]
    return occ, S, G


def _sealed():
    """A start sealed in a 3x3 room (OPEN runs out after 9 cells) and a goal enclosed by walls (OPEN runs
    out after every open cell), beside queries that succeed."""
    occ = _walled(14, 12)
    occ[2:7, 2] = occ[2:7, 6] = 1
    occ[2, 2:7] = occ[6, 2:7] = 1  # room: cells 3..5 x 3..5
    occ[9:12, 7] = occ[9:12, 9] = 1
    occ[9, 7:10] = occ[11, 7:10] = 1  # the goal (10, 8) enclosed
    S = [(4, 4), (3, 3), (8, 2), (12, 10), (8, 2), (4, 4)]
    G = [(8, 2), (5, 5), (10, 8), (10, 8), (12, 10), (10, 8)]
    return occ, S, G


def test_duplicates_dominate_lone_and_multi(engine):
    """Open ground pushes a cell up to 8 times, so many pops are stale (A*: 4 in 10 here; Dijkstra, in
    test_dijkstra_gbfs, 7 in 10); duplicates of the cell just closed reach the root at once, and
    straight runs push f-ties with a smaller h that become the root.  Once with one query per wave
    (<= 256 queries) and once repeated to 1,024 queries (four per wave)."""
    for name, build in _dup_both():
        case = _case(name, build)
        assert len(case[1]) == 32
        stale, pops = _check(case)
        assert 3 * stale > pops, (name, stale, pops)  # the case is what it claims to be
        _check(case, copies=32)


def test_tiny_heaps(engine):
    assert max(o["max_heap"] for o in _case("tiny", _tiny)[3]) <= 3
    for name, build in (("tiny", _tiny), ("tiny_diag", _tiny_diag)):
        case = _case(name, build)
        _check(case)
        _check(case, copies=64)


def test_open_exhausted_and_invalid_endpoints(engine):
    from python_motion_planning_amd import batch

    case = _case("sealed", _sealed)
    assert [o["status"] for o in case[3]] == [1, 0, 1, 1, 0, 1]
    assert case[3][0]["n_expanded"] == 9
    _check(case)
    _check(case, copies=64)
    # endpoints outside the grid between queries that succeed: no path, and the neighbours' results stand
    occ, S, G, ref = case
    S2, G2 = np.tile(S, (64, 1)), np.tile(G, (64, 1))
    out = np.arange(2, len(S2), 5)
    S2[out[0::2]] = (-1, 3)
    G2[out[1::2]] = (4, 12)
    r = batch.astar2d_batch(occ, S2, G2, path_cap=14 * 12 + 1, counters=True)
    st, cost, ne = r["status"].cpu().numpy(), r["cost"].cpu().numpy(), r["n_expanded"].cpu().numpy()
    pl, ctr = r["path_len"].cpu().numpy(), r["counters"].cpu().numpy()
    assert (st[out] == 1).all() and (cost[out] == 0.0).all() and (pl[out] == 0).all()
    for k in np.setdiff1d(np.arange(len(S2)), out):
        o = ref[k % len(S)]
        assert st[k] == o["status"] and cost[k] == o["cost"] and ne[k] == o["n_expanded"], k
        assert ctr[k].tolist() == [o["n_push"], o["n_pop"], o["n_expanded"], o["max_heap"]], k


def _reuse():
    rng = np.random.default_rng(5)
    occ = (rng.random((48, 48)) < 0.10).astype(np.uint8)
    occ[0, :] = occ[-1, :] = occ[:, 0] = occ[:, -1] = 1
    occ[20:23, 20] = occ[20:23, 22] = occ[20, 20:23] = occ[22, 20:23] = 1  # (21, 21) enclosed
    occ[21, 21] = 0
    free = np.argwhere(occ == 0)
    free = free[(free != (21, 21)).any(axis=1)]
    S = free[rng.integers(len(free), size=2048)].astype(np.int32)
    G = free[rng.integers(len(free), size=2048)].astype(np.int32)
    G[::7] = (21, 21)  # unreachable: the query ends with OPEN exhausted
    S[3::31] = (21, 21)  # sealed start: one expansion
    return occ, S, G


def test_slot_reuse_and_epoch_wrap(engine):
    """2,048 queries on 64 slots: each group serves 32 queries one after another, so the cell states'
    epoch wraps (the 15-query clear) twice per slot, and a hint must not outlive its query."""
    case = _case("reuse", _reuse)
    st = np.array([o["status"] for o in case[3]])
    assert (st == 1).sum() > 250 and (st == 0).sum() > 1500
    _check(case, reserve_slots=64)


@pytest.mark.parametrize("algo", ["dijkstra", "gbfs"])
def test_dijkstra_gbfs(engine, algo):
    for name, build in _dup_both() + [("tiny", _tiny), ("tiny_diag", _tiny_diag)]:
        case = _case(name, build, algo)
        stale, pops = _check(case, algo)
        if algo == "dijkstra" and name.startswith("dup"):
            assert 2 * stale > pops, (name, stale, pops)  # duplicates dominate
        _check(case, algo, copies=12)  # the duplicates cases' 384 queries run four per wave


def _theta_grid():
    rng = np.random.default_rng(5)
    occ = (rng.random((32, 32)) < 0.15).astype(np.uint8)
    occ[0, :] = occ[-1, :] = occ[:, 0] = occ[:, -1] = 1
    free = np.argwhere(occ == 0)
    S = free[rng.integers(len(free), size=48)].astype(np.int32)
    G = free[rng.integers(len(free), size=48)].astype(np.int32)
    return occ, S, G


@pytest.mark.parametrize("algo", ["theta_star", "lazy_theta_star"])
def test_theta_variants(engine, algo):
    case = _case("theta32", _theta_grid, algo)
    _check(case, algo)
    _check(case, algo, copies=8)
