"""What test_grid2d_edges_gpu.py, test_grid2d_edges_fixture.py and tests/golden/make_golden_grid2d_edges.py
share: the grid builders and query lists of the 2D coordinate-limit and switch-size cases, the launchers'
size formulas restated, the oracle / kernel runs in one form, the assert helpers, and the loader of
tests/golden/grid2d_edges.npz (the reference's runs on the walled cases)."""
import functools
import hashlib

import numpy as np

from golden_io import load_npz, seg

FIXTURE = "grid2d_edges.npz"
# (engine, tier-2 bits in LDS) of pmp_astar2d_set_engine, as test_astar2d_gpu.py runs them
ENGINES = [(2, 0), (2, 1), (0, 0), (3, 0), (1, 0)]
ENGINE_IDS = ["mq", "mq_t2lds", "wave", "sq", "auto"]
THETA_ENGINES = [(2, 0), (2, 1), (0, 0), (1, 0)]  # the single-query engine has no Theta* variant
THETA_ENGINE_IDS = ["mq", "mq_t2lds", "wave", "auto"]
FAMILY = [("astar", "euclidean"), ("astar", "manhattan"), ("dijkstra", "euclidean"), ("gbfs", "euclidean")]
THETA = [("theta_star", "euclidean"), ("lazy_theta_star", "euclidean")]
CELL_MASK = {False: 0x0FFFFFFF, True: 0x03FFFFFF}  # the cell field of an expand record (Theta*: 26 bits)

# ---- the launchers' size formulas (astar2d.hip, astar2d_sq.hip, jps2d.hip), restated ---------------------------------
LDS_BYTES = 160 * 1024
K_BITS_LDS = 4240      # astar2d.hip kBitsLdsBytes
K_LDSG_MIN_HEAP = 64   # astar2d.hip kLdsgMinHeap
K_SQ_MIN_CAP = 1024    # astar2d_sq.hip kSqMinCap
K_MQ_CAP = 32767       # astar2d_mq.hip kMqCap
K_JPS_LDS_WORDS = 4096  # jps2d.hip kOccLdsWords


def _up16(v):
    return (v + 15) & ~15


def ldsg_bytes(ncell):
    """astar2d.hip ldsg_bytes: occupancy words, state nibbles, G."""
    return _up16((ncell + 31) // 32 * 4) + (((ncell + 7) // 8 + 3) & ~3) * 4 + ncell * 8


def wave_ldsg_cap(ncell, per_cu):
    """LDS heap positions pmp_graph2d_batch leaves beside the LDS grid block at `per_cu` workers per CU
    (the grid moves to LDS while this is >= 64)."""
    b = LDS_BYTES // per_cu - 256 - K_BITS_LDS - ldsg_bytes(ncell)
    return (b // 12) & ~15 if b > 0 else 0


def sq_grid_bytes(ncell):
    return _up16((ncell + 31) // 32 * 4) + _up16(ncell) + ncell * 8


def sq_ldsg(ncell):
    return sq_grid_bytes(ncell) + 12 * K_SQ_MIN_CAP <= LDS_BYTES - 256


def sq_cap(ncell):
    """pmp_astar2d_sq_cap below its upper clamp."""
    cap = (LDS_BYTES - 256 - (sq_grid_bytes(ncell) if sq_ldsg(ncell) else 0)) // 12
    return 0 if cap < K_SQ_MIN_CAP else cap & ~15


def jps_row_words(W, H):
    """jps2d.hip: two row-padded copies, each row a whole number of words with at least one padding bit."""
    return W * ((H + 32) // 32) + H * ((W + 32) // 32)


# ---- grids ---------------------------------------------------------------------------------------------------------------
def walled_random(seed, W, H, density):
    """RandomState(seed).random_sample((W, H)) < density, then the four borders occupied."""
    occ = (np.random.RandomState(seed).random_sample((W, H)) < density).astype(np.uint8)
    occ[0], occ[-1], occ[:, 0], occ[:, -1] = 1, 1, 1, 1
    return occ


def open_random(seed, W, H, density):
    return (np.random.RandomState(seed).random_sample((W, H)) < density).astype(np.uint8)


def corridor(W, H):
    """A walled grid three cells thin whose only free cells are the middle line."""
    occ = np.ones((W, H), np.uint8)
    if H == 3:
        occ[1:-1, 1] = 0
    else:
        assert W == 3
        occ[1, 1:-1] = 0
    return occ


def staircase(n=8192):
    """All obstacles except the cells x == y and x == y + 1: one path of axis steps from corner to corner.
    (The cells x == y alone are not connected: a diagonal step between two occupied corners is a collision.)"""
    occ = np.ones((n, n), np.uint8)
    i = np.arange(n)
    occ[i, i] = 0
    occ[i[1:], i[:-1]] = 0
    return occ


def band(n=8192):
    """|x - y| <= 1 free."""
    occ = staircase(n)
    i = np.arange(n - 1)
    occ[i, i + 1] = 0
    return occ


def nearest_free(occ, p):
    free = np.argwhere(occ == 0)
    d = ((free - np.asarray(p)) ** 2).sum(axis=1)
    return tuple(int(v) for v in free[int(np.argmin(d))])


def pairs(occ, seed, nq):
    """nq (start, goal) pairs drawn from the free cells: RandomState(seed), starts then goals."""
    rng = np.random.RandomState(seed)
    free = np.argwhere(occ == 0)
    s = free[rng.randint(len(free), size=nq)]
    g = free[rng.randint(len(free), size=nq)]
    return s.astype(np.int32), g.astype(np.int32)


def strip_queries(occ):
    """A long strip's three queries: end to end both ways (the free cells nearest the two ends of the
    middle line) and one of about half the length."""
    W, H = occ.shape
    if W >= H:
        a, b, m = nearest_free(occ, (1, H // 2)), nearest_free(occ, (W - 2, H // 2)), nearest_free(occ, (W // 2, H // 2))
    else:
        a, b, m = nearest_free(occ, (W // 2, 1)), nearest_free(occ, (W // 2, H - 2)), nearest_free(occ, (W // 2, H // 2))
    return np.array([a, b, a], np.int32), np.array([b, a, m], np.int32)


# the walled grids the reference fixture covers: name -> (builder, arguments)
FIXTURE_GRIDS = {
    "corridor_x": (corridor, (8192, 3)), "corridor_y": (corridor, (3, 8192)), "corridor_y_theta": (corridor, (3, 4096)),
    "lds_last_48x383": (walled_random, (5100, 48, 383, 0.10)), "sq_last_54x307": (walled_random, (5200, 54, 307, 0.10)),
    "strip_8192x48": (walled_random, (5000, 8192, 48, 0.15)),
}


@functools.lru_cache(maxsize=None)
def fixture_grid(name):
    fn, args = FIXTURE_GRIDS[name]
    occ = fn(*args)
    occ.setflags(write=False)
    return occ


def sha1_cells(cells):
    return hashlib.sha1(np.ascontiguousarray(cells, dtype=np.int32).tobytes()).hexdigest()


def bits(a):
    return np.asarray(a, np.float64).view(np.int64)


# ---- the oracle and the kernels, one query = one dict ---------------------------------------------------------------------
def oracle_static(occ, S, G, algo, heur):
    """[dict(status, cost, n_expanded, path_cells, expand_cells, counters [pushes, pops, expansions, max heap])]"""
    from oracle import oracle as O

    out = []
    for s, g in zip(S, G):
        r = O.astar2d(occ, s, g, heur, algo=algo)
        r["counters"] = [r["n_push"], r["n_pop"], r["n_expanded"], r["max_heap"]]
        out.append(r)
    return out


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items() if hasattr(v, "cpu")}


def run_static(occ, S, G, algo, heur, expand_cap=None, **kw):
    from python_motion_planning_amd import batch

    W, H = occ.shape
    kw.setdefault("path_cap", min(W * H + 1, 1 << 16))
    return host(batch.astar2d_batch(occ, S, G, heur, expand_cap=expand_cap or W * H, counters=True, algo=algo, **kw))


def assert_static(out, q, ref, algo, tag, max_heap_exact=True):
    """Query q of an astar2d_batch output equals the oracle's record: status, cost bits, n_expanded, path,
    expand list, pushes / pops / expansions, and the largest heap (the multi-query engine samples it once
    a step, after the step's pop: there it is only bounded by the oracle's)."""
    tag = (tag, algo, q)
    theta = algo in ("theta_star", "lazy_theta_star")
    assert out["status"][q] == ref["status"], (tag, out["status"][q], ref["status"])
    assert bits(out["cost"][q]) == bits(ref["cost"]), (tag, out["cost"][q], ref["cost"])
    assert out["n_expanded"][q] == ref["n_expanded"], (tag, out["n_expanded"][q], ref["n_expanded"])
    assert out["path_len"][q] == len(ref["path_cells"]), (tag, out["path_len"][q], len(ref["path_cells"]))
    assert np.array_equal(out["path"][q, : out["path_len"][q]], ref["path_cells"]), tag
    e = (out["expand"][q, : ref["n_expanded"]].astype(np.uint32) & CELL_MASK[theta]).astype(np.int32)
    assert np.array_equal(e, ref["expand_cells"]), tag
    ctr = [int(v) for v in out["counters"][q]]
    assert ctr[:3] == ref["counters"][:3], (tag, ctr, ref["counters"])
    if max_heap_exact:
        assert ctr[3] == ref["counters"][3], (tag, ctr, ref["counters"])
    else:
        assert 1 <= ctr[3] <= ref["counters"][3], (tag, ctr, ref["counters"])


def max_heap_exact(engine, nq, ldsg=False):
    """Whether a batch of nq on `engine` reports the oracle's largest heap: not on the multi-query engine
    (engine 2; engine 1 from kMqMinBatch = 1024 queries on, unless the grid block sits in LDS)."""
    return not (engine[0] == 2 or (engine[0] == 1 and nq >= 1024 and not ldsg))


def oracle_dynamic(kind, occ, S, G, heur="euclidean"):
    """kind "lpastar" / "dstarlite" / "dstar" -> [dict(status, cost, n, path_cells, n_push, max_u)]"""
    from oracle import oracle as O

    out = []
    for s, g in zip(S, G):
        if kind == "dstar":
            r = O.dstar2d(occ, s, g)
            out.append(dict(status=r["status"], cost=r["cost"], n=r["n_process"], path_cells=r["path_cells"]))
        else:
            r = O.lpastar2d(occ, s, g, heur, lite=kind == "dstarlite")
            out.append(dict(status=r["status"], cost=r["cost"], n=r["n_expanded"], path_cells=r["path_cells"],
                            n_push=r["n_push"], max_u=r["max_u"]))
    return out


def run_dynamic(kind, occ, S, G, heur="euclidean"):
    from python_motion_planning_amd import batch

    if kind == "dstar":
        out = host(batch.dstar2d_batch(occ, S, G))
        out["n"] = out.pop("n_process")
    else:
        out = host(batch.lpastar2d_batch(occ, S, G, heur, counters=True, lite=kind == "dstarlite"))
        out["n"] = out.pop("n_expanded")
    return out


def assert_dynamic(out, q, ref, kind, tag):
    """Status and len(EXPAND) always; the cost where the planner returns one (status 0, or 1: extractPath
    gave up); the path on status 0; LPA* / D* Lite also the pushes and the longest U."""
    tag = (tag, kind, q)
    assert out["status"][q] == ref["status"], (tag, out["status"][q], ref["status"])
    assert out["n"][q] == ref["n"], (tag, out["n"][q], ref["n"])
    if ref["status"] in (0, 1) and (kind != "dstar" or ref["status"] == 0):
        assert bits(out["cost"][q]) == bits(ref["cost"]), (tag, out["cost"][q], ref["cost"])
    if ref["status"] == 0:
        assert np.array_equal(out["path"][q, : out["path_len"][q]], ref["path_cells"]), tag
    if kind != "dstar":
        ctr = out["counters"][q]
        assert ctr[0] == ref["n_push"] and ctr[3] == ref["max_u"], (tag, ctr, ref["n_push"], ref["max_u"])


def restated_jps(occ, S, G, heur):
    """jps2d_checks.Restated on each query, as the cases test_jps2d_gpu.compare takes."""
    import jps2d_checks as J

    rs = J.Restated(occ)
    out = []
    for i, (s, g) in enumerate(zip(S, G)):
        r = rs.plan(s, g, heur)
        closed, parent, gv = np.array(r["closed"], np.int32), np.array(r["parent"], np.int32), np.array(r["g"], np.float64)
        out.append(dict(i=i, found=r["found"], cost=np.float64(r["cost"]), path=np.array(r["path"], np.int32),
                        n_closed=len(closed), pushes=r["pushes"], pops=r["pops"], max_heap=r["max_heap"], closed=closed,
                        closed_parent=parent, closed_g=gv))
    return out


def run_jps(occ, S, G, heur, refs):
    from python_motion_planning_amd import batch

    ecap = max(c["n_closed"] for c in refs) + 1
    pcap = max(len(c["path"]) for c in refs) + 1
    return host(batch.jps2d_batch(occ, S, G, heur, path_cap=pcap, expand_cap=ecap, counters=True))


def assert_jps(out, q, c, tag):
    tag = (tag, q)
    assert out["status"][q] == (0 if c["found"] else 1), (tag, out["status"][q])
    assert bits(out["cost"][q]) == bits(c["cost"]), (tag, out["cost"][q], c["cost"])
    assert np.array_equal(out["path"][q, : out["path_len"][q]], c["path"]), tag
    ne = int(out["n_expanded"][q])
    assert ne == c["n_closed"], (tag, ne, c["n_closed"])
    assert tuple(int(v) for v in out["counters"][q]) == (c["pushes"], c["pops"], c["n_closed"], c["max_heap"]), tag
    assert np.array_equal(out["expand"][q, :ne], c["closed"]), tag
    assert np.array_equal(out["expand_parent"][q, :ne], c["closed_parent"]), tag
    assert np.array_equal(bits(out["expand_g"][q, :ne]), bits(c["closed_g"])), tag


# ---- the reference's runs (tests/golden/grid2d_edges.npz) -----------------------------------------------------------------
PLANNERS = ("astar", "dijkstra", "gbfs", "theta_star", "lazy_theta_star", "jps", "dstar", "lpastar", "dstarlite")


def fixture_case_list():
    """The cases make_golden_grid2d_edges.py runs: (grid name, planner, heuristic, start, goal).  The two
    corridors end to end (Theta* on the 4096-long one: its H limit), one drawn pair on 48x383 and 54x307,
    and the 8192x48 strip end to end (LPAStar and DStarLite take the reference 2.5 minutes each there)."""
    out = []
    for name, s, g in [("corridor_x", (1, 1), (8190, 1)), ("corridor_y", (1, 1), (1, 8190))]:
        for p in ("astar", "dijkstra", "gbfs", "jps", "dstar", "lpastar", "dstarlite"):
            out.append((name, p, "euclidean", s, g))
        out.append((name, "astar", "manhattan", g, s))
    for p in ("theta_star", "lazy_theta_star"):
        out.append(("corridor_x", p, "euclidean", (1, 1), (8190, 1)))
        out.append(("corridor_y_theta", p, "euclidean", (1, 1), (1, 4094)))
    for name, seed in (("lds_last_48x383", 5110), ("sq_last_54x307", 5210)):
        S, G = pairs(fixture_grid(name), seed, 64)
        s, g = tuple(int(v) for v in S[0]), tuple(int(v) for v in G[0])
        for p in PLANNERS:
            out.append((name, p, "euclidean", s, g))
        out.append((name, "astar", "manhattan", s, g))
    S, G = strip_queries(fixture_grid("strip_8192x48"))
    s, g = tuple(int(v) for v in S[0]), tuple(int(v) for v in G[0])
    for p in PLANNERS:
        out.append(("strip_8192x48", p, "euclidean", s, g))
    return out


def cases():
    """One dict per recorded run: i, grid (name), occ, planner, heuristic, start, goal, raised ('' or the
    exception's name), cost, n (len of CLOSED / EXPAND), path (cells x*H + y, in the planner's own order),
    closed_sha1 (the CLOSED cells in insertion order; '' where the planner keeps none)."""
    z = load_npz(FIXTURE)
    out = []
    for i in range(len(z["planner"])):
        name = str(z["grid"][i])
        occ = fixture_grid(name)
        assert sha1_cells(np.flatnonzero(occ)) == str(z["grid_sha1"][list(z["grid_name"]).index(name)]), name
        out.append(dict(i=i, grid=name, occ=occ, planner=str(z["planner"][i]),
                        heuristic="manhattan" if z["heuristic"][i] else "euclidean", start=z["start"][i], goal=z["goal"][i],
                        raised=str(z["raised"][i]), cost=z["cost"][i], n=int(z["n"][i]), path=seg(z["path"], z["path_off"], i),
                        closed_sha1=str(z["closed_sha1"][i])))
    return out


def oracle_fixture_run(c):
    """The oracle (jps2d_checks.Restated for JPS) on one fixture case -> dict(status, cost, n, path, closed)."""
    from oracle import oracle as O

    p, occ, s, g = c["planner"], c["occ"], c["start"], c["goal"]
    if p in ("astar", "dijkstra", "gbfs", "theta_star", "lazy_theta_star"):
        r = O.astar2d(occ, s, g, c["heuristic"], algo=p)
        return dict(status=r["status"], cost=r["cost"], n=r["n_expanded"], path=r["path_cells"], closed=r["expand_cells"])
    if p == "jps":
        r = restated_jps(occ, [s], [g], c["heuristic"])[0]
        return dict(status=0 if r["found"] else 1, cost=float(r["cost"]), n=r["n_closed"], path=r["path"], closed=r["closed"])
    r = oracle_dynamic(p, occ, [s], [g], c["heuristic"])[0]
    return dict(status=r["status"], cost=r["cost"], n=r["n"], path=r["path_cells"], closed=None)


def kernel_fixture_run(c):
    """The HIP kernels on one fixture case (one launch of one query), in oracle_fixture_run's form."""
    from python_motion_planning_amd import batch

    p, occ, s, g = c["planner"], np.asarray(c["occ"]), c["start"][None], c["goal"][None]
    if p in ("astar", "dijkstra", "gbfs", "theta_star", "lazy_theta_star"):
        out = run_static(occ, s, g, p, c["heuristic"])
        ne, pl = int(out["n_expanded"][0]), int(out["path_len"][0])
        mask = CELL_MASK[p in ("theta_star", "lazy_theta_star")]
        return dict(status=int(out["status"][0]), cost=out["cost"][0], n=ne, path=out["path"][0, :pl],
                    closed=(out["expand"][0, :ne].astype(np.uint32) & mask).astype(np.int32))
    if p == "jps":
        out = host(batch.jps2d_batch(occ, s, g, c["heuristic"], path_cap=len(c["path"]) + 1, expand_cap=c["n"] + 1))
        ne, pl = int(out["n_expanded"][0]), int(out["path_len"][0])
        return dict(status=int(out["status"][0]), cost=out["cost"][0], n=ne, path=out["path"][0, :pl],
                    closed=out["expand"][0, : min(ne, c["n"] + 1)])
    out = run_dynamic(p, occ, s, g, c["heuristic"])
    return dict(status=int(out["status"][0]), cost=out["cost"][0], n=int(out["n"][0]),
                path=out["path"][0, : int(out["path_len"][0])], closed=None)


def assert_matches_fixture(c, got):
    """`got` (oracle_fixture_run, or a kernel run in its form) reproduces the reference's record of case c:
    a run the reference raised on is status 4; otherwise cost bits, len(CLOSED) / len(EXPAND), the path
    and the CLOSED order."""
    tag = (c["i"], c["grid"], c["planner"], c["heuristic"])
    if c["raised"]:
        if c["planner"] == "jps":  # a ray deeper than Python's recursion limit: jps2d.hip does not reproduce it
            assert c["raised"] == "RecursionError", tag
        else:
            assert got["status"] == 4, (tag, c["raised"], got["status"])
        return
    assert got["status"] in (0, 1), (tag, got["status"])
    assert bits(got["cost"]) == bits(c["cost"]), (tag, got["cost"], c["cost"])
    assert int(got["n"]) == c["n"], (tag, got["n"], c["n"])
    assert np.array_equal(got["path"], c["path"]), tag
    if c["closed_sha1"]:
        assert sha1_cells(got["closed"]) == c["closed_sha1"], tag
