"""The 2D grid planners (astar2d.hip, astar2d_mq.hip, astar2d_sq.hip: A*, Dijkstra, GBFS, Theta*, Lazy Theta*;
lpa.hip: LPA*, D* Lite; dstar.hip: D*; jps2d.hip: JPS) at their coordinate limits and at the sizes where
the launchers change path, against the oracle (O.astar2d, O.lpastar2d, O.dstar2d) and, for JPS,
jps2d_checks.Restated.  Both count cells outside the grid as obstacles, as the kernels do; the walled cases
are pinned to the reference by tests/golden/grid2d_edges.npz (test_grid2d_edges_fixture.py).

Bar: exact -- status, cost bits, n_expanded, path, expand list, push / pop / expansion counters, and the
largest heap where the engine samples it as the oracle does.  No tolerances.

A. Coordinate limits (kMaxDim = 8192; the heap entry's 14-bit dx / dy, the Theta* layout's 13-bit dy):
  8192x3, 3x8192 corridors   (1, 1) <-> (8190, 1): dx, dy = +-8189 in the entry code, hkey = 8189^2 through
                             __mul24, sqrt_int_rn(8189^2); 3x4096 for Theta* (H <= 4096), and 8192x3 on every
                             engine that has Theta*.  LPA*, D* Lite and D* report status 4
                             here, as the oracle does (the reference raises).
  8192x2, open               (0, 0) <-> (8191, 1): coordinates 0 and 8191, every expanded cell on a border; Theta*
                             and Lazy Theta* too (dx = +-8191 in their layout).
  8192x48 walled, 15 %       end to end both ways and half way: ~316k expansions a query, heaps of thousands
                             (GBFS: above kMqCap = 32767, so engines 2 and 3 overflow and the host re-runs
                             the query with the full bound); 48x4096 for Theta*; 8192x24 at 10 % for
                             LPA* / D* Lite / D*; 8192x8 at 10 % for JPS (the restatement's time).
  8192^2 staircase           x == y and x == y + 1 free (the cells x == y alone are not connected: a diagonal
                             step between two occupied corners collides), (0, 0) <-> (8191, 8191): |dx| = |dy| =
                             8191, k = 2 * 8191^2, cell 2^26 - 1 in the path and expand records (28-bit cell
                             field), all ceil(8192 sqrt 2) + 1 = 11,587 longest-first bins, a heap of one or
                             two entries.  4 slots reserved.
  8192^2, |x - y| <= 1 free  Dijkstra everywhere; A* euclidean on engine (2, 0) alone, without the overflow
                             re-run: the oracle's largest heap lies in (32000, 32767], just inside kMqCap.
  refusals                   W or H of 0 / 8193 (pmp_graph2d_batch, pmp_jps2d_batch, pmp_lpastar2d_batch,
                             pmp_dstarlite2d_batch), Theta* with H = 4097, pmp_dstar2d_batch with 8193x8192
                             (W * H > 2^26): PMP_EINVAL, a message, outputs untouched.

B. Switch sizes (walled, 10 % obstacles, 64 drawn pairs), each side of the boundary; with
   share = 160 KiB / per_cu - 256, ldsg_bytes(n) = up16(ceil(n / 32) * 4) + up4(ceil(n / 8)) * 4 + 8 n:
  engine 0, 64 slots (per_cu 1)       cap = ((163584 - 4240 - ldsg_bytes) / 12) & ~15: 48x383 = 18,384 cells ->
                                      64 = kLdsgMinHeap, the last LDS grid block (astar2d_kernel<.., true>, nearly
                                      every query spilling past 64 LDS positions); 48x384 = 18,432 -> 16: HBM grid.
  engine 0, 1,024 slots (per_cu 4)    (40704 - 4240 - ldsg_bytes) / 12: 88x47 = 4,136 cells -> 64; 88x48 -> 0.
  engine 0, set_residency(16)         (9984 - 4240 - ldsg_bytes) / 12: 24x24 = 576 cells -> 64; 24x25 -> 32.
  engine 3                            sq_grid_bytes(n) = up16(ceil(n / 32) * 4) + up16(n) + 8 n beside kSqMinCap =
                                      1024 entries of 12 B in 163,584 B: 54x307 = 16,578 cells is the last grid in
                                      LDS (pmp_astar2d_sq_cap = 1024; larger heaps report status 3 and the host
                                      re-runs them), 54x308 is not (cap 13,632).
  engine 1 on 48x384                  nq = 256 (kSqMaxBatch: single-query engine), 257 and 1,023 (one query per
                                      wave), 1,024 (kMqMinBatch: multi-query engine).
  JPS                                 W * ceil((H + 1) / 32) + H * ceil((W + 1) / 32) padded words against
                                      kOccLdsWords = 4096: 255x255 -> 4,080 (LDS), 256x256 -> 4,608 (HBM).
  partial border tiles                unwalled 8x16, 9x17, 15x31, 16x32, 17x33 (the multi-query engine's 8 x 16
                                      cell-state and 4 x 4 G tiles: exact, one past, one short), endpoints in the
                                      corners and on the edges, one start sealed in a corner pocket."""
import contextlib
import functools

import numpy as np
import pytest

import grid2d_edges_checks as E

pytestmark = pytest.mark.gpu


def _ctx():
    from python_motion_planning_amd import _lib

    return _lib, _lib.load_library(), _lib.context()


@contextlib.contextmanager
def _engine(eng):
    """pmp_astar2d_set_engine on the shared context; afterwards launch-sized scratch and the default engine."""
    _lib, L, ctx = _ctx()
    _lib.check(ctx, L.pmp_astar2d_reserve_auto(ctx), "reserve_auto")
    _lib.check(ctx, L.pmp_astar2d_set_engine(ctx, *eng), "engine")
    try:
        yield
    finally:
        _lib.check(ctx, L.pmp_astar2d_reserve_auto(ctx), "reserve_auto")  # before the engine: it re-reserves a kept geometry
        _lib.check(ctx, L.pmp_astar2d_set_engine(ctx, 1, 0), "engine")


@pytest.fixture(params=E.ENGINES, ids=E.ENGINE_IDS)
def engine(request):
    with _engine(request.param):
        yield request.param


@pytest.fixture(params=E.THETA_ENGINES, ids=E.THETA_ENGINE_IDS)
def theta_engine(request):
    with _engine(request.param):
        yield request.param


def _bits_of(occ):
    import torch

    from python_motion_planning_amd import batch

    return batch.occ_bits_device(occ, torch)


def _check_batch(occ, S, G, algos, refs, engine, tag, occ_bits=None, copies=1, ldsg=False, **kw):
    """One launch per (algo, heuristic); every query (and every tiled copy) against its oracle record."""
    nq = len(S) * copies
    for algo, heur in algos:
        out = E.run_static(occ, np.tile(S, (copies, 1)), np.tile(G, (copies, 1)), algo, heur, occ_bits=occ_bits, **kw)
        exact = E.max_heap_exact(engine, nq, ldsg)
        for q in range(nq):
            E.assert_static(out, q, refs[algo, heur][q % len(S)], algo, (tag, heur, engine), max_heap_exact=exact)


@functools.lru_cache(maxsize=None)
def _refs(key):
    """The oracle's records of one group of cases, computed once for every engine: (occ, S, G, {(algo, heur): [..]})"""
    if key[0] == "corridor":
        occ = E.corridor(*key[1:])
        far = (key[1] - 2, 1) if key[2] == 3 else (1, key[2] - 2)
        S, G = np.array([(1, 1), far], np.int32), np.array([far, (1, 1)], np.int32)
        algos = E.FAMILY + (E.THETA if key[2] <= 4096 else [])
    elif key[0] == "open":
        occ = np.zeros((8192, 2), np.uint8)
        S, G = np.array([(0, 0), (8191, 1)], np.int32), np.array([(8191, 1), (0, 0)], np.int32)
        algos = E.FAMILY + E.THETA
    elif key[0] == "strip":
        occ = np.array(E.fixture_grid("strip_8192x48"))
        S, G = E.strip_queries(occ)
        algos = E.FAMILY
    elif key[0] == "strip_theta":
        occ = E.walled_random(5001, 48, 4096, 0.15)
        S, G = E.strip_queries(occ)
        S, G = S[:2], G[:2]
        algos = E.THETA
    elif key[0] == "staircase":
        occ = E.staircase()
        S, G = np.array([(0, 0), (8191, 8191)], np.int32), np.array([(8191, 8191), (0, 0)], np.int32)
        algos = E.FAMILY
    elif key[0] == "band":
        occ = E.band()
        S, G = np.array([(0, 0), (8191, 8191)], np.int32), np.array([(8191, 8191), (0, 0)], np.int32)
        algos = [("dijkstra", "euclidean"), ("astar", "euclidean")]
    elif key[0] == "switch":
        name, seed = {(48, 383): ("lds_last_48x383", 5110), (54, 307): ("sq_last_54x307", 5210)}.get(key[1:], (None, 0))
        if name:  # the two grids the reference fixture covers
            occ = np.array(E.fixture_grid(name))
            S, G = E.pairs(occ, seed, 64)
        else:
            occ = E.walled_random(5300 + key[1] + key[2], key[1], key[2], 0.10)
            S, G = E.pairs(occ, 5310 + key[1] + key[2], 64)
        algos = E.FAMILY
    else:
        occ, S, G = _border_case(*key[1:])
        algos = E.FAMILY + E.THETA
    occ.setflags(write=False)
    return occ, S, G, {a: E.oracle_static(occ, S, G, *a) for a in algos}


# ---- the reference's runs ---------------------------------------------------------------------------------------------------
FIXTURE_KINDS = {"graph": ("astar", "dijkstra", "gbfs", "theta_star", "lazy_theta_star"), "jps": ("jps",), "dstar": ("dstar",),
                 "lpastar": ("lpastar",), "dstarlite": ("dstarlite",)}


def _fixture_runs(grid=None, kind=None):
    """The fixture cases the kernels can be held to: not Theta* on the 8192x3 corridor (seconds a query;
    test_corridor_8192x3_theta holds it to the oracle, which test_grid2d_edges_fixture.py pins to these very
    records), not JPS where the reference hit Python's recursion limit (jps2d.hip does not reproduce that)."""
    return [c for c in E.cases() if (grid is None or (c["grid"] == grid and c["planner"] in FIXTURE_KINDS[kind]))
            and not (c["grid"] == "corridor_x" and "theta" in c["planner"]) and not (c["planner"] == "jps" and c["raised"])]


def _fixture_params():
    kind_of = {p: k for k, ps in FIXTURE_KINDS.items() for p in ps}
    return sorted({(c["grid"], kind_of[c["planner"]]) for c in _fixture_runs()})


@pytest.mark.parametrize("grid,kind", _fixture_params(), ids=lambda v: v)
def test_fixture_cases(grid, kind):
    """Every runnable case of grid2d_edges.npz through the kernels (one query a launch, the default engine):
    the reference's cost, path, len(CLOSED) / len(EXPAND) and CLOSED order; status 4 where it raises.  The
    parameters come from the fixture itself, so every collected case launches at least one query."""
    runs = _fixture_runs(grid, kind)
    assert runs
    for c in runs:
        E.assert_matches_fixture(c, E.kernel_fixture_run(c))


# ---- A. coordinate limits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(8192, 3), (3, 8192)], ids=["8192x3", "3x8192"])
def test_corridor_at_the_coordinate_limit(engine, dims):
    """(1, 1) <-> (8190, 1) along x, and along y: every entry's dx (or dy) runs through 0..+-8189."""
    occ, S, G, refs = _refs(("corridor",) + dims)
    for r in refs["astar", "euclidean"]:
        assert r["status"] == 0 and r["cost"] == 8189.0 and r["n_expanded"] == 8190
    _check_batch(occ, S, G, E.FAMILY, refs, engine, dims)


def test_corridor_3x4096_theta(theta_engine):
    """Theta* / Lazy Theta* along y: dy = +-4093 in the 13-bit field (H = 4096, the layout's limit).  The line
    of sight spans the corridor, so every node's parent is the start."""
    occ, S, G, refs = _refs(("corridor", 3, 4096))
    assert refs["theta_star", "euclidean"][0]["status"] == 0 and len(refs["theta_star", "euclidean"][0]["path_cells"]) == 2
    _check_batch(occ, S, G, E.THETA, refs, theta_engine, (3, 4096))


@pytest.mark.parametrize("algo", ["theta_star", "lazy_theta_star"])
def test_corridor_8192x3_theta(theta_engine, algo):
    """Theta* / Lazy Theta* along x, on every engine that has them: dx = +-8189 in the Theta* layout.  Every
    line-of-sight walk goes back to the start, up to 8,189 cells for each of the 8,190 nodes, which takes a query
    several seconds: one algorithm a case."""
    occ, S, G, refs = _refs(("corridor", 8192, 3))
    assert refs[algo, "euclidean"][0]["status"] == 0 and len(refs[algo, "euclidean"][0]["path_cells"]) == 2
    _check_batch(occ, S, G, [(algo, "euclidean")], refs, theta_engine, (8192, 3))


@pytest.mark.parametrize("dims", [(8192, 3), (3, 8192)], ids=["8192x3", "3x8192"])
def test_corridor_lpastar_dstarlite_dstar_report_the_reference_raising(dims):
    """lpa.hip and dstar.hip on the corridors: status 4 and the oracle's len(EXPAND), both ways."""
    occ, S, G, _ = _refs(("corridor",) + dims)
    for kind in ("lpastar", "dstarlite", "dstar"):
        refs = E.oracle_dynamic(kind, occ, S, G)
        assert [r["status"] for r in refs] == [4, 4], kind
        out = E.run_dynamic(kind, occ, S, G)
        for q in range(2):
            E.assert_dynamic(out, q, refs[q], kind, dims)


def test_open_strip_touches_coordinates_0_and_8191(engine):
    """8192x2 without walls or obstacles, (0, 0) <-> (8191, 1): every cell is a border cell.  A* keeps ~24.5k
    entries: above the LDS-tier multi-query limit (16,383) and the single-query capacity (13,632), whose
    overflow the host re-runs.  GBFS runs on engine 0 with an explicit capacity."""
    occ, S, G, refs = _refs(("open",))
    assert refs["astar", "euclidean"][0]["max_heap"] > 16383
    algos = [a for a in E.FAMILY if a[0] != "gbfs"]
    _check_batch(occ, S, G, algos, refs, engine, "open")
    if engine == (0, 0):
        _check_batch(occ, S, G, [("gbfs", "euclidean")], refs, engine, "open", reserve_slots=2, heap_cap=1 << 16)


@pytest.mark.parametrize("algo", ["theta_star", "lazy_theta_star"])
def test_open_strip_theta(theta_engine, algo):
    """Theta* / Lazy Theta* on the open 8192x2 grid, (0, 0) <-> (8191, 1): dx = +-8191 in the Theta* layout, live
    border cells at x = 0 and x = 8191, lines of sight along both border rows.  One algorithm a case."""
    occ, S, G, refs = _refs(("open",))
    assert all(r["status"] == 0 and len(r["path_cells"]) <= 3 for r in refs[algo, "euclidean"])
    _check_batch(occ, S, G, [(algo, "euclidean")], refs, theta_engine, "open")


def test_strip_8192x48(engine):
    """8192x48 walled, 15 % obstacles: end to end both ways (|dx| = 8189) and half way."""
    occ, S, G, refs = _refs(("strip",))
    a = refs["astar", "euclidean"]
    assert all(r["status"] == 0 for r in a) and a[0]["n_expanded"] > 250_000 and a[2]["n_expanded"] > 100_000
    assert abs(int(S[0, 0]) - int(G[0, 0])) >= 8180
    assert refs["gbfs", "euclidean"][0]["max_heap"] > E.K_MQ_CAP  # overflows engines 2 and 3: re-run with the full bound
    _check_batch(occ, S, G, E.FAMILY, refs, engine, "strip")


def test_strip_48x4096_theta(theta_engine):
    """48x4096 walled, 15 % obstacles, end to end along y both ways: |dy| up to 4093 in the 13-bit field."""
    occ, S, G, refs = _refs(("strip_theta",))
    assert all(r["status"] == 0 and r["n_expanded"] > 100_000 for r in refs["theta_star", "euclidean"])
    assert abs(int(S[0, 1]) - int(G[0, 1])) >= 4085
    _check_batch(occ, S, G, E.THETA, refs, theta_engine, "strip_theta")


@pytest.mark.parametrize("kind", ["lpastar", "dstarlite", "dstar"])
def test_strip_8192x24_lpastar_dstarlite_dstar(kind):
    """8192x24 walled, 10 % obstacles, the strip's three queries."""
    occ = E.walled_random(5002, 8192, 24, 0.10)
    S, G = E.strip_queries(occ)
    refs = E.oracle_dynamic(kind, occ, S, G)
    assert all(r["n"] > 70_000 for r in refs)
    out = E.run_dynamic(kind, occ, S, G)
    for q in range(3):
        E.assert_dynamic(out, q, refs[q], kind, "strip24")


def test_strip_8192x8_jps():
    """8192x8 walled, 10 % obstacles (the height at which the restatement takes under 3 s), both heuristics."""
    occ = E.walled_random(5003, 8192, 8, 0.10)
    S, G = E.strip_queries(occ)
    for heur, sl in (("euclidean", slice(0, 2)), ("manhattan", slice(2, 3))):
        refs = E.restated_jps(occ, S[sl], G[sl], heur)
        assert all(c["n_closed"] > 5_000 for c in refs)
        out = E.run_jps(occ, S[sl], G[sl], heur, refs)
        for q, c in enumerate(refs):
            E.assert_jps(out, q, c, ("strip8", heur))


def test_staircase_8192_squared(engine):
    """Only the cells x == y and x == y + 1 are free: (0, 0) <-> (8191, 8191).  dx = dy = +-8191 in the first entries, k up
    to 2 * 8191^2 under sqrt_int_rn, cell 2^26 - 1 in the path and expand records, every longest-first bin
    in range.  Four slots reserved (a multi-query slot is ~576 MB of cell state and G)."""
    occ, S, G, refs = _refs(("staircase",))
    for a in E.FAMILY:
        for r in refs[a]:
            assert r["status"] == 0 and r["n_expanded"] == 2 * 8192 - 1 and r["max_heap"] <= 2
            assert max(r["path_cells"][0], r["path_cells"][-1]) == 2 ** 26 - 1
    _check_batch(occ, S, G, E.FAMILY, refs, engine, "staircase", occ_bits=_bits_of(occ), reserve_slots=4, path_cap=16400,
                 expand_cap=16400)


def test_band_8192_squared_dijkstra(engine):
    """|x - y| <= 1 free: Dijkstra's heap stays below 8 entries while it closes all 24,574 cells."""
    occ, S, G, refs = _refs(("band",))
    d = refs["dijkstra", "euclidean"]
    assert all(r["status"] == 0 and r["max_heap"] <= 8 and r["n_expanded"] > 24_000 for r in d)
    _check_batch(occ, S, G, [("dijkstra", "euclidean")], refs, engine, "band", occ_bits=_bits_of(occ), reserve_slots=4,
                 path_cap=8200, expand_cap=24600)


def test_band_8192_squared_astar_heap_just_inside_the_multiquery_limit():
    """A* euclidean on the band, on engine (2, 0) alone and without the overflow re-run: the oracle's largest
    heap is just under kMqCap = 32767, so the query must finish (status 0) with the oracle's counters."""
    occ, S, G, refs = _refs(("band",))
    a = refs["astar", "euclidean"]
    for r in a:
        assert r["status"] == 0 and 32000 < r["max_heap"] <= E.K_MQ_CAP, r["max_heap"]
    with _engine((2, 0)):
        _check_batch(occ, S, G, [("astar", "euclidean")], refs, (2, 0), "band", occ_bits=_bits_of(occ), reserve_slots=4,
                     path_cap=8200, expand_cap=max(r["n_expanded"] for r in a) + 8, retry_overflow=False)


def _raw_outputs(nq=1, fill=-7):
    import torch

    i32 = dict(dtype=torch.int32, device="cuda")
    return dict(cost=torch.full((nq,), float(fill), dtype=torch.float64, device="cuda"), path_len=torch.full((nq,), fill, **i32),
                path=torch.full((nq, 8), fill, **i32), n=torch.full((nq,), fill, **i32),
                n64=torch.full((nq,), fill, dtype=torch.int64, device="cuda"), status=torch.full((nq,), fill, **i32))


def _assert_refused(rc, o, what, pattern):
    import re

    import torch

    _lib, L, ctx = _ctx()
    assert rc == -1, (what, rc)  # PMP_EINVAL
    msg = L.pmp_last_error(ctx).decode()
    assert re.search(pattern, msg), (what, msg)
    with pytest.raises(_lib.PMPError, match=pattern):
        _lib.check(ctx, rc, what)
    torch.cuda.synchronize()
    assert float(o["cost"][0]) == -7.0 and int(o["status"][0]) == -7 and int(o["path_len"][0]) == -7, what
    assert int(o["n"][0]) == -7 and int(o["n64"][0]) == -7 and bool((o["path"] == -7).all()), what


@pytest.mark.parametrize("dims", [(0, 16), (16, 0), (8193, 16), (16, 8193)], ids=lambda d: "x".join(map(str, d)))
def test_dimension_out_of_range_is_refused(dims):
    """W or H of 0 or 8193: PMP_EINVAL with a message from pmp_graph2d_batch (every algorithm),
    pmp_jps2d_batch, pmp_lpastar2d_batch and pmp_dstarlite2d_batch; nothing launched (outputs keep their fill)."""
    import torch

    _lib, L, ctx = _ctx()
    W, H = dims
    words = torch.zeros(max(1, (W * H + 31) // 32), dtype=torch.int32, device="cuda")
    s = torch.ones((1, 2), dtype=torch.int32, device="cuda")
    for algo in range(5):
        o = _raw_outputs()
        rc = L.pmp_graph2d_batch(ctx, _lib.stream_ptr(), algo, words.data_ptr(), W, H, 0, s.data_ptr(), s.data_ptr(), 1,
                                 o["cost"].data_ptr(), o["path_len"].data_ptr(), o["path"].data_ptr(), 8, o["n"].data_ptr(),
                                 None, 0, None, o["status"].data_ptr())
        _assert_refused(rc, o, ("pmp_graph2d_batch", algo), r"W and H must be in \[1, 8192\]|need H <= 4096")
    o = _raw_outputs()
    rc = L.pmp_jps2d_batch(ctx, _lib.stream_ptr(), words.data_ptr(), W, H, 0, s.data_ptr(), s.data_ptr(), 1,
                           o["cost"].data_ptr(), o["path_len"].data_ptr(), o["path"].data_ptr(), 8, o["n"].data_ptr(), None, None,
                           None, 0, 0, None, o["status"].data_ptr())
    _assert_refused(rc, o, "pmp_jps2d_batch", r"W, H must be in \[1, 8192\]")
    for fn in ("pmp_lpastar2d_batch", "pmp_dstarlite2d_batch"):
        o = _raw_outputs()
        rc = getattr(L, fn)(ctx, _lib.stream_ptr(), words.data_ptr(), W, H, 0, s.data_ptr(), s.data_ptr(), 1,
                            o["cost"].data_ptr(), o["path_len"].data_ptr(), o["path"].data_ptr(), 8, o["n"].data_ptr(), None,
                            o["status"].data_ptr())
        _assert_refused(rc, o, fn, r"W and H must be in \[1, 8192\]")


def test_theta_height_limit_and_dstar_cell_limit_are_refused():
    """Theta* / Lazy Theta* with H = 4097 (the 13-bit dy field), pmp_dstar2d_batch with 8193x8192 cells (> 2^26):
    PMP_EINVAL; H = 4096 is accepted and planned."""
    import torch

    _lib, L, ctx = _ctx()
    s = torch.ones((1, 2), dtype=torch.int32, device="cuda")
    words = torch.zeros((8193 * 8192 + 31) // 32, dtype=torch.int32, device="cuda")
    for algo in (3, 4):
        o = _raw_outputs()
        rc = L.pmp_graph2d_batch(ctx, _lib.stream_ptr(), algo, words.data_ptr(), 3, 4097, 0, s.data_ptr(), s.data_ptr(), 1,
                                 o["cost"].data_ptr(), o["path_len"].data_ptr(), o["path"].data_ptr(), 8, o["n"].data_ptr(),
                                 None, 0, None, o["status"].data_ptr())
        _assert_refused(rc, o, ("theta", algo), r"need H <= 4096")
    o = _raw_outputs()
    rc = L.pmp_dstar2d_batch(ctx, _lib.stream_ptr(), words.data_ptr(), 8193, 8192, s.data_ptr(), s.data_ptr(), 1,
                             o["cost"].data_ptr(), o["path_len"].data_ptr(), o["path"].data_ptr(), 8, o["n64"].data_ptr(),
                             o["status"].data_ptr(), 0)
    _assert_refused(rc, o, "pmp_dstar2d_batch", r"W\*H must be in \[1, 2\^26\]")
    occ, S, G, refs = _refs(("corridor", 3, 4096))
    with _engine((0, 0)):
        _check_batch(occ, S, G, E.THETA, refs, (0, 0), "H = 4096")


# ---- B. switch sizes --------------------------------------------------------------------------------------------------------
def _spilling(refs, bar):
    return [q for q, r in enumerate(refs["astar", "euclidean"]) if r["max_heap"] > bar]


@pytest.mark.parametrize("dims", [(48, 383), (48, 384)], ids=["48x383_lds_grid", "48x384_hbm_grid"])
def test_engine0_lds_grid_switch_one_worker_per_cu(dims):
    """64 slots = one worker per CU: 48x383 leaves exactly kLdsgMinHeap = 64 LDS heap positions beside the
    grid block, so nearly every query runs the LDS-grid kernel with the HBM spill; 48x384 keeps the grid in HBM."""
    n = dims[0] * dims[1]
    assert E.wave_ldsg_cap(n, 1) == (64 if dims[1] == 383 else 16)
    occ, S, G, refs = _refs(("switch",) + dims)
    assert len(_spilling(refs, 64)) >= 48
    with _engine((0, 0)):
        _check_batch(occ, S, G, E.FAMILY, refs, (0, 0), dims, reserve_slots=64)


@pytest.mark.parametrize("dims", [(88, 47), (88, 48)], ids=["88x47_lds_grid", "88x48_hbm_grid"])
def test_engine0_lds_grid_switch_four_workers_per_cu(dims):
    """1,024 slots and 1,024 queries (the 64 pairs 16 times) = four workers per CU: 88x47 is the last LDS grid
    block (64 positions), 88x48 the first HBM grid."""
    n = dims[0] * dims[1]
    assert E.wave_ldsg_cap(n, 4) == (64 if dims[1] == 47 else 0)
    occ, S, G, refs = _refs(("switch",) + dims)
    assert len(_spilling(refs, 64)) >= 48
    with _engine((0, 0)):
        _check_batch(occ, S, G, E.FAMILY, refs, (0, 0), dims, copies=16, reserve_slots=1024)


@pytest.mark.parametrize("dims", [(24, 24), (24, 25)], ids=["24x24_lds_grid", "24x25_hbm_grid"])
def test_engine0_lds_grid_switch_at_residency_16(dims):
    """pmp_astar2d_set_residency(ctx, 16): a 9,984-byte share; 24x24 = 576 cells is the last LDS grid block."""
    n = dims[0] * dims[1]
    assert E.wave_ldsg_cap(n, 16) == (64 if dims[1] == 24 else 32)
    occ, S, G, refs = _refs(("switch",) + dims)
    _lib, L, ctx = _ctx()
    with _engine((0, 0)):
        try:
            _lib.check(ctx, L.pmp_astar2d_set_residency(ctx, 16), "residency")
            _check_batch(occ, S, G, E.FAMILY, refs, (0, 0), dims, reserve_slots=64)
        finally:
            _lib.check(ctx, L.pmp_astar2d_reserve_auto(ctx), "reserve_auto")
            _lib.check(ctx, L.pmp_astar2d_set_residency(ctx, 0), "residency")


@pytest.mark.parametrize("dims", [(54, 307), (54, 308)], ids=["54x307_lds_grid_cap_1024", "54x308_cap_13632"])
def test_engine3_lds_grid_switch(dims):
    """The single-query engine: 54x307 is the last grid in LDS, beside kSqMinCap = 1024 heap entries; queries
    that need more report status 3 (once without the re-run) and are re-run on the one-query-per-wave engine
    (the default path); 54x308 keeps the grid in HBM and 13,632 entries in LDS."""
    _lib, L, ctx = _ctx()
    n = dims[0] * dims[1]
    last = dims[1] == 307
    assert E.sq_ldsg(n) == last and E.sq_cap(n) == (1024 if last else 13632)
    assert L.pmp_astar2d_sq_cap(*dims) == (1024 if last else 13632)
    occ, S, G, refs = _refs(("switch",) + dims)
    over = _spilling(refs, 1024)
    assert len(over) >= 16 and not any(r["max_heap"] > 13632 for r in refs["astar", "euclidean"])
    with _engine((3, 0)):
        if last:
            out = E.run_static(occ, S, G, "astar", "euclidean", retry_overflow=False)
            assert np.flatnonzero(out["status"] == 3).tolist() == over
            for q in set(range(64)) - set(over):
                E.assert_static(out, q, refs["astar", "euclidean"][q], "astar", (dims, "no re-run"))
        _check_batch(occ, S, G, E.FAMILY, refs, (3, 0), dims)


@pytest.mark.parametrize("nq", [256, 257, 1023, 1024])
def test_engine1_routing_by_batch_size(nq):
    """Engine 1 on 48x384 (HBM grid): 256 queries go to the single-query engine, 257 and 1,023 to the
    one-query-per-wave engine, 1,024 to the multi-query engine.  The 64 pairs tiled; every copy is the oracle's.
    The routing is inferred from pmp_graph2d_batch's conditions (kSqMaxBatch, kMqMinBatch, restated above), not
    observed: the launcher reports no engine, and the outputs of the three are equal by design, so this test
    shows that each batch size gives the oracle's records, whichever engine served it."""
    occ, S, G, refs = _refs(("switch", 48, 384))
    assert E.wave_ldsg_cap(48 * 384, 1) < 64
    idx = np.arange(nq) % 64
    with _engine((1, 0)):
        for algo, heur in E.FAMILY:
            out = E.run_static(occ, S[idx], G[idx], algo, heur)
            for q in range(nq):
                E.assert_static(out, q, refs[algo, heur][q % 64], algo, ("routing", nq, heur),
                                max_heap_exact=E.max_heap_exact((1, 0), nq))


@pytest.mark.parametrize("side", [255, 256], ids=["255x255_lds", "256x256_hbm"])
def test_jps_padded_rows_each_side_of_the_lds_limit(side):
    """255x255: 4,080 padded words, staged in LDS; 256x256: 4,608, read from HBM.  40 pairs against the restatement."""
    assert (E.jps_row_words(side, side) <= E.K_JPS_LDS_WORDS) == (side == 255)
    assert E.jps_row_words(side, side) == (4080 if side == 255 else 4608)
    occ = E.walled_random(5400 + side, side, side, 0.10)
    S, G = E.pairs(occ, 5410 + side, 40)
    for heur, sl in (("euclidean", slice(0, 20)), ("manhattan", slice(20, 40))):
        refs = E.restated_jps(occ, S[sl], G[sl], heur)
        out = E.run_jps(occ, S[sl], G[sl], heur, refs)
        for q, c in enumerate(refs):
            E.assert_jps(out, q, c, (side, heur))


BORDER_DIMS = [(8, 16), (9, 17), (15, 31), (16, 32), (17, 33)]


def _border_case(W, H):
    """Unwalled, 0-20 % obstacles; a 2x2 pocket in the corner (0, H - 1) sealed off; eight queries whose
    endpoints are the four corners and cells on each edge."""
    k = BORDER_DIMS.index((W, H))
    occ = E.open_random(5500 + k, W, H, 0.05 * k)
    occ[0:3, H - 3:] = 1
    occ[0:2, H - 2:] = 0
    c00, c10, c01, c11 = (0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)
    S = [c00, c11, c10, c01, c11, (W // 2, 0), (0, H // 2), (W - 1, H // 3)]
    G = [c11, c00, c00, c11, c01, (W // 2, H - 1), (W - 1, H // 2), c00]
    for p in S + G:
        assert p in (c01,) or not (p[0] < 3 and p[1] >= H - 3), p
        occ[p] = 0
    return occ, np.array(S, np.int32), np.array(G, np.int32)


@pytest.mark.parametrize("dims", BORDER_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_live_border_cells_and_partial_tiles(engine, dims):
    """Unwalled grids whose last cell-state / G tile is exact, one past and one short in x and in y: the cells
    x = 0, x = W - 1, y = 0, y = H - 1 are expanded and their outside neighbours are obstacles.  Query 3 starts in
    the sealed pocket: OPEN runs dry after its four cells; query 4 seeks it from outside and closes the rest."""
    occ, S, G, refs = _refs(("border",) + dims)
    a = refs["astar", "euclidean"]
    assert a[3]["status"] == 1 and a[3]["n_expanded"] == 4 and a[4]["status"] == 1
    assert a[4]["n_expanded"] > (int((occ == 0).sum()) - 4) // 2
    assert sum(r["status"] == 0 for r in a) >= 5
    algos = E.FAMILY + (E.THETA if engine in E.THETA_ENGINES else [])
    _check_batch(occ, S, G, algos, refs, engine, dims, ldsg=True)
