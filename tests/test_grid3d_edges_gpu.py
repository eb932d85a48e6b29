"""The seven planners of the one-wave-per-query 3D kernels (astar3d.hip: AStar3D, Dijkstra3D, GBFS3D,
ThetaStar3D, LazyThetaStar3D; dstar3d.hip: DStar3D; lpa3d.hip: LPAStar3D) at the grid sizes where the
launchers and kernels change behaviour, against the reference's runs (tests/golden/grid3d_edges.npz)
and the oracle.

Bar: exact -- status, cost bits, path, n_expanded / n_process, the expand list, the reference's push
count.  No tolerances.

What each group of cases reaches:
  33x32x32 (33,792 voxels, 1,056 words > grid3d::kOccLdsWords = 1024): astar3d_kernel<false, 0|1|2> with
      occ3 and los3d<false>; 32x32x32 is the last size of astar3d_kernel<true, *>.
  65x32x32 (66,560 voxels, 2,080 words > 2048): dstar3d_kernel<false> and lpa3d's occ_lds = 0 path, both
      with a per-worker HBM copy of the occupancy that the rounds modify; 64x32x32 is the last LDS size.
  56x56x56 (A*) and 72x72x72 (Theta*) unwalled, corner to corner, one query: more heap entries than a CU's LDS holds
      ((160 KiB - 256 B) / 24 B = 6,816 positions): heap16's HBM spill half under Key3.
  pmp_set_resident_per_cu 0 / 8 / 32: pmp_heap_lds_cap's share; at 32 astar3d.hip on 32x32x32 keeps 32 heap
      positions in LDS, dstar3d.hip on 40x30x30 exactly kMinLdsHeap = 16, and on 64x32x32 it takes the
      "LDS share cannot hold the occupancy too" branch.  (lpa3d.hip sizes U from the workers per CU only.)
  256x2x2, 2x256x2, 2x2x256, 256x16x1, 1x1x40: coordinate 255 in Ent.b's 8-bit fields, dimensions of 1 and 2;
      257 and 0 are refused.
  272 per-query 33x31x33 grids (33,759 voxels, 1,055 words, the last one partial): the q * words stride of
      the HBM occupancy, workers that run more than one query, the longest-first order.
  statuses of the astar3d.hip family: 1, 2, expand_cap < n_expanded, start == goal, occupied and off-grid
      endpoints (the early-exit block of astar3d_kernel)."""
import contextlib
import functools

import numpy as np
import pytest

import grid3d_edges_checks as E

pytestmark = pytest.mark.gpu

# (algo, heuristic) of the astar3d.hip family; Dijkstra3D takes no heuristic
FAMILY = [("astar", "euclidean"), ("astar", "manhattan"), ("dijkstra", "euclidean"), ("gbfs", "euclidean"),
          ("gbfs", "manhattan"), ("theta_star", "euclidean"), ("theta_star", "manhattan"),
          ("lazy_theta_star", "euclidean"), ("lazy_theta_star", "manhattan")]
LDS_BYTES = 160 * 1024  # per CU


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def _grid(seed, dims, density, walled):
    rng = np.random.RandomState(seed)
    occ = (rng.random_sample(dims) < density).astype(np.uint8)
    if walled:
        occ[0], occ[-1] = 1, 1
        occ[:, 0], occ[:, -1] = 1, 1
        occ[:, :, 0], occ[:, :, -1] = 1, 1
    return occ


def _pairs(occ, seed, nq, reach=None):
    """nq (start, goal) pairs of free voxels; with reach, the goal within that Chebyshev distance."""
    rng = np.random.RandomState(seed)
    free = np.argwhere(occ == 0)
    s = free[rng.randint(len(free), size=nq)]
    if reach is None:
        g = free[rng.randint(len(free), size=nq)]
    else:
        g = np.empty_like(s)
        for i in range(nq):
            near = free[(np.abs(free - s[i]).max(axis=1) <= reach)]
            g[i] = near[rng.randint(len(near))]
    return s.astype(np.int32), g.astype(np.int32)


def _ref_static(occ, s, g, algo, heur):
    from oracle import oracle as O

    if algo in ("theta_star", "lazy_theta_star"):
        return O.theta3d(occ, s, g, lazy=algo == "lazy_theta_star", heuristic=heur)
    return O.astar3d(occ, s, g, heur, algo=algo)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items() if hasattr(v, "cpu")}


def _run_static(occ, S, G, algo, heur, **kw):
    from python_motion_planning_amd import batch

    n = int(np.prod(np.asarray(occ).shape[-3:]))
    kw.setdefault("expand_cap", n)
    return _host(batch.astar3d_batch(occ, S, G, heur, counters=True, algo=algo, **kw))


def _assert_static(out, q, ref, algo, tag, all_counters=False):
    tag = (tag, algo, q)
    assert out["status"][q] == ref["status"], (tag, out["status"][q], ref["status"])
    assert _bits(out["cost"][q]) == _bits(ref["cost"]), (tag, out["cost"][q], ref["cost"])
    assert out["n_expanded"][q] == ref["n_expanded"], (tag, out["n_expanded"][q], ref["n_expanded"])
    assert out["path_len"][q] == len(ref["path_cells"]), tag
    assert np.array_equal(out["path"][q, : out["path_len"][q]], ref["path_cells"]), tag
    assert np.array_equal(out["expand"][q, : ref["n_expanded"]], ref["expand_cells"]), tag
    ctr = out["counters"][q]
    assert ctr[0] == ref["n_push"], (tag, ctr, ref["n_push"])  # pushes counted the reference's way
    if algo in ("theta_star", "lazy_theta_star") or all_counters:
        assert ctr[2] == ref["n_iter"], (tag, ctr, ref["n_iter"])
    if algo not in ("theta_star", "lazy_theta_star") or all_counters:
        assert ctr[3] <= ref["max_heap"], (tag, ctr, ref["max_heap"])  # the kernel drops dead duplicates
    if all_counters:
        assert ctr[1] == ref["n_pop"] and ctr[3] == ref["max_heap"], (tag, ctr, ref)


def _ref_dynamic(kind, occ, s, g, rounds, heur="euclidean"):
    from oracle import oracle as O

    if kind == "dstar":
        r = O.dstar3d(occ, s, g, rounds)
        return dict(status=r["status"], cost=r["cost"], n=r["n_process"], paths=r["paths"])
    r = O.lpastar3d(occ, s, g, rounds, heur)
    return dict(status=r["status"], cost=r["cost"], n=r["n_expanded"], paths=r["paths"])


def _run_dynamic(kind, occ, S, G, rounds, heur="euclidean"):
    from python_motion_planning_amd import batch

    if kind == "dstar":
        out = _host(batch.dstar3d_batch(occ, S, G, rounds))
        out["n"] = out.pop("n_process")
    else:
        out = _host(batch.lpastar3d_batch(occ, S, G, rounds, heur))
        out["n"] = out.pop("n_expanded")
    return out


def _assert_dynamic(out, q, ref, tag):
    for r in range(len(ref["cost"])):
        t = (tag, q, r)
        assert out["status"][q, r] == ref["status"][r], (t, out["status"][q, r], ref["status"][r])
        assert _bits(out["cost"][q, r]) == _bits(ref["cost"][r]), (t, out["cost"][q, r], ref["cost"][r])
        assert out["n"][q, r] == ref["n"][r], (t, out["n"][q, r], ref["n"][r])
        assert out["path_len"][q, r] == len(ref["paths"][r]), t
        assert np.array_equal(out["path"][q, r, : out["path_len"][q, r]], ref["paths"][r]), t


def _dynamic_rounds(kind, occ, S, G, seed):
    """Two rounds per query, chosen from the oracle's plan(): DStar3D blocks the middle voxel of the path
    and a voxel outside the grid, then a drawn voxel and one outside; LPAStar3D blocks the middle voxel of
    the path, then toggles a drawn voxel.  occ [nq, X, Y, Z] or [X, Y, Z]."""
    rng = np.random.RandomState(seed)
    X, Y, Z = occ.shape[-3:]
    nq = len(S)
    rounds = np.zeros((nq, 2, 2, 3), np.int32) if kind == "dstar" else np.zeros((nq, 2, 4), np.int32)
    for q in range(nq):
        o = occ[q] if occ.ndim == 4 else occ
        path = _ref_dynamic(kind, o, S[q], G[q], None)["paths"][0]
        drawn = (rng.randint(X), rng.randint(Y), rng.randint(Z))
        v = int(path[len(path) // 2]) if len(path) > 2 else -1
        mid = (v // (Y * Z), (v // Z) % Y, v % Z) if v >= 0 else drawn
        if kind == "dstar":
            rounds[q, 0] = [mid, (X, 0, 0)]
            rounds[q, 1] = [drawn, (0, -1, 0)]
        else:
            rounds[q, 0] = (*mid, 1)
            rounds[q, 1] = (*drawn, 0)
    return rounds


@contextlib.contextmanager
def _knob(name, value):
    """pmp_set_resident_per_cu / pmp_set_workers_per_cu on the shared context, restored to 0."""
    from python_motion_planning_amd import _lib

    L, ctx = _lib.load_library(), _lib.context()
    _lib.check(ctx, getattr(L, name)(ctx, value), name)
    try:
        yield
    finally:
        _lib.check(ctx, getattr(L, name)(ctx, 0), name)


# ---- the reference's runs -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cases():
    return E.cases()


@pytest.mark.parametrize("group", ["rand33", "big65", "thin", "sealed"])
def test_fixture_cases(group):
    """Every case of grid3d_edges.npz through astar3d_batch(algo=...), dstar3d_batch and lpastar3d_batch:
    the reference's cost, path, CLOSED order / len(EXPAND) of every call; status, push count and the
    rest as the oracle has them."""
    n = 0
    for c in _cases():
        if c["group"] != group:
            continue
        got, ref = E.kernel_run(c), E.oracle_run(c)
        E.assert_matches_fixture(c, got)
        assert [int(v) for v in got["status"]] == [int(v) for v in ref["status"]], (c["i"], c["planner"])
        if c["planner"] in E.STATIC:
            assert got["n_push"] == ref["n_push"], (c["i"], c["planner"])
        n += 1
    assert n >= 4


def test_fixture_cases_dropin():
    """The seven drop-in classes on the 256x4x4 cases (DStar3D and LPAStar3D with their rounds) and AStar3D
    on 33x32x32."""
    import python_motion_planning_amd as pmp

    classes = dict(astar=pmp.AStar3D, dijkstra=pmp.Dijkstra3D, gbfs=pmp.GBFS3D, theta_star=pmp.ThetaStar3D,
                   lazy_theta_star=pmp.LazyThetaStar3D, dstar=pmp.DStar3D, lpastar=pmp.LPAStar3D)
    seen = set()
    for c in _cases():
        X, Y, Z = c["occ"].shape
        if not ((X, Y, Z) == (256, 4, 4) or (c["group"] == "rand33" and c["planner"] == "astar")):
            continue
        env = pmp.Grid3D(X, Y, Z)
        env.update({(int(a), int(b), int(d)) for a, b, d in np.argwhere(c["occ"])})
        enc = lambda t: (t[0] * Y + t[1]) * Z + t[2]  # noqa: E731
        s, g = tuple(int(v) for v in c["start"]), tuple(int(v) for v in c["goal"])
        name = c["planner"]
        p = classes[name](s, g, env) if name in ("dijkstra", "dstar") else classes[name](s, g, env, c["heuristic"])
        cost, path, expand = p.plan()
        got = dict(cost=[cost], n=[len(expand)], paths=[[enc(t) for t in path]],
                   closed=[enc(nd.current) for nd in expand] if name in E.STATIC else None)
        for r in range(1, len(c["cost"])):
            if name == "dstar":
                cost, path = p.apply_dynamic_obstacles([tuple(int(v) for v in b) for b in c["blocks"][r - 1]])
                got["n"].append(len(p.EXPAND))
            else:
                x, y, z, mode = (int(v) for v in c["changes"][r - 1])
                cost, path, expand = p.apply_change((x, y, z), None if mode == 0 else mode == 1)
                got["n"].append(len(expand))
            got["cost"].append(cost)
            got["paths"].append([enc(t) for t in path])
        E.assert_matches_fixture(c, got)
        seen.add(name)
    assert seen == set(classes)


# ---- threshold neighbours against the oracle -------------------------------------------------------------
@pytest.mark.parametrize("walled", [True, False], ids=["walled", "unwalled"])
@pytest.mark.parametrize("dims", [(32, 32, 32), (33, 32, 32)], ids=["32x32x32_lds", "33x32x32_hbm"])
def test_astar_family_each_side_of_the_occupancy_threshold(dims, walled):
    """32x32x32 is exactly 1024 words (astar3d_kernel<true, *>), 33x32x32 the first size above
    (astar3d_kernel<false, *>): five queries per launch, every algorithm and heuristic."""
    occ = _grid(4100 + walled, dims, 0.2, walled)
    S, G = _pairs(occ, 4110, 5)
    assert (occ.size + 31) // 32 == (1024 if dims[0] == 32 else 1056)
    for algo, heur in FAMILY:
        out = _run_static(occ, S, G, algo, heur)
        for q in range(len(S)):
            _assert_static(out, q, _ref_static(occ, S[q], G[q], algo, heur), algo, (dims, walled, heur))


@pytest.mark.parametrize("walled", [True, False], ids=["walled", "unwalled"])
@pytest.mark.parametrize("dims", [(64, 32, 32), (65, 32, 32)], ids=["64x32x32_lds", "65x32x32_hbm"])
def test_dstar_lpastar_each_side_of_the_occupancy_threshold(dims, walled):
    """64x32x32 is exactly 2048 words (occupancy in LDS), 65x32x32 the first size above (dstar3d_kernel<false>,
    lpa3d's occ_lds = 0: the working occupancy is a per-worker HBM copy that the rounds modify).  Five
    per-query grids per launch, plan() and two rounds each."""
    occ = np.stack([_grid(4200 + 10 * walled + q, dims, 0.22, walled) for q in range(5)])
    S, G = np.zeros((5, 3), np.int32), np.zeros((5, 3), np.int32)
    for q in range(5):
        s, g = _pairs(occ[q], 4250 + q, 1, reach=9)
        S[q], G[q] = s[0], g[0]
    assert (occ[0].size + 31) // 32 == (2048 if dims[0] == 64 else 2080)
    for kind, heur in [("dstar", "euclidean"), ("lpastar", "euclidean"), ("lpastar", "manhattan")]:
        rounds = _dynamic_rounds(kind, occ, S, G, 4290)
        out = _run_dynamic(kind, occ, S, G, rounds, heur)
        for q in range(5):
            _assert_dynamic(out, q, _ref_dynamic(kind, occ[q], S[q], G[q], rounds[q], heur), (kind, heur, dims, walled))


# ---- heap spill -------------------------------------------------------------------------------------------
SPILL_BAR = 6826  # 160 KiB / 24 B: more entries than the whole CU's LDS could hold


@pytest.mark.parametrize("algo,dims,density", [("astar", (56, 56, 56), 0.3), ("theta_star", (72, 72, 72), 0.35)],
                         ids=["astar_56x56x56", "theta_star_72x72x72"])
def test_heap_spills_to_hbm(algo, dims, density):
    """One corner-to-corner query on an unwalled random grid: the kernel's own maximum heap size
    (counters[:, 3]) is above what the CU's LDS holds, so heap16's HBM half (pop<..., true>, sift_up<...,
    true>, 32 B spill records) carried part of the search -- and every output still equals the oracle's.
    The kernel never inserts an entry whose cell has a pending one at least as good, so its maximum is
    well below the oracle's (25,364 on 41x40x40 at 0.2 becomes about 7,400: too close to the bar); on
    these two grids that rule, restated on the CPU, gives about 11,000 and 12,000."""
    occ = _grid(4300, dims, density, False)
    S = np.array([[0, 0, 0]], np.int32)
    G = np.array([[dims[0] - 1, dims[1] - 1, dims[2] - 1]], np.int32)
    occ[tuple(S[0])] = occ[tuple(G[0])] = 0
    ref = _ref_static(occ, S[0], G[0], algo, "euclidean")
    out = _run_static(occ, S, G, algo, "euclidean")
    print(f"{algo} {dims}: kernel max_heap {out['counters'][0, 3]}, oracle max_heap {ref['max_heap']}, "
          f"n_expanded {ref['n_expanded']}")
    _assert_static(out, 0, ref, algo, dims)
    assert ref["status"] == 0
    assert out["counters"][0, 3] > SPILL_BAR, (out["counters"][0], ref["max_heap"])


# ---- LDS share ---------------------------------------------------------------------------------------------
def _same_outputs(a, b, tag):
    assert a.keys() == b.keys(), tag
    for k in a:
        if k in ("path", "expand"):  # rows are defined up to path_len / n_expanded
            n = a["path_len"] if k == "path" else np.minimum(a["n_expanded"], a[k].shape[-1])
            for idx in np.ndindex(n.shape):
                assert np.array_equal(a[k][idx][: n[idx]], b[k][idx][: n[idx]]), (tag, k, idx)
        elif k == "cost":
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (tag, k)
        else:
            assert np.array_equal(a[k], b[k]), (tag, k)


def test_lds_share_astar_family():
    """pmp_set_resident_per_cu 0 / 8 / 32 on 32x32x32 (4,096 B of occupancy in LDS): at 32 residents the
    share is 5,120 B and (5120 - 256 - 4096) / 24 = 32 heap positions stay in LDS, everything deeper spills.
    The launcher's "keep the occupancy in HBM" branch cannot be reached from astar3d.hip: the largest LDS
    occupancy is kOccLdsWords * 4 = 4,096 B and the smallest share 160 KiB / 32, which leaves those 32
    positions, twice kMinLdsHeap.  Outputs are identical across the settings and equal to the oracle."""
    assert (((LDS_BYTES // 32 - 256 - 1024 * 4) // 24) & ~15) == 32
    occ = _grid(4400, (32, 32, 32), 0.2, False)
    S, G = _pairs(occ, 4410, 5)
    for algo, heur in FAMILY:
        refs = [_ref_static(occ, S[q], G[q], algo, heur) for q in range(len(S))]
        first = None
        for resident in (0, 8, 32):
            with _knob("pmp_set_resident_per_cu", resident):
                out = _run_static(occ, S, G, algo, heur)
            for q in range(len(S)):
                _assert_static(out, q, refs[q], algo, ("resident", resident, heur))
            if first is None:
                first = out
            _same_outputs(first, out, (algo, heur, resident))


@pytest.mark.parametrize("dims", [(40, 30, 30), (64, 32, 32)], ids=["40x30x30_heap16", "64x32x32_hbm_fallback"])
def test_lds_share_dstar_lpastar(dims):
    """pmp_set_resident_per_cu 0 / 8 / 32.  At 32 residents dstar3d.hip's share is 5,120 B: on 40x30x30 (1,125
    words, 4,512 B) (5120 - 256 - 4512) / 16 = 22 -> 16 = kMinLdsHeap heap positions; on 64x32x32 (8,192 B)
    nothing is left, the launcher keeps the occupancy in HBM (dstar3d_kernel<false>) and the heap gets
    (5120 - 256) / 16 = 304.  lpa3d.hip takes its U share from the workers per CU only; it runs under the
    same settings.  Outputs identical across the settings and equal to the oracle."""
    words = (dims[0] * dims[1] * dims[2] + 31) // 32
    share = LDS_BYTES // 32 - 256 - ((words * 4 + 15) & ~15)
    assert ((share // 16) & ~15) == 16 if dims[0] == 40 else share < 0
    occ = _grid(4500, dims, 0.2, False)
    S, G = _pairs(occ, 4510, 5, reach=9)
    for kind in ("dstar", "lpastar"):
        rounds = _dynamic_rounds(kind, occ, S, G, 4520)
        refs = [_ref_dynamic(kind, occ, S[q], G[q], rounds[q]) for q in range(len(S))]
        first = None
        for resident in (0, 8, 32):
            with _knob("pmp_set_resident_per_cu", resident):
                out = _run_dynamic(kind, occ, S, G, rounds)
            for q in range(len(S)):
                _assert_dynamic(out, q, refs[q], (kind, dims, "resident", resident))
            if first is None:
                first = out
            for k in ("status", "cost", "n", "path_len"):
                assert np.array_equal(first[k].view(np.int64) if k == "cost" else first[k],
                                      out[k].view(np.int64) if k == "cost" else out[k]), (kind, resident, k)


# ---- dimension limit ------------------------------------------------------------------------------------------
LIMIT_DIMS = [(256, 2, 2), (2, 256, 2), (2, 2, 256), (256, 16, 1), (1, 1, 40)]


def _limit_case(dims):
    """Unwalled; the start at index 0 and the goal at the last index of the long axis (255, or 39)."""
    occ = _grid(4600 + dims[0] + dims[2], dims, 0.0 if dims == (1, 1, 40) else (0.15 if dims[2] == 1 else 0.02), False)
    a = int(np.argmax(dims))
    s, g = [0, 0, 0], [0, 0, 0]
    g[a] = dims[a] - 1
    occ[tuple(s)] = occ[tuple(g)] = 0
    return occ, np.array([s, g], np.int32), np.array([g, s], np.int32)  # there and back


@pytest.mark.parametrize("dims", LIMIT_DIMS, ids=["x".join(map(str, d)) for d in LIMIT_DIMS])
def test_dimension_limit(dims):
    """Coordinates up to 255 (Ent.b packs x, y, z into 8 bits each; kMaxDim3 = 256) and dimensions of 1 and
    2, all seven planners, there and back."""
    occ, S, G = _limit_case(dims)
    found = 0
    for algo, heur in FAMILY:
        out = _run_static(occ, S, G, algo, heur)
        for q in range(2):
            ref = _ref_static(occ, S[q], G[q], algo, heur)
            _assert_static(out, q, ref, algo, (dims, heur))
            found += ref["status"] == 0
    assert found == 2 * len(FAMILY)
    for kind in ("dstar", "lpastar"):
        rounds = _dynamic_rounds(kind, occ, S, G, 4690)
        out = _run_dynamic(kind, occ, S, G, rounds)
        for q in range(2):
            _assert_dynamic(out, q, _ref_dynamic(kind, occ, S[q], G[q], rounds[q]), (kind, dims))


@pytest.mark.parametrize("dims", [(257, 2, 2), (2, 257, 2), (2, 2, 257), (0, 4, 4), (4, 0, 4), (4, 4, 0)],
                         ids=lambda d: "x".join(map(str, d)))
def test_dimension_out_of_range_is_refused(dims):
    """A dimension of 257 or 0: PMP_EINVAL from all three entry points, before anything is launched (the
    outputs keep what they held)."""
    import torch

    from python_motion_planning_amd import _lib, batch

    L, ctx = _lib.load_library(), _lib.context()
    X, Y, Z = dims
    words = torch.zeros(max(1, (X * Y * Z + 31) // 32), dtype=torch.int32, device="cuda")
    s = torch.zeros((1, 3), dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.PMPError, match=r"X, Y, Z must be in \[1, 256\]"):
        batch.dstar3d_batch(dims, s, s, occ_bits=words)
    with pytest.raises(_lib.PMPError, match=r"X, Y, Z must be in \[1, 256\]"):
        batch.lpastar3d_batch(dims, s, s, occ_bits=words)
    i32 = dict(dtype=torch.int32, device="cuda")
    cost = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    plen, path, nexp, status = (torch.full(sh, -7, **i32) for sh in [(1,), (1, 8), (1,), (1,)])
    for algo in range(5):
        rc = L.pmp_graph3d_batch(ctx, _lib.stream_ptr(), algo, words.data_ptr(), 0, X, Y, Z, 0, s.data_ptr(), s.data_ptr(),
                                 1, cost.data_ptr(), plen.data_ptr(), path.data_ptr(), 8, nexp.data_ptr(), None, 0, None,
                                 status.data_ptr())
        with pytest.raises(_lib.PMPError, match=r"X, Y, Z must be in \[1, 256\]"):
            _lib.check(ctx, rc, "pmp_graph3d_batch")
    torch.cuda.synchronize()
    assert float(cost[0]) == -7.0 and int(status[0]) == -7 and int(plen[0]) == -7 and int(nexp[0]) == -7


# ---- per-query batch above the threshold ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _per_query_batch():
    nq, dims = 272, (33, 31, 33)
    occ = np.stack([_grid(4700 + q, dims, 0.2, q % 2 == 0) for q in range(nq)])
    S, G = np.zeros((nq, 3), np.int32), np.zeros((nq, 3), np.int32)
    for q in range(nq):
        s, g = _pairs(occ[q], 4990 + q, 1, reach=6)
        S[q], G[q] = s[0], g[0]
    # endpoints off the grid at a few indices (their neighbours in the batch are checked like every query)
    S[5], G[17], S[100], G[271] = (-1, 3, 3), (256, 1, 1), (33, 0, 0), (0, -5, 0)
    S[200], G[200] = (40, 40, 40), (-3, 0, 0)
    return occ, S, G


@pytest.mark.parametrize("algo,workers_per_cu", [("astar", 0), ("astar", 1), ("theta_star", 1)],
                         ids=["astar", "astar_1_worker_per_cu", "theta_star_1_worker_per_cu"])
def test_per_query_grids_above_the_threshold(algo, workers_per_cu):
    """272 queries, each on its own 33x31x33 grid: 33,759 voxels = 1,055 words with a partial last word, read
    from HBM at q * words.  By default every query gets its own worker (the launcher takes two per CU for
    257..512 queries); with pmp_set_workers_per_cu(1) 256 workers take the 272 queries in the
    longest-first order, so some workers reset their state and run a second query."""
    occ, S, G = _per_query_batch()
    assert occ[0].size == 33759 and (occ[0].size + 31) // 32 == 1055 and occ[0].size % 32 != 0
    with _knob("pmp_set_workers_per_cu", workers_per_cu):
        out = _run_static(occ, S, G, algo, "euclidean", expand_cap=2048)
    off = 0
    for q in range(len(S)):
        ref = _ref_static(occ[q], S[q], G[q], algo, "euclidean")
        assert ref["n_expanded"] <= 2048
        _assert_static(out, q, ref, algo, "per-query")
        if q in (5, 17, 100, 200, 271):
            assert ref["status"] == 1 and ref["n_expanded"] <= 1
            off += 1
    assert off == 5


# ---- statuses of the astar3d.hip family --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _status_grid():
    """Unwalled 33x32x32 (occupancy from HBM) with a free voxel sealed in a closed box."""
    occ = _grid(4800, (33, 32, 32), 0.15, False)
    occ[19:24, 19:24, 19:24] = 0
    occ[20:23, 20:23, 20:23] = 1
    occ[21, 21, 21] = 0
    occ[2, 2, 2] = occ[9, 12, 7] = 0
    occ[30, 3, 3] = 1
    return occ


STATUS_QUERIES = [
    ("sealed goal", (2, 2, 2), (21, 21, 21)), ("found", (2, 2, 2), (9, 12, 7)), ("start == goal", (9, 12, 7), (9, 12, 7)),
    ("start occupied", (30, 3, 3), (9, 12, 7)), ("goal occupied", (2, 2, 2), (30, 3, 3)),
    ("start == goal, occupied", (30, 3, 3), (30, 3, 3)), ("start negative", (-1, 2, 2), (9, 12, 7)),
    ("goal >= 256", (2, 2, 2), (256, 300, 7)), ("both off the grid", (2, -2, 2), (2, 2, 32)),
    ("start at X", (33, 2, 2), (9, 12, 7)), ("goal at Z", (2, 2, 2), (9, 12, 32)),
    ("start == goal, off the grid", (40, 40, 40), (40, 40, 40))]


@pytest.mark.parametrize("algo", ["astar", "dijkstra", "gbfs", "theta_star", "lazy_theta_star"])
def test_statuses(algo):
    """Unreachable goal: status 1, inf, path_len 0, n_expanded the oracle's.  start == goal, occupied
    endpoints, endpoints off the grid (negative, >= the dimension, >= 256): for the last the kernel's early
    exit sets n_expanded and all four counters itself, and they equal the oracle's."""
    occ = _status_grid()
    S = np.array([q[1] for q in STATUS_QUERIES], np.int32)
    G = np.array([q[2] for q in STATUS_QUERIES], np.int32)
    out = _run_static(occ, S, G, algo, "euclidean")
    for q, (name, s, g) in enumerate(STATUS_QUERIES):
        ref = _ref_static(occ, S[q], G[q], algo, "euclidean")
        off = not all(0 <= v < d for v, d in zip(s + g, occ.shape * 2))
        _assert_static(out, q, ref, algo, name, all_counters=off)
        if name == "found":
            assert ref["status"] == 0 and len(ref["path_cells"]) >= 3
        elif name in ("start == goal", "start == goal, occupied"):  # the goal test comes before any collision test
            assert ref["status"] == 0 and ref["cost"] == 0.0 and len(ref["path_cells"]) == 1 and ref["n_expanded"] == 1, name
        else:
            assert ref["status"] == 1 and np.isinf(ref["cost"]) and len(ref["path_cells"]) == 0, name
        if off:
            in_grid = all(0 <= v < d for v, d in zip(s, occ.shape))
            assert out["n_expanded"][q] == int(in_grid) and list(out["counters"][q]) == [1, 1, int(in_grid), 1], name
    assert out["n_expanded"][0] > 10000  # the sealed goal: the start's whole component was closed


def _graph3d_raw(occ, S, G, algo, path_cap, expand_cap, fill=-7):
    """pmp_graph3d_batch on output tensors filled beforehand, with one more expand row than queries."""
    import torch

    from python_motion_planning_amd import _lib
    from python_motion_planning_amd.env import pack_bits

    L, ctx = _lib.load_library(), _lib.context()
    X, Y, Z = occ.shape
    nq = len(S)
    i32 = dict(dtype=torch.int32, device="cuda")
    words = torch.as_tensor(pack_bits(occ).view(np.int32), device="cuda")
    s, g = torch.as_tensor(S, **i32).contiguous(), torch.as_tensor(G, **i32).contiguous()
    out = dict(cost=torch.full((nq,), float(fill), dtype=torch.float64, device="cuda"), path_len=torch.full((nq,), fill, **i32),
               path=torch.full((nq + 1, path_cap), fill, **i32), n_expanded=torch.full((nq,), fill, **i32),
               status=torch.full((nq,), fill, **i32), expand=torch.full((nq + 1, expand_cap), fill, **i32),
               counters=torch.full((nq, 4), fill, dtype=torch.int64, device="cuda"))
    rc = L.pmp_graph3d_batch(ctx, _lib.stream_ptr(), _lib.ALGOS[algo], words.data_ptr(), 0, X, Y, Z, 0, s.data_ptr(),
                             g.data_ptr(), nq, out["cost"].data_ptr(), out["path_len"].data_ptr(), out["path"].data_ptr(),
                             path_cap, out["n_expanded"].data_ptr(), out["expand"].data_ptr(), expand_cap,
                             out["counters"].data_ptr(), out["status"].data_ptr())
    _lib.check(ctx, rc, "pmp_graph3d_batch")
    return _host(out)


@pytest.mark.parametrize("algo", ["astar", "dijkstra", "gbfs", "theta_star", "lazy_theta_star"])
def test_path_cap_and_expand_cap_overflow(algo):
    """path_cap one below the true length: status 2 with the true path_len and the cost kept, nothing
    written to the path row or past it.  expand_cap below n_expanded: the count stays exact, the first
    expand_cap cells are the oracle's and nothing is written past them: the row after the last query's,
    which no query owns, keeps its fill."""
    occ = _status_grid()
    S = np.array([(2, 2, 2), (9, 12, 7)], np.int32)
    G = np.array([(9, 12, 7), (2, 2, 2)], np.int32)
    refs = [_ref_static(occ, S[q], G[q], algo, "euclidean") for q in range(2)]
    plen = [len(r["path_cells"]) for r in refs]
    nexp = [r["n_expanded"] for r in refs]
    assert min(plen) > 2 and min(nexp) > 4
    path_cap, expand_cap = max(plen) - 1, min(nexp) // 2
    out = _graph3d_raw(occ, S, G, algo, path_cap, expand_cap)
    for q in range(2):
        over = plen[q] > path_cap
        assert out["status"][q] == (2 if over else 0), (q, out["status"][q])
        assert out["path_len"][q] == plen[q] and _bits(out["cost"][q]) == _bits(refs[q]["cost"]), q
        if over:
            assert (out["path"][q] == -7).all(), q
        else:
            assert np.array_equal(out["path"][q, : plen[q]], refs[q]["path_cells"]) and (out["path"][q, plen[q]:] == -7).all(), q
        assert out["n_expanded"][q] == nexp[q] and out["counters"][q, 0] == refs[q]["n_push"], q
        assert np.array_equal(out["expand"][q], refs[q]["expand_cells"][:expand_cap]), q
    assert (out["path"][2] == -7).all() and (out["expand"][2] == -7).all()
    assert any(p > path_cap for p in plen)
