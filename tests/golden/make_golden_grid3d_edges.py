"""Generate tests/golden/grid3d_edges.npz by running the REFERENCE's seven 3D grid planners (AStar3D,
Dijkstra3D, GBFS3D, ThetaStar3D, LazyThetaStar3D, DStar3D, LPAStar3D) on walled grids at the sizes
where the kernels change behaviour: above the LDS occupancy thresholds, 256 long, goal sealed.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_grid3d_edges.py

Grid recipe (make_golden_jps3d.py's): rng = RandomState(seed); occ = rng.random_sample(dims) < density;
the six faces occupied; free = argwhere(~occ); start and goal are free[rng.randint(len(free))], drawn
in that order, as Python ints.  Every grid is walled: the reference's isCollision has no bounds test,
so only walled grids pin the kernels' "outside the grid is an obstacle" to it.

Groups (grid seed; endpoints):
  rand33  33x32x32, density 0.2, seeds 3000 and 3001; the recipe's start and goal.
          AStar3D euclidean and manhattan, Dijkstra3D, GBFS3D, ThetaStar3D, LazyThetaStar3D, DStar3D,
          LPAStar3D.
  big65   65x32x32, density 0.25, seed 3010.  AStar3D and ThetaStar3D from the free voxel nearest
          (1, 1, 1) to the one nearest (63, 30, 30); DStar3D and LPAStar3D from the free voxel nearest
          (26, 16, 16) to the one nearest (36, 21, 20) (about 12 apart).
  thin    256x4x4, 4x256x4, 4x4x256 at density 0.03 (seeds 3020, 3021, 3022) and 4x256x4 at 0.1
          (seed 3023: the 2x2 free cross-section is cut, no path); start = the first free voxel with the
          smallest index on the long axis, goal = the first with the largest.  All seven planners.
  sealed  33x32x32, density 0.2, seed 3030, then a 5x5x5 block around (16, 16, 16) freed, its inner
          3x3x3 shell occupied and the centre freed: the goal (16, 16, 16) is sealed in a closed box; the
          recipe's start.  All seven planners.
"Nearest" is the first minimum of the squared distance over argwhere(~occ).

DStar3D runs plan() and two apply_dynamic_obstacles() rounds of two voxels each: a voxel of the
current path (its middle, then the voxel a third of the way; a free voxel drawn by RandomState(seed + 500)
when there is no path) and a voxel outside the grid ((X, 1, 1), then (-1, 2, 2)).  LPAStar3D runs plan()
and two apply_change() calls: block (True) the middle voxel of the path (or the drawn voxel), then toggle
(None) the same voxel.  The rounds are stored, so the tests replay them.

Recorded: the grids (dims, packed occupancy) and per case its group, planner, grid, start, goal,
heuristic (0 euclidean, 1 manhattan), rounds (blocks / changes), per call (0 = plan) cost, path cells
and n (len of CLOSED for the one-shot planners, len(EXPAND) for the other two), the CLOSED cells in
insertion order (kept for rand33 and thin; count and sha1 of the int32 cells for every case) and the
reference's wall time.  Cells are (x*Y + y)*Z + z.
"""
from __future__ import annotations

import hashlib
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import close_figs, import_reference, ragged  # noqa: E402
from make_golden_jps3d import recipe  # noqa: E402

STATIC = ("astar", "dijkstra", "gbfs", "theta_star", "lazy_theta_star")
DYNAMIC = ("dstar", "lpastar")
NR = 2  # rounds after plan() for DStar3D / LPAStar3D


def nearest_free(occ, p):
    free = np.argwhere(occ == 0)
    d = ((free - np.asarray(p)) ** 2).sum(axis=1)
    return tuple(int(v) for v in free[int(np.argmin(d))])


def build_cases():
    """-> (grids [occ], cases [dict(group, planner, grid, start, goal, heur, seed)])"""
    grids, cases = [], []

    def add(group, occ, planners, start, goal, seed):
        grids.append(occ)
        for p in planners:
            name, heur = (p, 0) if isinstance(p, str) else p
            cases.append(dict(group=group, planner=name, grid=len(grids) - 1, start=start, goal=goal, heur=heur,
                              seed=seed))

    for seed in (3000, 3001):
        occ, s, g = recipe(seed, (33, 32, 32), 0.2)
        add("rand33", occ, [("astar", 0), ("astar", 1), "dijkstra", "gbfs", "theta_star", "lazy_theta_star", "dstar",
                            "lpastar"], s, g, seed)
    occ, _, _ = recipe(3010, (65, 32, 32), 0.25)
    add("big65", occ, ["astar", "theta_star"], nearest_free(occ, (1, 1, 1)), nearest_free(occ, (63, 30, 30)), 3010)
    near = (nearest_free(occ, (26, 16, 16)), nearest_free(occ, (36, 21, 20)))
    for p in DYNAMIC:
        cases.append(dict(group="big65", planner=p, grid=len(grids) - 1, start=near[0], goal=near[1], heur=0, seed=3010))
    for seed, dims, density in [(3020, (256, 4, 4), 0.03), (3021, (4, 256, 4), 0.03), (3022, (4, 4, 256), 0.03),
                                (3023, (4, 256, 4), 0.1)]:
        occ, _, _ = recipe(seed, dims, density)
        free = np.argwhere(occ == 0)
        k = free[:, int(np.argmax(dims))]
        s = tuple(int(v) for v in free[int(np.argmin(k))])
        g = tuple(int(v) for v in free[int(np.argmax(k))])
        add("thin", occ, STATIC + DYNAMIC, s, g, seed)
    occ, s, _ = recipe(3030, (33, 32, 32), 0.2)
    occ[14:19, 14:19, 14:19] = 0
    occ[15:18, 15:18, 15:18] = 1
    occ[16, 16, 16] = 0
    assert not occ[s]
    add("sealed", occ, STATIC + DYNAMIC, s, (16, 16, 16), 3030)
    return grids, cases


def run_case(args):
    occ, c = args
    pmp = import_reference()
    from python_motion_planning.global_planner.graph_search import LazyThetaStar3D, ThetaStar3D

    X, Y, Z = occ.shape

    class CachedGrid3D(pmp.Grid3D):
        _gm = None

        @property
        def grid_map(self):
            if self._gm is None:
                self._gm = {(i, j, o) for i in range(X) for j in range(Y) for o in range(Z)}
            return self._gm

    env = CachedGrid3D(X, Y, Z)
    env.update({(int(a), int(b), int(c)) for a, b, c in np.argwhere(occ)})
    start, goal = tuple(c["start"]), tuple(c["goal"])
    heur = "manhattan" if c["heur"] else "euclidean"

    def enc(t):
        assert 0 <= t[0] < X and 0 <= t[1] < Y and 0 <= t[2] < Z, t  # the reference's path stays inside the grid
        return (t[0] * Y + t[1]) * Z + t[2]

    name = c["planner"]
    t0 = time.perf_counter()
    out = dict(cost=[], path=[], n=[], closed=[], rounds=np.zeros((NR, 2, 4), np.int32))
    if name in STATIC:
        if name == "dijkstra":
            p = pmp.Dijkstra3D(start, goal, env)
        else:
            cls = dict(astar=pmp.AStar3D, gbfs=pmp.GBFS3D, theta_star=ThetaStar3D, lazy_theta_star=LazyThetaStar3D)[name]
            p = cls(start, goal, env, heur)
        cost, path, expand = p.plan()
        out["cost"].append(float(cost))
        out["path"].append([enc(t) for t in path])
        out["n"].append(len(expand))
        out["closed"] = [enc(n.current) for n in expand]
    else:
        rng = np.random.RandomState(c["seed"] + 500)
        free = np.argwhere(occ[1:-1, 1:-1, 1:-1] == 0) + 1
        drawn = tuple(int(v) for v in free[rng.randint(len(free))])
        if name == "dstar":
            p = pmp.DStar3D(start, goal, env)
            cost, path, expand = p.plan()
            n = len(expand)
            for r in range(NR + 1):
                out["cost"].append(float(cost))
                out["path"].append([enc(t) for t in path])
                out["n"].append(n)
                if r == NR:
                    break
                reached = len(path) > 3 and path[-1] == goal
                on_path = path[len(path) // 2 if r == 0 else len(path) // 3] if reached else drawn
                blk = [tuple(on_path), (X, 1, 1) if r == 0 else (-1, 2, 2)]
                out["rounds"][r, :, :3] = blk
                cost, path = p.apply_dynamic_obstacles(blk)
                n = len(p.EXPAND)
        else:
            p = pmp.LPAStar3D(start, goal, env, heur)
            cost, path, expand = p.plan()
            out["cost"].append(float(cost))
            out["path"].append([enc(t) for t in path])
            out["n"].append(len(expand))
            v = tuple(path[len(path) // 2]) if len(path) > 3 else drawn
            for r, mode in enumerate((1, 0)):
                out["rounds"][r, 0] = (*v, mode)
                cost, path, expand = p.apply_change(v, True if mode == 1 else None)
                out["cost"].append(float(cost))
                out["path"].append([enc(t) for t in path])
                out["n"].append(len(expand))
    out["seconds"] = time.perf_counter() - t0
    close_figs()
    return out


def has_path(c, r):
    """plan() returned a path that ends at the goal (DStar3D's cost may be inf all the same: its cost()
    takes isCollision(node, parent), which is not symmetric)."""
    X, Y, Z = c["dims"]
    goal = (c["goal"][0] * Y + c["goal"][1]) * Z + c["goal"][2]
    return len(r["path"][0]) > 0 and goal in (r["path"][0][0], r["path"][0][-1])


def main():
    grids, cases = build_cases()
    for c in cases:
        c["dims"] = grids[c["grid"]].shape
    # the longest reference runs (LPAStar3D, DStar3D on the large grids) first
    order = sorted(range(len(cases)), key=lambda i: (cases[i]["planner"] not in DYNAMIC, -grids[cases[i]["grid"]].size))
    with Pool(16) as pool:
        got = pool.map(run_case, [(grids[cases[i]["grid"]], cases[i]) for i in order], chunksize=1)
    res = [None] * len(cases)
    for i, r in zip(order, got):
        res[i] = r
    nopath = sum(not has_path(c, r) for c, r in zip(cases, res))
    assert nopath >= 4, nopath
    for group in ("rand33", "big65", "thin", "sealed"):
        names = {c["planner"] for c in cases if c["group"] == group}
        assert names == set(STATIC + DYNAMIC) or (group == "big65" and names == {"astar", "theta_star", "dstar", "lpastar"}), (group, names)
    for c, r in zip(cases, res):
        if c["group"] == "thin":
            assert has_path(c, r) == (c["seed"] != 3023), (c, r["cost"])
        if c["group"] == "sealed":
            assert not has_path(c, r), c
        if c["planner"] == "dstar" and c["group"] == "rand33":  # a block on the planned path and one outside the grid
            X, Y, Z = c["dims"]
            b = r["rounds"][0]
            assert (b[0][0] * Y + b[0][1]) * Z + b[0][2] in r["path"][0] and b[1][0] == X, c
    keep = [c["group"] in ("rand33", "thin") for c in cases]
    R = NR + 1
    pad = lambda v, f: list(v) + [f] * (R - len(v))  # noqa: E731
    occ_flat, occ_off = ragged([np.packbits(g.ravel()) for g in grids], np.uint8)
    path_flat, path_off = ragged([p for r in res for p in pad(r["path"], [])])
    closed_flat, closed_off = ragged([r["closed"] if k else [] for r, k in zip(res, keep)])
    out = os.path.join(HERE, "grid3d_edges.npz")
    np.savez_compressed(
        out, dims=np.array([g.shape for g in grids], np.int32), occ_bits=occ_flat, occ_off=occ_off,
        group=np.array([c["group"] for c in cases]), planner=np.array([c["planner"] for c in cases]),
        grid=np.array([c["grid"] for c in cases], np.int32), start=np.array([c["start"] for c in cases], np.int32),
        goal=np.array([c["goal"] for c in cases], np.int32), heuristic=np.array([c["heur"] for c in cases], np.int32),
        rounds=np.array([r["rounds"] for r in res], np.int32),
        n_calls=np.array([len(r["cost"]) for r in res], np.int32),
        cost=np.array([pad(r["cost"], float("nan")) for r in res]), n=np.array([pad(r["n"], 0) for r in res], np.int64),
        path=path_flat, path_off=path_off, closed=closed_flat, closed_off=closed_off, closed_kept=np.array(keep),
        closed_sha1=np.array([hashlib.sha1(np.asarray(r["closed"], np.int32).tobytes()).hexdigest() for r in res]),
        ref_seconds=np.array([r["seconds"] for r in res]))
    assert os.path.getsize(out) < 300 * 1024, os.path.getsize(out)
    print("grid3d edge cases", len(res), "no-path cases", nopath, "reference seconds %.1f (max %.1f)" %
          (sum(r["seconds"] for r in res), max(r["seconds"] for r in res)), "bytes", os.path.getsize(out))


if __name__ == "__main__":
    main()
