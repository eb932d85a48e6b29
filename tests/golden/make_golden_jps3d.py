"""Generate tests/golden/jps3d_runs.npz by running the REFERENCE JPS3D
(global_planner/graph_search/jps3d.py) on random walled grids and six hand-made cases.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_jps3d.py

Grid recipe (seed = 1000, 1001, ... over the groups in order): rng = RandomState(seed);
occ = rng.random_sample(dims) < density; the six faces occupied; free = argwhere(~occ); start and goal
are free[rng.randint(len(free))], drawn in that order, as Python ints (with numpy integers the
reference's isCollision adds np.bool_s and skips the corner cells -- another planner).

The reference runs on a Grid3D whose grid_map returns one cached set (same values; the reference's
property rebuilds the X*Y*Z-tuple set at every access) and in a JPS3D whose jump counts the calls
made with one of env.motions itself (the 26 per non-goal expansion).

Recorded per case: dims, packed occupancy, start, goal, heuristic (0 euclidean, 1 manhattan), cost,
path cells, CLOSED cells in insertion order with each node's parent cell and g, `expansions` (every
pop that was not skipped: top-level jump calls / 26, plus the goal's when it was reached) and the
reference's wall time.  Cells are (x*Y + y)*Z + z.
"""
from __future__ import annotations

import os
import sys
import time
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import close_figs, import_reference, ragged  # noqa: E402

# (dims, density, runs, alternate heuristics)
GROUPS = [((16, 14, 12), 0.15, 80, False), ((21, 15, 11), 0.25, 40, True), ((12, 10, 8), 0.35, 80, False),
          ((72, 7, 7), 0.05, 8, False), ((40, 30, 30), 0.2, 4, False), ((18, 16, 12), 0.0, 2, False)]
HAND_DIMS, HAND_DENSITY, HAND_SEED = (10, 9, 8), 0.15, 2000


def recipe(seed, dims, density):
    rng = np.random.RandomState(seed)
    occ = rng.random_sample(dims) < density
    occ[0], occ[-1] = True, True
    occ[:, 0], occ[:, -1] = True, True
    occ[:, :, 0], occ[:, :, -1] = True, True
    free = np.argwhere(~occ)
    start = tuple(int(v) for v in free[rng.randint(len(free))])
    goal = tuple(int(v) for v in free[rng.randint(len(free))])
    return occ.astype(np.uint8), start, goal


def hand_cases():
    """start == goal; start occupied; goal occupied; goal sealed in a closed box (10x9x8); two runs of
    an empty 72x7x7 corridor."""
    occ, s, g = recipe(HAND_SEED, HAND_DIMS, HAND_DENSITY)
    cases = [(occ, s, s, 0)]
    o = occ.copy()
    o[s] = 1
    cases.append((o, s, g, 0))
    o = occ.copy()
    o[g] = 1
    cases.append((o, s, g, 0))
    o = occ.copy()
    o[3:8, 3:8, 2:7] = 0
    o[4:7, 4:7, 3:6] = 1
    o[5, 5, 4] = 0
    cases.append((o, (1, 1, 1) if not o[1, 1, 1] else s, (5, 5, 4), 0))
    assert not cases[3][0][cases[3][1]]
    # jumps longer than 64 steps: an empty walled 72x7x7 corridor, along its axis and across it
    long_occ, _, _ = recipe(HAND_SEED, (72, 7, 7), 0.0)
    cases.append((long_occ, (1, 3, 3), (70, 3, 3), 0))
    cases.append((long_occ, (70, 5, 1), (1, 1, 5), 0))
    return cases


def run_jps3d(args):
    occ, start, goal, heur = args
    pmp = import_reference()
    X, Y, Z = occ.shape

    class CachedGrid3D(pmp.Grid3D):
        _gm = None

        @property
        def grid_map(self):
            if self._gm is None:
                self._gm = {(i, j, o) for i in range(X) for j in range(Y) for o in range(Z)}
            return self._gm

    class CountingJPS3D(pmp.JPS3D):
        top_jumps = 0

        def jump(self, node, motion):
            if id(motion) in self._motion_ids:
                self.top_jumps += 1
            return super().jump(node, motion)

    env = CachedGrid3D(X, Y, Z)
    env.update({(int(a), int(b), int(c)) for a, b, c in np.argwhere(occ)})
    p = CountingJPS3D(tuple(start), tuple(goal), env, "manhattan" if heur else "euclidean")
    p._motion_ids = {id(m) for m in env.motions}
    t0 = time.perf_counter()
    cost, path, expand = p.plan()
    dt = time.perf_counter() - t0
    close_figs()
    assert p.top_jumps % 26 == 0
    enc = lambda t: (t[0] * Y + t[1]) * Z + t[2]  # noqa: E731
    return dict(cost=float(cost), path=[enc(t) for t in path], closed=[enc(n.current) for n in expand],
                parent=[enc(n.parent) for n in expand], g=[float(n.g) for n in expand],
                expansions=p.top_jumps // 26 + (1 if path else 0), seconds=dt)


def main():
    cases = []
    seed = 1000
    for dims, density, runs, alternate in GROUPS:
        for k in range(runs):
            occ, s, g = recipe(seed, dims, density)
            cases.append((occ, s, g, k % 2 if alternate else 0))
            seed += 1
    cases += hand_cases()
    with Pool(16) as pool:
        res = pool.map(run_jps3d, cases, chunksize=1)
    reexp = sum(r["expansions"] > len(r["closed"]) for r in res)
    nopath = sum(not r["path"] for r in res)
    assert reexp >= 30 and nopath >= 5, (reexp, nopath)
    occ_flat, occ_off = ragged([np.packbits(c[0].ravel()) for c in cases], np.uint8)
    path_flat, path_off = ragged([r["path"] for r in res])
    closed_flat, closed_off = ragged([r["closed"] for r in res])
    parent_flat, _ = ragged([r["parent"] for r in res])
    g_flat, _ = ragged([r["g"] for r in res], np.float64)
    out = os.path.join(HERE, "jps3d_runs.npz")
    np.savez_compressed(
        out, dims=np.array([c[0].shape for c in cases], np.int32), occ_bits=occ_flat, occ_off=occ_off,
        start=np.array([c[1] for c in cases], np.int32), goal=np.array([c[2] for c in cases], np.int32),
        heuristic=np.array([c[3] for c in cases], np.int32), cost=np.array([r["cost"] for r in res]),
        path=path_flat, path_off=path_off, closed=closed_flat, closed_off=closed_off, closed_parent=parent_flat,
        closed_g=g_flat, expansions=np.array([r["expansions"] for r in res], np.int64),
        ref_seconds=np.array([r["seconds"] for r in res]))
    assert os.path.getsize(out) < 300 * 1024, os.path.getsize(out)
    print("jps3d runs", len(res), "re-expansion cases", reexp, "no-path cases", nopath,
          "reference seconds %.2f" % sum(r["seconds"] for r in res), "bytes", os.path.getsize(out))


if __name__ == "__main__":
    main()
