"""Generate tests/golden/grid2d_edges.npz by running the REFERENCE's nine 2D grid planners (AStar, Dijkstra,
GBFS, ThetaStar, LazyThetaStar, JPS, DStar, LPAStar, DStarLite) on the walled grids of the 2D coordinate-limit
and switch-size tests (tests/grid2d_edges_checks.py: FIXTURE_GRIDS, fixture_case_list), where
test_grid2d_edges_gpu.py leans on the oracle far beyond the sizes it had been compared at.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_grid2d_edges.py

Only walled grids: the reference's collision test has no bounds check, so off an unwalled grid it walks
on.  Grids are stored by recipe (the builders of grid2d_edges_checks.py) with the SHA-1 of their occupied
cell indices; the cases are
  corridor_x 8192x3, corridor_y 3x8192   (1, 1) -> (8190, 1) / (1, 8190): AStar (and back with manhattan),
                                         Dijkstra, GBFS, JPS, DStar, LPAStar, DStarLite; ThetaStar and
                                         LazyThetaStar on corridor_x and on corridor_y_theta 3x4096
  lds_last_48x383, sq_last_54x307        the first drawn pair of the tests' 64: all nine planners, AStar with
                                         both heuristics
  strip_8192x48                          end to end: all nine planners (LPAStar and DStarLite take 2.5 minutes
                                         each, the others under 30 s)
The reference may raise: DStar, LPAStar and DStarLite on the corridors, JPS past Python's recursion limit.
The exception's name is recorded, as the other fixtures do.

Recorded per case: grid, planner, heuristic (0 euclidean, 1 manhattan), start, goal, raised, cost, n
(len(CLOSED) for the one-shot planners, len(EXPAND) for DStar / LPAStar / DStarLite), the path cells
(x * H + y, in the planner's own order), the SHA-1 of the CLOSED cells (int32, insertion order; '' where the
planner keeps none).  The file is written with fixed zip timestamps and without wall times, so a second run
reproduces it byte for byte; the reference's seconds are printed.
"""
from __future__ import annotations

import io
import os
import sys
import time
import zipfile
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import grid2d_edges_checks as E  # noqa: E402
from make_golden import close_figs, import_reference, obstacles_of, ragged  # noqa: E402

ONE_SHOT = ("astar", "dijkstra", "gbfs", "theta_star", "lazy_theta_star", "jps")


def run_case(case):
    name, planner, heur, start, goal = case
    occ = E.fixture_grid(name)
    pmp = import_reference()
    W, H = occ.shape
    env = pmp.Grid(W, H)
    env.update(obstacles_of(occ))
    cls = dict(astar=pmp.AStar, dijkstra=pmp.Dijkstra, gbfs=pmp.GBFS, theta_star=pmp.ThetaStar,
               lazy_theta_star=pmp.LazyThetaStar, jps=pmp.JPS, dstar=pmp.DStar, lpastar=pmp.LPAStar,
               dstarlite=pmp.DStarLite)[planner]
    p = cls(tuple(start), tuple(goal), env) if planner == "dstar" else cls(tuple(start), tuple(goal), env, heur)
    enc = lambda t: t[0] * H + t[1]  # noqa: E731
    t0 = time.perf_counter()
    out = dict(raised="", cost=float("nan"), path=[], n=0, closed_sha1="")
    try:
        cost, path, expand = p.plan()
        out.update(cost=float(cost), path=[enc(t) for t in path])
        if planner in ONE_SHOT:
            closed = [enc(n.current) for n in expand]
            out.update(n=len(closed), closed_sha1=E.sha1_cells(closed))
        else:
            out.update(n=len(p.EXPAND))
    except Exception as e:  # noqa: BLE001  ValueError / KeyError / AttributeError (the dynamic planners), RecursionError (JPS)
        out.update(raised=type(e).__name__, n=len(getattr(p, "EXPAND", [])))
    out["seconds"] = time.perf_counter() - t0
    close_figs()
    return out


def save_npz(fname, **arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(fname, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    cases = E.fixture_case_list()
    # the longest runs first: the strip's, LPAStar and DStarLite ahead of the others
    order = sorted(range(len(cases)), key=lambda i: (-E.fixture_grid(cases[i][0]).size, cases[i][1] not in ("lpastar", "dstarlite")))
    with Pool(16) as pool:
        got = pool.map(run_case, [cases[i] for i in order], chunksize=1)
    res = [None] * len(cases)
    for i, r in zip(order, got):
        res[i] = r
    names = sorted(E.FIXTURE_GRIDS)
    assert {c[1] for c in cases} == set(E.PLANNERS)
    for c, r in zip(cases, res):
        if c[0].startswith("corridor") and c[1] in ("astar", "dijkstra", "gbfs", "theta_star", "lazy_theta_star"):
            assert not r["raised"] and r["cost"] == (4093.0 if c[0] == "corridor_y_theta" else 8189.0), (c, r["raised"], r["cost"])
    path_flat, path_off = ragged([r["path"] for r in res])
    out = os.path.join(HERE, E.FIXTURE)
    save_npz(
        out, grid_name=np.array(names), grid_dims=np.array([E.fixture_grid(n).shape for n in names], np.int32),
        grid_sha1=np.array([E.sha1_cells(np.flatnonzero(E.fixture_grid(n))) for n in names]),
        grid=np.array([c[0] for c in cases]), planner=np.array([c[1] for c in cases]),
        heuristic=np.array([c[2] == "manhattan" for c in cases], np.int32), start=np.array([c[3] for c in cases], np.int32),
        goal=np.array([c[4] for c in cases], np.int32), raised=np.array([r["raised"] for r in res]),
        cost=np.array([r["cost"] for r in res]), n=np.array([r["n"] for r in res], np.int64), path=path_flat, path_off=path_off,
        closed_sha1=np.array([r["closed_sha1"] for r in res]))
    assert os.path.getsize(out) < 300 * 1024, os.path.getsize(out)
    print("grid2d edge cases", len(res), "raised", {(c[0], c[1]): r["raised"] for c, r in zip(cases, res) if r["raised"]},
          "reference seconds %.1f (max %.1f)" % (sum(r["seconds"] for r in res), max(r["seconds"] for r in res)),
          "bytes", os.path.getsize(out))


if __name__ == "__main__":
    main()
