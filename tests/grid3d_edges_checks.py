"""Loader of tests/golden/grid3d_edges.npz (make_golden_grid3d_edges.py) and the oracle / kernel runs its
two test modules share: one case = one reference planner on one walled grid, with the rounds DStar3D and
LPAStar3D were given after plan()."""
import hashlib

import numpy as np

from golden_io import load_npz, seg

FIXTURE = "grid3d_edges.npz"
STATIC = ("astar", "dijkstra", "gbfs", "theta_star", "lazy_theta_star")
DYNAMIC = ("dstar", "lpastar")
R = 3  # calls stored per case: plan() and two rounds (the one-shot planners use the first only)


def sha1_cells(cells):
    return hashlib.sha1(np.ascontiguousarray(cells, dtype=np.int32).tobytes()).hexdigest()


def cases():
    z = load_npz(FIXTURE)
    grids = []
    for k in range(len(z["dims"])):
        shape = tuple(int(v) for v in z["dims"][k])
        n = int(np.prod(shape))
        grids.append(np.unpackbits(seg(z["occ_bits"], z["occ_off"], k))[:n].reshape(shape).astype(np.uint8))
    out = []
    for i in range(len(z["planner"])):
        nc = int(z["n_calls"][i])
        planner = str(z["planner"][i])
        rounds = z["rounds"][i]
        out.append(dict(
            i=i, group=str(z["group"][i]), planner=planner, occ=grids[int(z["grid"][i])], start=z["start"][i],
            goal=z["goal"][i], heuristic="manhattan" if z["heuristic"][i] else "euclidean",
            blocks=np.ascontiguousarray(rounds[:, :, :3]) if planner == "dstar" else None,
            changes=np.ascontiguousarray(rounds[:, 0, :]) if planner == "lpastar" else None,
            cost=z["cost"][i][:nc], n=z["n"][i][:nc], paths=[seg(z["path"], z["path_off"], i * R + r) for r in range(nc)],
            closed=seg(z["closed"], z["closed_off"], i) if z["closed_kept"][i] else None,
            closed_sha1=str(z["closed_sha1"][i]), ref_seconds=float(z["ref_seconds"][i])))
    return out


def same_cost(a, b):
    """The same bits; DStar3D's inf and LPAStar3D's 100000.0 are values like any other."""
    return np.asarray(a, np.float64).view(np.int64) == np.asarray(b, np.float64).view(np.int64)


def oracle_run(c):
    """The oracle on one case -> dict(status [], cost [], n [], paths [], closed or None)."""
    from oracle import oracle as O

    p = c["planner"]
    if p in ("astar", "dijkstra", "gbfs"):
        r = O.astar3d(c["occ"], c["start"], c["goal"], c["heuristic"], algo=p)
    elif p in ("theta_star", "lazy_theta_star"):
        r = O.theta3d(c["occ"], c["start"], c["goal"], lazy=p == "lazy_theta_star", heuristic=c["heuristic"])
    elif p == "dstar":
        r = O.dstar3d(c["occ"], c["start"], c["goal"], c["blocks"])
        return dict(status=list(r["status"]), cost=list(r["cost"]), n=list(r["n_process"]), paths=r["paths"], closed=None)
    else:
        r = O.lpastar3d(c["occ"], c["start"], c["goal"], c["changes"], c["heuristic"])
        return dict(status=list(r["status"]), cost=list(r["cost"]), n=list(r["n_expanded"]), paths=r["paths"], closed=None)
    return dict(status=[r["status"]], cost=[r["cost"]], n=[r["n_expanded"]], paths=[r["path_cells"]],
                closed=r["expand_cells"], n_push=r["n_push"], max_heap=r["max_heap"])


def kernel_run(c):
    """The HIP kernels on one case (one launch of one query), in oracle_run's form."""
    from python_motion_planning_amd import batch

    p = c["planner"]
    s, g = c["start"][None], c["goal"][None]
    if p in STATIC:
        out = batch.astar3d_batch(c["occ"], s, g, c["heuristic"], expand_cap=c["occ"].size, counters=True, algo=p)
        pl, ne = int(out["path_len"][0]), int(out["n_expanded"][0])
        ctr = out["counters"][0].cpu().numpy()
        return dict(status=[int(out["status"][0])], cost=[float(out["cost"][0])], n=[ne],
                    paths=[out["path"][0, :pl].cpu().numpy()], closed=out["expand"][0, :ne].cpu().numpy(),
                    n_push=int(ctr[0]), max_heap=int(ctr[3]))
    if p == "dstar":
        out = batch.dstar3d_batch(c["occ"], s, g, c["blocks"][None])
        n = out["n_process"][0].cpu().numpy()
    else:
        out = batch.lpastar3d_batch(c["occ"], s, g, c["changes"][None], c["heuristic"])
        n = out["n_expanded"][0].cpu().numpy()
    pl, path = out["path_len"][0].cpu().numpy(), out["path"][0].cpu().numpy()
    return dict(status=list(out["status"][0].cpu().numpy()), cost=list(out["cost"][0].cpu().numpy()), n=list(n),
                paths=[path[r, : pl[r]] for r in range(len(pl))], closed=None)


def assert_matches_fixture(c, got):
    """`got` (oracle_run / kernel_run) reproduces the reference's record of case c bit for bit."""
    tag = (c["i"], c["group"], c["planner"], c["occ"].shape)
    assert len(got["cost"]) == len(c["cost"]), tag
    for r in range(len(c["cost"])):
        assert same_cost(got["cost"][r], c["cost"][r]), (tag, r, got["cost"][r], c["cost"][r])
        assert int(got["n"][r]) == int(c["n"][r]), (tag, r, got["n"][r], c["n"][r])
        assert np.array_equal(got["paths"][r], c["paths"][r]), (tag, r)
    if c["planner"] in STATIC:
        assert sha1_cells(got["closed"]) == c["closed_sha1"], tag
        if c["closed"] is not None:
            assert np.array_equal(got["closed"], c["closed"]), tag
