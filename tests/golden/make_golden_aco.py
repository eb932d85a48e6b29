"""Generate tests/golden/aco.npz by running the REFERENCE's ACO (global_planner/evolutionary_search/aco.py) with
pyvista and osqp stubbed, as make_golden.py does.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_aco.py

Every case is random.seed(seed) (or the stated setstate), ACO(start, goal, grid, **params).plan() on a map of
aco_checks.grid_occupancy; see CASES.  The reference is not edited: aco.py's `random` is replaced by a proxy
that counts the draws, the planner is a subclass whose Ant registers every ant and takes plan()'s pheromone
dict from the calling frame, and h() is wrapped on the instance to see every roulette term.

Recorded per case: the map (bit-packed), the parameters, the 625 words of random.getstate() before and after
plan() and gauss_next, the returned triple (cost, path as cell ids x * H + y, cost_list) or the exception's
name, found_goal and len(path) of every ant of every iteration, the number of draws, the final pheromone as
[W * H][8] doubles (cell, motion index; 0.0 where there is no edge) for grids up to 21 x 15 and its SHA-256 for
all, the seconds plan() took, and the counts the assertions below use.

Asserted here, as conditions on the fixture (a case that misses one draws another seed, seed + 1000; `denormal`
another beta):
  walls        an ant ends with every neighbour visited (prob_sum == 0, candidates exhausted), and n_cost < max_iter
  adjacent     every path has 2 cells, no draw
  start_is_goal, enclosed   ([], [], []) with draws > 0; enclosed: an ant reaches the step cap
  denormal     a non-zero term below 2**-1022 enters a roulette that draws
  straddle     the generator stands at an odd number of 32-bit outputs, more than 624 draws
  readme_small some iteration before the first success finds nothing
  index_error  the first draw is 1 - 2**-53, the first roulette's cp[-1] is 1 - 2**-52, IndexError with index 12
"""
from __future__ import annotations

import math
import multiprocessing as mp
import os
import random
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import aco_checks as C  # noqa: E402
from make_golden import import_reference, obstacles_of  # noqa: E402


def case(name, seed, grid="empty", W=21, H=15, start=(5, 5), goal=(15, 9), prelude="seed", **kw):
    prm = dict(heuristic_type="euclidean", n_ants=8, alpha=1.0, beta=5.0, rho=0.1, Q=1.0, max_iter=6)
    prm.update(kw)
    return dict(name=name, seed=seed, grid=grid, W=W, H=H, start=start, goal=goal, prelude=prelude, prm=prm)


CASES = [
    case("empty", 1),
    case("walls", 2, grid="walls", start=(3, 7), goal=(17, 7)),
    case("tall", 3, W=15, H=21, start=(3, 3), goal=(11, 17)),
    case("corner", 4, grid="corner", start=(5, 3), goal=(15, 11)),
    case("adjacent", 5, goal=(6, 5)),
    case("start_is_goal", 6, goal=(5, 5), n_ants=3, max_iter=2),
    case("enclosed", 7, grid="enclosed", beta=1.0),
    case("manhattan", 8, heuristic_type="manhattan"),
    case("beta0", 9, beta=0.0),
    case("beta2p5", 10, beta=2.5),
    case("alpha0", 11, alpha=0.0),
    case("rho_q", 12, rho=0.5, Q=5.0),
    case("one_ant", 13, n_ants=1),
    case("iter0", 14, max_iter=0),
    case("iter1", 15, max_iter=1),
    case("denormal", 16, W=51, H=31, goal=(45, 25), beta=190.0, n_ants=4, max_iter=3),
    case("straddle", 17, prelude="straddle", n_ants=8, max_iter=8),
    case("readme_small", 18, grid="readme", W=51, H=31, goal=(45, 25), n_ants=10, max_iter=10),
    case("index_error", 19, start=(2, 5), goal=(17, 11), prelude="crafted", n_ants=2, max_iter=1),
    case("default", 0, grid="readme", W=51, H=31, goal=(45, 25), n_ants=50, max_iter=100),
]


def prepare(c, seed):
    """Put the global generator where the case's plan starts"""
    random.seed(seed)
    if c["prelude"] == "straddle":  # 2 * 3 + 1 outputs of 32 bits: every double's two words straddle an odd index
        for _ in range(3):
            random.random()
        random.getrandbits(32)
    elif c["prelude"] == "crafted":
        random.setstate((3, C.crafted_state(random.getstate()[1]), None))


class Draws:
    """Stands in for the module `random` inside aco.py: counts and remembers the last draw"""

    def __init__(self):
        self.n = 0
        self.first = None
        self.hook = None

    def random(self):
        r = random.random()
        if self.n == 0:
            self.first = r
        self.n += 1
        if self.hook:
            self.hook()
        return r


def run_once(c, seed):
    pmp = import_reference()
    from python_motion_planning.global_planner.evolutionary_search import aco as ref

    W, H = c["W"], c["H"]
    occ = C.grid_occupancy(c["grid"], W, H)
    env = pmp.Grid(W, H)
    env.update(obstacles_of(occ))
    assert [m.current for m in env.motions] == list(C.MOTIONS)
    seen = dict(ants=[], pher=None)

    class Traced(ref.ACO):
        class Ant(ref.ACO.Ant):
            def __init__(self):
                super().__init__()
                seen["ants"].append(self)
                if seen["pher"] is None:
                    seen["pher"] = sys._getframe(1).f_locals["pheromone_edges"]

    prm = c["prm"]
    planner = Traced(c["start"], c["goal"], env, **prm)
    draws = Draws()
    ref.random = draws
    max_steps = W * H / 2 + max(W, H)

    # every roulette term, through h(): the terms of the step in progress are the trailing run with one parent
    terms = []
    stats = dict(denormal=0, first_cp_last=None)
    h_orig = planner.h

    def h_wrapped(node, goal):
        v = h_orig(node, goal)
        if seen["pher"] is not None:
            cur = pmp.Node(node.parent, node.parent, 0, 0)
            t = seen["pher"][(cur, node)] ** prm["alpha"] * (1.0 / v) ** prm["beta"]
            if terms and terms[-1][0] != node.parent:
                terms.clear()
            terms.append((node.parent, t))
        return v

    planner.h = h_wrapped

    def at_draw():
        ts = [t for _, t in terms]
        if any(0.0 < t < 2.0 ** -1022 for t in ts):
            stats["denormal"] += 1
        if stats["first_cp_last"] is None:
            ps = 0.0
            for t in ts:
                ps = ps + t
            p0 = 0
            for t in ts:
                p0 = p0 + t / ps
            stats["first_cp_last"] = p0
        terms.clear()

    draws.hook = at_draw

    prepare(c, seed)
    st_in = random.getstate()
    rec = dict(seed=seed, raised="")
    t0 = time.perf_counter()
    try:
        cost, path, cost_list = planner.plan()
    except IndexError as e:
        rec["raised"] = type(e).__name__
        cost, path, cost_list = [], [], []
    finally:
        ref.random = random
    rec["seconds"] = time.perf_counter() - t0
    st_out = random.getstate()
    assert st_in[0] == 3 and st_out[0] == 3 and len(st_out[1]) == 625
    na, iters = prm["n_ants"], prm["max_iter"]
    ants = seen["ants"]
    if not rec["raised"]:
        assert len(ants) == na * iters
    found = np.zeros(na * iters, np.int32)
    lens = np.zeros(na * iters, np.int32)
    dead = capped = 0
    for i, a in enumerate(ants):
        found[i], lens[i] = a.found_goal, len(a.path)
        if not a.found_goal and a.steps >= max_steps:
            capped += 1
        elif not a.found_goal and not rec["raised"]:
            if all(n.current in a.path_set for n in ref.ACO.getNeighbor(planner, a.current_node)):
                dead += 1
    pher = np.zeros((W * H, 8), np.float64)
    edges = seen["pher"]
    if edges is None:  # no ant was made (max_iter = 0): the initial pheromone
        edges = {(pmp.Node((x, y)), n): 1.0 for x in range(W) for y in range(H) if not occ[x, y]
                 for n in ref.ACO.getNeighbor(planner, pmp.Node((x, y)))}
    for (a, b), v in edges.items():
        pher[a.x * H + a.y, C.MOTIONS.index((b.x - a.x, b.y - a.y))] = v
    if isinstance(cost, list):
        assert cost == [] and path == [] and cost_list == []
    else:
        assert path[0] == c["start"] and path[-1] == c["goal"] and all(isinstance(v, int) for v in cost_list)
    rec.update(state_in=np.array(st_in[1], np.uint32), state_out=np.array(st_out[1], np.uint32),
               gauss=math.nan if st_out[2] is None else st_out[2], found_any=bool(path),
               cost=float(cost) if path else math.nan, path=np.array([x * H + y for x, y in path], np.int32),
               cost_list=np.array(cost_list, np.int32), ant_found=found, ant_len=lens, draws=draws.n, pher=pher,
               dead_ends=dead, capped=capped, denormal_terms=stats["denormal"], first_draw=draws.first,
               first_cp_last=stats["first_cp_last"], occ=occ)
    return rec


def conditions(c, r):
    name, prm = c["name"], c["prm"]
    if name == "walls":
        return r["dead_ends"] >= 1 and 0 < len(r["cost_list"]) < prm["max_iter"]
    if name == "adjacent":
        return r["draws"] == 0 and (r["ant_len"] == 2).all() and r["ant_found"].all() and len(r["path"]) == 2
    if name == "start_is_goal":
        return not r["found_any"] and r["draws"] > 0
    if name == "enclosed":
        return not r["found_any"] and r["draws"] > 0 and r["capped"] >= 1
    if name == "denormal":
        return r["denormal_terms"] >= 1 and r["draws"] > 0
    if name == "straddle":
        return r["draws"] > 624 and r["found_any"]
    if name == "readme_small":
        return 0 < len(r["cost_list"]) < prm["max_iter"]
    if name == "index_error":
        return (r["raised"] == "IndexError" and r["first_draw"] == 1.0 - 2.0 ** -53 and r["first_cp_last"] == 1.0 - 2.0 ** -52
                and int(r["state_out"][624]) == 12 and r["draws"] == 1)
    if name == "iter0":
        return r["draws"] == 0 and not r["found_any"]
    return r["found_any"] and r["draws"] > 0 and not r["raised"]


def run_case(i):
    c = dict(CASES[i])
    seed = c["seed"]
    for _ in range(60):
        rec = run_once(c, seed)
        if conditions(c, rec):
            rec["beta"] = c["prm"]["beta"]
            return i, rec
        print("case", c["name"], "seed", seed, "beta", c["prm"]["beta"], "misses its conditions: draws", rec["draws"],
              "dead", rec["dead_ends"], "capped", rec["capped"], "denormal", rec["denormal_terms"], "n_cost",
              len(rec["cost_list"]), rec["raised"], rec["first_cp_last"], flush=True)
        if c["name"] == "denormal":
            c["prm"] = dict(c["prm"], beta=c["prm"]["beta"] - 2.0)
        else:
            seed += 1000
    raise AssertionError(c["name"])


def pack_list(arrs):
    off = np.zeros(len(arrs) + 1, np.int64)
    off[1:] = np.cumsum([len(a) for a in arrs])
    return np.concatenate(arrs), off


def main():
    order = sorted(range(len(CASES)), key=lambda i: -CASES[i]["prm"]["n_ants"] * CASES[i]["prm"]["max_iter"] * CASES[i]["W"])
    with mp.Pool(min(8, os.cpu_count() or 1)) as pool:
        recs = dict(pool.imap_unordered(run_case, order))
    recs = [recs[i] for i in range(len(CASES))]
    P = [dict(c["prm"], beta=r["beta"]) for c, r in zip(CASES, recs)]
    out = dict(names=np.array([c["name"] for c in CASES]), seed=np.array([r["seed"] for r in recs], np.int64),
               dims=np.array([(c["W"], c["H"]) for c in CASES], np.int32),
               start=np.array([c["start"] for c in CASES], np.int32), goal=np.array([c["goal"] for c in CASES], np.int32),
               heuristic=np.array([p["heuristic_type"] for p in P]), n_ants=np.array([p["n_ants"] for p in P], np.int32),
               max_iter=np.array([p["max_iter"] for p in P], np.int32),
               abrq=np.array([(p["alpha"], p["beta"], p["rho"], p["Q"]) for p in P], np.float64),
               state_in=np.array([r["state_in"] for r in recs], np.uint32),
               state_out=np.array([r["state_out"] for r in recs], np.uint32),
               gauss=np.array([r["gauss"] for r in recs], np.float64), raised=np.array([r["raised"] for r in recs]),
               found_any=np.array([r["found_any"] for r in recs]), cost=np.array([r["cost"] for r in recs], np.float64),
               draws=np.array([r["draws"] for r in recs], np.int64),
               pher_sha256=np.array([C.pheromone_sha256(r["pher"]) for r in recs]),
               ref_seconds=np.array([r["seconds"] for r in recs]), dead_ends=np.array([r["dead_ends"] for r in recs], np.int32),
               capped=np.array([r["capped"] for r in recs], np.int32),
               denormal_terms=np.array([r["denormal_terms"] for r in recs], np.int64))
    out["occ_bits"], out["occ_off"] = pack_list([np.packbits(r["occ"].ravel()) for r in recs])
    for key, dtype in (("path", np.int32), ("cost_list", np.int32), ("ant_found", np.int8), ("ant_len", np.int16)):
        out[key], out[key + "_off"] = pack_list([np.asarray(r[key], dtype).ravel() for r in recs])
    out["pher"], out["pher_off"] = pack_list([r["pher"].ravel() if c["W"] * c["H"] <= C.MAX_FULL_CELLS else np.zeros(0)
                                              for c, r in zip(CASES, recs)])
    fn = os.path.join(HERE, "aco.npz")
    np.savez_compressed(fn, **out)
    assert os.path.getsize(fn) < 900_000, os.path.getsize(fn)
    for c, r in zip(CASES, recs):
        print("%-14s seed %5d beta %5.1f draws %7d n_cost %3d dead %3d capped %2d denormal %4d found %d raised %r %.2f s" % (
            c["name"], r["seed"], r["beta"], r["draws"], len(r["cost_list"]), r["dead_ends"], r["capped"], r["denormal_terms"],
            r["found_any"], r["raised"], r["seconds"]))
    print("bytes", os.path.getsize(fn))


if __name__ == "__main__":
    main()
