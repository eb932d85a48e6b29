"""Generate tests/golden/rrt_connect.npz by running the REFERENCE RRTConnect
(global_planner/sample_search/rrt_connect.py) with np.random.seed(seed).

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_rrt_connect.py

Cases:
  readme   README map, (18, 8) -> (37, 18), the class defaults, seeds 0..15
  c3       C3 map, (5, 5) -> (505, 505), max_dist 8, seeds 0..2
  c3long   the same query with the class default max_dist 0.5, seed 0: trees of more than a thousand
           nodes and a path of more than a thousand points
  rate     readme with goal_sample_rate 0.5, seeds 0 and 1: the goal is sampled while the goal-rooted
           tree is forward, so its root is replaced in place many times
  never    README map, (18, 8) -> (27, 13): the goal lies inside rect (26, 7, 2, 12), the goal-rooted
           tree never grows; 400 samples, seeds 0 and 1
  few      readme with sample_num 20, seed 0: the samples run out before the trees meet
  short    README map, (18, 8) -> (18, 9), seed 0

The planner's extractPath is wrapped with a bound on the parent walks (the reference would hang on a
parent cycle), and generateRandomNode / isCollision are counted.  plan() keeps both trees in local
variables only, so they are read from its frame when it returns.

Recorded per case: both trees in dict order (x, y, g; parent as an index into the same tree), tree 0
rooted at the start and tree 1 at the goal; which of them was sample_list_f at the end; the meeting
node's index in each (-1: none); cost; path (start first); len(expand); the iterations run; the
isCollision calls; the draws consumed and the next global draw.
"""
from __future__ import annotations

import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import close_figs, import_reference  # noqa: E402
from make_golden_informed_rrt import C3_Q, NEVER_Q, README_Q, make_env  # noqa: E402

FIXTURE = "rrt_connect.npz"
SHORT_Q = ((18, 8), (18, 9))


class ParentCycle(Exception):
    pass


def run_case(args):
    kind, mapname, seed, sample_num, (start, goal), kw = args
    pmp = import_reference()
    p = pmp.RRTConnect(start, goal, make_env(pmp, mapname), sample_num=sample_num, **kw)
    count = dict(iters=0, coll=0)
    frame_locals = {}

    def extract(boundary, sample_list_b, sample_list_f):
        if p.start.current in sample_list_b:
            sample_list_f, sample_list_b = sample_list_b, sample_list_f
        out = []
        for tree, root in ((sample_list_f, p.start), (sample_list_b, p.goal)):
            node = tree[boundary.current]
            walk, steps = [node], 0
            while node != root:
                node = tree[node.parent]
                walk.append(node)
                steps += 1
                if steps > len(tree):
                    raise ParentCycle()
            out.append(walk)
        cost = out[0][0].g + out[1][0].g
        return cost, [n.current for n in reversed(out[0])] + [n.current for n in out[1][1:]]

    gen, coll = p.generateRandomNode, p.isCollision

    def generate():
        count["iters"] += 1
        return gen()

    def is_collision(a, b):
        count["coll"] += 1
        return coll(a, b)

    p.extractPath, p.generateRandomNode, p.isCollision = extract, generate, is_collision
    plan_code = type(p).plan.__code__

    def prof(frame, event, arg):
        if event == "return" and frame.f_code is plan_code:
            frame_locals.update(frame.f_locals)

    np.random.seed(seed)
    draws0 = np.random.get_state()
    sys.setprofile(prof)
    try:
        cost, path, expand = p.plan()
    finally:
        sys.setprofile(None)
    nxt = np.random.random()
    rs = np.random.RandomState()
    rs.set_state(draws0)
    stream = rs.random_sample(3 * sample_num + 2)
    draws = int(np.flatnonzero(stream == nxt)[0])
    close_figs()
    f, b = frame_locals["sample_list_f"], frame_locals["sample_list_b"]
    forward = 0 if p.start.current in f else 1
    trees = (f, b) if forward == 0 else (b, f)
    assert p.start.current in trees[0] and p.goal.current in trees[1]
    out = dict(forward=forward, iters=count["iters"], coll=count["coll"], next=nxt, draws=draws,
               cost=float(cost), found=path is not None, n_expand=len(expand) if expand is not None else 0,
               path=np.array(path if path else [], np.float64).reshape(-1, 2))
    boundary = [-1, -1]
    for t, tree in enumerate(trees):
        nodes = list(tree.values())
        index = {n.current: i for i, n in enumerate(nodes)}
        assert len(index) == len(nodes)
        out[f"tree{t}"] = np.array([[n.x, n.y, n.g] for n in nodes], np.float64)
        out[f"parent{t}"] = np.array([index[n.parent] for n in nodes], np.int32)
        if path is not None:
            boundary[t] = index[frame_locals["node_new"].current]
    out["boundary"] = np.array(boundary, np.int32)
    if path is not None:
        assert len(expand) == len(trees[0]) + len(trees[1])
        # getExpand's interleave: sample_list_f first, then sample_list_b, index by index
        want = []
        fl, bl = list(f.values()), list(b.values())
        for k in range(max(len(fl), len(bl))):
            want += ([fl[k]] if k < len(fl) else []) + ([bl[k]] if k < len(bl) else [])
        assert all(x is y for x, y in zip(expand, want))
    return out


def main():
    cases = [("readme", "readme", s, 10000, README_Q, {}) for s in range(16)]
    cases += [("c3", "c3", s, 10000, C3_Q, dict(max_dist=8.0)) for s in range(3)]
    cases += [("c3long", "c3", 0, 10000, C3_Q, {})]
    cases += [("rate", "readme", s, 10000, README_Q, dict(goal_sample_rate=0.5)) for s in (0, 1)]
    cases += [("never", "readme", s, 400, NEVER_Q, {}) for s in (0, 1)]
    cases += [("few", "readme", 0, 20, README_Q, {})]
    cases += [("short", "readme", 0, 10000, SHORT_Q, {})]
    with Pool(16) as pool:
        res = pool.map(run_case, cases, chunksize=1)
    by = {}
    for c, r in zip(cases, res):
        by.setdefault(c[0], []).append(r)
        n0, n1 = len(r["tree0"]), len(r["tree1"])
        assert r["draws"] <= 3 * r["iters"] and r["iters"] <= c[3]
        if r["found"]:
            assert tuple(r["path"][0]) == tuple(c[4][0]) and tuple(r["path"][-1]) == tuple(c[4][1])
            assert r["n_expand"] == n0 + n1 and min(r["boundary"]) >= 0
            assert np.array_equal(r["tree0"][r["boundary"][0], :2], r["tree1"][r["boundary"][1], :2])
            assert r["cost"] == r["tree0"][r["boundary"][0], 2] + r["tree1"][r["boundary"][1], 2]
            seg = np.hypot(*(r["path"][1:] - r["path"][:-1]).T)
            assert seg.min() > 1e-9
        else:
            assert r["cost"] == 0 and r["iters"] == c[3] and list(r["boundary"]) == [-1, -1]
    assert all(r["found"] for k in ("readme", "c3", "c3long", "rate", "short") for r in by[k])
    sizes = [len(r["tree0"]) + len(r["tree1"]) for r in by["readme"]]
    assert (min(sizes), max(sizes)) == (109, 282), sizes
    assert all(100 <= len(r["tree0"]) + len(r["tree1"]) <= 140 for r in by["c3"])
    long_ = by["c3long"][0]
    assert len(long_["tree0"]) + len(long_["tree1"]) == 1872 and len(long_["path"]) == 1610
    assert long_["coll"] == 8799
    assert all(not r["found"] and len(r["tree1"]) == 1 for r in by["never"])
    assert not by["few"][0]["found"] and len(by["few"][0]["tree1"]) > 1
    short = by["short"][0]
    assert len(short["tree0"]) + len(short["tree1"]) == 5 and len(short["path"]) == 4
    out = dict(n_cases=np.array(len(cases)))
    for i, (c, r) in enumerate(zip(cases, res)):
        out[f"c{i}_kind"] = np.array(c[0])
        out[f"c{i}_map"] = np.array(c[1])
        out[f"c{i}_seed"] = np.array(c[2])
        out[f"c{i}_sample_num"] = np.array(c[3])
        out[f"c{i}_start"] = np.array(c[4][0], np.float64)
        out[f"c{i}_goal"] = np.array(c[4][1], np.float64)
        out[f"c{i}_max_dist"] = np.array(c[5].get("max_dist", 0.5))
        out[f"c{i}_rate"] = np.array(c[5].get("goal_sample_rate", 0.05))
        for k, v in r.items():
            out[f"c{i}_{k}"] = np.asarray(v)
    path = os.path.join(HERE, FIXTURE)
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 700 * 1024, os.path.getsize(path)
    print("rrt_connect cases", [(c[0], c[2], len(r["tree0"]), len(r["tree1"]), r["forward"], r["iters"], r["coll"],
                                 r["draws"], round(r["cost"], 6), len(r["path"])) for c, r in zip(cases, res)])
    print("bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
