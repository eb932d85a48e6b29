"""HIP RRT-Connect (rrt_connect.hip via pmp_rrt_connect_batch) vs the reference's runs
(tests/golden/rrt_connect.npz, restated sequentially in rrt_connect_checks.py).

Bar, as for RRT / RRT* / Informed RRT*: the node counts of both trees, every parent index, which tree is
forward, the meeting node's indices, iterations, status, the draw count and the path length equal;
coordinates, g, cost and path within 1e-12 relative (the device atan2 / cos / sin are <= 1 ulp from
glibc, which steering feeds into the node coordinates).

The closing allowance.  The greedy loop ends on the exact test node_new_b == node_new, so a last-bit
difference in the final approach can add or drop one node there and nowhere else.  A case may pass
instead when the backward tree's count and the path length differ from the fixture by exactly one (the
same one), every node before the closing approach matches, and the cost matches within 1e-12.  At most
ALLOWANCE_CAP cases of the whole fixture may pass that way; the reference against itself uses it 0 times.
"""
import numpy as np
import pytest

import rrt_connect_checks as C

pytestmark = pytest.mark.gpu

RTOL = 1e-12
ALLOWANCE_CAP = 1
CASES, _Z = C.cases()
README = [i for i, c in enumerate(CASES) if c["kind"] == "readme"]
SHORT = next(i for i, c in enumerate(CASES) if c["kind"] == "short")
C3LONG = next(i for i, c in enumerate(CASES) if c["kind"] == "c3long")


def _launch(idx, **kw):
    """The fixture cases `idx` (one map, one setting) in one launch."""
    from python_motion_planning_amd import batch

    c0 = CASES[idx[0]]
    assert all((CASES[i]["map"], CASES[i]["sample_num"], CASES[i]["max_dist"], CASES[i]["rate"])
               == (c0["map"], c0["sample_num"], c0["max_dist"], c0["rate"]) for i in idx)
    rnd = np.stack([C.stream(CASES[i]) for i in idx])
    out = batch.rrt_connect_batch(C.env_of(c0["map"]), [CASES[i]["start"] for i in idx], [CASES[i]["goal"] for i in idx],
                                  rnd, c0["sample_num"], max_dist=c0["max_dist"], goal_sample_rate=c0["rate"], **kw)
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


@pytest.fixture(scope="module")
def readme_out():
    """README seeds 0..15 and the short query, one launch of 17: shared by the tests below, never changed."""
    return _launch(README + [SHORT])


def _tree(out, q, t):
    n = int(out["n_nodes"][q, t])
    return out["tree_xy"][q, t, :n], out["tree_g"][q, t, :n], out["tree_parent"][q, t, :n]


def _close(a, b):
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= RTOL * np.abs(b)))


def _tree_matches(out, q, c, t, upto=None):
    xy, g, par = _tree(out, q, t)
    ref, rpar = c[f"tree{t}"], c[f"parent{t}"]
    if upto is None:
        if len(g) != len(ref):
            return False
        upto = len(ref)
    return (np.array_equal(par[:upto], rpar[:upto]) and _close(xy[:upto], ref[:upto, :2])
            and _close(g[:upto], ref[:upto, 2]))


def _check_case(out, q, c, rnd, what):
    """-> (passed strictly, passed under the closing allowance, both trees bit-exact)."""
    found = c["found"]
    assert int(out["status"][q]) == (C.FOUND if found else C.NO_PATH), what
    assert int(out["forward"][q]) == c["forward"], what
    assert int(out["iters"][q]) == c["iters"], what
    assert int(out["draws"][q]) == c["draws"] and rnd[int(out["draws"][q])] == c["next"], what
    fw = c["forward"]
    bw = 1 - fw
    assert _tree_matches(out, q, c, fw), (what, "forward tree")
    assert int(out["boundary"][q, fw]) == c["boundary"][fw], what
    plen = int(out["path_len"][q])
    cost = float(out["cost"][q])
    assert abs(cost - c["cost"]) <= RTOL * c["cost"], (what, cost, c["cost"])
    nb, nb_ref = int(out["n_nodes"][q, bw]), len(c[f"tree{bw}"])
    strict = (_tree_matches(out, q, c, bw) and int(out["boundary"][q, bw]) == c["boundary"][bw]
              and plen == len(c["path"]) and _close(out["path"][q, :plen], c["path"]))
    exact = strict and all(np.array_equal(_tree(out, q, t)[0], c[f"tree{t}"][:, :2])
                           and np.array_equal(_tree(out, q, t)[1], c[f"tree{t}"][:, 2]) for t in (0, 1))
    if strict:
        return True, False, exact
    # the closing allowance: one node more or less at the very end of the backward tree, and nothing else
    d = nb - nb_ref
    assert found and abs(d) == 1, (what, "backward tree", nb, nb_ref)
    assert plen - len(c["path"]) == d and int(out["boundary"][q, bw]) - c["boundary"][bw] == d, what
    assert int(out["boundary"][q, bw]) == nb - 1 and c["boundary"][bw] == nb_ref - 1, what
    assert _tree_matches(out, q, c, bw, upto=min(nb, nb_ref) - 1), (what, "backward tree before the closing approach")
    return False, True, False


def test_fixture_cases_against_reference(readme_out):
    """Every fixture case, batched per map and setting; the closing allowance counted over all of them."""
    groups = {}
    for i, c in enumerate(CASES):
        groups.setdefault((c["map"], c["sample_num"], c["max_dist"], c["rate"], tuple(c["goal"])), []).append(i)
    assert len(groups) == 7
    allowed, exact = [], 0
    shared = {i: q for q, i in enumerate(README + [SHORT])}  # the queries of readme_out's launch
    for key, idx in groups.items():
        out = readme_out if idx[0] in shared else _launch(idx)
        for q, i in enumerate(idx):
            q = shared.get(i, q)
            c = CASES[i]
            what = (c["kind"], c["seed"])
            s, a, e = _check_case(out, q, c, C.stream(c), what)
            exact += e
            if a:
                allowed.append(what)
    print(f"closing allowance used by {len(allowed)} of {len(CASES)} cases {allowed}; "
          f"{exact}/{len(CASES)} cases with both trees bit-exact")
    assert len(allowed) <= ALLOWANCE_CAP, allowed


def test_c3_long_leaves_the_lds_share():
    """The default max_dist 0.5 on C3: both trees outgrow the nodes the kernel keeps in LDS."""
    from python_motion_planning_amd import batch

    lds = batch.rrt_connect_lds_nodes()
    c = CASES[C3LONG]
    assert min(len(c["tree0"]), len(c["tree1"])) > lds >= 64
    out = _launch([C3LONG])
    assert min(out["n_nodes"][0]) > lds and int(out["status"][0]) == C.FOUND
    assert int(out["path_len"][0]) in (len(c["path"]) - 1, len(c["path"]), len(c["path"]) + 1)


def _same_query(a, qa, b, qb):
    """Two launches computed the same plan for a query: every output equal, bit for bit."""
    for k in ("n_nodes", "forward", "boundary", "cost", "path_len", "iters", "draws", "status"):
        assert np.array_equal(a[k][qa], b[k][qb]), k
    for t in (0, 1):
        for x, y in zip(_tree(a, qa, t), _tree(b, qb, t)):
            assert np.array_equal(x, y), t
    n = int(a["path_len"][qa])
    assert np.array_equal(a["path"][qa, :n], b["path"][qb, :n])


@pytest.mark.parametrize("nq", [1, 5, 67])
def test_batch_shapes(readme_out, nq):
    """One query; five (not a multiple of the four per workgroup) with different queries in one launch;
    67.  Each query's plan is the one the 17-query launch computed, whatever its place in the batch."""
    pool = [README[0], README[1], SHORT, README[9], README[2]] + README[3:]  # (seed 9 ends with tree 0 forward)
    idx = [pool[k % len(pool)] for k in range(nq)]
    out = _launch(idx)
    where = {i: q for q, i in enumerate(README + [SHORT])}
    for q, i in enumerate(idx):
        _same_query(out, q, readme_out, where[i])
    assert len({tuple(CASES[i]["goal"]) for i in idx}) == (1 if nq == 1 else 2)


def test_dropin_readme(readme_out):
    """np.random.seed(0); RRTConnect((18, 8), (37, 18), README map).plan(): the reference's cost, path,
    len(expand) and interleave order, the global generator left where the reference leaves it."""
    import python_motion_planning_amd as pmp

    c = CASES[README[0]]
    assert (c["seed"], c["forward"], c["n_expand"]) == (0, 1, 127)
    planner = pmp.RRTConnect((18, 8), (37, 18), C.env_of("readme"))
    np.random.seed(0)
    cost, path, expand = planner.plan()
    assert np.random.random() == c["next"]
    assert abs(cost - c["cost"]) <= RTOL * cost
    allow = abs(len(path) - len(c["path"])) == 1  # (the closing allowance, counted by the fixture test)
    assert len(path) == len(c["path"]) or allow
    assert path[0] == (18, 8) and path[-1] == (37, 18)
    assert all(isinstance(v, int) for v in path[0] + path[-1])
    if not allow:
        np.testing.assert_allclose(np.array(path, np.float64), c["path"], rtol=RTOL)
        assert len(expand) == c["n_expand"]
    # getExpand: sample_list_f (here the goal-rooted tree) first, then sample_list_b, index by index
    f, b = c["tree1"], c["tree0"]
    fp, bp = c["parent1"], c["parent0"]
    assert expand[0] is planner.goal and expand[1] is planner.start
    for k in range(1, min(len(f), len(b)) - 1):
        for node, tree, par in ((expand[2 * k], f, fp), (expand[2 * k + 1], b, bp)):
            np.testing.assert_allclose([node.x, node.y, node.g], tree[k], rtol=RTOL)
            np.testing.assert_allclose(node.parent, tree[par[k], :2], rtol=RTOL)
    # plan() and the batch launch agree
    q = 0
    assert len(expand) == int(readme_out["n_nodes"][q].sum()) and len(path) == int(readme_out["path_len"][q])


def test_never_found_returns_0_none_none():
    import python_motion_planning_amd as pmp

    c = next(c for c in CASES if c["kind"] == "never")
    planner = pmp.RRTConnect((18, 8), (27, 13), C.env_of("readme"), sample_num=400)
    np.random.seed(c["seed"])
    assert planner.plan() == (0, None, None)
    assert np.random.random() == c["next"]


def test_cap_overflow_and_rerun(monkeypatch):
    """A tree capacity below the plan's needs gives status 3 with the trees filled up to it; plan()
    doubles the capacity and re-runs on the same draws."""
    import python_motion_planning_amd as pmp
    from python_motion_planning_amd import batch

    c = CASES[README[0]]
    assert max(len(c["tree0"]), len(c["tree1"])) == 67
    out = _launch([README[0]], cap=32)
    ref = C.plan(c["map"], c["start"], c["goal"], C.stream(c).tolist(), c["sample_num"], cap=32)
    assert int(out["status"][0]) == C.CAP_OVERFLOW == ref["status"]
    assert list(out["n_nodes"][0]) == [len(ref["tree"][0][0]), len(ref["tree"][1][0])] and max(out["n_nodes"][0]) == 32
    assert int(out["iters"][0]) == ref["iters"] and int(out["draws"][0]) == ref["draws"]
    assert int(out["path_len"][0]) == 0 and list(out["boundary"][0]) == [-1, -1]

    caps = []
    real = batch.rrt_connect_batch

    def spy(*a, **kw):
        caps.append(kw["cap"])
        return real(*a, **kw)

    monkeypatch.setattr(batch, "rrt_connect_batch", spy)
    monkeypatch.setattr(batch, "RRT_CONNECT_DEFAULT_CAP", 32)
    planner = pmp.RRTConnect((18, 8), (37, 18), C.env_of("readme"))
    np.random.seed(0)
    cost, path, expand = planner.plan()
    assert caps == [32, 64, 128]
    assert np.random.random() == c["next"]
    assert abs(cost - c["cost"]) <= RTOL * cost and abs(len(path) - len(c["path"])) <= 1


def test_path_cap_overflow(readme_out):
    """A path_cap below the path's length gives status 2; cost, length and trees are complete, and the
    part of the path that fits is written."""
    c = CASES[README[0]]
    out = _launch([README[0]], path_cap=10)
    assert int(out["status"][0]) == C.PATH_OVERFLOW
    assert int(out["path_len"][0]) == int(readme_out["path_len"][0]) > 10
    assert out["cost"][0] == readme_out["cost"][0]
    assert np.array_equal(out["n_nodes"][0], readme_out["n_nodes"][0])
    assert out["path"].shape[1] == 10 and np.array_equal(out["path"][0], readme_out["path"][0, :10])
    assert tuple(out["path"][0, 0]) == tuple(c["start"])
