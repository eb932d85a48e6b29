"""ACO on gfx950 (pmp_aco_batch, csrc/aco.hip on csrc/mt19937_dev.h) against the reference's own runs
(tests/golden/aco.npz, make_golden_aco.py), under the rule of aco_checks.py: every comparison is equality."""
import functools
import random

import numpy as np
import pytest

import aco_checks as C

pytestmark = pytest.mark.gpu

Z = C.load()
CASES = [C.case(Z, i) for i in range(len(Z["names"]))]
BY = {c["name"]: c for c in CASES}
SMALL = [c["name"] for c in CASES if c["name"] != "default"]
KEYS = ("status", "best_len", "best_path", "n_cost", "cost_list", "draws", "mt_state_out", "ant_found", "ant_len", "pheromone")


def _planner(c):
    from python_motion_planning_amd import ACO

    return ACO(c["start"], c["goal"], C.grid_of(c), **c["params"])


@functools.lru_cache(maxsize=None)
def _run(name, waves=None):
    """The case through the batch entry with the trace on; computed once per wave count, shared by the tests"""
    from python_motion_planning_amd import batch

    c = BY[name]
    p = c["params"]
    table = _planner(c).heuristic_table()
    out = batch.aco_batch(C.grid_of(c), [c["start"]], [c["goal"]], table[None], [0], [np.array(c["state_in"], np.uint32)],
                          p["n_ants"], p["max_iter"], p["alpha"], 1 - p["rho"], p["Q"], trace=True, waves=waves)
    return {k: out[k].cpu().numpy()[0] for k in KEYS}


def _same(a, b):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("n", [0, 1, 311, 312, 313, 2000])
@pytest.mark.parametrize("index", [0, 1, 623, 624])
def test_generator_against_random(n, index):
    from python_motion_planning_amd import batch
    from python_motion_planning_amd.evolutionary_search import random_stream

    random.seed(1234 + index)
    state = (3, random.getstate()[1][:624] + (index,), None)
    want, after = random_stream(n, state)
    got, words = batch.mt19937_doubles(state, n)
    assert np.array_equal(C.bits(got.cpu().numpy()), C.bits(want))
    assert tuple(int(w) for w in words) == after[1]
    random.setstate(state)
    assert [random.random() for _ in range(min(n, 5))] == list(want[:5])
    for _ in range(max(n - 5, 0)):
        random.random()
    assert random.getstate()[1] == tuple(int(w) for w in words)


@pytest.mark.parametrize("name", SMALL)
def test_small_case_against_fixture(name):
    c, r = BY[name], _run(name)
    want_status = 5 if c["raised"] else (0 if c["found_any"] else 1)
    print(name, "status", int(r["status"]), "draws", int(r["draws"]), "of", c["draws"], "n_cost", int(r["n_cost"]))
    assert int(r["status"]) == want_status
    assert int(r["draws"]) == c["draws"]
    assert tuple(int(w) for w in r["mt_state_out"].view(np.uint32)) == c["state_out"]
    assert np.array_equal(r["ant_found"], c["ant_found"]) and np.array_equal(r["ant_len"], c["ant_len"])
    n = int(r["best_len"])
    assert n == len(c["path"]) and np.array_equal(r["best_path"][:n], c["path"])
    assert int(r["n_cost"]) == len(c["cost_list"]) and np.array_equal(r["cost_list"][: len(c["cost_list"])], c["cost_list"])
    assert C.pheromone_sha256(r["pheromone"]) == c["pher_sha256"]
    if c["pher"] is not None:
        assert np.array_equal(C.bits(r["pheromone"]), C.bits(c["pher"]))


@pytest.mark.parametrize("name", [n for n in SMALL if BY[n]["found_any"]])
def test_plan_of_the_class(name):
    c = BY[name]
    C.set_state(c)
    planner = _planner(c)
    cost, path, cost_list = planner.plan()
    assert random.getstate() == (3, c["state_out"], None) and planner.draws == c["draws"]
    assert isinstance(cost, float) and C.bits(cost) == C.bits(c["cost"])
    assert isinstance(path, list) and all(isinstance(p, tuple) and isinstance(p[0], int) and isinstance(p[1], int) for p in path)
    assert path[0] == c["start"] and [x * c["H"] + y for x, y in path] == list(c["path"])
    assert isinstance(cost_list, list) and all(type(v) is int for v in cost_list) and cost_list == list(c["cost_list"])


@pytest.mark.parametrize("name", ["start_is_goal", "enclosed", "iter0"])
def test_empty_results(name):
    c = BY[name]
    C.set_state(c)
    assert _planner(c).plan() == ([], [], [])
    assert random.getstate()[1] == c["state_out"]


def test_gauss_next_is_kept():
    c = BY["one_ant"]
    C.set_state(c)
    random.setstate((3, c["state_in"], 0.25))
    _planner(c).run()
    assert random.getstate() == (3, c["state_out"], 0.25)


def test_index_error():
    c, r = BY["index_error"], _run("index_error")
    assert int(r["status"]) == 5 and int(r["draws"]) == 1 and int(r["best_len"]) == 0
    C.set_state(c)
    with pytest.raises(IndexError, match="list index out of range"):
        _planner(c).plan()
    assert random.getstate()[1][624] == 12 and random.getstate()[1] == c["state_out"]


@pytest.mark.parametrize("name", SMALL)
def test_wave_counts_give_identical_outputs(name):
    from python_motion_planning_amd import batch

    chosen, most = batch.aco_default_waves(), batch.aco_max_waves()
    assert 1 <= chosen <= most
    base = _run(name)
    for waves in (1, chosen, most):
        _same(_run(name, waves), base)


def test_ragged_batch_equals_single_launches():
    from python_motion_planning_amd import ACO

    c = BY["walls"]
    env = C.grid_of(c)
    starts = [(3, 7), (17, 7), (3, 2), (8, 7), (17, 12), (3, 7), (12, 3)]
    goals = [(17, 7), (3, 7), (17, 12), (17, 7), (3, 2), (17, 7), (4, 12)]
    seeds = [31, 32, 33, 34, 35, 36, 37]
    kw = dict(n_ants=6, max_iter=5, trace=True)
    got = ACO.plan_batch(env, starts, goals, seeds, **kw)
    both = {k: got[k].cpu().numpy() for k in KEYS}
    assert list(got["heur_of"]) == [0, 1, 2, 0, 3, 0, 4]  # plans with one goal share a table
    assert len({both["draws"][i].tobytes() for i in range(7)}) > 1
    for i in range(7):
        one = ACO.plan_batch(env, starts[i : i + 1], goals[i : i + 1], seeds[i : i + 1], **kw)
        _same({k: one[k].cpu().numpy()[0] for k in KEYS}, {k: v[i] for k, v in both.items()})
        assert one["random_states"][0] == got["random_states"][i]
    # plan 0 is the class's own plan from the same seed
    random.seed(seeds[0])
    cost, path, cost_list = ACO(starts[0], goals[0], env, n_ants=6, max_iter=5).plan()
    assert random.getstate() == got["random_states"][0]
    if int(both["status"][0]) == 0:
        n = int(both["best_len"][0])
        assert [x * env.y_range + y for x, y in path] == both["best_path"][0, :n].tolist()
        assert cost_list == both["cost_list"][0, : int(both["n_cost"][0])].tolist()
    else:
        assert (cost, path, cost_list) == ([], [], [])
    # a state tuple in place of a seed
    again = ACO.plan_batch(env, starts[:1], goals[:1], [random.Random(seeds[0]).getstate()], **kw)
    _same({k: again[k].cpu().numpy()[0] for k in KEYS}, {k: v[0] for k, v in both.items()})


def test_largest_grid_at_the_most_waves():
    """65,536 cells: the largest visited bitmap, at the most waves per workgroup (the largest LDS request), against
    one wave per workgroup"""
    from python_motion_planning_amd import ACO, batch

    grid = occ_grid(C.boundary(256, 256))
    starts, goals = [(100, 100)] * 9, [(101, 100)] * 8 + [(120, 110)]
    kw = dict(n_ants=2, max_iter=2)
    most = ACO.plan_batch(grid, starts, goals, list(range(9)), waves=batch.aco_max_waves(), **kw)
    one = ACO.plan_batch(grid, starts, goals, list(range(9)), waves=1, **kw)
    for k in KEYS[:7]:
        assert most[k].cpu().numpy().tobytes() == one[k].cpu().numpy().tobytes(), k
    assert most["status"].tolist()[:8] == [0] * 8 and most["best_len"].tolist()[:8] == [2] * 8
    assert most["draws"].tolist()[:8] == [0] * 8 and int(most["draws"][8]) > 0
    assert most["random_states"][8] != (3, random.Random(8).getstate()[1], None)
    assert most["best_path"][0, :2].tolist() == [100 * 256 + 100, 101 * 256 + 100]


def occ_grid(occ):
    from python_motion_planning_amd import Grid

    return Grid.from_occupancy(occ)


def test_refusals():
    from python_motion_planning_amd import batch
    from python_motion_planning_amd._lib import PMPError

    c = BY["empty"]
    table = _planner(c).heuristic_table()
    state = np.array(c["state_in"], np.uint32)

    def call(occ=None, start=(5, 5), goal=(15, 9), heur=None, heur_of=0, index=None, **over):
        p = dict(n_ants=2, max_iter=1, alpha=1.0, one_minus_rho=0.9, Q=1.0)
        p.update(over)
        st = state.copy()
        if index is not None:
            st[624] = index
        return batch.aco_batch(c["occ"] if occ is None else occ, [start], [goal], (table if heur is None else heur)[None],
                               [heur_of], [st], **p)

    assert int(call()["status"][0]) in (0, 1)
    open_border = c["occ"].copy()
    open_border[0, 7] = 0
    bad_heur = table.copy()
    bad_heur[6 * 15 + 6] = np.inf
    nan_heur = table.copy()
    nan_heur[7 * 15 + 7] = np.nan
    for over in (dict(alpha=0.5), dict(alpha=2.0), dict(n_ants=0), dict(max_iter=-1), dict(one_minus_rho=float("nan")),
                 dict(one_minus_rho=float("inf")), dict(Q=float("inf")), dict(Q=float("nan")), dict(heur=bad_heur),
                 dict(heur=nan_heur), dict(start=(21, 5)), dict(start=(-1, 5)), dict(goal=(5, 15)), dict(start=(0, 5)),
                 dict(goal=(20, 14)), dict(occ=C.boundary(257, 256), heur=np.zeros(257 * 256)), dict(waves=-1),
                 dict(waves=batch.aco_max_waves() + 1), dict(index=625), dict(occ=open_border), dict(heur_of=1)):
        with pytest.raises(PMPError, match="pmp_aco_batch"):
            call(**over)
    # a non-finite entry under an obstacle is never read: taken
    under = table.copy()
    under[0] = np.inf
    assert int(call(heur=under)["status"][0]) in (0, 1)
