"""PSO on gfx950 (pmp_pso_batch, csrc/pso.hip) against the reference's own runs (tests/golden/pso.npz,
make_golden_pso.py), under the rules of pso_checks.py: the swarm's state exact, what carries the B-spline's
rounding within bs_rtol (2.12e-12) relative to max(1, |value|).

Worst deviations measured on an MI355X over the fixture: see DESIGN.md 3.12."""
import functools
import random

import numpy as np
import pytest

import pso_checks as C

pytestmark = pytest.mark.gpu

Z = C.load()
CASES = [C.case(Z, i) for i in range(len(Z["names"]))]
BY = {c["name"]: c for c in CASES}
SMALL = [c["name"] for c in CASES if c["name"] != "default"]
EXACT = ("status", "best_position", "positions", "trace_positions", "repeats")
ROUNDED = ("best_fitness", "fitness_history", "fitness", "particle_best_fitness", "points", "length", "trace_fitness")


def _planner(c):
    from python_motion_planning_amd import PSO

    return PSO(c["start"], c["goal"], C.grid_of(c), **c["params"])


@functools.lru_cache(maxsize=None)
def _run(name, waves=None):
    """The case as the class runs it (seed, initial positions on the host, the stream), through the batch entry
    with the trace on; computed once per wave count, shared by the tests"""
    from python_motion_planning_amd import batch
    from python_motion_planning_amd.evolutionary_search import random_stream

    c = BY[name]
    p = c["params"]
    random.seed(c["seed"])
    init = np.array(_planner(c).initializePositions(), np.int32).reshape(p["n_particles"], p["point_num"], 2)
    rnd, after = random_stream(batch.pso_draws(p["n_particles"], p["point_num"], p["max_iter"]))
    out = batch.pso_batch(C.grid_of(c), [c["start"]], [c["goal"]], init[None], rnd[None], p["n_particles"], p["point_num"],
                          p["max_iter"], p["w_inertial"], p["w_cognitive"], p["w_social"], p["max_speed"],
                          trace=c["traced"], waves=waves)
    host = {k: v.cpu().numpy()[0] for k, v in out.items() if v is not None}
    host.update(init=init, after=after)
    return host


def _same(a, b, keys=EXACT + ROUNDED + ("velocities",)):
    for k in keys:
        if k in a or k in b:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("name", SMALL)
def test_small_case_against_fixture(name):
    c, r = BY[name], _run(name)
    assert np.array_equal(r["init"], c["init"])
    assert np.array_equal(r["trace_positions"], c["trace_pos"])
    assert np.array_equal(r["positions"], c["pos"])
    assert np.array_equal(C.bits(r["velocities"]), C.bits(c["vel"]))
    assert np.array_equal(r["best_position"], c["gbest_pos"])
    assert int(r["status"]) == (4 if c["expect_inf"] else 0)
    assert r["after"][1] == c["state"]
    dev = dict(trace_fitness=C.deviation(r["trace_fitness"], c["trace_fit"]), fitness=C.deviation(r["fitness"], c["fit"]),
               particle_best=C.deviation(r["particle_best_fitness"], c["best_fit"]),
               history=C.deviation(r["fitness_history"], c["history"]),
               best_fitness=C.deviation(r["best_fitness"], c["gbest_fit"]))
    if c["expect_inf"]:
        assert np.isnan(r["points"]).all() and np.isnan(r["length"])
    else:
        dev.update(rows=C.deviation(r["points"], c["rows"]), cost=C.deviation(r["length"], c["cost"]))
    print(name, "deviations", dev, "repeats", int(r["repeats"]), "improve", c["improve"])
    assert max(dev.values()) <= C.RTOL, dev


@pytest.mark.parametrize("name", ["walls_random", "empty_circle", "tall_random", "reverse_circle", "iter0"])
def test_plan_of_the_class(name):
    c, r = BY[name], _run(name)
    random.seed(c["seed"])
    planner = _planner(c)
    cost, path, history = planner.plan()
    assert random.getstate()[1] == c["state"] and random.getstate()[2] is None
    assert isinstance(cost, float) and cost == float(r["length"])
    assert isinstance(path[0], tuple) and isinstance(path[0][0], float)
    assert np.array_equal(C.bits(np.array(path)), C.bits(r["points"]))
    assert np.array_equal(C.bits(np.array(history, np.float64)), C.bits(r["fitness_history"]))
    assert len(planner.particles) == c["params"]["n_particles"]
    for i, p in enumerate(planner.particles):
        assert p.best_pos is p.position and isinstance(p.position[0], tuple) and isinstance(p.position[0][0], int)
        assert np.array_equal(np.array(p.position), c["pos"][i])
        assert np.array_equal(C.bits(np.array(p.velocity)), C.bits(c["vel"][i]))
        assert p.fitness == r["fitness"][i] and p.best_fitness == r["particle_best_fitness"][i]
    assert planner.best_particle.position == [tuple(int(v) for v in pt) for pt in c["gbest_pos"]]
    assert planner.best_particle.fitness == float(r["best_fitness"]) and planner.repeats == int(r["repeats"])
    with pytest.raises(RuntimeError):
        planner.plan()


def test_verbose_prints_the_reference_lines(capsys):
    c = BY["p8"]
    random.seed(c["seed"])
    _, _, history = _planner(c).run()
    lines = capsys.readouterr().out.splitlines()
    assert lines == [f"iteration {i}: best fitness = {f}" for i, f in enumerate(history)] and len(lines) == 12


@pytest.mark.parametrize("name", ["close_inf", "p1"])
def test_inf_case_raises_and_reports_status_4(name):
    c, r = BY[name], _run(name)
    assert int(r["status"]) == 4 and np.isinf(r["best_fitness"]) and np.isinf(r["fitness_history"]).all()
    random.seed(c["seed"])
    planner = _planner(c)
    with pytest.raises(np.linalg.LinAlgError):
        planner.plan()
    assert random.getstate()[1] == c["state"]  # the reference raises at plan()'s last line, after every draw
    assert planner.best_particle.fitness == float("inf") and len(planner.particles) == c["params"]["n_particles"]


@pytest.mark.parametrize("name", SMALL)
def test_wave_counts_give_identical_outputs(name):
    from python_motion_planning_amd import batch

    chosen = batch.pso_default_waves()
    assert 1 <= chosen <= 16
    base = _run(name)
    for waves in (1, 4, chosen, 16):
        _same(_run(name, waves), base)


def test_ragged_launch_equals_single_launches():
    from python_motion_planning_amd import PSO

    c = BY["walls_circle"]
    env = C.grid_of(c)
    starts = [(5, 5), (45, 25), (5, 25), (25, 3), (12, 20), (5, 5), (44, 4)]
    goals = [(45, 25), (5, 5), (45, 5), (25, 28), (13, 21), (45, 25), (3, 27)]
    seeds = [21, 22, 23, 24, 25, 26, 27]
    kw = dict(n_particles=24, max_iter=12, init_mode=C.GEN_MODE_CIRCLE, trace=True)
    both = {k: v.cpu().numpy() for k, v in PSO.plan_batch(env, starts, goals, seeds, **kw).items() if hasattr(v, "cpu")}
    assert len({both["best_position"][i].tobytes() for i in range(len(seeds))}) > 1
    for i in range(len(seeds)):
        one = PSO.plan_batch(env, starts[i : i + 1], goals[i : i + 1], seeds[i : i + 1], **kw)
        _same({k: v.cpu().numpy()[0] for k, v in one.items() if hasattr(v, "cpu")}, {k: v[i] for k, v in both.items()})
    # plan 0 is the class's own plan from the same seed
    random.seed(seeds[0])
    cost, path, history = PSO(starts[0], goals[0], env, n_particles=24, max_iter=12, init_mode=C.GEN_MODE_CIRCLE).plan()
    assert cost == both["length"][0] and np.array_equal(np.array(history), both["fitness_history"][0])


@pytest.mark.parametrize("name", ["walls_random", "empty_random", "p3", "p8", "tall_random"])
def test_best_curve_is_the_bspline_kernels(name):
    """The shared header: the best particle's curve has the bits of bspline_batch on the same points"""
    from python_motion_planning_amd import batch

    c, r = BY[name], _run(name)
    pts = [c["start"]] + [tuple(int(v) for v in p) for p in r["best_position"]] + [c["goal"]]
    pts = sorted(set(pts), key=pts.index)
    b = batch.bspline_batch([np.array(pts, np.float64)], 0.01, 4, cost_only=True)
    length = b["length"].cpu().numpy()[0]
    assert int(b["status"][0]) == 0
    assert C.bits(length) == C.bits(r["length"])
    full = batch.bspline_batch([np.array(pts, np.float64)], 0.01, 4)["points"].cpu().numpy()[0]
    assert np.array_equal(C.bits(full), C.bits(r["points"]))
    f = float(r["best_fitness"])
    obs = round((100000.0 / f - float(length)) / 50000.0)
    assert obs >= 0 and f == 100000.0 / (float(length) + 50000 * obs)


def test_cal_fitness_value_is_one_particle():
    c = BY["iter0"]
    planner = _planner(c)
    for i in (0, 7, 23):
        f = planner.calFitnessValue([tuple(int(v) for v in p) for p in c["init"][i]])
        assert isinstance(f, float) and C.deviation(f, c["fit"][i]) <= C.RTOL
    assert planner.calFitnessValue([(5, 5)] * 5) == float("inf")  # two points left: the curve raises


@pytest.mark.parametrize("name", SMALL)
def test_repeat_counter(name):
    """The invariant: a replacement of the global best by particle i repeats the n - 1 - i particles after it,
    so the counter is the fixture's `later`.  That it is at least the number of replacements is no invariant (a
    replacement by an iteration's last particle repeats nothing); it holds on every stored case."""
    c, r = BY[name], _run(name)
    assert int(r["repeats"]) == c["later"]
    assert c["improve"] <= c["later"] <= c["improve"] * (c["params"]["n_particles"] - 1)
    assert int(r["repeats"]) >= c["improve"]


def test_refusals():
    from python_motion_planning_amd import batch
    from python_motion_planning_amd._lib import PMPError

    occ = BY["walls_random"]["occ"]
    base = dict(n_particles=4, point_num=5, max_iter=3, w_inertial=1.0, w_cognitive=1.0, w_social=1.0, max_speed=6)

    def call(stream=None, init=None, waves=None, **over):
        p = dict(base, **over)
        n, pn, it = max(p["n_particles"], 0), max(p["point_num"], 0), max(p["max_iter"], 0)
        init = np.full((1, n, pn, 2), 7, np.int32) if init is None else init
        rnd = np.zeros((1, 2 * n * pn * it if stream is None else stream))
        return batch.pso_batch(occ, [(5, 5)], [(45, 25)], init, rnd, waves=waves, **p)

    assert int(call()["status"][0]) == 4  # every point the same: a swarm the entry takes, whose curves all raise
    outside = np.full((1, 4, 5, 2), 7, np.int32)
    for over in (dict(n_particles=0), dict(point_num=0), dict(point_num=63), dict(max_iter=-1),
                 dict(w_inertial=float("nan")), dict(w_cognitive=float("inf")), dict(w_social=float("-inf")),
                 dict(max_speed=-1), dict(stream=2 * 4 * 5 * 3 - 1), dict(waves=17), dict(n_particles=3000),
                 dict(waves=16, point_num=62),  # 16 curve states of 64 waypoints outgrow the LDS; the default shrinks
                 dict(init=np.where(np.arange(40).reshape(1, 4, 5, 2) == 13, 31, outside)),
                 dict(init=np.where(np.arange(40).reshape(1, 4, 5, 2) == 12, 51, outside)),
                 dict(init=np.where(np.arange(40).reshape(1, 4, 5, 2) == 0, -1, outside))):
        with pytest.raises(PMPError, match="pmp_pso_batch"):
            call(**over)
    assert int(call(point_num=62, n_particles=2, max_iter=1)["status"][0]) == 4


def test_default_size_case():
    c, r = BY["default"], _run("default")
    assert np.array_equal(r["best_position"], c["gbest_pos"]) and int(r["status"]) == 0
    dev = dict(history=C.deviation(r["fitness_history"], c["history"]), rows=C.deviation(r["points"], c["rows"]),
               cost=C.deviation(r["length"], c["cost"]), fitness=C.deviation(r["fitness"], c["fit"]))
    print("default deviations", dev, "repeats", int(r["repeats"]), "improve", c["improve"])
    assert C.deviation(r["fitness_history"], c["history"]) <= C.RTOL
    assert np.array_equal(r["positions"], c["pos"]) and np.array_equal(C.bits(r["velocities"]), C.bits(c["vel"]))
    assert r["after"][1] == c["state"] and max(dev.values()) <= C.RTOL
    assert int(r["repeats"]) == c["later"] >= c["improve"]
