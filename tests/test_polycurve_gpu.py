"""Polynomial and Bezier on gfx950 (pmp_polycurve_batch, pmp_polycurve_time_matrix, pmp_bezier_batch) against
the reference's own runs (tests/golden/polycurve.npz, make_golden_polycurve.py), under the rules of
polycurve_checks.py."""
import functools

import numpy as np
import pytest

import polycurve_checks as C

pytestmark = pytest.mark.gpu

Z = C.load()
CASES = list(C.cases(Z))
BCASES = list(C.bezier_cases(Z))
BY = {c[1]: c[0] for c in CASES}
BBY = {c[1]: c[0] for c in BCASES}
PRM = (0.1, 1.0, 0.5, 0.1, 1.0, 30.0)
COMMON = [c for c in CASES if c[4] == PRM]  # 300 random + the examples and named ones at (0.1, 1.0, 0.5)
KEYS = ("t_index", "T", "n_points", "points", "status")
BKEYS = ("control", "n_points", "points", "status")
BP = (0.1, 3.0)


def _host(r, keys=KEYS):
    return {k: None if r[k] is None else r[k].cpu().numpy() for k in keys}


@functools.lru_cache(maxsize=None)
def _single(i):
    """Polynomial case i in a launch of its own (computed once, shared by the tests)"""
    from python_motion_planning_amd import batch

    _, _, s, g, prm = CASES[i]
    return _host(batch.polynomial_batch([s], [g], *prm))


@functools.lru_cache(maxsize=None)
def _bsingle(i):
    from python_motion_planning_amd import batch

    _, _, s, g, prm = BCASES[i]
    return _host(batch.bezier_batch([s], [g], *prm), BKEYS)


def _rows(r, q=0):
    return r["points"][q, : int(r["n_points"][q])]


def test_kernel_against_reference_runs():
    """Every polynomial case in its own launch: t_index, count and status exact (trajectories of 11 to 291
    rows, chosen candidates 0, beyond 64 and 128, the last one, none), values under polycurve_checks' rules."""
    worst = {}
    for i, name, *_ in CASES:
        r = _single(i)
        C.compare_polynomial(Z, i, r["t_index"][0], r["T"][0], r["n_points"][0], _rows(r), r["status"][0], worst)
    print("worst deviation per column:", {k: f"{v:.3g}" for k, v in worst.items()})
    ti = np.array([int(_single(c[0])["t_index"][0]) for c in COMMON])
    assert (ti > 128).any() and ((ti > 64) & (ti <= 128)).any() and (ti == -1).any()
    assert int(_single(BY["last_candidate"])["t_index"][0]) == 28 and int(_single(BY["one_candidate"])["t_index"][0]) == 0


def test_rows_equal_the_restatement_beyond_the_stored_ones():
    """The cases that store three rows: every row against the restatement (more than one round of 64)."""
    for name in ("ex1_0_1", "ex2_3_2", "rng_200"):
        i, _, s, g, prm = CASES[BY[name]]
        r, want = _single(i), C.restate_polynomial(s, g, *prm)
        assert int(r["n_points"][0]) == len(want["rows"]) > 64
        C.poly_rows_close(_rows(r), want["rows"], np.zeros((len(want["rows"]), 2), bool), name)


def test_batch_equals_single_runs():
    """All (0.1, 1.0, 0.5) cases in one launch (not a multiple of 64) give the single launches bit for bit."""
    from python_motion_planning_amd import batch

    assert len(COMMON) >= 300 and len(COMMON) % 64
    r = _host(batch.polynomial_batch([c[2] for c in COMMON], [c[3] for c in COMMON], *PRM))
    for j, c in enumerate(COMMON):
        s = _single(c[0])
        for k in ("t_index", "T", "n_points", "status"):
            assert np.array_equal(r[k][j], s[k][0]), (c[1], k)
        assert np.array_equal(_rows(r, j), _rows(s), equal_nan=True), c[1]


def test_cost_only_equals_sampling_launch():
    from python_motion_planning_amd import batch

    sel = COMMON[:130]
    a = batch.polynomial_batch([c[2] for c in sel], [c[3] for c in sel], *PRM, cost_only=True)
    b = batch.polynomial_batch([c[2] for c in sel], [c[3] for c in sel], *PRM)
    assert a["points"] is None and b["points"] is not None
    for k in ("t_index", "T", "n_points", "status"):
        assert np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), k


def test_time_matrix_against_fixture():
    from python_motion_planning_amd import batch

    m = batch.polynomial_time_matrix(Z["tm_start"], Z["tm_goal"], *Z["tm_params"])
    assert tuple(m["T"].shape) == (5, 7) and tuple(m["t_index"].shape) == (5, 7)
    assert np.array_equal(m["t_index"].cpu().numpy(), Z["tm_index"])
    print("time matrix worst deviation:", C.close(m["T"].cpu().numpy(), Z["tm_T"], "time matrix"))


def test_time_matrix_equals_batch():
    """65 x 3: every pair bit for bit what polynomial_batch gives for it"""
    from python_motion_planning_amd import batch

    s = np.array([c[2] for c in COMMON[20:85]])
    g = np.array([c[3] for c in COMMON[100:103]])
    m = batch.polynomial_time_matrix(s, g, *PRM)
    r = batch.polynomial_batch(np.repeat(s, 3, axis=0), np.tile(g, (65, 1)), *PRM, cost_only=True)
    assert np.array_equal(m["T"].cpu().numpy().ravel(), r["T"].cpu().numpy())
    assert np.array_equal(m["t_index"].cpu().numpy().ravel(), r["t_index"].cpu().numpy())
    assert (r["t_index"].cpu().numpy() >= 0).sum() > 100


def test_generation_returns_a_trajectory():
    from python_motion_planning_amd import Polynomial

    i, _, s, g, prm = CASES[BY["start_yaw_back"]]
    gen = Polynomial(*prm[:3])
    tr = gen.generation(s, g)
    assert isinstance(tr, Polynomial.Trajectory) and tr.size == 131
    for k in C.COLS:
        assert type(getattr(tr, k)) is list and all(type(v) is float for v in getattr(tr, k))
    rows = np.column_stack([getattr(tr, k) for k in C.COLS])
    C.compare_polynomial(Z, i, Z["t_index"][i], Z["T"][i], tr.size, rows, 0)
    assert tr.yaw[0] == 0.0 and np.copysign(1.0, tr.yaw[0]) == 1.0
    far = gen.generation(*CASES[BY["far_goal"]][2:4])
    assert isinstance(far, Polynomial.Trajectory) and far.size == 0 and far.x == []
    # dt, t_min and t_max are read at call time
    j, _, s, g, prm = CASES[BY["dt_coarse"]]
    gen = Polynomial(*prm[:3])
    gen.dt = prm[3]
    tr = gen.generation(s, g)
    C.compare_polynomial(Z, j, Z["t_index"][j], Z["T"][j], tr.size, np.column_stack([getattr(tr, k) for k in C.COLS]), 0)
    gen.t_max = 2.0
    assert gen.generation(s, g).size == 0


def test_run_concatenates_the_segments():
    from python_motion_planning_amd import Polynomial

    px, py, pyaw = Polynomial(*Z["run_params"]).run([tuple(p) for p in Z["run_points"]])
    assert type(px) is list and len(px) == len(py) == len(pyaw) == len(Z["run_path"])
    assert all(type(v) is float for v in px + py + pyaw)
    C.close(np.column_stack([px, py]), Z["run_path"][:, :2], "run path")
    # the segments' own launches (checked against the reference above, yaw through v), bit for bit
    rows = np.concatenate([_rows(_single(BY[f"ex1_{k}_0"])) for k in range(len(Z["run_points"]) - 1)])
    assert np.array_equal(np.column_stack([px, py, pyaw]), rows[:, 1:4])
    assert pyaw[0] == Z["run_path"][0, 2]  # at rest: the signed zeros of dx(0)


def test_status_overflow_and_retry():
    from python_motion_planning_amd import batch

    i, _, s, g, prm = CASES[BY["ex1_0_1"]]
    full = _single(i)
    n = int(full["n_points"][0])
    assert n > 10
    r = _host(batch.polynomial_batch([s], [g], *prm, point_cap=10, retry_overflow=False))
    assert int(r["status"][0]) == 2 and int(r["n_points"][0]) == n and r["points"].shape == (1, 10, 7)
    assert np.array_equal(r["points"][0], full["points"][0, :10])
    for k in ("t_index", "T"):
        assert np.array_equal(r[k], full[k])
    # with the retry, beside a pair that fits the first cap (no feasible T: no rows)
    j = BY["far_goal"]
    r = _host(batch.polynomial_batch([s, CASES[j][2]], [g, CASES[j][3]], *prm, point_cap=10))
    assert r["status"].tolist() == [0, 1] and r["n_points"].tolist() == [n, 0] and r["points"].shape == (2, n, 7)
    assert np.array_equal(_rows(r, 0), _rows(full))
    k = BY["same_pose"]
    r = _host(batch.polynomial_batch([CASES[k][2], s], [CASES[k][3], g], *prm, point_cap=11))
    assert r["status"].tolist() == [0, 0] and r["n_points"].tolist() == [11, n]
    assert np.array_equal(_rows(r, 0), _rows(_single(k))) and np.array_equal(_rows(r, 1), _rows(full))


def test_status_no_feasible_time_beside_a_good_pair():
    from python_motion_planning_amd import batch

    i, _, s, g, prm = CASES[BY["ex1_1_1"]]
    nan, inf = float("nan"), float("inf")
    z5 = (0.0, 0.0, 0.0, 0.0, 0.0)
    r = _host(batch.polynomial_batch([(0, nan, 0, 0, 0), s, z5, (0, 0, inf, 1, 0)], [(9, 9, 0, 1, 0), g, (1e6, 0, 0, 1, 0), (9, 9, 0, 1, 0)], *prm))
    assert r["status"].tolist() == [1, 0, 1, 1] and r["t_index"].tolist() == [-1, int(Z["t_index"][i]), -1, -1]
    assert r["n_points"].tolist()[::2] == [0, 0] and r["T"].tolist()[::2] == [inf, inf]
    full = _single(i)
    assert np.array_equal(_rows(r, 1), _rows(full)) and r["T"][1] == full["T"][0]
    m = batch.polynomial_time_matrix([(0, nan, 0, 0, 0), s], [g], *prm)
    assert m["t_index"].cpu().numpy().ravel().tolist() == [-1, int(Z["t_index"][i])]
    assert m["T"].cpu().numpy().ravel().tolist() == [inf, float(full["T"][0])]
    # no candidate at all
    r = _host(batch.polynomial_batch([s], [g], 0.1, 1.0, 0.5, t_min=3.0, t_max=3.0))
    assert r["status"].tolist() == [1] and r["t_index"].tolist() == [-1]


NAN, INF = float("nan"), float("inf")
GOOD = dict(step=0.1, max_acc=1.0, max_jerk=0.5, dt=0.1, t_min=1.0, t_max=30.0)


@pytest.mark.parametrize("bad", [dict(step=0.0), dict(step=-0.1), dict(step=NAN), dict(step=INF), dict(dt=0.0), dict(dt=-0.1),
                                 dict(dt=NAN), dict(t_min=0.0), dict(t_min=-1.0), dict(t_min=NAN), dict(t_max=INF),
                                 dict(max_acc=NAN), dict(max_acc=INF), dict(max_jerk=NAN), dict(max_jerk=-INF),
                                 dict(step=1e-7), dict(dt=1e-7)], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_refused_parameters(bad):
    """step <= 0 or non-finite, dt <= 0, t_min <= 0, non-finite limits, more than 2^24 candidates (step 1e-7) or
    sample times (dt 1e-7)"""
    from python_motion_planning_amd import batch
    from python_motion_planning_amd._lib import PMPError

    kw = dict(GOOD, **bad)
    with pytest.raises(PMPError, match="pmp_polycurve_batch"):
        batch.polynomial_batch([(0, 0, 0, 0, 0)], [(10, 0, 0, 1, 0)], **kw)
    with pytest.raises(PMPError, match="pmp_polycurve_time_matrix"):
        batch.polynomial_time_matrix([(0, 0, 0, 0, 0)], [(10, 0, 0, 1, 0)], **kw)


# ---- Bezier ------------------------------------------------------------------------------------------------
def test_bezier_against_reference_runs():
    """Every Bezier case in its own launch: count and status exact (0, 1, 2 and up to 484 points), control
    points and x, y within RTOL."""
    worst, other = {}, []
    for i, name, *_ in BCASES:
        r = _bsingle(i)
        if C.compare_bezier(Z, i, r["control"][0], r["n_points"][0], _rows(r), r["status"][0], worst):
            other.append(name)
    print("worst deviation per column:", {k: f"{v:.3g}" for k, v in worst.items()}, "other count:", other)
    assert [int(_bsingle(BBY[n])["n_points"][0]) for n in ("n0", "n1", "n2", "pythagorean")] == [0, 1, 2, 50]
    n1 = _bsingle(BBY["n1"])
    assert np.array_equal(_rows(n1)[0], Z["b_start"][BBY["n1"], :2])
    n2 = _rows(_bsingle(BBY["n2"]))
    assert np.array_equal(n2[0], Z["b_start"][BBY["n2"], :2]) and np.array_equal(n2[1], Z["b_goal"][BBY["n2"], :2])


def test_bezier_batch_equals_single_runs_and_cost_only():
    from python_motion_planning_amd import batch

    assert len(BCASES) % 64
    s, g = [c[2] for c in BCASES], [c[3] for c in BCASES]
    r = _host(batch.bezier_batch(s, g, *BP), BKEYS)
    for j, c in enumerate(BCASES):
        one = _bsingle(c[0])
        for k in ("control", "n_points", "status"):
            assert np.array_equal(r[k][j], one[k][0]), (c[1], k)
        assert np.array_equal(_rows(r, j), _rows(one)), c[1]
    a = batch.bezier_batch(s, g, *BP, cost_only=True)
    assert a["points"] is None
    for k in ("control", "n_points", "status"):
        assert np.array_equal(a[k].cpu().numpy(), r[k]), k


def test_bezier_generation_and_run():
    from python_motion_planning_amd import Bezier

    i, _, s, g, prm = BCASES[BBY["ex1_0"]]
    pts, ctrl = Bezier(*prm).generation(s, g)
    assert type(pts) is list and all(isinstance(p, np.ndarray) and p.shape == (2,) for p in pts)
    assert type(ctrl) is list and len(ctrl) == 4 and all(type(c) is tuple and len(c) == 2 for c in ctrl)
    C.compare_bezier(Z, i, np.array(ctrl), len(pts), np.array(pts).reshape(-1, 2), 0)
    pts, ctrl = Bezier(*prm).generation(*BCASES[BBY["n0"]][2:4])
    assert pts == [] and len(ctrl) == 4
    px, py = Bezier(*Z["b_run_params"]).run([tuple(p) for p in Z["b_run_points"]])
    assert type(px) is list and len(px) == len(py) == len(Z["b_run_path"])
    C.close(np.column_stack([px, py]), Z["b_run_path"], "bezier run path")
    with pytest.raises(ValueError):
        Bezier(*prm).generation((0, NAN, 0), (1, 1, 0))
    with pytest.raises(OverflowError):
        Bezier(*prm).generation((0, 0, 0), (INF, 1, 0))


def test_bezier_status_overflow_retry_and_reference_raises():
    from python_motion_planning_amd import batch

    i, _, s, g, prm = BCASES[BBY["ex1_0"]]
    full = _bsingle(i)
    n = int(full["n_points"][0])
    r = _host(batch.bezier_batch([s], [g], *prm, point_cap=10, retry_overflow=False), BKEYS)
    assert int(r["status"][0]) == 2 and int(r["n_points"][0]) == n > 10 and r["points"].shape == (1, 10, 2)
    assert np.array_equal(r["points"][0], full["points"][0, :10]) and np.array_equal(r["control"], full["control"])
    j = BBY["n2"]
    r = _host(batch.bezier_batch([s, BCASES[j][2]], [g, BCASES[j][3]], *prm, point_cap=10), BKEYS)
    assert r["status"].tolist() == [0, 0] and r["n_points"].tolist() == [n, 2] and r["points"].shape == (2, n, 2)
    assert np.array_equal(_rows(r, 0), _rows(full)) and np.array_equal(_rows(r, 1), _rows(_bsingle(j)))
    # status 4 beside a good pair, which is unchanged
    r = _host(batch.bezier_batch([(0, NAN, 0), s, (0, 0, 0)], [(1, 1, 0), g, (INF, 0, 0)], *prm), BKEYS)
    assert r["status"].tolist() == [4, 0, 4] and r["n_points"].tolist() == [0, n, 0]
    assert np.array_equal(_rows(r, 1), _rows(full)) and np.array_equal(r["control"][1], full["control"][0])


@pytest.mark.parametrize("step,offset", [(0.0, 3.0), (-0.1, 3.0), (NAN, 3.0), (INF, 3.0), (0.1, 0.0), (0.1, NAN), (0.1, INF)])
def test_bezier_refused_parameters(step, offset):
    from python_motion_planning_amd import batch
    from python_motion_planning_amd._lib import PMPError

    with pytest.raises(PMPError, match="pmp_bezier_batch"):
        batch.bezier_batch([(0, 0, 0)], [(10, 0, 0)], step, offset)
