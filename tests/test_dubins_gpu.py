"""Dubins on gfx950 (pmp_dubins_batch, pmp_dubins_cost_matrix) against the reference's own runs
(tests/golden/dubins.npz, make_golden_dubins.py), under the rules of dubins_checks.py."""
import functools

import numpy as np
import pytest

import dubins_checks as C

pytestmark = pytest.mark.gpu

Z = C.load()
CASES = list(C.cases(Z))
BY = {c[1]: c[0] for c in CASES}
STEP, CURV = 0.1, 0.25
COMMON = [c for c in CASES if (c[4], c[5]) == (STEP, CURV)]  # 300 random + the named ones at (0.1, 0.25)
KEYS = ("word", "tpq", "cost", "n_points", "points", "status")


def _host(r):
    return {k: None if r[k] is None else r[k].cpu().numpy() for k in KEYS}


@functools.lru_cache(maxsize=None)
def _single(i):
    """Fixture case i in a launch of its own (computed once, shared by the tests)"""
    from python_motion_planning_amd import batch

    _, _, s, g, step, curv = CASES[i]
    return _host(batch.dubins_batch([s], [g], step, curv))


def _rows(r, q=0):
    return r["points"][q, : int(r["n_points"][q])]


def test_kernel_against_reference_runs():
    """Every fixture case in its own launch: word, count and status exact (0 points for equal poses, 28 on the
    axis), t / p / q / cost / x / y within 1e-9 max(1, |ref|), yaw by its wrapped difference; fragile
    cases by their own rule."""
    worst, fragile = {}, []
    for i, name, *_ in CASES:
        r = _single(i)
        if C.compare_case(Z, i, r["word"][0], r["tpq"][0], r["cost"][0], r["n_points"][0], _rows(r), r["status"][0], worst):
            fragile.append((name, C.WORDS[r["word"][0]]))
    print("worst deviation per column:", {k: f"{v:.3g}" for k, v in worst.items()}, "fragile:", fragile)


def test_more_than_64_points_per_piece():
    """step 0.05, max_curv 1: 323 points in six rounds of a wave, the straight piece alone 251 steps"""
    i = BY["diag_fine"]
    r = _single(i)
    assert int(r["n_points"][0]) == 323 and float(r["tpq"][0, 1]) / 0.05 > 3 * 64
    C.rows_close(_rows(r), C.restate(*CASES[i][2:])["points"], "diag_fine against the restatement")


def test_batch_equals_single_runs():
    """All (0.1, 0.25) cases in one launch (not a multiple of 64) give the single launches bit for bit."""
    from python_motion_planning_amd import batch

    assert len(COMMON) >= 300 and len(COMMON) % 64
    r = _host(batch.dubins_batch([c[2] for c in COMMON], [c[3] for c in COMMON], STEP, CURV))
    for j, c in enumerate(COMMON):
        s = _single(c[0])
        for k in ("word", "tpq", "cost", "n_points", "status"):
            assert np.array_equal(r[k][j], s[k][0]), (c[1], k)
        assert np.array_equal(_rows(r, j), _rows(s)), c[1]


def test_cost_only_equals_sampling_launch():
    from python_motion_planning_amd import batch

    sel = COMMON[:130]
    a = batch.dubins_batch([c[2] for c in sel], [c[3] for c in sel], STEP, CURV, cost_only=True)
    b = batch.dubins_batch([c[2] for c in sel], [c[3] for c in sel], STEP, CURV)
    assert a["points"] is None and b["points"] is not None
    for k in ("word", "tpq", "cost", "n_points", "status"):
        assert np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), k


def test_cost_matrix_against_fixture():
    from python_motion_planning_amd import batch

    m = batch.dubins_cost_matrix(Z["cm_start"], Z["cm_goal"], *Z["cm_params"])
    assert tuple(m["cost"].shape) == (5, 7) and tuple(m["word"].shape) == (5, 7)
    assert np.array_equal(m["word"].cpu().numpy(), Z["cm_word"])
    print("cost matrix worst deviation:", C.close(m["cost"].cpu().numpy(), Z["cm_cost"], "cost matrix"))


def test_cost_matrix_equals_batch():
    """65 x 3: every pair bit for bit what dubins_batch gives for it"""
    from python_motion_planning_amd import batch

    s = np.array([c[2] for c in COMMON[20:85]])
    g = np.array([c[3] for c in COMMON[100:103]])
    m = batch.dubins_cost_matrix(s, g, STEP, CURV)
    r = batch.dubins_batch(np.repeat(s, 3, axis=0), np.tile(g, (65, 1)), STEP, CURV, cost_only=True)
    assert np.array_equal(m["cost"].cpu().numpy().ravel(), r["cost"].cpu().numpy())
    assert np.array_equal(m["word"].cpu().numpy().ravel(), r["word"].cpu().numpy())


def test_generation_returns_the_reference_tuple():
    from python_motion_planning_amd import Dubins

    for name in ("ex1_0", "same_position"):
        i, _, s, g, step, curv = CASES[BY[name]]
        cost, mode, x, y, yaw = Dubins(step, curv).generation(s, g)
        assert type(cost) is float and type(mode) is list and type(yaw) is list
        assert isinstance(x, np.ndarray) and isinstance(y, np.ndarray) and all(type(v) is float for v in yaw)
        assert mode == list(C.WORDS[Z["word"][i]])
        C.compare_case(Z, i, Z["word"][i], Z["words6"][i, Z["word"][i], :3], cost, len(x), np.column_stack([x, y, yaw]), 0)
    cost, mode, x, y, yaw = Dubins(STEP, CURV).generation((1, 2, np.pi / 2), (1, 2, np.pi / 2))
    assert cost == 0.0 and mode == ["L", "S", "R"] and len(x) == 0 and len(y) == 0 and yaw == []
    with pytest.raises(ValueError):
        Dubins(STEP, CURV).generation((0, 0, float("nan")), (1, 1, 0))


def test_run_concatenates_the_segments():
    from python_motion_planning_amd import CurveFactory, Dubins

    gen = CurveFactory()("dubins", step=STEP, max_curv=CURV)
    assert isinstance(gen, Dubins)
    px, py, pyaw = gen.run([tuple(p) for p in Z["run_points"]])
    assert type(px) is list and len(px) == len(py) == len(pyaw) == len(Z["run_path"])
    C.rows_close(np.column_stack([px, py, pyaw]), Z["run_path"], "run path")


def test_status_overflow_and_retry():
    from python_motion_planning_amd import batch

    i, _, s, g, step, curv = CASES[BY["ex1_0"]]
    full = _single(i)
    n = int(full["n_points"][0])
    assert n > 10
    r = _host(batch.dubins_batch([s], [g], step, curv, point_cap=10, retry_overflow=False))
    assert int(r["status"][0]) == 2 and int(r["n_points"][0]) == n and r["points"].shape == (1, 10, 3)
    assert np.array_equal(r["points"][0], full["points"][0, :10])
    for k in ("word", "tpq", "cost"):
        assert np.array_equal(r[k], full[k])
    # with the retry, beside a pair that fits the first cap
    j = BY["tiny"]
    r = _host(batch.dubins_batch([s, CASES[j][2]], [g, CASES[j][3]], step, curv, point_cap=10))
    assert r["status"].tolist() == [0, 0] and r["n_points"].tolist() == [n, 4] and r["points"].shape == (2, n, 3)
    assert np.array_equal(_rows(r, 0), _rows(full)) and np.array_equal(_rows(r, 1), _rows(_single(j)))


def test_status_reference_raises_beside_a_good_pair():
    from python_motion_planning_amd import batch

    i, _, s, g, step, curv = CASES[BY["ex1_1"]]
    nan, inf = float("nan"), float("inf")
    r = _host(batch.dubins_batch([(0, 0, nan), s, (nan, 0, 0), (0, 0, 0)], [(1, 1, 0), g, (1, 1, 0), (inf, 0, 0)], step, curv))
    assert r["status"].tolist() == [4, 0, 4, 4] and r["n_points"].tolist()[::2] == [0, 0]
    assert r["word"].tolist() == [255, int(Z["word"][i]), 255, 255]
    full = _single(i)
    assert np.array_equal(_rows(r, 1), _rows(full)) and r["cost"][1] == full["cost"][0]
    m = batch.dubins_cost_matrix([(0, 0, nan), s], [g], step, curv)
    assert m["word"].cpu().numpy().ravel().tolist() == [255, int(Z["word"][i])]
    assert m["cost"].cpu().numpy().ravel().tolist() == [inf, float(full["cost"][0])]


def test_status_of_pairs_no_buffer_holds():
    """A goal 1e9 away has 2.5e9 steps: status 2 with count 0 (the polynomial generator's convention beyond
    2^24 steps); a yaw near 1e300 whose mod2pi (exact IEEE operations, the same on the host) is a multiple of
    its 1.5e284 ulp and no angle, so the reference's pi2pi never ends: status 4.  The cost of the far goal is
    still its distance in curvature units."""
    from python_motion_planning_amd import batch

    yaw = next(k * 1e299 for k in range(1, 100) if abs(C.mod2pi(k * 1e299)) > 64.0)
    r = _host(batch.dubins_batch([(0, 0, 0), (0, 0, yaw), (0, 0, 0)], [(1e9, 0, 0), (5, 5, 0), (10, 0, 0)], STEP, CURV))
    assert r["status"].tolist() == [2, 4, 0] and r["n_points"].tolist() == [0, 0, 28]
    assert r["points"].shape[1] < 1000 and r["cost"][0] == 2.5e8


@pytest.mark.parametrize("step,curv", [(0.0, 0.25), (-0.1, 0.25), (float("nan"), 0.25), (float("inf"), 0.25),
                                       (0.1, 0.0), (0.1, -1.0), (0.1, float("nan")), (0.1, float("inf"))])
def test_refused_parameters(step, curv):
    from python_motion_planning_amd import batch
    from python_motion_planning_amd._lib import PMPError

    with pytest.raises(PMPError, match="pmp_dubins_batch"):
        batch.dubins_batch([(0, 0, 0)], [(10, 0, 0)], step, curv)
    with pytest.raises(PMPError, match="pmp_dubins_cost_matrix"):
        batch.dubins_cost_matrix([(0, 0, 0)], [(10, 0, 0)], step, curv)
