"""Polynomial and Bezier without a device: the sequential restatement of csrc/polycurve.hip's arithmetic
(polycurve_checks.py) against the reference's own runs (tests/golden/polycurve.npz, made by
make_golden_polycurve.py), and the feature's exposure through the library and the package."""
import inspect
import math

import numpy as np
import pytest

import polycurve_checks as C
from golden_io import seg

Z = C.load()
CASES = list(C.cases(Z))
BCASES = list(C.bezier_cases(Z))
BY = {c[1]: c[0] for c in CASES}
BBY = {c[1]: c[0] for c in BCASES}


def test_fixture_holds_the_cases():
    assert len(CASES) == 347 and int(Z["n_examples"]) == 39 and int(Z["n_named"]) == 8
    assert sum(n.startswith("rng_") for n in BY) == 300
    i = BY["same_pose"]
    assert int(Z["count"][i]) == 11 and int(Z["t_index"][i]) == 0 and Z["T"][i] == 1.0
    assert not seg(Z["rows"], Z["rows_off"], i)[:, 1:].any()
    i = BY["start_yaw_back"]
    r0 = seg(Z["rows"], Z["rows_off"], i)[0]
    assert int(Z["count"][i]) == 131 and r0[3] == 0.0 and math.copysign(1.0, r0[3]) == 1.0 and r0[4] == 0.0
    for name in ("far_goal", "nan_pose", "inf_pose"):
        assert int(Z["count"][BY[name]]) == 0 and int(Z["t_index"][BY[name]]) == -1 and Z["T"][BY[name]] == np.inf
    assert int(Z["t_index"][BY["one_candidate"]]) == 0 and Z["params"][BY["one_candidate"], 0] == 29.0
    assert int(Z["t_index"][BY["last_candidate"]]) == 28 and Z["params"][BY["last_candidate"], 0] == 1.0
    assert Z["params"][BY["dt_coarse"], 3] == 0.5 and int(Z["count"][BY["dt_coarse"]]) > 0
    rnd = np.array([n.startswith("rng_") for _, n, *_ in CASES])
    assert Z["t_index"][rnd].max() > 128 and 0 <= Z["t_index"][rnd].min() and (Z["count"][rnd] > 64).any()
    assert Z["margin"].min() >= 1e-6
    flags = np.concatenate([seg(Z["rows_safe"], Z["rows_off"], i) for i, n, *_ in CASES if n != "same_pose"])
    assert (~flags).mean() <= 0.01
    assert int(Z["full"].sum()) == 8 + 24 and Z["tm_T"].shape == (5, 7) and Z["tm_index"].shape == (5, 7)
    assert len(Z["run_path"]) == sum(int(Z["count"][BY[f"ex1_{i}_0"]]) for i in range(7))
    # Bezier
    assert len(BCASES) == 217 and int(Z["b_n_named"]) == 17
    assert [int(Z["b_count"][BBY[n]]) for n in ("n0", "n1", "n2", "pythagorean")] == [0, 1, 2, 50]
    assert np.array_equal(seg(Z["b_rows"], Z["b_rows_off"], BBY["n1"])[0], Z["b_start"][BBY["n1"], :2])
    assert not Z["b_fragile"][int(Z["b_n_named"]):].any() and Z["b_fragile"][BBY["pythagorean"]]


def test_restatement_reproduces_reference_polynomial():
    """Every polynomial case under the rules of polycurve_checks; prints the worst deviation per column, from
    which RTOL is derived (16 times the worst, rounded up to a power of ten, within the 1e-5 contract)."""
    worst = {}
    for i, name, s, g, prm in CASES:
        r = C.restate_polynomial(s, g, *prm)
        C.compare_polynomial(Z, i, r["t_index"], r["T"], len(r["rows"]), r["rows"], r["status"], worst)
    print("worst deviation per column:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert 16 * max(worst.values()) <= C.RTOL <= 1e-5


def test_restatement_reproduces_reference_bezier():
    worst, other = {}, []
    for i, name, s, g, (step, offset) in BCASES:
        r = C.restate_bezier(s, g, step, offset)
        if C.compare_bezier(Z, i, r["control"], len(r["rows"]), r["rows"], r["status"], worst):
            other.append(name)
    print("worst deviation per column:", {k: f"{v:.3g}" for k, v in worst.items()}, "other count:", other)
    assert 16 * max(worst.values()) <= C.RTOL


def test_restatement_time_matrix_and_run_paths():
    prm = tuple(float(v) for v in Z["tm_params"])
    for a in range(5):
        for b in range(7):
            r = C.restate_polynomial(tuple(Z["tm_start"][a]), tuple(Z["tm_goal"][b]), *prm)
            assert r["t_index"] == int(Z["tm_index"][a, b])
            C.close(r["T"], Z["tm_T"][a, b], f"time matrix {a} {b}")
    pts = Z["run_points"]
    v = [0.0] + [1.0] * (len(pts) - 1)
    acc = [(v[i + 1] - v[i]) / 5 for i in range(len(pts) - 1)] + [0.0]
    st = [(p[0], p[1], float(np.deg2rad(p[2])), v[i], acc[i]) for i, p in enumerate(pts)]
    rows = np.concatenate([C.restate_polynomial(st[k], st[k + 1], *Z["run_params"])["rows"] for k in range(len(pts) - 1)])
    assert len(rows) == len(Z["run_path"])
    C.close(rows[:, 1:3], Z["run_path"][:, :2], "run path x, y")
    bp = [(p[0], p[1], float(np.deg2rad(p[2]))) for p in Z["b_run_points"]]
    brows = np.concatenate([C.restate_bezier(bp[k], bp[k + 1], *Z["b_run_params"])["rows"] for k in range(len(bp) - 1)])
    C.close(brows, Z["b_run_path"], "bezier run path")


def test_arange_and_linspace_rules():
    """np.arange(1, 30, 0.1)[i] is 1 + i ((1 + 0.1) - 1), not 1 + i 0.1; np.linspace(0, 1, n)[i] is i (1 / (n - 1)),
    not i / (n - 1)."""
    T = C.candidate_times(0.1, 1.0, 30.0)
    ref = np.arange(1, 30, 0.1)
    assert len(T) == len(ref) == 290 and T == ref.tolist()
    assert T[3] == 1.3000000000000003 == 1 + 3 * ((1 + 0.1) - 1) and T[3] != 1 + 3 * 0.1
    assert T[7] == ref[7] == 1 + 7 * ((1 + 0.1) - 1) and T[289] == ref[289]
    assert C.sample_count(T[3], 0.1) == len(np.arange(0.0, T[3] + 0.1, 0.1))
    t = C.linspace01(141)
    ref = np.linspace(0, 1, 141)
    assert t == ref.tolist() and t[7] == 7 * (1 / 140) and t[7] != 7 / 140 and t[140] == 1.0
    assert t[93] == ref[93] == 93 * (1 / 140)
    assert C.linspace01(1) == [0.0] and C.linspace01(0) == [] and C.linspace01(2) == [0.0, 1.0]


def test_restatement_status():
    nan, inf = float("nan"), float("inf")
    assert C.restate_polynomial((0, 0, 0, 0, 0), (1e6, 0, 0, 1, 0), 0.1, 1.0, 0.5)["status"] == 1
    assert C.restate_polynomial((0, 0, inf, 0, 0), (5, 5, 0, 1, 0), 0.5, 1.0, 0.5)["status"] == 1
    assert C.restate_polynomial((0, 0, 0, 0, 0), (5, 5, 0, 1, 0), 0.5, 1.0, 0.5, t_min=3.0, t_max=3.0)["t_index"] == -1
    assert C.restate_bezier((0, nan, 0), (1, 1, 0), 0.1, 3.0)["status"] == 4
    assert C.restate_bezier((0, 0, 0), (inf, 1, 0), 0.1, 3.0)["status"] == 4


# ---- exposure: each of these fails without the feature --------------------------------------------------
def test_signatures_registered_and_symbols_built():
    from python_motion_planning_amd import _lib, batch

    assert len(_lib.SIGNATURES["pmp_polycurve_batch"][1]) == 12
    assert len(_lib.SIGNATURES["pmp_polycurve_time_matrix"][1]) == 9
    assert len(_lib.SIGNATURES["pmp_bezier_batch"][1]) == 11
    L = _lib.load_library()
    for name in ("pmp_polycurve_batch", "pmp_polycurve_time_matrix", "pmp_bezier_batch"):
        assert hasattr(L, name)
    p = _lib.PolyCurveParams(0.1, 1.0, 0.5, 0.1, 1.0, 30.0)
    assert (p.step, p.max_acc, p.max_jerk, p.dt, p.t_min, p.t_max) == (0.1, 1.0, 0.5, 0.1, 1.0, 30.0)
    b = _lib.BezierParams(0.1, 3.0)
    assert (b.step, b.offset) == (0.1, 3.0)
    assert list(inspect.signature(batch.polynomial_batch).parameters) == [
        "starts", "goals", "step", "max_acc", "max_jerk", "dt", "t_min", "t_max", "cost_only", "point_cap", "retry_overflow"]
    assert list(inspect.signature(batch.polynomial_time_matrix).parameters) == [
        "starts", "goals", "step", "max_acc", "max_jerk", "dt", "t_min", "t_max"]
    assert list(inspect.signature(batch.bezier_batch).parameters) == [
        "starts", "goals", "step", "offset", "cost_only", "point_cap", "retry_overflow"]
    sig = inspect.signature(batch.polynomial_batch).parameters
    assert (sig["dt"].default, sig["t_min"].default, sig["t_max"].default) == (0.1, 1, 30)
    assert batch._polycurve_point_cap(p) == 301


def test_classes_are_exported_with_the_reference_signature():
    import python_motion_planning_amd as pmp

    for n in ("Polynomial", "Bezier"):
        assert n in pmp.__all__ and hasattr(pmp, n) and issubclass(getattr(pmp, n), pmp.Curve)
    assert list(inspect.signature(pmp.Polynomial.__init__).parameters) == ["self", "step", "max_acc", "max_jerk"]
    assert list(inspect.signature(pmp.Bezier.__init__).parameters) == ["self", "step", "offset"]
    g = pmp.Polynomial(2, 1.0, 0.5)
    assert str(g) == "Quintic Polynomial Curve" and (g.step, g.max_acc, g.max_jerk) == (2, 1.0, 0.5)
    assert (g.dt, g.t_min, g.t_max) == (0.1, 1, 30)
    for m in ("generation", "run", "generation_batch", "time_matrix"):
        assert callable(getattr(g, m))
    t = g.Trajectory()
    assert t.size == 0 and all(getattr(t, k) == [] for k in C.COLS)
    t.time.append(0.0)
    with pytest.raises(AssertionError):
        t.size
    t.clear()
    assert t.size == 0
    assert not hasattr(g, "Poly")  # the kernel's
    b = pmp.Bezier(0.1, 3.0)
    assert str(b) == "Bezier Curve" and (b.step, b.offset) == (0.1, 3.0)
    for m in ("generation", "run", "generation_batch", "bezier", "getControlPoints"):
        assert callable(getattr(b, m))
    for gen in (g, b):
        with pytest.raises(AssertionError):
            gen.run([(0, 0, 0)])


def test_bezier_host_methods_equal_the_fixture():
    import python_motion_planning_amd as pmp

    for i, name, s, g, (step, offset) in BCASES[:40]:
        gen = pmp.Bezier(step, offset)
        ctrl = gen.getControlPoints(s, g)
        assert type(ctrl) is list and len(ctrl) == 4 and all(type(c) is tuple for c in ctrl)
        C.close(np.array(ctrl, np.float64), Z["b_control"][i], name + " control")
        idx, ref = seg(Z["b_rows_idx"], Z["b_rows_off"], i), seg(Z["b_rows"], Z["b_rows_off"], i)
        ts = np.linspace(0, 1, int(Z["b_count"][i]))
        for k, row in zip(idx, ref):
            p = gen.bezier(ts[k], [tuple(c) for c in Z["b_control"][i]])
            assert isinstance(p, np.ndarray) and p.shape == (2,)
            C.close(p, row, f"{name} point {k}")
    # any number of control points: a line, a quadratic
    gen = pmp.Bezier(0.1, 3.0)
    assert np.array_equal(gen.bezier(0.25, [(0, 0), (4, 8)]), [1.0, 2.0])
    assert np.array_equal(gen.bezier(0.5, [(0, 0), (2, 4), (4, 0)]), [2.0, 2.0])


def test_factory_still_refuses_the_two_names():
    import python_motion_planning_amd as pmp

    f = pmp.CurveFactory()
    with pytest.raises(NotImplementedError):
        f("bezier", step=0.1, offset=3.0)
    with pytest.raises(NotImplementedError):
        f("polynomial", step=2, max_acc=1.0, max_jerk=0.5)
