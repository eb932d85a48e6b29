"""Dubins without a device: the sequential restatement of csrc/dubins.hip's arithmetic (dubins_checks.py)
against the reference's own runs (tests/golden/dubins.npz, made by make_golden_dubins.py), and the
feature's exposure through the library and the package."""
import inspect
import math

import numpy as np
import pytest

import dubins_checks as C
from golden_io import seg

Z = C.load()
CASES = list(C.cases(Z))
BY = {c[1]: c[0] for c in CASES}


def test_fixture_holds_the_cases():
    assert len(CASES) == 322 and int(Z["n_named"]) == 22
    want = dict(axis_fwd=28, zero_origin=0, zero_offset=0, same_position=74, tiny=4, diag_fine=323, diag_coarse=16,
                diag_odd=37)
    for name, n in want.items():
        assert int(Z["count"][BY[name]]) == n, name
    assert C.WORDS[Z["word"][BY["same_position"]]] == "LRL"
    assert C.WORDS[Z["word"][BY["zero_origin"]]] == "LSL" and C.WORDS[Z["word"][BY["zero_offset"]]] == "LSR"
    assert Z["cost"][BY["zero_origin"]] == 0.0 and Z["cost"][BY["zero_offset"]] == 0.0
    assert set(Z["word"].tolist()) == set(range(6))
    assert sum(n.startswith("ex") for n in BY) == 13 and sum(n.startswith("rng_") for n in BY) == 300
    assert not (Z["fragile"] & Z["real"]).any()
    plain = np.array([n.startswith("ex") or n.startswith("rng_") for _, n, *_ in CASES])
    assert Z["fragile"][plain].mean() <= 0.01
    assert int(Z["has_rows"].sum()) == 22 + 64 and Z["run_points"].shape == (8, 3)
    assert len(Z["run_path"]) == sum(int(Z["count"][BY[f"ex1_{i}"]]) for i in range(7))
    assert Z["cm_cost"].shape == (5, 7) and Z["cm_word"].shape == (5, 7)
    for i in range(len(CASES)):  # the chosen word is the first strictly cheapest of the recorded six
        c = Z["words6"][i, :, 3]
        assert int(Z["word"][i]) == int(np.nanargmin(c)) and Z["cost"][i] == np.nanmin(c)


def test_restatement_reproduces_reference():
    """Every fixture case under the rules of dubins_checks (fragile cases with the recorded word)."""
    worst, fragile = {}, []
    for i, name, s, g, step, curv in CASES:
        r = C.restate(s, g, step, curv, force_word=int(Z["word"][i]) if Z["fragile"][i] else None)
        if C.compare_case(Z, i, r["word"], r["tpq"], r["cost"], len(r["points"]), r["points"], r["status"], worst):
            fragile.append(name)
        else:  # all six words, feasible or not
            C.close(r["words6"], Z["words6"][i], name + " words6")
    print("worst deviation per column:", {k: f"{v:.3g}" for k, v in worst.items()}, "fragile:", fragile)


def test_restatement_cost_matrix_and_run_path():
    step, curv = (float(v) for v in Z["cm_params"])
    for a in range(5):
        for b in range(7):
            r = C.restate(tuple(Z["cm_start"][a]), tuple(Z["cm_goal"][b]), step, curv)
            assert r["word"] == int(Z["cm_word"][a, b])
            C.close(r["cost"], Z["cm_cost"][a, b], f"cost matrix {a} {b}")
    poses = [(p[0], p[1], float(np.deg2rad(p[2]))) for p in Z["run_points"]]
    rows = np.concatenate([C.restate(poses[k], poses[k + 1], 0.1, 0.25)["points"] for k in range(7)])
    C.rows_close(rows, Z["run_path"], "run path")


def test_count_is_the_repeated_sum():
    """(0,0,0) -> (10,0,0) at step 0.1, max_curv 0.25: p = 2.5 takes 24 steps of the repeated sum (28
    points); k * step <= p holds for one more (29)."""
    i = BY["axis_fwd"]
    p = float(Z["words6"][i, int(Z["word"][i]), 1])
    assert p == 2.5
    k = 0
    while (k + 1) * 0.1 <= p:
        k += 1
    assert C.piece_steps(0.1, p) == 24 and k == 25
    assert len(C.restate((0, 0, 0), (10, 0, 0), 0.1, 0.25, force_word=int(Z["word"][i]))["points"]) == 28 == k + 3
    assert len(seg(Z["rows"], Z["rows_off"], i)) == 28


def test_restatement_status():
    assert C.restate((0, 0, float("nan")), (1, 1, 0), 0.1, 0.25)["status"] == 4
    assert C.restate((0, 0, 0), (float("inf"), 1, 0), 0.1, 0.25)["status"] == 4


# ---- exposure: each of these fails without the feature --------------------------------------------------
def test_signatures_registered_and_symbols_built():
    from python_motion_planning_amd import _lib, batch

    assert len(_lib.SIGNATURES["pmp_dubins_batch"][1]) == 13
    assert len(_lib.SIGNATURES["pmp_dubins_cost_matrix"][1]) == 9
    L = _lib.load_library()
    assert hasattr(L, "pmp_dubins_batch") and hasattr(L, "pmp_dubins_cost_matrix")
    assert callable(batch.dubins_batch) and callable(batch.dubins_cost_matrix)
    assert _lib.DUBINS_WORDS == C.WORDS
    p = _lib.DubinsParams(0.1, 0.25)
    assert (p.step, p.max_curv) == (0.1, 0.25)
    assert list(inspect.signature(batch.dubins_batch).parameters) == [
        "starts", "goals", "step", "max_curv", "cost_only", "point_cap", "retry_overflow"]


def test_classes_are_exported_with_the_reference_signature():
    import python_motion_planning_amd as pmp

    for n in ("Dubins", "Curve", "CurveFactory"):
        assert n in pmp.__all__ and hasattr(pmp, n)
    assert issubclass(pmp.Dubins, pmp.Curve)
    assert list(inspect.signature(pmp.Dubins.__init__).parameters) == ["self", "step", "max_curv"]
    d = pmp.Dubins(0.1, 0.25)
    assert str(d) == "Dubins Curve" and d.step == 0.1 and d.max_curv == 0.25
    for m in ("generation", "run", "generation_batch", "cost_matrix", "trigonometric", "pi2pi", "mod2pi", "length"):
        assert callable(getattr(d, m))
    assert d.mod2pi(-0.5) == C.mod2pi(-0.5) and d.pi2pi(4.0) == 4.0 - 2.0 * math.pi
    assert d.length([(0, 0), (3, 4), (3, 6)]) == 7.0
    assert d.trigonometric(0.3, 0.1) == (math.sin(0.3), math.sin(0.1), math.cos(0.3), math.cos(0.1), math.sin(0.3 - 0.1),
                                         math.cos(0.3 - 0.1))
    with pytest.raises(TypeError):
        pmp.Curve(0.1)  # abstract, as the reference's
    with pytest.raises(AssertionError):
        d.run([(0, 0, 0)])


def test_factory_names():
    import python_motion_planning_amd as pmp

    f = pmp.CurveFactory()
    d = f("dubins", step=0.1, max_curv=0.25)
    assert isinstance(d, pmp.Dubins) and (d.step, d.max_curv) == (0.1, 0.25)
    for name in ("bezier", "polynomial", "reeds_shepp", "cubic_spline", "bspline", "fem_pos_smoother"):
        with pytest.raises(NotImplementedError):
            f(name, step=0.1)
    with pytest.raises(ValueError):
        f("clothoid")
