"""tests/golden/bspline.npz (make_golden_bspline.py) without a GPU: the conditions the generator asserted on its
inputs hold in the committed file, and bspline_checks' restatements reproduce the reference on every case."""
import math

import numpy as np

import bspline_checks as C

Z = C.load()
NB, NC = len(Z["bs_names"]), len(Z["cs_names"])
BCASES = [C.bs_case(Z, i) for i in range(NB)]
CCASES = [C.cs_case(Z, i) for i in range(NC)]
BBY = {c["name"]: c for c in BCASES}
CBY = {c["name"]: c for c in CCASES}


def test_case_list():
    n_ex, n_pso = int(Z["bs_n_examples"]), int(Z["bs_n_pso"])
    assert n_ex == 2 * 4 * 3 * 2 and n_pso == 300
    assert {(c["k"], c["param_mode"], c["spline_mode"]) for c in BCASES[:n_ex]} == {
        (k, pm, sm) for k in (2, 3, 4, 5) for pm in C.PARAM_MODES for sm in C.SPLINE_MODES}
    pso = BCASES[n_ex : n_ex + n_pso]
    assert all(c["k"] == 4 and c["step"] == 0.01 and c["status"] == C.ST_OK and c["T"] == 100 for c in pso)
    assert all(tuple(c["points"][0]) == (5, 5) and tuple(c["points"][-1]) == (45, 25) and 2 <= len(c["points"]) <= 7 for c in pso)
    assert max(len(c["points"]) for c in pso) == 7 and len({len(c["points"]) for c in pso}) > 1
    for name in ("len2_k1", "len33", "len64_k3", "len64_k5", "collinear", "d3_8_interpolation", "d3_64_approximation",
                 "d2_in_3d", "step15_3d") + tuple(f"min_k{k}" for k in range(1, 6)) + tuple(f"approx_min_k{k}" for k in range(1, 6)):
        assert BBY[name]["status"] == C.ST_OK, name
    for k in range(1, 6):
        assert len(BBY[f"min_k{k}"]["points"]) == k + 1 and len(BBY[f"approx_min_k{k}"]["points"]) == k + 2
    for name in ("len4_k4", "len2_k4", "repeat", "d3_repeat", "all_equal_3d"):
        assert BBY[name]["status"] == C.ST_LINALG, name
    assert BBY["step15"]["status"] == C.ST_INDEX and BBY["step15_3d"]["T"] == 2 and BBY["step06"]["T"] == 1
    assert np.array_equal(BBY["step06"]["rows"][0], BBY["step06"]["points"][0] + BBY["step06"]["points"][-1])
    assert [BBY[f"T{t}"]["T"] for t in (1, 2, 64, 65)] == [1, 2, 64, 65]
    e = BBY["all_equal"]
    assert e["status"] == C.ST_OK and np.isnan(e["rows"]).all() and np.isnan(e["control"]).all() and math.isnan(e["length"])
    assert e["params"][0] == 0 and np.isnan(e["params"][1:]).all()
    assert len(BBY["len64_k3"]["points"]) == 64 and BBY["d3_64_interpolation"]["dim"] == 3


def test_conditions_asserted_by_the_generator():
    for c in BCASES:
        n, k = len(c["points"]), c["k"]
        if c["status"] == C.ST_LINALG:
            repeated = any(np.array_equal(a, b) for a, b in zip(c["points"][:-1], c["points"][1:]))
            assert n <= k or repeated, c["name"]
        elif c["status"] == C.ST_OK and math.isfinite(c["cond"]):
            assert c["cond"] <= (1e3 if c["spline_mode"] == "interpolation" else 1e4), c["name"]
        if c["spline_mode"] == "approximation":
            assert n >= k + 2, c["name"]
    assert float(Z["bs_rtol"]) == 64 * float(Z["bs_restate_dev"].max()) < 1e-9
    assert float(Z["cs_rtol"]) == 64 * float(Z["cs_restate_dev"].max()) < 1e-9
    n_named = int(Z["cs_n_named"])
    assert not any(c["fragile"] for c in CCASES[n_named:]) and NC - n_named == 200
    assert CBY["pythagorean"]["count"] == 50 and CBY["inf_coord"]["status"] == C.ST_LINALG
    r = CBY["repeat"]
    assert r["status"] == C.ST_OK and r["count"] == len(r["rows"]) > 0 and np.isnan(r["rows"][:, :3]).all()
    rows = np.concatenate([c["rows"] for c in CCASES])
    ok = ~np.isnan(rows[:, 0])
    assert (ok & (np.hypot(rows[:, 3], rows[:, 4]) < 1e-9)).sum() <= 0.01 * len(rows)
    for c in CCASES:
        if c["status"] == C.ST_OK and c["count"]:
            assert (c["count"] - 1) * c["step"] < c["arc"], c["name"]
    lens = {len(c["points"]) for c in CCASES[n_named:]}
    assert min(lens) == 2 and max(lens) == 64


def test_bspline_restatement_reproduces_the_reference():
    worst = 0.0
    for c in BCASES:
        r = C.bs_restate(c["points"], c["step"], c["k"], c["param_mode"], c["spline_mode"], c["three_d"])
        assert r["status"] == c["status"] and r["T"] == c["T"], c["name"]
        if c["status"] != C.ST_OK:
            continue
        sc = C.scale_of(c["points"])
        assert r["n_control"] == c["n_control"] and len(r["rows"]) == c["T"]
        dev = max(C.deviation(r["params"], c["params"], 1.0), C.deviation(r["knot"], c["knot"], 1.0),
                  C.deviation(r["control"], c["control"], sc), C.deviation(r["rows"][c["rows_idx"]], c["rows"], sc),
                  C.deviation([r["length"]], [c["length"]], sc))
        assert dev <= c["restate_dev"] * (1 + 1e-9) + 1e-300, (c["name"], dev, c["restate_dev"])
        worst = max(worst, dev)
    print("worst B-spline restatement deviation", worst, "RTOL", float(Z["bs_rtol"]))
    assert worst * 64 <= float(Z["bs_rtol"]) * (1 + 1e-9)


def test_cubic_restatement_reproduces_the_reference():
    worst = 0.0
    for c in CCASES:
        st, count, rows = C.cs_restate(c["points"], c["step"], None if c["status"] != C.ST_OK else c["rows_idx"])
        assert st == c["status"] and count == c["count"], c["name"]
        if st != C.ST_OK:
            continue
        assert np.array_equal(C.cs_table(c["points"])[-1:], [c["arc"]])
        dev, _ = C.cs_deviation(rows, c["rows"], C.scale_of(c["points"]))
        worst = max(worst, dev)
    print("worst cubic-spline restatement deviation", worst, "RTOL", float(Z["cs_rtol"]))
    assert worst * 64 <= float(Z["cs_rtol"]) * (1 + 1e-9)


def test_host_methods_of_the_classes():
    """baseFunction, generation and spline run without a device: against the fixture's rows."""
    from python_motion_planning_amd import BSpline, BSpline3D, CubicSpline

    c = BBY["ex1_k3_centripetal_interpolation"]
    g = BSpline(c["step"], c["k"])
    rows = g.generation(np.linspace(0, 1, c["T"]), c["k"], c["knot"].tolist(), c["control"])
    assert C.deviation(rows, c["rows"], C.scale_of(c["points"])) <= float(Z["bs_rtol"])
    knot = c["knot"].tolist()
    assert g.baseFunction(0, 3, 0.0, knot) == 1.0 and g.baseFunction(len(c["control"]) - 1, 3, 1.0, knot) == 0.0
    assert str(g) == "B-Spline Curve" and str(BSpline3D(0.1, 2)) == "B-Spline Curve 3D" and str(CubicSpline(0.1)) == "Cubic Spline"
    for bad in (dict(param_mode="x"), dict(spline_mode="y")):
        for cls in (BSpline, BSpline3D):
            try:
                cls(0.1, 3, **bad)
            except AssertionError:
                continue
            raise AssertionError("the constructor accepted " + str(bad))
    cc = CBY["ex1_0.5"]
    s = C.cs_table(cc["points"])
    t = np.arange(0, s[-1], cc["step"])
    gen = CubicSpline(cc["step"])
    px, dpx = gen.spline(s.tolist(), cc["points"][:, 0].tolist(), t)
    py, dpy = gen.spline(s.tolist(), cc["points"][:, 1].tolist(), t)
    rows = np.array([px, py, np.arctan2(dpy, dpx), dpx, dpy]).T
    assert C.cs_deviation(rows, cc["rows"], C.scale_of(cc["points"]))[0] <= float(Z["cs_rtol"])
    assert gen.generation((0, 0, 0), (1, 1, 1)) is None
