"""BSpline, BSpline3D and CubicSpline on gfx950 (pmp_bspline_batch, pmp_cubic_spline_batch) against the
reference's own runs (tests/golden/bspline.npz, make_golden_bspline.py), under the rules of bspline_checks.py.

Worst deviations measured on an MI355X over the fixture (the tolerances are the fixture's: bs_rtol 2.12e-12,
cs_rtol 1.71e-13): see DESIGN.md 3.11."""
import functools

import numpy as np
import pytest

import bspline_checks as C

pytestmark = pytest.mark.gpu

Z = C.load()
RTOL, CS_RTOL = float(Z["bs_rtol"]), float(Z["cs_rtol"])
BCASES = [C.bs_case(Z, i) for i in range(len(Z["bs_names"]))]
CCASES = [C.cs_case(Z, i) for i in range(len(Z["cs_names"]))]
BBY = {c["name"]: i for i, c in enumerate(BCASES)}
CBY = {c["name"]: i for i, c in enumerate(CCASES)}
N_EX, N_PSO = int(Z["bs_n_examples"]), int(Z["bs_n_pso"])
PSO = list(range(N_EX, N_EX + N_PSO))
BKEYS = ("params", "knot", "control", "n_control", "points", "length", "status")
CKEYS = ("arc_length", "n_points", "points", "status")


def _host(r, keys):
    return {k: None if r[k] is None else r[k].cpu().numpy() for k in keys}


def _launch(cases, **kw):
    """The cases (sharing step, k, modes and class) in one launch"""
    from python_motion_planning_amd import batch

    c = cases[0]
    r = batch.bspline_batch([x["points"] for x in cases], c["step"], c["k"], c["param_mode"], c["spline_mode"],
                            three_d=c["three_d"], **kw)
    return dict(_host(r, BKEYS), n_samples=r["n_samples"])


@functools.lru_cache(maxsize=None)
def _single(i):
    """B-spline case i in a launch of its own (computed once, shared by the tests)"""
    return _launch([BCASES[i]])


@functools.lru_cache(maxsize=None)
def _csingle(i):
    from python_motion_planning_amd import batch

    c = CCASES[i]
    return _host(batch.cubic_spline_batch([c["points"]], c["step"], with_derivative=True), CKEYS)


def _compare(c, r, q, worst):
    """Outputs q of launch r against fixture case c"""
    k, nc = c["k"], c["n_control"]
    assert int(r["status"][q]) == c["status"], c["name"]
    assert int(r["n_control"][q]) == nc, c["name"]
    assert C.deviation(r["params"][q, :nc], c["params"], 1.0) <= RTOL, c["name"]
    assert C.deviation(r["knot"][q, : nc + k + 1], c["knot"], 1.0) <= RTOL, c["name"]
    if c["status"] != C.ST_OK:
        assert np.isnan(r["control"][q, :nc]).all() and np.isnan(r["length"][q]) and np.isnan(r["points"][q]).all()
        return
    assert r["n_samples"] == c["T"] == r["points"].shape[1], c["name"]
    sc = C.scale_of(c["points"])
    dev = dict(control=C.deviation(r["control"][q, :nc], c["control"], sc),
               rows=C.deviation(r["points"][q][c["rows_idx"]], c["rows"], sc),
               length=C.deviation([r["length"][q]], [c["length"]], sc))
    for key, v in dev.items():
        worst[key] = max(worst.get(key, 0.0), v)
        assert v <= RTOL, (c["name"], key, v)


def test_every_bspline_case_in_its_own_launch():
    """Status, n_control and the row count exact; parameters, knots, control points, rows and length within
    the fixture's RTOL; NaN patterns equal (all_equal: every value NaN, status 0)."""
    worst = {}
    for i, c in enumerate(BCASES):
        if c["status"] == C.ST_INDEX:  # no launch: the class raises (test_classes)
            continue
        _compare(c, _single(i), 0, worst)
    print("worst B-spline deviation:", {k: f"{v:.3g}" for k, v in worst.items()}, "RTOL", RTOL)
    e = _single(BBY["all_equal"])
    assert np.isnan(e["points"]).all() and np.isnan(e["control"][0, :6]).all() and int(e["status"][0]) == 0


def test_rows_beyond_the_stored_ones_equal_the_restatement():
    for name in ("pso_100", "pso_299"):
        c = BCASES[BBY[name]]
        want = C.bs_restate(c["points"], c["step"], c["k"], c["param_mode"], c["spline_mode"], c["three_d"])
        assert C.deviation(_single(BBY[name])["points"][0], want["rows"], C.scale_of(c["points"])) <= RTOL


def _k4(name):
    return dict(BCASES[BBY[name]], k=4, name=name + "@k4")


def test_ragged_launch_equals_single_launches():
    """All PSO-shaped cases with a 2-, a 4- (= k: both singular), a 33- and a 64-point list in one launch of 304
    curves: every curve's outputs are the single launch's, bit for bit, the singular ones included."""
    extra = [_k4("len2_k4"), _k4("len4_k4"), _k4("len33"), _k4("len64_k3")]
    cases = [BCASES[i] for i in PSO[:150]] + extra[:2] + [BCASES[i] for i in PSO[150:]] + extra[2:]
    assert len(cases) == 304 and len(cases) % 64 and {len(c["points"]) for c in cases} >= {2, 4, 7, 33, 64}
    r = _launch(cases)
    assert r["params"].shape == (304, 64) and r["knot"].shape == (304, 69) and r["points"].shape == (304, 100, 2)
    singles = {c["name"]: (_single(BBY[c["name"]]) if c["name"] in BBY else _launch([c])) for c in cases}
    n_sing = 0
    for q, c in enumerate(cases):
        s, n = singles[c["name"]], len(c["points"])
        assert r["status"][q] == s["status"][0] and r["n_control"][q] == s["n_control"][0] == n, c["name"]
        n_sing += int(r["status"][q] == C.ST_LINALG)
        for key, m in (("params", n), ("knot", n + 5), ("control", n)):
            assert np.array_equal(r[key][q, :m], s[key][0, :m], equal_nan=True), (c["name"], key)
            assert not r[key][q, m:].any(), (c["name"], key)
        assert np.array_equal(r["points"][q], s["points"][0], equal_nan=True), c["name"]
        assert np.array_equal(r["length"][q], s["length"][0], equal_nan=True), c["name"]
    assert n_sing == 2
    assert int(singles["len33@k4"]["status"][0]) == 0 and int(singles["len64_k3@k4"]["status"][0]) == 0


def test_cost_only_equals_the_sampling_launch():
    cases = [BCASES[i] for i in PSO[:70]]
    a, b = _launch(cases), _launch(cases, cost_only=True)
    assert b["points"] is None
    for key in ("params", "knot", "control", "n_control", "length", "status"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def test_sampler_round_boundaries():
    """T = 1, 2, 64, 65 and 100: the rows on either side of the 64-row rounds, against the reference's"""
    for name, T in (("T1", 1), ("T2", 2), ("T64", 64), ("T65", 65), ("pso_0", 100), ("step06", 1)):
        r, c = _single(BBY[name]), BCASES[BBY[name]]
        assert r["points"].shape == (1, T, 2) and len(c["rows"]) == T
        assert C.deviation(r["points"][0], c["rows"], C.scale_of(c["points"])) <= RTOL
    p = BCASES[BBY["T65"]]["points"]
    assert np.array_equal(_single(BBY["T65"])["points"][0, -1], p[-1]) and np.array_equal(_single(BBY["T65"])["points"][0, 0], p[0])


def test_variants_agree_where_their_rules_coincide():
    """2D points under BSpline's and BSpline3D's rules: uniform parameters are the same bits, the
    others differ by hypot against sqrt of the squared sum"""
    cases = [BCASES[i] for i in PSO[:40]]
    for pm, exact in (("uniform_spaced", True), ("centripetal", False), ("chord_length", False)):
        a = _launch([dict(c, param_mode=pm) for c in cases])
        b = _launch([dict(c, param_mode=pm, three_d=True) for c in cases])
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["n_control"], b["n_control"])
        for key in ("params", "knot", "control", "points", "length"):
            if exact:
                assert np.array_equal(a[key], b[key]), (pm, key)
            else:
                assert C.deviation(a[key], b[key], 45.0 if key not in ("params", "knot") else 1.0) <= RTOL, (pm, key)


def test_classes():
    from python_motion_planning_amd import BSpline, BSpline3D

    c = BCASES[BBY["ex1_k3_centripetal_interpolation"]]
    pts3 = [(float(x), float(y), 30.0) for x, y in c["points"]]  # 3-tuples: cut to (x, y)
    g = BSpline(0.01, 3)
    path = g.run(pts3, display=False)
    assert isinstance(path, list) and len(path) == 100 and all(type(p) is tuple and len(p) == 2 for p in path)
    assert all(type(v) is float for p in path for v in p)
    sc = C.scale_of(c["points"])
    assert C.deviation(path, c["rows"], sc) <= RTOL
    assert abs(g.length(path) - c["length"]) <= RTOL * sc * 100
    params = g.paramSelection(pts3)
    knot = g.knotGeneration(params, len(pts3))
    assert type(params) is list and type(knot) is list and len(knot) == len(pts3) + 4
    assert C.deviation(params, c["params"], 1.0) <= RTOL and C.deviation(knot, c["knot"], 1.0) <= RTOL
    ctrl = g.interpolation([p[:2] for p in pts3], params, knot)
    assert isinstance(ctrl, np.ndarray) and ctrl.shape == (8, 2) and C.deviation(ctrl, c["control"], sc) <= RTOL
    assert C.deviation(g.generation(np.linspace(0, 1, 100), 3, knot, ctrl), c["rows"], sc) <= RTOL
    a = BCASES[BBY["ex1_k3_centripetal_approximation"]]
    ga = BSpline(0.01, 3, spline_mode="approximation")
    ca = ga.approximation([p[:2] for p in pts3], params, knot)
    assert ca.shape == (7, 2) and C.deviation(ca, a["control"], sc) <= RTOL
    assert C.deviation(ga.run(pts3), a["rows"], sc) <= RTOL
    both = g.run_batch([pts3, [tuple(p) for p in BCASES[PSO[0]]["points"]]])
    assert len(both) == 2 and C.deviation(both[0], path, sc) == 0.0
    pair = BSpline(0.01, 4).run_batch([[tuple(p) for p in BCASES[i]["points"]] for i in PSO[:2]])
    assert all(C.deviation(pair[j], BCASES[PSO[j]]["rows"], 45.0) <= RTOL for j in range(2))
    with pytest.raises(np.linalg.LinAlgError):
        g.run([tuple(p) for p in BCASES[BBY["repeat"]]["points"]])
    with pytest.raises(np.linalg.LinAlgError):
        BSpline(0.01, 4).run([(0, 0), (3, 4)])
    with pytest.raises(IndexError):
        BSpline(1.5, 4).run(pts3)
    with pytest.raises(NotImplementedError):
        BSpline(0.01, 4, spline_mode="approximation").run(pts3[:5])
    with pytest.raises(AssertionError):
        g.run(pts3[:1])
    with pytest.raises(AssertionError):
        BSpline(0.01, 3, param_mode="chord")
    with pytest.raises(AssertionError):
        BSpline3D(0.01, 3, spline_mode="smooth")
    d = BCASES[BBY["d3_8_interpolation"]]
    g3 = BSpline3D(0.01, 3)
    p3 = g3.run([tuple(p) for p in d["points"]], display=False)
    assert len(p3) == 100 and all(type(p) is tuple and len(p) == 3 for p in p3)
    assert C.deviation(p3, d["rows"], C.scale_of(d["points"])) <= RTOL
    two = BSpline3D(1.5, 4).run([tuple(p) for p in BCASES[BBY["step15_3d"]]["points"]])
    assert C.deviation(two, BCASES[BBY["step15_3d"]]["rows"], 45.0) <= RTOL and len(two) == 2
    with pytest.raises(np.linalg.LinAlgError):
        g3.run([tuple(p) for p in BCASES[BBY["d3_repeat"]]["points"]])
    with pytest.raises(np.linalg.LinAlgError):
        g3.run([(2.0, 3.0, 1.0)] * 6)


def test_refused_parameters_name_the_entry():
    from python_motion_planning_amd import batch
    from python_motion_planning_amd._lib import PMPError

    seven = BCASES[BBY["T1"]]["points"]
    walk65 = np.cumsum(np.ones((65, 2)), axis=0)
    bad = [dict(k=0), dict(k=6), dict(curves=[walk65]), dict(curves=[seven[:1]]), dict(step=0.0), dict(step=float("nan")),
           dict(step=1e-9), dict(curves=[np.ones((5, 4)) * np.arange(5)[:, None]]), dict(step=1.5),
           dict(k=4, spline_mode="approximation", curves=[seven[:5]])]
    for kw in bad:
        args = dict(curves=[seven], step=0.01, k=4)
        args.update(kw)
        with pytest.raises(PMPError, match="pmp_bspline_batch"):
            batch.bspline_batch(**args)
    for kw in (dict(step=0.0), dict(step=float("inf")), dict(curves=[seven[:1]]), dict(curves=[np.zeros((3, 4))])):
        args = dict(curves=[seven], step=0.1)
        args.update(kw)
        with pytest.raises(PMPError, match="pmp_cubic_spline_batch"):
            batch.cubic_spline_batch(**args)


# ---- cubic spline --------------------------------------------------------------------------------------------
def test_every_cubic_case_in_its_own_launch():
    """Count and status exact on every case (the fragile one too: its quotient is the host's own division);
    x, y and yaw under bspline_checks' rules; the NaN rows of a repeated waypoint; status 4 of an infinite one."""
    worst, skipped, total = 0.0, 0, 0
    for i, c in enumerate(CCASES):
        r = _csingle(i)
        assert int(r["status"][0]) == c["status"], c["name"]
        assert int(r["n_points"][0]) == c["count"], c["name"]
        if c["status"] != C.ST_OK:
            continue
        assert r["arc_length"][0] == c["arc"], c["name"]
        rows = r["points"][0, : c["count"]][c["rows_idx"]]
        dev, skip = C.cs_deviation(rows, c["rows"], C.scale_of(c["points"]))
        assert dev <= CS_RTOL, (c["name"], dev)
        worst, skipped, total = max(worst, dev), skipped + skip, total + len(rows)
    print("worst cubic-spline deviation:", f"{worst:.3g}", "RTOL", CS_RTOL, "yaw skipped on", skipped, "of", total, "rows")
    assert skipped <= 0.01 * total
    rep = _csingle(CBY["repeat"])
    assert int(rep["n_points"][0]) > 0 and np.isnan(rep["points"][0, : int(rep["n_points"][0]), :3]).all()
    assert int(_csingle(CBY["pythagorean"])["n_points"][0]) == 50


def test_cubic_rows_beyond_the_stored_ones_equal_the_restatement():
    long = [c["name"] for c in CCASES if c["name"].startswith("rng_") and c["count"] > 200 and len(c["rows"]) == 3]
    for name in ("ex1_0.1", long[0], long[-1]):
        c = CCASES[CBY[name]]
        st, count, want = C.cs_restate(c["points"], c["step"])
        r = _csingle(CBY[name])
        assert count == int(r["n_points"][0]) > 64
        assert C.cs_deviation(r["points"][0, :count], want, C.scale_of(c["points"]))[0] <= CS_RTOL


def test_cubic_batch_equals_singles_and_overflow_retry():
    from python_motion_planning_amd import batch

    sel = [i for i, c in enumerate(CCASES) if c["step"] == 0.25 and c["name"].startswith("rng_")]
    sel += [CBY["repeat"]]  # another step in the fixture, 0.25 here: compared with its own single launch below
    assert len(sel) > 40 and len(sel) % 64
    lists = [CCASES[i]["points"] for i in sel]
    r = _host(batch.cubic_spline_batch(lists, 0.25, with_derivative=True), CKEYS)
    for q, i in enumerate(sel):
        s = _csingle(i) if CCASES[i]["step"] == 0.25 else _host(batch.cubic_spline_batch([lists[q]], 0.25, with_derivative=True), CKEYS)
        n = int(s["n_points"][0])
        assert int(r["n_points"][q]) == n and r["status"][q] == s["status"][0] and r["arc_length"][q] == s["arc_length"][0]
        assert np.array_equal(r["points"][q, :n], s["points"][0, :n], equal_nan=True), CCASES[i]["name"]
    # a cap below most counts: status 2 with the count reported and the first rows valid, then the retry
    counts = r["n_points"]
    cap = int(np.median(counts))
    o = _host(batch.cubic_spline_batch(lists, 0.25, point_cap=cap, retry_overflow=False, with_derivative=True), CKEYS)
    assert np.array_equal(o["n_points"], counts) and np.array_equal(o["status"] == 2, counts > cap) and (counts > cap).any()
    for q in range(len(sel)):
        m = min(int(counts[q]), cap)
        assert np.array_equal(o["points"][q, :m], r["points"][q, :m], equal_nan=True)
    f = _host(batch.cubic_spline_batch(lists, 0.25, point_cap=cap, with_derivative=True), CKEYS)
    assert not f["status"].any() and f["points"].shape[1] == counts.max()
    for q in range(len(sel)):
        assert np.array_equal(f["points"][q, : counts[q]], r["points"][q, : counts[q]], equal_nan=True)
    c = _host(batch.cubic_spline_batch(lists, 0.25, cost_only=True), CKEYS)
    assert c["points"] is None and np.array_equal(c["n_points"], counts) and np.array_equal(c["arc_length"], r["arc_length"])
    three = _host(batch.cubic_spline_batch(lists[:5], 0.25), CKEYS)
    assert three["points"].shape[2] == 3 and np.array_equal(three["points"][0, : counts[0]], r["points"][0, : counts[0], :3])


def test_cubic_class():
    from python_motion_planning_amd import CubicSpline

    c = CCASES[CBY["ex1_0.5"]]
    pts3 = [(float(x), float(y), 10.0) for x, y in c["points"]]
    gen = CubicSpline(0.5)
    out = gen.run(pts3)
    assert type(out) is tuple and len(out) == 3 and all(type(v) is list and len(v) == c["count"] for v in out)
    assert all(type(v) is float for v in out[0])
    rows = np.array(list(out) + [c["rows"][:, 3], c["rows"][:, 4]]).T
    assert C.cs_deviation(rows, c["rows"], C.scale_of(c["points"]))[0] <= CS_RTOL
    assert gen.run([tuple(p) for p in c["points"]]) == out
    both = gen.run_batch([pts3, [(0.0, 0.0), (3.0, 4.0)]])
    assert both[0] == out and len(both[1][0]) == 10
    with pytest.raises(ValueError):
        gen.run([(0.0, 0.0), (float("inf"), 1.0), (2.0, 2.0)])
    with pytest.raises(NotImplementedError):
        gen.run([(0.0, 0.0, 1.0, 2.0), (1.0, 1.0, 1.0, 2.0)])
    with pytest.raises(AssertionError):
        gen.run([(0.0, 0.0)])
    assert gen.generation((0, 0, 0), (1, 1, 1)) is None
