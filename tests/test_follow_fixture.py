"""PID / APF / RPP without a GPU: the sequential restatement of follow.hip's arithmetic
(follow_checks.run) reproduces every reference run of tests/golden/follow_plans.npz, the library
exports the entry point, and the drop-in classes have the reference's constructors."""
import inspect

import numpy as np
import pytest

import follow_checks as fc

CASES = list(fc.cases())
TOL = dict(rtol=1e-9, atol=1e-9)


def test_fixture_holds_the_issue_cases():
    got = sorted((c["name"], c["kind"]) for c in CASES)
    want = sorted([(n, k) for n in ("reach_a", "reach_b", "never", "cut") for k in fc.KINDS]
                  + [("engaged_a", "rpp"), ("engaged_b", "rpp"), ("raises", "rpp")])
    assert got == want
    by = {(c["name"], c["kind"]): c for c in CASES}
    assert [len(by[("reach_a", k)]["poses"]) for k in fc.KINDS] == [1157, 1074, 1049]
    assert [len(by[("reach_b", k)]["poses"]) for k in fc.KINDS] == [993, 894, 889]
    assert [len(by[(n, "rpp")]["poses"]) for n in ("engaged_a", "engaged_b")] == [1278, 958]
    assert by[("raises", "rpp")]["exc"] == "ZeroDivisionError"


def test_restatement_reproduces_every_fixture_case():
    grid = fc.readme_grid()
    exact = 0
    for c in CASES:
        kind = c["kind"]
        st0 = [*c["start"], 0.0, 0.0]
        r = fc.run(kind, c["path"], c["goal"], st0, c["max_iteration"], f=fc.follow_params(**c["over"]), grid=grid)
        assert r["status"] == fc.expected_status(c), c["id"]
        assert r["n_steps"] == len(c["poses"]), c["id"]
        assert np.array_equal(r["counters"], c["counters"]), (c["id"], r["counters"], c["counters"])
        np.testing.assert_allclose(r["poses"], c["poses"], err_msg=c["id"], **TOL)
        np.testing.assert_allclose(r["look"], c["look"], err_msg=c["id"], **TOL)
        np.testing.assert_allclose(r["state"], c["final"], err_msg=c["id"], **TOL)
        same = np.array_equal(r["poses"], c["poses"]) and np.array_equal(r["state"], c["final"])
        if kind == "pid":
            np.testing.assert_allclose(r["pid"], c["integrators"], err_msg=c["id"], **TOL)
            same = same and np.array_equal(r["pid"], c["integrators"])
        exact += int(same)
    print(f"follow restatement: {exact} of {len(CASES)} fixture cases bit-exact")


def test_window_scan_equals_all_obstacle_cells():
    """The window of cells the kernel scans holds every cell that matters: against the sum / minimum over
    all obstacle cells, at the grid's edges, outside it and for a negative coordinate."""
    grid = fc.readme_grid()
    for px, py in [(1.2, 1.3), (49.6, 29.5), (-0.4, 15.2), (25.5, 14.5), (60.0, 40.0), (-7.0, -3.0)]:
        for d in (0.6, 1.0, 2.5):
            w = fc.obstacle_term(grid, px, py, d, 1.0 / d, True)
            b = fc.obstacle_term(grid, px, py, d, 1.0 / d, True, brute=True)
            np.testing.assert_allclose(w[1:], b[1:], rtol=1e-12, atol=1e-15, err_msg=str((px, py, d)))
            wm = fc.obstacle_term(grid, px, py, d, 0.0, False)[0]
            bm = b[0]
            assert wm == bm if bm < d else wm >= d, (px, py, d, wm, bm)


def test_library_exports_and_binds_the_entry_point():
    from python_motion_planning_amd import _lib

    L = _lib.load_library()
    assert hasattr(L, "pmp_follow_step_batch")
    res, args = _lib.SIGNATURES["pmp_follow_step_batch"]
    assert len(args) == 22
    assert _lib.FOLLOW_KINDS == {"pid": 0, "apf": 1, "rpp": 2}
    f = _lib.FollowParams.make()
    assert {n: getattr(f, n) for n, _ in f._fields_} == fc.FOLLOW_DEFAULTS


@pytest.mark.parametrize("kind", fc.KINDS)
def test_classes_have_the_reference_constructors(kind):
    import python_motion_planning_amd as pmp

    z = fc.load_npz(fc.FIXTURE)
    cls = {"pid": pmp.PID, "apf": pmp.APF, "rpp": pmp.RPP}[kind]
    names, defaults = [], []
    for n, q in inspect.signature(cls.__init__).parameters.items():
        if n == "self":
            continue
        names.append(("**" if q.kind is q.VAR_KEYWORD else "") + n)
        d = q.default
        defaults.append(float(d) if isinstance(d, (int, float)) and not isinstance(d, bool) else float("nan"))
    assert names == [str(n) for n in z[f"ctor_{kind}_names"]]
    np.testing.assert_array_equal(np.array(defaults), z[f"ctor_{kind}_defaults"])
    strs = {c["kind"]: str(c["str"]) for c in CASES}
    assert cls.__str__(object.__new__(cls)) == strs[kind]
