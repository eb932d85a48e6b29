"""SplineTrajectory3D without a device: the sequential restatement of csrc/splinetraj3d.hip's arithmetic
(splinetraj_checks.py: knots by the fixed rule, banded collocation without pivoting, de Boor's recursion;
no scipy spline object) against the reference's own runs (tests/golden/splinetraj.npz, made by
make_golden_splinetraj.py), and the feature's exposure through the library and the package.

Measured: every stored value of the restatement is within 5e-12 of the reference's relative to
max(1, |ref|) (bound 1e-9), the worst column the yaw rate; counts and NaN patterns equal."""
import inspect

import numpy as np
import pytest

import splinetraj_checks as C
from golden_io import seg

CASES = list(C.cases())
NAMES = [c[1] for c in CASES]
COLS = ["t", "x", "y", "z", "vx", "vy", "vz", "ax", "ay", "az", "yaw", "yaw_rate"]


@pytest.fixture(scope="module")
def restated():
    """generate() of every case, computed once"""
    return {name: C.restate(path, vmax, amax, dt, deg) for _, name, path, (vmax, amax, dt), deg, _ in CASES}


def test_fixture_holds_the_cases():
    z = CASES[0][5]
    by = {c[1]: c[0] for c in CASES}
    n = {name: len(path) for _, name, path, _, _, _ in CASES}
    k = {name: int(z["k"][i]) for i, name, *_ in CASES}
    assert (n["a_three"], k["a_three"], int(z["degree"][by["a_three"]])) == (3, 2, 5)
    assert (n["b_four_k3"], k["b_four_k3"]) == (4, 3) and (n["c_six_k5"], k["c_six_k5"]) == (6, 5)
    assert (n["d_five_k3"], k["d_five_k3"]) == (5, 3) and (n["e_seven_k5"], k["e_seven_k5"]) == (7, 5)
    assert (n["f_six_k4"], k["f_six_k4"]) == (6, 4) and (n["g_five_k2"], k["g_five_k2"]) == (5, 2)
    assert n["m_walk64"] == 64 and n["n_walk65"] == 65
    for name in ("m_walk64", "n_walk65"):
        p = CASES[by[name]][2]
        assert len({tuple(r) for r in p}) == len(p) and np.all(np.abs(np.diff(p, axis=0)).max(axis=1) == 1)
    assert np.all(CASES[by["j_2d"]][2][:, 2] == 0.0)
    assert np.any(CASES[by["k_real"]][2] != np.round(CASES[by["k_real"]][2]))
    ch = np.linalg.norm(np.diff(CASES[by["l_anyangle"]][2], axis=0), axis=1)
    assert ch.min() == 1.0 and ch.max() > 11.0
    assert z["scale"][by["o_loose"]] == 1.0 and np.all(z["ratios"][by["o_loose"]] < 0.9)
    sc = z["scale"] != 1.0
    rv, ra = z["ratios"][:, 0], np.sqrt(z["ratios"][:, 1])
    assert np.any(sc & (rv > ra)) and np.any(sc & (rv < ra))
    npt = z["n_pts"]
    assert np.any(npt < 64) and np.any((npt >= 64) & (npt <= 128)) and np.any(npt > 1000)


def test_restatement_reproduces_reference(restated):
    """Counts and the NaN pattern exact; times and total_time within 1e-12 relative; rows within 1e-9 of
    max(1, |ref|).  Prints the largest error per column."""
    worst = np.zeros(12)
    for i, name, path, _, _, z in CASES:
        r = restated[name]
        worst = np.maximum(worst, C.compare_case(z, i, r["points"], r["total_time"]))
        C.times_match([r["T0"]], [z["total_time_unscaled"][i]], f"{name} unscaled total_time")
        assert (r["scale"] == 1.0) == (z["scale"][i] == 1.0), name
        C.close(list(r["ratios"]) + [r["scale"]], list(z["ratios"][i]) + [z["scale"][i]], f"{name} ratios")
    print("largest error per column:", ", ".join(f"{c} {e:.1e}" for c, e in zip(COLS, worst)))


def test_restatement_knots_and_coefficients(restated):
    """u_waypoints within 1e-12, the knots bit-equal to FITPACK's, the coefficients within 1e-9"""
    worst = 0.0
    for i, name, path, _, _, z in CASES:
        r = restated[name]
        C.times_match(r["u"], seg(z["u_waypoints"], z["path_off"], i), f"{name} u_waypoints")
        kn = seg(z["knots"], z["knot_off"], i)
        assert int(z["k"][i]) == r["k"] and len(kn) == len(path) + r["k"] + 1
        # the fixture's knots are FITPACK's; the rule on the fixture's u must give them bit for bit
        assert np.array_equal(np.array(C.knots_rule(list(seg(z["u_waypoints"], z["path_off"], i)), r["k"])), kn), name
        C.times_match(r["knots"], kn, f"{name} knots")
        worst = max(worst, float(np.max(C.close(r["coef"], z["coef"][:, z["path_off"][i]:z["path_off"][i + 1]],
                                                f"{name} coefficients"))))
    print(f"largest coefficient error: {worst:.1e}")


def test_restatement_check_constraints(restated):
    skipped = 0
    for i, name, path, (vmax, amax, dt), _, z in CASES:
        skipped += C.compare_checks(z, i, C.check_constraints(restated[name]["points"], vmax, amax))
    print("flags decided by the reference's own rounding (skipped):", skipped)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_evaluate(name):
    """evaluate(t) below 0, above total_time, at total_time / 3, 0 and total_time"""
    i, _, path, (vmax, amax, dt), deg, z = CASES[NAMES.index(name)]
    r = C.restate(path, vmax, amax, dt, deg, eval_t=z["eval_t"][i])
    assert np.isnan(r["points"][:, 10:]).all()
    C.close(r["points"], z["eval_pts"][i], f"{name} evaluate")
    C.times_match(r["points"][:, 0], z["eval_pts"][i][:, 0], f"{name} evaluate times")


def test_restatement_resample_and_constant_speed():
    z = CASES[0][5]
    i, name, path, (vmax, amax, dt), deg, _ = CASES[int(z["rs_case"])]
    r = C.restate(path, vmax, amax, dt, deg, sample_dt=float(z["rs_dt"]))
    C.times_match(r["points"][:, 0], z["rs_pts"][:, 0], "resample times")
    C.close(r["points"], z["rs_pts"], "resample")
    r = C.restate(path, vmax, amax, dt, deg, constant_speed=True)
    C.times_match([r["total_time"]], [z["cs_total"]], "constant-speed total_time")
    C.times_match(r["points"][:, 0], z["cs_pts"][:, 0], "constant-speed times")
    C.close(r["points"], z["cs_pts"], "constant speed")
    assert np.isnan(r["points"][:, 10:]).all() and np.all(r["points"][:, 7:10] == 0.0)


def test_restatement_refuses_what_the_reference_raises_on():
    for path, deg in (([(0, 0, 0), (1, 1, 0)], 5), ([(0, 0, 0), (1, 1, 0), (2, 1, 1)], 1),
                      ([(0, 0, 0), (1, 1, 0), (1, 1, 0), (2, 1, 1)], 3)):
        with pytest.raises(ValueError):
            C.restate(np.array(path, float), (2.0,) * 3, (1.0,) * 3, 0.01, deg)


# ---- exposure: each of these fails without the feature --------------------------------------------------
def test_signature_registered_and_symbol_built():
    from python_motion_planning_amd import _lib, batch

    assert len(_lib.SIGNATURES["pmp_splinetraj3d_batch"][1]) == 22
    L = _lib.load_library()
    assert hasattr(L, "pmp_splinetraj3d_batch") and L.pmp_splinetraj3d_max_waypoints() >= 480
    assert callable(batch.splinetraj3d_batch)
    p = _lib.SplineTrajParams.make()
    assert list(p.max_velocity) == [2.0] * 3 and list(p.max_acceleration) == [1.0] * 3
    assert p.min_time_step == 0.01 and p.spline_degree == 5


def test_class_is_exported_with_the_reference_signature():
    import python_motion_planning_amd as pmp

    assert "SplineTrajectory3D" in pmp.__all__
    sig = inspect.signature(pmp.SplineTrajectory3D.__init__)
    assert list(sig.parameters) == ["self", "path", "constraints", "spline_degree", "smoothing_factor"]
    assert [sig.parameters[k].default for k in ("constraints", "spline_degree", "smoothing_factor")] == [None, 5, 0.0]
    tr = pmp.SplineTrajectory3D([(0, 0), (3, 4), (6, 4)])
    assert tr.path.tolist() == [[0, 0, 0], [3, 4, 0], [6, 4, 0]] and tr.get_path_length() == 8.0
    assert tr.spline_degree == 2 and tr.smoothing_factor == 0.0 and tr.u_waypoints is None and tr.u_max == 1.0
    assert tr.trajectory_points == [] and tr.total_time == 0.0
    assert list(tr.constraints.max_velocity) == [2.0] * 3 and tr.constraints.min_time_step == 0.01
    assert pmp.SplineTrajectory3D([(0, 0, 0)] * 9, spline_degree=3).spline_degree == 3
    for m in ("generate", "evaluate", "resample", "reparameterize_constant_speed", "check_constraints", "get_positions",
              "get_velocities", "get_accelerations", "get_times", "get_path_length"):
        assert callable(getattr(tr, m))


def test_errors_before_any_device_call(monkeypatch):
    """The empty path and smoothing_factor > 0 in the constructor; in generate() whatever the reference
    raises on or never returns from.  No device call is made: batch.splinetraj3d_batch is never entered."""
    from python_motion_planning_amd import SplineTrajectory3D, TrajectoryConstraints, batch

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(batch, "splinetraj3d_batch", no_device)
    with pytest.raises(ValueError):
        SplineTrajectory3D([])
    with pytest.raises(NotImplementedError):
        SplineTrajectory3D([(0, 0, 0), (1, 1, 0), (2, 1, 1)], smoothing_factor=0.1)
    good = [(0, 0, 0), (1, 1, 0), (2, 1, 1), (3, 3, 1)]
    ok = TrajectoryConstraints(np.array([2.0] * 3), np.array([1.0] * 3))
    bad = [
        ([(0, 0, 0), (1, 1, 0)], ok, 5),                           # 2 waypoints: k = 1, derivative(2) raises
        ([(0, 0, 0), (1, 1, 0), (1, 1, 0), (2, 1, 1)], ok, 3),     # a repeated waypoint
        (good, ok, 0), ([(i, i * i % 5, i % 3) for i in range(8)], ok, 6),  # scipy: 1 <= k <= 5 (6 < n - 1 stays 6)
        (good, ok, 1),                                             # effective degree 1
        (good, TrajectoryConstraints(np.array([2.0, 0.0, 2.0]), np.array([1.0] * 3)), 3),
        (good, TrajectoryConstraints(np.array([2.0] * 3), np.array([1.0, 0.0, 1.0])), 3),
        (good, TrajectoryConstraints(np.array([2.0, np.inf, 2.0]), np.array([1.0] * 3)), 3),
        (good, TrajectoryConstraints(np.array([2.0] * 3), np.array([1.0] * 3), min_time_step=0.0), 3),
    ]
    for path, cons, deg in bad:
        tr = SplineTrajectory3D(path, cons, spline_degree=deg)
        with pytest.raises(ValueError):
            tr.generate()
        with pytest.raises(ValueError):
            tr.evaluate(0.5)
