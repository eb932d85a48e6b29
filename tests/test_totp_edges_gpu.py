"""TimeOptimalTrajectory3D on gfx950 (pmp_totp3d_batch) off the grid: the reference's own runs of
tests/golden/totp_edges.npz (make_golden_totp_edges.py) -- row exchanges in the spline solve, non-integer
waypoints at several scales, sample and point counts on the 64-wide rounds, yaw wraps and gaps, the largest
waypoint count -- under the rules of totp_checks.py; evaluate(t) at and around the ends of its ranges; the
caps and refusals of the C entry."""
import ctypes
import functools

import numpy as np
import pytest

import totp_checks as C
from golden_io import seg

pytestmark = pytest.mark.gpu

CASES = C.cases()
NAMES = list(CASES)
EX = CASES["piv_mid"][2]
# one launch, the 2- and 3-waypoint paths beside the 60-waypoint one (the LDS layout is sized by the longest)
MIXED = ["piv_mid", "ns128", "walk60", "piv3_a", "ns129", "piv_last", "piv_run", "piv3_b", "noswap_uneven", "tiny", "stuck",
         "ns130", "np64k", "np64k1_appended", "yaw_wrap", "yaw_gap"]
EVAL = ["piv_run", "walk60", "ns129", "yaw_wrap", "piv3_a", "np64k_exact"]
KEYS = C.PROFILES + ("n_samples", "points", "n_points", "total_time", "status")
SENTINEL = -7.25


def _prm(p):
    from python_motion_planning_amd import _lib

    return _lib.TotpParams.make(*p)


def _host(r, q=0):
    """Path q of a batch result as host arrays, the profiles and rows cut to their counts"""
    o = {k: r[k][q].cpu().numpy() for k in KEYS}
    ns, n = int(o["n_samples"]), int(o["n_points"])
    for k in C.PROFILES:
        o[k] = o[k][:ns]
    o["points"] = o["points"][: min(n, len(o["points"]))]
    return o


@functools.lru_cache(maxsize=None)
def _single(name):
    from python_motion_planning_amd import batch

    _, path, p, _ = CASES[name]
    return _host(batch.totp3d_batch([path], _prm(p)))


def _same_run(a, b):
    return (int(a["status"]) == int(b["status"]) and int(a["n_samples"]) == int(b["n_samples"])
            and int(a["n_points"]) == int(b["n_points"]) and float(a["total_time"]) == float(b["total_time"])
            and all(np.array_equal(a[k], b[k]) for k in C.PROFILES) and C.same_bits(a["points"], b["points"]))


@pytest.mark.parametrize("name", NAMES)
def test_kernel_against_reference_and_oracle(name):
    """Every case alone: counts and None pattern exact, values within 1e-9 of max(1, |ref|), against the
    reference's run and against the CPU oracle on the same input.  Prints both measured maxima."""
    i, path, p, z = CASES[name]
    r = _single(name)
    assert int(r["status"]) == 0
    ref = C.compare(z, i, r["n_samples"], r, r["n_points"], r["points"], float(r["total_time"]), C.RTOL_GPU)
    orc = C.compare_runs(r, C.oracle_run(path, p), C.RTOL_GPU)
    print(f"{name}: kernel - reference {ref:.3g}, kernel - oracle {orc:.3g}")
    if name in ("stuck", "np64k_exact"):  # sums and quotients of the samples alone: to the bit
        assert float(r["total_time"]) == float(z["total_time"][i])


def test_mixed_launch_equals_single_runs():
    """The cases of the example's parameter set in one launch: rows, profiles and counts bit-equal to the
    single-path calls."""
    from python_motion_planning_amd import batch

    assert all(CASES[n][2] == EX for n in MIXED) and set(MIXED) == {n for n in NAMES if CASES[n][2] == EX} - {"wp_limit"}
    lens = [len(CASES[n][1]) for n in MIXED]
    k = lens.index(60)
    assert lens[k - 1] == 2 and lens[k + 1] == 3 and max(lens) == 60
    r = batch.totp3d_batch([CASES[n][1] for n in MIXED], _prm(EX))
    for q, name in enumerate(MIXED):
        assert _same_run(_host(r, q), _single(name)), name


@pytest.mark.parametrize("name", EVAL)
def test_evaluate_against_reference(name):
    """evaluate(t) below 0, at 0, at and beyond total_time, an ulp below it, on three time_profile knots and
    an ulp either side of each, and at 63 interior times: 77 in one call (a full round and a part)."""
    from python_motion_planning_amd import batch

    i, path, p, z = CASES[name]
    et, want = seg(z["eval_t"], z["eval_off"], i), seg(z["eval_pts"], z["eval_off"], i)
    r = _host(batch.totp3d_batch([path], _prm(p), eval_t=et))
    assert int(r["status"]) == 0 and int(r["n_points"]) == len(et) == 77
    got = r["points"]
    assert np.isnan(got[:, 10:]).all()
    T = float(r["total_time"])
    # clamped as the reference clamps, to the kernel's own total_time (an ulp from the reference's on some paths)
    assert np.array_equal(got[:, 0], np.clip(et, 0.0, T)) and got[0, 0] == 0.0 and got[3, 0] == T
    err = C.max_err(got, want, f"{name} evaluate")
    print(f"{name}: evaluate, kernel - reference {err:.3g}")
    assert err <= C.RTOL_GPU


def test_evaluate_batch_equals_single_calls():
    from python_motion_planning_amd import batch

    names = ["ns129", "walk60", "piv3_a"]
    i, _, _, z = CASES["walk60"]
    et = seg(z["eval_t"], z["eval_off"], i)  # beyond the shorter trajectories' total_time for some
    r = batch.totp3d_batch([CASES[n][1] for n in names], _prm(EX), eval_t=et)
    for q, n in enumerate(names):
        s = batch.totp3d_batch([CASES[n][1]], _prm(EX), eval_t=et)
        assert _same_run(_host(r, q), _host(s)), n
        assert int(r["n_points"][q]) == 77


def test_dropin_evaluate_clamps():
    """TimeOptimalTrajectory3D.evaluate(t) outside [0, total_time] is the end point, with the clamped time."""
    from python_motion_planning_amd.trajectory import TimeOptimalTrajectory3D, TrajectoryConstraints

    i, path, p, z = CASES["piv_run"]
    tr = TimeOptimalTrajectory3D([tuple(v) for v in path], TrajectoryConstraints(np.array(p[0]), np.array(p[1]), min_time_step=p[2]),
                                 path_resolution=p[3])
    pts = tr.generate()
    want = seg(z["eval_pts"], z["eval_off"], i)
    lo, hi = tr.evaluate(-1.0), tr.evaluate(tr.total_time + 1.0)
    assert lo.time == 0.0 and hi.time == tr.total_time and lo.yaw is None and hi.yaw_rate is None
    assert np.array_equal(lo.position, pts[0].position) and np.array_equal(hi.position, pts[-1].position)
    for e, w in ((lo, want[0]), (hi, want[3])):
        row = np.concatenate([[e.time], e.position, e.velocity, e.acceleration])
        assert C.max_err(row, w[:10], "drop-in evaluate") <= C.RTOL_GPU


def _raw(paths, p, max_waypoints, sample_cap, point_cap):
    """pmp_totp3d_batch called directly, every output buffer prefilled with SENTINEL (-1 for the integers)"""
    import torch

    from python_motion_planning_amd import _lib

    L, ctx = _lib.load_library(), _lib.context()
    nq = len(paths)
    off = np.zeros(nq + 1, np.int32)
    off[1:] = np.cumsum([len(a) for a in paths])
    flat = torch.as_tensor(np.concatenate(paths), device="cuda")
    off_d = torch.as_tensor(off, device="cuda")
    f = lambda *s: torch.full(s, SENTINEL, dtype=torch.float64, device="cuda")  # noqa: E731
    n = lambda: torch.full((nq,), -1, dtype=torch.int32, device="cuda")  # noqa: E731
    o = dict(s_values=f(nq, sample_cap), s_dot=f(nq, sample_cap), s_ddot=f(nq, sample_cap), time=f(nq, sample_cap),
             n_samples=n(), points=f(nq, point_cap, 12), n_points=n(), total_time=f(nq), status=n())
    prm = _prm(p)
    rc = L.pmp_totp3d_batch(ctx, _lib.stream_ptr(), ctypes.byref(prm), nq, flat.data_ptr(), off_d.data_ptr(), max_waypoints,
                            sample_cap, o["s_values"].data_ptr(), o["s_dot"].data_ptr(), o["s_ddot"].data_ptr(),
                            o["time"].data_ptr(), o["n_samples"].data_ptr(), point_cap, o["points"].data_ptr(),
                            o["n_points"].data_ptr(), o["total_time"].data_ptr(), o["status"].data_ptr(), None, 0)
    _lib.check(ctx, rc, "pmp_totp3d_batch")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _raw_equals_single(o, q, name):
    s = _single(name)
    ns, n = int(s["n_samples"]), int(s["n_points"])
    assert int(o["status"][q]) == 0 and int(o["n_samples"][q]) == ns and int(o["n_points"][q]) == n, name
    assert float(o["total_time"][q]) == float(s["total_time"]), name
    for k in C.PROFILES:
        assert np.array_equal(o[k][q, :ns], s[k]) and np.all(o[k][q, ns:] == SENTINEL), (name, k)
    assert C.same_bits(o["points"][q, :n], s["points"]) and np.all(o["points"][q, n:] == SENTINEL), name


def test_sample_cap_refuses_one_path():
    """sample_cap one below the middle path's n_samples: PMP_PATH_OVERFLOW for it with n_samples still
    reported, n_points 0 and none of its rows written; its neighbours as in an uncapped call."""
    names = ["piv3_a", "piv_run", "ns128"]
    ns = [int(_single(n)["n_samples"]) for n in names]
    npt = max(int(_single(n)["n_points"]) for n in names)
    assert ns[1] - 1 >= max(ns[0], ns[2])
    o = _raw([CASES[n][1] for n in names], EX, 6, ns[1] - 1, npt)
    assert o["status"].tolist() == [0, 2, 0] and int(o["n_samples"][1]) == ns[1] and int(o["n_points"][1]) == 0
    assert all(np.all(o[k][1] == SENTINEL) for k in C.PROFILES + ("points",))
    _raw_equals_single(o, 0, names[0])
    _raw_equals_single(o, 2, names[2])


def test_max_waypoints_refuses_one_path():
    """max_waypoints one below the longest path's count: PMP_CAP_OVERFLOW for it, the others unaffected."""
    names = ["piv3_a", "walk60", "ns128"]
    sc = max(int(_single(n)["n_samples"]) for n in names)
    npt = max(int(_single(n)["n_points"]) for n in names)
    o = _raw([CASES[n][1] for n in names], EX, 59, sc, npt)
    assert o["status"].tolist() == [0, 3, 0] and int(o["n_samples"][1]) == 0 and int(o["n_points"][1]) == 0
    assert all(np.all(o[k][1] == SENTINEL) for k in C.PROFILES + ("points",))
    _raw_equals_single(o, 0, names[0])
    _raw_equals_single(o, 2, names[2])
    full = _raw([CASES[n][1] for n in names], EX, 60, sc, npt)
    for q, n in enumerate(names):
        _raw_equals_single(full, q, n)


def test_waypoint_limit():
    """The largest max_waypoints follows from the entry's LDS formula, 8 (34 n - 12) <= 160 KiB: 602.  That
    count launches (the fixture's wp_limit, compared with the reference's run above); one more is refused with
    the number in the message."""
    from python_motion_planning_amd import _lib, batch

    _, path, p, _ = CASES["wp_limit"]
    assert len(path) == C.MAX_WAYPOINTS == 602
    assert int(_single("wp_limit")["status"]) == 0
    longer = np.vstack([path, path[-1] + (path[-1] - path[-2])])
    with pytest.raises(_lib.PMPError, match=r"max_waypoints too large for one CU's LDS \(<= 602\)"):
        batch.totp3d_batch([longer], _prm(p))


def test_appended_row_in_the_retried_tail():
    """np64k1_appended (65 points) with a first point_cap of 64: the appended total_time is the only row of the
    round that the retry delivers; the result is the uncapped one bit for bit."""
    from python_motion_planning_amd import batch

    _, path, p, _ = CASES["np64k1_appended"]
    r = batch.totp3d_batch([path], _prm(p), point_cap=64)
    assert r["points"].shape[1] == 65
    first = batch.totp3d_batch([path], _prm(p), point_cap=64, retry_overflow=False)
    assert int(first["status"][0]) == 2 and int(first["n_points"][0]) == 65
    assert _same_run(_host(r), _single("np64k1_appended"))
    assert C.same_bits(first["points"][0].cpu().numpy(), _single("np64k1_appended")["points"][:64])
