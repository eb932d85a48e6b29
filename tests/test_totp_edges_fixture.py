"""TimeOptimalTrajectory3D's edge fixture without a device: what each case of tests/golden/totp_edges.npz
(the reference's own runs, make_golden_totp_edges.py) is for, asserted again from the file, and the CPU
oracle (oracle/pmp_oracle.c, the arithmetic csrc/totp3d.hip shares) against every case."""
import numpy as np
import pytest

import totp_checks as C
from golden_io import seg

CASES = C.cases()
NAMES = list(CASES)
EX = ((2.0, 2.0, 1.5), (1.5, 1.5, 1.0), 0.05, 0.05)


def _rows(name):
    i, path, p, z = CASES[name]
    assert int(z["n_pts"][i]) == int(z["pts_off"][i + 1] - z["pts_off"][i]), name  # every row is stored
    return seg(z["pts"], z["pts_off"], i)


def _prof(name, k):
    i, _, _, z = CASES[name]
    return seg(z[k], z["prof_off"], i)


def _count_margin(name):
    """(total_time - the last repeated-sum time, whether total_time was appended), with the point count and
    the last rows checked against the sampling loop"""
    i, path, p, z = CASES[name]
    pts, T = _rows(name), float(z["total_time"][i])
    ts, appended = C.step_times(T, p[2])
    assert len(ts) + appended == len(pts) and pts[-1, 0] == T, name
    assert appended == bool(pts[-2, 0] + p[2] > T), name
    return T - ts[-1], appended


def test_fixture_holds_the_cases():
    want = ["piv_mid", "piv_last", "piv_run", "piv3_a", "piv3_b", "noswap_uneven", "walk60", "big", "tiny", "slow_axis",
            "fine", "stuck", "ns128", "ns129", "ns130", "np64k", "np64k1_appended", "np64k_exact", "yaw_wrap", "yaw_gap",
            "wp_limit"]
    assert NAMES == want
    path = {k: v[1] for k, v in CASES.items()}
    prm = {k: v[2] for k, v in CASES.items()}
    z = CASES["piv_mid"][3]
    # the spline solve's row exchanges
    for name, n, ex in (("piv_mid", 8, [3]), ("piv_last", 4, [1, 2]), ("piv_run", 6, [1, 2, 3, 4]), ("piv3_a", 3, [0]),
                        ("piv3_b", 3, []), ("noswap_uneven", 6, [])):
        assert len(path[name]) == n and C.exchanges(path[name]) == ex, name
    assert 0 < 3 < 8 - 2 and 2 == 4 - 2  # piv_mid's is interior, piv_last's second is the last row's
    assert np.diff(C.arc_lengths(path["piv3_a"]))[1] > 1.0 > np.diff(C.arc_lengths(path["piv3_b"]))[1]
    d = np.diff(C.arc_lengths(path["noswap_uneven"]))
    assert d.max() / d.min() > 1.5
    # every grid path of the older fixture: no exchange for n >= 4 (what this fixture adds)
    from golden_io import totp_cases

    assert not any(C.exchanges(p) for _, p, _, _ in totp_cases() if len(p) >= 4)
    # non-integer waypoints, scales, limits
    assert len(path["walk60"]) == 60 and not np.any(path["walk60"] == np.round(path["walk60"]))
    assert np.min(np.abs(path["big"])) >= 1e4 and prm["big"][3] == 2.0 and min(prm["big"][0]) >= 15.0
    assert C.arc_lengths(path["tiny"])[-1] < 5e-3 and len(_prof("tiny", "s_values")) == 100 and len(_rows("tiny")) == 3
    assert prm["slow_axis"][0][2] == 0.05 and prm["slow_axis"][1][2] == 0.02
    assert C.slow_axis_dominates(_rows("slow_axis"), prm["slow_axis"][0])
    assert prm["fine"][2] == prm["fine"][3] == 0.01
    for name in NAMES:
        if name not in ("big", "slow_axis", "fine", "np64k_exact"):
            assert prm[name] == EX, name
    # stuck: s_dot never leaves 0, no yaw, total_time = sum ds / 0.1
    for name in ("stuck", "np64k_exact"):
        sv, tot = _prof(name, "s_values"), 0.0
        for k in range(1, len(sv)):
            tot = tot + (sv[k] - sv[k - 1]) / 0.1
        assert _prof(name, "s_dot").max() == 0.0 and np.isnan(_rows(name)[:, 10]).all(), name
        assert tot == float(z["total_time"][CASES[name][0]]) and path[name][1][0] < path[name][0][0], name
    # the 64-wide rounds of the profiles
    for name, ns, n in (("ns128", 128, 2), ("ns129", 129, 3), ("ns130", 130, 2)):
        got, q = C.n_samples_of(path[name], prm[name][3])
        assert got == ns == len(_prof(name, "s_values")) and len(path[name]) == n, name
        assert 1e-6 < q - int(q) < 1 - 1e-6, (name, q)
    # ... and of the points; every count is clear of its rounding edge
    for name in ("np64k", "np64k1_appended", "ns128", "ns129", "ns130", "tiny"):
        gap, appended = _count_margin(name)
        T = float(z["total_time"][CASES[name][0]])
        assert appended and 1e-9 * T < gap < prm[name][2] - 1e-9 * T, (name, gap)
    assert len(_rows("np64k")) == 128 and len(_rows("np64k1_appended")) == 65
    gap, appended = _count_margin("np64k_exact")
    assert gap == 0.0 and not appended and len(_rows("np64k_exact")) == 128
    # yaw
    w = C.yaw_wraps(_rows("yaw_wrap"))
    p = path["yaw_wrap"]
    assert np.all(p[:, 2] == 0.0) and p[1][0] > p[0][0] and p[-1][0] < p[-2][0]
    assert w[0] == 256 and len(w) == 3 and all(k % 64 for k in w[1:]), w  # one on a round's first row, two inside
    yaw = _rows("yaw_wrap")[:, 10]
    assert all(np.pi - abs(yaw[k]) > 1e-3 and np.pi - abs(yaw[k - 1]) > 1e-3 for k in w)
    assert C.yaw_wraps(_rows("walk60")) and all(k % 64 for k in C.yaw_wraps(_rows("walk60")))
    nan = np.isnan(_rows("yaw_gap")[:, 10])
    edges = np.nonzero(np.diff(nan.astype(int)))[0] + 1
    inside = [(a, b) for a, b in zip(edges[:-1], edges[1:]) if nan[a] and not nan[a - 1] and not nan[b]]
    assert inside and inside[0][1] - inside[0][0] >= 3 and nan.any() and (~nan).any(), edges
    # the limit case
    n = len(path["wp_limit"])
    assert n == C.MAX_WAYPOINTS == 602 and C.lds_bytes(n) <= C.LDS_BYTES < C.lds_bytes(n + 1)
    assert 1000 <= len(_prof("wp_limit", "s_values")) <= 1400
    step = np.diff(C.arc_lengths(path["wp_limit"]))
    assert 0.05 < step.min() and step.max() < 0.16
    # evaluate(t): the clamped ends, three interior knots with an ulp either side, 77 times in all
    for name in ("piv_run", "walk60", "ns129", "yaw_wrap"):
        i = CASES[name][0]
        et, ep = seg(z["eval_t"], z["eval_off"], i), seg(z["eval_pts"], z["eval_off"], i)
        T, tp = float(z["total_time"][i]), _prof(name, "time")
        assert len(et) == len(ep) == 77 and len(et) > 64 and len(et) % 64
        assert et[:5].tolist() == [-1.0, 0.0, T, T + 1.0, float(np.nextafter(T, 0.0))]
        assert ep[:5, 0].tolist() == [0.0, 0.0, T, T, et[4]] and np.isnan(ep[:, 10:]).all()
        for j in range(3):
            k, lo, hi = et[5 + 3 * j: 8 + 3 * j]
            assert k in tp[1:-1] and lo == np.nextafter(k, -np.inf) and hi == np.nextafter(k, np.inf)
        assert np.all((et[14:] > 0.0) & (et[14:] < T))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_against_reference(name):
    """Counts and None pattern exact, values within 1e-11 of max(1, |ref|) (test_oracle.py's bound for the
    36 grid paths).  Prints the measured maximum."""
    i, path, p, z = CASES[name]
    o = C.oracle_run(path, p)
    n = int(o["n_points"])
    worst = C.compare(z, i, o["n_samples"], o, n, o["points"][:n], float(o["total_time"]), C.RTOL_ORACLE)
    print(f"{name}: oracle - reference {worst:.3g}")
    if name in ("stuck", "np64k_exact"):  # nothing but sums and quotients of the samples: to the bit
        assert float(o["total_time"]) == float(z["total_time"][i])
