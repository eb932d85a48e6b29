"""TimeOptimalTrajectory3D edge fixture (tests/golden/totp_edges.npz, made by make_golden_totp_edges.py):
the loader, the comparison rule (golden_io.totp_compare's: counts exact, None pattern exact, values
relative to max(1, |ref|)) with the measured maximum returned, and numpy restatements of what decides
which code of csrc/totp3d.hip a path runs: the row exchanges of spline_slopes' LU, the sample count and
the sampling loop's times."""
import numpy as np

from golden_io import load_npz, seg

RTOL_GPU = 1e-9      # the project's trajectory tolerance (golden_io.totp_compare)
RTOL_ORACLE = 1e-11  # tests/test_oracle.py's bound for the CPU oracle against the reference
PROFILES = ("s_values", "s_dot", "s_ddot", "time")
# the waypoint count of the one limit case: the largest max_waypoints pmp_totp3d_batch accepts,
# 8 (34 n - 12) bytes of LDS <= 160 KiB (arc n, coefficients 12 (n - 1), path and solve scratch 21 n doubles)
LDS_BYTES = 160 * 1024
MAX_WAYPOINTS = (LDS_BYTES // 8 + 12) // 34


def lds_bytes(n):
    return 8 * (34 * n - 12)


def cases():
    """name -> (i, path [n, 3], (vmax, amax, dt, res), fixture), in the fixture's order."""
    z = load_npz("totp_edges.npz")
    out = {}
    for i, name in enumerate(z["names"]):
        c = z["cons"][i]
        out[str(name)] = (i, seg(z["path"], z["path_off"], i), (tuple(c[0:3]), tuple(c[3:6]), float(c[6]), float(c[7])), z)
    return out


def arc_lengths(path):
    """_parameterize_path (time_optimal_trajectory.py:41-74): the running sum of the segment norms"""
    path = np.asarray(path, np.float64).reshape(-1, 3)
    arc = np.zeros(len(path))
    for i in range(1, len(path)):
        d = path[i] - path[i - 1]
        arc[i] = arc[i - 1] + np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return arc


def exchanges(path):
    """The elimination steps k at which spline_slopes (csrc/totp3d.hip) exchanges rows k and k + 1 (n >= 4,
    the banded LU: the sub-diagonal entry of row k + 1 against the diagonal of row k as the steps before left
    it) or rows k and p > k (n == 3, the dense solve).  The right-hand sides play no part, so the three
    axes of a path exchange alike.  n == 2 has no system."""
    x = arc_lengths(path)
    n = len(x)
    dx = np.diff(x)
    if n == 2:
        return []
    out = []
    if n == 3:
        A = np.array([[1.0, 1.0, 0.0], [dx[1], 2.0 * (dx[0] + dx[1]), dx[0]], [0.0, 1.0, 1.0]])
        for k in range(3):
            p = k + int(np.argmax(np.abs(A[k:, k])))  # the first of the largest, as the kernel's > keeps it
            if p != k:
                A[[k, p]] = A[[p, k]]
                out.append(k)
            for r in range(k + 1, 3):
                A[r, k + 1:] -= A[r, k] * (1.0 / A[k, k]) * A[k, k + 1:]
        return out
    D = np.zeros(n)
    U1 = np.zeros(n)
    U2 = np.zeros(n)
    D[1:-1] = 2.0 * (dx[:-1] + dx[1:])
    U1[1:-1] = dx[:-1]
    D[0], U1[0] = dx[1], x[2] - x[0]
    D[-1] = dx[-2]
    last = x[-1] - x[-3]  # the last row's sub-diagonal entry
    for k in range(n - 1):
        low = last if k + 1 == n - 1 else dx[k + 1]
        if abs(low) > abs(D[k]):
            out.append(k)
            low, D[k], D[k + 1], U1[k], U1[k + 1], U2[k] = D[k], low, U1[k], D[k + 1], U2[k], U1[k + 1]
        m = low * (1.0 / D[k])
        D[k + 1] -= m * U1[k]
        if k + 2 < n:
            U1[k + 1] -= m * U2[k]
    return out


def n_samples_of(path, res):
    """(max(int(L / res), 100), L / res): the sample count and the quotient it truncates"""
    q = arc_lengths(path)[-1] / res
    return max(int(q), 100), q


def step_times(total, dt):
    """generate()'s loop (:293-301): (the repeated-sum times <= total_time, whether total_time is appended)"""
    ts = []
    t = 0.0
    while t <= total:
        ts.append(t)
        t += dt
    return ts, ts[-1] < total


def slow_axis_dominates(pts, vmax):
    """The z velocity peaks within 5 % of its limit (the linear interpolation between samples overshoots it a
    little) while x and y stay below half of theirs"""
    peak = np.max(np.abs(np.asarray(pts)[:, 4:7]), axis=0) / np.asarray(vmax)
    return bool(0.95 < peak[2] < 1.05 and peak[0] < 0.5 and peak[1] < 0.5)


def yaw_wraps(pts):
    """Rows k whose yaw and row k - 1's both exist and differ by more than pi"""
    y = np.asarray(pts)[:, 10]
    with np.errstate(invalid="ignore"):
        return (np.nonzero(np.abs(np.diff(y)) > np.pi)[0] + 1).tolist()


def max_err(a, b, what):
    """totp_compare's closeness without the bound: shape and NaN pattern exact; returns the largest
    |a - b| / max(1, |b|)"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert (np.isnan(a) == np.isnan(b)).all(), what
    m = ~np.isnan(b)
    err = np.abs(a[m] - b[m]) / np.maximum(1.0, np.abs(b[m]))
    return float(err.max()) if err.size else 0.0


def compare(z, i, n_samples, prof, n_points, pts, total_time, rtol):
    """One trajectory against fixture case i under golden_io.totp_compare's rule at rtol; returns the
    largest difference seen (asserted <= rtol)."""
    po, pto = z["prof_off"], z["pts_off"]
    ns = int(po[i + 1] - po[i])
    assert int(n_samples) == ns, (int(n_samples), ns)
    assert int(n_points) == int(z["n_pts"][i]), (int(n_points), int(z["n_pts"][i]))
    worst = 0.0
    for k in PROFILES:
        worst = max(worst, max_err(np.asarray(prof[k])[:ns], z[k][po[i]:po[i + 1]], f"case {i} {k}"))
    idx = z["pts_idx"][pto[i]:pto[i + 1]]
    worst = max(worst, max_err(np.asarray(pts)[idx], z["pts"][pto[i]:pto[i + 1]], f"case {i} points"))
    worst = max(worst, max_err([total_time], [z["total_time"][i]], f"case {i} total_time"))
    assert worst <= rtol, (i, worst)
    return worst


def compare_runs(a, b, rtol):
    """Two runs of one path (dicts of host arrays: the four profiles, n_samples, points, n_points,
    total_time), b the reference of the two, under the same rule; returns the largest difference."""
    ns, n = int(b["n_samples"]), int(b["n_points"])
    assert int(a["n_samples"]) == ns and int(a["n_points"]) == n
    worst = max_err([a["total_time"]], [b["total_time"]], "total_time")
    for k in PROFILES:
        worst = max(worst, max_err(a[k][:ns], b[k][:ns], k))
    worst = max(worst, max_err(a["points"][:n], b["points"][:n], "points"))
    assert worst <= rtol, worst
    return worst


def oracle_run(path, p):
    """The CPU oracle's run of one path as compare_runs takes it"""
    from oracle import oracle as O

    r = O.totp3d_batch([path], O.TotpParams.make(*p))
    assert int(r["status"][0]) == 0
    return {k: (v[0] if np.ndim(v) else v) for k, v in r.items()}


def same_bits(a, b):
    a = np.asarray(a)
    b = np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan], b[~nan])
