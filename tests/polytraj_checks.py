"""PolynomialTrajectory3D fixture (tests/golden/polytraj.npz, made by make_golden_polytraj.py): the
loader, the comparison rules and a sequential Python restatement of the arithmetic of
csrc/polytraj3d.hip (the reference's operation order, trajectory/polynomial_trajectory.py:52-286 and
trajectory_base.py:193-216, :245-261, in plain IEEE doubles)."""
import math
from fractions import Fraction

import numpy as np

from golden_io import load_npz, seg

NAN = float("nan")
RTOL = 1e-9      # rows: relative to max(1, |ref|), the project's trajectory tolerance (golden_io.totp_compare)
RTOL_T = 1e-12   # times / segment_times of non-integer waypoints (integer waypoints: bit-equal)


def fma(a, b, c):
    """a * b + c with one rounding"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def cases():
    """Yield (i, name, path [n, 3], (vmax, amax, dt), bc [4, 3] or None, fixture)."""
    z = load_npz("polytraj.npz")
    for i, name in enumerate(z["names"]):
        c = z["cons"][i]
        bc = z["bc"][i]
        yield (i, str(name), seg(z["path"], z["path_off"], i), (tuple(c[0:3]), tuple(c[3:6]), float(c[6])),
               bc if np.any(bc != 0.0) else None, z)


def is_integer_case(path):
    return bool(np.all(path == np.round(path)))


def segment_times(path, vmax, amax):
    """_compute_segment_times (:89-111)"""
    out = []
    vavg = min(vmax) * 0.7
    am = min(amax)
    for i in range(len(path) - 1):
        a, b, c = (path[i + 1][d] - path[i][d] for d in range(3))
        dist = math.sqrt((a * a + b * b) + c * c)
        est = dist / vavg if vavg > 0 else 1.0
        out.append(max(est, 2.0 * math.sqrt(dist / am), 0.5))
    return out


class Poly:
    """One path's segments: times, running start times, waypoint velocities; evaluate(t) computes the
    quintic coefficients of the segment it lands in (the kernel stores none)."""

    def __init__(self, path, vmax, amax, bc=None):
        self.P = [[float(v) for v in p] for p in path]
        n = len(self.P)
        if n < 2:
            raise ValueError("Need at least 2 waypoints for trajectory generation")
        self.bc = [[0.0] * 3 for _ in range(4)] if bc is None else [[float(v) for v in r] for r in bc]
        self.T = segment_times(self.P, vmax, amax)
        self.S = [0.0]  # S[i] = start of segment i; S[i + 1] = S[i] + T[i] is also its end (:203-232, :266)
        for t in self.T:
            self.S.append(self.S[-1] + t)
        self.total = self.S[-1]  # sum(segment_times): the same left-to-right sum
        self.V = [self.bc[0]]
        for i in range(1, n - 1):  # :162-187
            den = self.T[i] + self.T[i - 1]
            self.V.append([min(max((self.P[i + 1][d] - self.P[i - 1][d]) / den, -vmax[d]), vmax[d]) for d in range(3)])
        self.V.append(self.bc[1])

    def evaluate(self, t, total=None):
        """evaluate(t) (:253-286) -> the 13 leading columns of a row"""
        total = self.total if total is None else total
        t = min(max(t, 0.0), total)
        ns = len(self.T)
        lo, hi = 0, ns  # first i with t <= S[i + 1]
        while lo < hi:
            mid = (lo + hi) // 2
            if t <= self.S[mid + 1]:
                hi = mid
            else:
                lo = mid + 1
        if lo == ns:
            i, u = ns - 1, self.T[ns - 1]
        else:
            i, u = lo, t - self.S[lo]
        T = self.T[i]
        u = min(max(u, 0.0), T)
        T2 = T * T
        T3 = T2 * T
        T4 = T3 * T
        T5 = T4 * T
        # u ** k is libm's pow, correctly rounded (the kernel: a double-double product chain)
        u2, u3, u4, u5 = u * u, math.pow(u, 3), math.pow(u, 4), math.pow(u, 5)
        row = [t] + [0.0] * 12
        for d in range(3):
            p0, p1, v0, v1 = self.P[i][d], self.P[i + 1][d], self.V[i][d], self.V[i + 1][d]
            a0 = self.bc[2][d] if i == 0 else 0.0
            a1 = self.bc[3][d] if i == ns - 1 else 0.0
            c2 = a0 / 2.0
            c3 = (((20 * p1 - 20 * p0) - (8 * v1 + 12 * v0) * T) - (3 * a0 - a1) * T2) / (2 * T3)
            c4 = (((30 * p0 - 30 * p1) + (14 * v1 + 16 * v0) * T) + (3 * a0 - 2 * a1) * T2) / (2 * T4)
            c5 = (((12 * p1 - 12 * p0) - (6 * v1 + 6 * v0) * T) - (a0 - a1) * T2) / (2 * T5)
            # coeffs @ vec as the reference's BLAS sums six products (the fixture shows this order and the
            # fused tail): ((x0 + x2) + (x1 + x3)) + fma(c4, w4, c5 w5); products by 0 dropped
            row[1 + d] = ((p0 + c2 * u2) + (v0 * u + c3 * u3)) + fma(c4, u4, c5 * u5)
            row[4 + d] = (c2 * (2 * u) + (v0 + c3 * (3 * u2))) + fma(c4, 4 * u3, c5 * (5 * u4))
            row[7 + d] = (c2 * 2 + c3 * (6 * u)) + fma(c4, 12 * u2, c5 * (20 * u3))
            row[10 + d] = c3 * 6 + fma(c4, 24 * u, c5 * (60 * u2))
        return row


def sample_times(total, dt):
    """generate()'s / resample()'s times: the repeated sum, then total_time if the last is short of it"""
    ts = []
    t = 0.0
    while t <= total:
        ts.append(t)
        t += dt
    if ts and ts[-1] < total:
        ts.append(total)
    return ts


def restate(path, vmax, amax, dt, bc=None, eval_t=None, sample_dt=None):
    """What pmp_polytraj3d_batch writes for one path: points [n, 15], total_time, segment_times."""
    pl = Poly(path, vmax, amax, bc)
    with_yaw = eval_t is None and sample_dt is None
    ts = list(eval_t) if eval_t is not None else sample_times(pl.total, dt if sample_dt is None else sample_dt)
    rows = [pl.evaluate(t) + [NAN, NAN] for t in ts]
    if with_yaw:  # compute_yaw_from_velocity (trajectory_base.py:245-261)
        for r in rows:
            if math.sqrt(r[4] * r[4] + r[5] * r[5]) > 1e-6:
                r[13] = math.atan2(r[5], r[4])
        for k in range(1, len(rows)):
            d = rows[k][0] - rows[k - 1][0]
            if d > 0 and not math.isnan(rows[k][13]) and not math.isnan(rows[k - 1][13]):
                dy = rows[k][13] - rows[k - 1][13]
                while dy > math.pi:
                    dy -= 2 * math.pi
                while dy < -math.pi:
                    dy += 2 * math.pi
                rows[k][14] = dy / d
    return dict(points=np.array(rows, np.float64).reshape(-1, 15), total_time=pl.total,
                segment_times=np.array(pl.T, np.float64))


def close(a, b, what, rtol=RTOL):
    """|a - b| <= rtol max(1, |b|) elementwise, the NaN (= None) pattern exact; returns bit equality"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert (np.isnan(a) == np.isnan(b)).all(), what
    m = ~np.isnan(b)
    err = np.abs(a[m] - b[m]) / np.maximum(1.0, np.abs(b[m]))
    assert err.size == 0 or err.max() <= rtol, (what, float(err.max()))
    return bool(np.array_equal(a[m], b[m]))


def times_match(a, b, integer, what):
    """bit-equal for integer waypoints, else within RTOL_T relative"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if integer:
        assert np.array_equal(a, b), what
    else:
        assert np.all(np.abs(a - b) <= RTOL_T * np.abs(b)), what


def compare_case(z, i, path, points, total_time, seg_times):
    """One generated trajectory against fixture case i; returns True when every stored value is bit-equal."""
    integer = is_integer_case(path)
    points = np.asarray(points)
    assert len(points) == int(z["n_pts"][i]), (i, len(points), int(z["n_pts"][i]))
    times_match(seg_times, seg(z["seg_times"], z["seg_off"], i), integer, f"case {i} segment_times")
    times_match([total_time], [z["total_time"][i]], integer, f"case {i} total_time")
    times_match(points[:, 0], seg(z["times"], z["t_off"], i), integer, f"case {i} times")
    idx = seg(z["pts_idx"], z["pts_off"], i)
    return close(points[idx], seg(z["pts"], z["pts_off"], i), f"case {i} points")


def check_constraints(points, vmax, amax, max_jerk=None):
    """trajectory_base.py:150-190 on rows"""
    p = np.asarray(points)
    res = dict(velocity_satisfied=not np.any(np.max(np.abs(p[:, 4:7]), axis=0) > np.asarray(vmax)),
               acceleration_satisfied=not np.any(np.max(np.abs(p[:, 7:10]), axis=0) > np.asarray(amax)),
               jerk_satisfied=True)
    if max_jerk is not None and not np.any(np.isnan(max_jerk)):
        res["jerk_satisfied"] = not np.any(np.max(np.abs(p[:, 10:13]), axis=0) > np.asarray(max_jerk))
    return res


def optimize_state(points, seg_times, vmax, amax, dt, max_jerk=None):
    """segment_times / total_time after optimize_time_allocation (:288-330): every iteration's generate()
    recomputes the plain times, so the state is one scaling pass over the plain trajectory."""
    T = [float(t) for t in seg_times]
    if all(check_constraints(points, vmax, amax, max_jerk).values()):
        return T, sum(T)
    p = np.asarray(points)
    start = 0.0
    for i in range(len(T)):
        dur = float(seg_times[i])
        a = int(start / dt)
        b = min(int((start + dur) / dt), len(p) - 1)
        if b > a:
            r = max(np.max(np.abs(p[a:b + 1, 4:7]) / np.asarray(vmax)), np.max(np.abs(p[a:b + 1, 7:10]) / np.asarray(amax)))
            if r > 1.0:
                T[i] *= r ** 0.5
        start += dur
    return T, sum(T)
