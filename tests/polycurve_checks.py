"""Polynomial / Bezier fixture (tests/golden/polycurve.npz, made by make_golden_polycurve.py): the loader, the
comparison rules and a sequential Python restatement of csrc/polycurve.hip's arithmetic (the reference's
operation order, curve_generation/polynomial_curve.py:43-164 and bezier_curve.py:34-89, in plain IEEE doubles:
powers as repeated multiplication, the 3 x 3 solve by the kernel's elimination with partial pivoting where the
reference calls LAPACK).

Rules.  Polynomial: t_index, the count and the status are exact; T, time, x, y, v and the magnitudes of a and
jerk are within RTOL max(1, |ref|); yaw is compared through (v cos yaw, v sin yaw), because yaw is
ill-conditioned where v -> 0, and yaw[0] exactly where v[0] == 0; the signs of a and jerk only on the rows the
fixture marks safe (the difference they turn on is not itself rounding).  Bezier: the count and the status are
exact (a fragile case, whose hypot / step lies within 4 ulp of an integer, may differ by one and is then
compared with the restatement at that count); control points and x, y within RTOL max(1, |ref|).

The bound was measured, not assumed: the worst deviation of the restatement from the reference's rows over
the whole fixture (test_polycurve_fixture.py prints it per column) is
    time 0, x 1.42e-13, y 7.05e-14, yaw (as v cos, v sin) 5.22e-14, v 4.21e-14, a 1.13e-14, jerk 8.55e-15, T 0;
    Bezier x 4.62e-16, y 1.11e-15, control 0
(the quintic's coefficients come out of a system whose condition grows with T^5; the Bezier sum differs from
the reference only by pow() against repeated multiplication).  16 times the worst, 2.3e-12, rounded up to a
power of ten: RTOL = 1e-11, six orders inside the project's 1e-5 contract; the factor allows for the one-ulp
differences of the device's hypot / atan2 / sin / cos and for FMA contraction (which the build switches off)."""
import math

import numpy as np

from golden_io import load_npz, seg

RTOL = 1e-11
COLS = ("time", "x", "y", "yaw", "v", "a", "jerk")
INF = float("inf")


def load():
    return load_npz("polycurve.npz")


# ---- the restatement ---------------------------------------------------------------------------------------
def solve3(A, b):
    """Gaussian elimination with partial pivoting, the kernel's operations in its order"""
    A = [list(r) for r in A]
    b = list(b)
    for c in range(2):
        piv = c
        for r in range(c + 1, 3):
            if abs(A[r][c]) > abs(A[piv][c]):
                piv = r
        if piv != c:
            A[c], A[piv] = A[piv], A[c]
            b[c], b[piv] = b[piv], b[c]
        rcp = _div(1.0, A[c][c])
        for r in range(c + 1, 3):
            l = A[r][c] * rcp
            for j in range(c + 1, 3):
                A[r][j] = A[r][j] - l * A[c][j]
            b[r] = b[r] - l * b[c]
    x2 = _div(b[2], A[2][2])
    x1 = _div(b[1] - x2 * A[1][2], A[1][1])
    x0 = _div((b[0] - x2 * A[0][2]) - x1 * A[0][1], A[0][0])
    return x0, x1, x2


def _div(a, b):
    """IEEE division: no ZeroDivisionError"""
    return float(np.float64(a) / np.float64(b))


class Poly:
    """Poly (:39-75) with t ** n as repeated multiplication"""

    def __init__(self, state0, state1, t):
        x0, v0, a0 = state0
        xt, vt, at = state1
        t2 = t * t
        t3 = t2 * t
        t4 = t3 * t
        t5 = t4 * t
        A = [[t3, t4, t5], [3 * t2, 4 * t3, 5 * t4], [6 * t, 12 * t2, 20 * t3]]
        b = [xt - x0 - v0 * t - a0 * t2 / 2, vt - v0 - a0 * t, at - a0]
        self.p0, self.p1, self.p2 = x0, v0, a0 / 2.0
        self.p3, self.p4, self.p5 = solve3(A, b)

    def x(self, t):
        t2 = t * t
        t3 = t2 * t
        t4 = t3 * t
        return self.p0 + self.p1 * t + self.p2 * t2 + self.p3 * t3 + self.p4 * t4 + self.p5 * (t4 * t)

    def dx(self, t):
        t2 = t * t
        t3 = t2 * t
        return self.p1 + 2 * self.p2 * t + 3 * self.p3 * t2 + 4 * self.p4 * t3 + 5 * self.p5 * (t3 * t)

    def ddx(self, t):
        t2 = t * t
        return 2 * self.p2 + 6 * self.p3 * t + 12 * self.p4 * t2 + 20 * self.p5 * (t2 * t)

    def dddx(self, t):
        return 6 * self.p3 + 24 * self.p4 * t + 60 * self.p5 * (t * t)


def candidate_times(step, t_min, t_max):
    """np.arange(t_min, t_max, step) by its own rule: ceil((t_max - t_min) / step) values t_min + i delta with
    delta = (t_min + step) - t_min"""
    n = max(int(math.ceil((t_max - t_min) / step)), 0)
    delta = (t_min + step) - t_min
    return [t_min + i * delta for i in range(n)]


def sample_count(T, dt):
    return int(math.ceil((T + dt) / dt))


def hyp(a, b):
    return math.hypot(a, b)


def restate_polynomial(s, g, step, max_acc, max_jerk, dt=0.1, t_min=1.0, t_max=30.0):
    """What pmp_polycurve_batch writes for one pair: t_index, T, rows [n, 7], status."""
    sx, sy, syaw, sv, sa = (float(v) for v in s)
    gx, gy, gyaw, gv, ga = (float(v) for v in g)
    t_min, t_max, dt = float(t_min), float(t_max), float(dt)
    with np.errstate(all="ignore"):
        try:
            cs, sn, cg, sg = math.cos(syaw), math.sin(syaw), math.cos(gyaw), math.sin(gyaw)
        except ValueError:  # an infinite yaw: NaN on the device, and no candidate is feasible
            cs = sn = cg = sg = float("nan")
        for i, T in enumerate(candidate_times(step, t_min, t_max)):
            px = Poly((sx, sv * cs, sa * cs), (gx, gv * cg, ga * cg), T)
            py = Poly((sy, sv * sn, sa * sn), (gy, gv * sg, ga * sg), T)
            n = sample_count(T, dt)
            ok = True
            for k in range(n):
                t = k * dt
                if not (hyp(px.ddx(t), py.ddx(t)) <= max_acc and hyp(px.dddx(t), py.dddx(t)) <= max_jerk):
                    ok = False
                    break
            if not ok:
                continue
            rows = []
            for k in range(n):
                t = k * dt
                vx, vy = px.dx(t), py.dx(t)
                v = hyp(vx, vy)
                a = hyp(px.ddx(t), py.ddx(t))
                if rows and v - rows[-1][4] < 0.0:
                    a = -a
                j = hyp(px.dddx(t), py.dddx(t))
                if rows and a - rows[-1][5] < 0.0:
                    j = -j
                rows.append((t, px.x(t), py.x(t), math.atan2(vy, vx), v, a, j))
            return dict(t_index=i, T=T, rows=np.array(rows, np.float64).reshape(-1, 7), status=0)
    return dict(t_index=-1, T=INF, rows=np.zeros((0, 7)), status=1)


def control_points(s, g, offset):
    sx, sy, syaw = (float(v) for v in s)
    gx, gy, gyaw = (float(v) for v in g)
    dist = math.hypot(sx - gx, sy - gy) / offset
    return [(sx, sy), (sx + dist * math.cos(syaw), sy + dist * math.sin(syaw)),
            (gx - dist * math.cos(gyaw), gy - dist * math.sin(gyaw)), (gx, gy)]


def linspace01(n):
    """np.linspace(0, 1, n) by its own rule: i (1 / (n - 1)), the last exactly 1; a single value is 0"""
    if n == 1:
        return [0.0]
    step = 1.0 / (n - 1) if n > 1 else 0.0
    return [1.0 if i == n - 1 else i * step for i in range(n)]


def bezier_point(t, P):
    u = 1 - t
    t2, u2 = t * t, u * u
    b = ((1.0 * 1.0) * (u2 * u), (3.0 * t) * u2, (3.0 * t2) * u, (1.0 * (t2 * t)) * 1.0)
    return tuple(((b[0] * P[0][c] + b[1] * P[1][c]) + b[2] * P[2][c]) + b[3] * P[3][c] for c in (0, 1))


def restate_bezier(s, g, step, offset, force_count=None):
    """What pmp_bezier_batch writes for one pair: control [4, 2], rows [n, 2], status."""
    q = math.hypot(float(s[0]) - float(g[0]), float(s[1]) - float(g[1])) / step
    if not math.isfinite(q):
        return dict(control=np.full((4, 2), np.nan), rows=np.zeros((0, 2)), status=4)
    n = int(q) if force_count is None else int(force_count)
    P = control_points(s, g, offset)
    return dict(control=np.array(P, np.float64), rows=np.array([bezier_point(t, P) for t in linspace01(n)],
                                                               np.float64).reshape(-1, 2), status=0)


# ---- the cases ---------------------------------------------------------------------------------------------
def cases(z=None):
    """Yield (i, name, start, goal, params (step, max_acc, max_jerk, dt, t_min, t_max)) of every polynomial case."""
    z = load() if z is None else z
    for i, name in enumerate(z["names"]):
        yield i, str(name), tuple(z["start"][i]), tuple(z["goal"][i]), tuple(float(v) for v in z["params"][i])


def bezier_cases(z=None):
    """Yield (i, name, start, goal, (step, offset)) of every Bezier case."""
    z = load() if z is None else z
    for i, name in enumerate(z["b_names"]):
        yield i, str(name), tuple(z["b_start"][i]), tuple(z["b_goal"][i]), tuple(float(v) for v in z["b_params"][i])


# ---- the rules ---------------------------------------------------------------------------------------------
def close(a, b, what, rtol=RTOL):
    """|a - b| <= rtol max(1, |b|) elementwise, the NaN and inf patterns exact; returns the worst deviation"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    fin = np.isfinite(b)
    assert np.array_equal(a[~fin], b[~fin], equal_nan=True), what
    err = np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin]))
    worst = float(err.max()) if err.size else 0.0
    assert worst <= rtol, (what, worst)
    return worst


def _note(worst, k, v):
    if worst is not None:
        worst[k] = max(worst.get(k, 0.0), v)


def poly_rows_close(rows, ref, safe, what, worst=None):
    """rows [m, 7] against the reference's rows ref [m, 7] with their safe flags [m, 2], under the rules of
    this module; worst: a dict of the worst deviation per column, updated"""
    rows, ref = np.asarray(rows, np.float64).reshape(-1, 7), np.asarray(ref, np.float64).reshape(-1, 7)
    assert rows.shape == ref.shape, (what, rows.shape, ref.shape)
    for c, k in ((0, "time"), (1, "x"), (2, "y"), (4, "v")):
        _note(worst, k, close(rows[:, c], ref[:, c], f"{what} {k}"))
    v = ref[:, 4]
    e = max(close(rows[:, 4] * np.cos(rows[:, 3]), v * np.cos(ref[:, 3]), what + " v cos yaw"),
            close(rows[:, 4] * np.sin(rows[:, 3]), v * np.sin(ref[:, 3]), what + " v sin yaw"))
    _note(worst, "yaw", e)
    for c, k in ((5, "a"), (6, "jerk")):
        _note(worst, k, close(np.abs(rows[:, c]), np.abs(ref[:, c]), f"{what} |{k}|"))
        ok = np.asarray(safe, bool)[:, c - 5]  # the signed values there: a wrong sign of a value that is not
        close(rows[ok, c], ref[ok, c], f"{what} signed {k}")  # itself rounding noise is a deviation of 2 |value|


def compare_polynomial(z, i, t_index, T, n_points, rows, status, worst=None):
    """One computed pair (the device's, or the restatement's) against polynomial case i.  rows: all n_points
    rows [n_points, 7]."""
    name = str(z["names"][i])
    assert int(t_index) == int(z["t_index"][i]), (name, int(t_index), int(z["t_index"][i]))
    assert int(n_points) == int(z["count"][i]), (name, int(n_points), int(z["count"][i]))
    assert int(status) == (1 if int(z["t_index"][i]) < 0 else 0), (name, status)
    _note(worst, "T", close(T, z["T"][i], name + " T"))
    rows = np.asarray(rows, np.float64).reshape(-1, 7)
    assert len(rows) == int(n_points), name
    idx = seg(z["rows_idx"], z["rows_off"], i)
    ref = seg(z["rows"], z["rows_off"], i)
    poly_rows_close(rows[idx], ref, seg(z["rows_safe"], z["rows_off"], i), name, worst)
    if len(ref) and idx[0] == 0 and ref[0, 4] == 0.0:  # yaw[0] of a start at rest: the signed zeros of dx(0)
        assert rows[0, 3] == ref[0, 3] and math.copysign(1.0, rows[0, 3]) == math.copysign(1.0, ref[0, 3]), name


def compare_bezier(z, i, control, n_points, rows, status, worst=None):
    """One computed pair against Bezier case i.  rows: all n_points rows [n_points, 2].  Returns True where
    a fragile case took the other count."""
    name = str(z["b_names"][i])
    assert int(status) == 0, (name, status)
    rows = np.asarray(rows, np.float64).reshape(-1, 2)
    n, want = int(n_points), int(z["b_count"][i])
    assert len(rows) == n, name
    _note(worst, "control", close(control, z["b_control"][i], name + " control"))
    if n != want:
        assert z["b_fragile"][i] and abs(n - want) == 1, (name, n, want)
        s, g, (step, offset) = tuple(z["b_start"][i]), tuple(z["b_goal"][i]), z["b_params"][i]
        ref = restate_bezier(s, g, float(step), float(offset), force_count=n)["rows"]
        close(rows, ref, name + " rows at the other count")
        return True
    idx = seg(z["b_rows_idx"], z["b_rows_off"], i)
    ref = seg(z["b_rows"], z["b_rows_off"], i)
    for c, k in ((0, "x"), (1, "y")):
        _note(worst, "bezier " + k, close(rows[idx, c], ref[:, c], f"{name} {k}"))
    return False
