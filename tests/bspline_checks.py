"""BSpline / BSpline3D / CubicSpline fixture (tests/golden/bspline.npz, made by make_golden_bspline.py): the
loader, float64 restatements of csrc/bspline.hip's arithmetic on the host, and the comparison rules.

The restatements follow the reference (curve_generation/bspline_curve.py, bspline_curve3d.py, cubic_spline.py)
except where the kernel does: the basis values come from the triangular scheme over the k + 1 functions of a
span (the reference recurses over every function; the generator asserts that both give the same bits), the
linear systems are solved (np.linalg.solve; the kernel: banded elimination) where the reference inverts, and
the cubic spline's tridiagonal system goes through the Thomas algorithm.

Rules.  B-spline: status, n_control and the row count are exact; parameters, knots, control points, rows
and length are within RTOL max(1, max |coordinate| of the curve) (parameters and knots: max(1, .) = 1); NaN
patterns are equal.  Cubic spline: the count and the status are exact on every case that is not fragile; x
and y within CS_RTOL max(1, max |coordinate|); yaw as an angle difference, skipped where hypot(dx, dy) < 1e-9.

The tolerances are not chosen here: RTOL = 64 x the worst deviation of the restatement from the reference's
control points and rows over the fixture, computed by the generator and stored in the npz (bs_rtol, cs_rtol).
64 x: the device sums dot products of up to 64 terms in another order and differs by an ulp in pow, hypot and
atan2; each is amplified by at most the condition numbers the generator caps (1e3 for the collocation matrix,
1e4 for the normal equations)."""
import math

import numpy as np

from golden_io import load_npz, seg

PARAM_MODES = ("centripetal", "chord_length", "uniform_spaced")
SPLINE_MODES = ("interpolation", "approximation")
ST_OK, ST_LINALG, ST_INDEX = 0, 4, 5  # as the kernel's status; 5: the 2D class raises IndexError before any launch
NAN = float("nan")


def load():
    return load_npz("bspline.npz")


def bs_case(z, i):
    """Case i of the B-spline block as a dict"""
    dim = int(z["bs_dim"][i])
    c = dict(name=str(z["bs_names"][i]), dim=dim, k=int(z["bs_k"][i]), step=float(z["bs_step"][i]),
             param_mode=PARAM_MODES[int(z["bs_pm"][i])], spline_mode=SPLINE_MODES[int(z["bs_sm"][i])],
             three_d=bool(z["bs_3d"][i]), status=int(z["bs_status"][i]), n_control=int(z["bs_nc"][i]), T=int(z["bs_T"][i]),
             points=seg(z["bs_pts"], z["bs_pts_off"], i).reshape(-1, dim), params=seg(z["bs_params"], z["bs_par_off"], i),
             knot=seg(z["bs_knot"], z["bs_knot_off"], i), control=seg(z["bs_control"], z["bs_ctl_off"], i).reshape(-1, dim),
             rows=seg(z["bs_rows"], z["bs_rows_off"], i).reshape(-1, dim),
             rows_idx=seg(z["bs_rows_idx"], z["bs_idx_off"], i), length=float(z["bs_length"][i]),
             restate_dev=float(z["bs_restate_dev"][i]), cond=float(z["bs_cond"][i]))
    return c


def cs_case(z, i):
    return dict(name=str(z["cs_names"][i]), step=float(z["cs_step"][i]), status=int(z["cs_status"][i]),
                count=int(z["cs_count"][i]), fragile=bool(z["cs_fragile"][i]),
                points=seg(z["cs_pts"], z["cs_pts_off"], i).reshape(-1, 2),
                rows=seg(z["cs_rows"], z["cs_rows_off"], i).reshape(-1, 5), rows_idx=seg(z["cs_rows_idx"], z["cs_idx_off"], i),
                arc=float(z["cs_arc"][i]))


def scale_of(points):
    p = np.asarray(points, np.float64)
    p = p[np.isfinite(p)]
    return max(1.0, float(np.abs(p).max())) if p.size else 1.0


def deviation(a, b, scale):
    """The largest |a - b| / scale where both are numbers; inf where the NaN patterns or shapes differ"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return float("inf")
    m = ~np.isnan(b)
    return float(np.abs(a[m] - b[m]).max() / scale) if m.any() else 0.0


# ---- the B-spline restatement ------------------------------------------------------------------------------
def n_samples(step, three_d):
    n = int(1 / step)
    return max(2, n) if three_d else n


def bs_params(P, param_mode, three_d):
    P = np.asarray(P, np.float64)
    n = len(P)
    if param_mode == "uniform_spaced":
        return np.linspace(0, 1, n)
    d = np.diff(P, axis=0)
    if three_d:
        length = np.sqrt(np.add.reduce(d * d, axis=1))
    else:
        length = np.array([math.hypot(a, b) for a, b in d[:, :2]])
    s = np.cumsum(np.sqrt(length) if param_mode == "centripetal" else length)
    par = np.zeros(n)
    if three_d and not s[-1] > 0:
        return par
    with np.errstate(all="ignore"):
        par[1:] = s / s[-1]
    return par


def bs_knots(par, n, k):
    knot = np.zeros(n + k + 1)
    knot[n:] = 1.0
    for i in range(k + 1, n):
        acc = 0.0
        for j in range(i - k, i):
            acc = acc + par[j]
        knot[i] = acc / k
    return knot


def bs_span(knot, n, t):
    """mu with knot[mu] <= t < knot[mu + 1], 0 <= mu <= n - 1, or -1"""
    for mu in range(n):
        if knot[mu] <= t < knot[mu + 1]:
            return mu
    return -1


def bs_basis(knot, k, mu, t):
    """N_{mu - k .. mu, k}(t): the triangular scheme, each entry by the reference's expression"""
    N = [0.0] * (k + 1)
    N[k] = 1.0
    for d in range(1, k + 1):
        for r in range(k - d, k + 1):
            i = mu - k + r
            if i < 0:
                continue
            a, b = N[r], (N[r + 1] if r + 1 <= k else 0.0)
            l1, l2 = knot[i + d] - knot[i], knot[i + d + 1] - knot[i + 1]
            t1 = 0.0 if l1 == 0 else (t - knot[i]) / l1 * a
            t2 = 0.0 if l2 == 0 else (knot[i + d + 1] - t) / l2 * b
            N[r] = t1 + t2
    return N


def bs_matrix(ts, knot, n_knot_pts, n_funcs, k):
    """The matrix [len(ts), n_funcs] of basis values over the knot vector of n_knot_pts points"""
    M = np.zeros((len(ts), n_funcs))
    for i, t in enumerate(ts):
        mu = bs_span(knot, n_knot_pts, t)
        if mu < 0:
            continue
        for r, v in enumerate(bs_basis(knot, k, mu, t)):
            j = mu - k + r
            if 0 <= j < n_funcs:
                M[i, j] = v
    return M


def bs_restate(points, step, k, param_mode, spline_mode, three_d):
    """dict(status, T, params, knot, control, rows, length) as pmp_bspline_batch defines them"""
    P = np.asarray(points, np.float64)
    if not three_d:
        P = P[:, :2]
    n, dim = P.shape
    T = n_samples(step, three_d)
    if T == 0:
        return dict(status=ST_INDEX, T=0)
    par = bs_params(P, param_mode, three_d)
    knot = bs_knots(par, n, k)
    nc = n if spline_mode == "interpolation" else n - 1
    poisoned = not (np.isfinite(par).all() and np.isfinite(knot).all())
    status = ST_OK
    ctrl = np.full((nc, dim), NAN)
    try:
        if poisoned:
            pass
        elif spline_mode == "interpolation":
            N = bs_matrix(par, knot, n, n, k)
            N[n - 1, n - 1] = 1
            ctrl = np.linalg.solve(N, P)
        else:
            h = n - 1
            N = bs_matrix(par, knot, n, h, k)
            N_ = N[1 : n - 1, 1 : h - 1]
            qk = np.array([P[i] - N[i, 0] * P[0] - N[i, h - 1] * P[-1] for i in range(1, n - 1)]).reshape(n - 2, dim)
            inner = np.linalg.solve(N_.T @ N_, N_.T @ qk) if h > 2 else np.zeros((0, dim))
            ctrl = np.vstack([P[0], inner, P[-1]])
    except np.linalg.LinAlgError:
        status = ST_LINALG
    if status == ST_OK and spline_mode == "approximation":
        par = bs_params(ctrl, param_mode, three_d)
        knot = bs_knots(par, nc, k)
        poisoned = poisoned or not (np.isfinite(par).all() and np.isfinite(knot).all())
    out = dict(status=status, T=T, params=par, knot=knot, control=ctrl, n_control=nc)
    if status != ST_OK:
        return out
    if poisoned:
        rows = np.full((T, dim), NAN)
    else:
        M = bs_matrix(np.linspace(0, 1, T), knot, nc, nc, k)
        M[T - 1, nc - 1] = 1
        rows = M @ ctrl
    out.update(rows=rows, length=polyline_length(rows, three_d))
    return out


def polyline_length(rows, three_d):
    """The length the kernel reports: hypot of x and y (Curve.length); BSpline3D on 3D rows: the Euclidean norm"""
    rows = np.asarray(rows, np.float64)
    d = np.diff(rows, axis=0)
    if three_d and rows.shape[1] == 3:
        return float(np.sqrt((d * d).sum(axis=1)).sum())
    return float(sum(math.hypot(a, b) for a, b in d[:, :2]))


# ---- the cubic-spline restatement --------------------------------------------------------------------------
def cs_table(points):
    """s = [0] + cumsum(hypot) as CubicSpline.run builds it"""
    P = np.asarray(points, np.float64)
    s = [0.0]
    acc = None
    for a, b in zip(P[:-1], P[1:]):
        h = math.hypot(b[0] - a[0], b[1] - a[1])
        acc = h if acc is None else acc + h
        s.append(acc)
    return np.array(s)


def cs_count(s_last, step):
    """len(np.arange(0, s_last, step)), or None where it raises"""
    with np.errstate(all="ignore"):
        q = math.ceil(s_last / step) if math.isfinite(s_last) else None
    return None if q is None or q > 1 << 24 else max(int(q), 0)


def cs_coeffs(s, a):
    n = len(s)
    h = np.diff(s)
    with np.errstate(all="ignore"):
        cp, dp, c = np.zeros(n), np.zeros(n), np.zeros(n)
        for i in range(1, n - 1):
            B = 3.0 * (a[i + 1] - a[i]) / h[i] - 3.0 * (a[i] - a[i - 1]) / h[i - 1]
            m = 2.0 * (h[i - 1] + h[i]) - h[i - 1] * cp[i - 1]
            cp[i] = h[i] / m
            dp[i] = (B - h[i - 1] * dp[i - 1]) / m
        for i in range(n - 2, 0, -1):
            c[i] = dp[i] - cp[i] * c[i + 1]
        d = np.array([(c[i + 1] - c[i]) / (3.0 * h[i]) for i in range(n - 1)])
        b = np.array([(a[i + 1] - a[i]) / h[i] - h[i] * (c[i + 1] + 2.0 * c[i]) / 3.0 for i in range(n - 1)])
    return b, c, d


def cs_restate(points, step, rows_idx=None):
    """(status, count, rows [len(rows_idx) or count, 5]: x, y, yaw, dx, dy)"""
    P = np.asarray(points, np.float64)[:, :2]
    s = cs_table(P)
    count = cs_count(float(s[-1]), step)
    if count is None:
        return ST_LINALG, 0, np.zeros((0, 5))
    idx = np.arange(count) if rows_idx is None else np.asarray(rows_idx)
    co = [cs_coeffs(s, P[:, ax]) for ax in range(2)]
    rows = np.zeros((len(idx), 5))
    with np.errstate(all="ignore"):
        for r, i in enumerate(idx):
            t = float(i) * step
            j = min(max(int(np.searchsorted(s, t, side="right")) - 1, 0), len(s) - 2)
            dx = t - s[j]
            for ax in range(2):
                b, c, d = co[ax]
                a = P[j, ax]
                rows[r, ax] = a + b[j] * dx + c[j] * (dx * dx) + d[j] * (dx * dx * dx)
                rows[r, 3 + ax] = b[j] + 2.0 * c[j] * dx + 3.0 * d[j] * (dx * dx)
            rows[r, 2] = math.atan2(rows[r, 4], rows[r, 3])
    return ST_OK, count, rows


def angle_diff(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return np.abs((d + math.pi) % (2.0 * math.pi) - math.pi)


def cs_deviation(rows, ref, scale):
    """(worst deviation of x, y relative to scale and of yaw as an angle, rows whose yaw was skipped)"""
    rows, ref = np.asarray(rows, np.float64), np.asarray(ref, np.float64)
    if rows.shape[0] != ref.shape[0]:
        return float("inf"), 0
    if not np.array_equal(np.isnan(rows[:, :2]), np.isnan(ref[:, :2])):
        return float("inf"), 0
    ok = ~np.isnan(ref[:, 0]) & ~np.isnan(ref[:, 1])
    dev = float(np.abs(rows[ok, :2] - ref[ok, :2]).max() / scale) if ok.any() else 0.0
    with np.errstate(all="ignore"):
        firm = ok & (np.hypot(ref[:, 3], ref[:, 4]) >= 1e-9)
    if firm.any():
        dev = max(dev, float(angle_diff(rows[firm, 2], ref[firm, 2]).max()))
    return dev, int((ok & ~firm).sum())
