"""SplineTrajectory3D fixture (tests/golden/splinetraj.npz, made by make_golden_splinetraj.py): the
loader, the comparison rules and a sequential Python restatement of the arithmetic of
csrc/splinetraj3d.hip in the kernel's operation order (trajectory/spline_trajectory.py:16-392 and
trajectory_base.py:193-216, :245-261 for smoothing_factor = 0, in plain IEEE doubles).  No scipy spline
object is used: knots by the fixed rule, a banded collocation solve without pivoting, de Boor's
recursion."""
import math

import numpy as np

from golden_io import load_npz, seg

NAN = float("nan")
RTOL = 1e-9      # rows and coefficients: relative to max(1, |ref|), the project's trajectory bound
RTOL_T = 1e-12   # times and total_time, relative
NS, NARC = 500, 1000


def cases():
    """Yield (i, name, path [n, 3], (vmax, amax, dt), spline_degree, fixture)."""
    z = load_npz("splinetraj.npz")
    for i, name in enumerate(z["names"]):
        c = z["cons"][i]
        yield (i, str(name), seg(z["path"].reshape(-1, 3), z["path_off"], i), (tuple(c[0:3]), tuple(c[3:6]), float(c[6])),
               int(z["degree"][i]), z)


def norm3(a, b, c):
    return math.sqrt((a * a + b * b) + c * c)


def lin01(ns, i):
    """np.linspace(0, 1, ns)[i]"""
    return 1.0 if i == ns - 1 else i * (1.0 / (ns - 1))


def knots_rule(u, k):
    """FITPACK's knots for s = 0"""
    n = len(u)
    if k % 2:
        mid = [u[j] for j in range((k + 1) // 2, n - (k + 1) // 2)]
    else:
        mid = [(u[j] + u[j + 1]) / 2.0 for j in range(k // 2, n - k // 2 - 1)]
    return [u[0]] * (k + 1) + mid + [u[-1]] * (k + 1)


class Spline:
    """One path's fit: u, knots, coefficients of q, q', q'' per axis."""

    def __init__(self, path, degree):
        P = [[float(v) for v in p] for p in path]
        n = len(P)
        self.n = n
        k = min(int(degree), n - 1)
        if n < 3 or k < 2:
            raise ValueError("the second derivative of a linear spline does not exist")
        self.k = k
        # centripetal parameter (:60-77) and the polyline's length (trajectory_base.py:144-149)
        acc, length, d = 0.0, 0.0, [0.0]
        for i in range(1, n):
            ch = norm3(P[i][0] - P[i - 1][0], P[i][1] - P[i - 1][1], P[i][2] - P[i - 1][2])
            acc = acc + math.sqrt(ch)
            length = length + ch
            d.append(acc)
        self.path_length = length
        if not (0.0 < acc < math.inf):
            raise ValueError("x must be strictly increasing if s = 0")
        self.u = [v / acc for v in d]
        if any(not (self.u[i + 1] - self.u[i] > 0.0) for i in range(n - 1)):
            raise ValueError("x must be strictly increasing if s = 0")
        self.t = knots_rule(self.u, k)
        # collocation rows: the degree-k basis on the span of u_i, columns off[i] .. off[i] + k
        A, off = [], []
        for i in range(n):
            s = self.span(self.u[i])
            off.append(s - k)
            A.append(self.stages(self.u[i], s)[k] + [0.0] * (5 - k))
        b = [[P[i][dd] for i in range(n)] for dd in range(3)]
        # elimination without pivoting, the kernel's order
        for c in range(n - 1):
            for r in range(c + 1, min(c + k, n - 1) + 1):
                if off[r] <= c:
                    m = A[r][c - off[r]] / A[c][c - off[c]]
                    for col in range(c + 1, off[c] + k + 1):
                        A[r][col - off[r]] = A[r][col - off[r]] - m * A[c][col - off[c]]
                    for dd in range(3):
                        b[dd][r] = b[dd][r] - m * b[dd][c]
        for dd in range(3):
            x = b[dd]
            for i in range(n - 1, -1, -1):
                s = x[i]
                for j in range(i + 1, off[i] + k + 1):
                    s = s - A[i][j - off[i]] * x[j]
                x[i] = s / A[i][i - off[i]]
        t = self.t
        self.c0 = b
        self.c1 = [[(c[i + 1] - c[i]) * float(k) / (t[i + k + 1] - t[i + 1]) for i in range(n - 1)] for c in self.c0]
        self.c2 = [[(c[i + 1] - c[i]) * float(k - 1) / (t[i + k + 1] - t[i + 2]) for i in range(n - 2)] for c in self.c1]

    def span(self, x):
        lo, hi = self.k, self.n - 1
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if self.t[mid] <= x:
                lo = mid
            else:
                hi = mid - 1
        return lo

    def stages(self, x, s):
        """de Boor's recursion: the basis functions of degree 0 .. k on span s"""
        t = self.t
        h = [1.0]
        out = [list(h)]
        for j in range(1, self.k + 1):
            hh = list(h)
            h = [0.0] * (j + 1)
            for i in range(j):
                tr, tl = t[s + 1 + i], t[s + 1 + i - j]
                g = hh[i] / (tr - tl)
                h[i] = h[i] + g * (tr - x)
                h[i + 1] = g * (x - tl)
            out.append(list(h))
        return out

    def eval(self, x):
        """q(x), q'(x), q''(x)"""
        s = self.span(x)
        st = self.stages(x, s)
        k, base = self.k, s - self.k
        res = []
        for c, j in ((self.c0, k), (self.c1, k - 1), (self.c2, k - 2)):
            v = []
            for dd in range(3):
                acc = 0.0
                for i in range(j + 1):
                    acc = acc + c[dd][base + i] * st[j][i]
                v.append(acc)
            res.append(v)
        return res


def interp01(xs, x):
    """interp1d(xs, linspace(0, 1, len(xs)), 'linear', extrapolate)(x) clipped to [0, 1]"""
    ns = len(xs)
    lo, hi = 0, ns
    while lo < hi:
        mid = (lo + hi) >> 1
        if xs[mid] < x:
            lo = mid + 1
        else:
            hi = mid
    h = min(max(lo, 1), ns - 1)
    l0 = h - 1
    yl, yh = lin01(ns, l0), lin01(ns, h)
    with np.errstate(all="ignore"):
        u = float((np.float64(yh) - yl) / (np.float64(xs[h]) - xs[l0]) * (x - xs[l0]) + yl)
    return 0.0 if u < 0.0 else (1.0 if u > 1.0 else u)


def table(sp, ns, vclip=None):
    """times[] (:154-203) with vclip, else the raw arc-length table (:122-152), summed left to right"""
    out = [0.0]
    acc = 0.0
    ppos, pvel = None, 0.0
    for i in range(ns):
        pos, q1, _ = sp.eval(lin01(ns, i))
        speed = norm3(*q1)
        vel = (vclip if vclip is not None and vclip < speed else speed) if speed > 0.0 else 0.0
        if i >= 1:
            ds = norm3(pos[0] - ppos[0], pos[1] - ppos[1], pos[2] - ppos[2])
            if vclip is None:
                inc = ds
            else:
                avg = (vel + pvel) / 2.0
                inc = ds / avg if avg > 0.0 else 0.1
            acc = acc + inc
            out.append(acc)
        ppos, pvel = pos, vel
    return out


def sample_times(total, dt):
    """(times, appended): the repeated sum, then total_time if the last is short of it"""
    ts = []
    t = 0.0
    while t <= total:
        ts.append(t)
        t += dt
    app = bool(ts) and ts[-1] < total
    if app:
        ts.append(total)
    return ts, app


def add_yaw(rows):
    """compute_yaw_from_velocity (trajectory_base.py:245-261)"""
    for r in rows:
        if math.sqrt(r[4] * r[4] + r[5] * r[5]) > 1e-6:
            r[10] = math.atan2(r[5], r[4])
    for k in range(1, len(rows)):
        d = rows[k][0] - rows[k - 1][0]
        if d > 0 and not math.isnan(rows[k][10]) and not math.isnan(rows[k - 1][10]):
            dy = rows[k][10] - rows[k - 1][10]
            while dy > math.pi:
                dy -= 2 * math.pi
            while dy < -math.pi:
                dy += 2 * math.pi
            rows[k][11] = dy / d


def restate(path, vmax, amax, dt, degree, eval_t=None, sample_dt=None, constant_speed=False):
    """What pmp_splinetraj3d_batch writes for one path: points [n, 12], total_time; and the fit."""
    sp = Spline(path, degree)
    vclip = min(abs(v) for v in vmax)
    TM = table(sp, NS, vclip)
    T0 = TM[-1]
    if not T0 < math.inf:
        raise ValueError("total_time is not finite")
    du = 1.0 / T0 if T0 > 0 else 0.0
    # generate()'s loop (:216-263)
    ts, app = sample_times(T0, dt)
    gen = []
    for j, t in enumerate(ts):
        last = app and j == len(ts) - 1
        pos, v, a = sp.eval(1.0 if last else interp01(TM, t))
        v = [0.0 if last else x * du for x in v]
        a = [0.0 if last else x * (du * du) for x in a]
        gen.append([t] + pos + v + a + [NAN, NAN])
    # _enforce_constraints (:304-323)
    rv = max(abs(r[4 + d]) / vmax[d] for r in gen for d in range(3))
    ra = max(abs(r[7 + d]) / amax[d] for r in gen for d in range(3))
    scaled = rv > 1.0 or ra > 1.0
    scale, total = 1.0, T0
    if scaled:
        sa = math.sqrt(ra)
        scale = sa if sa > rv else rv
        total = T0 * scale
    fit = dict(u=np.array(sp.u), knots=np.array(sp.t), coef=np.array(sp.c0), ratios=(rv, ra), scale=scale, T0=T0, k=sp.k)
    if eval_t is None and sample_dt is None and not constant_speed:
        if scaled:
            for r in gen:
                r[0] = r[0] * scale
                for d in range(3):
                    r[4 + d] = r[4 + d] / scale
                    r[7 + d] = r[7 + d] / (scale * scale)
        add_yaw(gen)
        return dict(points=np.array(gen, np.float64).reshape(-1, 12), total_time=total, **fit)
    rows = []
    if constant_speed:  # :325-392
        ARC = table(sp, NARC)
        al = ARC[-1]
        if al > 0.0:
            ARC = [x / al for x in ARC]
        want = sp.path_length / total if total > 0 else 1.0
        vmin = min(vmax)
        cs = vmin if vmin < want else want
        total = sp.path_length / cs
        ts, app = sample_times(total, dt)
        for j, t in enumerate(ts):
            last = app and j == len(ts) - 1
            pos, v, _ = sp.eval(1.0 if last else interp01(ARC, t / total if total > 0 else 0.0))
            nv = norm3(*v)
            v = [(x / nv) * cs if nv > 0.0 and not last else 0.0 for x in v]
            rows.append([t] + pos + v + [0.0] * 3 + [NAN, NAN])
    else:  # evaluate(t) (:273-302), resample(dt) (trajectory_base.py:193-216)
        ts = list(eval_t) if eval_t is not None else sample_times(total, sample_dt)[0]
        du = 1.0 / total if total > 0 else 0.0
        for t in ts:
            tc = 0.0 if t < 0.0 else (total if t > total else t)
            u = tc / total if total > 0 else 0.0
            u = 0.0 if u < 0.0 else (1.0 if u > 1.0 else u)
            pos, v, a = sp.eval(u)
            rows.append([tc] + pos + [x * du for x in v] + [x * (du * du) for x in a] + [NAN, NAN])
    return dict(points=np.array(rows, np.float64).reshape(-1, 12), total_time=total, **fit)


def close(a, b, what, rtol=RTOL):
    """|a - b| <= rtol max(1, |b|) elementwise, the NaN (= None) pattern exact; returns the largest error
    per column (of 2-D input) or overall"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert (np.isnan(a) == np.isnan(b)).all(), what
    with np.errstate(invalid="ignore"):
        err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    err = np.where(np.isnan(b), 0.0, err)
    assert err.size == 0 or err.max() <= rtol, (what, float(err.max()))
    if err.ndim == 2:
        return err.max(axis=0) if len(err) else np.zeros(err.shape[1])
    return float(err.max()) if err.size else 0.0


def times_match(a, b, what):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.all(np.abs(a - b) <= RTOL_T * np.abs(b)), (what, float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))))


def compare_case(z, i, points, total_time):
    """One generated trajectory against fixture case i: exact count and NaN pattern, times within RTOL_T,
    rows within RTOL; returns the largest error per column."""
    points = np.asarray(points)
    assert len(points) == int(z["n_pts"][i]), (i, len(points), int(z["n_pts"][i]))
    times_match([total_time], [z["total_time"][i]], f"case {i} total_time")
    times_match(points[:, 0], seg(z["times"], z["t_off"], i), f"case {i} times")
    idx = seg(z["pts_idx"], z["pts_off"], i)
    return close(points[idx], seg(z["pts"], z["pts_off"], i), f"case {i} points")


def check_constraints(points, vmax, amax):
    """trajectory_base.py:150-190 on rows"""
    p = np.asarray(points)
    return dict(velocity_satisfied=not np.any(np.max(np.abs(p[:, 4:7]), axis=0) > np.asarray(vmax)),
                acceleration_satisfied=not np.any(np.max(np.abs(p[:, 7:10]), axis=0) > np.asarray(amax)),
                jerk_satisfied=True)


def compare_checks(z, i, got):
    """check_constraints() against the fixture: the jerk flag always; a velocity / acceleration flag only
    where the fixture's ratio after scaling is off 1 by more than 1e-9 (when the reference scales, the
    binding quantity lands on its limit to an ulp and its flag is decided by the reference's own
    rounding).  Returns how many flags were skipped."""
    want = z["checks"][i]
    after = z["ratios_after"][i]
    assert got["jerk_satisfied"] is True and bool(want[2]) is True
    skipped = 0
    for j, key in enumerate(("velocity_satisfied", "acceleration_satisfied")):
        if abs(after[j] - 1.0) > 1e-9:
            assert got[key] == bool(want[j]), (i, key)
        else:
            skipped += 1
    assert skipped <= 1, i
    if float(z["scale"][i]) == 1.0:
        assert skipped == 0, i
    return skipped
