"""Reeds-Shepp fixture (tests/golden/reeds_shepp.npz, made by make_golden_reeds_shepp.py): the loader, the
comparison rules and a sequential Python restatement of csrc/reeds_shepp.hip's arithmetic (the kernel's
structure: one sin / cos of phi shared by the reflections, the reflections as a loop, one family at a
time; plain IEEE doubles), with an optional forced slot.

Rules: the slot, the count, the status and the zero-point cases are exact; lengths, cost and the rows' x, y
are within 1e-9 max(1, |ref|); yaw by its difference wrapped to (-pi, pi].  An untied case is compared with
the reference's recorded slot, lengths, cost, count and rows.  A tied case (more than one slot within
1e-12 max(1, best) of the best: the mirrored CCC words have the same length mathematically, so which one
the reference takes is a rounding accident) must choose a slot of its tie_set, match the fixture's recorded
lengths of that slot and the reference's own count for that slot (and its rows, where recorded), and cost
what the reference's best does within the tolerance.  slot_costs [46]: the NaN pattern exact on
feas_stable slots, the values within the tolerance."""
import math

import numpy as np

from dubins_checks import close, interpolate, piece_steps, rows_close, step_sums, yaw_close  # noqa: F401
from golden_io import load_npz, seg

RTOL = 1e-9
PI = math.pi
HALF_PI = 0.5 * math.pi
NAN = float("nan")
INF = float("inf")
NSLOT = 46
MAX_ANGLE = 64.0
MAX_STEPS = 16777216.0
WORDS = (
    "SLS", "SRS",
    "LRL", "LRL", "RLR", "RLR", "LRL", "LRL", "RLR", "RLR",
    "LSL", "LSL", "RSR", "RSR", "LSR", "LSR", "RSL", "RSL",
    "LRLR", "LRLR", "RLRL", "RLRL", "LRLR", "LRLR", "RLRL", "RLRL",
    "LRSL", "LRSL", "RLSR", "RLSR", "LRSR", "LRSR", "RLSL", "RLSL",
    "LSRL", "LSRL", "RSLR", "RSLR", "RSRL", "RSRL", "LSLR", "LSLR",
    "LRSLR", "LRSLR", "RLSRL", "RLSRL",
)


def load():
    return load_npz("reeds_shepp.npz")


def M(th):
    while th > PI:
        th -= 2.0 * PI
    while th < -PI:
        th += 2.0 * PI
    return th


def R(x, y):
    return math.hypot(x, y), math.atan2(y, x)


def reflect(x, y, phi, s, c, r):
    """(x, y, phi, sin phi, cos phi) of reflection r: bit 0 time-flip, bit 1 reflect"""
    neg = (r ^ (r >> 1)) & 1
    return (-x if r & 1 else x, -y if r & 2 else y, -phi if neg else phi, -s if neg else s, c)


def SLS(a):
    x, y, phi = a[0], a[1], M(a[2])
    if y > 0.0 and 0.0 < phi < PI * 0.99:
        xd = -y / math.tan(phi) + x
        return xd - math.tan(phi / 2.0), phi, math.sqrt((x - xd) * (x - xd) + y * y) - math.tan(phi / 2.0)
    if y < 0.0 and 0.0 < phi < PI * 0.99:
        xd = -y / math.tan(phi) + x
        return xd - math.tan(phi / 2.0), phi, -math.sqrt((x - xd) * (x - xd) + y * y) - math.tan(phi / 2.0)
    return None


def LRL(a):
    x, y, phi, s, c = a
    r, theta = R(x - s, y - 1.0 + c)
    if r <= 4.0:
        u = -2.0 * math.asin(0.25 * r)
        t = M(theta + 0.5 * u + PI)
        v = M(phi - t + u)
        if t >= 0.0 and u <= 0.0:
            return t, u, v
    return None


def LSL(a):
    x, y, phi, s, c = a
    u, t = R(x - s, y - 1.0 + c)
    if t >= 0.0:
        v = M(phi - t)
        if v >= 0.0:
            return t, u, v
    return None


def LSR(a):
    x, y, phi, s, c = a
    r, theta = R(x + s, y - 1.0 - c)
    r = r * r
    if r >= 4.0:
        u = math.sqrt(r - 4.0)
        t = M(theta + math.atan2(2.0, u))
        v = M(t - phi)
        if t >= 0.0 and v >= 0.0:
            return t, u, v
    return None


def cal_tau_omega(u, v, xi, eta, phi):
    delta = M(u - v)
    A = math.sin(u) - math.sin(delta)
    B = math.cos(u) - math.cos(delta) - 1.0
    t1 = math.atan2(eta * A - xi * B, xi * A + eta * B)
    t2 = 2.0 * (math.cos(delta) - math.cos(v) - math.cos(u)) + 3.0
    tau = M(t1 + PI) if t2 < 0 else M(t1)
    return tau, M(tau - u + v - phi)


def LRLRn(a):
    x, y, phi, s, c = a
    xi, eta = x + s, y - 1.0 - c
    rho = 0.25 * (2.0 + math.sqrt(xi * xi + eta * eta))
    if rho <= 1.0:
        u = math.acos(rho)
        t, v = cal_tau_omega(u, -u, xi, eta, phi)
        if t >= 0.0 and v <= 0.0:
            return t, u, v
    return None


def LRLRp(a):
    x, y, phi, s, c = a
    xi, eta = x + s, y - 1.0 - c
    rho = (20.0 - xi * xi - eta * eta) / 16.0
    if 0.0 <= rho <= 1.0:
        u = -math.acos(rho)
        if u >= -0.5 * PI:
            t, v = cal_tau_omega(u, u, xi, eta, phi)
            if t >= 0.0 and v >= 0.0:
                return t, u, v
    return None


def LRSR(a):
    x, y, phi, s, c = a
    xi, eta = x + s, y - 1.0 - c
    rho, theta = R(-eta, xi)
    if rho >= 2.0:
        t, u = theta, 2.0 - rho
        v = M(t + 0.5 * PI - phi)
        if t >= 0.0 and u <= 0.0 and v <= 0.0:
            return t, u, v
    return None


def LRSL(a):
    x, y, phi, s, c = a
    xi, eta = x - s, y - 1.0 + c
    rho, theta = R(xi, eta)
    if rho >= 2.0:
        r = math.sqrt(rho * rho - 4.0)
        u = 2.0 - r
        t = M(theta + math.atan2(r, -2.0))
        v = M(phi - 0.5 * PI - t)
        if t >= 0.0 and u <= 0.0 and v <= 0.0:
            return t, u, v
    return None


def LRSLR(a):
    x, y, phi, s, c = a
    xi, eta = x + s, y - 1.0 - c
    r = math.hypot(xi, eta)
    if r >= 2.0:
        u = 4.0 - math.sqrt(r * r - 4.0)
        if u <= 0.0:
            t = M(math.atan2((4.0 - u) * xi - 2.0 * eta, -2.0 * xi + (u - 4.0) * eta))
            v = M(t - phi)
            if t >= 0.0 and v >= 0.0:
                return t, u, v
    return None


def all_slots(x, y, phi):
    """[lengths tuple or None] * 46 for the frame (x, y, phi), in the kernel's order of evaluation"""
    out = [None] * NSLOT
    s, c = math.sin(phi), math.cos(phi)
    xb, yb = x * c + y * s, x * s - y * c

    def put(slot, tuv, flip, pattern):
        if tuv is not None:
            ls = pattern(*tuv)
            out[slot] = tuple(-v for v in ls) if flip else tuple(ls)

    for k in range(2):
        put(k, SLS(reflect(x, y, phi, s, c, 2 * k)), False, lambda t, u, v: (t, u, v))
    for k in range(8):
        back = k >= 4
        tuv = LRL(reflect(xb if back else x, yb if back else y, phi, s, c, k & 3))
        put(2 + k, tuv, k & 1, (lambda t, u, v: (v, u, t)) if back else (lambda t, u, v: (t, u, v)))
    for k in range(4):
        put(10 + k, LSL(reflect(x, y, phi, s, c, k)), k & 1, lambda t, u, v: (t, u, v))
    for k in range(4):
        put(14 + k, LSR(reflect(x, y, phi, s, c, k)), k & 1, lambda t, u, v: (t, u, v))
    for k in range(4):
        put(18 + k, LRLRn(reflect(x, y, phi, s, c, k)), k & 1, lambda t, u, v: (t, u, -u, v))
    for k in range(4):
        put(22 + k, LRLRp(reflect(x, y, phi, s, c, k)), k & 1, lambda t, u, v: (t, u, u, v))
    for k in range(16):
        back = k >= 8
        a = reflect(xb if back else x, yb if back else y, phi, s, c, k & 3)
        tuv = LRSR(a) if k & 4 else LRSL(a)
        put(26 + k, tuv, k & 1, (lambda t, u, v: (v, u, -HALF_PI, t)) if back else (lambda t, u, v: (t, -HALF_PI, u, v)))
    for k in range(4):
        put(42 + k, LRSLR(reflect(x, y, phi, s, c, k)), k & 1, lambda t, u, v: (t, -HALF_PI, u, -HALF_PI, v))
    return out


def path_length(ls):
    cost = 0.0
    for v in ls:
        cost += abs(v)
    return cost


def sample(pieces, step, max_curv):
    """The local points of a list of (mode, signed length) pieces from the pose (0, 0, 0), the trailing ones
    with x == 0.0 dropped; total: the count before the strip"""
    R_ = step_sums(step, max((piece_steps(step, ln) for _, ln in pieces), default=0))
    pts = [(0.0, 0.0, 0.0)]
    cur = pts[0]
    for mode, ln in pieces:
        for k in range(1, piece_steps(step, ln) + 1):
            pts.append(interpolate(mode, R_[k] if ln > 0.0 else -R_[k], cur, max_curv))
        cur = interpolate(mode, ln, cur, max_curv)
        pts.append(cur)
    total = len(pts)
    while pts and pts[-1][0] == 0.0:
        pts.pop()
    return pts, total


def restate(s, g, step, max_curv, force_slot=None):
    """What pmp_reeds_shepp_batch writes for one pair: slot, lengths [5], cost, slot_costs [46], all_lengths
    [46, 5], points [n, 3], status."""
    none = dict(slot=255, lengths=np.full(5, NAN), cost=INF, slot_costs=np.full(NSLOT, NAN),
                all_lengths=np.full((NSLOT, 5), NAN), points=np.zeros((0, 3)), status=4)
    sx, sy, syaw = s
    dx, dy, phi = g[0] - sx, g[1] - sy, g[2] - syaw
    if not (abs(syaw) <= MAX_ANGLE and abs(phi) <= MAX_ANGLE):
        return none
    x = (math.cos(syaw) * dx + math.sin(syaw) * dy) * max_curv
    y = (-math.sin(syaw) * dx + math.cos(syaw) * dy) * max_curv
    try:
        slots = all_slots(x, y, phi)
    except (ValueError, OverflowError):  # libm on a non-finite coordinate: the kernel's comparisons are all false
        return none
    costs = np.array([NAN if ls is None else path_length(ls) for ls in slots])
    all_lengths = np.full((NSLOT, 5), NAN)
    for k, ls in enumerate(slots):
        if ls is not None:
            all_lengths[k, : len(ls)] = ls
    best, cost = -1, INF
    for k, ls in enumerate(slots):
        if ls is not None and costs[k] < cost:
            best, cost = k, float(costs[k])
    if force_slot is not None:
        best = int(force_slot)
        cost = float(costs[best])
    out = dict(slot=255 if best < 0 else best, lengths=all_lengths[best].copy() if best >= 0 else np.full(5, NAN),
               cost=cost / max_curv, slot_costs=costs, all_lengths=all_lengths, points=np.zeros((0, 3)), status=4)
    nslots = cost / step
    if best < 0 or not nslots < INF:
        return out
    if not nslots < MAX_STEPS:
        out["status"] = 2
        return out
    ls = slots[best]
    loc, total = sample(list(zip(WORDS[best], ls)), step, max_curv)
    if total > math.trunc(nslots) + len(ls) + 3:
        return out
    cm, sm = math.cos(-syaw), math.sin(-syaw)
    rows = [((cm * px + sm * py) + sx, (-sm * px + cm * py) + sy, M(yaw + syaw)) for px, py, yaw in loc]
    out.update(points=np.array(rows, np.float64).reshape(-1, 3), status=0)
    return out


def cases(z=None):
    """Yield (i, name, start, goal, step, max_curv) of every fixture case."""
    z = load() if z is None else z
    for i, name in enumerate(z["names"]):
        yield i, str(name), tuple(z["start"][i]), tuple(z["goal"][i]), float(z["params"][i, 0]), float(z["params"][i, 1])


def tie_slots(mask):
    return [k for k in range(NSLOT) if int(mask) >> k & 1]


def tie_rows_of(z, i, slot):
    """The reference's own rows of tied case i forced to `slot` (None where not recorded)"""
    if slot == int(z["slot"][i]):
        return seg(z["rows"], z["rows_off"], i) if z["has_rows"][i] else None
    hit = np.nonzero((z["tie_rows_case"] == i) & (z["tie_rows_slot"] == slot))[0]
    return seg(z["tie_rows"], z["tie_rows_off"], int(hit[0])) if len(hit) else None


def _worst(worst, key, e):
    if worst is not None:
        worst[key] = max(worst.get(key, 0.0), e)


def compare_case(z, i, slot, lengths, cost, n_points, rows, status, worst=None):
    """One computed pair (the device's, or the restatement's) against fixture case i under the rules of
    this module.  rows: the n_points rows.  Returns None for an untied case, else whether the tied case
    chose the reference's slot."""
    name = str(z["names"][i])
    slot, n_points = int(slot), int(n_points)
    tied = bool(z["tied"][i])
    assert int(status) == 0, (name, status)
    if tied:
        assert int(z["tie_set"][i]) >> slot & 1, (name, slot, tie_slots(z["tie_set"][i]))
        want_count = int(z["tie_count"][i, slot])
        ref_rows = tie_rows_of(z, i, slot)
    else:
        assert slot == int(z["slot"][i]), (name, slot, int(z["slot"][i]))
        want_count = int(z["count"][i])
        ref_rows = seg(z["rows"], z["rows_off"], i) if z["has_rows"][i] else None
    assert n_points == want_count, (name, slot, n_points, want_count)
    if want_count == 0:  # the zero-point cases: exact
        assert float(cost) == 0.0 and float(z["cost"][i]) == 0.0, (name, cost)
    _worst(worst, "lengths", close(lengths, z["lengths"][i, slot], name + " lengths"))
    _worst(worst, "cost", close(cost, z["cost"][i], name + " cost"))
    if ref_rows is not None:
        rows_close(rows, ref_rows, name, worst)
    return slot == int(z["slot"][i]) if tied else None


def compare_slot_costs(z, i, slot_costs, worst=None):
    """slot_costs [46] against the fixture's path_length: NaN pattern exact on feas_stable slots"""
    name = str(z["names"][i])
    got, ref = np.asarray(slot_costs, np.float64), z["path_length"][i]
    stable = z["feas_stable"][i]
    assert got.shape == ref.shape == (NSLOT,), name
    assert (np.isnan(got) == np.isnan(ref))[stable].all(), (name, np.nonzero(np.isnan(got) != np.isnan(ref))[0])
    m = ~np.isnan(got) & ~np.isnan(ref)
    _worst(worst, "slot_costs", close(got[m], ref[m], name + " slot_costs"))
