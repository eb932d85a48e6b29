"""Dubins fixture (tests/golden/dubins.npz, made by make_golden_dubins.py): the loader, the comparison
rules and a sequential Python restatement of csrc/dubins.hip's arithmetic (the reference's operation
order, curve_generation/dubins_curve.py:38-313 and curve.py:41-55, in plain IEEE doubles), with an optional
forced word.

Rules: the word, the count, the status and the zero-point cases are exact; t, p, q, cost and the rows' x, y
are within 1e-9 max(1, |ref|) (polytraj_checks' rule: far inside the project's 1e-5, four orders above the
5.7e-14 an ulp on every libm result moves a coordinate); yaw by its difference wrapped to (-pi, pi], as
values at +-pi may land on either side.  A fragile case (two words tie to the last bit: an ulp in a libm
result changes the reference's own choice) must choose a word of its recorded set, match the restatement
forced to that word, and cost no less than the reference's best cost less the tolerance."""
import math

import numpy as np

from golden_io import load_npz, seg

WORDS = ("LSL", "RSR", "LSR", "RSL", "RLR", "LRL")
RTOL = 1e-9
PI = math.pi
NAN = float("nan")


def load():
    return load_npz("dubins.npz")


def mod2pi(th):
    return th - 2.0 * PI * math.floor(th / PI / 2.0)


def pi2pi(th):
    while th > PI:
        th -= 2.0 * PI
    while th < -PI:
        th += 2.0 * PI
    return th


def frame(s, g, max_curv):
    gx, gy = g[0] - s[0], g[1] - s[1]
    theta = mod2pi(math.atan2(gy, gx))
    return theta, math.hypot(gx, gy) * max_curv, mod2pi(s[2] - theta), mod2pi(g[2] - theta)


def six_words(alpha, beta, d):
    """[(t, p, q, cost)] * 6 in the reference's order, None where the word is infeasible"""
    sa, sb, ca, cb, cab = math.sin(alpha), math.sin(beta), math.cos(alpha), math.cos(beta), math.cos(alpha - beta)
    d2 = d * d
    at_l = math.atan2(cb - ca, d + sa - sb)
    at_r = math.atan2(ca - cb, d - sa + sb)
    out = [None] * 6

    def put(w, t, p, q):
        out[w] = (t, p, q, abs(t) + abs(p) + abs(q))

    pp = 2 + d2 - 2 * cab + 2 * d * (sa - sb)
    if not pp < 0:
        put(0, mod2pi(-alpha + at_l), math.sqrt(pp), mod2pi(beta - at_l))
    pp = 2 + d2 - 2 * cab + 2 * d * (sb - sa)
    if not pp < 0:
        put(1, mod2pi(alpha - at_r), math.sqrt(pp), mod2pi(-beta + at_r))
    pp = -2 + d2 + 2 * cab + 2 * d * (sa + sb)
    if not pp < 0:
        p = math.sqrt(pp)
        a1, a2 = math.atan2(-ca - cb, d + sa + sb), math.atan2(-2.0, p)
        put(2, mod2pi(-alpha + a1 - a2), p, mod2pi(-beta + a1 - a2))
    pp = -2 + d2 + 2 * cab - 2 * d * (sa + sb)
    if not pp < 0:
        p = math.sqrt(pp)
        a1, a2 = math.atan2(ca + cb, d - sa - sb), math.atan2(2.0, p)
        put(3, mod2pi(alpha - a1 + a2), p, mod2pi(beta - a1 + a2))
    pc = (6.0 - d2 + 2.0 * cab + 2.0 * d * (sa - sb)) / 8.0
    if not abs(pc) > 1.0:
        p = mod2pi(2 * PI - math.acos(pc))
        t = mod2pi(alpha - at_r + p / 2.0)
        put(4, t, p, mod2pi(alpha - beta - t + p))
        t = mod2pi(-alpha + at_l + p / 2.0)
        put(5, t, p, mod2pi(beta - alpha - t + p))
    return out


def interpolate(mode, length, pose, max_curv):
    x, y, yaw = pose
    if mode == "S":
        return x + length / max_curv * math.cos(yaw), y + length / max_curv * math.sin(yaw), yaw
    yaw2 = yaw + length if mode == "L" else yaw - length
    ds = (math.sin(yaw2) - math.sin(yaw)) / max_curv
    dc = (math.cos(yaw2) - math.cos(yaw)) / max_curv
    return (x + ds, y - dc, yaw2) if mode == "L" else (x - ds, y + dc, yaw2)


def step_sums(step, n):
    """R[0] = 0, R[k + 1] = R[k] + step: the reference's `length += d_length`"""
    R = [0.0]
    for _ in range(n):
        R.append(R[-1] + step)
    return R


def piece_steps(step, seg_len):
    """How many k >= 1 have R[k] <= |seg_len|"""
    a, k, length = abs(seg_len), 0, step
    while length <= a:
        k += 1
        length += step
    return k


def sample(pieces, alpha, step, max_curv):
    """The local points of a list of (mode, signed length) pieces, the trailing ones with x == 0.0 dropped"""
    R = step_sums(step, max((piece_steps(step, ln) for _, ln in pieces), default=0))
    pts = [(0.0, 0.0, alpha)]
    cur = pts[0]
    for mode, ln in pieces:
        for k in range(1, piece_steps(step, ln) + 1):
            pts.append(interpolate(mode, R[k] if ln > 0.0 else -R[k], cur, max_curv))
        cur = interpolate(mode, ln, cur, max_curv)
        pts.append(cur)
    while pts and pts[-1][0] == 0.0:
        pts.pop()
    return pts


def restate(s, g, step, max_curv, force_word=None):
    """What pmp_dubins_batch writes for one pair: word, tpq, cost, words6 [6, 4] (NaN = infeasible),
    points [n, 3], status."""
    try:  # a non-finite pose: floor(nan) raises, as in the reference's mod2pi
        theta, d, alpha, beta = frame(s, g, max_curv)
        six = six_words(alpha, beta, d)
    except (ValueError, OverflowError):
        return dict(word=255, tpq=np.full(3, NAN), cost=float("inf"), words6=np.full((6, 4), NAN),
                    points=np.zeros((0, 3)), status=4)
    words6 = np.array([[NAN] * 4 if w is None else list(w) for w in six])
    best, cost = None, float("inf")
    for w, r in enumerate(six):
        if r is not None and cost > r[3]:
            best, cost = w, r[3]
    if force_word is not None:
        best = int(force_word)
        cost = six[best][3]
    if best is None or not math.isfinite(sum(six[best][:3]) / step):
        return dict(word=255 if best is None else best, tpq=np.full(3, NAN), cost=cost, words6=words6,
                    points=np.zeros((0, 3)), status=4)
    t, p, q, _ = six[best]
    loc = sample(list(zip(WORDS[best], (t, p, q))), alpha, step, max_curv)
    ct, sn = math.cos(theta), math.sin(theta)
    rows = [((ct * x - sn * y) + s[0], (sn * x + ct * y) + s[1], pi2pi(yaw + theta)) for x, y, yaw in loc]
    return dict(word=best, tpq=np.array([t, p, q]), cost=cost, words6=words6,
                points=np.array(rows, np.float64).reshape(-1, 3), status=0)


def cases(z=None):
    """Yield (i, name, start, goal, step, max_curv) of every fixture case."""
    z = load() if z is None else z
    for i, name in enumerate(z["names"]):
        yield i, str(name), tuple(z["start"][i]), tuple(z["goal"][i]), float(z["params"][i, 0]), float(z["params"][i, 1])


def close(a, b, what, rtol=RTOL):
    """|a - b| <= rtol max(1, |b|) elementwise, the NaN pattern exact; returns the worst deviation"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert (np.isnan(a) == np.isnan(b)).all(), what
    m = ~np.isnan(b)
    err = np.abs(a[m] - b[m]) / np.maximum(1.0, np.abs(b[m]))
    worst = float(err.max()) if err.size else 0.0
    assert worst <= rtol, (what, worst)
    return worst


def yaw_close(a, b, what, rtol=RTOL):
    """the difference wrapped to (-pi, pi] within rtol (|yaw| <= pi: max(1, |ref|) <= pi is not used)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    d = a - b
    d = d - 2.0 * PI * np.ceil((d - PI) / (2.0 * PI))
    worst = float(np.abs(d).max()) if d.size else 0.0
    assert worst <= rtol, (what, worst)
    return worst


def rows_close(rows, ref, what, worst=None):
    """rows [n, 3] against ref: the count exact, x and y by close(), yaw by yaw_close(); worst: a dict
    of the worst deviation per column, updated"""
    rows, ref = np.asarray(rows, np.float64).reshape(-1, 3), np.asarray(ref, np.float64).reshape(-1, 3)
    assert len(rows) == len(ref), (what, len(rows), len(ref))
    got = dict(x=close(rows[:, 0], ref[:, 0], what + " x"), y=close(rows[:, 1], ref[:, 1], what + " y"),
               yaw=yaw_close(rows[:, 2], ref[:, 2], what + " yaw"))
    if worst is not None:
        for k, v in got.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return got


def compare_case(z, i, word, tpq, cost, n_points, rows, status, worst=None):
    """One computed pair (the device's, or the restatement's) against fixture case i under the rules of
    this module.  rows: the n_points rows.  Returns True for a fragile case."""
    name = str(z["names"][i])
    s, g = tuple(z["start"][i]), tuple(z["goal"][i])
    step, curv = float(z["params"][i, 0]), float(z["params"][i, 1])
    word, n_points = int(word), int(n_points)
    assert int(status) == 0, (name, status)
    if int(z["count"][i]) == 0:  # the zero-point cases: exact whatever else
        assert n_points == 0 and float(cost) == 0.0 and word == int(z["word"][i]), (name, word, n_points, cost)
        return bool(z["fragile"][i])
    if z["fragile"][i]:
        assert int(z["words_seen"][i]) >> word & 1, (name, word)
        r = restate(s, g, step, curv, force_word=word)
        assert n_points == len(r["points"]), (name, n_points, len(r["points"]))
        rows_close(rows, r["points"], name, worst)
        close(tpq, r["tpq"], name + " tpq")
        close(cost, r["cost"], name + " cost")
        assert float(cost) >= float(z["cost"][i]) - RTOL * max(1.0, abs(float(z["cost"][i]))), name
        return True
    assert word == int(z["word"][i]), (name, word, int(z["word"][i]))
    assert n_points == int(z["count"][i]), (name, n_points, int(z["count"][i]))
    ref = z["words6"][i, word]
    for k, v in zip("tpq", np.asarray(tpq)):
        e = close(v, ref["tpq".index(k)], f"{name} {k}")
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), e)
    e = close(cost, z["cost"][i], name + " cost")
    if worst is not None:
        worst["cost"] = max(worst.get("cost", 0.0), e)
    if z["has_rows"][i]:
        rows_close(rows, seg(z["rows"], z["rows_off"], i), name, worst)
    return False
