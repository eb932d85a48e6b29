"""Generate tests/golden/polycurve.npz by running the REFERENCE's Polynomial and Bezier
(curve_generation/polynomial_curve.py, bezier_curve.py) with pyvista and osqp stubbed, as make_golden.py does.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_polycurve.py

Polynomial cases (start / goal are x, y, yaw in radians, v, a; params are step, max_acc, max_jerk, dt,
t_min, t_max):
  ex{1,2}_{i}_{p}   the consecutive pairs of the two commented pose lists of examples/curve_examples.py:11-15
                    through run()'s v / a heuristic (:177-182), at p = 0: (2, 1.0, 0.5) (the example's own), 1:
                    (0.1, 1.0, 0.5), 2: (0.5, 2.0, 1.0)
  rng_{i}           300 default_rng(5) pairs at (0.1, 1.0, 0.5): x, y in 0..40, yaw in +-pi, v in 0..2, a in +-0.3
  same_pose, start_yaw_back, far_goal, nan_pose, inf_pose, one_candidate, last_candidate, dt_coarse
Per case: t_index (-1: no feasible T), T, the row count, the peaks of |a| and |jerk| of the chosen
candidate, the decision margin (the least |max(peak_a / max_acc, peak_j / max_jerk) - 1| over every candidate
up to and including the chosen one, every candidate where none is chosen), and rows (time, x, y, yaw, v, a,
jerk): all of them for the named cases and the first 24 random ones, else the first, a middle and the last.
Per stored row two flags: the sign of a is safe (row 0, or |v[k] - v[k-1]| > 1e-9 max(1, v[k])), the sign of
jerk is safe (row 0, or the signs of a[k] and a[k-1] are safe and |a[k] - a[k-1]| > 1e-9 max(1, |a[k]|)).
Asserted here, as conditions on the inputs: no margin under 1e-6; at most 1 % of the stored rows have an
unsafe sign, same_pose (all zeros) apart.
Also: run() of the first pose list at (2, 1.0, 0.5) (x, y, yaw), a 5 x 7 time matrix at (0.1, 1.0, 0.5), and
the reference's seconds per generation() on one core of the machine that made the fixture.

Bezier cases (start / goal are x, y, yaw in radians; params are step, offset): the same pose lists at
(0.1, 3.0), 200 default_rng(6) pairs (x, y in 0..40), and n0 (0.05 apart: no point), n1 (0.15 apart: the start
alone), n2, pythagorean ((0,0) -> (3,4): 50 points).  Per case: the count, the four control points, the rows
(x, y) stored as above, and a fragile flag where hypot / step lies within 4 ulp of an integer (asserted: no
random case is)."""
from __future__ import annotations

import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

LIST1 = [(0, 0, 0), (10, 10, -90), (20, 5, 60), (30, 10, 120), (35, -5, 30), (25, -10, -120), (15, -15, 100), (0, -10, -90)]
LIST2 = [(-3, 3, 120), (10, -7, 30), (10, 13, 30), (20, 5, -25), (35, 10, 180), (32, -10, 180), (5, -12, 90)]
PARAMS = [(2.0, 1.0, 0.5), (0.1, 1.0, 0.5), (0.5, 2.0, 1.0)]
N_FULL_RANDOM = 24


def run_states(points):
    """The 5-tuples run() hands to generation() (polynomial_curve.py:177-190)"""
    v = [0]
    for i in range(len(points) - 1):
        v.append(1.0)
    a = [(v[i + 1] - v[i]) / 5 for i in range(len(points) - 1)]
    a.append(0)
    return [(float(p[0]), float(p[1]), float(np.deg2rad(p[2])), float(v[i]), float(a[i])) for i, p in enumerate(points)]


def peaks(gen, s, g, T):
    """(peak |a|, peak |jerk|) of candidate T, from the reference's own Poly"""
    sx, sy, syaw, sv, sa = s
    gx, gy, gyaw, gv, ga = g
    with np.errstate(all="ignore"):
        try:
            px = gen.Poly((sx, sv * math.cos(syaw), sa * math.cos(syaw)), (gx, gv * math.cos(gyaw), ga * math.cos(gyaw)), T)
            py = gen.Poly((sy, sv * math.sin(syaw), sa * math.sin(syaw)), (gy, gv * math.sin(gyaw), ga * math.sin(gyaw)), T)
        except (ValueError, np.linalg.LinAlgError):
            return float("nan"), float("nan")
        t = np.arange(0.0, T + gen.dt, gen.dt)
        return float(np.hypot(px.ddx(t), py.ddx(t)).max()), float(np.hypot(px.dddx(t), py.dddx(t)).max())


def safe_flags(v, a):
    """[n, 2] bool: the sign of a[k] / of jerk[k] does not turn on rounding"""
    n = len(v)
    sa = np.ones(n, bool)
    sj = np.ones(n, bool)
    for k in range(1, n):
        sa[k] = abs(v[k] - v[k - 1]) > 1e-9 * max(1.0, v[k])
    for k in range(1, n):
        sj[k] = sa[k] and sa[k - 1] and abs(a[k] - a[k - 1]) > 1e-9 * max(1.0, abs(a[k]))
    return np.column_stack([sa, sj])


def stored_rows(n, full):
    return np.arange(n) if full else np.unique([0, n // 2, n - 1]) if n else np.zeros(0, np.int64)


def main():
    import_reference()
    from python_motion_planning.curve_generation import Bezier, Polynomial

    def make(p):
        gen = Polynomial(p[0], p[1], p[2])
        gen.dt, gen.t_min, gen.t_max = p[3], p[4], p[5]
        return gen

    nan, inf = float("nan"), float("inf")
    D = (0.1, 1, 30)  # the reference's dt, t_min, t_max
    cases = []  # name, start, goal, params (6), full rows
    for k, lst in enumerate((LIST1, LIST2)):
        st = run_states(lst)
        for p, prm in enumerate(PARAMS):
            for i in range(len(lst) - 1):
                cases.append((f"ex{k + 1}_{i}_{p}", st[i], st[i + 1], prm + D, False))
    n_examples = len(cases)
    # last_candidate: step 1 has candidates T = 1 .. 29; the limits are set below between the peaks of T = 28
    # and of T = 29
    lc_s, lc_g = (0.0, 0.0, 0.3, 0.5, 0.0), (30.0, 20.0, 1.0, 1.0, 0.0)
    probe = make((1.0, 1.0, 1.0) + D)
    pk = np.array([peaks(probe, lc_s, lc_g, T) for T in np.arange(1, 30, 1.0)])
    assert len(pk) == 29 and pk[28, 0] < pk[:28, 0].min()
    lc_acc = float(0.5 * (pk[28, 0] + pk[:28, 0].min()))
    named = [
        ("same_pose", (0.0, 0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0, 0.0), (0.1, 1.0, 0.5) + D),
        ("start_yaw_back", (0.0, 0.0, 2.5, 0.0, 0.0), (10.0, 10.0, 0.0, 1.0, 0.2), (2.0, 1.0, 0.5) + D),
        ("far_goal", (0.0, 0.0, 0.0, 0.0, 0.0), (1e6, 0.0, 0.0, 1.0, 0.0), (0.1, 1.0, 0.5) + D),
        ("nan_pose", (0.0, nan, 0.0, 0.0, 0.0), (10.0, 10.0, 0.0, 1.0, 0.0), (0.1, 1.0, 0.5) + D),
        ("inf_pose", (0.0, 0.0, 0.0, 0.0, 0.0), (inf, 10.0, 0.0, 1.0, 0.0), (0.1, 1.0, 0.5) + D),
        ("one_candidate", (0.0, 0.0, 0.3, 1.0, 0.0), (0.957, 0.297, 0.3, 1.0, 0.0), (29.0, 1.0, 0.5) + D),
        ("last_candidate", lc_s, lc_g, (1.0, lc_acc, 10.0 * float(pk[:, 1].max())) + D),
        ("dt_coarse", run_states(LIST1)[1], run_states(LIST1)[2], (0.5, 1.0, 0.5, 0.5, 1, 30)),
    ]
    cases += [c + (True,) for c in named]
    n_named = len(named)
    rng = np.random.default_rng(5)
    for i in range(300):
        s = (rng.uniform(0, 40), rng.uniform(0, 40), rng.uniform(-math.pi, math.pi), rng.uniform(0, 2), rng.uniform(-0.3, 0.3))
        g = (rng.uniform(0, 40), rng.uniform(0, 40), rng.uniform(-math.pi, math.pi), rng.uniform(0, 2), rng.uniform(-0.3, 0.3))
        cases.append((f"rng_{i}", tuple(map(float, s)), tuple(map(float, g)), (0.1, 1.0, 0.5) + D, i < N_FULL_RANDOM))

    N = len(cases)
    t_index = np.zeros(N, np.int32)
    Tc = np.zeros(N)
    count = np.zeros(N, np.int32)
    peak = np.full((N, 2), np.nan)
    margin = np.full(N, np.inf)
    rows, idxs, safes, secs = [], [], [], []
    trajs = {}
    for i, (name, s, g, prm, full) in enumerate(cases):
        gen = make(prm)
        assert str(gen) == "Quintic Polynomial Curve"
        with np.errstate(all="ignore"):
            t0 = time.perf_counter()
            tr = gen.generation(s, g)
            secs.append(time.perf_counter() - t0)
            seen = []
            gen.Poly = lambda s0, s1, t, _P=Polynomial.Poly: (seen.append(float(t)), _P(s0, s1, t))[1]
            assert gen.generation(s, g).size == tr.size  # again, recording each candidate's T
            del gen.Poly
        cand = np.arange(gen.t_min, gen.t_max, gen.step)
        n = tr.size
        count[i] = n
        if n:
            k = len(seen) // 2 - 1  # two Poly per candidate tried; the last pair is the chosen one's
            assert seen[-1] == cand[k] and n == len(np.arange(0.0, cand[k] + gen.dt, gen.dt)), name
            t_index[i], Tc[i] = k, cand[k]
            peak[i] = max(np.abs(tr.a)), max(np.abs(tr.jerk))
            upto = cand[: k + 1]
        else:
            t_index[i], Tc[i] = -1, inf
            upto = cand
        pk_i = np.array([peaks(gen, s, g, T) for T in upto]).reshape(-1, 2)
        ratio = np.maximum(pk_i[:, 0] / prm[1], pk_i[:, 1] / prm[2])
        ok = np.isfinite(ratio)
        if ok.any():
            margin[i] = float(np.abs(ratio[ok] - 1.0).min())
        if n:  # the peaks above are the trajectory's, and they decide as the reference decided
            assert abs(pk_i[-1, 0] - peak[i, 0]) <= 1e-9 * max(1.0, peak[i, 0]), name
            assert ratio[-1] <= 1.0 and (ratio[:-1][ok[:-1]] > 1.0).all(), name
        R = np.column_stack([tr.time, tr.x, tr.y, tr.yaw, tr.v, tr.a, tr.jerk]).reshape(-1, 7)
        sel = stored_rows(n, full)
        rows.append(R[sel])
        idxs.append(sel)
        safes.append(safe_flags(R[:, 4], R[:, 5])[sel] if n else np.zeros((0, 2), bool))
        if name.startswith("ex1_") and name.endswith("_0"):
            trajs[name] = R
    by = {c[0]: k for k, c in enumerate(cases)}
    assert count[by["same_pose"]] == 11 and t_index[by["same_pose"]] == 0 and not rows[by["same_pose"]][:, 1:].any()
    assert count[by["start_yaw_back"]] == 131 and rows[by["start_yaw_back"]][0, 3] == 0.0
    assert math.copysign(1.0, rows[by["start_yaw_back"]][0, 3]) == 1.0
    for name in ("far_goal", "nan_pose", "inf_pose"):
        assert count[by[name]] == 0 and t_index[by[name]] == -1, name
    assert t_index[by["one_candidate"]] == 0 and count[by["one_candidate"]] == 11
    assert t_index[by["last_candidate"]] == 28 and count[by["last_candidate"]] in (291, 292), count[by["last_candidate"]]
    assert count[by["dt_coarse"]] > 0
    assert margin.min() >= 1e-6, (margin.min(), cases[int(margin.argmin())][0])
    flags = np.concatenate([f for k, f in enumerate(safes) if cases[k][0] != "same_pose"])
    assert (~flags).mean() <= 0.01, (~flags).mean()

    # run() of the first list at the example's own parameters: the segments in order (:186-195)
    run_path = np.concatenate([trajs[f"ex1_{i}_0"][:, 1:4] for i in range(len(LIST1) - 1)])

    # 5 x 7 time matrix
    def pose5(n):
        return np.column_stack([rng.uniform(0, 40, n), rng.uniform(0, 40, n), rng.uniform(-math.pi, math.pi, n),
                                rng.uniform(0, 2, n), rng.uniform(-0.3, 0.3, n)])

    tm_s, tm_g = pose5(5), pose5(7)
    tm_prm = (0.1, 1.0, 0.5) + D
    gen = make(tm_prm)
    cand = np.arange(gen.t_min, gen.t_max, gen.step)
    tm_T, tm_idx = np.full((5, 7), inf), np.full((5, 7), -1, np.int32)
    tm_margin = inf
    for a in range(5):
        for b in range(7):
            seen = []
            gen.Poly = lambda s0, s1, t, _P=Polynomial.Poly: (seen.append(float(t)), _P(s0, s1, t))[1]
            tr = gen.generation(tuple(tm_s[a]), tuple(tm_g[b]))
            del gen.Poly
            if tr.size:
                k = len(seen) // 2 - 1
                assert seen[-1] == cand[k] and len(np.arange(0.0, cand[k] + gen.dt, gen.dt)) == tr.size
                tm_T[a, b], tm_idx[a, b] = cand[k], k
            upto = cand[: tm_idx[a, b] + 1] if tr.size else cand
            pk_i = np.array([peaks(gen, tuple(tm_s[a]), tuple(tm_g[b]), T) for T in upto])
            tm_margin = min(tm_margin, float(np.abs(np.maximum(pk_i[:, 0] / 1.0, pk_i[:, 1] / 0.5) - 1.0).min()))
    assert tm_margin >= 1e-6, tm_margin

    off = np.zeros(N + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    out = dict(names=np.array([c[0] for c in cases]), start=np.array([c[1] for c in cases], np.float64),
               goal=np.array([c[2] for c in cases], np.float64), params=np.array([c[3] for c in cases], np.float64),
               t_index=t_index, T=Tc, count=count, peak=peak, margin=margin, rows=np.concatenate(rows),
               rows_idx=np.concatenate(idxs).astype(np.int32), rows_safe=np.concatenate(safes), rows_off=off,
               full=np.array([c[4] for c in cases]), n_examples=np.int32(n_examples), n_named=np.int32(n_named),
               run_points=np.array(LIST1, np.float64), run_params=np.array(PARAMS[0]), run_path=run_path,
               tm_start=tm_s, tm_goal=tm_g, tm_params=np.array(tm_prm, np.float64), tm_T=tm_T, tm_index=tm_idx,
               ref_seconds_per_generation=np.float64(np.median([t for t, c in zip(secs, cases) if c[3][0] == 0.1 and c[0][:2] in ("ex", "rn")])))

    # ---- Bezier ----
    def rad(p):
        return (float(p[0]), float(p[1]), float(np.deg2rad(p[2])))

    BP = (0.1, 3.0)
    bcases = []  # name, start, goal, params, full rows, expected count
    for k, lst in enumerate((LIST1, LIST2)):
        for i in range(len(lst) - 1):
            bcases.append((f"ex{k + 1}_{i}", rad(lst[i]), rad(lst[i + 1]), BP, True, None))
    bcases += [
        ("n0", (1.0, 2.0, 0.3), (1.03, 2.04, -1.0), BP, True, 0),
        ("n1", (1.0, 2.0, 0.3), (1.09, 2.12, -1.0), BP, True, 1),
        ("n2", (1.0, 2.0, 0.3), (1.15, 2.2, -1.0), BP, True, 2),
        ("pythagorean", (0.0, 0.0, 0.0), (3.0, 4.0, 1.0), BP, True, 50),
    ]
    nb_named = len(bcases)
    brng = np.random.default_rng(6)
    for i in range(200):
        s = (brng.uniform(0, 40), brng.uniform(0, 40), brng.uniform(-math.pi, math.pi))
        g = (brng.uniform(0, 40), brng.uniform(0, 40), brng.uniform(-math.pi, math.pi))
        bcases.append((f"rng_{i}", tuple(map(float, s)), tuple(map(float, g)), BP, i < N_FULL_RANDOM, None))
    NB = len(bcases)
    bcount = np.zeros(NB, np.int32)
    bctrl = np.zeros((NB, 4, 2))
    bfragile = np.zeros(NB, bool)
    brows, bidx, bsecs = [], [], []
    for i, (name, s, g, prm, full, want) in enumerate(bcases):
        gen = Bezier(*prm)
        assert str(gen) == "Bezier Curve"
        t0 = time.perf_counter()
        pts, ctrl = gen.generation(s, g)
        bsecs.append(time.perf_counter() - t0)
        bcount[i] = len(pts)
        if want is not None:
            assert len(pts) == want, (name, len(pts), want)
        bctrl[i] = np.array(ctrl, np.float64)
        q = float(np.hypot(s[0] - g[0], s[1] - g[1]) / prm[0])
        bfragile[i] = abs(q - round(q)) <= 4 * np.spacing(q)
        R = np.array(pts, np.float64).reshape(-1, 2)
        sel = stored_rows(len(R), full)
        brows.append(R[sel])
        bidx.append(sel)
    bby = {c[0]: k for k, c in enumerate(bcases)}
    assert np.array_equal(brows[bby["n1"]][0], [1.0, 2.0])
    assert not bfragile[nb_named:].any()
    gen = Bezier(*BP)
    brun = gen_run_path(gen, LIST1)
    boff = np.zeros(NB + 1, np.int64)
    boff[1:] = np.cumsum([len(r) for r in brows])
    out.update(b_names=np.array([c[0] for c in bcases]), b_start=np.array([c[1] for c in bcases], np.float64),
               b_goal=np.array([c[2] for c in bcases], np.float64), b_params=np.array([c[3] for c in bcases], np.float64),
               b_count=bcount, b_control=bctrl, b_fragile=bfragile, b_rows=np.concatenate(brows),
               b_rows_idx=np.concatenate(bidx).astype(np.int32), b_rows_off=boff, b_full=np.array([c[4] for c in bcases]),
               b_n_named=np.int32(nb_named), b_run_points=np.array(LIST1, np.float64), b_run_params=np.array(BP),
               b_run_path=brun, b_ref_seconds_per_generation=np.float64(np.median(bsecs)))

    fn = os.path.join(HERE, "polycurve.npz")
    np.savez_compressed(fn, **out)
    assert os.path.getsize(fn) < 500_000, os.path.getsize(fn)
    ok = t_index >= 0
    print("polynomial cases", N, "examples", n_examples, "named", n_named, "t_index", int(t_index[ok].min()), "..",
          int(t_index[ok].max()), "none", int((~ok).sum()), "counts", int(count[ok].min()), "..", int(count.max()),
          "least margin", float(margin.min()), "matrix margin", tm_margin, "unsafe rows", float((~flags).mean()),
          "rows stored", len(out["rows"]), "reference s/generation (median)", float(out["ref_seconds_per_generation"]))
    print("bezier cases", NB, "named", nb_named, "counts", int(bcount.min()), "..", int(bcount.max()), "fragile",
          [bcases[i][0] for i in np.nonzero(bfragile)[0]], "rows stored", len(out["b_rows"]),
          "reference s/generation (median)", float(np.median(bsecs)), "bytes", os.path.getsize(fn))


def gen_run_path(gen, points):
    """run()'s path of a Bezier generator (bezier_curve.py:102-111), without the plot"""
    path = []
    for i in range(len(points) - 1):
        pts, _ = gen.generation((points[i][0], points[i][1], np.deg2rad(points[i][2])),
                                (points[i + 1][0], points[i + 1][1], np.deg2rad(points[i + 1][2])))
        path.extend(pts)
    return np.array(path, np.float64).reshape(-1, 2)


if __name__ == "__main__":
    main()
