"""Generate tests/golden/bspline.npz by running the REFERENCE's BSpline, BSpline3D and CubicSpline
(curve_generation/bspline_curve.py, bspline_curve3d.py, cubic_spline.py) with pyvista and osqp stubbed, as
make_golden.py does.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_bspline.py

B-spline cases (points, step, k, param_mode, spline_mode, 2D or 3D class):
  ex{1,2}_k{k}_{pm}_{sm}  the two commented pose lists of examples/curve_examples.py:11-15 (3-tuples: the 2D class
                          cuts them to x, y) at step 0.01, k = 2..5, the three param_modes, both spline_modes
  pso_{i}                 300 PSO-shaped lists (pso.py:150-197): (5, 5), five points of sorted integer x in 5..45
                          and sorted integer y in 5..25 from default_rng(11), (45, 25), de-duplicated in order;
                          k = 4, step 0.01, centripetal interpolation (PSO's own generator)
  len2_k1, min_k{1..5} (k + 1 points: the smallest system that can be solved), len4_k4 and len2_k4 (n <= k:
  singular), len33, len64_k3, len64_k5 (random walks), repeat (a repeated consecutive waypoint: singular),
  collinear, all_equal (2D: every value NaN) and all_equal_3d (parameters 0, singular), step06 (T = 1),
  step15 (2D: IndexError, status 5 here) and step15_3d (two rows), T1, T2, T64, T65 (the sampler's rounds),
  approx_min_k{1..5} (k + 2 points), approx_33, and in 3D: d3_8 and d3_64 in both modes, d3_repeat, d2_in_3d.
Per case: status (0, 4 = LinAlgError, 5 = IndexError), the parameters, knots and control points generation()
was given, T, the rows (all of them for the named cases and the first 24 pso ones, else the first, a middle and
the last), the length (bspline_checks.polyline_length of the reference's rows), cond (of the collocation
matrix, or of N_^T N_), and restate_dev: the deviation of bspline_checks.bs_restate's control points and rows
from the reference's, relative to max(1, max |coordinate|).
Asserted here, as conditions on the inputs: every interpolation case that does not raise has cond <= 1e3,
every approximation case cond <= 1e4; every raising case has n <= k or a repeated consecutive waypoint; no
pso case raises; the triangular basis scheme gives the bits of the reference's recursion on every collocation
matrix; run() returns the staged rows.

Cubic-spline cases (points, step): the two example lists at steps 0.1 and 0.5, 200 default_rng(12) random
walks of 2..64 points, two, three_h_gt1, three_h_lt1, repeat (the full count of NaN rows), pythagorean ((0, 0)
-> (3, 4) at 0.1: exactly 50 rows), inf_coord (np.arange raises: status 4).  Per case: the count, s[-1], rows
(x, y, yaw, dx, dy; stored as above), a fragile flag where s[-1] / step lies within 4 ulp of an integer.
Asserted: no random case is fragile; no sample time reaches s[-1]; at most 1 % of the stored rows have
hypot(dx, dy) < 1e-9 (the rows whose yaw a comparison skips).

Also: bs_rtol and cs_rtol = 64 x the worst restate_dev of each family, and the reference's seconds per run() on
one core of the machine that made the fixture (pso-shaped, the 64-point lists, the cubic spline)."""
from __future__ import annotations

import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402
import bspline_checks as bc  # noqa: E402

LIST1 = [(0, 0, 0), (10, 10, -90), (20, 5, 60), (30, 10, 120), (35, -5, 30), (25, -10, -120), (15, -15, 100), (0, -10, -90)]
LIST2 = [(-3, 3, 120), (10, -7, 30), (10, 13, 30), (20, 5, -25), (35, 10, 180), (32, -10, 180), (5, -12, 90)]
N_FULL_RANDOM = 24
PM, SM = bc.PARAM_MODES, bc.SPLINE_MODES


def stored_rows(n, full):
    if full or n <= 3:
        return np.arange(n, dtype=np.int32)
    return np.array([0, n // 2, n - 1], np.int32)


def walk(rng, n, dim, lo=0.5, hi=3.0):
    """A random walk of n points: steps of length lo..hi in a direction that turns by at most 60 degrees"""
    p = np.zeros((n, dim))
    ang, z = rng.uniform(-math.pi, math.pi), 0.0
    for i in range(1, n):
        ang += rng.uniform(-math.pi / 3, math.pi / 3)
        r = rng.uniform(lo, hi)
        p[i, 0] = p[i - 1, 0] + r * math.cos(ang)
        p[i, 1] = p[i - 1, 1] + r * math.sin(ang)
        if dim == 3:
            p[i, 2] = p[i - 1, 2] + rng.uniform(-1.0, 1.0)
    return [tuple(map(float, row)) for row in p]


def pso_list(rng):
    xs = sorted(int(v) for v in rng.integers(5, 46, 5))
    ys = sorted(int(v) for v in rng.integers(5, 26, 5))
    points = [(5, 5)] + list(zip(xs, ys)) + [(45, 25)]
    return sorted(set(points), key=points.index)


def run_bspline(pmp, case):
    """The reference's run(), stage by stage.  Returns the fixture's record of it."""
    name, pts, step, k, pm, sm, three_d = case[:7]
    Cls = pmp.curve_generation.BSpline3D if three_d else pmp.curve_generation.BSpline
    gen = Cls(step, k, pm, sm)
    points = [tuple(p) for p in pts] if three_d else [(p[0], p[1]) for p in pts]
    P = np.array(points, np.float64)
    n, dim = P.shape
    T = bc.n_samples(step, three_d)
    rec = dict(status=bc.ST_OK, T=T, dim=dim, points=P, cond=float("nan"))
    with np.errstate(all="ignore"):
        params = gen.paramSelection(points)
        knot = gen.knotGeneration(params, n)
        par0, knot0 = np.array(params), np.array(knot)
        nc = n if sm == "interpolation" else n - 1
        finite = np.isfinite(par0).all() and np.isfinite(knot0).all()
        if sm == "interpolation":
            N = bc.bs_matrix(par0, knot0, n, n, k)
            N[n - 1, n - 1] = 1
            if finite:  # the claim csrc/bspline.hip rests on: the triangular scheme has the recursion's bits
                R = np.array([[gen.baseFunction(j, k, params[i], knot) for j in range(n)] for i in range(n)])
                R[n - 1, n - 1] = 1
                assert np.array_equal(N, R), name
                rec["cond"] = float(np.linalg.cond(N))
        elif finite:
            N = bc.bs_matrix(par0, knot0, n, n - 1, k)
            N_ = N[1 : n - 1, 1 : n - 2]
            rec["cond"] = float(np.linalg.cond(N_.T @ N_)) if N_.size else 1.0
        try:
            if sm == "interpolation":
                ctrl = gen.interpolation(points, params, knot)
            else:
                ctrl = gen.approximation(points, params, knot)
                new_points = ctrl.tolist() if three_d else [(ctrl[i][0], ctrl[i][1]) for i in range(len(ctrl))]
                params = gen.paramSelection(new_points)
                knot = gen.knotGeneration(params, len(ctrl))
        except np.linalg.LinAlgError:
            rec.update(status=bc.ST_LINALG, params=par0, knot=knot0, control=np.full((nc, dim), np.nan), n_control=nc,
                       rows=np.zeros((0, dim)), length=float("nan"))
            try:
                gen.run(pts, display=False)
                raise AssertionError(name + ": run() did not raise")
            except np.linalg.LinAlgError:
                pass
            return rec
        rec.update(params=np.array(params), knot=np.array(knot), control=np.array(ctrl, np.float64), n_control=len(ctrl))
        try:
            rows = gen.generation(np.linspace(0, 1, T), k, knot, ctrl)
        except IndexError:
            assert T == 0, name
            rec.update(status=bc.ST_INDEX, rows=np.zeros((0, dim)), length=float("nan"))
            try:
                gen.run(pts, display=False)
                raise AssertionError(name + ": run() did not raise")
            except IndexError:
                pass
            return rec
        rows = np.array(rows, np.float64).reshape(T, dim)
        t0 = time.perf_counter()
        path = gen.run(pts, display=False)
        rec["seconds"] = time.perf_counter() - t0
        assert np.array_equal(np.array(path, np.float64).reshape(T, dim), rows, equal_nan=True), name
        assert all(isinstance(v, float) for v in path[0]) and isinstance(path[0], tuple)
        rec.update(rows=rows, length=bc.polyline_length(rows, three_d))
    return rec


def cubic_reference(gen, points):
    """run()'s path of a CubicSpline generator (cubic_spline.py:94-111), without the plots: (s, rows)"""
    x_list = [p[0] for p in points]
    y_list = [p[1] for p in points]
    ds = [math.hypot(a, b) for a, b in zip(np.diff(x_list), np.diff(y_list))]
    s = [0]
    s.extend(np.cumsum(ds))
    t = np.arange(0, s[-1], gen.step)
    px, dpx = gen.spline(s, x_list, t)
    py, dpy = gen.spline(s, y_list, t)
    yaw = [math.atan2(dpy[i], dpx[i]) for i in range(len(dpx))]
    assert len(px) == len(t)
    return np.array(s, np.float64), np.array([px, py, yaw, dpx, dpy], np.float64).T.reshape(-1, 5), t


def main():
    pmp = import_reference()
    out = {}
    # ---- B-spline ----
    cases = []  # name, points, step, k, param_mode, spline_mode, three_d, full rows
    for li, lst in enumerate((LIST1, LIST2)):
        for k in (2, 3, 4, 5):
            for pm in PM:
                for sm in SM:
                    cases.append((f"ex{li + 1}_k{k}_{pm}_{sm}", lst, 0.01, k, pm, sm, False, True))
    rng = np.random.default_rng(11)
    n_ex = len(cases)
    for i in range(300):
        cases.append((f"pso_{i}", pso_list(rng), 0.01, 4, PM[0], SM[0], False, i < N_FULL_RANDOM))
    n_pso = 300
    wr = np.random.default_rng(13)
    seven = [(5, 5), (9, 6), (14, 11), (22, 12), (30, 18), (41, 21), (45, 25)]
    named = [("len2_k1", [(0, 0), (3, 4)], 0.01, 1)]
    named += [(f"min_k{k}", walk(wr, k + 1, 2), 0.01, k) for k in range(1, 6)]
    named += [("len4_k4", walk(wr, 4, 2), 0.01, 4), ("len2_k4", [(0, 0), (3, 4)], 0.01, 4),
              ("len33", walk(wr, 33, 2), 0.01, 3), ("len64_k3", walk(wr, 64, 2), 0.01, 3),
              ("len64_k5", walk(wr, 64, 2), 0.01, 5),
              ("repeat", [(0, 0), (2, 1), (4, 3), (4, 3), (7, 4), (9, 8), (12, 9)], 0.01, 3),
              ("collinear", [(float(i * i) / 4, float(i * i) / 2) for i in range(8)], 0.01, 3),
              ("all_equal", [(2.0, 3.0)] * 6, 0.01, 3), ("step06", seven, 0.6, 4), ("step15", seven, 1.5, 4),
              ("T1", seven, 1.0, 4), ("T2", seven, 0.5, 4), ("T64", seven, 1 / 64, 4), ("T65", seven, 0.0153, 4)]
    for name, pts, step, k in named:
        cases.append((name, pts, step, k, PM[0], SM[0], False, True))
    cases += [(f"approx_min_k{k}", walk(wr, k + 2, 2), 0.01, k, PM[0], SM[1], False, True) for k in range(1, 6)]
    cases.append(("approx_33", walk(wr, 33, 2), 0.01, 4, PM[1], SM[1], False, True))
    d3_8, d3_64 = walk(wr, 8, 3), walk(wr, 64, 3)
    for sm in SM:
        cases.append((f"d3_8_{sm}", d3_8, 0.01, 3, PM[0], sm, True, True))
        cases.append((f"d3_64_{sm}", d3_64, 0.01, 3, PM[1], sm, True, True))
    cases += [("d3_repeat", d3_8[:4] + d3_8[3:], 0.01, 3, PM[0], SM[0], True, True),
              ("all_equal_3d", [(2.0, 3.0, 1.0)] * 6, 0.01, 3, PM[0], SM[0], True, True),
              ("step15_3d", [p + (1.0,) for p in seven], 1.5, 4, PM[0], SM[0], True, True),
              ("d2_in_3d", seven, 0.01, 4, PM[1], SM[0], True, True)]
    NB = len(cases)
    recs = []
    for c in cases:
        r = run_bspline(pmp, c)
        name, pts, step, k, pm, sm, three_d, full = c
        n = len(r["points"])
        if r["status"] == bc.ST_LINALG:
            rep = any(np.array_equal(a, b) for a, b in zip(r["points"][:-1], r["points"][1:]))
            assert n <= k or rep, name
        elif r["status"] == bc.ST_OK and np.isfinite(r["cond"]):
            assert r["cond"] <= (1e3 if sm == SM[0] else 1e4), (name, r["cond"])
        # the restatement against the reference
        rs = bc.bs_restate(r["points"], step, k, pm, sm, three_d)
        assert rs["status"] == r["status"] and rs["T"] == r["T"], (name, rs["status"], r["status"])
        dev = 0.0
        if r["status"] == bc.ST_OK:
            sc = bc.scale_of(r["points"])
            assert rs["n_control"] == r["n_control"]
            dev = max(bc.deviation(rs["control"], r["control"], sc), bc.deviation(rs["rows"], r["rows"], sc),
                      bc.deviation(rs["params"], r["params"], 1.0), bc.deviation(rs["knot"], r["knot"], 1.0),
                      bc.deviation([rs["length"]], [r["length"]], sc))
            assert math.isfinite(dev), name
        r["restate_dev"] = dev
        r["idx"] = stored_rows(len(r["rows"]), full)
        recs.append(r)
    by = {c[0]: i for i, c in enumerate(cases)}
    assert all(recs[n_ex + i]["status"] == bc.ST_OK for i in range(n_pso))
    assert recs[by["all_equal"]]["status"] == bc.ST_OK and np.isnan(recs[by["all_equal"]]["rows"]).all()
    assert np.isnan(recs[by["all_equal"]]["control"]).all()
    for nm in ("len4_k4", "len2_k4", "repeat", "d3_repeat", "all_equal_3d"):
        assert recs[by[nm]]["status"] == bc.ST_LINALG, nm
    assert recs[by["step15"]]["status"] == bc.ST_INDEX and len(recs[by["step15_3d"]]["rows"]) == 2
    assert len(recs[by["step06"]]["rows"]) == 1 and [recs[by[f"T{t}"]]["T"] for t in (1, 2, 64, 65)] == [1, 2, 64, 65]

    def pack(key, dtype=np.float64):
        arrs = [np.asarray(r[key], dtype).ravel() for r in recs]
        off = np.zeros(NB + 1, np.int64)
        off[1:] = np.cumsum([len(a) for a in arrs])
        return np.concatenate(arrs), off

    for r in recs:
        r["rows_sel"] = r["rows"][r["idx"]]
    worst = max(r["restate_dev"] for r in recs)
    out.update(bs_names=np.array([c[0] for c in cases]), bs_dim=np.array([r["dim"] for r in recs], np.int32),
               bs_k=np.array([c[3] for c in cases], np.int32), bs_step=np.array([c[2] for c in cases], np.float64),
               bs_pm=np.array([PM.index(c[4]) for c in cases], np.int32), bs_sm=np.array([SM.index(c[5]) for c in cases], np.int32),
               bs_3d=np.array([c[6] for c in cases]), bs_full=np.array([c[7] for c in cases]),
               bs_status=np.array([r["status"] for r in recs], np.int32), bs_nc=np.array([r["n_control"] for r in recs], np.int32),
               bs_T=np.array([r["T"] for r in recs], np.int32), bs_length=np.array([r["length"] for r in recs], np.float64),
               bs_restate_dev=np.array([r["restate_dev"] for r in recs]), bs_cond=np.array([r["cond"] for r in recs]),
               bs_n_examples=np.int32(n_ex), bs_n_pso=np.int32(n_pso), bs_rtol=np.float64(64 * worst))
    for key, short, name in (("points", "pts", "pts"), ("params", "par", "params"), ("knot", "knot", "knot"),
                             ("control", "ctl", "control"), ("rows_sel", "rows", "rows")):
        out["bs_" + name], out["bs_" + short + "_off"] = pack(key)
    flat, off = pack("idx", np.int32)
    out.update(bs_rows_idx=flat, bs_idx_off=off)
    secs = [r["seconds"] for r in recs[n_ex : n_ex + n_pso]]
    out["bs_ref_seconds_per_run_pso"] = np.float64(np.median(secs))
    out["bs_ref_seconds_per_run_64"] = np.float64(recs[by["len64_k3"]]["seconds"])

    # ---- cubic spline ----
    CubicSpline = pmp.curve_generation.CubicSpline
    ccases = []  # name, points, step, full
    for li, lst in enumerate((LIST1, LIST2)):
        for step in (0.1, 0.5):
            ccases.append((f"ex{li + 1}_{step}", [(float(p[0]), float(p[1])) for p in lst], step, step == 0.5))
    ccases += [("two", [(1.0, 2.0), (4.0, 3.0)], 0.1, True),
               ("three_h_gt1", [(0.0, 0.0), (3.0, 1.0), (4.0, 4.0)], 0.1, True),
               ("three_h_lt1", [(0.0, 0.0), (0.4, 0.3), (2.0, 1.0)], 0.1, True),
               ("repeat", [(0.0, 0.0), (2.0, 1.0), (2.0, 1.0), (4.0, 0.0), (5.0, 2.0)], 0.1, True),
               ("pythagorean", [(0.0, 0.0), (3.0, 4.0)], 0.1, True),
               ("inf_coord", [(0.0, 0.0), (float("inf"), 1.0), (2.0, 2.0)], 0.1, True)]
    nc_named = len(ccases)
    crng = np.random.default_rng(12)
    for i in range(200):
        n = int(crng.integers(2, 65))
        ccases.append((f"rng_{i}", [p[:2] for p in walk(crng, n, 2)], float(crng.choice([0.1, 0.25, 0.5])), i < N_FULL_RANDOM))
    NC = len(ccases)
    crecs, csecs = [], []
    for name, pts, step, full in ccases:
        gen = CubicSpline(step)
        assert str(gen) == "Cubic Spline" and gen.generation((0, 0, 0), (1, 1, 1)) is None
        rec = dict(points=np.array(pts, np.float64), status=bc.ST_OK, fragile=False, dev=0.0)
        with np.errstate(all="ignore"):
            try:
                t0 = time.perf_counter()
                s, rows, t = cubic_reference(gen, pts)
                csecs.append(time.perf_counter() - t0)
            except ValueError:
                rec.update(status=bc.ST_LINALG, count=0, rows=np.zeros((0, 5)), arc=float("inf"), idx=np.zeros(0, np.int32))
                st, cnt, _ = bc.cs_restate(pts, step)
                assert st == bc.ST_LINALG
                crecs.append(rec)
                continue
            q = float(s[-1] / step)
            rec.update(count=len(rows), rows=rows, arc=float(s[-1]), fragile=bool(abs(q - round(q)) <= 4 * np.spacing(q)))
            assert len(rows) == 0 or t[-1] < s[-1], name
            assert np.array_equal(s, bc.cs_table(pts)), name
            st, cnt, rr = bc.cs_restate(pts, step)
            assert st == bc.ST_OK and cnt == len(rows), (name, cnt, len(rows))
            rec["dev"], _ = bc.cs_deviation(rr, rows, bc.scale_of(pts))
            assert math.isfinite(rec["dev"]), name
            rec["idx"] = stored_rows(len(rows), full)
        crecs.append(rec)
    cby = {c[0]: i for i, c in enumerate(ccases)}
    assert crecs[cby["pythagorean"]]["count"] == 50
    rp = crecs[cby["repeat"]]
    assert rp["count"] == math.ceil(rp["arc"] / 0.1) and np.isnan(rp["rows"][:, :3]).all()
    assert crecs[cby["inf_coord"]]["status"] == bc.ST_LINALG
    assert not any(r["fragile"] for r in crecs[nc_named:])
    sel = [r["rows"][r["idx"]] for r in crecs]
    allrows = np.concatenate(sel)
    okrow = ~np.isnan(allrows[:, 0])
    skipped = okrow & (np.hypot(allrows[:, 3], allrows[:, 4]) < 1e-9)
    assert skipped.sum() <= 0.01 * len(allrows), (int(skipped.sum()), len(allrows))

    def cpack(arrs, dtype=np.float64):
        arrs = [np.asarray(a, dtype).ravel() for a in arrs]
        off = np.zeros(NC + 1, np.int64)
        off[1:] = np.cumsum([len(a) for a in arrs])
        return np.concatenate(arrs), off

    cworst = max(r["dev"] for r in crecs)
    out.update(cs_names=np.array([c[0] for c in ccases]), cs_step=np.array([c[2] for c in ccases], np.float64),
               cs_status=np.array([r["status"] for r in crecs], np.int32), cs_count=np.array([r["count"] for r in crecs], np.int32),
               cs_fragile=np.array([r["fragile"] for r in crecs]), cs_arc=np.array([r["arc"] for r in crecs], np.float64),
               cs_restate_dev=np.array([r["dev"] for r in crecs]), cs_n_named=np.int32(nc_named), cs_rtol=np.float64(64 * cworst),
               cs_ref_seconds_per_run=np.float64(np.median(csecs)))
    out["cs_pts"], out["cs_pts_off"] = cpack([r["points"] for r in crecs])
    out["cs_rows"], out["cs_rows_off"] = cpack(sel)
    out["cs_rows_idx"], out["cs_idx_off"] = cpack([r["idx"] for r in crecs], np.int32)

    fn = os.path.join(HERE, "bspline.npz")
    np.savez_compressed(fn, **out)
    assert os.path.getsize(fn) < 900_000, os.path.getsize(fn)
    conds = np.array([r["cond"] for r in recs])
    print("bspline cases", NB, "statuses", np.bincount(out["bs_status"]).tolist(), "worst restate_dev", worst, "bs_rtol",
          float(out["bs_rtol"]), "cond pso", float(np.nanmax(conds[n_ex : n_ex + n_pso])), "cond all",
          float(np.nanmax(conds)), "ref s/run pso", float(out["bs_ref_seconds_per_run_pso"]), "64",
          float(out["bs_ref_seconds_per_run_64"]))
    print("cubic cases", NC, "counts", int(out["cs_count"].min()), "..", int(out["cs_count"].max()), "worst dev", cworst,
          "cs_rtol", float(out["cs_rtol"]), "fragile", [ccases[i][0] for i in np.nonzero(out["cs_fragile"])[0]],
          "skipped yaw rows", int(skipped.sum()), "of", len(allrows), "ref s/run", float(out["cs_ref_seconds_per_run"]),
          "bytes", os.path.getsize(fn))


if __name__ == "__main__":
    main()
