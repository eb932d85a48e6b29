#!/usr/bin/env python3
"""Pairs/s, segments/s, points/s and store bandwidth of the curve kernels (dubins.hip, reeds_shepp.hip,
polycurve.hip, bspline.hip).

    python tools/curve_rate.py --kind dubins|reeds_shepp|polynomial|bezier|bspline|cubic_spline [--matrix 1024] [--segments 65536] [--warmup 3] [--repeats 9]
                               [--out FILE] [--reference-src DIR [--reference-pairs 200]]

Poses are default_rng(0): x, y in 0..40, yaw in -pi..pi; step 0.1, max_curv 0.25
(examples/curve_examples.py:27).  Per repeat, between two device events each:
(dubins shown; reeds_shepp: batch.reeds_shepp_*, pmp_reeds_shepp_batch without slot_costs, ReedsShepp;
polynomial: states with v in 0..2 and a in -0.3..0.3, step 0.1, max_acc 1.0, max_jerk 0.5, batch.polynomial_batch /
polynomial_time_matrix, pmp_polycurve_batch, 56 B a row, Polynomial; bezier: step 0.1, offset 3.0,
batch.bezier_batch, pmp_bezier_batch, 16 B a row, Bezier, no matrix leg)
  cost_matrix   batch.dubins_cost_matrix of --matrix x --matrix poses (1024: 1.05M pairs): pairs/s
  kernel        pmp_dubins_batch alone on --segments pairs, buffers allocated once: segments/s, points/s and
                the bytes of point rows stored (24 B a point) per second as a share of the 8 TB/s HBM peak
  call          batch.dubins_batch on the same pairs as a caller uses it (the cap estimate, the
                allocations, the launch, the status read of the overflow retry)
  cost_only     the same call with cost_only=True
  generation    one Dubins.generation() end to end (upload, launch, read-back, the Python tuple)
The legs alternate inside each repeat, so drift on a shared machine falls on all of them alike.
Reported per leg: the median over the repeats and its min-max spread.
With --reference-src (the reference's `src` directory, where it is installed) the reference's own
generation() is timed on one CPU core on the first --reference-pairs pairs; with no HIP device only that
part runs.  One JSON line per leg.
--kind bspline and cubic_spline take waypoint lists, not pose pairs: their shapes and legs are waypoint_legs()'s."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEP, CURV = 0.1, 0.25
POLY = (0.1, 1.0, 0.5)  # step, max_acc, max_jerk; dt, t_min, t_max are the reference's 0.1, 1, 30
BEZIER = (0.1, 3.0)     # step, offset
HBM_PEAK = 8.0e12
ROW_BYTES = dict(dubins=24, reeds_shepp=24, polynomial=56, bezier=16)
REF_CLASS = dict(dubins="Dubins", reeds_shepp="ReedsShepp", polynomial="Polynomial", bezier="Bezier")


def poses(rng, n, kind="dubins"):
    cols = [rng.uniform(0, 40, n), rng.uniform(0, 40, n), rng.uniform(-np.pi, np.pi, n)]
    if kind == "polynomial":
        cols += [rng.uniform(0, 2, n), rng.uniform(-0.3, 0.3, n)]
    return np.column_stack(cols)


def kind_args(kind):
    return POLY if kind == "polynomial" else BEZIER if kind == "bezier" else (STEP, CURV)


def reference_seconds(src, s, g, kind="dubins"):
    import types
    import unittest.mock

    sys.path.insert(0, src)
    sys.modules.setdefault("osqp", types.ModuleType("osqp"))
    sys.modules["pyvista"] = unittest.mock.MagicMock()
    os.environ.setdefault("MPLBACKEND", "Agg")
    from python_motion_planning import curve_generation

    gen = getattr(curve_generation, REF_CLASS[kind])(*kind_args(kind))
    secs, npts = [], []
    for a, b in zip(s, g):
        t0 = time.perf_counter()
        r = gen.generation(tuple(a), tuple(b))
        secs.append(time.perf_counter() - t0)
        npts.append(r.size if kind == "polynomial" else len(r[0]) if kind == "bezier" else len(r[2]))
    return dict(leg="reference_cpu_1core", kind=kind, pairs=len(secs), points=int(sum(npts)),
                median_s_per_generation=float(np.median(secs)), min_s=float(min(secs)), max_s=float(max(secs)),
                points_per_s=float(sum(npts) / sum(secs)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kind", choices=("dubins", "reeds_shepp", "polynomial", "bezier", "bspline", "cubic_spline"), required=True)
    ap.add_argument("--matrix", type=int, default=1024)
    ap.add_argument("--segments", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--reference-src", default=None)
    ap.add_argument("--reference-pairs", type=int, default=200)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    lines = []

    def emit(d):
        d = dict(kind=a.kind, **d) if "kind" not in d else d
        lines.append(d)
        print(json.dumps(d), flush=True)

    if a.kind in ("bspline", "cubic_spline"):
        if not torch.cuda.is_available():
            raise SystemExit("needs a HIP device (there is no CPU fallback)")
        waypoint_legs(a, emit, torch)
        return write_out(a, lines)
    rng = np.random.default_rng(0)
    ms, mg = poses(rng, a.matrix, a.kind), poses(rng, a.matrix, a.kind)
    ss, sg = poses(rng, a.segments, a.kind), poses(rng, a.segments, a.kind)
    if not torch.cuda.is_available():
        if not a.reference_src:
            raise SystemExit("needs a HIP device (there is no CPU fallback) or --reference-src")
    else:
        from python_motion_planning_amd import Bezier, Dubins, Polynomial, ReedsShepp, _lib, batch

        L, ctx = _lib.load_library(), _lib.context()
        dev = [torch.as_tensor(v, device="cuda") for v in (ms, mg, ss, sg)]
        args = kind_args(a.kind)
        entry, run_batch, run_matrix, params, gen_cls, heads = dict(
            dubins=("pmp_dubins_batch", batch.dubins_batch, batch.dubins_cost_matrix, _lib.DubinsParams, Dubins,
                    ("word", "tpq", "cost")),
            reeds_shepp=("pmp_reeds_shepp_batch", batch.reeds_shepp_batch, batch.reeds_shepp_cost_matrix,
                         _lib.ReedsSheppParams, ReedsShepp, ("slot", "lengths", "cost", None)),
            polynomial=("pmp_polycurve_batch", batch.polynomial_batch, batch.polynomial_time_matrix,
                        lambda *p: _lib.PolyCurveParams(*p, 0.1, 1.0, 30.0), Polynomial, ("t_index", "T")),
            bezier=("pmp_bezier_batch", batch.bezier_batch, None, _lib.BezierParams, Bezier, ("control",)))[a.kind]
        first = run_batch(dev[2], dev[3], *args)
        # a polynomial pair with no feasible T has status 1 and no rows: counted, not an error
        assert int(((first["status"] != 0) & (first["status"] != 1)).sum()) == 0
        npts = int(first["n_points"].sum())
        pc = int(first["points"].shape[1])
        prm = params(*args)
        o = {k: torch.empty_like(first[k]) for k in tuple(h for h in heads if h) + ("n_points", "status")}
        gen = gen_cls(*args)
        head = [None if h is None else o[h].data_ptr() for h in heads]

        def kernel():
            rc = getattr(L, entry)(ctx, _lib.stream_ptr(), ctypes.byref(prm), a.segments, dev[2].data_ptr(),
                                   dev[3].data_ptr(), *head, o["n_points"].data_ptr(), pc, first["points"].data_ptr(),
                                   o["status"].data_ptr())
            _lib.check(ctx, rc, entry)

        legs = dict(cost_matrix=lambda: run_matrix(dev[0], dev[1], *args), kernel=kernel,
                    call=lambda: run_batch(dev[2], dev[3], *args),
                    cost_only=lambda: run_batch(dev[2], dev[3], *args, cost_only=True),
                    generation=lambda: gen.generation(tuple(ss[0]), tuple(sg[0])))
        if run_matrix is None:
            del legs["cost_matrix"]
        secs = {k: [] for k in legs}
        for rep in range(a.warmup + a.repeats):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                r = fn()
                e1.record()
                torch.cuda.synchronize()
                host = time.perf_counter() - t0
                del r
                if rep >= a.warmup:  # generation() ends in its own read-back: the host clock spans it
                    secs[k].append(host if k == "generation" else e0.elapsed_time(e1) * 1e-3)
        assert int(o["n_points"].sum()) == npts and torch.equal(o["status"], first["status"])
        for k in legs:
            v = np.array(secs[k])
            med = float(np.median(v))
            d = dict(leg=k, repeats=a.repeats, median_ms=med * 1e3, min_ms=float(v.min() * 1e3), max_ms=float(v.max() * 1e3))
            if k == "cost_matrix":
                n = a.matrix * a.matrix
                d.update(pairs=n, pairs_per_s=n / med, pairs_per_s_min=n / float(v.max()), pairs_per_s_max=n / float(v.min()))
            elif k == "generation":
                d.update(points=int(first["n_points"][0]), clock="host")
            else:
                if a.kind == "polynomial":
                    d.update(no_feasible_T=int((first["status"] == 1).sum()),
                             median_t_index=float(first["t_index"].float().median()))
                d.update(segments=a.segments, segments_per_s=a.segments / med)
                if k != "cost_only":
                    d.update(points=npts, point_cap=pc, points_per_s=npts / med)
                if k == "kernel":
                    rb = ROW_BYTES[a.kind]
                    d.update(store_bytes=npts * rb, store_GBps=npts * rb / med * 1e-9, hbm_peak_frac=npts * rb / med / HBM_PEAK)
            emit(d)
    if a.reference_src:
        emit(reference_seconds(a.reference_src, ss[: a.reference_pairs], sg[: a.reference_pairs], a.kind))
    write_out(a, lines)


def write_out(a, lines):
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


def pso_lists(rng, n):
    """n waypoint lists of 7 points as PSO.calFitnessValue hands them to BSpline.run (pso.py:186-212): (5, 5),
    five points of sorted x in 5..45 and sorted y in 5..25, (45, 25); real-valued, so no two coincide"""
    xs, ys = np.sort(rng.uniform(5, 45, (n, 5)), axis=1), np.sort(rng.uniform(5, 25, (n, 5)), axis=1)
    p = np.empty((n, 7, 2))
    p[:, 0], p[:, 6] = (5.0, 5.0), (45.0, 25.0)
    p[:, 1:6, 0], p[:, 1:6, 1] = xs, ys
    return p


def walks(rng, n, m):
    """n random walks of m points: steps of 0.5..3 that turn by at most 60 degrees"""
    ang = np.cumsum(rng.uniform(-np.pi / 3, np.pi / 3, (n, m)), axis=1)
    r = rng.uniform(0.5, 3.0, (n, m))
    p = np.stack([np.cumsum(r * np.cos(ang), axis=1), np.cumsum(r * np.sin(ang), axis=1)], axis=2)
    return p - p[:, :1]


def timed(torch, legs, warmup, repeats, host_legs=()):
    """{leg: seconds per repeat}: the legs alternate inside each repeat, each between two device events (the
    legs named in host_legs end in their own read-back: the host clock spans them)"""
    secs = {k: [] for k in legs}
    for rep in range(warmup + repeats):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            r = fn()
            e1.record()
            torch.cuda.synchronize()
            host = time.perf_counter() - t0
            del r
            if rep >= warmup:
                secs[k].append(host if k in host_legs else e0.elapsed_time(e1) * 1e-3)
    return {k: np.array(v) for k, v in secs.items()}


def waypoint_legs(a, emit, torch):
    """--kind bspline: 61,440 PSO-shaped curves (7 points, k = 4, step 0.01: 100 rows; one PSO plan's 300 particles x
    201 evaluations, rounded up) and 4,096 curves of 64 points at k = 3.  --kind cubic_spline: --segments walks of 16
    points at step 0.1.  Legs: kernel (the C entry alone, buffers allocated once), call (the batch wrapper),
    cost_only, run (one run() of the class end to end, host clock); the reference's seconds per run() are read
    from tests/golden/bspline.npz, measured on the machine that made the fixture."""
    from python_motion_planning_amd import BSpline, CubicSpline, _lib, batch

    L, ctx = _lib.load_library(), _lib.context()
    rng = np.random.default_rng(0)
    fx = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "bspline.npz"))
    i32 = torch.int32
    if a.kind == "bspline":
        shapes = [("pso", pso_lists(rng, 61440), 4, float(fx["bs_ref_seconds_per_run_pso"])),
                  ("walk64", walks(rng, 4096, 64), 3, float(fx["bs_ref_seconds_per_run_64"]))]
    else:
        shapes = [("walk16", walks(rng, a.segments, 16), 0, float(fx["cs_ref_seconds_per_run"]))]
    for name, P, k, ref_s in shapes:
        n, m = P.shape[:2]
        flat = torch.as_tensor(P.reshape(-1, 2), device="cuda")
        off = torch.arange(0, (n + 1) * m, m, dtype=i32, device="cuda")
        if a.kind == "bspline":
            first = batch.bspline_batch((flat, off), 0.01, k)
            T, rowb = first["n_samples"], 16
            npts = n * T
            prm = _lib.BSplineParams(0.01, k, 0, 0, 0)
            gen, one = BSpline(0.01, k), [tuple(p) for p in P[0]]

            def kernel():
                rc = L.pmp_bspline_batch(ctx, _lib.stream_ptr(), ctypes.byref(prm), n, flat.data_ptr(), off.data_ptr(), 2, m, m,
                                         None, None, first["params"].data_ptr(), first["knot"].data_ptr(),
                                         first["control"].data_ptr(), first["n_control"].data_ptr(), T,
                                         first["points"].data_ptr(), first["length"].data_ptr(), first["status"].data_ptr())
                _lib.check(ctx, rc, "pmp_bspline_batch")

            legs = dict(kernel=kernel, call=lambda: batch.bspline_batch((flat, off), 0.01, k),
                        cost_only=lambda: batch.bspline_batch((flat, off), 0.01, k, cost_only=True),
                        run=lambda: gen.run(one, display=False))
        else:
            first = batch.cubic_spline_batch((flat, off), STEP)
            pc, rowb = int(first["points"].shape[1]), 24
            npts = int(first["n_points"].sum())
            prm = _lib.CubicSplineParams(STEP, 0, 0)
            gen, one = CubicSpline(STEP), [tuple(p) for p in P[0]]

            def kernel():
                rc = L.pmp_cubic_spline_batch(ctx, _lib.stream_ptr(), ctypes.byref(prm), n, flat.data_ptr(), off.data_ptr(), 2, m, m,
                                              first["arc_length"].data_ptr(), first["n_points"].data_ptr(), pc,
                                              first["points"].data_ptr(), first["status"].data_ptr())
                _lib.check(ctx, rc, "pmp_cubic_spline_batch")

            legs = dict(kernel=kernel, call=lambda: batch.cubic_spline_batch((flat, off), STEP),
                        cost_only=lambda: batch.cubic_spline_batch((flat, off), STEP, cost_only=True),
                        run=lambda: gen.run(one))
        assert int((first["status"] != 0).sum()) == 0
        secs = timed(torch, legs, a.warmup, a.repeats, host_legs=("run",))
        for leg, v in secs.items():
            med = float(np.median(v))
            d = dict(shape=name, leg=leg, repeats=a.repeats, median_ms=med * 1e3, min_ms=float(v.min() * 1e3),
                     max_ms=float(v.max() * 1e3))
            if leg == "run":
                d.update(clock="host", reference_ms_per_run=ref_s * 1e3)
            else:
                d.update(curves=n, waypoints=m, curves_per_s=n / med)
                if leg != "cost_only":
                    d.update(points=npts, points_per_s=npts / med)
                if leg == "kernel":
                    d.update(store_bytes=npts * rowb, store_GBps=npts * rowb / med * 1e-9, hbm_peak_frac=npts * rowb / med / HBM_PEAK)
            emit(d)


if __name__ == "__main__":
    main()
