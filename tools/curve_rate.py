#!/usr/bin/env python3
"""Pairs/s, segments/s, points/s and store bandwidth of the curve kernels (dubins.hip, reeds_shepp.hip).

    python tools/curve_rate.py --kind dubins|reeds_shepp [--matrix 1024] [--segments 65536] [--warmup 3] [--repeats 9]
                               [--out FILE] [--reference-src DIR [--reference-pairs 200]]

Poses are default_rng(0): x, y in 0..40, yaw in -pi..pi; step 0.1, max_curv 0.25
(examples/curve_examples.py:27).  Per repeat, between two device events each:
(dubins shown; reeds_shepp: batch.reeds_shepp_*, pmp_reeds_shepp_batch without slot_costs, ReedsShepp)
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
part runs.  One JSON line per leg."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEP, CURV = 0.1, 0.25
HBM_PEAK = 8.0e12
ROW_BYTES = 24


def poses(rng, n):
    return np.column_stack([rng.uniform(0, 40, n), rng.uniform(0, 40, n), rng.uniform(-np.pi, np.pi, n)])


def reference_seconds(src, s, g, kind="dubins"):
    import types
    import unittest.mock

    sys.path.insert(0, src)
    sys.modules.setdefault("osqp", types.ModuleType("osqp"))
    sys.modules["pyvista"] = unittest.mock.MagicMock()
    os.environ.setdefault("MPLBACKEND", "Agg")
    from python_motion_planning import curve_generation

    gen = getattr(curve_generation, "ReedsShepp" if kind == "reeds_shepp" else "Dubins")(STEP, CURV)
    secs, npts = [], []
    for a, b in zip(s, g):
        t0 = time.perf_counter()
        r = gen.generation(tuple(a), tuple(b))
        secs.append(time.perf_counter() - t0)
        npts.append(len(r[2]))
    return dict(leg="reference_cpu_1core", kind=kind, pairs=len(secs), points=int(sum(npts)),
                median_s_per_generation=float(np.median(secs)), min_s=float(min(secs)), max_s=float(max(secs)),
                points_per_s=float(sum(npts) / sum(secs)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kind", choices=("dubins", "reeds_shepp"), required=True)
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

    rng = np.random.default_rng(0)
    ms, mg = poses(rng, a.matrix), poses(rng, a.matrix)
    ss, sg = poses(rng, a.segments), poses(rng, a.segments)
    if not torch.cuda.is_available():
        if not a.reference_src:
            raise SystemExit("needs a HIP device (there is no CPU fallback) or --reference-src")
    else:
        from python_motion_planning_amd import Dubins, ReedsShepp, _lib, batch

        L, ctx = _lib.load_library(), _lib.context()
        dev = [torch.as_tensor(v, device="cuda") for v in (ms, mg, ss, sg)]
        rs = a.kind == "reeds_shepp"
        entry = "pmp_reeds_shepp_batch" if rs else "pmp_dubins_batch"
        run_batch = batch.reeds_shepp_batch if rs else batch.dubins_batch
        run_matrix = batch.reeds_shepp_cost_matrix if rs else batch.dubins_cost_matrix
        first = run_batch(dev[2], dev[3], STEP, CURV)
        assert int((first["status"] != 0).sum()) == 0
        npts = int(first["n_points"].sum())
        pc = int(first["points"].shape[1])
        prm = (_lib.ReedsSheppParams if rs else _lib.DubinsParams)(STEP, CURV)
        o = {k: torch.empty_like(first[k]) for k in (("slot", "lengths") if rs else ("word", "tpq")) + ("cost", "n_points", "status")}
        gen = (ReedsShepp if rs else Dubins)(STEP, CURV)
        head = [o["slot"].data_ptr(), o["lengths"].data_ptr(), o["cost"].data_ptr(), None] if rs else \
            [o["word"].data_ptr(), o["tpq"].data_ptr(), o["cost"].data_ptr()]

        def kernel():
            rc = getattr(L, entry)(ctx, _lib.stream_ptr(), ctypes.byref(prm), a.segments, dev[2].data_ptr(),
                                   dev[3].data_ptr(), *head, o["n_points"].data_ptr(), pc, first["points"].data_ptr(),
                                   o["status"].data_ptr())
            _lib.check(ctx, rc, entry)

        legs = dict(cost_matrix=lambda: run_matrix(dev[0], dev[1], STEP, CURV), kernel=kernel,
                    call=lambda: run_batch(dev[2], dev[3], STEP, CURV),
                    cost_only=lambda: run_batch(dev[2], dev[3], STEP, CURV, cost_only=True),
                    generation=lambda: gen.generation(tuple(ss[0]), tuple(sg[0])))
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
        assert int(o["n_points"].sum()) == npts and int((o["status"] != 0).sum()) == 0
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
                d.update(segments=a.segments, segments_per_s=a.segments / med)
                if k != "cost_only":
                    d.update(points=npts, point_cap=pc, points_per_s=npts / med)
                if k == "kernel":
                    d.update(store_bytes=npts * ROW_BYTES, store_GBps=npts * ROW_BYTES / med * 1e-9,
                             hbm_peak_frac=npts * ROW_BYTES / med / HBM_PEAK)
            emit(d)
    if a.reference_src:
        emit(reference_seconds(a.reference_src, ss[: a.reference_pairs], sg[: a.reference_pairs], a.kind))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
