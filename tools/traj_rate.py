#!/usr/bin/env python3
"""Trajectories/s, points/s and store bandwidth of PolynomialTrajectory3D (polytraj3d.hip) or
SplineTrajectory3D (splinetraj3d.hip) on C5 paths planned by the 3D A* kernel, with the other generators on
the same paths timed in the same run for scale.

    python tools/traj_rate.py --kind polynomial|spline [--paths 4096] [--warmup 3] [--repeats 9] [--out FILE]
                              [--reference-src DIR [--reference-paths 6]]

Workload: `--paths` C5 queries (workloads.c5_workload) planned by batch.astar3d_batch, the constraints of
examples/3d_example.py:104-109 (2 / 2 / 1.5 m/s, 1.5 / 1.5 / 1 m/s^2, dt 0.05), for the spline
spline_degree = 3 as the example passes it.  Per repeat, between two device events each:
  kernel_cells / kernel_host   the kind's C entry alone on buffers allocated once: the paths as the
                               planner's cell ids on the device / as uploaded f64 waypoints
  call_cells                   the kind's batch call as a caller uses it, from the planner's device tensors
                               (sizing, launch, the status read of the overflow retry)
  call_host   (polynomial)     the same from the paths copied to the host and decoded there (that copy
                               included)
  polytraj    (spline)         batch.polytraj3d_batch (cells form) on the same paths
  totp                         batch.totp3d_batch on the host-decoded paths
The legs alternate inside each repeat, so drift on a shared machine falls on all of them alike.
Reported per leg: the median over the repeats and its min-max spread; for the kernel legs also the
bytes of point rows stored (120 B per point, 96 B for the spline) per second as a fraction of the 8 TB/s
HBM peak.
With --reference-src (the reference's `src` directory, where it is installed) the reference's own
generate() of the kind is timed on one CPU core on the first `--reference-paths` paths; with no HIP device
only that part runs (on seeded random-walk paths).
One JSON line per leg."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VMAX, AMAX, DT, DEGREE = (2.0, 2.0, 1.5), (1.5, 1.5, 1.0), 0.05, 3
HBM_PEAK = 8.0e12


def reference_seconds(src, paths, spline):
    import types
    import unittest.mock

    sys.path.insert(0, src)
    sys.modules.setdefault("osqp", types.ModuleType("osqp"))
    sys.modules["pyvista"] = unittest.mock.MagicMock()
    os.environ.setdefault("MPLBACKEND", "Agg")
    from python_motion_planning import trajectory as T

    cons = T.TrajectoryConstraints(np.array(VMAX), np.array(AMAX), np.array([1.0, 1.0, 0.8]), DT)
    secs, npts = [], []
    for p in paths:
        wp = [tuple(v) for v in p]
        tr = T.SplineTrajectory3D(wp, cons, spline_degree=DEGREE) if spline else T.PolynomialTrajectory3D(wp, cons)
        t0 = time.perf_counter()
        pts = tr.generate()
        secs.append(time.perf_counter() - t0)
        npts.append(len(pts))
    return dict(leg="reference_cpu_1core", paths=len(paths), waypoints=[len(p) for p in paths], points=npts,
                median_s_per_trajectory=float(np.median(secs)), min_s=float(min(secs)), max_s=float(max(secs)),
                points_per_s=float(sum(npts) / sum(secs)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kind", choices=("polynomial", "spline"), required=True)
    ap.add_argument("--paths", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--reference-src", default=None)
    ap.add_argument("--reference-paths", type=int, default=6)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    spline = a.kind == "spline"

    import torch

    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    if not torch.cuda.is_available():
        if not a.reference_src:
            raise SystemExit("needs a HIP device (there is no CPU fallback) or --reference-src")
        rng = np.random.default_rng(0)
        walks = []
        for n in (18, 22, 26, 30, 34, 60):
            st = rng.integers(-1, 2, size=(n, 3))
            if spline:
                st[:, 0] = 1  # no repeated waypoint
            walks.append(np.cumsum(st, axis=0) + 30)
        emit(reference_seconds(a.reference_src, walks[: a.reference_paths], spline))
    else:
        from python_motion_planning_amd import _lib, batch, workloads as wl

        occ, s, g = wl.c5_workload(a.paths)
        X, Y, Z = occ.shape[-3:]
        pa = batch.astar3d_batch(occ, s, g, path_cap=256)
        pl = pa["path_len"].cpu().numpy()
        nq = len(pl)

        def host_paths():
            P = pa["path"].cpu().numpy()
            out = []
            for q in range(nq):
                v = P[q, : pl[q]].astype(np.int64)
                out.append(np.stack([v // (Y * Z), (v // Z) % Y, v % Z], axis=1).astype(np.float64))
            return out

        paths = host_paths()
        pprm = _lib.PolyTrajParams.make(VMAX, AMAX, DT)
        tprm = _lib.TotpParams.make(VMAX, AMAX, DT, 0.05)
        prm = _lib.SplineTrajParams.make(VMAX, AMAX, DT, DEGREE) if spline else pprm
        call = batch.splinetraj3d_batch if spline else batch.polytraj3d_batch
        row_bytes = 96 if spline else 120
        L, ctx = _lib.load_library(), _lib.context()
        cells = (pa["path"], pa["path_len"], (X, Y, Z))
        first = call(None, prm, cells=cells)
        assert int((first["status"] == 2).sum()) == 0
        npts = int(first["n_points"].sum())
        ntraj = int((first["status"] == 0).sum())
        pc = int(first["points"].shape[1])
        nmax = int(max(3 if spline else 2, pl.max()))
        flat = torch.as_tensor(np.concatenate(paths), device="cuda")
        off = np.zeros(nq + 1, np.int32)
        off[1:] = np.cumsum(pl)
        off_d = torch.as_tensor(off, device="cuda")
        o = dict(points=first["points"], n=torch.empty(nq, dtype=torch.int32, device="cuda"),
                 tt=torch.empty(nq, dtype=torch.float64, device="cuda"),
                 seg=torch.empty((nq, 256), dtype=torch.float64, device="cuda"),
                 st=torch.empty(nq, dtype=torch.int32, device="cuda"))

        def kernel(as_cells):
            src = (None, None, pa["path"].data_ptr(), pa["path_len"].data_ptr(), 256, X, Y, Z) if as_cells else \
                  (flat.data_ptr(), off_d.data_ptr(), None, None, 0, 0, 0, 0)
            head = (ctx, _lib.stream_ptr(), ctypes.byref(prm), nq) + src
            outs = (o["points"].data_ptr(), o["n"].data_ptr(), o["tt"].data_ptr())
            if spline:
                rc = L.pmp_splinetraj3d_batch(*head, nmax, pc, *outs, o["st"].data_ptr(), None, 0, 0.0, 0)
            else:
                rc = L.pmp_polytraj3d_batch(*head, None, nmax, pc, *outs, o["seg"].data_ptr(), o["st"].data_ptr(),
                                            None, 0, 0.0)
            _lib.check(ctx, rc, "pmp_splinetraj3d_batch" if spline else "pmp_polytraj3d_batch")

        legs = dict(kernel_cells=lambda: kernel(True), kernel_host=lambda: kernel(False),
                    call_cells=lambda: call(None, prm, cells=cells, max_waypoints=nmax))
        if spline:
            legs["polytraj"] = lambda: batch.polytraj3d_batch(None, pprm, cells=cells, max_waypoints=nmax)
        else:
            legs["call_host"] = lambda: batch.polytraj3d_batch(host_paths(), prm)
        legs["totp"] = lambda: batch.totp3d_batch(paths, tprm)
        secs = {k: [] for k in legs}
        for rep in range(a.warmup + a.repeats):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                r = fn()
                e1.record()
                torch.cuda.synchronize()
                del r
                if rep >= a.warmup:
                    secs[k].append(e0.elapsed_time(e1) * 1e-3)
        assert int(o["n"].sum()) == npts and int((o["st"] == 0).sum()) == ntraj
        other = {k: int(legs[k]()["n_points"].sum()) for k in ("polytraj", "totp") if k in legs}
        for k in legs:
            v = np.array(secs[k])
            n_p = other.get(k, npts)
            d = dict(leg=k, paths=nq, trajectories=ntraj, points=n_p)
            if spline:
                d["waypoints_max"] = nmax
            d.update(repeats=a.repeats, median_ms=float(np.median(v) * 1e3), min_ms=float(v.min() * 1e3),
                     max_ms=float(v.max() * 1e3), trajectories_per_s=float(ntraj / np.median(v)),
                     points_per_s=float(n_p / np.median(v)))
            if k.startswith("kernel"):
                d["store_bytes"] = npts * row_bytes
                d["store_GBps"] = float(npts * row_bytes / np.median(v) * 1e-9)
                d["hbm_peak_frac"] = float(npts * row_bytes / np.median(v) / HBM_PEAK)
            emit(d)
        if a.reference_src:
            usable = [p for p in paths if len(p) >= 3] if spline else paths
            emit(reference_seconds(a.reference_src, usable[: a.reference_paths], spline))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
