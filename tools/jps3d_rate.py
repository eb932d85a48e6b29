"""Dev probe: JPS3D (pmp_jps3d_batch) beside AStar3D (pmp_astar3d_batch) on the 8192 C5 queries
(26x20x16 "door", per-query grids), same process, launches alternated: 5 warm-up + 20 timed launches
of each (JPS3D also with 8 workers per CU), every launch between its own pair of HIP events.  Prints
plans/s (median and mean launch), mean expansions per query from an untimed launch with counters, and
the reference's CPU time for the fixture cases as make_golden_jps3d.py recorded it.  Needs a HIP
device; there is no fallback."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from python_motion_planning_amd import _lib, workloads as wl  # noqa: E402
from python_motion_planning_amd.env import pack_bits  # noqa: E402

WARMUP, TIMED, NQ = 5, 20, 8192


def main():
    torch = _lib.device_check()
    torch.cuda.set_device(0)
    L, ctx = _lib.load_library(), _lib.context()
    occ, s, g = wl.c5_workload(NQ)
    X, Y, Z = occ.shape[1:]
    words = np.stack([pack_bits(o) for o in occ])
    occ_d = torch.as_tensor(np.ascontiguousarray(words).view(np.int32), device="cuda")
    s_d, g_d = torch.as_tensor(s, device="cuda"), torch.as_tensor(g, device="cuda")
    cap = X * Y * Z + 1
    i32 = dict(dtype=torch.int32, device="cuda")

    def buffers():
        return dict(cost=torch.empty(NQ, dtype=torch.float64, device="cuda"), plen=torch.empty(NQ, **i32),
                    path=torch.empty((NQ, cap), **i32), nexp=torch.empty(NQ, **i32), status=torch.empty(NQ, **i32),
                    ctr=torch.empty((NQ, 4), dtype=torch.int64, device="cuda"))

    bj, ba = buffers(), buffers()

    def jps(counters=False):
        rc = L.pmp_jps3d_batch(ctx, _lib.stream_ptr(), occ_d.data_ptr(), 1, X, Y, Z, 0, s_d.data_ptr(), g_d.data_ptr(), NQ,
                               bj["cost"].data_ptr(), bj["plen"].data_ptr(), bj["path"].data_ptr(), cap,
                               bj["nexp"].data_ptr(), None, None, None, 0, bj["ctr"].data_ptr() if counters else None,
                               bj["status"].data_ptr())
        _lib.check(ctx, rc, "pmp_jps3d_batch")

    def astar(counters=False):
        rc = L.pmp_astar3d_batch(ctx, _lib.stream_ptr(), occ_d.data_ptr(), 1, X, Y, Z, 0, s_d.data_ptr(), g_d.data_ptr(), NQ,
                                 ba["cost"].data_ptr(), ba["plen"].data_ptr(), ba["path"].data_ptr(), cap,
                                 ba["nexp"].data_ptr(), None, 0, ba["ctr"].data_ptr() if counters else None,
                                 ba["status"].data_ptr())
        _lib.check(ctx, rc, "pmp_astar3d_batch")

    def jps8():  # as many workers per CU as the kernel's registers keep resident (2 waves per SIMD)
        _lib.check(ctx, L.pmp_set_workers_per_cu(ctx, 8), "workers")
        try:
            jps()
        finally:
            _lib.check(ctx, L.pmp_set_workers_per_cu(ctx, 0), "workers")

    ms = {"jps3d": [], "jps3d, 8 workers per CU": [], "astar3d": []}
    for it in range(WARMUP + TIMED):
        for name, fn in (("jps3d", jps), ("jps3d, 8 workers per CU", jps8), ("astar3d", astar)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= WARMUP:
                ms[name].append(e0.elapsed_time(e1))
    jps(True)
    astar(True)
    torch.cuda.synchronize()
    found = {"jps3d": int((bj["status"] == 0).sum()), "astar3d": int((ba["status"] == 0).sum())}
    exps = {"jps3d": float(bj["ctr"][:, 2].double().mean()), "astar3d": float(ba["ctr"][:, 2].double().mean())}
    exps["jps3d, 8 workers per CU"], found["jps3d, 8 workers per CU"] = exps["jps3d"], found["jps3d"]
    for name in ms:
        t = np.array(ms[name])
        print(f"{name}: {NQ / (np.median(t) * 1e-3):.0f} plans/s (median launch {np.median(t):.3f} ms, mean {t.mean():.3f} ms, "
              f"min {t.min():.3f}, max {t.max():.3f}; {TIMED} launches of {NQ} queries), "
              f"{exps[name]:.2f} expansions/query, {found[name]} found", flush=True)
    z = np.load(os.path.join(REPO, "tests", "golden", "jps3d_runs.npz"))
    print(f"reference JPS3D on the CPU: {z['ref_seconds'].sum():.2f} s for the {len(z['ref_seconds'])} fixture cases "
          f"({int(z['expansions'].sum())} expansions, grid_map cached)")


if __name__ == "__main__":
    main()
