"""Dev probe: JPS (pmp_jps2d_batch) beside A* (pmp_astar2d_batch) on two 1024^2 workloads of 4096 pairs,
same process, launches alternated, every launch between its own pair of HIP events, each workload as
one batch per launch and as four batches per launch (a launch lasts at least as long as its longest
query, which a single batch of 4096 does not hide):
  C2     workloads.c2_workload(): 20 % random obstacles -- clutter, which favours A*
  rooms  walls every 64 cells with 2-cell doors in the middle of every room side, pairs of free cells
         drawn with default_rng(2) -- open space, where jump points are few
Prints plans/s (median launch), mean expansions per query and the statuses from an untimed launch with
counters, and the reference's CPU seconds for the fixture's six C2 queries as make_golden_jps2d.py
recorded them.  Usage: python tools/jps2d_rate.py [warmup [timed]] (default 1 and 3 launches of each).
Needs a HIP device; there is no fallback."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from python_motion_planning_amd import _lib, batch, workloads as wl  # noqa: E402

NQ = 4096


def rooms_workload(n=1024, pitch=64, nq=NQ, seed=2):
    occ = wl.boundary_grid(n, n)
    for k in range(pitch, n - 1, pitch):
        occ[k, :] = occ[:, k] = 1
    for k in range(pitch, n - 1, pitch):  # a 2-cell door in the middle of every room side
        for j in range(0, n, pitch):
            occ[k, j + pitch // 2 - 1: j + pitch // 2 + 1] = 0
            occ[j + pitch // 2 - 1: j + pitch // 2 + 1, k] = 0
    free = np.argwhere(occ == 0)
    rng = np.random.default_rng(seed)
    starts = free[rng.integers(0, len(free), nq)].astype(np.int32)
    return occ, starts, free[rng.integers(0, len(free), nq)].astype(np.int32)


def main():
    warmup = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    timed = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    torch = _lib.device_check()
    torch.cuda.set_device(0)
    for wname, (occ, s, g) in (("C2", wl.c2_workload(NQ)), ("rooms", rooms_workload())):
        W, H = occ.shape
        bits = batch.occ_bits_device(occ, torch)
        s_d, g_d = torch.as_tensor(s, device="cuda"), torch.as_tensor(g, device="cuda")
        s4, g4 = s_d.repeat(4, 1), g_d.repeat(4, 1)  # four batches through one launch's workers
        runs = {"jps2d": lambda **kw: batch.jps2d_batch((W, H), s_d, g_d, path_cap=4096, occ_bits=bits, **kw),
                "astar2d": lambda **kw: batch.astar2d_batch((W, H), s_d, g_d, path_cap=4096, occ_bits=bits,
                                                            retry_overflow=False, **kw),
                "jps2d x4": lambda **kw: batch.jps2d_batch((W, H), s4, g4, path_cap=4096, occ_bits=bits, **kw),
                "astar2d x4": lambda **kw: batch.astar2d_batch((W, H), s4, g4, path_cap=4096, occ_bits=bits,
                                                               retry_overflow=False, **kw)}
        ms = {k: [] for k in runs}
        for it in range(warmup + timed):
            for name, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= warmup:
                    ms[name].append(e0.elapsed_time(e1))
        for name, fn in runs.items():
            r = fn(counters=True)
            torch.cuda.synchronize()
            st = np.bincount(r["status"].cpu().numpy(), minlength=4)
            t = np.array(ms[name])
            n = NQ * (4 if name.endswith("x4") else 1)
            print(f"{wname} {name}: {n / (np.median(t) * 1e-3):.0f} plans/s (median launch {np.median(t):.2f} ms, min "
                  f"{t.min():.2f}, max {t.max():.2f}; {timed} launches of {n} queries), "
                  f"{float(r['counters'][:, 2].double().mean()):.1f} expansions/query, "
                  f"{float(r['counters'][:, 0].double().mean()):.1f} pushes/query "
                  f"(max {int(r['counters'][:, 0].max())}), "
                  f"status found/none/path_cap/cap = {st[0]}/{st[1]}/{st[2]}/{st[3]}", flush=True)
    z = np.load(os.path.join(REPO, "tests", "golden", "jps2d_runs.npz"))
    big = z["grid"] == int(np.flatnonzero(z["grid_kind"] == 1)[0])
    print("reference JPS on the CPU, the fixture's six C2 queries: "
          + ", ".join(f"{v:.1f} s" for v in z["ref_seconds"][big]) + f" ({int(z['n_closed'][big].sum())} expansions)")


if __name__ == "__main__":
    main()
