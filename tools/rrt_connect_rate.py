"""Dev probe: RRT-Connect (pmp_rrt_connect_batch) with plain RRT (pmp_rrt_batch, star off) beside it for
context, on two workloads: 4096 README-map queries (18, 8) -> (37, 18) with the class defaults, and 256
C3 queries (5, 5) -> (505, 505) with max_dist 8.  Query q reads np.random.seed(q)'s stream, the same
inputs for both planners, same process, launches alternated, every launch between its own pair of HIP
events (output allocation and the obstacle upload included, as a caller pays them).  The two planners
solve the same query by different algorithms; neither rate is a bound on the other.
Prints plans/s (median launch), and from an untimed launch: statuses, iterations, nodes, draws and
collision tests per query.
Usage: python tools/rrt_connect_rate.py [warmup [timed]] (default 1 and 5 launches of each).  Needs a
HIP device; there is no fallback."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import python_motion_planning_amd as pmp  # noqa: E402
from python_motion_planning_amd import _lib, batch, workloads as wl  # noqa: E402

SAMPLES = 10000  # the class default of both planners
CAP = 512        # nodes per RRT-Connect tree (the reference's runs of these queries need at most 150)


def workload(torch, name):
    if name == "readme":
        env = pmp.Map(51, 31)
        env.update(obs_rect=[list(r) for r in wl.README_MAP_RECT], obs_circ=[list(c) for c in wl.README_MAP_CIRC])
        return env, 4096, (18.0, 8.0), (37.0, 18.0), dict(max_dist=0.5)
    env = pmp.Map(512, 512)
    rects, circs = wl.c3_map()
    env.update(obs_rect=rects, obs_circ=circs)
    return env, 256, (5.0, 5.0), (505.0, 505.0), dict(max_dist=8.0)


def main():
    warmup = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    timed = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    torch = _lib.device_check()
    torch.cuda.set_device(0)
    for name in ("readme", "c3"):
        env, nq, start, goal, kw = workload(torch, name)
        rnd = torch.as_tensor(np.stack([np.random.RandomState(q).random_sample(3 * SAMPLES + 1) for q in range(nq)]),
                              device="cuda")
        s = torch.as_tensor(np.tile(start, (nq, 1)), device="cuda")
        g = torch.as_tensor(np.tile(goal, (nq, 1)), device="cuda")
        runs = {"rrt_connect": lambda **k: batch.rrt_connect_batch(env, s, g, rnd, SAMPLES, cap=CAP, **kw, **k),
                "rrt": lambda **k: batch.rrt_batch(env, s, g, rnd, SAMPLES, star=False, **kw, **k)}
        ms = {k: [] for k in runs}
        for it in range(warmup + timed):
            for planner, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= warmup:
                    ms[planner].append(e0.elapsed_time(e1))
        for planner, fn in runs.items():
            r = fn(counters=True)
            torch.cuda.synchronize()
            st = np.bincount(r["status"].cpu().numpy(), minlength=5)
            c = r["counters"].cpu().numpy().astype(np.float64)
            t = np.array(ms[planner])
            nodes = r["n_nodes"].double().reshape(nq, -1).sum(1)
            tests = c[:, 2] if planner == "rrt_connect" else c[:, 3]
            extra = ""
            if planner == "rrt_connect":
                extra = (f", largest tree {int(r['n_nodes'].max())} of cap {CAP}, greedy steps/query {c[:, 3].mean():.0f}, "
                         f"path points/query {float(r['path_len'].double().mean()):.0f}")
            print(f"{name} {planner}: {nq / (np.median(t) * 1e-3):.0f} plans/s (median launch {np.median(t):.2f} ms, min "
                  f"{t.min():.2f}, max {t.max():.2f}; {timed} launches of {nq} queries), iterations/query "
                  f"{c[:, 0].mean():.0f}, nodes/query {float(nodes.mean()):.0f}, draws/query "
                  f"{float(r['draws'].double().mean()):.0f}, collision tests/query {tests.mean():.0f}, cost median "
                  f"{float(r['cost'].median()):.1f}{extra}, status found/none/path_cap/cap/cycle = "
                  f"{st[0]}/{st[1]}/{st[2]}/{st[3]}/{st[4]}", flush=True)
        del rnd


if __name__ == "__main__":
    main()
