"""Dev probe: Informed RRT* (pmp_informed_rrt_batch) beside RRT* (pmp_rrt_batch) on 256 C3 queries
(5, 5) -> (505, 505), max_dist 8, r 24, np.random.seed(q) streams, the same inputs for both, same
process, launches alternated, every launch between its own pair of HIP events.  RRT* stops at its first
connection; Informed RRT* always runs every sample, so its plans cost more by construction.
Prints plans/s (median launch), and from an untimed launch with counters: nodes, connections, draws,
in-radius candidates and collision tests per iteration, statuses.
Usage: python tools/informed_rrt_rate.py [samples [warmup [timed]]] (default 8192 samples, 1 and 3
launches of each).  Needs a HIP device; there is no fallback."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import python_motion_planning_amd as pmp  # noqa: E402
from python_motion_planning_amd import _lib, batch, workloads as wl  # noqa: E402

NQ = 256


def main():
    sn = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    timed = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    torch = _lib.device_check()
    torch.cuda.set_device(0)
    env = pmp.Map(512, 512)
    rects, circs = wl.c3_map()
    env.update(obs_rect=rects, obs_circ=circs)
    stride = 8 * sn + 64  # the ellipse sampler's rejected tries: about 3.2 draws per iteration on C3
    rnd = torch.as_tensor(np.stack([np.random.RandomState(q).random_sample(stride) for q in range(NQ)]), device="cuda")
    s = torch.as_tensor(np.tile([5.0, 5.0], (NQ, 1)), device="cuda")
    g = torch.as_tensor(np.tile([505.0, 505.0], (NQ, 1)), device="cuda")
    kw = dict(max_dist=8.0, radius=24.0)
    runs = {"informed_rrt": lambda **k: batch.informed_rrt_batch(env, s, g, rnd, sn, **kw, **k),
            "rrt_star": lambda **k: batch.rrt_batch(env, s, g, rnd, sn, star=True, **kw, **k)}
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
        st = np.bincount(r["status"].cpu().numpy(), minlength=5)
        c = r["counters"].cpu().numpy().astype(np.float64)
        t = np.array(ms[name])
        extra = ""
        if name == "informed_rrt":
            bc = r["best_cost"].cpu().numpy()
            extra = (f", connections/query {float(r['n_finds'].double().mean()):.1f}, best cost median "
                     f"{np.median(bc[np.isfinite(bc)]):.1f} (straight line {np.hypot(500, 500):.1f})")
        print(f"C3 {name} {sn} samples: {NQ / (np.median(t) * 1e-3):.1f} plans/s (median launch {np.median(t):.1f} ms, min "
              f"{t.min():.1f}, max {t.max():.1f}; {timed} launches of {NQ} queries), iterations/query "
              f"{c[:, 0].mean():.0f}, nodes/query {float(r['n_nodes'].double().mean()):.0f}, draws/iteration "
              f"{float(r['draws'].double().sum()) / c[:, 0].sum():.2f}, in-radius/iteration "
              f"{c[:, 2].sum() / c[:, 0].sum():.1f}, collision tests/iteration {c[:, 3].sum() / c[:, 0].sum():.2f}{extra}, "
              f"status found/none/path_cap/cap/cycle = {st[0]}/{st[1]}/{st[2]}/{st[3]}/{st[4]}", flush=True)


if __name__ == "__main__":
    main()
