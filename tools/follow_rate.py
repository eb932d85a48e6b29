#!/usr/bin/env python3
"""Agent-steps/s of the PID / APF / RPP plan iterations (follow.hip) on the C4 workload, with LQR
(track.hip) timed in the same run for scale.

    python tools/follow_rate.py [--agents 256 4096] [--iters 200] [--warmup 3] [--repeats 9] [--out FILE]

Per (kind, agent count): every repeat restarts from the same C4 states, runs one batch call of `--iters`
plan iterations between two device events, and counts the steps the agents actually took (an agent
that reaches its goal stops stepping).  The kinds alternate inside each repeat, so drift on a shared
machine falls on all of them alike.  Reported: the median rate over the repeats and its min-max
spread.  One JSON line per (kind, agent count); needs a HIP device (there is no CPU fallback)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--agents", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch

    from python_motion_planning_amd import _lib, batch, local_planner, workloads as wl

    _lib.device_check()
    kinds = ("pid", "apf", "rpp", "lqr")
    lines = []
    for na in a.agents:
        occ, states, goals = wl.c4_workload(na)
        r = batch.astar2d_batch(occ, states[:, :2].astype(np.int32), np.tile([45, 25], (na, 1)).astype(np.int32),
                                path_cap=2048)
        pl, P, H = r["path_len"].cpu().numpy(), r["path"].cpu().numpy(), occ.shape[1]
        xy, off = batch.pack_paths([np.column_stack([P[i, : pl[i]][::-1] // H, P[i, : pl[i]][::-1] % H]).astype(np.float64)
                                    for i in range(na)])
        xy_d = torch.as_tensor(xy, device="cuda")
        off_d = torch.as_tensor(off, device="cuda")
        goals_d = torch.as_tensor(goals, device="cuda")
        grid = (0, 0, batch.occ_bits_device(occ.astype(np.uint8), torch), occ.shape)
        st0 = torch.as_tensor(states, device="cuda")
        fp, lq = _lib.FollowParams.make(), _lib.LQRParams.make()

        def call(kind):
            st = st0.clone()
            if kind == "lqr":
                lp = _lib.LPParams.from_params(local_planner.LocalPlanner.DEFAULTS)
                run = lambda: batch.track_step_batch("lqr", lp, st, goals_d, xy_d, off_d, iters=a.iters, lqr_params=lq)  # noqa: E731
            else:
                lp = _lib.LPParams.from_params(dict(local_planner.LocalPlanner.DEFAULTS,
                                                    **({"MIN_LOOKAHEAD_DIST": 0.75} if kind == "pid" else {})))
                pid = torch.zeros((na, 4), dtype=torch.float64, device="cuda")
                run = lambda: batch.follow_step_batch(kind, grid, lp, fp, st, goals_d, xy_d, off_d, iters=a.iters,  # noqa: E731
                                                      pid_state=pid)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            out = run()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3, int(out["n_steps"].sum())

        rates = {k: [] for k in kinds}
        steps = {}
        for rep in range(a.warmup + a.repeats):
            for k in kinds:
                t, n = call(k)
                steps[k] = n
                if rep >= a.warmup:
                    rates[k].append(n / t)
        for k in kinds:
            v = np.array(rates[k])
            lines.append(dict(kind=k, agents=na, iters=a.iters, agent_steps=steps[k], repeats=a.repeats,
                              median_steps_per_s=float(np.median(v)), min_steps_per_s=float(v.min()),
                              max_steps_per_s=float(v.max()), median_ms=float(steps[k] / np.median(v) * 1e3)))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
