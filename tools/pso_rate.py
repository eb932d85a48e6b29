"""Dev probe: PSO (pmp_pso_batch) at the class defaults (300 particles x 5 points x 200 iterations) on the README
grid, (5, 5) -> (45, 25).
  * the kernel: batch.pso_batch on device-resident inputs between a pair of HIP events (output allocation
    included, as a caller pays it), for 1, 256 and 4096 plans (or the counts given).  The plans of a launch
    are POOL distinct ones (seeds 0 .. POOL - 1: their own initial positions and streams) tiled on the device: a
    plan's stream is 600,000 doubles, and 4096 of them drawn on the host would cost more than the run;
  * the waves per workgroup: the 256-plan launch at each of --waves (default 1, 2, 4, 8, 12, 16);
  * the whole call: PSO.plan() for one plan and PSO.plan_batch() for 256, wall clock, with the host's draws
    (initializePositions, the stream), the upload and the read-back.
Prints plans/s and fitness evaluations/s (a plan is n_particles (max_iter + 1) evaluations, repeats on top)
next to the bare curve's rate, the share of repeated evaluations, the statuses, and the
reference's seconds for the default-size plan recorded in tests/golden/pso.npz.  Nothing is asserted.
Usage: python tools/pso_rate.py [--plans 1,256,4096] [--waves 1,2,4,8,12,16] [--timed 3].  Needs a HIP device;
there is no fallback."""
import argparse
import os
import random
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import python_motion_planning_amd as pmp  # noqa: E402
from python_motion_planning_amd import _lib, batch, workloads as wl  # noqa: E402
from python_motion_planning_amd.evolutionary_search import _initial_positions, random_stream  # noqa: E402

N, PN, IT = 300, 5, 200
POOL = 16
START, GOAL = (5, 5), (45, 25)
BARE_CURVES_PER_S = 157e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", default="1,256,4096")
    ap.add_argument("--waves", default="1,2,4,8,12,16")
    ap.add_argument("--timed", type=int, default=3)
    a = ap.parse_args()
    torch = _lib.device_check()
    torch.cuda.set_device(0)
    env = pmp.Grid.from_occupancy(wl.readme_grid())
    draws = batch.pso_draws(N, PN, IT)
    inits, streams = [], []
    for seed in range(POOL):
        rng = random.Random(seed)
        inits.append(_initial_positions(rng, START, GOAL, 51, 31, N, PN, pmp.GEN_MODE_RANDOM))
        streams.append(random_stream(draws, rng.getstate())[0])
    init_pool = torch.as_tensor(np.array(inits, np.int32), device="cuda")
    rnd_pool = torch.as_tensor(np.array(streams), device="cuda")
    evals = N * (IT + 1)

    def timed(nq, waves, reps):
        idx = torch.arange(nq, device="cuda") % POOL
        init, rnd = init_pool[idx].contiguous(), rnd_pool[idx].contiguous()
        s = torch.as_tensor(np.tile(START, (nq, 1)).astype(np.int32), device="cuda")
        g = torch.as_tensor(np.tile(GOAL, (nq, 1)).astype(np.int32), device="cuda")
        ms, r = [], None
        for it in range(1 + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = batch.pso_batch(env, s, g, init, rnd, N, PN, IT, waves=waves)
            e1.record()
            e1.synchronize()
            if it:
                ms.append(e0.elapsed_time(e1))
        return np.array(ms), r

    def report(tag, nq, t, r):
        rep = r["repeats"].double().mean().item()
        st = np.bincount(r["status"].cpu().numpy(), minlength=5)
        sec = np.median(t) * 1e-3
        print(f"{tag}: {nq} plans, median launch {np.median(t):.2f} ms (min {t.min():.2f}, max {t.max():.2f}); "
              f"{nq / sec:.1f} plans/s, {nq * (evals + rep) / sec / 1e6:.2f}M fitness evaluations/s "
              f"({nq * (evals + rep) / sec / BARE_CURVES_PER_S * 100:.1f} % of the bare curve's 157M/s), repeats/plan "
              f"{rep:.0f} = {100 * rep / evals:.2f} % of {evals}, status ok/raises = {st[0]}/{st[4]}, best fitness median "
              f"{r['best_fitness'].median().item():.4f}", flush=True)

    for nq in (int(v) for v in a.plans.split(",")):
        t, r = timed(nq, None, a.timed)
        report(f"kernel, waves {batch.pso_default_waves()} (default)", nq, t, r)
    for w in (int(v) for v in a.waves.split(",") if v):
        t, r = timed(256, w, a.timed)
        report(f"kernel, waves {w}", 256, t, r)

    for nq in (1, 256):
        ts = []
        for rep in range(1 + min(a.timed, 2)):
            t0 = time.perf_counter()
            if nq == 1:
                random.seed(rep)
                pmp.PSO(START, GOAL, env).plan()
            else:
                out = pmp.PSO.plan_batch(env, [START] * nq, [GOAL] * nq, list(range(nq)))
                out["length"].cpu()
            if rep:
                ts.append(time.perf_counter() - t0)
        print(f"whole call ({'PSO.plan()' if nq == 1 else 'PSO.plan_batch()'}): {nq} plans in {np.median(ts) * 1e3:.1f} ms "
              f"= {nq / np.median(ts):.1f} plans/s (host draws, upload, launch, read-back)", flush=True)
    z = np.load(os.path.join(REPO, "tests", "golden", "pso.npz"))
    i = list(z["names"]).index("default")
    print(f"reference: {float(z['ref_seconds'][i]):.1f} s for the default-size plan on one core (tests/golden/pso.npz)")


if __name__ == "__main__":
    main()
