"""Dev probe: ACO (pmp_aco_batch) at the class defaults (50 ants x 100 iterations, alpha 1, beta 5, rho 0.1, Q 1)
on the README grid, (5, 5) -> (45, 25).
  * first the `default` case of tests/golden/aco.npz is run and compared exactly (status, path, cost_list, the
    draw count, the generator's words, the pheromone's SHA-256); a mismatch ends the run;
  * the kernel: batch.aco_batch on device-resident inputs between a pair of HIP events (output and scratch
    allocation included, as a caller pays it), for 1, 256 and 4096 plans (or the counts given), plan i from
    random.seed(i);
  * the waves per workgroup: the launches of --sweep plans (default 256 and 4096) at each of --waves (default
    1, 2, 4, 8, the supported values);
  * the whole call: ACO.plan() for one plan and ACO.plan_batch() for 256, wall clock, with the host's table,
    the upload and the read-back.
Each figure is the median of --timed (2) launches after one warm-up.  Prints plans/s and ant-steps/s (a step
that chooses is a draw) next to the reference's seconds for the default plan recorded in the fixture.
Usage: python tools/aco_rate.py [--plans 1,256,4096] [--waves 1,2,4,8] [--sweep 256,4096] [--timed 2].  Needs a
HIP device; there is no fallback."""
import argparse
import os
import random
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import aco_checks as C  # noqa: E402
import python_motion_planning_amd as pmp  # noqa: E402
from python_motion_planning_amd import _lib, batch  # noqa: E402

START, GOAL = (5, 5), (45, 25)


def check_default(c):
    p = c["params"]
    planner = pmp.ACO(c["start"], c["goal"], C.grid_of(c), **p)
    t0 = time.perf_counter()
    out = batch.aco_batch(C.grid_of(c), [c["start"]], [c["goal"]], planner.heuristic_table()[None], [0],
                          [np.array(c["state_in"], np.uint32)], p["n_ants"], p["max_iter"], p["alpha"], 1 - p["rho"], p["Q"],
                          trace=True)
    n, nc = int(out["best_len"][0]), int(out["n_cost"][0])
    ok = dict(status=int(out["status"][0]) == 0, path=out["best_path"][0, :n].tolist() == c["path"].tolist(),
              cost_list=out["cost_list"][0, :nc].tolist() == c["cost_list"].tolist(), draws=int(out["draws"][0]) == c["draws"],
              state=tuple(int(w) for w in out["mt_state_out"][0].cpu().numpy().view(np.uint32)) == c["state_out"],
              ants=np.array_equal(out["ant_len"][0].cpu().numpy(), c["ant_len"]) and
              np.array_equal(out["ant_found"][0].cpu().numpy(), c["ant_found"]),
              pheromone=C.pheromone_sha256(out["pheromone"][0].cpu().numpy()) == c["pher_sha256"])
    print(f"default case ({c['draws']} draws, path of {len(c['path'])} cells, n_cost {len(c['cost_list'])}): "
          f"{'exact' if all(ok.values()) else 'MISMATCH'} {ok}; first call {time.perf_counter() - t0:.3f} s", flush=True)
    return all(ok.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", default="1,256,4096")
    ap.add_argument("--waves", default="1,2,4,8")
    ap.add_argument("--sweep", default="256,4096")
    ap.add_argument("--timed", type=int, default=2)
    a = ap.parse_args()
    torch = _lib.device_check()
    torch.cuda.set_device(0)
    z = C.load()
    c = C.case(z, list(z["names"]).index("default"))
    if not check_default(c):
        sys.exit(1)
    env = C.grid_of(c)
    planner = pmp.ACO(START, GOAL, env)
    table = torch.as_tensor(planner.heuristic_table()[None], device="cuda")
    most = max([int(v) for v in a.plans.split(",")] + [int(v) for v in a.sweep.split(",") if v])
    words = np.array([random.Random(i).getstate()[1] for i in range(most)], np.uint32)
    states = torch.as_tensor(words.view(np.int32), device="cuda")

    def timed(nq, waves):
        s = torch.as_tensor(np.tile(START, (nq, 1)).astype(np.int32), device="cuda")
        g = torch.as_tensor(np.tile(GOAL, (nq, 1)).astype(np.int32), device="cuda")
        of = torch.zeros(nq, dtype=torch.int32, device="cuda")
        ms, r = [], None
        for it in range(1 + a.timed):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = batch.aco_batch(env, s, g, table, of, states[:nq], waves=waves)
            e1.record()
            e1.synchronize()
            if it:
                ms.append(e0.elapsed_time(e1))
        return np.array(ms), r

    def report(tag, nq, t, r):
        sec = np.median(t) * 1e-3
        draws = r["draws"].double().sum().item()
        st = np.bincount(r["status"].cpu().numpy(), minlength=6)
        print(f"{tag}: {nq} plans, median launch {np.median(t):.1f} ms (min {t.min():.1f}, max {t.max():.1f}); "
              f"{nq / sec:.1f} plans/s, {draws / sec / 1e6:.2f}M ant-steps/s, {sec / max(draws / nq, 1) * 1e6:.3f} us per "
              f"step of one plan, draws/plan {draws / nq:.0f}, status path/none/raises = {st[0]}/{st[1]}/{st[5]}, "
              f"best length median {r['best_len'].median().item()}", flush=True)

    for nq in (int(v) for v in a.plans.split(",")):
        t, r = timed(nq, None)
        report(f"kernel, waves {batch.aco_default_waves()} (default)", nq, t, r)
    for nq in (int(v) for v in a.sweep.split(",") if v):
        for w in (int(v) for v in a.waves.split(",") if v):
            t, r = timed(nq, w)
            report(f"kernel, waves {w}", nq, t, r)

    for nq in (1, 256):
        ts = []
        for rep in range(1 + a.timed):
            t0 = time.perf_counter()
            if nq == 1:
                random.seed(rep)
                pmp.ACO(START, GOAL, env).plan()
            else:
                out = pmp.ACO.plan_batch(env, [START] * nq, [GOAL] * nq, list(range(nq)))
                out["best_len"].cpu()
            if rep:
                ts.append(time.perf_counter() - t0)
        print(f"whole call ({'ACO.plan()' if nq == 1 else 'ACO.plan_batch()'}): {nq} plans in {np.median(ts) * 1e3:.1f} ms "
              f"= {nq / np.median(ts):.1f} plans/s (host table, upload, launch, read-back)", flush=True)
    print(f"reference: {c['ref_seconds']:.1f} s for the default plan on one core ({c['draws'] / c['ref_seconds'] / 1e3:.1f}k "
          f"ant-steps/s; tests/golden/aco.npz)")


if __name__ == "__main__":
    main()
