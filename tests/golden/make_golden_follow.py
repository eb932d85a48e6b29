"""Generate tests/golden/follow_plans.npz by running the REFERENCE PID / APF / RPP planners
(local_planner/pid.py, apf.py, rpp.py) on the README grid.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_follow.py

Cases (README grid, A* global path as the planners build it themselves):
  reach A     (5, 5, 0) -> (45, 25, 0), each kind: PID 1157 poses, APF 1074, RPP 1049
  reach B     (8, 24, -1.0) -> (45, 25, 0.5), each kind: 993 / 894 / 889
  engaged     RPP with scaling_dist = 1.5 and regulated_radius_min = 3.0 on A and B (1278 / 958 poses):
              with the defaults neither constraint ever changes the speed on this grid
  never       (5, 25, 1.5) -> (35, 5, 3.0), each kind: (False, None) after 1500 iterations, the last of
              them turning at the goal
  cut         A with MAX_ITERATION = 300, each kind: (False, None)
  raises      RPP (5, 5, 0) -> (15, 5, 0): ZeroDivisionError in the first iteration

The planner's methods are wrapped, not changed, to record per case: the global path, the poses, the
lookahead point of every step, the robot's final (px, py, theta, v, w), PID's final integrators, the
exception's name, and how often each branch ran (at the goal, rotating towards the path, APF with a
non-zero repulsive force, each of RPP's two constraints lowering the speed).

Robustness gate.  A device libm may differ from glibc in the last bit, so every case is run a second
time with angle() moved by one ulp up or down at random (exact zeros are kept: atan2(0, x > 0) is 0
in every libm) and, after every kinematic step, each of px, py, theta moved by one ulp up or down
with probability 1/2 (half an ulp on average).  A case is kept only when that run takes the same
number of steps, ends the same way and keeps every pose within 1e-10; a case that fails is to be
replaced by another query, not loosened.

Also recorded: the three constructors' parameter names and defaults and the planners' str().
"""
from __future__ import annotations

import inspect
import math
import os
import random
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import close_figs, import_reference, readme_env  # noqa: E402

FIXTURE = "follow_plans.npz"
A = ((5, 5, 0), (45, 25, 0))
B = ((8, 24, -1.0), (45, 25, 0.5))
NEVER = ((5, 25, 1.5), (35, 5, 3.0))
RAISE = ((5, 5, 0), (15, 5, 0))
ENGAGED = dict(scaling_dist=1.5, regulated_radius_min=3.0)
KINDS = ("pid", "apf", "rpp")

# (name, kind, (start, goal), attributes set after construction, LocalPlanner params)
CASES = [("reach_a", k, A, {}, {}) for k in KINDS] + [("reach_b", k, B, {}, {}) for k in KINDS]
CASES += [("engaged_a", "rpp", A, ENGAGED, {}), ("engaged_b", "rpp", B, ENGAGED, {})]
CASES += [("never", k, NEVER, {}, {}) for k in KINDS]
CASES += [("cut", k, A, {}, dict(MAX_ITERATION=300)) for k in KINDS]
CASES += [("raises", "rpp", RAISE, {}, {})]
# pose counts of the successful cases, from the reference
EXPECT_POSES = {("reach_a", "pid"): 1157, ("reach_a", "apf"): 1074, ("reach_a", "rpp"): 1049,
                ("reach_b", "pid"): 993, ("reach_b", "apf"): 894, ("reach_b", "rpp"): 889,
                ("engaged_a", "rpp"): 1278, ("engaged_b", "rpp"): 958}


def nudge(x, rng):
    return math.nextafter(x, math.inf if rng.random() < 0.5 else -math.inf)


def run_case(args):
    (name, kind, (start, goal), attrs, params), noise_seed = args
    pmp = import_reference()
    cls = {"pid": pmp.PID, "apf": pmp.APF, "rpp": pmp.RPP}[kind]
    p = cls(start, goal, readme_env(pmp), **params)
    for k, v in attrs.items():
        setattr(p, k, v)
    rng = random.Random(noise_seed) if noise_seed is not None else None
    cnt = dict(at_goal=0, rotate=0, rep=0, curv=0, obs=0)
    look, it = [], dict(lin=False)

    angle0, lookahead0, lin0, kin0 = p.angle, p.getLookaheadPoint, p.linearRegularization, p.robot.kinematic

    def angle(a, b):
        r = angle0(a, b)
        return nudge(r, rng) if rng is not None and r != 0.0 else r

    def lookahead():
        r = lookahead0()
        look.append(r[0])
        return r

    def lin(v_d):
        it["lin"] = True
        return lin0(v_d)

    def kinematic(u, dt):
        if not p.shouldMoveToGoal(p.robot.position, p.goal):
            cnt["at_goal"] += 1
        elif not it["lin"]:
            cnt["rotate"] += 1
        it["lin"] = False
        kin0(u, dt)
        if rng is not None:
            r = p.robot
            for k in ("px", "py", "theta"):
                if rng.random() < 0.5:
                    setattr(r, k, nudge(getattr(r, k), rng))

    p.angle, p.getLookaheadPoint, p.linearRegularization, p.robot.kinematic = angle, lookahead, lin, kinematic
    if kind == "apf":
        rep0 = p.getRepulsiveForce

        def rep():
            r = rep0()
            cnt["rep"] += int(not np.all(r == 0))
            return r

        p.getRepulsiveForce = rep
    if kind == "rpp":
        curv0, obs0 = p.applyCurvatureConstraint, p.applyObstacleConstraint

        def curv(raw, k):
            r = curv0(raw, k)
            cnt["curv"] += int(r != raw)
            return r

        def obs(raw):
            r = obs0(raw)
            cnt["obs"] += int(r != raw)
            return r

        p.applyCurvatureConstraint, p.applyObstacleConstraint = curv, obs

    exc, ok = "", False
    try:
        ok = bool(p.plan()[0])
    except ZeroDivisionError as e:
        exc = type(e).__name__
    close_figs()
    r = p.robot
    poses = np.asarray(r.history_pose, np.float64).reshape(-1, 3)
    out = dict(ok=ok, exc=exc, poses=poses, look=np.asarray(look[: len(poses)], np.float64).reshape(-1, 2),
               final=np.array([r.px, r.py, r.theta, r.v, r.w], np.float64),
               counters=np.array([cnt[k] for k in ("at_goal", "rotate", "rep", "curv", "obs")], np.int64),
               path=np.asarray(p.path, np.float64), str=str(p))
    if kind == "pid":
        out["integrators"] = np.array([p.e_v, p.i_v, p.e_w, p.i_w], np.float64)
    return out


def constructor_record(pmp):
    """name -> (parameter names, defaults as float; NaN where there is none or it is not a number)."""
    rec = {}
    for kind, cls in (("pid", pmp.PID), ("apf", pmp.APF), ("rpp", pmp.RPP)):
        names, defaults = [], []
        for n, q in inspect.signature(cls.__init__).parameters.items():
            if n == "self":
                continue
            names.append(("**" if q.kind is q.VAR_KEYWORD else "") + n)
            d = q.default
            defaults.append(float(d) if isinstance(d, (int, float)) and not isinstance(d, bool) else float("nan"))
        rec[kind] = (names, defaults)
    return rec


def main():
    pmp = import_reference()
    with Pool(16) as pool:
        res = pool.map(run_case, [(c, None) for c in CASES] + [(c, 1000 + i) for i, c in enumerate(CASES)], chunksize=1)
    res, noisy = res[: len(CASES)], res[len(CASES):]
    out = dict(n_cases=np.array(len(CASES)), counter_names=np.array(["at_goal", "rotate", "rep", "curv", "obs"]))
    for kind, (names, defaults) in constructor_record(pmp).items():
        out[f"ctor_{kind}_names"] = np.array(names)
        out[f"ctor_{kind}_defaults"] = np.array(defaults, np.float64)
    worst = 0.0
    for i, (c, r, nz) in enumerate(zip(CASES, res, noisy)):
        name, kind = c[0], c[1]
        # the issue's outcomes
        if (name, kind) in EXPECT_POSES:
            assert r["ok"] and len(r["poses"]) == EXPECT_POSES[(name, kind)], (name, kind, r["ok"], len(r["poses"]))
        elif name == "raises":
            assert r["exc"] == "ZeroDivisionError" and len(r["poses"]) == 0, (name, r["exc"], len(r["poses"]))
        else:
            assert not r["ok"] and not r["exc"] and len(r["poses"]) == c[4].get("MAX_ITERATION", 1500), (name, kind)
        if name == "never":
            assert r["counters"][0] > 0, (name, kind, r["counters"])
        if kind == "apf" and name in ("reach_a", "reach_b"):
            assert r["counters"][2] > 0, (name, r["counters"])
        if name.startswith("engaged"):
            assert r["counters"][3] > 0 and r["counters"][4] > 0, (name, r["counters"])
        elif kind == "rpp":
            assert r["counters"][3] == 0 and r["counters"][4] == 0, (name, r["counters"])
        # the robustness gate
        assert (nz["ok"], nz["exc"], len(nz["poses"])) == (r["ok"], r["exc"], len(r["poses"])), (name, kind, "gate: outcome")
        dev = float(np.abs(nz["poses"] - r["poses"]).max()) if len(r["poses"]) else 0.0
        assert dev <= 1e-10, (name, kind, "gate: poses", dev)
        worst = max(worst, dev)
        out[f"c{i}_name"] = np.array(name)
        out[f"c{i}_kind"] = np.array(kind)
        out[f"c{i}_start"] = np.array(c[2][0], np.float64)
        out[f"c{i}_goal"] = np.array(c[2][1], np.float64)
        out[f"c{i}_scaling_dist"] = np.array(c[3].get("scaling_dist", 0.6))
        out[f"c{i}_regulated_radius_min"] = np.array(c[3].get("regulated_radius_min", 0.9))
        out[f"c{i}_max_iteration"] = np.array(c[4].get("MAX_ITERATION", 1500))
        for k, v in r.items():
            out[f"c{i}_{k}"] = np.asarray(v)
    path = os.path.join(HERE, FIXTURE)
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 700 * 1024, os.path.getsize(path)
    print("follow cases", [(c[0], c[1], r["ok"], r["exc"], len(r["poses"]), r["counters"].tolist()) for c, r in zip(CASES, res)])
    print("gate: worst pose deviation under noise %.3g; bytes %d" % (worst, os.path.getsize(path)))


if __name__ == "__main__":
    main()
