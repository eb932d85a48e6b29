"""Generate tests/golden/dubins.npz by running the REFERENCE's Dubins (curve_generation/dubins_curve.py)
with pyvista and osqp stubbed, as make_golden.py does.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_dubins.py

Cases: the 13 consecutive pairs of the two commented pose lists of examples/curve_examples.py:11-15, the
named edge cases below (their point counts asserted here) and 300 default_rng(11) pairs of three kinds
(integer poses with headings in multiples of 15 degrees, real poses in 0..40, real poses in 0..6) at
step 0.1, max_curv 0.25.
Per case: the poses (yaw in radians), step and max_curv, the six words' (t, p, q, cost) in the reference's
order (NaN where infeasible), the chosen word and the point count, every row (x, y, yaw) for the named
cases and the first 64 random ones, and a fragile flag with the set of words seen: each case is run 8
more times with every sin / cos / atan2 / acos result of the two reference modules moved one ulp up or
down at random (their `math` swapped for a wrapper); a case whose word or count ever differs is fragile.
Asserted: no real-valued case is fragile, and at most 1 % of the examples' and the random pairs are; of
the hand-made cases only the degenerate ones (axis-aligned, equal poses, 0.001 apart) may be: they are ties.
Also: the run() path of the first pose list (8 poses, yaw in degrees), a 5 x 7 cost matrix, and the
reference's seconds per generation() on one core of the machine that made the fixture."""
from __future__ import annotations

import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

WORDS = ("LSL", "RSR", "LSR", "RSL", "RLR", "LRL")
LIST1 = [(0, 0, 0), (10, 10, -90), (20, 5, 60), (30, 10, 120), (35, -5, 30), (25, -10, -120), (15, -15, 100), (0, -10, -90)]
LIST2 = [(-3, 3, 120), (10, -7, 30), (10, 13, 30), (20, 5, -25), (35, 10, 180), (32, -10, 180), (5, -12, 90)]
STEP, CURV = 0.1, 0.25
N_TRIALS = 8


class UlpMath:
    """`math` with every sin / cos / atan2 / acos result moved one ulp up or down at random"""

    def __init__(self, rng):
        self.rng = rng

    def __getattr__(self, name):
        return getattr(math, name)

    def _move(self, v):
        return float(np.nextafter(v, math.inf if self.rng.integers(2) else -math.inf))

    def sin(self, x):
        return self._move(math.sin(x))

    def cos(self, x):
        return self._move(math.cos(x))

    def atan2(self, y, x):
        return self._move(math.atan2(y, x))

    def acos(self, x):
        return self._move(math.acos(x))


def rad(p):
    return (float(p[0]), float(p[1]), float(np.deg2rad(p[2])))


def six_words(gen, s, g):
    """(t, p, q, cost) of each word for the frame generation() builds (:253-261)"""
    gx, gy = g[0] - s[0], g[1] - s[1]
    theta = gen.mod2pi(math.atan2(gy, gx))
    dist = math.hypot(gx, gy) * gen.max_curv
    alpha, beta = gen.mod2pi(s[2] - theta), gen.mod2pi(g[2] - theta)
    out = np.full((6, 4), np.nan)
    for w, fn in enumerate((gen.LSL, gen.RSR, gen.LSR, gen.RSL, gen.RLR, gen.LRL)):
        t, p, q, mode = fn(alpha, beta, dist)
        assert "".join(mode) == WORDS[w]
        if t is not None:
            out[w] = (t, p, q, abs(t) + abs(p) + abs(q))
    return out


def main():
    import_reference()
    from python_motion_planning.curve_generation import curve as curve_mod
    from python_motion_planning.curve_generation import dubins_curve as dubins_mod
    from python_motion_planning.utils import CurveFactory

    def make(step, curv):
        return CurveFactory()("dubins", step=step, max_curv=curv)

    d2r = float(np.deg2rad(1.0))
    cases = []  # name, start, goal, step, max_curv, real-valued, expected count (or None)
    for k, lst in enumerate((LIST1, LIST2)):
        for i in range(len(lst) - 1):
            cases.append((f"ex{k + 1}_{i}", rad(lst[i]), rad(lst[i + 1]), STEP, CURV, False, None))
    cases += [
        ("axis_fwd", rad((0, 0, 0)), rad((10, 0, 0)), STEP, CURV, False, 28),
        ("axis_rev", rad((0, 0, 0)), rad((-10, 0, 0)), STEP, CURV, False, None),
        ("zero_origin", rad((0, 0, 0)), rad((0, 0, 0)), STEP, CURV, False, 0),
        ("zero_offset", rad((1, 2, 90)), rad((1, 2, 90)), STEP, CURV, False, 0),
        ("same_position", rad((1, 2, 30)), rad((1, 2, 200)), STEP, CURV, False, 74),
        ("tiny", rad((0, 0, 0)), rad((0.001, 0, 0)), STEP, CURV, False, 4),
        ("diag_fine", rad((0, 0, 0)), rad((10, 10, -90)), 0.05, 1.0, False, 323),
        ("diag_coarse", rad((0, 0, 0)), rad((10, 10, -90)), 0.5, 0.1, False, 16),
        ("diag_odd", rad((0, 0, 0)), rad((10, 10, -90)), 0.3, 0.6, False, 37),
    ]
    n_named = len(cases)
    rng = np.random.default_rng(11)
    for i in range(300):
        kind = i % 3
        if kind == 0:
            s = (float(rng.integers(0, 41)), float(rng.integers(0, 41)), float(rng.integers(-12, 13)) * 15 * d2r)
            g = (float(rng.integers(0, 41)), float(rng.integers(0, 41)), float(rng.integers(-12, 13)) * 15 * d2r)
        else:
            hi = 40.0 if kind == 1 else 6.0
            s = (float(rng.uniform(0, hi)), float(rng.uniform(0, hi)), float(rng.uniform(-math.pi, math.pi)))
            g = (float(rng.uniform(0, hi)), float(rng.uniform(0, hi)), float(rng.uniform(-math.pi, math.pi)))
        cases.append((f"rng_{('int', 'wide', 'near')[kind]}_{i}", s, g, STEP, CURV, kind != 0, None))

    N = len(cases)
    words6 = np.full((N, 6, 4), np.nan)
    word = np.zeros(N, np.int8)
    count = np.zeros(N, np.int32)
    cost = np.zeros(N)
    rows, has_rows = [], np.zeros(N, bool)
    secs = []
    for i, (name, s, g, step, curv, real, want) in enumerate(cases):
        gen = make(step, curv)
        assert str(gen) == "Dubins Curve"
        t0 = time.perf_counter()
        c, mode, x, y, yaw = gen.generation(s, g)
        secs.append(time.perf_counter() - t0)
        words6[i] = six_words(gen, s, g)
        word[i] = WORDS.index("".join(mode))
        count[i] = len(x)
        cost[i] = c
        assert len(y) == len(x) == len(yaw) and c == words6[i, word[i], 3]
        if want is not None:
            assert len(x) == want, (name, len(x), want)
        keep = i < n_named + 64
        has_rows[i] = keep
        rows.append(np.column_stack([x, y, yaw]).reshape(-1, 3) if keep else np.zeros((0, 3)))
    by = {c[0]: k for k, c in enumerate(cases)}
    assert WORDS[word[by["same_position"]]] == "LRL"
    assert WORDS[word[by["zero_origin"]]] == "LSL" and WORDS[word[by["zero_offset"]]] == "LSR"
    assert cost[by["zero_origin"]] == 0.0 and cost[by["zero_offset"]] == 0.0
    assert set(word.tolist()) == set(range(6))

    # the run() path of the first list: the segments in order, joints duplicated (:327-335)
    run_path = np.concatenate([rows[by[f"ex1_{i}"]] for i in range(len(LIST1) - 1)])

    # 5 x 7 cost matrix of real-valued poses
    cm_s = np.column_stack([rng.uniform(0, 40, 5), rng.uniform(0, 40, 5), rng.uniform(-math.pi, math.pi, 5)])
    cm_g = np.column_stack([rng.uniform(0, 40, 7), rng.uniform(0, 40, 7), rng.uniform(-math.pi, math.pi, 7)])
    gen = make(STEP, CURV)
    cm_cost, cm_word = np.zeros((5, 7)), np.zeros((5, 7), np.int8)
    for a in range(5):
        for b in range(7):
            c, mode = gen.generation(tuple(cm_s[a]), tuple(cm_g[b]))[:2]
            cm_cost[a, b], cm_word[a, b] = c, WORDS.index("".join(mode))

    # fragility: the reference again with its libm results moved by an ulp
    seen = (1 << word.astype(np.int64)).astype(np.uint8)
    fragile = np.zeros(N, bool)
    prng = np.random.default_rng(12)
    wrap = UlpMath(prng)
    curve_mod.math = dubins_mod.math = wrap
    try:
        for trial in range(N_TRIALS):
            for i, (name, s, g, step, curv, real, want) in enumerate(cases):
                c, mode, x, y, yaw = make(step, curv).generation(s, g)
                w = WORDS.index("".join(mode))
                seen[i] |= 1 << w
                if w != word[i] or len(x) != count[i]:
                    fragile[i] = True
            for a in range(5):
                for b in range(7):
                    mode = gen.generation(tuple(cm_s[a]), tuple(cm_g[b]))[1]
                    assert WORDS.index("".join(mode)) == cm_word[a, b]
    finally:
        curve_mod.math = dubins_mod.math = math
    real = np.array([c[5] for c in cases])
    # The hand-made degenerate cases are exact ties by construction (on the axis every CSC word costs dist,
    # equal poses cost 0 in all of them; an ulp on atan2(0, dist) turns t = 0 into a full turn): axis_fwd,
    # zero_origin, zero_offset and tiny are fragile, 4 of 322 = 1.24 %.  The 1 % bound is therefore held on
    # the pairs nobody constructed (the examples' 13 and the 300 random ones), and the fragile named cases
    # must be of that degenerate kind.
    names = [c[0] for c in cases]
    degenerate = {"axis_fwd", "axis_rev", "zero_origin", "zero_offset", "tiny"}
    plain = np.array([n not in degenerate and (n.startswith("ex") or n.startswith("rng_")) for n in names])
    assert plain.sum() == 313 and fragile[plain].mean() <= 0.01, [n for n, f in zip(names, fragile) if f]
    assert {n for n, f in zip(names, fragile) if f and not n.startswith("rng_") and not n.startswith("ex")} <= degenerate
    assert not (fragile & real).any()

    off = np.zeros(N + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    out = dict(names=np.array([c[0] for c in cases]), start=np.array([c[1] for c in cases]),
               goal=np.array([c[2] for c in cases]), params=np.array([[c[3], c[4]] for c in cases]), real=real,
               words6=words6, word=word, count=count, cost=cost, rows=np.concatenate(rows), rows_off=off,
               has_rows=has_rows, fragile=fragile, words_seen=seen, n_named=np.int32(n_named),
               run_points=np.array(LIST1, np.float64), run_path=run_path, cm_start=cm_s, cm_goal=cm_g,
               cm_params=np.array([STEP, CURV]), cm_cost=cm_cost, cm_word=cm_word,
               ref_seconds_per_generation=np.float64(np.median(secs)))
    fn = os.path.join(HERE, "dubins.npz")
    np.savez_compressed(fn, **out)
    assert os.path.getsize(fn) < 500_000
    print("dubins cases", N, "named", n_named, "words", np.bincount(word, minlength=6).tolist(), "counts",
          int(count.min()), "..", int(count.max()), "fragile", [cases[i][0] for i in np.nonzero(fragile)[0]],
          "rows stored", len(out["rows"]), "reference s/generation (median)", float(np.median(secs)), "bytes",
          os.path.getsize(fn))


if __name__ == "__main__":
    main()
