"""Generate tests/golden/reeds_shepp.npz by running the REFERENCE's ReedsShepp
(curve_generation/reeds_shepp.py) with pyvista and osqp stubbed, as make_golden_dubins.py does.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_reeds_shepp.py

Cases: the 13 consecutive pairs of the two commented pose lists of examples/curve_examples.py:11-15, the
named cases below (their point counts asserted here) and 300 default_rng(11) pairs of three kinds (integer
poses with headings in multiples of 15 degrees, real poses in 0..40, real poses in 0..6) at step 0.1,
max_curv 0.25: make_golden_dubins.py's lists and stream.

The reference evaluates 46 candidates per pair; their positions are slots 0..45.  The slot of a candidate
is found by wrapping the nine primitives and Path on the instance (the reference looks them up as
self.SLS ..., so instance attributes shadow them) and counting the calls: each planner makes exactly one
primitive call per slot, 46 in all (asserted).

Per case: the poses (yaw in radians), step and max_curv; all 46 slots' lengths [46, 5] and path_length [46]
(NaN where infeasible or beyond the word's pieces); the chosen slot, the cost (best_cost / max_curv) and
the point count; every row (x, y, yaw) for the named cases and the first 64 random ones.

Ties: L-+R+-L-+ and its mirror R+-L-+R+- have the same length mathematically, so which of them the
reference takes is a rounding accident.  tie_set is the 64-bit mask of the slots within 1e-12 max(1, best)
of the best path_length; a case with more than one bit set is tied.  For every slot of a tied case's
tie_set the reference's own count is recorded, and for the cases that have rows its own rows: the six
planners on the instance are replaced by functions that return only that slot's Path, and the reference's
generation() runs on.

Each case is run 8 more times with every sin / cos / atan2 / acos result of the two reference modules
moved one ulp up or down at random (make_golden_dubins.UlpMath): fragile = the slot or the count ever
differs; feas_stable [46] = the slot's feasibility never differs.

Asserted (conditions the reference alone meets): no fragile case is untied; untied cases are at least
75 % of the 313 pairs nobody constructed and at least 40 of the 100 near pairs; at least 40 distinct slots
win somewhere; every slot is feasible in some case; no real-valued untied case has an unstable slot
feasibility.
Also: the run() path of the first pose list (8 poses, yaw in degrees), a 5 x 7 cost matrix of real-valued
poses with its slots and tie sets, and the reference's seconds per generation() on one core of the machine
that made the fixture."""
from __future__ import annotations

import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402
from make_golden_dubins import CURV, LIST1, LIST2, N_TRIALS, STEP, UlpMath, rad  # noqa: E402

PRIMITIVES = ("SLS", "LRL", "LSL", "LSR", "LRLRn", "LRLRp", "LRSR", "LRSL", "LRSLR")
PLANNERS = ("SCS", "CCC", "CSC", "CCCC", "CCSC", "CCSCC")
NSLOT = 46
TIE_RTOL = 1e-12


class Probe:
    """A reference instance whose primitive calls are counted and whose Paths carry their slot"""

    def __init__(self, gen, only_slot=None):
        self.gen, self.calls, self.paths = gen, 0, {}
        for name in PRIMITIVES:
            setattr(gen, name, self._counted(getattr(gen, name)))
        path_cls = gen.Path

        def path(**kw):
            p = path_cls(**kw)
            p.slot = self.calls - 1
            self.paths[p.slot] = p
            return p

        gen.Path = path
        if only_slot is not None:
            for name in PLANNERS:
                setattr(gen, name, self._only(getattr(gen, name), only_slot))

    def _counted(self, fn):
        def call(x, y, phi):
            self.calls += 1
            return fn(x, y, phi)

        return call

    @staticmethod
    def _only(planner, slot):
        return lambda x, y, phi: [p for p in planner(x, y, phi) if p.slot == slot]

    def generation(self, s, g):
        self.calls, self.paths = 0, {}
        out = self.gen.generation(s, g)
        assert self.calls == NSLOT, self.calls
        return out

    def table(self):
        """lengths [46, 5], path_length [46], words [46] of the last generation()"""
        ln, pl, words = np.full((NSLOT, 5), np.nan), np.full(NSLOT, np.nan), [None] * NSLOT
        for k, p in self.paths.items():
            ln[k, : len(p.lengths)] = p.lengths
            pl[k] = p.path_length
            words[k] = "".join(p.ctypes)
        return ln, pl, words


def first_best(pl):
    """the first strictly shortest, as the reference's loop takes it (:633-637)"""
    best, cost = -1, math.inf
    for k, v in enumerate(pl):
        if v < cost:
            best, cost = k, v
    return best, cost


def tie_mask(pl, best_cost):
    m = 0
    for k, v in enumerate(pl):
        if v <= best_cost + TIE_RTOL * max(1.0, best_cost):
            m |= 1 << k
    return m


def main():
    import_reference()
    from python_motion_planning.curve_generation import curve as curve_mod
    from python_motion_planning.curve_generation import reeds_shepp as rs_mod
    from python_motion_planning.utils import CurveFactory

    def make(step, curv):
        return CurveFactory()("reeds_shepp", step=step, max_curv=curv)

    d2r = float(np.deg2rad(1.0))
    rng = np.random.default_rng(11)
    random_cases = []
    for i in range(300):
        kind = i % 3
        if kind == 0:
            s = (float(rng.integers(0, 41)), float(rng.integers(0, 41)), float(rng.integers(-12, 13)) * 15 * d2r)
            g = (float(rng.integers(0, 41)), float(rng.integers(0, 41)), float(rng.integers(-12, 13)) * 15 * d2r)
        else:
            hi = 40.0 if kind == 1 else 6.0
            s = (float(rng.uniform(0, hi)), float(rng.uniform(0, hi)), float(rng.uniform(-math.pi, math.pi)))
            g = (float(rng.uniform(0, hi)), float(rng.uniform(0, hi)), float(rng.uniform(-math.pi, math.pi)))
        random_cases.append((f"rng_{('int', 'wide', 'near')[kind]}_{i}", s, g, STEP, CURV, kind != 0, None))

    # the first random pair whose winner is a five-piece CCSCC slot and has no second slot near it
    five = None
    for c in random_cases:
        pr = Probe(make(STEP, CURV))
        pr.generation(c[1], c[2])
        pl = pr.table()[1]
        b, cost = first_best(pl)
        if b >= 42 and tie_mask(pl, cost) == 1 << b:
            five = c
            break
    assert five is not None

    cases = []  # name, start, goal, step, max_curv, real-valued, expected count (or None)
    for k, lst in enumerate((LIST1, LIST2)):
        for i in range(len(lst) - 1):
            cases.append((f"ex{k + 1}_{i}", rad(lst[i]), rad(lst[i + 1]), STEP, CURV, False, None))
    cases += [
        ("axis_fwd", rad((0, 0, 0)), rad((10, 0, 0)), STEP, CURV, False, 28),
        ("axis_rev", rad((0, 0, 0)), rad((-10, 0, 0)), STEP, CURV, False, 28),
        ("zero_origin", rad((0, 0, 0)), rad((0, 0, 0)), STEP, CURV, False, 0),
        ("zero_offset", rad((1, 2, 90)), rad((1, 2, 90)), STEP, CURV, False, 0),
        ("same_position", rad((1, 2, 30)), rad((1, 2, 200)), STEP, CURV, False, 32),
        ("side", rad((0, 0, 0)), rad((0, 5, 0)), STEP, CURV, False, 33),
        ("tiny", rad((0, 0, 0)), rad((0.001, 0, 0)), STEP, CURV, False, 4),
        ("yaw_unwrapped", (0.0, 0.0, 0.0), (5.0, 5.0, 50.0), STEP, CURV, False, 28),
        ("five_piece", five[1], five[2], STEP, CURV, True, None),
        ("diag_fine", rad((0, 0, 0)), rad((10, 10, -90)), 0.05, 1.0, False, None),
        ("diag_coarse", rad((0, 0, 0)), rad((10, 10, -90)), 0.5, 0.1, False, None),
        ("diag_odd", rad((0, 0, 0)), rad((10, 10, -90)), 0.3, 0.6, False, None),
    ]
    n_named = len(cases)
    cases += random_cases

    N = len(cases)
    lengths = np.full((N, NSLOT, 5), np.nan)
    pl46 = np.full((N, NSLOT), np.nan)
    slot = np.zeros(N, np.int16)
    count = np.zeros(N, np.int32)
    cost = np.zeros(N)
    tie_set = np.zeros(N, np.uint64)
    tie_count = np.full((N, NSLOT), -1, np.int32)
    rows, has_rows = [], np.zeros(N, bool)
    tie_rows, tie_rows_case, tie_rows_slot = [], [], []
    words = None
    secs = []
    for i, (name, s, g, step, curv, real, want) in enumerate(cases):
        gen = make(step, curv)
        assert str(gen) == "Reeds Shepp Curve"
        t0 = time.perf_counter()
        c, mode, x, y, yaw = gen.generation(s, g)
        secs.append(time.perf_counter() - t0)
        pr = Probe(make(step, curv))
        c2, mode2, x2, y2, yaw2 = pr.generation(s, g)
        assert c2 == c and mode2 == mode and list(x2) == list(x) and list(yaw2) == list(yaw)
        lengths[i], pl46[i], w = pr.table()
        if words is None:
            words = [None] * NSLOT
        for k in range(NSLOT):
            if w[k] is not None:
                assert words[k] in (None, w[k])
                words[k] = w[k]
        b, bc = first_best(pl46[i])
        assert b >= 0 and "".join(mode) == w[b] and c == bc / curv, (name, b, mode)
        slot[i], cost[i], count[i] = b, c, len(x)
        assert len(y) == len(x) == len(yaw)
        if want is not None:
            assert len(x) == want, (name, len(x), want)
        keep = i < n_named + 64
        has_rows[i] = keep
        rows.append(np.column_stack([x, y, yaw]).reshape(-1, 3) if keep else np.zeros((0, 3)))
        tie_set[i] = tie_mask(pl46[i], bc)
        assert int(tie_set[i]) >> b & 1
        if int(tie_set[i]) != 1 << b:  # tied: the reference's own run of every slot of the set
            for k in range(NSLOT):
                if int(tie_set[i]) >> k & 1:
                    fc, fmode, fx, fy, fyaw = Probe(make(step, curv), only_slot=k).generation(s, g)
                    assert "".join(fmode) == w[k] and fc == pl46[i, k] / curv
                    tie_count[i, k] = len(fx)
                    if k == b:
                        assert len(fx) == len(x) and list(fx) == list(x)
                    elif keep:
                        tie_rows.append(np.column_stack([fx, fy, fyaw]).reshape(-1, 3))
                        tie_rows_case.append(i)
                        tie_rows_slot.append(k)
    tied = np.array([bin(int(m)).count("1") > 1 for m in tie_set])
    by = {c[0]: k for k, c in enumerate(cases)}
    assert all(w is not None for w in words), words  # every slot is feasible in at least one case
    assert cost[by["zero_origin"]] == 0.0 and cost[by["zero_offset"]] == 0.0
    assert (pl46[by["axis_rev"], slot[by["axis_rev"]]] > 0) and (lengths[by["axis_rev"], slot[by["axis_rev"]]] < 0).any()
    assert "S" in words[slot[by["axis_rev"]]]
    assert len(words[slot[by["side"]]]) == 4 and len(words[slot[by["five_piece"]]]) == 5
    assert np.nanmax(np.abs(lengths[by["diag_fine"], slot[by["diag_fine"]]])) / 0.05 > 64
    wins = set(slot.tolist())
    assert len(wins) >= 40, sorted(wins)

    # the run() path of the first list: the segments in order, joints duplicated (:686-696)
    run_path = np.concatenate([rows[by[f"ex1_{i}"]] for i in range(len(LIST1) - 1)])

    # 5 x 7 cost matrix of real-valued poses
    cm_s = np.column_stack([rng.uniform(0, 40, 5), rng.uniform(0, 40, 5), rng.uniform(-math.pi, math.pi, 5)])
    cm_g = np.column_stack([rng.uniform(0, 40, 7), rng.uniform(0, 40, 7), rng.uniform(-math.pi, math.pi, 7)])
    cm_cost, cm_slot, cm_tie = np.zeros((5, 7)), np.zeros((5, 7), np.int16), np.zeros((5, 7), np.uint64)
    for a in range(5):
        for b in range(7):
            pr = Probe(make(STEP, CURV))
            c = pr.generation(tuple(cm_s[a]), tuple(cm_g[b]))[0]
            pl = pr.table()[1]
            k, bc = first_best(pl)
            assert c == bc / CURV
            cm_cost[a, b], cm_slot[a, b], cm_tie[a, b] = c, k, tie_mask(pl, bc)

    # fragility: the reference again with its libm results moved by an ulp
    fragile = np.zeros(N, bool)
    feas_stable = np.ones((N, NSLOT), bool)
    wrap = UlpMath(np.random.default_rng(12))
    curve_mod.math = rs_mod.math = wrap
    try:
        for trial in range(N_TRIALS):
            for i, (name, s, g, step, curv, real, want) in enumerate(cases):
                pr = Probe(make(step, curv))
                x = pr.generation(s, g)[2]
                pl = pr.table()[1]
                if first_best(pl)[0] != slot[i] or len(x) != count[i]:
                    fragile[i] = True
                feas_stable[i] &= np.isnan(pl) == np.isnan(pl46[i])
    finally:
        curve_mod.math = rs_mod.math = math
    real = np.array([c[5] for c in cases])
    names = [c[0] for c in cases]
    plain = np.array([n.startswith("ex") or n.startswith("rng_") for n in names])
    near = np.array([n.startswith("rng_near") for n in names])
    assert not (fragile & ~tied).any(), [n for n, f, t in zip(names, fragile, tied) if f and not t]
    assert plain.sum() == 313 and (~tied[plain]).mean() >= 0.75, (~tied[plain]).sum()
    assert near.sum() == 100 and (~tied[near]).sum() >= 40, (~tied[near]).sum()
    unstable = [n for n, r, t, f in zip(names, real, tied, feas_stable) if r and not t and not f.all()]
    assert not unstable, unstable

    def offsets(rs):
        off = np.zeros(len(rs) + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in rs])
        return off

    out = dict(names=np.array(names), start=np.array([c[1] for c in cases]), goal=np.array([c[2] for c in cases]),
               params=np.array([[c[3], c[4]] for c in cases]), real=real, words=np.array(words), lengths=lengths,
               path_length=pl46, slot=slot, count=count, cost=cost, rows=np.concatenate(rows), rows_off=offsets(rows),
               has_rows=has_rows, tie_set=tie_set, tied=tied, tie_count=tie_count,
               tie_rows=np.concatenate(tie_rows) if tie_rows else np.zeros((0, 3)), tie_rows_off=offsets(tie_rows),
               tie_rows_case=np.array(tie_rows_case, np.int32), tie_rows_slot=np.array(tie_rows_slot, np.int16),
               fragile=fragile, feas_stable=feas_stable, n_named=np.int32(n_named),
               run_points=np.array(LIST1, np.float64), run_path=run_path, cm_start=cm_s, cm_goal=cm_g,
               cm_params=np.array([STEP, CURV]), cm_cost=cm_cost, cm_slot=cm_slot, cm_tie_set=cm_tie,
               ref_seconds_per_generation=np.float64(np.median(secs)))
    fn = os.path.join(HERE, "reeds_shepp.npz")
    np.savez_compressed(fn, **out)
    assert os.path.getsize(fn) < 500_000, os.path.getsize(fn)
    kinds = {k: int(tied[[n.startswith(k) for n in names]].sum()) for k in ("ex", "rng_int", "rng_wide", "rng_near")}
    print("reeds_shepp cases", N, "named", n_named, "slots that win", len(wins), "never", sorted(set(range(NSLOT)) - wins),
          "counts", int(count.min()), "..", int(count.max()), "named counts",
          {n: int(count[by[n]]) for n in names[13:n_named]}, "named slots", {n: int(slot[by[n]]) for n in names[13:n_named]},
          "tied of the 313", int(tied[plain].sum()), kinds, "untied share", float((~tied[plain]).mean()),
          "fragile", int(fragile.sum()), "fragile and untied", int((fragile & ~tied).sum()),
          "five_piece from", five[0], "rows stored", len(out["rows"]), "tie rows", len(out["tie_rows"]),
          "reference s/generation (median)", float(np.median(secs)), "bytes", os.path.getsize(fn))


if __name__ == "__main__":
    main()
