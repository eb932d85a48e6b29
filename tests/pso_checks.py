"""PSO fixture (tests/golden/pso.npz, made by make_golden_pso.py from the reference's own runs): the loader and
the comparison rules.

Rules.  The swarm's state is exact: initial positions, every particle's position after every iteration, final
positions, velocities (bit for bit), the best position, the status and the words of `random` after plan().
Fitness values, fitness_history, the rows and the cost carry the B-spline's rounding and are compared within
RTOL relative to max(1, |value|); an inf is an inf.  RTOL is not chosen here: it is bs_rtol of
tests/golden/bspline.npz (64 x the worst deviation of the curve's float64 restatement from the reference over
that fixture), the bound the B-spline kernel's own tests use.

The exact rules hold because the generator asserted, for every case it stored, that every fitness comparison of
the reference's run was between bit-identical values or values at least gap_required (1e-9) apart, relative, and
that no row coordinate lay within 1e-9 of a half-integer: both five orders above RTOL's scale at the achieved
margins (min_rel_gap, min_half_dist)."""
import numpy as np

import bspline_checks
from golden_io import load_npz, seg

GEN_MODE_CIRCLE, GEN_MODE_RANDOM = 0, 1
RTOL = float(bspline_checks.load()["bs_rtol"])


def load():
    return load_npz("pso.npz")


def case(z, i):
    """Case i as a dict"""
    W, H = (int(v) for v in z["dims"][i])
    n, pn, it = int(z["n_particles"][i]), int(z["point_num"][i]), int(z["max_iter"][i])
    occ = np.unpackbits(seg(z["occ_bits"], z["occ_off"], i))[: W * H].reshape(W, H).astype(np.uint8)

    def block(key, shape, dtype):
        return seg(z[key], z[key + "_off"], i).astype(dtype).reshape(shape)

    traced = bool(z["traced"][i])
    wi, wc, ws = (float(v) for v in z["weights"][i])
    return dict(name=str(z["names"][i]), seed=int(z["seed"][i]), W=W, H=H, occ=occ,
                start=tuple(int(v) for v in z["start"][i]), goal=tuple(int(v) for v in z["goal"][i]),
                params=dict(n_particles=n, point_num=pn, max_iter=it, w_inertial=wi, w_cognitive=wc, w_social=ws,
                            max_speed=int(z["max_speed"][i]), init_mode=int(z["init_mode"][i])),
                traced=traced, expect_inf=bool(z["expect_inf"][i]), raised=str(z["raised"][i]),
                state=tuple(int(w) for w in z["state"][i]), gauss=float(z["gauss"][i]),
                init=block("init", (n, pn, 2), np.int32), history=block("history", (it,), np.float64),
                pos=block("pos", (n, pn, 2), np.int32), vel=block("vel", (n, pn, 2), np.float64),
                fit=block("fit", (n,), np.float64), best_fit=block("best_fit", (n,), np.float64),
                gbest_pos=block("gbest_pos", (pn, 2), np.int32), gbest_fit=float(z["gbest_fit"][i]),
                rows=block("rows", (-1, 2), np.float64), cost=float(z["cost"][i]), improve=int(z["improve"][i]), later=int(z["later"][i]),
                min_rel_gap=float(z["min_rel_gap"][i]), min_half_dist=float(z["min_half_dist"][i]),
                n_identical=int(z["n_identical"][i]), ref_seconds=float(z["ref_seconds"][i]),
                trace_pos=block("trace_pos", (it, n, pn, 2), np.int32) if traced else None,
                trace_fit=block("trace_fit", (it, n), np.float64) if traced else None)


def grid_of(c):
    """The case's map as this package's Grid"""
    from python_motion_planning_amd import Grid

    return Grid.from_occupancy(c["occ"])


def deviation(a, b):
    """The largest |a - b| / max(1, |b|) over the finite entries of b; inf where the shapes or the patterns of
    inf / NaN differ"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return float("inf")
    fin = np.isfinite(b)
    if not np.array_equal(fin, np.isfinite(a)) or not np.array_equal(a[~fin], b[~fin], equal_nan=True):
        return float("inf")
    if not fin.any():
        return 0.0
    return float((np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin]))).max())


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
