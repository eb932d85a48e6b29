"""Drop-in trajectory generators for the step after 3D planning (examples/3d_example.py:93-133 of the
reference), each on its gfx950 kernel:

  TimeOptimalTrajectory3D  trajectory/time_optimal_trajectory.py:8-353  pmp_totp3d_batch
  PolynomialTrajectory3D   trajectory/polynomial_trajectory.py:52-331   pmp_polytraj3d_batch
  SplineTrajectory3D       trajectory/spline_trajectory.py:8-392        pmp_splinetraj3d_batch (smoothing_factor = 0)

Same constructors, attributes and return values as the reference (TrajectoryPoint / TrajectoryConstraints
dataclasses as in trajectory/trajectory_base.py:8-45); generate(), evaluate(), resample() and
reparameterize_constant_speed() run on the GPU.  For many paths at once use batch.totp3d_batch,
batch.polytraj3d_batch and batch.splinetraj3d_batch.

What the reference keeps in TrajectoryBase is in _Trajectory3D here: the path, the default constraints, the
accessors, check_constraints() and the step from a kernel status to the reference's exception.
_CurveTrajectory3D adds what the polynomial and the spline share: the curve stays on the device as
generate() left it, so evaluate() and resample() launch again, or walk the reference's host loop once a
later call has changed total_time.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import _lib, batch


@dataclass
class TrajectoryPoint:
    """trajectory_base.py:8-22"""
    time: float
    position: np.ndarray
    velocity: np.ndarray
    acceleration: np.ndarray
    jerk: Optional[np.ndarray] = None
    yaw: Optional[float] = None
    yaw_rate: Optional[float] = None

    def to_tuple(self):
        return tuple(self.position)


@dataclass
class TrajectoryConstraints:
    """trajectory_base.py:25-45"""
    max_velocity: np.ndarray
    max_acceleration: np.ndarray
    max_jerk: Optional[np.ndarray] = None
    min_time_step: float = 0.01

    def __post_init__(self):
        self.max_velocity = np.asarray(self.max_velocity)
        self.max_acceleration = np.asarray(self.max_acceleration)
        if self.max_jerk is not None:
            self.max_jerk = np.asarray(self.max_jerk)


def _params(constraints: TrajectoryConstraints, path_resolution: float):
    return _lib.TotpParams.make(np.asarray(constraints.max_velocity, np.float64),
                                np.asarray(constraints.max_acceleration, np.float64), float(constraints.min_time_step),
                                float(path_resolution))


def _points(rows: np.ndarray) -> List[TrajectoryPoint]:
    """Point rows of a kernel (12 doubles, or 15 with the jerk): time, position, velocity, acceleration,
    [jerk,] yaw, yaw rate.  NaN = None: the kernels leave the yaw columns NaN in every mode but generate()."""
    jerk = rows.shape[1] == 15
    return [TrajectoryPoint(time=float(r[0]), position=r[1:4].copy(), velocity=r[4:7].copy(), acceleration=r[7:10].copy(),
                            jerk=r[10:13].copy() if jerk else None,
                            yaw=None if np.isnan(r[-2]) else float(r[-2]),
                            yaw_rate=None if np.isnan(r[-1]) else float(r[-1])) for r in rows]


def _all_points(r) -> List[TrajectoryPoint]:
    return _points(r["points"][0, : int(r["n_points"][0].item())].cpu().numpy())


class _Trajectory3D:
    """TrajectoryBase (trajectory_base.py:48-191) for a 3D path.  A subclass names its C entry and what the
    reference raises where the kernel reports PMP_REF_RAISES, and launches one path in _launch()."""
    _entry = ""
    _ref_raises = ""

    def __init__(self, path, constraints: Optional[TrajectoryConstraints]):
        if not path:
            raise ValueError("Path cannot be empty")
        # _process_path (trajectory_base.py:64-95): 2D points get z = 0
        self.dimension = 3
        self.path = np.array([[p[0], p[1], 0.0] if len(p) == 2 else list(p) for p in path], dtype=float)
        if constraints is None:
            constraints = TrajectoryConstraints(np.array([2.0] * 3), np.array([1.0] * 3))
        self.constraints = constraints
        self.trajectory_points: List[TrajectoryPoint] = []
        self.total_time = 0.0
        self.segment_times: List[float] = []

    def _run(self, **kw):
        r = self._launch(**kw)
        st = int(r["status"][0].item())
        if st == _lib.STATUS_REF_RAISES:
            raise ValueError(self._ref_raises)
        if st != _lib.STATUS_FOUND:
            raise _lib.PMPError(f"{self._entry} status {st}")
        return r

    # TrajectoryBase accessors (trajectory_base.py:97-149)
    def get_positions(self) -> np.ndarray:
        if not self.trajectory_points:
            self.generate()
        return np.array([tp.position for tp in self.trajectory_points])

    def get_velocities(self) -> np.ndarray:
        if not self.trajectory_points:
            self.generate()
        return np.array([tp.velocity for tp in self.trajectory_points])

    def get_accelerations(self) -> np.ndarray:
        if not self.trajectory_points:
            self.generate()
        return np.array([tp.acceleration for tp in self.trajectory_points])

    def get_times(self) -> np.ndarray:
        if not self.trajectory_points:
            self.generate()
        return np.array([tp.time for tp in self.trajectory_points])

    def get_path_length(self) -> float:
        return float(sum(np.linalg.norm(self.path[i] - self.path[i - 1]) for i in range(1, len(self.path))))

    def check_constraints(self) -> dict:
        """trajectory_base.py:150-190"""
        if not self.trajectory_points:
            self.generate()
        res = {"velocity_satisfied": True, "acceleration_satisfied": True, "jerk_satisfied": True}
        if np.any(np.max(np.abs(self.get_velocities()), axis=0) > self.constraints.max_velocity):
            res["velocity_satisfied"] = False
        if np.any(np.max(np.abs(self.get_accelerations()), axis=0) > self.constraints.max_acceleration):
            res["acceleration_satisfied"] = False
        return res


class _CurveTrajectory3D(_Trajectory3D):
    """A curve that stays on the device as generate() left it.  Its _launch() takes eval_t and sample_dt."""

    def __init__(self, path, constraints):
        super().__init__(path, constraints)
        self._generated_total = None  # total_time of the curve on the device (generate()'s)

    def _time_scale(self) -> float:
        """Device time per unit of this object's time.  1 for the polynomial (:253-286): after
        optimize_time_allocation() scaled total_time, times past the segments' end give the last one's end."""
        return 1.0

    def _evaluate_many(self, ts) -> List[TrajectoryPoint]:
        # the reference's evaluate(t) clips t to self.total_time, which a later call may have changed while
        # the curve stays generate()'s: the device evaluates at t * k and the chain-rule factors follow here
        tc = [float(np.clip(t, 0, self.total_time)) for t in ts]
        k = self._time_scale()
        pts = _points(self._run(eval_t=tc if k == 1.0 else [t * k for t in tc])["points"][0, : len(tc)].cpu().numpy())
        for p, t in zip(pts, tc):
            p.time = t
            if k != 1.0:
                p.velocity *= k
                p.acceleration *= k * k
        return pts

    def evaluate(self, t: float) -> TrajectoryPoint:
        if self._generated_total is None:
            self.generate()
        return self._evaluate_many([t])[0]

    def resample(self, dt: float) -> List[TrajectoryPoint]:
        """trajectory_base.py:193-216"""
        if not self.trajectory_points:
            self.generate()
        if not dt > 0:
            raise ValueError("dt must be > 0")
        if self.total_time == self._generated_total:
            return _all_points(self._run(sample_dt=float(dt)))
        ts, t = [], 0.0  # the reference's loop over the changed total_time
        while t <= self.total_time:
            ts.append(t)
            t += dt
        out = self._evaluate_many(ts)
        if out[-1].time < self.total_time:
            out += self._evaluate_many([self.total_time])
        return out


class TimeOptimalTrajectory3D(_Trajectory3D):
    """time_optimal_trajectory.py:8-39 (path-velocity decomposition along a waypoint path)."""
    _entry = "pmp_totp3d_batch"
    _ref_raises = "`x` must be strictly increasing sequence."

    def __init__(self, path, constraints: Optional[TrajectoryConstraints] = None, path_resolution: float = 0.01):
        super().__init__(path, constraints)
        self.path_resolution = path_resolution
        self.s_values = None
        self.path_length = 0.0
        self.s_dot_profile = None
        self.s_ddot_profile = None
        self.time_profile = None

    def _launch(self, eval_t=None):
        if len(self.path) < 2:
            raise ValueError("Need at least 2 waypoints for trajectory generation")
        return batch.totp3d_batch([self.path], _params(self.constraints, self.path_resolution), eval_t=eval_t)

    def generate(self) -> List[TrajectoryPoint]:
        """generate() (:260-302) + compute_yaw_from_velocity (trajectory_base.py:245-261)."""
        r = self._run()
        ns = int(r["n_samples"][0].item())
        self.s_values = r["s_values"][0, :ns].cpu().numpy()
        self.path_length = float(self.s_values[-1])
        self.s_dot_profile = r["s_dot"][0, :ns].cpu().numpy()
        self.s_ddot_profile = r["s_ddot"][0, :ns].cpu().numpy()
        self.time_profile = r["time"][0, :ns].cpu().numpy()
        self.total_time = float(r["total_time"][0].item())
        self.trajectory_points = _all_points(r)
        return self.trajectory_points

    def evaluate(self, t: float) -> TrajectoryPoint:
        """evaluate(t) (:304-335) after generate()."""
        if self.time_profile is None:
            raise AttributeError("'TimeOptimalTrajectory3D' object has no attribute 's_of_t' (call generate() first)")
        return _points(self._run(eval_t=[float(t)])["points"][0, :1].cpu().numpy())[0]


_BC_KEYS = ("initial_velocity", "final_velocity", "initial_acceleration", "final_acceleration")


class PolynomialTrajectory3D(_CurveTrajectory3D):
    """polynomial_trajectory.py:52-331 (quintic segments through the waypoints) on pmp_polytraj3d_batch:
    generate(), evaluate() and resample() run on the GPU; optimize_time_allocation() is the reference's
    host loop around generate().  For many paths at once use batch.polytraj3d_batch."""
    _entry = "pmp_polytraj3d_batch"
    _ref_raises = "the path's total time is not finite"

    def __init__(self, path, constraints: Optional[TrajectoryConstraints] = None,
                 boundary_conditions: Optional[dict] = None):
        super().__init__(path, constraints)
        self.boundary_conditions = boundary_conditions or {}
        for k in _BC_KEYS:
            if k not in self.boundary_conditions:
                self.boundary_conditions[k] = np.zeros(3)

    def _params(self):
        c = self.constraints
        vmax, amax = np.asarray(c.max_velocity, np.float64), np.asarray(c.max_acceleration, np.float64)
        dt = float(c.min_time_step)
        # the reference divides by zero or never leaves its sampling loop on these
        if not (np.all(np.isfinite(vmax)) and np.all(np.isfinite(amax)) and np.min(amax) > 0):
            raise ValueError("constraints must be finite with min(max_acceleration) > 0")
        if not (np.isfinite(dt) and dt > 0):
            raise ValueError("min_time_step must be > 0")
        return _lib.PolyTrajParams.make(vmax, amax, dt)

    def _launch(self, **kw):
        if len(self.path) < 2:
            raise ValueError("Need at least 2 waypoints for trajectory generation")
        bc = np.array([[np.asarray(self.boundary_conditions[k], np.float64).reshape(3) for k in _BC_KEYS]])
        return batch.polytraj3d_batch([self.path], self._params(), bc=bc, **kw)

    def generate(self) -> List[TrajectoryPoint]:
        """generate() (:189-251): segment times, segments, sampling, yaw."""
        r = self._run()
        self.segment_times = [float(v) for v in r["segment_times"][: len(self.path) - 1].cpu().numpy()]
        self.total_time = float(r["total_time"][0].item())
        self._generated_total = self.total_time
        self.trajectory_points = _all_points(r)
        return self.trajectory_points

    def optimize_time_allocation(self, max_iterations: int = 10):
        """:288-330, literally: generate() recomputes segment_times in every iteration, so the scaled times
        survive only in segment_times / total_time after the call and the next generate() restores the
        plain result."""
        for _ in range(max_iterations):
            self.generate()
            if all(self.check_constraints().values()):
                break
            velocities = self.get_velocities()
            accelerations = self.get_accelerations()
            start = 0.0
            for i, dur in enumerate(list(self.segment_times)):
                a = int(start / self.constraints.min_time_step)
                b = min(int((start + dur) / self.constraints.min_time_step), len(velocities) - 1)
                if b > a:
                    v_ratio = np.max(np.abs(velocities[a:b + 1]) / self.constraints.max_velocity)
                    a_ratio = np.max(np.abs(accelerations[a:b + 1]) / self.constraints.max_acceleration)
                    max_ratio = max(v_ratio, a_ratio)
                    if max_ratio > 1.0:
                        self.segment_times[i] *= (max_ratio ** 0.5)
                start += dur
        self.total_time = sum(self.segment_times)

    def check_constraints(self) -> dict:
        """trajectory_base.py:150-190, the jerk check included"""
        res = super().check_constraints()
        if self.constraints.max_jerk is not None:
            jerks = [tp.jerk for tp in self.trajectory_points if tp.jerk is not None]
            if jerks and np.any(np.max(np.abs(np.array(jerks)), axis=0) > self.constraints.max_jerk):
                res["jerk_satisfied"] = False
        return res


class SplineTrajectory3D(_CurveTrajectory3D):
    """spline_trajectory.py:8-392 (B-splines through the waypoints, time-scaled to the constraints) on
    pmp_splinetraj3d_batch: generate(), evaluate(), resample() and reparameterize_constant_speed() run on
    the GPU.  smoothing_factor > 0 (FITPACK's knot search) is not offered.  For many paths at once use
    batch.splinetraj3d_batch."""
    _entry = "pmp_splinetraj3d_batch"
    _ref_raises = "x must be strictly increasing if s = 0, or the path's total time is not finite"

    def __init__(self, path, constraints: Optional[TrajectoryConstraints] = None, spline_degree: int = 5,
                 smoothing_factor: float = 0.0):
        super().__init__(path, constraints)
        if smoothing_factor > 0:
            raise NotImplementedError("smoothing_factor > 0 (FITPACK's smoothing knot search) is not offered; "
                                      "smoothing_factor = 0 interpolates the waypoints")
        self.spline_degree = min(spline_degree, len(path) - 1)
        self.smoothing_factor = smoothing_factor
        self.u_waypoints = None
        self.u_max = 1.0

    def _params(self):
        """Everything the reference raises on, or never returns from, before any device call."""
        c = self.constraints
        vmax, amax = np.asarray(c.max_velocity, np.float64), np.asarray(c.max_acceleration, np.float64)
        dt = float(c.min_time_step)
        n = len(self.path)
        if n < 3:
            raise ValueError("Need at least 3 waypoints: the second derivative of a linear spline does not exist")
        if not 1 <= self.spline_degree <= 5:
            raise ValueError("k should be 1 <= k <= 5")
        if self.spline_degree < 2:
            raise ValueError("spline_degree 1: the second derivative of a linear spline does not exist")
        if np.any(np.all(self.path[1:] == self.path[:-1], axis=1)):
            raise ValueError("x must be strictly increasing if s = 0 (two consecutive waypoints are equal)")
        if not (np.all(np.isfinite(vmax)) and np.all(np.isfinite(amax)) and np.min(np.abs(vmax)) > 0 and np.min(amax) > 0):
            raise ValueError("constraints must be finite with min|max_velocity| > 0 and min(max_acceleration) > 0")
        if not (np.isfinite(dt) and dt > 0):
            raise ValueError("min_time_step must be > 0")
        return _lib.SplineTrajParams.make(vmax, amax, dt, self.spline_degree)

    def _launch(self, **kw):
        return batch.splinetraj3d_batch([self.path], self._params(), **kw)

    def _compute_centripetal_parameterization(self) -> np.ndarray:
        """:60-77"""
        d = np.zeros(len(self.path))
        for i in range(1, len(self.path)):
            d[i] = d[i - 1] + np.sqrt(np.linalg.norm(self.path[i] - self.path[i - 1]))
        return d / d[-1] if d[-1] > 0 else np.linspace(0, 1, len(self.path))

    def generate(self) -> List[TrajectoryPoint]:
        """generate() (:205-271): fit, time parameterisation, sampling, _enforce_constraints, yaw."""
        r = self._run()
        self.u_waypoints = self._compute_centripetal_parameterization()
        self.total_time = float(r["total_time"][0].item())
        self._generated_total = self.total_time
        self.trajectory_points = _all_points(r)
        return self.trajectory_points

    def _time_scale(self) -> float:
        # evaluate(t) (:273-302) divides by self.total_time, which reparameterize_constant_speed() replaces
        # while the spline stays generate()'s (u agrees to rounding)
        return 1.0 if self.total_time == self._generated_total else self._generated_total / self.total_time

    def reparameterize_constant_speed(self):
        """:325-392, on generate()'s spline and total_time"""
        if self._generated_total is None:
            self.generate()
        r = self._run(constant_speed=True)
        self.total_time = float(r["total_time"][0].item())
        self.trajectory_points = _all_points(r)
