"""Drop-in curve generation (curve_generation/ of the reference) on the gfx950 kernels:

  Curve    curve_generation/curve.py:10-64         the base: step, trigonometric, pi2pi, mod2pi, length
  Dubins   curve_generation/dubins_curve.py:14-335 pmp_dubins_batch / pmp_dubins_cost_matrix
  ReedsShepp curve_generation/reeds_shepp.py:13-736 pmp_reeds_shepp_batch / pmp_reeds_shepp_cost_matrix
  Polynomial curve_generation/polynomial_curve.py:13-195 pmp_polycurve_batch / pmp_polycurve_time_matrix
  Bezier   curve_generation/bezier_curve.py:13-111 pmp_bezier_batch
  BSpline  curve_generation/bspline_curve.py:12-271 pmp_bspline_batch
  BSpline3D curve_generation/bspline_curve3d.py:13-220 pmp_bspline_batch (its own rules)
  CubicSpline curve_generation/cubic_spline.py:13-128 pmp_cubic_spline_batch

The first four take pose pairs, the last three a whole waypoint list: run(points) without yaw, run_batch for
many lists in one launch (batch.bspline_batch / batch.cubic_spline_batch).

Same constructor, generation() return values and run() input (yaw in degrees) as the reference; run() does
not plot (as Planner.run, planner.py:31-33).  Many pose pairs at once: generation_batch and cost_matrix of
either class, or batch.dubins_batch / batch.dubins_cost_matrix and batch.reeds_shepp_batch /
batch.reeds_shepp_cost_matrix.  Dubins.generation() returns its cost in curvature-normalised units and
ReedsShepp.generation() in the units of x and y, as the reference's do.  Polynomial takes 5-tuples (x, y,
yaw, v, a) and has generation_batch and time_matrix; Bezier has generation_batch.  CurveFactory builds
"dubins" only: construct ReedsShepp, Polynomial, Bezier, BSpline, BSpline3D and CubicSpline directly.  There is no CPU fallback: without the library or a HIP device the calls
raise PMPError.
"""
from __future__ import annotations

import math
from abc import ABC, abstractmethod

import numpy as np

from . import _lib, batch


class Curve(ABC):
    """curve.py:10-64"""

    def __init__(self, step: float) -> None:
        self.step = step

    @abstractmethod
    def run(self, points: list):
        pass

    @abstractmethod
    def generation(self, start_pose: tuple, goal_pose: tuple):
        pass

    def trigonometric(self, alpha: float, beta: float):
        """sin a, sin b, cos a, cos b, sin(a - b), cos(a - b) (curve.py:34-39)"""
        return (math.sin(alpha), math.sin(beta), math.cos(alpha), math.cos(beta), math.sin(alpha - beta),
                math.cos(alpha - beta))

    def pi2pi(self, theta: float) -> float:
        """The angle brought into [-pi, pi] by whole turns (curve.py:41-49)"""
        while theta > math.pi:
            theta -= 2.0 * math.pi
        while theta < -math.pi:
            theta += 2.0 * math.pi
        return theta

    def mod2pi(self, theta: float) -> float:
        """theta modulo 2 pi (curve.py:51-55)"""
        return theta - 2.0 * math.pi * math.floor(theta / math.pi / 2.0)

    def length(self, path: list) -> float:
        """The length of the polyline [(x, y), ...] (curve.py:57-64)"""
        dist = 0
        for a, b in zip(path[:-1], path[1:]):
            dist = dist + math.hypot(b[0] - a[0], b[1] - a[1])
        return dist


class Dubins(Curve):
    """Dubins curve generation (dubins_curve.py:14-335).

    Parameters:
        step (float): Simulation or interpolation size
        max_curv (float): The maximum curvature of the curve
    """

    def __init__(self, step: float, max_curv: float) -> None:
        super().__init__(step)
        self.max_curv = max_curv

    def __str__(self) -> str:
        return "Dubins Curve"

    def generation_batch(self, start_poses, goal_poses, **kw):
        """batch.dubins_batch with this generator's step and max_curv (yaw in radians)."""
        return batch.dubins_batch(start_poses, goal_poses, self.step, self.max_curv, **kw)

    def cost_matrix(self, start_poses, goal_poses):
        """batch.dubins_cost_matrix with this generator's step and max_curv (yaw in radians)."""
        return batch.dubins_cost_matrix(start_poses, goal_poses, self.step, self.max_curv)

    def _segments(self, starts, goals):
        """One launch -> per pair (cost, mode, x, y, yaw) as generation() returns them."""
        r = self.generation_batch(starts, goals)
        st = r["status"].cpu().numpy()
        if np.any(st == _lib.STATUS_REF_RAISES):  # the reference: int(nan) in generation() (:277)
            raise ValueError("cannot convert float NaN to integer")
        cost, word, npt = r["cost"].cpu().numpy(), r["word"].cpu().numpy(), r["n_points"].cpu().numpy()
        pts = r["points"].cpu().numpy()
        out = []
        for i in range(len(st)):
            p = pts[i, : npt[i]]
            out.append((float(cost[i]), list(_lib.DUBINS_WORDS[word[i]]), p[:, 0].copy(), p[:, 1].copy(), p[:, 2].tolist()))
        return out

    def generation(self, start_pose: tuple, goal_pose: tuple):
        """(best_cost, best_mode, x_list, y_list, yaw_list) of dubins_curve.py:238-313: the cost in
        curvature-normalised units, the mode as ["L", "S", "R"], x / y as arrays, yaw as a list."""
        return self._segments([tuple(start_pose)], [tuple(goal_pose)])[0]

    def run(self, points: list):
        """The curve through `points` [(x, y, yaw in degrees)] (:315-335): every segment in one launch,
        concatenated with the joints duplicated as the reference leaves them.  Returns (path_x, path_y,
        path_yaw); nothing is plotted."""
        assert len(points) >= 2, "Number of points should be at least 2."
        poses = [(p[0], p[1], np.deg2rad(p[2])) for p in points]
        path_x, path_y, path_yaw = [], [], []
        for _, _, x, y, yaw in self._segments(poses[:-1], poses[1:]):
            path_x.extend(x.tolist())
            path_y.extend(y.tolist())
            path_yaw.extend(yaw)
        return path_x, path_y, path_yaw


class ReedsShepp(Curve):
    """Reeds-Shepp curve generation (reeds_shepp.py:13-736): the car that can reverse.

    Parameters:
        step (float): Simulation or interpolation size
        max_curv (float): The maximum curvature of the curve

    The reference's word primitives (SLS .. LRSLR, _calTauOmega), its six planners and its Path class are
    the kernel's and are not methods here; batch.reeds_shepp_batch(slot_costs=True) returns every
    candidate's length.
    """

    MAX_ANGLE = 64.0  # |syaw| and |gyaw - syaw| beyond this are refused (include/pmp.h)

    def __init__(self, step: float, max_curv: float) -> None:
        super().__init__(step)
        self.max_curv = max_curv

    def __str__(self) -> str:
        return "Reeds Shepp Curve"

    def R(self, x, y):
        """The polar coordinates (r, theta) of the point (x, y) (:37-53)"""
        return math.hypot(x, y), math.atan2(y, x)

    def M(self, theta):
        """The angle brought into [-pi, pi] (:55-65)"""
        return self.pi2pi(theta)

    def generation_batch(self, start_poses, goal_poses, **kw):
        """batch.reeds_shepp_batch with this generator's step and max_curv (yaw in radians)."""
        return batch.reeds_shepp_batch(start_poses, goal_poses, self.step, self.max_curv, **kw)

    def cost_matrix(self, start_poses, goal_poses):
        """batch.reeds_shepp_cost_matrix with this generator's step and max_curv (yaw in radians)."""
        return batch.reeds_shepp_cost_matrix(start_poses, goal_poses, self.step, self.max_curv)

    def _raise(self, start, goal):
        """What the reference raises for a pair of status 4 (or that this package's limit refuses)"""
        syaw, gyaw = float(start[2]), float(goal[2])
        if math.isinf(syaw) or math.isinf(gyaw):  # math.cos(inf) / math.sin(inf) (:626, :106)
            raise ValueError("math domain error")
        if abs(syaw) > self.MAX_ANGLE or abs(gyaw - syaw) > self.MAX_ANGLE:
            raise ValueError(f"|start yaw| and |goal yaw - start yaw| must not exceed {self.MAX_ANGLE:g} radians")
        # no candidate below inf, or int(inf / step) (:640)
        raise OverflowError("cannot convert float infinity to integer")

    def _segments(self, starts, goals):
        """One launch -> per pair (cost, mode, x, y, yaw) as generation() returns them."""
        r = self.generation_batch(starts, goals)
        st = r["status"].cpu().numpy()
        for i in np.nonzero(st == _lib.STATUS_REF_RAISES)[0]:
            self._raise(starts[i], goals[i])
        cost, slot, npt = r["cost"].cpu().numpy(), r["slot"].cpu().numpy(), r["n_points"].cpu().numpy()
        pts = r["points"].cpu().numpy()
        out = []
        for i in range(len(st)):
            p = pts[i, : npt[i]]
            out.append((float(cost[i]), list(_lib.RS_WORDS[slot[i]]), p[:, 0].copy(), p[:, 1].copy(), p[:, 2].tolist()))
        return out

    def generation(self, start_pose: tuple, goal_pose: tuple):
        """(best_cost / max_curv, best_mode, x_list, y_list, yaw_list) of reeds_shepp.py:606-674: the
        mode as a list of 3 to 5 of "L", "S", "R", x / y as arrays, yaw as a list."""
        return self._segments([tuple(start_pose)], [tuple(goal_pose)])[0]

    def run(self, points: list):
        """The curve through `points` [(x, y, yaw in degrees)] (:676-696): every segment in one launch,
        concatenated with the joints duplicated as the reference leaves them.  Returns (path_x, path_y,
        path_yaw); nothing is plotted."""
        assert len(points) >= 2, "Number of points should be at least 2."
        poses = [(p[0], p[1], np.deg2rad(p[2])) for p in points]
        path_x, path_y, path_yaw = [], [], []
        for _, _, x, y, yaw in self._segments(poses[:-1], poses[1:]):
            path_x.extend(x.tolist())
            path_y.extend(y.tolist())
            path_yaw.extend(yaw)
        return path_x, path_y, path_yaw


class Polynomial(Curve):
    """Quintic polynomial curve generation (polynomial_curve.py:13-195): the first T of
    np.arange(t_min, t_max, step) whose trajectory keeps its peak acceleration and jerk under the limits.

    Parameters:
        step (float): The spacing of the candidate times T
        max_acc (float): Maximum acceleration
        max_jerk (float): Maximum jerk

    dt, t_min and t_max are instance attributes as in the reference (0.1, 1, 30), read at call time.  The
    reference's Poly class (the 3 x 3 boundary-value solve and its x / dx / ddx / dddx) is the kernel's and is
    not a class here.
    """

    def __init__(self, step: float, max_acc: float, max_jerk: float) -> None:
        super().__init__(step)
        self.max_acc = max_acc
        self.max_jerk = max_jerk
        self.dt = 0.1
        self.t_min = 1
        self.t_max = 30

    def __str__(self) -> str:
        return "Quintic Polynomial Curve"

    class Trajectory:
        """time, x, y, yaw, v, a, jerk as lists of floats (polynomial_curve.py:77-102)"""

        def __init__(self):
            self.clear()

        def clear(self):
            self.time = []
            self.x = []
            self.y = []
            self.yaw = []
            self.v = []
            self.a = []
            self.jerk = []

        @property
        def size(self):
            assert len(self.time) == len(self.x) and \
                   len(self.x) == len(self.y) and    \
                   len(self.y) == len(self.yaw) and  \
                   len(self.yaw) == len(self.v) and  \
                   len(self.v) == len(self.a) and    \
                   len(self.a) == len(self.jerk),    \
                   "Unequal dimensions of each attribute, this should not happen."
            return len(self.time)

    def _params(self):
        return dict(step=self.step, max_acc=self.max_acc, max_jerk=self.max_jerk, dt=self.dt, t_min=self.t_min,
                    t_max=self.t_max)

    def generation_batch(self, start_states, goal_states, **kw):
        """batch.polynomial_batch with this generator's parameters (states x, y, yaw in radians, v, a)."""
        return batch.polynomial_batch(start_states, goal_states, **self._params(), **kw)

    def time_matrix(self, start_states, goal_states):
        """batch.polynomial_time_matrix with this generator's parameters."""
        return batch.polynomial_time_matrix(start_states, goal_states, **self._params())

    def _segments(self, starts, goals):
        """One launch -> a Trajectory per pair, empty where no T is feasible."""
        r = self.generation_batch(starts, goals)
        npt, pts = r["n_points"].cpu().numpy(), r["points"].cpu().numpy()
        out = []
        for i in range(len(npt)):
            traj = self.Trajectory()
            p = pts[i, : npt[i]]
            for c, name in enumerate(("time", "x", "y", "yaw", "v", "a", "jerk")):
                setattr(traj, name, p[:, c].tolist())
            out.append(traj)
        return out

    def generation(self, start_pose: tuple, goal_pose: tuple):
        """The first trajectory that satisfies the acceleration and jerk constraints (:104-164), from
        start_pose to goal_pose (x, y, yaw in radians, v, a); an empty Trajectory where none does."""
        return self._segments([tuple(start_pose)], [tuple(goal_pose)])[0]

    def run(self, points: list):
        """The curve through `points` [(x, y, yaw in degrees)] (:166-195) with the reference's heuristic
        speeds (0, then 1) and accelerations: every segment in one launch, concatenated.  Returns (path_x,
        path_y, path_yaw); nothing is plotted."""
        assert len(points) >= 2, "Number of points should be at least 2."
        v = [0]
        for i in range(len(points) - 1):
            v.append(1.0)
        a = [(v[i + 1] - v[i]) / 5 for i in range(len(points) - 1)]
        a.append(0)
        states = [(p[0], p[1], np.deg2rad(p[2]), v[i], a[i]) for i, p in enumerate(points)]
        path_x, path_y, path_yaw = [], [], []
        for traj in self._segments(states[:-1], states[1:]):
            path_x.extend(traj.x)
            path_y.extend(traj.y)
            path_yaw.extend(traj.yaw)
        return path_x, path_y, path_yaw


class Bezier(Curve):
    """Bezier curve generation (bezier_curve.py:13-111).

    Parameters:
        step (float): Simulation or interpolation size
        offset (float): The offset of control points
    """

    def __init__(self, step: float, offset: float) -> None:
        super().__init__(step)
        self.offset = offset

    def __str__(self) -> str:
        return "Bezier Curve"

    def generation_batch(self, start_poses, goal_poses, **kw):
        """batch.bezier_batch with this generator's step and offset (yaw in radians)."""
        return batch.bezier_batch(start_poses, goal_poses, self.step, self.offset, **kw)

    def _segments(self, starts, goals):
        """One launch -> per pair (points, control_points) as generation() returns them."""
        r = self.generation_batch(starts, goals)
        st = r["status"].cpu().numpy()
        for i in np.nonzero(st == _lib.STATUS_REF_RAISES)[0]:  # int() of hypot / step (:49)
            if any(math.isnan(float(v)) for v in tuple(starts[i])[:2] + tuple(goals[i])[:2]):
                raise ValueError("cannot convert float NaN to integer")
            raise OverflowError("cannot convert float infinity to integer")
        npt, pts, ctrl = r["n_points"].cpu().numpy(), r["points"].cpu().numpy(), r["control"].cpu().numpy()
        return [([pts[i, k].copy() for k in range(npt[i])], [(c[0], c[1]) for c in ctrl[i]]) for i in range(len(st))]

    def generation(self, start_pose: tuple, goal_pose: tuple):
        """(points, control_points) of bezier_curve.py:34-53: the int(hypot / step) points as arrays of
        shape (2,), the four control points as (x, y) tuples."""
        return self._segments([tuple(start_pose)], [tuple(goal_pose)])[0]

    def bezier(self, t: float, control_points: list) -> np.ndarray:
        """The point at t of the Bezier curve of any number of control points (:55-69), on the host."""
        n = len(control_points) - 1
        control_points = np.array(control_points)
        return np.sum([math.comb(n, i) * t ** i * (1 - t) ** (n - i) * control_points[i] for i in range(n + 1)], axis=0)

    def getControlPoints(self, start_pose: tuple, goal_pose: tuple):
        """The four control points of a pose pair (:71-89), on the host."""
        sx, sy, syaw = start_pose
        gx, gy, gyaw = goal_pose
        dist = np.hypot(sx - gx, sy - gy) / self.offset
        return [(sx, sy), (sx + dist * np.cos(syaw), sy + dist * np.sin(syaw)),
                (gx - dist * np.cos(gyaw), gy - dist * np.sin(gyaw)), (gx, gy)]

    def run(self, points: list):
        """The curve through `points` [(x, y, yaw in degrees)] (:91-111): every segment in one launch,
        concatenated.  Returns (path_x, path_y); nothing is plotted."""
        assert len(points) >= 2, "Number of points should be at least 2."
        poses = [(p[0], p[1], np.deg2rad(p[2])) for p in points]
        path_x, path_y = [], []
        for path, _ in self._segments(poses[:-1], poses[1:]):
            for pt in path:
                path_x.append(pt[0])
                path_y.append(pt[1])
        return path_x, path_y


class BSpline(Curve):
    """B-spline curve generation through a waypoint list (bspline_curve.py:12-271).

    Parameters:
        step (float): Simulation or interpolation size: int(1 / step) samples
        k (int): Degree of curve (1..5 on the kernel)
        param_mode (str): "centripetal" | "chord_length" | "uniform_spaced"
        spline_mode (str): "interpolation" | "approximation"

    run() and the four stage methods read their result from one launch of pmp_bspline_batch (at most 64
    waypoints; the entry refuses more with PMPError); generation() and baseFunction() run on the host.
    approximation with fewer than k + 2 waypoints, outside the reference's own precondition N > H > k, raises
    NotImplementedError.
    """

    _three_d = False

    def __init__(self, step: float, k: int, param_mode: str = "centripetal", spline_mode: str = "interpolation") -> None:
        super().__init__(step)
        self.k = k
        assert param_mode in _lib.BSPLINE_PARAM_MODES, "Parameter selection mode error!"
        self.param_mode = param_mode
        assert spline_mode in _lib.BSPLINE_SPLINE_MODES, "Spline mode selection error!"
        self.spline_mode = spline_mode

    def __str__(self) -> str:
        return "B-Spline Curve"

    def baseFunction(self, i: int, k: int, t: float, knot: list):
        """N_{i,k}(t) by the Cox-de Boor recursion with the reference's half-open degree-0 test and its
        zero-length guards (:42-70), on the host."""
        if k == 0:
            return 1.0 if knot[i] <= t < knot[i + 1] else 0.0
        left, right = knot[i + k] - knot[i], knot[i + k + 1] - knot[i + 1]
        value = 0.0
        if left:
            value = (t - knot[i]) / left * self.baseFunction(i, k - 1, t, knot)
        if right:
            value = value + (knot[i + k + 1] - t) / right * self.baseFunction(i + 1, k - 1, t, knot)
        return value

    def _cut(self, points):
        """The waypoints as an [n, 2] array: the 2D class keeps x and y (:229-230)."""
        return np.asarray([(p[0], p[1]) for p in points], np.float64).reshape(-1, 2)

    def _stage(self, points, spline_mode="interpolation", params=None, knot=None):
        """One launch without samples for the stage methods: its outputs on the host."""
        r = batch.bspline_batch([self._cut(points)], 0.5, self.k, self.param_mode, spline_mode, cost_only=True,
                                three_d=self._three_d, params=params, knot=knot)
        return {key: v.cpu().numpy()[0] for key, v in r.items() if hasattr(v, "cpu")}

    def paramSelection(self, points: list):
        """The parameters of the waypoints as a list (:72-104)"""
        return self._stage(points)["params"][: len(points)].tolist()

    def knotGeneration(self, param: list, n: int):
        """The knot vector [n + k + 1] of n parameters as a list (:106-127)"""
        r = self._stage(np.zeros((n, 2)), params=np.asarray(param, np.float64)[None, :n])
        return r["knot"][: n + self.k + 1].tolist()

    def _given(self, points, param, knot):
        n = len(points)
        return (np.asarray(param, np.float64)[None, :n], np.asarray(knot, np.float64)[None, : n + self.k + 1])

    def interpolation(self, points: list, param: list, knot: list):
        """The n control points of the curve through the waypoints, as an array [n, dim] (:129-154)"""
        p, kn = self._given(points, param, knot)
        r = self._stage(points, params=p, knot=kn)
        if r["status"] == _lib.STATUS_REF_RAISES:
            raise np.linalg.LinAlgError("Singular matrix")
        return r["control"][: len(points)].copy()

    def approximation(self, points: list, param: list, knot: list):
        """The n - 1 control points of the least-squares curve with fixed ends, as an array (:156-195)"""
        if len(points) < self.k + 2:
            raise NotImplementedError("approximation needs at least k + 2 waypoints (N > H > k)")
        p, kn = self._given(points, param, knot)
        r = self._stage(points, "approximation", params=p, knot=kn)
        if r["status"] == _lib.STATUS_REF_RAISES:
            raise np.linalg.LinAlgError("Singular matrix")
        return r["control"][: len(points) - 1].copy()

    def generation(self, t, k, knot, control_pts):
        """The curve's points at the parameter values t, as an array [len(t), dim] (:197-217), on the host."""
        control_pts = np.asarray(control_pts)
        N = np.array([[self.baseFunction(j, k, ti, knot) for j in range(len(control_pts))] for ti in t], np.float64)
        N = N.reshape(len(t), len(control_pts))
        N[len(t) - 1][len(control_pts) - 1] = 1
        return N @ control_pts

    def run_batch(self, point_lists, **kw):
        """run() of many waypoint lists (all 2D or all 3D) in one launch: a list of run()'s results."""
        lists = [self._cut(p) for p in point_lists]
        for p in lists:
            assert len(p) >= 2, "Number of points should be at least 2."
        if batch.bspline_samples(self.step, self._three_d) == 0:  # N[len(t) - 1] of an empty N (:215)
            raise IndexError("index -1 is out of bounds for axis 0 with size 0")
        if self.spline_mode == "approximation" and any(len(p) < self.k + 2 for p in lists):
            raise NotImplementedError("approximation needs at least k + 2 waypoints (N > H > k)")
        r = batch.bspline_batch(lists, self.step, self.k, self.param_mode, self.spline_mode, three_d=self._three_d, **kw)
        if np.any(r["status"].cpu().numpy() == _lib.STATUS_REF_RAISES):  # np.linalg.inv (:150, :191)
            raise np.linalg.LinAlgError("Singular matrix")
        return [[tuple(row) for row in curve] for curve in r["points"].cpu().numpy().tolist()]

    def run(self, points: list, display: bool = True):
        """The curve through (or near) `points` (:219-271): [(x, y), ...] of Python floats; 3-tuples are cut
        to (x, y).  Nothing is plotted, whatever `display` says."""
        assert len(points) >= 2, "Number of points should be at least 2."
        return self.run_batch([points])[0]


class BSpline3D(BSpline):
    """B-spline curve generation in 2D or 3D (bspline_curve3d.py:13-220): BSpline with the Euclidean norm in
    the points' own dimension, parameters 0 where all points coincide, and at least two samples.  run() returns
    tuples in the native dimension."""

    _three_d = True

    def __str__(self) -> str:
        return "B-Spline Curve 3D"

    def _cut(self, points):
        P = np.asarray(points, dtype=np.float64)
        P = P.reshape(len(P), -1)
        assert P.shape[1] in (2, 3), "BSpline3D supports 2D or 3D points."
        return P


class CubicSpline(Curve):
    """Cubic spline generation through a waypoint list, parametrised by arc length (cubic_spline.py:13-128).

    Parameters:
        step (float): Simulation or interpolation size
    """

    def __init__(self, step: float) -> None:
        super().__init__(step)

    def __str__(self) -> str:
        return "Cubic Spline"

    def spline(self, x_list: list, y_list: list, t: list):
        """The natural cubic spline y(x) through (x_list, y_list) at the values of t inside
        [x_list[0], x_list[-1]]: (p, dp), its values and first derivatives (:32-79), on the host."""
        x, a = np.asarray(x_list, np.float64), np.asarray(y_list, np.float64)
        h, num = np.diff(x), len(x)
        A, B = np.zeros((num, num)), np.zeros(num)
        A[0, 0] = A[num - 1, num - 1] = 1.0
        for i in range(1, num - 1):
            A[i, i - 1 : i + 2] = h[i - 1], 2.0 * (h[i - 1] + h[i]), h[i]
            B[i] = 3.0 * (a[i + 1] - a[i]) / h[i] - 3.0 * (a[i] - a[i - 1]) / h[i - 1]
        c = np.linalg.solve(A, B)
        d = [(c[i + 1] - c[i]) / (3.0 * h[i]) for i in range(num - 1)]
        b = [(a[i + 1] - a[i]) / h[i] - h[i] * (c[i + 1] + 2.0 * c[i]) / 3.0 for i in range(num - 1)]
        p, dp = [], []
        for it in t:
            if it < x[0] or it > x[-1]:
                continue
            i = int(np.searchsorted(x, it, side="right")) - 1
            dx = it - x[i]
            p.append(a[i] + b[i] * dx + c[i] * dx ** 2 + d[i] * dx ** 3)
            dp.append(b[i] + 2.0 * c[i] * dx + 3.0 * d[i] * dx ** 2)
        return p, dp

    def generation(self, start_pose: tuple, goal_pose: tuple):
        pass

    def _xy(self, points):
        if len(points[0]) not in (2, 3):
            raise NotImplementedError
        return np.asarray([(p[0], p[1]) for p in points], np.float64).reshape(-1, 2)

    def run_batch(self, point_lists, **kw):
        """run() of many waypoint lists in one launch: a list of (path_x, path_y, path_yaw)."""
        lists = []
        for p in point_lists:
            assert len(p) >= 2, "Number of points should be at least 2."
            lists.append(self._xy(p))
        r = batch.cubic_spline_batch(lists, self.step, **kw)
        if np.any(r["status"].cpu().numpy() == _lib.STATUS_REF_RAISES):  # np.arange(0, s[-1], step) (:107)
            raise ValueError("arange: cannot compute length")
        npt, pts = r["n_points"].cpu().numpy(), r["points"].cpu().numpy()
        return [(pts[i, : npt[i], 0].tolist(), pts[i, : npt[i], 1].tolist(), pts[i, : npt[i], 2].tolist())
                for i in range(len(lists))]

    def run(self, points: list):
        """The spline through `points` [(x, y) or (x, y, anything)] (:84-111), sampled every `step` of arc
        length.  Returns (path_x, path_y, path_yaw) as lists: the reference only plots them and returns None;
        returning the path follows Dubins.run here.  Nothing is plotted."""
        assert len(points) >= 2, "Number of points should be at least 2."
        return self.run_batch([points])[0]
