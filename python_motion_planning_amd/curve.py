"""Drop-in curve generation (curve_generation/ of the reference) on the gfx950 kernels:

  Curve    curve_generation/curve.py:10-64         the base: step, trigonometric, pi2pi, mod2pi, length
  Dubins   curve_generation/dubins_curve.py:14-335 pmp_dubins_batch / pmp_dubins_cost_matrix
  ReedsShepp curve_generation/reeds_shepp.py:13-736 pmp_reeds_shepp_batch / pmp_reeds_shepp_cost_matrix

Same constructor, generation() return values and run() input (yaw in degrees) as the reference; run() does
not plot (as Planner.run, planner.py:31-33).  Many pose pairs at once: generation_batch and cost_matrix of
either class, or batch.dubins_batch / batch.dubins_cost_matrix and batch.reeds_shepp_batch /
batch.reeds_shepp_cost_matrix.  Dubins.generation() returns its cost in curvature-normalised units and
ReedsShepp.generation() in the units of x and y, as the reference's do.  CurveFactory builds "dubins" only:
construct ReedsShepp directly.  There is no CPU fallback: without the library or a HIP device the calls
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
