"""Sample-search planners: drop-in RRT / RRTStar / InformedRRT (global_planner/sample_search/) on the
gfx950 kernel rrt.hip, and RRTConnect on rrt_connect.hip.

plan() keeps the reference's signature, return convention and its use of the global numpy RNG:
the draws generateRandomNode (rrt.py:91-103) would make are read from a copy of np.random's
state, and afterwards the global generator is advanced by exactly the number the kernel
consumed, so a caller's later np.random draws are unchanged.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib, batch
from .env import Map, Node
from .planner import Planner


def random_stream(sample_num: int, state=None) -> np.ndarray:
    """The doubles generateRandomNode would draw from np.random (or from `state`): at most
    3 per iteration, in RandomState.random_sample order."""
    rs = np.random.RandomState()
    rs.set_state(np.random.get_state() if state is None else state)
    return rs.random_sample(3 * int(sample_num) + 1)


def _tree_nodes(out, n: int, t=None):
    """(nodes, g, parent): the first n nodes of query 0's tree (t: which of RRT-Connect's two) as
    Node(current, the parent's coordinates, g, 0), and the g and parent-index columns they were built from."""
    xy, g, par = (batch.query0(out, k, n, t) for k in ("tree_xy", "tree_g", "tree_parent"))
    nodes = [Node((float(xy[i, 0]), float(xy[i, 1])), (float(xy[par[i], 0]), float(xy[par[i], 1])), float(g[i]), 0)
             for i in range(n)]
    return nodes, g, par


def _path_points(out) -> list:
    """Query 0's path as [(x, y), ...] of Python floats."""
    return [(float(x), float(y)) for x, y in batch.query0(out, "path", int(out["path_len"][0]))]


class SampleSearcher(Planner):
    """global_planner/sample_search/sample_search.py:13-135 (collision tests run on the device)."""

    def __init__(self, start: tuple, goal: tuple, env: Map, delta: float = 0.5) -> None:
        super().__init__(start, goal, env)
        self.delta = delta


class RRT(SampleSearcher):
    """Rapidly-exploring Random Tree (rrt.py:14-151)."""

    STAR = False

    def __init__(self, start: tuple, goal: tuple, env: Map, max_dist: float = 0.5, sample_num: int = 10000,
                 goal_sample_rate: float = 0.05) -> None:
        super().__init__(start, goal, env)
        self.max_dist = max_dist
        self.sample_num = sample_num
        self.goal_sample_rate = goal_sample_rate
        self.r = 10.0

    def __str__(self) -> str:
        return "Rapidly-exploring Random Tree(RRT)"

    def plan(self) -> tuple:
        """(cost, path goal->start, expand list of Node) or (0, None, expand) (rrt.py:49-83)."""
        rnd = random_stream(self.sample_num)
        out = batch.rrt_batch(self.env, [self.start.current], [self.goal.current], rnd[None], self.sample_num,
                              star=self.STAR, max_dist=self.max_dist, radius=self.r,
                              goal_sample_rate=self.goal_sample_rate, delta=self.delta)
        st = int(out["status"][0])
        draws = int(out["draws"][0])
        if draws:
            np.random.random_sample(draws)  # advance the global RNG exactly as the reference's loop does
        if st not in (0, 1):
            raise RuntimeError(f"RRT kernel status {st}")
        n = int(out["n_nodes"][0])
        expand, g, par = _tree_nodes(out, n)
        # the start and goal keep the caller's coordinates (ints in the README examples)
        expand[0] = self.start
        if st == 1:
            return 0, None, expand
        self.goal.parent = expand[int(par[n - 1])].current
        self.goal.g = float(g[n - 1])
        expand[-1] = self.goal
        path = _path_points(out)
        path[0], path[-1] = self.goal.current, self.start.current
        return float(out["cost"][0]), path, expand

    def run(self):
        return self.plan()

    @staticmethod
    def plan_batch(env: Map, starts, goals, rnd, sample_num: int, star: bool = False, **kw):
        """Independent queries on one Map; rnd [nq, stride] random streams.  Device-tensor dict."""
        return batch.rrt_batch(env, starts, goals, rnd, sample_num, star=star, **kw)


class RRTStar(RRT):
    """RRT* (rrt_star.py:11-76): choose-parent and rewire within radius r."""

    STAR = True

    def __init__(self, start: tuple, goal: tuple, env: Map, max_dist: float = 0.5, sample_num: int = 10000,
                 r: float = 10.0, goal_sample_rate: float = 0.05) -> None:
        super().__init__(start, goal, env, max_dist, sample_num, goal_sample_rate)
        self.r = r

    def __str__(self) -> str:
        return "RRT*"

    @staticmethod
    def plan_batch(env: Map, starts, goals, rnd, sample_num: int, star: bool = True, **kw):
        return batch.rrt_batch(env, starts, goals, rnd, sample_num, star=star, **kw)


class InformedRRT(RRTStar):
    """Informed RRT* (informed_rrt.py:36-152): RRT* that keeps planning after the goal is connected,
    sampling from the ellipse of paths no longer than the best one found."""

    def __init__(self, start: tuple, goal: tuple, env: Map, max_dist: float = 0.5, sample_num: int = 1500,
                 r: float = 12.0, goal_sample_rate: float = 0.05) -> None:
        # informed_rrt.py:61 hands goal_sample_rate to RRTStar's `r` slot: the caller's rate is dropped
        # and RRT's default 0.05 applies, whatever is passed
        super().__init__(start, goal, env, max_dist, sample_num, goal_sample_rate)
        self.r = r
        self.c_best = float("inf")
        self.c_min = math.hypot(self.goal.x - self.start.x, self.goal.y - self.start.y)

    def __str__(self) -> str:
        return "Informed RRT*"

    def plan(self) -> tuple:
        """(best_cost, best path goal->start, expand list of Node) or (inf, None, expand)
        (informed_rrt.py:74-112).  The ellipse sampler's draw count has no bound: the stream starts at
        4*sample_num+64 doubles and doubles while the kernel reports that it ran out (the re-run reads
        the same draws, so the result does not depend on the stream's length)."""
        state = np.random.get_state()
        stride = 4 * int(self.sample_num) + 64
        for _ in range(16):
            rs = np.random.RandomState()
            rs.set_state(state)
            rnd = rs.random_sample(stride)
            out = batch.informed_rrt_batch(self.env, [self.start.current], [self.goal.current], rnd[None],
                                           self.sample_num, max_dist=self.max_dist, radius=self.r, delta=self.delta,
                                           goal_sample_rate=self.goal_sample_rate)
            st = int(out["status"][0])
            if st != _lib.STATUS_CAP_OVERFLOW:
                break
            stride *= 2
        n = int(out["n_nodes"][0])
        draws = int(out["draws"][0])
        if st not in (0, 1):
            # (4: the reference's extractPath would never return; 3 here: no try lands in the map)
            raise RuntimeError(f"Informed RRT* kernel status {st}")
        if draws:
            np.random.random_sample(draws)  # advance the global RNG exactly as the reference's loop does
        expand, g, par = _tree_nodes(out, n)
        # the start and goal keep the caller's coordinates (ints in the README examples)
        expand[0] = self.start
        if st == 1:
            return float("inf"), None, expand
        gs = int(out["goal_slot"][0])
        self.goal.parent = expand[int(par[gs])].current
        self.goal.g = float(g[gs])
        expand[gs] = self.goal
        path = _path_points(out)
        path[0], path[-1] = self.goal.current, self.start.current
        self.c_best = float(out["best_cost"][0])
        return self.c_best, path, expand

    @staticmethod
    def plan_batch(env: Map, starts, goals, rnd, sample_num: int, **kw):
        """Independent queries on one Map; rnd [nq, stride] random streams.  Device-tensor dict."""
        return batch.informed_rrt_batch(env, starts, goals, rnd, sample_num, **kw)


class RRTConnect(RRT):
    """RRT-Connect (rrt_connect.py:13-147): a tree from the start and one from the goal, each iteration
    extending one towards a sample and the other greedily towards the new node until they meet."""

    def __init__(self, start: tuple, goal: tuple, env: Map, max_dist: float = 0.5, sample_num: int = 10000,
                 goal_sample_rate: float = 0.05) -> None:
        super().__init__(start, goal, env, max_dist, sample_num, goal_sample_rate)

    def __str__(self) -> str:
        return "RRT-Connect"

    def plan(self) -> tuple:
        """(cost, path start->goal, expand list of Node) or (0, None, None) (rrt_connect.py:42-90).
        expand is getExpand's interleave (rrt_connect.py:128-147): sample_list_f and sample_list_b of the
        last iteration, index by index, the forward one first.  The trees start at batch.rrt_connect_batch's
        default capacity, which doubles while the kernel reports that a tree outgrew it (the re-run reads
        the same draws, so the result does not depend on the capacity)."""
        rnd = random_stream(self.sample_num)
        cap = batch.RRT_CONNECT_DEFAULT_CAP
        for _ in range(16):
            out = batch.rrt_connect_batch(self.env, [self.start.current], [self.goal.current], rnd[None],
                                          self.sample_num, max_dist=self.max_dist,
                                          goal_sample_rate=self.goal_sample_rate, delta=self.delta, cap=cap)
            st = int(out["status"][0])
            if st != _lib.STATUS_CAP_OVERFLOW:
                break
            cap *= 2
        if st not in (0, 1):
            # (4: the reference's extractPath would never return)
            raise RuntimeError(f"RRT-Connect kernel status {st}")
        draws = int(out["draws"][0])
        if draws:
            np.random.random_sample(draws)  # advance the global RNG exactly as the reference's loop does
        if st == 1:
            return 0, None, None
        counts = out["n_nodes"][0].cpu().numpy()
        roots = (self.start, self.goal)
        trees = []
        for t in (0, 1):
            nodes = _tree_nodes(out, int(counts[t]), t)[0]
            # the roots keep the caller's coordinates (ints in the README examples)
            nodes[0] = roots[t]
            trees.append(nodes)
        fw = int(out["forward"][0])
        f, b = trees[fw], trees[1 - fw]
        expand = []
        for k in range(max(len(f), len(b))):
            if k < len(f):
                expand.append(f[k])
            if k < len(b):
                expand.append(b[k])
        path = _path_points(out)
        path[0], path[-1] = self.start.current, self.goal.current
        return float(out["cost"][0]), path, expand

    @staticmethod
    def plan_batch(env: Map, starts, goals, rnd, sample_num: int, **kw):
        """Independent queries on one Map; rnd [nq, stride] random streams.  Device-tensor dict."""
        return batch.rrt_connect_batch(env, starts, goals, rnd, sample_num, **kw)
