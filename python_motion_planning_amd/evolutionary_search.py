"""Evolutionary global planners: drop-in for global_planner/evolutionary_search/ (evolutionary_search.py:11-87,
pso.py:18-356, aco.py:14-186).  ACO.plan() runs the whole colony in one launch of pmp_aco_batch (csrc/aco.hip),
which draws from MT19937 itself: the draw count depends on every earlier draw, so the generator's state goes in
and comes back.  PSO.plan() runs the whole swarm in one launch of pmp_pso_batch (csrc/pso.hip): the initial
positions are drawn on the host from the global `random` (their draw count depends on the draws), the
iterations' draws, whose count is fixed, are handed to the kernel as a stream.

`random` and numpy's RandomState share MT19937 and the construction of a double from two outputs, so the
stream is taken by copying the generator's words into a RandomState, and the global `random` is left exactly
where the reference's random.random() calls would have left it (random_stream).
"""
from __future__ import annotations

import math
import random

import numpy as np

from . import batch
from ._lib import STATUS_REF_INDEX_ERROR
from .curve import BSpline
from .env import Grid, Node
from .planner import Planner

GEN_MODE_CIRCLE = 0
GEN_MODE_RANDOM = 1


def random_stream(n: int, state=None):
    """(the n doubles random.random() would return next, the state random.setstate() takes after them), from
    the global generator's state or from `state` (a random.getstate() tuple).  gauss_next is kept."""
    version, words, gauss_next = random.getstate() if state is None else state
    rs = np.random.RandomState()
    rs.set_state(("MT19937", np.array(words[:624], dtype=np.uint32), int(words[624])))
    out = rs.random_sample(int(n))
    after = rs.get_state()
    return out, (version, tuple(int(w) for w in after[1]) + (int(after[2]),), gauss_next)


class EvolutionarySearcher(Planner):
    """Base class of the evolutionary planners (evolutionary_search.py:11-87)."""

    def __init__(self, start: tuple, goal: tuple, env: Grid, heuristic_type: str = "euclidean") -> None:
        super().__init__(start, goal, env)
        self.heuristic_type = heuristic_type
        self.motions = self.env.motions
        self.obstacles = self.env.obstacles

    def h(self, node: Node, goal: Node) -> float:
        if self.heuristic_type == "manhattan":
            return abs(goal.x - node.x) + abs(goal.y - node.y)
        elif self.heuristic_type == "euclidean":
            return math.hypot(goal.x - node.x, goal.y - node.y)

    def cost(self, node1: Node, node2: Node) -> float:
        if self.isCollision(node1, node2):
            return float("inf")
        return self.dist(node1, node2)

    def isCollision(self, node1: Node, node2: Node) -> bool:
        """An endpoint in an obstacle, or a diagonal move with an obstacle in one of the two cells beside it
        (evolutionary_search.py:61-87), as GraphSearcher.isCollision.  One difference shows on moves longer than
        a grid step, which the graph searchers never make: where x and y run in opposite directions by unequal
        amounts, the reference's pairing of minima and maxima names the endpoints again, so nothing more is
        tested."""
        obs = self.obstacles
        if node1.current in obs or node2.current in obs:
            return True
        dx, dy = node2.x - node1.x, node2.y - node1.y
        if dx == 0 or dy == 0 or (dx * dy < 0 and dx != -dy):
            return False
        return (node1.x, node2.y) in obs or (node2.x, node1.y) in obs


def _initial_positions(rng, start, goal, x_range, y_range, n_particles, point_num, init_mode) -> list:
    """PSO.initializePositions (pso.py:125-184) with `rng` (the `random` module or a random.Random) as the source."""
    x_order, y_order = goal[0] > start[0], goal[1] > start[1]
    if init_mode == GEN_MODE_CIRCLE:
        center_x, center_y = (start[0] + goal[0]) / 2, (start[1] + goal[1]) / 2
        half = math.hypot(goal[0] - start[0], goal[1] - start[1]) / 2.0
        radius = 5 if half < 5 else half
    positions = []
    for _ in range(n_particles):
        visited, pts_x, pts_y = [], [], []
        while len(visited) < point_num:
            if init_mode == GEN_MODE_RANDOM:
                pt_x = rng.randint(start[0], goal[0])
                pt_y = rng.randint(start[1], goal[1])
            else:
                angle = rng.random() * 2 * math.pi
                r = math.sqrt(rng.random()) * radius
                pt_x = int(center_x + r * math.cos(angle))
                pt_y = int(center_y + r * math.sin(angle))
                if not (0 <= pt_x < x_range and 0 <= pt_y < y_range):
                    continue
            pos_id = pt_x + x_range * pt_y
            if pos_id not in visited:
                visited.append(pos_id)
                pts_x.append(pt_x)
                pts_y.append(pt_y)
        pts_x = sorted(pts_x, reverse=not x_order)
        pts_y = sorted(pts_y, reverse=not y_order)
        positions.append(list(zip(pts_x, pts_y)))
    return positions


class PSO(EvolutionarySearcher):
    """Particle Swarm Optimization (PSO) motion planning (pso.py:18-356); the swarm runs on the device.

    Parameters:
        start (tuple), goal (tuple), env (Grid), heuristic_type (str): as EvolutionarySearcher
        n_particles (int): number of particles
        point_num (int): number of position points contained in each particle (1..62 on the kernel)
        w_inertial, w_cognitive, w_social (float): the weights.  best_pos is position in the reference (the same
            list), so the cognitive term is always w_cognitive * rand1 * 0
        max_speed (int): the maximum velocity of particle motion
        max_iter (int): maximum iterations
        init_mode (int): GEN_MODE_CIRCLE or GEN_MODE_RANDOM

    The swarm's state lives in one workgroup's LDS: two copies of it beside the waves' curve states must fit
    160 KiB (at point_num 5 about 430 particles with 16 waves and 600 with one; the entry launches fewer waves
    where that makes a swarm fit); a larger swarm, which the reference would run, raises PMPError.

    plan() may be called once per object: the reference's second call appends another swarm to `particles` and
    iterates both; here it raises RuntimeError.
    """

    def __init__(self, start: tuple, goal: tuple, env: Grid, heuristic_type: str = "euclidean",
                 n_particles: int = 300, point_num: int = 5, w_inertial: float = 1.0,
                 w_cognitive: float = 1.0, w_social: float = 1.0, max_speed: int = 6,
                 max_iter: int = 200, init_mode: int = GEN_MODE_RANDOM) -> None:
        super().__init__(start, goal, env, heuristic_type)
        self.max_iter = max_iter
        self.n_particles = n_particles
        self.w_inertial = w_inertial
        self.w_social = w_social
        self.w_cognitive = w_cognitive
        self.point_num = point_num
        self.init_mode = init_mode
        self.max_speed = max_speed

        self.particles = []
        self.inherited_particles = []
        self.best_particle = self.Particle()
        self.b_spline_gen = BSpline(step=0.01, k=4)
        self.repeats = None  # after plan(): the evaluations the kernel threw away (batch.pso_batch)
        self._planned = False

    def __str__(self) -> str:
        return "Particle Swarm Optimization (PSO)"

    class Particle:
        def __init__(self) -> None:
            self.reset()

        def reset(self):
            self.position = []
            self.velocity = []
            self.fitness = -1
            self.best_pos = []
            self.best_fitness = -1

    def _launch(self, init_positions, rnd, n_particles, max_iter, **kw):
        return batch.pso_batch(self.env, [self.start.current], [self.goal.current],
                               np.asarray(init_positions, np.int32).reshape(1, n_particles, self.point_num, 2),
                               np.asarray(rnd, np.float64)[None], n_particles, self.point_num, max_iter, self.w_inertial,
                               self.w_cognitive, self.w_social, self.max_speed, **kw)

    def plan(self, verbose: bool = False):
        """(cost, path [(x, y), ...], fitness_history) (pso.py:77-123): one launch.  The global `random` ends
        where the reference's draws would leave it.  Raises numpy.linalg.LinAlgError where the reference's last
        line does (a best fitness of inf)."""
        if self._planned:
            raise RuntimeError("PSO.plan() was already called on this object (the reference would append a second "
                               "swarm to the first); construct a new PSO")
        init_positions = self.initializePositions()
        rnd, after = random_stream(batch.pso_draws(self.n_particles, self.point_num, self.max_iter))
        out = self._launch(init_positions, rnd, self.n_particles, self.max_iter)
        host = {k: v[0].cpu().numpy() for k, v in out.items() if v is not None}
        random.setstate(after)
        self._planned = True
        self.repeats = int(host["repeats"])
        for i in range(self.n_particles):
            p = self.Particle()
            p.position = [(int(x), int(y)) for x, y in host["positions"][i]]
            p.velocity = [(float(x), float(y)) for x, y in host["velocities"][i]]
            p.best_pos = p.position
            p.fitness = float(host["fitness"][i])
            p.best_fitness = float(host["particle_best_fitness"][i])
            self.particles.append(p)
        self.best_particle.fitness = float(host["best_fitness"])
        self.best_particle.position = [(int(x), int(y)) for x, y in host["best_position"]]
        fitness_history = [float(f) for f in host["fitness_history"]]
        if verbose:
            for i, f in enumerate(fitness_history):
                print(f"iteration {i}: best fitness = {f}")
        if int(host["status"]) != 0:
            raise np.linalg.LinAlgError("Singular matrix")
        path = [(float(x), float(y)) for x, y in host["points"]]
        return float(host["length"]), path, fitness_history

    @staticmethod
    def plan_batch(env: Grid, starts, goals, seeds_or_states, n_particles: int = 300, point_num: int = 5,
                   w_inertial: float = 1.0, w_cognitive: float = 1.0, w_social: float = 1.0, max_speed: int = 6,
                   max_iter: int = 200, init_mode: int = GEN_MODE_RANDOM, **kw):
        """Independent plans on one Grid in one launch.  seeds_or_states: per plan an int (random.seed's) or a
        random.getstate() tuple; each plan draws its initial positions and its stream from a generator of its
        own, as PSO(...).plan() does after random.seed(seed).  Returns batch.pso_batch's device-tensor dict with
        init_positions (numpy [nq, n_particles, point_num, 2]) and random_states (each generator's state after
        its plan) added."""
        inits, streams, states = [], [], []
        draws = batch.pso_draws(n_particles, point_num, max_iter)
        for s, g, seed in zip(starts, goals, seeds_or_states):
            rng = random.Random()
            if isinstance(seed, tuple):
                rng.setstate(seed)
            else:
                rng.seed(seed)
            inits.append(_initial_positions(rng, tuple(s), tuple(g), env.x_range, env.y_range, n_particles, point_num,
                                            init_mode))
            rnd, after = random_stream(draws, rng.getstate())
            streams.append(rnd)
            states.append(after)
        init = np.asarray(inits, np.int32).reshape(len(inits), n_particles, point_num, 2)
        out = batch.pso_batch(env, np.asarray(starts, np.int32), np.asarray(goals, np.int32), init,
                              np.asarray(streams, np.float64).reshape(len(inits), -1), n_particles, point_num, max_iter,
                              w_inertial, w_cognitive, w_social, max_speed, **kw)
        out["init_positions"] = init
        out["random_states"] = states
        return out

    def initializePositions(self) -> list:
        """n_particles lists of point_num unique points between start and goal (GEN_MODE_RANDOM) or inside the
        circle on them (GEN_MODE_CIRCLE), x and y each sorted towards the goal (pso.py:125-184).  Runs on the
        host from the global `random`; a start beyond the goal in GEN_MODE_RANDOM raises random.randint's own
        ValueError, as the reference does."""
        return _initial_positions(random, self.start.current, self.goal.current, self.env.x_range, self.env.y_range,
                                  self.n_particles, self.point_num, self.init_mode)

    def calFitnessValue(self, position: list) -> float:
        """100000 / (length + 50000 obs_cost) of the curve through [start] + position + [goal], inf where the
        curve raises (pso.py:186-212): one launch of one particle."""
        out = self._launch([position], np.zeros(0), 1, 0)
        return float(out["fitness"][0, 0])

    def run(self):
        """Reference: plan(verbose=True) and its animation.  Animation is out of scope; returns plan()'s result."""
        return self.plan(verbose=True)

    def isCollision(self, p1: tuple, p2: tuple) -> bool:
        """True where p1 or p2 is an obstacle or out of range, or the class's Bresenham walk from p1 to p2 meets
        an obstacle (pso.py:295-356).  Runs on the host, on the obstacle set."""
        if p1 in self.obstacles or p2 in self.obstacles:
            return True
        (x1, y1), (x2, y2) = p1, p2
        W, H = self.env.x_range, self.env.y_range
        if not (0 <= x1 < W and 0 <= y1 < H and 0 <= x2 < W and 0 <= y2 < H):
            return True
        d_x, d_y = abs(x2 - x1), abs(y2 - y1)
        s_x = 0 if x2 == x1 else (x2 - x1) / d_x
        s_y = 0 if y2 == y1 else (y2 - y1) / d_y
        x, y, e = x1, y1, 0
        x_major = d_x > d_y
        d_u, d_v = (d_x, d_y) if x_major else (d_y, d_x)  # along the walk's own axis, across it
        tau = (d_v - d_u) / 2
        while not (x == x2 if x_major else y == y2):
            along, across = e > tau, e < tau  # neither: a diagonal step
            if not across:
                x, y = (x + s_x, y) if x_major else (x, y + s_y)
            if not along:
                x, y = (x, y + s_y) if x_major else (x + s_x, y)
            e = e + (0 if across else -d_v) + (0 if along else d_u)
            if (x, y) in self.obstacles:
                return True
        return False


def aco_max_steps(x_range: int, y_range: int) -> float:
    """ACO's step cap (aco.py:86), a float: an ant makes choices while steps < it."""
    return x_range * y_range / 2 + max(x_range, y_range)


def _aco_table(planner, goal: Node, beta: float) -> np.ndarray:
    """[W * H] f64, cell x * H + y: (1.0 / h(cell, goal)) ** beta by the planner's own h() and CPython's own **
    for every free cell but the goal (aco.py:118); 0.0 for the goal and the obstacles, which enter no sum."""
    W, H = planner.env.x_range, planner.env.y_range
    obs = planner.obstacles
    tab = np.zeros(W * H, np.float64)
    for x in range(W):
        for y in range(H):
            if (x, y) in obs or (x, y) == goal.current:
                continue
            tab[x * H + y] = (1.0 / planner.h(Node((x, y), (x, y), 0, 0), goal)) ** beta
    return tab


def _aco_check(env: Grid, alpha: float) -> None:
    """What ACO.plan() refuses before anything touches the device"""
    if alpha not in (0.0, 1.0):
        raise NotImplementedError("ACO on the device takes alpha 0.0 or 1.0 only: pheromone ** alpha is then the "
                                  "pheromone or 1.0 bit for bit, and there is no bit-reproducible device pow")
    W, H = env.x_range, env.y_range
    obs = env.obstacles
    if any((x, y) not in obs for x in range(W) for y in (0, H - 1)) or \
            any((x, y) not in obs for y in range(H) for x in (0, W - 1)):
        raise ValueError("ACO needs every border cell of the grid to be an obstacle: from a free one the reference's "
                         "ant steps outside the grid and dies with KeyError one step later")


class ACO(EvolutionarySearcher):
    """Ant Colony Optimization(ACO) motion planning (aco.py:14-186); the colony runs on the device, one wave per
    plan, with the random.random() draws made in the kernel from the global generator's state.

    Parameters:
        start (tuple), goal (tuple), env (Grid), heuristic_type (str): as EvolutionarySearcher
        n_ants (int): number of ants
        alpha (float), beta (float): pheromone and heuristic factor weight coefficients.  plan() takes alpha 0.0
            or 1.0 (NotImplementedError otherwise); beta goes into a table built on the host
        rho (float): evaporation coefficient
        Q (float): pheromone gain
        max_iter (int): maximum iterations

    Grids of more than 65,536 cells and grids with a free border cell are refused.
    """

    def __init__(self, start: tuple, goal: tuple, env: Grid, heuristic_type: str = "euclidean",
                 n_ants: int = 50, alpha: float = 1.0, beta: float = 5.0, rho: float = 0.1, Q: float = 1.0,
                 max_iter: int = 100) -> None:
        super().__init__(start, goal, env, heuristic_type)
        self.n_ants = n_ants
        self.alpha = alpha
        self.beta = beta
        self.rho = rho
        self.Q = Q
        self.max_iter = max_iter
        self.draws = None  # after plan(): the random.random() calls it made

    def __str__(self) -> str:
        return "Ant Colony Optimization(ACO)"

    class Ant:
        def __init__(self) -> None:
            self.reset()

        def reset(self) -> None:
            self.found_goal = False
            self.current_node = None
            self.path = []
            self.path_set = set()
            self.steps = 0

    def heuristic_table(self) -> np.ndarray:
        """(1.0 / h(cell, goal)) ** beta per cell x * y_range + y, as plan() hands it to the kernel.  Python's own
        OverflowError propagates where beta makes a cell overflow (the reference raises only when an ant gets
        there)."""
        return _aco_table(self, self.goal, self.beta)

    def plan(self) -> tuple:
        """(cost, path [(x, y), ...], cost_list) or ([], [], []) where no ant found the goal (aco.py:65-166): one
        launch.  The global `random` ends where the reference's draws would leave it; IndexError where the
        reference's roulette raises it."""
        _aco_check(self.env, self.alpha)
        table = self.heuristic_table()
        version, _, gauss_next = state = random.getstate()
        out = batch.aco_batch(self.env, [self.start.current], [self.goal.current], table[None], [0], [state],
                              self.n_ants, self.max_iter, self.alpha, 1 - self.rho, self.Q)
        status, n, n_cost = int(out["status"][0]), int(out["best_len"][0]), int(out["n_cost"][0])
        words = out["mt_state_out"][0].cpu().numpy().view(np.uint32)
        random.setstate((version, tuple(int(w) for w in words), gauss_next))
        self.draws = int(out["draws"][0])
        if status == STATUS_REF_INDEX_ERROR:
            raise IndexError("list index out of range")
        if status != 0:
            return [], [], []
        H = self.env.y_range
        cells = out["best_path"][0, :n].cpu().numpy()
        nodes = [Node((int(c) // H, int(c) % H)) for c in cells]
        cost = 0
        path = [self.start.current]
        for i in range(len(nodes) - 1):
            cost += self.dist(nodes[i], nodes[i + 1])
            path.append(nodes[i + 1].current)
        return cost, path, [int(v) for v in out["cost_list"][0, :n_cost].cpu().numpy()]

    @staticmethod
    def plan_batch(env: Grid, starts, goals, seeds_or_states, heuristic_type: str = "euclidean", n_ants: int = 50,
                   alpha: float = 1.0, beta: float = 5.0, rho: float = 0.1, Q: float = 1.0, max_iter: int = 100, **kw):
        """Independent plans on one Grid in one launch.  seeds_or_states: per plan an int (random.seed's) or a
        random.getstate() tuple; each plan draws from a generator of its own, as ACO(...).plan() does after
        random.seed(seed).  Plans with the same goal share one heuristic table.  Returns batch.aco_batch's
        device-tensor dict with heur_of (numpy [nq], each plan's table) and random_states (each generator's
        state after its plan; reads the states back) added."""
        _aco_check(env, alpha)
        probe = ACO((0, 0), (0, 0), env, heuristic_type)
        states, tables, index, heur_of = [], [], {}, []
        for g, seed in zip(goals, seeds_or_states):
            states.append(seed if isinstance(seed, tuple) else random.Random(seed).getstate())
            g = tuple(int(v) for v in g)
            if g not in index:
                index[g] = len(tables)
                tables.append(_aco_table(probe, Node(g, g, 0, 0), beta))
            heur_of.append(index[g])
        out = batch.aco_batch(env, np.asarray(starts, np.int32), np.asarray(goals, np.int32),
                              np.asarray(tables, np.float64).reshape(len(tables), -1), np.asarray(heur_of, np.int32),
                              states, n_ants, max_iter, alpha, 1 - rho, Q, **kw)
        words = out["mt_state_out"].cpu().numpy().view(np.uint32)
        out["heur_of"] = np.asarray(heur_of, np.int32)
        out["random_states"] = [(st[0], tuple(int(w) for w in row), st[2]) for st, row in zip(states, words)]
        return out

    def getNeighbor(self, node: Node) -> list:
        """The neighbours of node the class's isCollision lets it move to, in motion order (aco.py:168-179); on
        the host."""
        return [node + motion for motion in self.motions if not self.isCollision(node, node + motion)]

    def run(self):
        """Reference: plan() and its animation.  Animation is out of scope; returns plan()'s result."""
        return self.plan()

