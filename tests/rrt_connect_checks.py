"""RRT-Connect: a sequential restatement of the arithmetic rrt_connect.hip uses, and the fixture of
reference runs (tests/golden/rrt_connect.npz, made by make_golden_rrt_connect.py).

plan() below is the reference's loop (rrt_connect.py:42-147 over rrt.py:92-130, sample_search.py:27-135)
written over flat lists with the kernel's conventions: tree 0 rooted at the start and tree 1 at the
goal, nodes in dict order with parents as indices into their own tree, `forward` naming the tree that
is sample_list_f, draws read from a given stream, every loop bounded by the tree capacity, and the
kernel's operation order wherever rounding depends on it (informed_rrt_checks' collision tests).  On
the CPU, where atan2 / cos / sin are the reference's own libm, it reproduces the fixture bit for bit
(test_rrt_connect_fixture.py); the kernel is held to the same runs (test_rrt_connect_gpu.py).
"""
from __future__ import annotations

import math

import numpy as np

from golden_io import load_npz
from informed_rrt_checks import MapTests, env_of, map_of  # noqa: F401

FIXTURE = "rrt_connect.npz"
FOUND, NO_PATH, PATH_OVERFLOW, CAP_OVERFLOW, REF_RAISES = range(5)


class _Overflow(Exception):
    pass


def plan(kind, start, goal, rnd, sample_num, max_dist=0.5, delta=0.5, rate=0.05, cap=None, path_cap=None):
    """-> dict(status, tree [2] of (x, y, g, parent) lists, forward, boundary, cost, path (start first),
    iters, draws, collision_tests)."""
    rects, circs, X, Y = map_of(kind)
    M = MapTests(rects, circs, X, Y, delta)
    sx0, sy0, gx, gy = float(start[0]), float(start[1]), float(goal[0]), float(goal[1])
    T = [([sx0], [sy0], [0.0], [0]), ([gx], [gy], [0.0], [0])]
    lox, rgx = delta, (X - delta) - delta
    loy, rgy = delta, (Y - delta) - delta
    cap = 10 ** 9 if cap is None else cap
    fw, cur, iters, status = 0, 0, 0, NO_PATH
    boundary, cost, path = [-1, -1], 0.0, None

    def append(t, x, y, g, parent):
        xs, ys, gs, par = T[t]
        if len(xs) >= cap:
            raise _Overflow()
        xs.append(x); ys.append(y); gs.append(g); par.append(parent)
        return len(xs) - 1

    def extend(t, px, py):
        """getNearest (rrt.py:105-130) of tree t towards (px, py) and the insert: the slot, or -1."""
        xs, ys, gs, par = T[t]
        dist = [math.hypot(xs[j] - px, ys[j] - py) for j in range(len(xs))]
        near = dist.index(min(dist))
        ex, ey = xs[near], ys[near]
        d0 = math.hypot(px - ex, py - ey)
        theta = math.atan2(py - ey, px - ex)
        d = d0 if d0 < max_dist else max_dist
        nx, ny = ex + d * math.cos(theta), ey + d * math.sin(theta)
        G = gs[near] + d
        if M.collision(nx, ny, ex, ey):
            return -1
        if d0 == 0.0:
            # the same key: the dict entry is replaced in place, its parent its own coordinates
            xs[near], ys[near], gs[near], par[near] = nx, ny, G, near
            return near
        return append(t, nx, ny, G, near)

    try:
        for _ in range(sample_num):
            if cur + 3 > len(rnd):
                status = CAP_OVERFLOW
                break
            iters += 1
            sx, sy = gx, gy
            cur += 1
            if rnd[cur - 1] > rate:
                sx = lox + rgx * rnd[cur]
                sy = loy + rgy * rnd[cur + 1]
                cur += 2
            bw = 1 - fw
            slot = extend(fw, sx, sy)
            if slot >= 0:
                nx, ny = T[fw][0][slot], T[fw][1][slot]
                bs = extend(bw, nx, ny)
                if bs >= 0:
                    xs, ys, gs, par = T[bw]
                    while True:
                        bx, by = xs[bs], ys[bs]
                        if bx == nx and by == ny:
                            status = FOUND
                            boundary[fw], boundary[bw] = slot, bs
                            break
                        d = math.hypot(bx - nx, by - ny)
                        d = d if d < max_dist else max_dist
                        theta = math.atan2(ny - by, nx - bx)
                        b2x, b2y = bx + d * math.cos(theta), by + d * math.sin(theta)
                        if M.collision(b2x, b2y, bx, by):
                            break
                        bs = append(bw, b2x, b2y, gs[bs] + d, bs)
                    if status == FOUND:
                        break
            if len(T[bw][0]) < len(T[fw][0]):
                fw = bw
    except _Overflow:
        status = CAP_OVERFLOW
    if status == FOUND:
        cost = T[0][2][boundary[0]] + T[1][2][boundary[1]]
        walks = []
        for t in (0, 1):
            xs, ys, gs, par = T[t]
            v, walk, reached = boundary[t], [], False
            for _s in range(len(xs) + 1):
                walk.append((xs[v], ys[v]))
                if v == 0:
                    reached = True
                    break
                v = par[v]
            if not reached:
                status = REF_RAISES
            walks.append(walk)
        if status == FOUND:
            path = walks[0][::-1] + walks[1][1:]
            if path_cap is not None and len(path) > path_cap:
                status = PATH_OVERFLOW
    return dict(status=status, tree=T, forward=fw, boundary=boundary, cost=cost, path=path, iters=iters, draws=cur,
                collision_tests=M.calls)


# ---- the fixture ---------------------------------------------------------------------------------------
def cases():
    """The fixture's cases as dicts (kind, map, seed, sample_num, start, goal, max_dist, rate, tree0 /
    tree1 [n,3], parent0 / parent1, forward, boundary, cost, found, path, n_expand, iters, coll, draws,
    next)."""
    z = load_npz(FIXTURE)
    out = []
    for i in range(int(z["n_cases"])):
        c = {k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")}
        for k in ("seed", "sample_num", "forward", "iters", "coll", "draws", "n_expand"):
            c[k] = int(c[k])
        for k in ("max_dist", "rate", "cost", "next"):
            c[k] = float(c[k])
        c["kind"], c["map"], c["found"] = str(c["kind"]), str(c["map"]), bool(c["found"])
        out.append(c)
    return out, z


def stream(case, n=None):
    """np.random.seed(case seed)'s doubles: 3 * sample_num + 1 of them unless n is given."""
    return np.random.RandomState(case["seed"]).random_sample(3 * case["sample_num"] + 1 if n is None else n)
