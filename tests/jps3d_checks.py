"""Host-side checks shared by the JPS3D tests (tests/golden/jps3d_runs.npz, make_golden_jps3d.py)."""
import math

import numpy as np

from golden_io import load_npz, seg

FIXTURE = "jps3d_runs.npz"


def cases():
    """List of dicts, one per fixture case: occ [X, Y, Z] uint8, start, goal, heuristic name, cost, path,
    closed, closed_parent, closed_g (cells (x*Y + y)*Z + z), expansions."""
    z = load_npz(FIXTURE)
    out = []
    for i in range(len(z["dims"])):
        shape = tuple(int(v) for v in z["dims"][i])
        n = int(np.prod(shape))
        occ = np.unpackbits(seg(z["occ_bits"], z["occ_off"], i))[:n].reshape(shape).astype(np.uint8)
        a, b = int(z["closed_off"][i]), int(z["closed_off"][i + 1])
        out.append(dict(i=i, occ=occ, start=z["start"][i], goal=z["goal"][i],
                        heuristic="manhattan" if z["heuristic"][i] else "euclidean", cost=float(z["cost"][i]),
                        path=seg(z["path"], z["path_off"], i), closed=z["closed"][a:b],
                        closed_parent=z["closed_parent"][a:b], closed_g=z["closed_g"][a:b],
                        expansions=int(z["expansions"][i])))
    return out


def decode(c, dims):
    _, Y, Z = dims
    c = int(c)
    return (c // (Y * Z), (c // Z) % Y, c % Z)


def step_collides(occ, p, d):
    """GraphSearcher3D.isCollision (graph_search_3d.py:66-107) for the unit step p -> p + d inside the
    grid, plus jump()'s bounds test: either end occupied or outside, or an occupied corner cell."""
    q = tuple(p[k] + d[k] for k in range(3))
    if any(not 0 <= q[k] < occ.shape[k] for k in range(3)) or occ[p] or occ[q]:
        return True
    if sum(v != 0 for v in d) < 2:
        return False
    for k in range(3):
        if d[k]:
            c = list(p)
            c[k] += d[k]
            if occ[tuple(c)]:
                return True
    return False


def path_cost(occ, path):
    """Validate a jump-point path (cells) on `occ` and return extractPath's cost (jps3d.py:248-261):
    every segment a straight run along one of the 26 directions whose unit steps do not collide, the
    cost summed goal -> start with math.sqrt of the integer square distance."""
    pts = [decode(c, occ.shape) for c in path]
    for a, b in zip(pts[:-1], pts[1:]):
        delta = [b[k] - a[k] for k in range(3)]
        n = max(abs(v) for v in delta)
        assert n > 0 and all(abs(v) in (0, n) for v in delta), (a, b)
        d = tuple(v // n for v in delta)
        p = a
        for _ in range(n):
            assert not step_collides(occ, p, d), (a, b, p)
            p = tuple(p[k] + d[k] for k in range(3))
    cost = 0.0
    for a, b in zip(pts[:0:-1], pts[-2::-1]):
        cost += math.sqrt(sum((a[k] - b[k]) ** 2 for k in range(3)))
    return cost
