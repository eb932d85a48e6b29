"""How does numpy round the 3x3 @ 3 product of generateRandomNode (informed_rrt.py:146)?

Builds T exactly as Ellipse.transform does, multiplies it with p = (x, y, 1) for points of the unit
disk, and counts how many outputs each candidate operation order reproduces bit for bit.  fma is
evaluated exactly with fractions.Fraction and rounded once.  CPU only:

    python tools/informed_matvec_probe.py [n]

rrt.hip's ellipse sampler uses the order that matches every output: fma(t0, x, t1 * y) + t2.
"""
import sys
from fractions import Fraction

import numpy as np


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def main(n):
    rng = np.random.default_rng(1)
    forms = {
        "fma(t0,x,t1*y)+t2": lambda t0, t1, t2, x, y: fma(t0, x, t1 * y) + t2,
        "(t0*x+t1*y)+t2": lambda t0, t1, t2, x, y: (t0 * x + t1 * y) + t2,
        "fma(t1,y,t0*x)+t2": lambda t0, t1, t2, x, y: fma(t1, y, t0 * x) + t2,
        "fma(t0,x,fma(t1,y,t2))": lambda t0, t1, t2, x, y: fma(t0, x, fma(t1, y, t2)),
        "fma(t1,y,fma(t0,x,t2))": lambda t0, t1, t2, x, y: fma(t1, y, fma(t0, x, t2)),
        "t0*x+(t1*y+t2)": lambda t0, t1, t2, x, y: t0 * x + (t1 * y + t2),
    }
    hits = dict.fromkeys(forms, 0)
    total = 0
    while total < n:
        p1, p2 = rng.uniform(0, 500, 2), rng.uniform(0, 500, 2)
        c = float(np.hypot(*(p2 - p1))) / 2
        a = c * float(rng.uniform(1.0, 3.0))
        theta = -np.arctan2(p2[1] - p1[1], p2[0] - p1[0])
        b = np.sqrt(a ** 2 - c ** 2)
        T = np.array([[a * np.cos(theta), b * np.sin(theta), (p1[0] + p2[0]) / 2],
                      [-a * np.sin(theta), b * np.cos(theta), (p1[1] + p2[1]) / 2], [0, 0, 1]])
        for _ in range(50):
            x, y = rng.uniform(-1, 1), rng.uniform(-1, 1)
            if x ** 2 + y ** 2 >= 1:
                continue
            p = np.array([.0, .0, 1.])
            p[0], p[1] = x, y
            out = T @ p.T
            for row in (0, 1):
                t0, t1, t2 = (float(v) for v in T[row])
                for name, f in forms.items():
                    hits[name] += f(t0, t1, t2, float(x), float(y)) == out[row]
                total += 1
    for name, h in hits.items():
        print(f"{name:28s} {h}/{total}")
    return hits, total


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20000)
