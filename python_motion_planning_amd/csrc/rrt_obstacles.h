// Obstacle primitives of SampleSearcher.isCollision (global_planner/sample_search/sample_search.py:51-135)
// shared by the sample-search kernels (rrt.hip, rrt_connect.hip): same operation order as the oracle.
#pragma once
#include "localplan.h"

namespace {

// ---- obstacle tests (sample_search.py), same operation order as the oracle ----
__device__ inline bool in_box(const double* r, double d, double x, double y)
{
    const double px = x - (r[0] - d), py = y - (r[1] - d);
    return 0 <= px && px <= r[2] + 2 * d && 0 <= py && py <= r[3] + 2 * d;
}

__device__ inline double cross3(double p1x, double p1y, double p2x, double p2y, double p3x, double p3y)
{
    const double x1 = p2x - p1x, y1 = p2y - p1y, x2 = p3x - p1x, y2 = p3y - p1y;
    return x1 * y2 - x2 * y1;
}

__device__ bool inter_rect(const double* r, double d, double x1, double y1, double x2, double y2)
{
    const double vx[4] = {r[0] - d, r[0] + r[2] + d, r[0] + r[2] + d, r[0] - d};
    const double vy[4] = {r[1] - d, r[1] - d, r[1] + r[3] + d, r[1] + r[3] + d};
    for (int a = 0; a < 4; a++)
        for (int b = a + 1; b < 4; b++) {
            if (fmax(x1, x2) >= fmin(vx[a], vx[b]) && fmin(x1, x2) <= fmax(vx[a], vx[b]) &&
                fmax(y1, y2) >= fmin(vy[a], vy[b]) && fmin(y1, y2) <= fmax(vy[a], vy[b])) {
                if (cross3(vx[a], vy[a], vx[b], vy[b], x1, y1) * cross3(vx[a], vy[a], vx[b], vy[b], x2, y2) <= 0 &&
                    cross3(x1, y1, x2, y2, vx[a], vy[a]) * cross3(x1, y1, x2, y2, vx[b], vy[b]) <= 0)
                    return true;
            }
        }
    return false;
}

// np.dot of 2-vectors = OpenBLAS ddot: fma(a1, b1, a0 * b0)
__device__ bool inter_circle(const double* c, double d, double x, double y, double x2, double y2)
{
    const double dx = x2 - x, dy = y2 - y;
    const double d2 = fma(dy, dy, dx * dx);
    if (d2 == 0) return false;
    const double t = fma(c[1] - y, dy, (c[0] - x) * dx) / d2;
    if (0 <= t && t <= 1) {
        const double sx = x + t * dx, sy = y + t * dy;
        if (lp::py_hypot(c[0] - sx, c[1] - sy) <= c[2] + d) return true;
    }
    return false;
}

}  // namespace
