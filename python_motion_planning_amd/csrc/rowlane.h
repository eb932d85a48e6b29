// Row-per-agent helpers shared by the local-planner kernels that keep four agents per wave64, one
// per 16-lane DPP row (track.hip, follow.hip): DPP moves inside a row, the row reductions and
// getLookaheadPoint on a row.
//
// Cross-lane traffic stays inside a row: row_newbcast:k broadcasts lane k of each row, row_shr /
// row_shl shift within the row (bound_ctrl: a lane with no source reads 0), row_ror rotates.  f64
// values move as two 32-bit DPP halves.
#pragma once
#include "localplan.h"

namespace {

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x)
{
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true); }

// getLookaheadPoint (local_planner.py:103-170) for the row's agent: the distance scan, the
// first-index argmin and the first-beyond-lookahead search over the row's 16 lanes (stride 16), the
// tail on every lane of the row (same inputs, same result).  Called with the whole row active.
__device__ __forceinline__ void row_best_min(double& v, int& i)
{
    // (v, i) minimum with ties to the lowest i, over the row (rotations)
#define PMP_ROW_STEP(CTRL)                                                        \
    {                                                                             \
        const double ov = dpp_f64<CTRL>(v);                                       \
        const int oi = dpp_i32<CTRL>(i);                                          \
        if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }                    \
    }
    PMP_ROW_STEP(0x128) PMP_ROW_STEP(0x124) PMP_ROW_STEP(0x122) PMP_ROW_STEP(0x121)
#undef PMP_ROW_STEP
}
__device__ inline int lookahead_row(const double* path, int P, double rx, double ry, double v, const pmp_lp_params& Pm,
                                    double* pt, double* theta, double* kappa)
{
    const int r = lane_id() & 15;
    const double L = lp::lookahead_dist(v, Pm);
    // idx_closest = dist_to_robot.index(min(dist_to_robot))
    double bd = INFINITY;
    int bi = 0x7fffffff;
#pragma unroll 1
    for (int i = r; i < P; i += 16) {
        const double d = lp::py_hypot(rx - path[2 * i], ry - path[2 * i + 1]);
        if (d < bd) { bd = d; bi = i; }  // strided in increasing i: keeps the first minimum
    }
    row_best_min(bd, bi);
    const int idx_closest = bi;
    // first i >= idx_closest with dist >= L
    int fi = 0x7fffffff;
#pragma unroll 1
    for (int i = idx_closest + r; i < P; i += 16) {
        if (lp::py_hypot(rx - path[2 * i], ry - path[2 * i + 1]) >= L) { fi = i; break; }
    }
    double fd = 0.0;
    row_best_min(fd, fi);
    const int idx_goal = fi == 0x7fffffff ? P - 1 : fi;
    return lp::lookahead_tail(path, P, rx, ry, L, idx_goal, pt, theta, kappa);
}

// min / sum over the row, in every lane of the row (rotations: every lane combines the same pairs,
// so the sum's bits are the same in all 16 lanes)
__device__ __forceinline__ double min16(double t)
{
    t = fmin(t, dpp_f64<0x128>(t));  // row_ror:8
    t = fmin(t, dpp_f64<0x124>(t));
    t = fmin(t, dpp_f64<0x122>(t));
    t = fmin(t, dpp_f64<0x121>(t));
    return t;
}
__device__ __forceinline__ double sum16(double t)
{
    t += dpp_f64<0x128>(t);
    t += dpp_f64<0x124>(t);
    t += dpp_f64<0x122>(t);
    t += dpp_f64<0x121>(t);
    return t;
}

}  // namespace
