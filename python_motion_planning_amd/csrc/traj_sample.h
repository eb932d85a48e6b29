// The sampling loop's time stepping and the yaw / yaw-rate tail shared by the trajectory kernels
// (totp3d.hip, polytraj3d.hip, splinetraj3d.hip): generate() / resample() step t = 0, dt, ... by repeated addition and
// append total_time when the last step falls short of it (time_optimal_trajectory.py:260-302,
// polynomial_trajectory.py:238-246, trajectory_base.py:193-216); compute_yaw_from_velocity
// (trajectory_base.py:245-261) sets yaw where the planar speed exceeds 1e-6 and the yaw rate where
// both neighbouring yaws exist.  One wave64 per path, 64 points per round.
#pragma once
#include "pmp_internal.h"

// Lane 0 only: the next (up to 64) query times into tq, meta[0] = how many, meta[1] = last round.
// eval_t: these times instead (count = how many were taken in earlier rounds).  t / last_t carry the
// reference's accumulated time (`t += dt`; k * dt rounds differently) across rounds.  appended (nullable):
// set to whether this round's last time is the total_time the reference appends after its loop.
__device__ __forceinline__ void traj_next_times(const double* __restrict__ eval_t, int n_eval, int count, double dt,
                                                double total, double& t, double& last_t, double* tq, int* meta,
                                                bool* appended = nullptr)
{
    if (appended) *appended = false;
    int k = 0;
    bool fin = false;
    if (eval_t) {
        for (; k < 64 && count + k < n_eval; k++) tq[k] = eval_t[count + k];
        fin = count + k >= n_eval;
    } else {
        while (k < 64) {
            if (t <= total) {
                tq[k++] = t;
                last_t = t;
                t += dt;
            } else {
                if (count + k > 0 && last_t < total) {
                    tq[k++] = total;
                    last_t = total;
                    if (appended) *appended = true;
                }
                fin = true;
                break;
            }
        }
    }
    meta[0] = k;
    meta[1] = fin ? 1 : 0;
}

// The previous round's last point (wave-uniform)
struct traj_prev {
    double t = 0.0, yaw = 0.0;
    bool has = false, yaw_ok = false;
};

// All lanes (shuffles inside): lane < k holds a point at time my_t with planar velocity (vx, vy);
// yaw_col / rate_col get its yaw and yaw rate, NaN where the reference leaves None (always when
// !with_yaw: evaluate() sets neither).  pv is advanced to this round's last point.
__device__ __forceinline__ void traj_yaw_tail(int lane, int k, bool with_yaw, double vx, double vy, double my_t,
                                              traj_prev& pv, double& yaw_col, double& rate_col)
{
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const bool valid = lane < k;
    if (!valid) my_t = 0.0;
    const bool has = valid && with_yaw && __dsqrt_rn(vx * vx + vy * vy) > 1e-6;
    const double yaw = has ? atan2(vy, vx) : 0.0;
    yaw_col = has ? yaw : nan;
    // the previous point: lane - 1, or the previous round's last point
    const double pt = __shfl_up(my_t, 1), py = __shfl_up(yaw, 1);
    const bool ph = __shfl_up(has ? 1 : 0, 1) != 0;
    double rate = nan;
    if (valid) {
        const double qt = lane == 0 ? pv.t : pt, qy = lane == 0 ? pv.yaw : py;
        const bool qh = lane == 0 ? (pv.has && pv.yaw_ok) : ph;
        const double dtp = my_t - qt;
        if (qh && has && dtp > 0) {
            double dy = yaw - qy;
            while (dy > M_PI) dy -= 2.0 * M_PI;
            while (dy < -M_PI) dy += 2.0 * M_PI;
            rate = dy / dtp;
        }
    }
    rate_col = rate;
    if (k > 0) {
        pv.t = rl_f64(my_t, k - 1);
        pv.yaw = rl_f64(yaw, k - 1);
        pv.yaw_ok = rl_u32(has ? 1u : 0u, k - 1) != 0;
        pv.has = true;
    }
}
