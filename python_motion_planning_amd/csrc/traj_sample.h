// What the trajectory kernels (totp3d.hip, polytraj3d.hip, splinetraj3d.hip) share.  One wave64 per path, 64
// points per round:
//  - the waypoints of a path into LDS, from the f64 list or decoded from the cell ids a 3D grid planner
//    left on the device, and the write that refuses a path;
//  - the sampling loop's round: generate() / resample() step t = 0, dt, ... by repeated addition and append
//    total_time when the last step falls short of it (time_optimal_trajectory.py:260-302,
//    polynomial_trajectory.py:238-246, trajectory_base.py:193-216); the rows that fit the buffer go
//    from an LDS stage to HBM as one contiguous run;
//  - the yaw / yaw-rate tail: compute_yaw_from_velocity (trajectory_base.py:245-261) sets yaw where the
//    planar speed exceeds 1e-6 and the yaw rate where both neighbouring yaws exist;
//  - scipy's interp1d interval search.
#pragma once
#include "pmp_internal.h"

// The waypoint count of path q (path_len[q] in the cells form, else off[q + 1] - off[q]) and wp_cap, the
// most a path of this launch may have: what the LDS block holds and, in the cells form, what a row holds.
__device__ __forceinline__ int traj_waypoint_count(int q, const int32_t* __restrict__ off,
                                                   const int32_t* __restrict__ cells,
                                                   const int32_t* __restrict__ path_len, int path_cap, int nmax,
                                                   int& wp_cap)
{
    wp_cap = cells && path_cap < nmax ? path_cap : nmax;
    return cells ? path_len[q] : off[q + 1] - off[q];
}

// All lanes: the n waypoints of path q into P [3][nmax] (SoA), cell v = (x * Y + y) * Z + z decoded.
__device__ __forceinline__ void traj_load_waypoints(double* P, int nmax, int n, int q, int lane,
                                                    const double* __restrict__ path, const int32_t* __restrict__ off,
                                                    const int32_t* __restrict__ cells, int path_cap, int Y, int Z)
{
    for (int i = lane; i < n; i += 64) {
        if (cells) {
            const int v = cells[(size_t)q * path_cap + i];
            P[i] = (double)(v / (Y * Z));
            P[nmax + i] = (double)((v / Z) % Y);
            P[2 * nmax + i] = (double)(v % Z);
        } else {
            const double* w = path + 3 * ((size_t)off[q] + i);
            P[i] = w[0];
            P[nmax + i] = w[1];
            P[2 * nmax + i] = w[2];
        }
    }
}

// A path the kernel does not run: its status, no points, no time.
__device__ __forceinline__ void traj_refuse(int lane, int q, int status, int32_t* __restrict__ st_out,
                                            int32_t* __restrict__ np_out, double* __restrict__ total_out)
{
    if (lane == 0) {
        st_out[q] = status;
        np_out[q] = 0;
        total_out[q] = 0.0;
    }
}

// Lane 0 only: the next (up to 64) query times into tq, meta[0] = how many, meta[1] = bit 0: last round,
// bit 1: this round's last time is the total_time the reference appends after its loop.
// eval_t: these times instead (count = how many were taken in earlier rounds).  t / last_t carry the
// reference's accumulated time (`t += dt`; k * dt rounds differently) across rounds.
__device__ __forceinline__ void traj_next_times(const double* __restrict__ eval_t, int n_eval, int count, double dt,
                                                double total, double& t, double& last_t, double* tq, int* meta)
{
    int k = 0;
    bool fin = false, appended = false;
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
                    appended = true;
                }
                fin = true;
                break;
            }
        }
    }
    meta[0] = k;
    meta[1] = (fin ? 1 : 0) | (appended ? 2 : 0);
}

// One round of the sampling loop (wave-uniform)
struct traj_round {
    int k;          // query times in tq
    int nrow;       // of those, the rows that fit the point buffer: clamp(point_cap - count, 0, k)
    bool done;      // the last round
    bool appended;  // tq[k - 1] is the appended total_time
};

// All lanes (a barrier inside): lane 0 fills tq with the round's times, everyone reads what it left in meta.
__device__ __forceinline__ traj_round traj_round_head(int lane, const double* __restrict__ eval_t, int n_eval, int count,
                                                      double dt, double total, double& t, double& last_t, double* tq,
                                                      int* meta, int point_cap)
{
    if (lane == 0) traj_next_times(eval_t, n_eval, count, dt, total, t, last_t, tq, meta);
    __syncthreads();
    traj_round r;
    r.k = meta[0];
    r.done = (meta[1] & 1) != 0;
    r.appended = (meta[1] & 2) != 0;
    const int room = point_cap - count;
    r.nrow = room < 0 ? 0 : (room < r.k ? room : r.k);
    return r;
}

// All lanes: the round's nrow staged rows (kRow doubles each) to rows count.. of pts as one contiguous run
// (64 x 8 B per instruction)
template <int kRow>
__device__ __forceinline__ void traj_store_rows(double* __restrict__ pts, const double* stage, int count, int nrow, int lane)
{
    for (int j = lane; j < nrow * kRow; j += 64) pts[(size_t)count * kRow + j] = stage[j];
}

// The upper index of x's interval in xs [ns], ascending, as interp1d(kind='linear',
// fill_value='extrapolate') finds it (scipy _call_linear): searchsorted (left), clipped to [1, ns - 1]
__device__ __forceinline__ int traj_interp_upper(const double* xs, int ns, double x)
{
    int lo = 0, hi = ns;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (xs[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < 1 ? 1 : (lo > ns - 1 ? ns - 1 : lo);
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
