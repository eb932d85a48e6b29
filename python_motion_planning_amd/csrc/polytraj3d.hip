// Batched PolynomialTrajectory3D.generate() / evaluate() / resample() for gfx950
// (trajectory/polynomial_trajectory.py:52-286, trajectory_base.py:193-216, :245-261): the `polynomial`
// choice after 3D planning (examples/3d_example.py:100-133).
//
// One wave64 per path:
//  1. waypoints into LDS (from the f64 list, or decoded from the cell ids a 3D grid planner left on the
//     device), segment times lane-parallel, their running sum (= the segments' start and end times and
//     total_time, the reference's left-to-right additions) on lane 0, waypoint velocities lane-parallel;
//  2. lane 0 steps t = 0, dt, ... (the reference's repeated sum), the lanes evaluate 64 points at a
//     time: binary search of the segment, its quintic coefficients recomputed from the waypoints (six
//     divisions a point instead of an [nseg][3][6] table), the four 6-term products, yaw and yaw rate
//     from the neighbouring lane;
//  3. the 64 rows go through an LDS stage so that the wave stores them as one contiguous run
//     (64 x 8 B per instruction) instead of 15 doubles at a 120-B stride per lane.
// Values follow the reference's operation order (CPython / numpy float64, -ffp-contract=off).  The
// reference's `coeffs @ t_vec` is a BLAS dgemv whose six products are summed as
// ((x0 + x2) + (x1 + x3)) + fma(c4, w4, c5 w5) (tests/golden/polytraj.npz pins it: with a plain
// left-to-right sum the last point's velocity, a difference of 1e-6 between terms of 1, moves by
// 1e-10 relative and its yaw rate by more than the 1e-9 bound), and its `t ** k` is libm's pow,
// correctly rounded: here a double-double product chain.
#include "pmp_internal.h"
#include "traj_entry.h"
#include "traj_sample.h"

namespace {

constexpr int kCh = 64;        // points per round (one per lane)
constexpr int kRow = 15;       // doubles per point
constexpr int kMaxWp = 880;    // waypoints whose LDS block (8 n + 1 doubles) fits 64 KiB beside the stage
constexpr double kMaxSteps = 16777216.0;  // total_time / dt beyond this is refused per path (2 GB of points)

__host__ __device__ constexpr size_t lds_doubles(int nmax) { return 8 * (size_t)nmax + 1 + kCh * kRow + kCh + 1; }

// (h, l) <- (h, l) * u in double-double (error-free product by fma); returns the rounded value
__device__ __forceinline__ double dd_mul(double& h, double& l, double u)
{
    const double p = h * u, e = __builtin_fma(h, u, -p), t = __builtin_fma(l, u, e);
    const double s = p + t;
    l = t - (s - p);
    h = s;
    return s;
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void polytraj3d_kernel(pmp_polytraj_params C, int nq, const double* __restrict__ path,
                                                        const int32_t* __restrict__ off, const int32_t* __restrict__ cells,
                                                        const int32_t* __restrict__ path_len, int path_cap, int Y, int Z,
                                                        const double* __restrict__ bc, int nmax, int point_cap,
                                                        double* __restrict__ pts_out, int32_t* __restrict__ np_out,
                                                        double* __restrict__ total_out, double* __restrict__ seg_out,
                                                        int32_t* __restrict__ st_out, const double* __restrict__ eval_t,
                                                        int n_eval, double sample_dt)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int q = blockIdx.x;
    const int lane = lane_id();
    if (q >= nq) return;
    int wp_cap;
    const int n = traj_waypoint_count(q, off, cells, path_len, path_cap, nmax, wp_cap);
    // LDS: P [3][nmax] | V [3][nmax] | T [nmax] | S [nmax + 1] | stage [kCh][kRow] | tq [kCh] | meta
    double* P = sm;
    double* V = P + 3 * (size_t)nmax;
    double* T = V + 3 * (size_t)nmax;
    double* S = T + nmax;
    double* stage = S + nmax + 1;
    double* tq = stage + kCh * kRow;
    int* meta = (int*)(tq + kCh);
    if (n < 2 || n > wp_cap) {  // n < 2: the reference raises ValueError (polynomial_trajectory.py:191)
        traj_refuse(lane, q, n < 2 ? PMP_REF_RAISES : PMP_CAP_OVERFLOW, st_out, np_out, total_out);
        return;
    }
    traj_load_waypoints(P, nmax, n, q, lane, path, off, cells, path_cap, Y, Z);
    double b0[3] = {0, 0, 0}, b1[3] = {0, 0, 0}, b2[3] = {0, 0, 0}, b3[3] = {0, 0, 0};  // v0, v1, a0, a1
    if (bc)
        for (int d = 0; d < 3; d++) {
            b0[d] = bc[12 * (size_t)q + d];
            b1[d] = bc[12 * (size_t)q + 3 + d];
            b2[d] = bc[12 * (size_t)q + 6 + d];
            b3[d] = bc[12 * (size_t)q + 9 + d];
        }
    __syncthreads();
    // _compute_segment_times (:89-111)
    const int nseg = n - 1;
    double* seg = seg_out + (cells ? (size_t)q * path_cap : (size_t)off[q]);
    {
        const double vavg = fmin(fmin(C.max_velocity[0], C.max_velocity[1]), C.max_velocity[2]) * 0.7;
        const double amin = fmin(fmin(C.max_acceleration[0], C.max_acceleration[1]), C.max_acceleration[2]);
        for (int i = lane; i < nseg; i += 64) {
            const double a = P[i + 1] - P[i], b = P[nmax + i + 1] - P[nmax + i], e = P[2 * nmax + i + 1] - P[2 * nmax + i];
            const double dist = __dsqrt_rn((a * a + b * b) + e * e);
            const double est = vavg > 0 ? dist / vavg : 1.0;
            const double mt = 2.0 * __dsqrt_rn(dist / amin);
            double t = est > mt ? est : mt;  // max(est, mt, 0.5)
            t = t > 0.5 ? t : 0.5;
            T[i] = t;
            seg[i] = t;
        }
    }
    __syncthreads();
    // segment i runs from S[i] to S[i] + T[i] = S[i + 1] (:203-232, :266); total_time = sum(segment_times)
    // is the same left-to-right sum
    if (lane == 0) {
        double acc = 0.0;
        S[0] = 0.0;
        for (int i = 0; i < nseg; i++) {
            acc = acc + T[i];
            S[i + 1] = acc;
        }
    }
    // _generate_waypoint_velocities (:162-187)
    for (int i = lane; i < n; i += 64)
        for (int d = 0; d < 3; d++) {
            double v;
            if (i == 0) v = b0[d];
            else if (i == n - 1) v = b1[d];
            else {
                v = (P[d * nmax + i + 1] - P[d * nmax + i - 1]) / (T[i] + T[i - 1]);
                const double hi = C.max_velocity[d], lo = -hi;  // np.clip
                v = v < lo ? lo : v;
                v = v > hi ? hi : v;
            }
            V[d * nmax + i] = v;
        }
    __syncthreads();
    const double total = S[nseg];
    const bool resample = sample_dt > 0.0;
    const double dt = resample ? sample_dt : C.min_time_step;
    if (lane == 0) total_out[q] = total;
    // not finite (the reference never ends or raises), or more steps than any buffer holds
    if (!(total < __longlong_as_double(0x7ff0000000000000ll)) || (!eval_t && !(total / dt < kMaxSteps))) {
        if (lane == 0) {
            st_out[q] = !(total < __longlong_as_double(0x7ff0000000000000ll)) ? PMP_REF_RAISES : PMP_PATH_OVERFLOW;
            np_out[q] = 0;
        }
        return;
    }

    // ---- generate (:234-251) / resample / evaluate (:253-286) + compute_yaw_from_velocity
    double* pts = pts_out + (size_t)q * point_cap * kRow;
    const bool with_yaw = !eval_t && !resample;
    double t = 0.0, last_t = -1.0;  // lane 0: the reference's accumulated t
    int count = 0;
    bool done = false;
    traj_prev pv;
    while (!done) {
        const traj_round r = traj_round_head(lane, eval_t, n_eval, count, dt, total, t, last_t, tq, meta, point_cap);
        done = r.done;
        const int nrow = r.nrow;
        double my_t = 0.0, vx = 0.0, vy = 0.0;
        double* o = stage + lane * kRow;
        if (lane < nrow) {
            const double tc = tq[lane] < 0.0 ? 0.0 : (tq[lane] > total ? total : tq[lane]);
            // the first segment with t <= start + duration (:265-274)
            int lo = 0, hi = nseg;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (tc <= S[mid + 1]) hi = mid;
                else lo = mid + 1;
            }
            const int i = lo < nseg ? lo : nseg - 1;  // lo == nseg (a NaN time only): the last segment's end
            const double Ti = T[i];
            double u = lo < nseg ? tc - S[i] : Ti;
            u = u < 0.0 ? 0.0 : (u > Ti ? Ti : u);
            const double T2 = Ti * Ti, T3 = T2 * Ti, T4 = T3 * Ti, T5 = T4 * Ti;
            // u ** k, correctly rounded (up to the double-double error, 2^-100)
            double ph = u * u, plo = __builtin_fma(u, u, -ph);
            const double u2 = ph, u3 = dd_mul(ph, plo, u), u4 = dd_mul(ph, plo, u), u5 = dd_mul(ph, plo, u);
            o[0] = tc;
#pragma unroll
            for (int d = 0; d < 3; d++) {
                const double p0 = P[d * nmax + i], p1 = P[d * nmax + i + 1], v0 = V[d * nmax + i], v1 = V[d * nmax + i + 1];
                const double a0 = i == 0 ? b2[d] : 0.0, a1 = i == nseg - 1 ? b3[d] : 0.0;
                // _solve_quintic_coefficients (:142-158)
                const double c2 = a0 / 2.0;
                const double c3 = (((20.0 * p1 - 20.0 * p0) - (8.0 * v1 + 12.0 * v0) * Ti) - (3.0 * a0 - a1) * T2) / (2.0 * T3);
                const double c4 = (((30.0 * p0 - 30.0 * p1) + (14.0 * v1 + 16.0 * v0) * Ti) + (3.0 * a0 - 2.0 * a1) * T2) / (2.0 * T4);
                const double c5 = (((12.0 * p1 - 12.0 * p0) - (6.0 * v1 + 6.0 * v0) * Ti) - (a0 - a1) * T2) / (2.0 * T5);
                // PolynomialSegment.evaluate (:25-49) in the reference's BLAS order (products by 0 dropped)
                o[1 + d] = ((p0 + c2 * u2) + (v0 * u + c3 * u3)) + __builtin_fma(c4, u4, c5 * u5);
                o[4 + d] = (c2 * (2.0 * u) + (v0 + c3 * (3.0 * u2))) + __builtin_fma(c4, 4.0 * u3, c5 * (5.0 * u4));
                o[7 + d] = (c2 * 2.0 + c3 * (6.0 * u)) + __builtin_fma(c4, 12.0 * u2, c5 * (20.0 * u3));
                o[10 + d] = c3 * 6.0 + __builtin_fma(c4, 24.0 * u, c5 * (60.0 * u2));
            }
            my_t = tc;
            vx = o[4];
            vy = o[5];
        }
        double yaw_col, rate_col;
        traj_yaw_tail(lane, nrow, with_yaw, vx, vy, my_t, pv, yaw_col, rate_col);
        if (lane < nrow) {
            o[13] = yaw_col;
            o[14] = rate_col;
        }
        __syncthreads();
        traj_store_rows<kRow>(pts, stage, count, nrow, lane);
        count += r.k;
    }
    if (lane == 0) {
        np_out[q] = count;
        st_out[q] = count > point_cap ? PMP_PATH_OVERFLOW : PMP_FOUND;
    }
}

}  // namespace

extern "C" int pmp_polytraj3d_max_waypoints(void) { return kMaxWp; }

extern "C" int pmp_polytraj3d_batch(pmp_ctx* ctx, void* stream, const pmp_polytraj_params* prm, int nq,
                                    const double* path_xyz, const int32_t* path_off, const int32_t* cells,
                                    const int32_t* path_len, int path_cap, int X, int Y, int Z, const double* bc,
                                    int max_waypoints, int point_cap, double* points, int32_t* n_points,
                                    double* total_time, double* segment_times, int32_t* status, const double* eval_t,
                                    int n_eval, double sample_dt)
{
    const char* fn = "pmp_polytraj3d_batch";
    if (!ctx) return PMP_EINVAL;
    if (!prm || nq < 0 || max_waypoints < 2)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_polytraj3d_batch: bad params/nq/max_waypoints");
    if (max_waypoints > kMaxWp)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_polytraj3d_batch: max_waypoints too large for the LDS stage (<= 880)");
    // the reference divides by zero or never leaves its sampling loop on these
    const double amin = std::min(std::min(prm->max_acceleration[0], prm->max_acceleration[1]), prm->max_acceleration[2]);
    if (!finite3(prm->max_velocity) || !finite3(prm->max_acceleration) || !(amin > 0))
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_polytraj3d_batch: constraints must be finite and min(max_acceleration) > 0");
    if (int rc = traj_check_sampling(ctx, fn, point_cap, eval_t, n_eval, prm->min_time_step, sample_dt)) return rc;
    if (nq == 0) return PMP_OK;
    bool form_cells;
    if (int rc = traj_check_paths(ctx, fn, path_xyz, path_off, cells, path_len, path_cap, X, Y, Z, form_cells)) return rc;
    if (!points || !n_points || !total_time || !segment_times || !status)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_polytraj3d_batch: null pointer argument");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(polytraj3d_kernel, dim3(nq), dim3(64), 8 * lds_doubles(max_waypoints), (hipStream_t)stream, *prm,
                       nq, form_cells ? nullptr : path_xyz, form_cells ? nullptr : path_off, form_cells ? cells : nullptr,
                       form_cells ? path_len : nullptr, path_cap, Y, Z, bc, max_waypoints, point_cap, points, n_points,
                       total_time, segment_times, status, eval_t, n_eval, sample_dt);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}
