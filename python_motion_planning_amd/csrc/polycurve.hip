// Batched Polynomial.generation() (curve_generation/polynomial_curve.py:43-164) and Bezier.generation()
// (curve_generation/bezier_curve.py:34-89) for gfx950: the two pose-pair curves beside Dubins and Reeds-Shepp.
// All f64 in the reference's operation order (-ffp-contract=off: no expression here is fused; the only
// fma() calls are crmath.h's error-free products), powers as repeated multiplication.
//
// Polynomial: the minimum-time quintic between two states (x, y, yaw, v, a) under peak |a| and |jerk| limits,
// found by a search over T in np.arange(t_min, t_max, step).  Three kernels:
//  1. search: one wave64 per pose pair, 64 candidates a round, one per lane.  A candidate is feasible when no
//     sample time k dt has hypot(ax, ay) > max_acc or hypot(jx, jy) > max_jerk: one violating sample rejects it,
//     only all of them accept it.  So a round has two passes.  Sieve: a lane solves its candidate's two
//     3 x 3 systems (Poly.__init__, :43-61: Gaussian elimination with partial pivoting) and tests every 8th
//     of its samples and the last one, leaving at its first violation.  Proof: the survivors in candidate
//     order, the coefficients read from the survivor's lane and all its samples on the lanes, 64 a step,
//     until one has no violation; a ballot, no reduction.  The hypot of the test is CPython's only within
//     1e-12 of the limit; elsewhere the squared sum decides the same.  In the time-matrix form pair n is
//     (starts[n / B], goals[n % B]), decoded here.
//  2. sample: one wave64 per pair, 64 rows a round: time, x, y, yaw, v, a, jerk of the chosen candidate
//     (:134-156).  The signs of a and jerk look back one and two rows (a is negated where v fell, jerk where
//     the signed a fell): v and |a| of the rows before come from the lanes below, and for a round's first
//     two lanes from the round before (kept wave-uniform).  Rows go through an LDS stage to one contiguous
//     store.
// Bezier: one kernel, one wave64 per pair: n = int(hypot / step), the four control points (:82-89), the points
// at np.linspace(0, 1, n) as the left-to-right sum of the four Bernstein terms (:66-69).
#include <cmath>
#include "localplan.h"
#include "traj_sample.h"
#include "crmath.h"

namespace {

constexpr int kCh = 64;        // rows per round (one per lane)
constexpr int kPolyRow = 7;    // time, x, y, yaw, v, a, jerk
constexpr int kBezRow = 2;     // x, y
constexpr double kMaxCount = 16777216.0;  // candidates, sample times or points beyond this are refused
constexpr double kInf = __builtin_huge_val();
constexpr double kBand = 1e-12;  // the squared sum decides outside lim^2 (1 -+ kBand); inside, hypot itself

// Poly (:43-75): p0 .. p5 of one axis
struct quintic {
    double p0, p1, p2, p3, p4, p5;
};

// X = solve(A, b) of Poly.__init__ (:47-53): elimination with partial pivoting (the first largest |entry| of
// the column, its reciprocal scaling the column below it, as LAPACK's getrf does), then the two triangular
// solves.  A singular or non-finite system gives non-finite coefficients, never a trap.
__device__ __forceinline__ quintic make_poly(double x0, double v0, double a0, double xt, double vt, double at, double t)
{
    const double t2 = t * t, t3 = t2 * t, t4 = t3 * t, t5 = t4 * t;
    double A[3][3] = {{t3, t4, t5}, {3 * t2, 4 * t3, 5 * t4}, {6 * t, 12 * t2, 20 * t3}};
    double b[3] = {xt - x0 - v0 * t - a0 * t2 / 2, vt - v0 - a0 * t, at - a0};
#pragma unroll
    for (int c = 0; c < 2; c++) {
        int piv = c;
#pragma unroll
        for (int r = c + 1; r < 3; r++)
            if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
#pragma unroll
        for (int r = c + 1; r < 3; r++) {  // swap rows c and piv (register arrays: selects, not indexing)
            if (piv == r) {
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const double tmp = A[c][j];
                    A[c][j] = A[r][j];
                    A[r][j] = tmp;
                }
                const double tb = b[c];
                b[c] = b[r];
                b[r] = tb;
            }
        }
        const double rcp = 1.0 / A[c][c];
#pragma unroll
        for (int r = c + 1; r < 3; r++) {
            const double l = A[r][c] * rcp;
#pragma unroll
            for (int j = c + 1; j < 3; j++) A[r][j] = A[r][j] - l * A[c][j];
            b[r] = b[r] - l * b[c];
        }
    }
    const double x2 = b[2] / A[2][2];
    const double x1 = (b[1] - x2 * A[1][2]) / A[1][1];
    const double x0s = ((b[0] - x2 * A[0][2]) - x1 * A[0][1]) / A[0][0];
    quintic q;
    q.p0 = x0;
    q.p1 = v0;
    q.p2 = a0 / 2.0;
    q.p3 = x0s;
    q.p4 = x1;
    q.p5 = x2;
    return q;
}

// Poly.x / dx / ddx / dddx (:63-75), the sums left to right
__device__ __forceinline__ double poly_x(const quintic& q, double t)
{
    const double t2 = t * t, t3 = t2 * t, t4 = t3 * t, t5 = t4 * t;
    return q.p0 + q.p1 * t + q.p2 * t2 + q.p3 * t3 + q.p4 * t4 + q.p5 * t5;
}
__device__ __forceinline__ double poly_dx(const quintic& q, double t)
{
    const double t2 = t * t, t3 = t2 * t, t4 = t3 * t;
    return q.p1 + 2 * q.p2 * t + 3 * q.p3 * t2 + 4 * q.p4 * t3 + 5 * q.p5 * t4;
}
__device__ __forceinline__ double poly_ddx(const quintic& q, double t)
{
    const double t2 = t * t, t3 = t2 * t;
    return 2 * q.p2 + 6 * q.p3 * t + 12 * q.p4 * t2 + 20 * q.p5 * t3;
}
__device__ __forceinline__ double poly_dddx(const quintic& q, double t)
{
    const double t2 = t * t;
    return 6 * q.p3 + 24 * q.p4 * t + 60 * q.p5 * t2;
}

// The two boundary states of a pair, split by cos / sin of the yaws (:115-126)
struct poly_pair {
    double sx, sy, svx, svy, sax, say, gx, gy, gvx, gvy, gax, gay;
};
__device__ __forceinline__ poly_pair make_pair(const double* __restrict__ s, const double* __restrict__ g)
{
    double ss, sc, gs, gc;
    crm::sincos(s[2], ss, sc);
    crm::sincos(g[2], gs, gc);
    poly_pair P;
    P.sx = s[0];
    P.sy = s[1];
    P.svx = s[3] * sc;
    P.svy = s[3] * ss;
    P.sax = s[4] * sc;
    P.say = s[4] * ss;
    P.gx = g[0];
    P.gy = g[1];
    P.gvx = g[3] * gc;
    P.gvy = g[3] * gs;
    P.gax = g[4] * gc;
    P.gay = g[4] * gs;
    return P;
}
__device__ __forceinline__ void solve_pair(const poly_pair& P, double T, quintic& qx, quintic& qy)
{
    qx = make_poly(P.sx, P.svx, P.sax, P.gx, P.gvx, P.gax, T);
    qy = make_poly(P.sy, P.svy, P.say, P.gy, P.gvy, P.gay, T);
}

// np.arange(t_min, t_max, step)[i] = t_min + i ((t_min + step) - t_min); len(np.arange(0, T + dt, dt))
__device__ __forceinline__ double candidate_time(const pmp_polycurve_params& C, int i)
{
    return C.t_min + (double)i * ((C.t_min + C.step) - C.t_min);
}
__device__ __forceinline__ int sample_count(const pmp_polycurve_params& C, double T)
{
    const double n = ceil((T + C.dt) / C.dt);
    return n < kMaxCount + 2.0 ? (int)n : (int)kMaxCount + 2;
}

// hypot(a, b) > lim as the reference's max(...) <= lim sees it (a NaN exceeds every limit)
struct limit_test {
    double lim, lo, hi;
    __device__ __forceinline__ explicit limit_test(double l) : lim(l)
    {
        const double l2 = l * l;
        lo = l < 0.0 ? -1.0 : l2 * (1.0 - kBand);
        hi = l < 0.0 ? -1.0 : l2 * (1.0 + kBand);
    }
    __device__ __forceinline__ bool exceeds(double a, double b) const
    {
        const double s = a * a + b * b;
        if (s < lo) return false;
        if (s > hi) return true;
        return !(lp::py_hypot(a, b) <= lim);
    }
};

constexpr int kSieve = 8;  // the search's first pass looks at every kSieve-th sample

// ddx and dddx of both axes as Poly writes them, (6 p3) t, (12 p4) t^2, ..., and the test of one sample
struct sample_test {
    double ax0, ax1, ax2, ax3, jx1, jx2, ay0, ay1, ay2, ay3, jy1, jy2;
    __device__ __forceinline__ sample_test() {}
    __device__ __forceinline__ sample_test(const quintic& qx, const quintic& qy)
        : ax0(2 * qx.p2), ax1(6 * qx.p3), ax2(12 * qx.p4), ax3(20 * qx.p5), jx1(24 * qx.p4), jx2(60 * qx.p5),
          ay0(2 * qy.p2), ay1(6 * qy.p3), ay2(12 * qy.p4), ay3(20 * qy.p5), jy1(24 * qy.p4), jy2(60 * qy.p5)
    {
    }
    // lane c's (c wave-uniform)
    __device__ __forceinline__ sample_test of_lane(int c) const
    {
        sample_test o;
        o.ax0 = rl_f64(ax0, c);
        o.ax1 = rl_f64(ax1, c);
        o.ax2 = rl_f64(ax2, c);
        o.ax3 = rl_f64(ax3, c);
        o.jx1 = rl_f64(jx1, c);
        o.jx2 = rl_f64(jx2, c);
        o.ay0 = rl_f64(ay0, c);
        o.ay1 = rl_f64(ay1, c);
        o.ay2 = rl_f64(ay2, c);
        o.ay3 = rl_f64(ay3, c);
        o.jy1 = rl_f64(jy1, c);
        o.jy2 = rl_f64(jy2, c);
        return o;
    }
    // hypot(ax, ay) > max_acc or hypot(jx, jy) > max_jerk at t = k dt
    __device__ __forceinline__ bool exceeds(int k, double dt, const limit_test& acc, const limit_test& jerk) const
    {
        const double t = (double)k * dt, t2 = t * t, t3 = t2 * t;
        const double ax = ax0 + ax1 * t + ax2 * t2 + ax3 * t3, ay = ay0 + ay1 * t + ay2 * t2 + ay3 * t3;
        const double jx = ax1 + jx1 * t + jx2 * t2, jy = ay1 + jy1 * t + jy2 * t2;
        return acc.exceeds(ax, ay) || jerk.exceeds(jx, jy);
    }
};

template <bool MATRIX>
__global__ __launch_bounds__(256) void polycurve_search_kernel(pmp_polycurve_params C, int nc, size_t n,
                                                                const double* __restrict__ starts,
                                                                const double* __restrict__ goals, size_t B, int point_cap,
                                                                int with_points, int32_t* __restrict__ ti_out,
                                                                double* __restrict__ T_out, int32_t* __restrict__ np_out,
                                                                int32_t* __restrict__ st_out)
{
    const size_t q = (size_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;  // wave-uniform
    const int lane = lane_id();
    if (q >= n) return;
    const size_t ia = MATRIX ? q / B : q, ib = MATRIX ? q % B : q;
    const poly_pair P = make_pair(starts + 5 * ia, goals + 5 * ib);
    const limit_test acc(C.max_acc), jerk(C.max_jerk);
    int found = -1;
    for (int base = 0; base < nc && found < 0; base += kCh) {
        const int i = base + lane;
        const double T = candidate_time(C, i);
        const int ns = sample_count(C, T);
        quintic qx, qy;
        solve_pair(P, T, qx, qy);
        const sample_test mine(qx, qy);
        // sieve: every kSieve-th sample and the last one.  A violation there rejects the candidate for good.
        bool viol = i >= nc;
        for (int k = 0;; k += kSieve) {
            const bool act = !viol && k < ns;
            if (!ballot(act)) break;
            if (act) viol = mine.exceeds(k, C.dt, acc, jerk);
        }
        if (!viol) viol = mine.exceeds(ns - 1, C.dt, acc, jerk);
        // proof: the survivors in order, all samples of one on the lanes, until one has no violation
        uint64_t surv = ballot(!viol);
        while (surv && found < 0) {
            const int c = __builtin_ctzll(surv);
            surv &= surv - 1;
            const sample_test his = mine.of_lane(c);
            const int ns_c = (int)rl_u32((uint32_t)ns, c);
            bool any = false;
            for (int kb = 0; kb < ns_c && !any; kb += kCh) {
                const int k = kb + lane;
                any = ballot(k < ns_c && his.exceeds(k, C.dt, acc, jerk)) != 0;
            }
            if (!any) found = base + c;
        }
    }
    if (lane != 0) return;
    const double T = found < 0 ? kInf : candidate_time(C, found);
    ti_out[q] = found;
    T_out[q] = T;
    if (MATRIX) return;
    const int cnt = found < 0 ? 0 : sample_count(C, T);
    np_out[q] = cnt;
    st_out[q] = found < 0 ? PMP_NO_PATH : (with_points && cnt > point_cap ? PMP_PATH_OVERFLOW : PMP_FOUND);
}

__global__ __launch_bounds__(64) void polycurve_sample_kernel(pmp_polycurve_params C, int n, const double* __restrict__ starts,
                                                              const double* __restrict__ goals,
                                                              const int32_t* __restrict__ ti_in,
                                                              const int32_t* __restrict__ np_in, int point_cap,
                                                              double* __restrict__ pts_out)
{
    __shared__ __attribute__((aligned(16))) double stage[kCh * kPolyRow];
    const int q = blockIdx.x;
    const int lane = lane_id();
    if (q >= n) return;
    const int ti = ti_in[q], count = np_in[q];
    const int nrow_all = count < point_cap ? count : point_cap;
    if (ti < 0 || nrow_all <= 0) return;
    const poly_pair P = make_pair(starts + 5 * (size_t)q, goals + 5 * (size_t)q);
    quintic qx, qy;
    solve_pair(P, candidate_time(C, ti), qx, qy);
    double* pts = pts_out + (size_t)q * point_cap * kPolyRow;
    double pv1 = 0.0, pv2 = 0.0, pa1 = 0.0;  // v of the rows base - 1 and base - 2, |a| of row base - 1
    for (int base = 0; base < nrow_all; base += kCh) {
        const int nrow = nrow_all - base < kCh ? nrow_all - base : kCh;
        // every lane computes (the lanes past nrow too: their values are never stored), so the shifts below
        // read lanes that hold a row
        const int k = base + lane;
        const double t = (double)k * C.dt;
        const double vx = poly_dx(qx, t), vy = poly_dx(qy, t);
        const double v = lp::py_hypot(vx, vy);
        const double a_abs = lp::py_hypot(poly_ddx(qx, t), poly_ddx(qy, t));
        const double j_abs = lp::py_hypot(poly_dddx(qx, t), poly_dddx(qy, t));
        // the two rows before: the lanes below, or the round before
        double v1 = __shfl_up(v, 1), v2 = __shfl_up(v, 2), a1 = __shfl_up(a_abs, 1);
        if (lane == 0) {
            v1 = pv1;
            v2 = pv2;
            a1 = pa1;
        }
        if (lane == 1) v2 = pv1;
        pv1 = rl_f64(v, 63);
        pv2 = rl_f64(v, 62);
        pa1 = rl_f64(a_abs, 63);
        const double ap = k >= 2 && v1 - v2 < 0.0 ? -a1 : a1;      // the signed a of row k - 1
        const double a = k >= 1 && v - v1 < 0.0 ? -a_abs : a_abs;
        const double j = k >= 1 && a - ap < 0.0 ? -j_abs : j_abs;
        if (lane < nrow) {
            double* r = stage + lane * kPolyRow;
            r[0] = t;
            r[1] = poly_x(qx, t);
            r[2] = poly_x(qy, t);
            r[3] = crm::atan2(vy, vx);
            r[4] = v;
            r[5] = a;
            r[6] = j;
        }
        __syncthreads();
        traj_store_rows<kPolyRow>(pts, stage, base, nrow, lane);
        __syncthreads();
    }
}

// Bezier.generation() (bezier_curve.py:47-53) of pair q by one wave
__global__ __launch_bounds__(64) void bezier_kernel(pmp_bezier_params C, int n, const double* __restrict__ starts,
                                                    const double* __restrict__ goals, double* __restrict__ ctrl_out,
                                                    int32_t* __restrict__ np_out, int point_cap,
                                                    double* __restrict__ pts_out, int32_t* __restrict__ st_out)
{
    __shared__ __attribute__((aligned(16))) double stage[kCh * kBezRow];
    const int q = blockIdx.x;
    const int lane = lane_id();
    if (q >= n) return;
    const double* s = starts + 3 * (size_t)q;
    const double* g = goals + 3 * (size_t)q;
    const double sx = s[0], sy = s[1], gx = g[0], gy = g[1];
    const double h = lp::py_hypot(sx - gx, sy - gy);
    const double cnt_f = h / C.step;  // int() of it: towards zero; non-finite: int() raises (:49)
    double ss, sc, gs, gc;
    crm::sincos(s[2], ss, sc);
    crm::sincos(g[2], gs, gc);
    // getControlPoints (:82-89)
    const double dist = h / C.offset;
    const double px[4] = {sx, sx + dist * sc, gx - dist * gc, gx};
    const double py[4] = {sy, sy + dist * ss, gy - dist * gs, gy};
    const bool raises = !(fabs(cnt_f) < kInf);
    const bool huge = !raises && !(cnt_f < kMaxCount);
    const int count = raises || huge ? 0 : (int)cnt_f;
    if (lane == 0) {
        for (int i = 0; i < 4; i++) {
            ctrl_out[8 * (size_t)q + 2 * i] = px[i];
            ctrl_out[8 * (size_t)q + 2 * i + 1] = py[i];
        }
        np_out[q] = count;
        st_out[q] = raises ? PMP_REF_RAISES : (huge || (pts_out && count > point_cap) ? PMP_PATH_OVERFLOW : PMP_FOUND);
    }
    if (!pts_out) return;
    const int nrow_all = count < point_cap ? count : point_cap;
    const double dtq = 1.0 / (double)(count - 1);  // np.linspace's step = delta / div (count 1: unused)
    double* pts = pts_out + (size_t)q * point_cap * kBezRow;
    for (int base = 0; base < nrow_all; base += kCh) {
        const int nrow = nrow_all - base < kCh ? nrow_all - base : kCh;
        if (lane < nrow) {
            const int i = base + lane;
            const double t = count == 1 ? 0.0 : (i == count - 1 ? 1.0 : (double)i * dtq);
            const double u = 1 - t;
            const double t2 = t * t, t3 = t2 * t, u2 = u * u, u3 = u2 * u;
            // comb(3, i) * t ** i * (1 - t) ** (3 - i), left to right (:68)
            const double b0 = (1.0 * 1.0) * u3, b1 = (3.0 * t) * u2, b2 = (3.0 * t2) * u, b3 = (1.0 * t3) * 1.0;
            stage[lane * kBezRow] = ((b0 * px[0] + b1 * px[1]) + b2 * px[2]) + b3 * px[3];
            stage[lane * kBezRow + 1] = ((b0 * py[0] + b1 * py[1]) + b2 * py[2]) + b3 * py[3];
        }
        __syncthreads();
        traj_store_rows<kBezRow>(pts, stage, base, nrow, lane);
        __syncthreads();
    }
}

// The candidate count len(np.arange(t_min, t_max, step)), or -1 with the error set
int check_poly_params(pmp_ctx* ctx, const char* fn, const pmp_polycurve_params* p, int* nc)
{
    if (!p) return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": null params");
    if (!std::isfinite(p->step) || !(p->step > 0))
        return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": step must be > 0 and finite");
    if (!std::isfinite(p->dt) || !(p->dt > 0)) return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": dt must be > 0 and finite");
    if (!std::isfinite(p->t_min) || !(p->t_min > 0) || !std::isfinite(p->t_max))
        return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": t_min must be > 0, t_min and t_max finite");
    if (!std::isfinite(p->max_acc) || !std::isfinite(p->max_jerk))
        return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": max_acc and max_jerk must be finite");
    const double cand = std::ceil((p->t_max - p->t_min) / p->step);
    const double samples = std::ceil((p->t_max + p->dt) / p->dt);
    if (!(cand <= kMaxCount) || !(samples <= kMaxCount))
        return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": more than 2^24 candidate times or sample times");
    *nc = cand > 0 ? (int)cand : 0;
    return PMP_OK;
}

}  // namespace

extern "C" int pmp_polycurve_batch(pmp_ctx* ctx, void* stream, const pmp_polycurve_params* prm, int n, const double* start,
                                   const double* goal, int32_t* t_index, double* T, int32_t* n_points, int point_cap,
                                   double* points, int32_t* status)
{
    const char* fn = "pmp_polycurve_batch";
    if (!ctx) return PMP_EINVAL;
    int nc = 0;
    if (int rc = check_poly_params(ctx, fn, prm, &nc)) return rc;
    if (n < 0 || point_cap < 1) return pmp_set_err(ctx, PMP_EINVAL, "pmp_polycurve_batch: bad n/point_cap");
    if (n == 0) return PMP_OK;
    if (!start || !goal || !t_index || !T || !n_points || !status)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_polycurve_batch: null pointer argument");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(polycurve_search_kernel<false>, dim3((unsigned)(((size_t)n + 3) / 4)), dim3(256), 0, s, *prm, nc, (size_t)n,
                       start, goal, (size_t)1, point_cap, points ? 1 : 0, t_index, T, n_points, status);
    if (points)
        hipLaunchKernelGGL(polycurve_sample_kernel, dim3(n), dim3(64), 0, s, *prm, n, start, goal, t_index, n_points, point_cap,
                           points);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}

extern "C" int pmp_polycurve_time_matrix(pmp_ctx* ctx, void* stream, const pmp_polycurve_params* prm, int A, const double* start,
                                         int B, const double* goal, double* T, int32_t* t_index)
{
    const char* fn = "pmp_polycurve_time_matrix";
    if (!ctx) return PMP_EINVAL;
    int nc = 0;
    if (int rc = check_poly_params(ctx, fn, prm, &nc)) return rc;
    if (A < 0 || B < 0) return pmp_set_err(ctx, PMP_EINVAL, "pmp_polycurve_time_matrix: bad A/B");
    if (A == 0 || B == 0) return PMP_OK;
    if (!start || !goal || !T || !t_index) return pmp_set_err(ctx, PMP_EINVAL, "pmp_polycurve_time_matrix: null pointer argument");
    const size_t n = (size_t)A * (size_t)B;
    if ((n + 3) / 4 > 0x7fffffffull) return pmp_set_err(ctx, PMP_EINVAL, "pmp_polycurve_time_matrix: A x B too large");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(polycurve_search_kernel<true>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, *prm, nc, n,
                       start, goal, (size_t)B, 0, 0, t_index, T, nullptr, nullptr);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}

extern "C" int pmp_bezier_batch(pmp_ctx* ctx, void* stream, const pmp_bezier_params* prm, int n, const double* start_xyyaw,
                                const double* goal_xyyaw, double* control, int32_t* n_points, int point_cap, double* points,
                                int32_t* status)
{
    const char* fn = "pmp_bezier_batch";
    if (!ctx) return PMP_EINVAL;
    if (!prm) return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": null params");
    if (!std::isfinite(prm->step) || !(prm->step > 0))
        return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": step must be > 0 and finite");
    if (!std::isfinite(prm->offset) || prm->offset == 0.0)
        return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": offset must be finite and not 0");
    if (n < 0 || point_cap < 1) return pmp_set_err(ctx, PMP_EINVAL, "pmp_bezier_batch: bad n/point_cap");
    if (n == 0) return PMP_OK;
    if (!start_xyyaw || !goal_xyyaw || !control || !n_points || !status)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_bezier_batch: null pointer argument");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(bezier_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, *prm, n, start_xyyaw, goal_xyyaw, control,
                       n_points, point_cap, points, status);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}
