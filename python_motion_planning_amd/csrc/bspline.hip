// Batched waypoint curves for gfx950: BSpline.run() (curve_generation/bspline_curve.py:219-271), BSpline3D.run()
// (bspline_curve3d.py:164-220) and CubicSpline.run() (cubic_spline.py:84-111).  All f64, -ffp-contract=off.
//
// B-spline: one wave64 per curve (one wave per workgroup, so __syncthreads() is the wave's own barrier), the
// curve's whole state in LDS, sized by the launch's longest curve (7 waypoints at k = 4: 3,120 B; 64 at
// k = 5: 16,688 B).  Stages:
//  1. parameters (paramSelection): the segment lengths on the lanes, their left-to-right sum by lane 0;
//  2. knots (knotGeneration): one knot per lane, the k parameters summed in the reference's order;
//  3. basis values: the reference's Cox-de Boor recursion visits every (point, function) pair; only the
//     k + 1 functions of the span knot[mu] <= t < knot[mu + 1] can be non-zero, and the triangular scheme
//     over them evaluates the same expressions in the same order (the recursion's other operands are exact
//     zeros), so the values are the reference's bits;
//  4. control points.  interpolation: row i of the collocation matrix has its non-zeros in columns
//     mu_i - k .. mu_i, inside i - k .. i + k for every matrix that can be inverted (Schoenberg-Whitney), so it
//     is kept as a band of 2 k + 1 columns and eliminated without pivoting (it is totally positive), one
//     pivot a step with the k rows x (k + dim) columns it touches on the lanes.  A pivot that is exactly zero,
//     or a non-zero outside the band, is status 4: the reference's LinAlgError.  approximation: the normal
//     equations of the interior block (n - 3 unknowns, the same band width) through the same elimination,
//     then parameters and knots again from the control polygon;
//  5. samples: 64 rows a round, one per lane, staged through LDS into one contiguous store; the polyline
//     length accumulates on the lanes and is reduced once.
// Cubic spline: one wave64 per waypoint list.  Lane 0 builds the arc-length table (CPython's hypot, a left to
// right sum: the point count and the interval lookup turn on its bits), lanes 0 and 1 solve the natural
// spline's tridiagonal system for x and y (Thomas), then 64 rows a round as above.
// The B-spline's device pieces (the LDS layout, stages 1 to 5) are in bspline_dev.h, which pso.hip shares.
#include <cmath>
#include "bspline_dev.h"

namespace {

using namespace bsdev;

constexpr int kCsMaxWp = 512;      // waypoints of a cubic-spline list
constexpr double kMaxCount = 16777216.0;

__global__ __launch_bounds__(64) void bspline_kernel(bs_cfg C, int n_curves, const double* __restrict__ pts,
                                                     const int32_t* __restrict__ off, int min_wp,
                                                     const double* __restrict__ par_in, const double* __restrict__ knot_in,
                                                     double* __restrict__ par_out, double* __restrict__ knot_out,
                                                     double* __restrict__ ctrl_out, int32_t* __restrict__ nc_out, int T,
                                                     double* __restrict__ pts_out, double* __restrict__ len_out,
                                                     int32_t* __restrict__ st_out)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int q = blockIdx.x, lane = lane_id();
    if (q >= n_curves) return;
    const int k = C.k, dim = C.dim, nm = C.nm, W = 2 * k + 1, nk = nm + k + 1;
    const bs_layout L(nm, k);
    double *D = sm + L.D, *par = sm + L.par, *knot = sm + L.knot, *band = sm + L.band, *rowN = sm + L.rowN;
    double *qk = sm + L.qk, *rhs = sm + L.rhs, *seg = sm + L.seg, *stage = sm + L.stage;
    int* mus = (int*)(sm + L.mu);
    const int n = off[q + 1] - off[q];
    double* po = par_out + (size_t)q * nm;
    double* ko = knot_out + (size_t)q * nk;
    double* co = ctrl_out + (size_t)q * nm * dim;
    double* rows = pts_out ? pts_out + (size_t)q * T * dim : nullptr;
    if (n < min_wp || n > nm) {  // the entry refuses such a launch; a count that changed since is not run
        for (int i = lane; i < nm; i += 64) po[i] = 0.0;
        for (int i = lane; i < nk; i += 64) ko[i] = 0.0;
        for (int i = lane; i < nm * dim; i += 64) co[i] = qnan();
        if (rows)
            for (int i = lane; i < T * dim; i += 64) rows[i] = qnan();
        if (lane == 0) {
            nc_out[q] = 0;
            len_out[q] = qnan();
            st_out[q] = PMP_REF_RAISES;
        }
        return;
    }
    for (int i = lane; i < n * dim; i += 64) D[i] = pts[(size_t)off[q] * dim + i];
    __syncthreads();
    if (par_in) {
        if (lane < n) par[lane] = par_in[(size_t)q * nm + lane];
        __syncthreads();
    } else {
        bs_params(C, D, n, par, seg, lane);
    }
    if (knot_in) {
        for (int i = lane; i < n + k + 1; i += 64) knot[i] = knot_in[(size_t)q * nk + i];
        __syncthreads();
    } else {
        bs_knots(C, par, n, knot, lane);
    }
    bool poisoned = bs_poisoned(par, knot, n, k, lane);
    bool singular = false;
    int nc = n;
    double N[kMaxDeg + 1];
    if (!poisoned && !C.approx) {
        singular = bs_interpolate(C, D, n, par, knot, band, lane);
    } else if (!poisoned) {
        const int h = n - 1, na = n - 3;
        if (lane < n) {
            const double t = par[lane];
            const int mu = bs_span(knot, n, k, t);
            mus[lane] = mu;
            if (mu >= 0) {
                bs_basis(knot, k, mu, t, N);
#pragma unroll
                for (int r = 0; r <= kMaxDeg; r++)
                    if (r <= k) rowN[lane * (k + 1) + r] = N[r];
            }
        }
        __syncthreads();
        if (lane >= 1 && lane <= n - 2) {  // qk (:186-188)
            const double n0 = bs_rowval(rowN, mus, k, lane, 0), n1 = bs_rowval(rowN, mus, k, lane, h - 1);
            for (int c = 0; c < dim; c++)
                qk[(lane - 1) * dim + c] = D[lane * dim + c] - n0 * D[c] - n1 * D[(n - 1) * dim + c];
        }
        __syncthreads();
        if (lane < na) {  // row `lane` of N_^T N_ and of N_^T qk, N_ = N[1 : n - 1, 1 : h - 1]
            double acc[2 * kMaxDeg + 1], b[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int c = 0; c < 2 * kMaxDeg + 1; c++) acc[c] = 0.0;
            for (int i = 1; i <= n - 2; i++) {
                const double v = bs_rowval(rowN, mus, k, i, lane + 1);
                if (v == 0.0) continue;
#pragma unroll
                for (int c = 0; c < 2 * kMaxDeg + 1; c++) {
                    const int o = lane + c - k;  // the other column of N_
                    if (c < W && o >= 0 && o < na) acc[c] += v * bs_rowval(rowN, mus, k, i, o + 1);
                }
#pragma unroll
                for (int c = 0; c < 3; c++)
                    if (c < dim) b[c] += v * qk[(i - 1) * dim + c];
            }
#pragma unroll
            for (int c = 0; c < 2 * kMaxDeg + 1; c++)
                if (c < W) band[lane * W + c] = acc[c];
#pragma unroll
            for (int c = 0; c < 3; c++)
                if (c < dim) rhs[lane * dim + c] = b[c];
        }
        __syncthreads();
        singular = bs_solve(band, k, rhs, dim, na, lane);
        // P = [D[0], the solution, D[-1]] (:192-193)
        const double last = lane < dim ? D[(n - 1) * dim + lane] : 0.0;
        __syncthreads();
        for (int i = lane; i < na * dim; i += 64) D[dim + i] = rhs[i];
        if (lane < dim) D[(h - 1) * dim + lane] = last;
        __syncthreads();
        nc = h;
    }
    if (C.approx) nc = n - 1;
    if (poisoned || singular) {
        for (int i = lane; i < nc * dim; i += 64) D[i] = qnan();
        __syncthreads();
    }
    if (C.approx && !singular) {  // run() (:240-244): parameters and knots of the control polygon
        bs_params(C, D, nc, par, seg, lane);
        bs_knots(C, par, nc, knot, lane);
        if (!poisoned) poisoned = bs_poisoned(par, knot, nc, k, lane);
    }
    for (int i = lane; i < nm; i += 64) po[i] = i < nc ? par[i] : 0.0;
    for (int i = lane; i < nk; i += 64) ko[i] = i < nc + k + 1 ? knot[i] : 0.0;
    for (int i = lane; i < nm * dim; i += 64) co[i] = i < nc * dim ? D[i] : 0.0;
    if (lane == 0) {
        nc_out[q] = nc;
        st_out[q] = singular ? PMP_REF_RAISES : PMP_FOUND;
    }
    if (singular) {
        if (rows)
            for (int i = lane; i < T * dim; i += 64) rows[i] = qnan();
        if (lane == 0) len_out[q] = qnan();
        return;
    }
    // generation() (:197-217) at np.linspace(0, 1, T) and the polyline's length
    const double len = bs_rows(C, knot, D, nc, T, poisoned, stage, rows, lane, [](bool, const double*, const double*) {});
    if (lane == 0) len_out[q] = len;
}

// ---------------------------------------------------------------------------------------------------------
// cubic spline

struct cs_layout {
    int s, a, c, b, d, cp, dp, stage, total;  // a, c, b, d, cp, dp: [2][nm] (x then y)
    __host__ __device__ cs_layout(int nm)
    {
        const int e = even(nm);
        int o = 0;
        s = o; o += e;
        a = o; o += 2 * e;
        c = o; o += 2 * e;
        b = o; o += 2 * e;
        d = o; o += 2 * e;
        cp = o; o += 2 * e;
        dp = o; o += 2 * e;
        stage = o; o += kCh * 5;
        total = o;
    }
};

__global__ __launch_bounds__(64) void cubic_spline_kernel(double step, int row, int n_lists, const double* __restrict__ pts,
                                                          const int32_t* __restrict__ off, int dim, int nm,
                                                          double* __restrict__ arc_out, int32_t* __restrict__ np_out,
                                                          int point_cap, double* __restrict__ pts_out,
                                                          int32_t* __restrict__ st_out)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int q = blockIdx.x, lane = lane_id();
    if (q >= n_lists) return;
    const cs_layout L(nm);
    const int e = even(nm);
    double *S = sm + L.s, *stage = sm + L.stage;
    const int n = off[q + 1] - off[q];
    if (n < 2 || n > nm) {
        if (lane == 0) {
            arc_out[q] = qnan();
            np_out[q] = 0;
            st_out[q] = PMP_REF_RAISES;
        }
        return;
    }
    for (int i = lane; i < n; i += 64) {
        const double* w = pts + ((size_t)off[q] + i) * dim;
        sm[L.a + i] = w[0];
        sm[L.a + e + i] = w[1];
    }
    __syncthreads();
    if (lane == 0) {  // s = [0] + cumsum(hypot) (:103-106)
        double acc = 0.0;
        S[0] = 0.0;
        for (int i = 0; i < n - 1; i++) {
            const double h = lp::py_hypot(sm[L.a + i + 1] - sm[L.a + i], sm[L.a + e + i + 1] - sm[L.a + e + i]);
            acc = i == 0 ? h : acc + h;
            S[i + 1] = acc;
        }
    }
    __syncthreads();
    const double total = S[n - 1];
    const double cnt_f = ceil(total / step);  // len(np.arange(0, s[-1], step))
    const bool raises = !(fabs(total) < kInf) || !(cnt_f <= kMaxCount);
    const int count = raises || !(cnt_f > 0) ? 0 : (int)cnt_f;
    if (lane == 0) {
        arc_out[q] = total;
        np_out[q] = count;
        st_out[q] = raises ? PMP_REF_RAISES : (pts_out && count > point_cap ? PMP_PATH_OVERFLOW : PMP_FOUND);
    }
    if (!pts_out || raises) return;
    if (lane < 2) {  // spline() (:46-67) of this lane's axis: c by the Thomas algorithm, then d and b
        const double* a = sm + L.a + lane * e;
        double *c = sm + L.c + lane * e, *b = sm + L.b + lane * e, *d = sm + L.d + lane * e;
        double *cp = sm + L.cp + lane * e, *dp = sm + L.dp + lane * e;
        cp[0] = 0.0;
        dp[0] = 0.0;
        for (int i = 1; i < n - 1; i++) {
            const double h0 = S[i] - S[i - 1], h1 = S[i + 1] - S[i];
            const double B = 3.0 * (a[i + 1] - a[i]) / h1 - 3.0 * (a[i] - a[i - 1]) / h0;
            const double m = 2.0 * (h0 + h1) - h0 * cp[i - 1];
            cp[i] = h1 / m;
            dp[i] = (B - h0 * dp[i - 1]) / m;
        }
        c[n - 1] = 0.0;
        for (int i = n - 2; i >= 1; i--) c[i] = dp[i] - cp[i] * c[i + 1];
        c[0] = 0.0;
        for (int i = 0; i < n - 1; i++) {
            const double h = S[i + 1] - S[i];
            d[i] = (c[i + 1] - c[i]) / (3.0 * h);
            b[i] = (a[i + 1] - a[i]) / h - h * (c[i + 1] + 2.0 * c[i]) / 3.0;
        }
    }
    __syncthreads();
    const int nrow_all = count < point_cap ? count : point_cap;
    double* out = pts_out + (size_t)q * point_cap * row;
    for (int base = 0; base < nrow_all; base += kCh) {
        const int nrow = nrow_all - base < kCh ? nrow_all - base : kCh;
        if (lane < nrow) {
            const double t = (double)(base + lane) * step;
            int lo = 0, hi = n;  // bisect.bisect(s, t)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (t < S[mid]) hi = mid;
                else lo = mid + 1;
            }
            int i = lo - 1;
            i = i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
            const double dx = t - S[i], dx2 = dx * dx, dx3 = dx2 * dx;
            double p[2], dpv[2];
            for (int ax = 0; ax < 2; ax++) {
                const double a = sm[L.a + ax * e + i], b = sm[L.b + ax * e + i], c = sm[L.c + ax * e + i];
                const double d = sm[L.d + ax * e + i];
                p[ax] = a + b * dx + c * dx2 + d * dx3;
                dpv[ax] = b + 2.0 * c * dx + 3.0 * d * dx2;
            }
            stage[lane * row] = p[0];
            stage[lane * row + 1] = p[1];
            stage[lane * row + 2] = atan2(dpv[1], dpv[0]);
            if (row == 5) {
                stage[lane * row + 3] = dpv[0];
                stage[lane * row + 4] = dpv[1];
            }
        }
        __syncthreads();
        for (int j = lane; j < nrow * row; j += 64) out[(size_t)base * row + j] = stage[j];
        __syncthreads();
    }
}

}  // namespace

extern "C" int pmp_bspline_batch(pmp_ctx* ctx, void* stream, const pmp_bspline_params* prm, int n_curves, const double* pts,
                                 const int32_t* off, int dim, int min_waypoints, int max_waypoints, const double* params_in,
                                 const double* knot_in, double* params, double* knot, double* control, int32_t* n_control,
                                 int n_samples, double* points, double* length, int32_t* status)
{
    const std::string fn = "pmp_bspline_batch";
    if (!ctx) return PMP_EINVAL;
    if (!prm) return pmp_set_err(ctx, PMP_EINVAL, fn + ": null params");
    if (prm->k < 1 || prm->k > kMaxDeg) return pmp_set_err(ctx, PMP_EINVAL, fn + ": k must be 1..5");
    if (!std::isfinite(prm->step) || !(prm->step > 0)) return pmp_set_err(ctx, PMP_EINVAL, fn + ": step must be > 0 and finite");
    if (dim != 2 && dim != 3) return pmp_set_err(ctx, PMP_EINVAL, fn + ": dim must be 2 or 3");
    if (prm->param_mode < PMP_BSPLINE_CENTRIPETAL || prm->param_mode > PMP_BSPLINE_UNIFORM || prm->spline_mode < 0 ||
        prm->spline_mode > 1 || prm->variant < 0 || prm->variant > 1)
        return pmp_set_err(ctx, PMP_EINVAL, fn + ": bad param_mode / spline_mode / variant");
    const double tf = 1.0 / prm->step;  // int(1 / step); BSpline3D: at least 2
    if (!(tf <= kMaxCount)) return pmp_set_err(ctx, PMP_EINVAL, fn + ": more than 2^24 samples (int(1 / step))");
    int T = (int)tf;
    if (prm->variant == PMP_BSPLINE_3D && T < 2) T = 2;
    if (T < 1) return pmp_set_err(ctx, PMP_EINVAL, fn + ": step > 1 gives no sample (the 2D class raises IndexError)");
    if (n_samples != T) return pmp_set_err(ctx, PMP_EINVAL, fn + ": n_samples is not int(1 / step)");
    if (n_curves < 0) return pmp_set_err(ctx, PMP_EINVAL, fn + ": bad n_curves");
    if (n_curves == 0) return PMP_OK;
    const int need = prm->spline_mode == PMP_BSPLINE_APPROXIMATION ? prm->k + 2 : 2;
    if (min_waypoints < 2) return pmp_set_err(ctx, PMP_EINVAL, fn + ": a curve needs at least 2 waypoints");
    if (max_waypoints > kBsMaxWp) return pmp_set_err(ctx, PMP_EINVAL, fn + ": a curve may have at most 64 waypoints");
    if (min_waypoints > max_waypoints) return pmp_set_err(ctx, PMP_EINVAL, fn + ": min_waypoints > max_waypoints");
    if (min_waypoints < need)
        return pmp_set_err(ctx, PMP_EINVAL, fn + ": approximation needs at least k + 2 waypoints (N > H > k)");
    if (!pts || !off || !params || !knot || !control || !n_control || !length || !status)
        return pmp_set_err(ctx, PMP_EINVAL, fn + ": null pointer argument");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    bs_cfg C;
    C.k = prm->k;
    C.dim = dim;
    C.nm = max_waypoints;
    C.param_mode = prm->param_mode;
    C.approx = prm->spline_mode == PMP_BSPLINE_APPROXIMATION;
    C.three_d = prm->variant == PMP_BSPLINE_3D;
    const bs_layout L(C.nm, C.k);
    hipLaunchKernelGGL(bspline_kernel, dim3(n_curves), dim3(64), (size_t)L.total * sizeof(double), (hipStream_t)stream, C,
                       n_curves, pts, off, need, params_in, knot_in, params, knot, control,
                       n_control, T, points, length, status);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}

extern "C" int pmp_cubic_spline_batch(pmp_ctx* ctx, void* stream, const pmp_cubic_spline_params* prm, int n_lists,
                                      const double* pts, const int32_t* off, int dim, int min_waypoints, int max_waypoints,
                                      double* arc_length, int32_t* n_points, int point_cap, double* points, int32_t* status)
{
    const std::string fn = "pmp_cubic_spline_batch";
    if (!ctx) return PMP_EINVAL;
    if (!prm) return pmp_set_err(ctx, PMP_EINVAL, fn + ": null params");
    if (!std::isfinite(prm->step) || !(prm->step > 0)) return pmp_set_err(ctx, PMP_EINVAL, fn + ": step must be > 0 and finite");
    if (dim != 2 && dim != 3) return pmp_set_err(ctx, PMP_EINVAL, fn + ": dim must be 2 or 3");
    if (n_lists < 0 || point_cap < 1) return pmp_set_err(ctx, PMP_EINVAL, fn + ": bad n_lists/point_cap");
    if (n_lists == 0) return PMP_OK;
    if (min_waypoints < 2) return pmp_set_err(ctx, PMP_EINVAL, fn + ": a list needs at least 2 waypoints");
    if (max_waypoints > kCsMaxWp) return pmp_set_err(ctx, PMP_EINVAL, fn + ": a list may have at most 512 waypoints");
    if (min_waypoints > max_waypoints) return pmp_set_err(ctx, PMP_EINVAL, fn + ": min_waypoints > max_waypoints");
    if (!pts || !off || !arc_length || !n_points || !status) return pmp_set_err(ctx, PMP_EINVAL, fn + ": null pointer argument");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const cs_layout L(max_waypoints);
    hipLaunchKernelGGL(cubic_spline_kernel, dim3(n_lists), dim3(64), (size_t)L.total * sizeof(double), (hipStream_t)stream,
                       prm->step, prm->with_derivative ? 5 : 3, n_lists, pts, off, dim, max_waypoints, arc_length, n_points,
                       point_cap, points, status);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}
