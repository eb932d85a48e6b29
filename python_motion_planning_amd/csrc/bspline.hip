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
#include <cmath>
#include "localplan.h"

namespace {

constexpr int kCh = 64;            // rows per round (one per lane)
constexpr int kMaxDeg = 5;         // largest degree k
constexpr int kBsMaxWp = 64;       // waypoints of a B-spline curve: one per lane
constexpr int kCsMaxWp = 512;      // waypoints of a cubic-spline list
constexpr double kMaxCount = 16777216.0;
constexpr double kInf = __builtin_huge_val();

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000ll); }
__host__ __device__ inline int even(int v) { return (v + 1) & ~1; }

// The LDS of one curve, in doubles (every block a multiple of 16 B)
struct bs_layout {
    int D, par, knot, band, rowN, qk, rhs, seg, stage, mu, total;
    __host__ __device__ bs_layout(int nm, int k)
    {
        int o = 0;
        D = o; o += even(nm * 3);
        par = o; o += even(nm);
        knot = o; o += even(nm + k + 1);
        band = o; o += even(nm * (2 * k + 1));
        rowN = o; o += even(nm * (k + 1));
        qk = o; o += even(nm * 3);
        rhs = o; o += even(nm * 3);
        seg = o; o += even(nm);
        stage = o; o += kCh * 3;
        mu = o; o += even((nm + 1) / 2);  // int32
        total = o;
    }
};

struct bs_cfg {
    int k, dim, nm;
    int param_mode;   // PMP_BSPLINE_CENTRIPETAL ..
    bool approx, three_d;
};

// paramSelection of the n points P [n][dim] -> par [n].  All lanes; barriers inside.
__device__ void bs_params(const bs_cfg& C, const double* P, int n, double* par, double* seg, int lane)
{
    if (C.param_mode == PMP_BSPLINE_UNIFORM) {
        const double st = 1.0 / (double)(n - 1);  // np.linspace: i * (delta / div), the last exactly 1
        if (lane < n) par[lane] = lane == n - 1 ? 1.0 : (double)lane * st;
        __syncthreads();
        return;
    }
    if (lane < n - 1) {
        const double* a = P + lane * C.dim;
        const double dx = a[C.dim] - a[0], dy = a[C.dim + 1] - a[1];
        double len;
        if (C.three_d) {  // np.linalg.norm(diffs, axis=1): sqrt of the left-to-right sum of squares
            double s = dx * dx + dy * dy;
            if (C.dim == 3) {
                const double dz = a[C.dim + 2] - a[2];
                s = s + dz * dz;
            }
            len = sqrt(s);
        } else {
            len = lp::py_hypot(dx, dy);
        }
        // pow(len, 0.5): the square root, correctly rounded (a libm pow may differ from it by one ulp)
        seg[lane] = C.param_mode == PMP_BSPLINE_CENTRIPETAL ? sqrt(len) : len;
    }
    __syncthreads();
    if (lane == 0) {  // np.cumsum
        double acc = seg[0];
        for (int i = 1; i < n - 1; i++) {
            acc += seg[i];
            seg[i] = acc;
        }
    }
    __syncthreads();
    const double total = seg[n - 2];
    const bool guard = C.three_d && !(total > 0);  // BSpline3D: `if s[-1] > 0`, else zeros
    if (lane < n) par[lane] = lane == 0 || guard ? 0.0 : seg[lane - 1] / total;
    __syncthreads();
}

// knotGeneration of n parameters -> knot [n + k + 1]
__device__ void bs_knots(const bs_cfg& C, const double* par, int n, double* knot, int lane)
{
    for (int i = lane; i < n + C.k + 1; i += 64) {
        double v;
        if (i >= n) v = 1.0;  // also overwrites the zeros n .. k when n <= k
        else if (i <= C.k) v = 0.0;
        else {
            double acc = 0.0;
            for (int j = i - C.k; j < i; j++) acc = acc + par[j];
            v = acc / (double)C.k;
        }
        knot[i] = v;
    }
    __syncthreads();
}

// The mu with knot[mu] <= t < knot[mu + 1] among the functions 0 .. n - 1 of an ascending knot vector
// [n + k + 1] whose entries from n on are equal, or -1 (t outside [knot[0], knot[n]), or NaN)
__device__ __forceinline__ int bs_span(const double* knot, int n, int k, double t)
{
    int lo = 0, hi = n + k + 1;  // the count of knots <= t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (knot[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    const int mu = lo - 1;
    return mu >= 0 && mu <= n - 1 && knot[mu] <= t && t < knot[mu + 1] ? mu : -1;
}

// N[r] = N_{mu - k + r, k}(t), r = 0 .. k, by baseFunction's expressions (bspline_curve.py:55-70): level d
// overwrites N[r] from the level below's N[r] (function i) and N[r + 1] (function i + 1), r ascending.
// Functions of negative index are never an operand of one of index >= 0 and stay 0.
__device__ __forceinline__ void bs_basis(const double* knot, int k, int mu, double t, double* N)
{
#pragma unroll
    for (int r = 0; r <= kMaxDeg; r++) N[r] = 0.0;
#pragma unroll
    for (int r = 0; r <= kMaxDeg; r++)
        if (r == k) N[r] = 1.0;
#pragma unroll
    for (int d = 1; d <= kMaxDeg; d++) {
        if (d > k) break;
#pragma unroll
        for (int r = 0; r <= kMaxDeg; r++) {
            if (r < k - d || r > k) continue;
            const int i = mu - k + r;
            if (i < 0) continue;
            const double a = N[r];
            double b = 0.0;
#pragma unroll
            for (int s = 1; s <= kMaxDeg; s++)
                if (s == r + 1 && s <= k) b = N[s];
            const double len1 = knot[i + d] - knot[i], len2 = knot[i + d + 1] - knot[i + 1];
            const double t1 = len1 == 0.0 ? 0.0 : (t - knot[i]) / len1 * a;
            const double t2 = len2 == 0.0 ? 0.0 : (knot[i + d + 1] - t) / len2 * b;
            N[r] = t1 + t2;
        }
    }
}

// Solve the banded system in place without pivoting: band [n][2 k + 1] (entry (i, j) at column j - i + k), the
// right-hand sides X [n][dim].  Returns true where a pivot is exactly 0.  All lanes; barriers inside.
__device__ bool bs_solve(double* band, int k, double* X, int dim, int n, int lane)
{
    const int W = 2 * k + 1, Wc = k + dim;
    const int r = lane / Wc, c = lane - r * Wc;
    for (int j = 0; j < n; j++) {
        const double piv = band[j * W + k];
        if (piv == 0.0) return true;  // wave-uniform
        const int row = j + 1 + r;
        if (r < k && row < n) {
            const double f = band[row * W + (k - 1 - r)] / piv;
            if (c < k) {
                if (j + 1 + c < n) band[row * W + (c - r + k)] -= f * band[j * W + k + 1 + c];
            } else {
                X[row * dim + (c - k)] -= f * X[j * dim + (c - k)];
            }
        }
        __syncthreads();
    }
    if (lane < dim) {  // back substitution: a lane keeps to its own column
        for (int j = n - 1; j >= 0; j--) {
            double acc = X[j * dim + lane];
            for (int u = 1; u <= k && j + u < n; u++) acc -= band[j * W + k + u] * X[(j + u) * dim + lane];
            X[j * dim + lane] = acc / band[j * W + k];
        }
    }
    __syncthreads();
    return false;
}

// N[i][j] of the approximation's matrix from the stored spans
__device__ __forceinline__ double bs_rowval(const double* rowN, const int* mu, int k, int i, int j)
{
    const int m = mu[i];
    return m >= 0 && j >= m - k && j <= m ? rowN[i * (k + 1) + (j - (m - k))] : 0.0;
}

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
    // A parameter or knot that is no number (the 2D class where all points coincide: 0 / 0) makes every
    // entry of the reference's matrices NaN, and with them every control point and row
    bool poisoned = ballot((lane < n && !(fabs(par[lane]) < kInf)) || (lane < n + k + 1 && !(fabs(knot[lane]) < kInf)) ||
                           (lane + 64 < n + k + 1 && !(fabs(knot[lane + 64]) < kInf))) != 0;
    bool singular = false;
    int nc = n;
    double N[kMaxDeg + 1];
    if (!poisoned && !C.approx) {
        bool outside = false;
        if (lane < n) {
            for (int c = 0; c < W; c++) band[lane * W + c] = 0.0;
            const double t = par[lane];
            const int mu = bs_span(knot, n, k, t);
            if (mu >= 0) {
                bs_basis(knot, k, mu, t, N);
#pragma unroll
                for (int r = 0; r <= kMaxDeg; r++) {
                    const int j = mu - k + r;
                    if (r > k || j < 0) continue;
                    const int c = j - lane + k;
                    if (c >= 0 && c < W) band[lane * W + c] = N[r];
                    else if (N[r] != 0.0) outside = true;
                }
            }
            if (lane == n - 1) band[lane * W + k] = 1.0;  // N[n - 1][n - 1] = 1 (:149)
        }
        __syncthreads();
        singular = ballot(outside) != 0;
        if (!singular) singular = bs_solve(band, k, D, dim, n, lane);
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
        if (!poisoned)
            poisoned = ballot((lane < nc && !(fabs(par[lane]) < kInf)) || (lane < nc + k + 1 && !(fabs(knot[lane]) < kInf)) ||
                              (lane + 64 < nc + k + 1 && !(fabs(knot[lane + 64]) < kInf))) != 0;
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
    const double dtq = 1.0 / (double)(T - 1);
    double len_acc = 0.0, carry[3] = {0.0, 0.0, 0.0};
    for (int base = 0; base < T; base += kCh) {
        const int nrow = T - base < kCh ? T - base : kCh;
        double p[3] = {0.0, 0.0, 0.0};
        if (lane < nrow) {
            const int i = base + lane;
            const double t = T == 1 ? 0.0 : (i == T - 1 ? 1.0 : (double)i * dtq);
            const int mu = bs_span(knot, nc, k, t);
            bool hit = false;  // the last row's N[-1][-1] = 1 replaces a basis value, or stands alone
            if (mu >= 0) {
                bs_basis(knot, k, mu, t, N);
#pragma unroll
                for (int r = 0; r <= kMaxDeg; r++) {
                    const int j = mu - k + r;
                    if (r > k || j < 0) continue;
                    double v = N[r];
                    if (i == T - 1 && j == nc - 1) {
                        v = 1.0;
                        hit = true;
                    }
#pragma unroll
                    for (int c = 0; c < 3; c++)
                        if (c < dim) p[c] += v * D[j * dim + c];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; c++) {
                if (c >= dim) continue;
                if (i == T - 1 && !hit) p[c] += D[(nc - 1) * dim + c];
                if (poisoned) p[c] = qnan();
                stage[lane * dim + c] = p[c];
            }
        }
        // the row before: the lane below, or the round before's last
        double prev[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double up = __shfl_up(p[c], 1);
            prev[c] = lane == 0 ? carry[c] : up;
        }
        if (lane < nrow && base + lane > 0) {
            const double dx = p[0] - prev[0], dy = p[1] - prev[1];
            if (C.three_d && dim == 3) {
                const double dz = p[2] - prev[2];
                len_acc += sqrt(dx * dx + dy * dy + dz * dz);
            } else {
                len_acc += lp::py_hypot(dx, dy);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) carry[c] = rl_f64(p[c], 63);
        __syncthreads();
        if (rows)
            for (int j = lane; j < nrow * dim; j += 64) rows[(size_t)base * dim + j] = stage[j];
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) len_acc += __shfl_xor(len_acc, o);
    if (lane == 0) len_out[q] = len_acc;
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
