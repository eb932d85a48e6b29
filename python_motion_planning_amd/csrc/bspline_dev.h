// The device pieces of BSpline.run() (curve_generation/bspline_curve.py:219-271) and BSpline3D.run(), shared by
// bspline.hip (one curve per workgroup of one wave) and pso.hip (one curve per wave of a larger workgroup).
// One wave64 works on one curve whose state lies in LDS (bs_layout).  All f64, -ffp-contract=off.
//
// BS_SYNC() orders a wave's LDS writes before the reads of its other lanes.  Where the workgroup is the wave
// (bspline.hip) it is __syncthreads(), as it always was; a file whose workgroup has several waves, each on a
// curve of its own, defines it before the include as a wave-scope fence (the waves take different paths, so a
// workgroup barrier inside these functions would not be met by all of them).  The functions' bodies therefore
// differ between the files that include this one, so they have internal linkage (the unnamed namespace): no two
// translation units share a definition, with relocatable device code as without.
#pragma once
#include <cmath>
#include "localplan.h"

#ifndef BS_SYNC
#define BS_SYNC() __syncthreads()
#endif

namespace bsdev {
namespace {

constexpr int kCh = 64;           // rows per round (one per lane)
constexpr int kMaxDeg = 5;         // largest degree k
constexpr int kBsMaxWp = 64;       // waypoints of a B-spline curve: one per lane
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
__device__ inline void bs_params(const bs_cfg& C, const double* P, int n, double* par, double* seg, int lane)
{
    if (C.param_mode == PMP_BSPLINE_UNIFORM) {
        const double st = 1.0 / (double)(n - 1);  // np.linspace: i * (delta / div), the last exactly 1
        if (lane < n) par[lane] = lane == n - 1 ? 1.0 : (double)lane * st;
        BS_SYNC();
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
    BS_SYNC();
    if (lane == 0) {  // np.cumsum
        double acc = seg[0];
        for (int i = 1; i < n - 1; i++) {
            acc += seg[i];
            seg[i] = acc;
        }
    }
    BS_SYNC();
    const double total = seg[n - 2];
    const bool guard = C.three_d && !(total > 0);  // BSpline3D: `if s[-1] > 0`, else zeros
    if (lane < n) par[lane] = lane == 0 || guard ? 0.0 : seg[lane - 1] / total;
    BS_SYNC();
}

// knotGeneration of n parameters -> knot [n + k + 1]
__device__ inline void bs_knots(const bs_cfg& C, const double* par, int n, double* knot, int lane)
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
    BS_SYNC();
}

// A parameter or knot that is no number (the 2D class where all points coincide: 0 / 0) makes every
// entry of the reference's matrices NaN, and with them every control point and row
__device__ __forceinline__ bool bs_poisoned(const double* par, const double* knot, int n, int k, int lane)
{
    return ballot((lane < n && !(fabs(par[lane]) < kInf)) || (lane < n + k + 1 && !(fabs(knot[lane]) < kInf)) ||
                  (lane + 64 < n + k + 1 && !(fabs(knot[lane + 64]) < kInf))) != 0;
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
__device__ inline bool bs_solve(double* band, int k, double* X, int dim, int n, int lane)
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
        BS_SYNC();
    }
    if (lane < dim) {  // back substitution: a lane keeps to its own column
        for (int j = n - 1; j >= 0; j--) {
            double acc = X[j * dim + lane];
            for (int u = 1; u <= k && j + u < n; u++) acc -= band[j * W + k + u] * X[(j + u) * dim + lane];
            X[j * dim + lane] = acc / band[j * W + k];
        }
    }
    BS_SYNC();
    return false;
}

// N[i][j] of the approximation's matrix from the stored spans
__device__ __forceinline__ double bs_rowval(const double* rowN, const int* mu, int k, int i, int j)
{
    const int m = mu[i];
    return m >= 0 && j >= m - k && j <= m ? rowN[i * (k + 1) + (j - (m - k))] : 0.0;
}

// interpolation() (bspline_curve.py:130-152): the collocation matrix of the n points D [n][dim] at their
// parameters as a band, solved in place: D becomes the control points.  Returns true where the reference raises
// LinAlgError (a pivot that is exactly zero, or a non-zero outside the band).  All lanes; barriers inside.
__device__ inline bool bs_interpolate(const bs_cfg& C, double* D, int n, const double* par, const double* knot,
                                      double* band, int lane)
{
    const int k = C.k, W = 2 * k + 1;
    double N[kMaxDeg + 1];
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
    BS_SYNC();
    if (ballot(outside) != 0) return true;
    return bs_solve(band, k, D, C.dim, n, lane);
}

// generation() (:197-217) of the nc control points D at np.linspace(0, 1, T), 64 rows a round, one per lane,
// staged through LDS into one contiguous store to rows (nullable), and the polyline's length, which every lane
// returns.  on_pair(has, p, prev) is called by every lane once a round: has where the lane holds a row that
// has a row before it, p that row and prev the one before.  All lanes; barriers inside.
template <class F>
__device__ inline double bs_rows(const bs_cfg& C, const double* knot, const double* D, int nc, int T, bool poisoned,
                                 double* stage, double* rows, int lane, F&& on_pair)
{
    const int k = C.k, dim = C.dim;
    double N[kMaxDeg + 1];
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
        const bool has = lane < nrow && base + lane > 0;
        if (has) {
            const double dx = p[0] - prev[0], dy = p[1] - prev[1];
            if (C.three_d && dim == 3) {
                const double dz = p[2] - prev[2];
                len_acc += sqrt(dx * dx + dy * dy + dz * dz);
            } else {
                len_acc += lp::py_hypot(dx, dy);
            }
        }
        on_pair(has, p, prev);
#pragma unroll
        for (int c = 0; c < 3; c++) carry[c] = rl_f64(p[c], 63);
        BS_SYNC();
        if (rows)
            for (int j = lane; j < nrow * dim; j += 64) rows[(size_t)base * dim + j] = stage[j];
        BS_SYNC();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) len_acc += __shfl_xor(len_acc, o);
    return len_acc;
}

}  // namespace
}  // namespace bsdev
