// What the curve kernels (dubins.hip, reeds_shepp.hip) share: the sampler of a curve given as a list of
// (mode, signed length) pieces, as the reference's loop walks it (dubins_curve.py:283-294,
// reeds_shepp.py:646-657: d_length follows the length's sign, the repeated sum `length += d_length` and not
// k * step, then the piece's exact end), templated on the largest piece count of the word family.  A word
// family brings its solver, its local start yaw and its transformation back; everything here is in the
// local frame.
#pragma once
#include <cmath>
#include "pmp_internal.h"

namespace {

enum { MODE_L = 0, MODE_S = 1, MODE_R = 2 };

struct pose {
    double x, y, yaw;
};

// Where a word family takes sin and cos from: the device's libm, or a family's own (reeds_shepp.hip rounds
// them as glibc does, crmath.h)
struct libm_trig {
    static __device__ __forceinline__ void sincos(double x, double& s, double& c)
    {
        s = ::sin(x);
        c = ::cos(x);
    }
};
// interpolate() (dubins_curve.py:207-236, reeds_shepp.py:575-604).  R is L with the length negated: x -+ and
// y +- of the same differences.
template <class T = libm_trig>
__device__ __forceinline__ pose interpolate(int mode, double length, const pose& a, double max_curv)
{
    pose o;
    double s1, c1;
    T::sincos(a.yaw, s1, c1);
    if (mode == MODE_S) {
        o.x = a.x + length / max_curv * c1;
        o.y = a.y + length / max_curv * s1;
        o.yaw = a.yaw;
    } else {
        const double yaw2 = mode == MODE_L ? a.yaw + length : a.yaw - length;
        double s2, c2;
        T::sincos(yaw2, s2, c2);
        const double ds = (s2 - s1) / max_curv, dc = (c2 - c1) / max_curv;
        o.x = mode == MODE_L ? a.x + ds : a.x - ds;
        o.y = mode == MODE_L ? a.y - dc : a.y + dc;
        o.yaw = yaw2;
    }
    return o;
}

// How many steps the reference's loop `length = d; while |length| <= |seg|: length += d` takes: the k >= 1
// with R[k] <= |seg|, R [nr] the repeated sums (R[0] = 0).  A piece longer than the table is finished by
// the same additions.
__device__ __forceinline__ int piece_steps(const double* __restrict__ R, int nr, double step, double seg)
{
    const double a = fabs(seg);
    int lo = 1, hi = nr;  // the first k in [1, nr] with !(R[k] <= a)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (R[mid] <= a) lo = mid + 1;
        else hi = mid;
    }
    int k = lo - 1;
    if (lo == nr && nr >= 1) {
        double len = R[nr - 1] + step, prev = R[nr - 1];
        while (len <= a && len > prev && k < 0x3fffffff) {
            k++;
            prev = len;
            len += step;
        }
    }
    return k;
}

// R[k] of the table, or the same additions carried on past its end (k >= nr: only a piece longer than
// every buffer of the launch, and only when the strip below reaches into it)
__device__ __forceinline__ double step_sum(const double* __restrict__ R, int nr, double step, int k)
{
    if (k < nr) return R[k];
    double acc = R[nr - 1];
    for (int m = nr - 1; m < k; m++) acc += step;
    return acc;
}

// A curve as the sampler sees it: np <= NP pieces of (mode, signed length), their step counts and start poses
template <int NP>
struct curve_pieces {
    int mode[NP];
    double len[NP];
    int cnt[NP];
    pose start[NP];
    pose end;  // of the last piece
    int total;  // 1 + sum(cnt + 1): the points the reference writes
};

// yaw0: the yaw of the local frame's first pose (0, 0, yaw0)
template <int NP, class T = libm_trig>
__device__ __forceinline__ void lay_pieces(curve_pieces<NP>& P, int np, double yaw0, const double* __restrict__ R, int nr,
                                           double step, double max_curv)
{
    pose cur = {0.0, 0.0, yaw0};
    int total = 1;
#pragma unroll
    for (int j = 0; j < NP; j++) {
        if (j < np) {
            P.cnt[j] = piece_steps(R, nr, step, P.len[j]);
            P.start[j] = cur;
            cur = interpolate<T>(P.mode[j], P.len[j], cur, max_curv);
            total += P.cnt[j] + 1;
        }
    }
    P.end = cur;
    P.total = total;
}

// Point i (0 <= i < total) in the local frame: the start, or piece j's k-th step / its end
template <int NP, class T = libm_trig>
__device__ __forceinline__ pose local_point(const curve_pieces<NP>& P, int np, int i, double yaw0,
                                            const double* __restrict__ R, int nr, double step, double max_curv)
{
    if (i == 0) return pose{0.0, 0.0, yaw0};
    int base = 0;
    pose o = P.end;
#pragma unroll
    for (int j = 0; j < NP; j++) {
        if (j < np) {
            const int k = i - base;  // 1 .. cnt: a step; cnt + 1: the piece's end
            if (k >= 1 && k <= P.cnt[j]) {
                const double r = step_sum(R, nr, step, k);
                const double l = P.len[j] > 0.0 ? r : -r;
                o = interpolate<T>(P.mode[j], l, P.start[j], max_curv);
            } else if (k == P.cnt[j] + 1 && j + 1 < np) {
                o = P.start[j + 1];
            }
            base += P.cnt[j] + 1;
        }
    }
    return o;
}

// The reference's count: total less the trailing points whose local x is exactly 0.0 (its unused slots are
// 0.0 too, so the strip runs on into the real points)
template <int NP, class T = libm_trig>
__device__ __forceinline__ int stripped_count(const curve_pieces<NP>& P, int np, double yaw0, const double* __restrict__ R,
                                              int nr, double step, double max_curv)
{
    int n = P.total;
    while (n >= 1) {
        const pose o = local_point<NP, T>(P, np, n - 1, yaw0, R, nr, step, max_curv);
        if (!(o.x == 0.0)) break;
        n--;
    }
    return n;
}

// R[0] = 0, R[k + 1] = R[k] + step: one lane, the reference's own additions.  The step is one value per
// launch, so the table is built once and every pair searches it.
__global__ void curve_steps_kernel(double step, int nr, double* __restrict__ R)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double acc = 0.0;
    for (int k = 0; k < nr; k++) {
        R[k] = acc;
        acc += step;
    }
}

}  // namespace
