// Batched Dubins.generation() (curve_generation/dubins_curve.py:38-313, curve.py:34-55) for gfx950: the
// steering function and distance metric of the nonholonomic sampling planners.
//
// Three kernels, all f64 in the reference's operation order (-ffp-contract=off):
//  1. steps: R[k], the reference's repeated sum `length += d_length` (:283-294; k * step rounds
//     differently: (0,0,0) -> (10,0,0) at step 0.1 has 28 points, k * step would give 29).  The step is one
//     value per launch, so one lane builds the table once and every pair searches it.
//  2. solve: one lane per pose pair.  theta / dist / alpha / beta (:253-261), the six words LSL, RSR, LSR,
//     RSL, RLR, LRL (:38-205), the first strictly cheapest (:267-273), each piece's count by binary search
//     in R, the point count 1 + sum(count + 1) less the trailing points whose local x is exactly 0.0
//     (:301-304: the reference strips real points too, so a pair of equal poses has no point).  In the
//     cost-matrix form pair n is (starts[n / B], goals[n % B]), decoded here, and nothing is counted.
//  3. sample: one wave64 per pair, 64 points a round.  A lane's point i lies in piece j at step k:
//     interpolate() (:207-236) from the piece's start pose by the signed R[k], or by the piece's exact
//     length at its end; pieces 2.. start where the previous piece ends, computed once per wave.  Rotation by
//     theta, translation, pi2pi on the yaw; the rows (x, y, yaw) go through an LDS stage so that the
//     wave stores them as one contiguous run.
// The sampler (the steps kernel, interpolate, the pieces and their points, the strip) takes a list of
// (mode, signed length) pieces, as the reference's loop does (d_length follows the length's sign); it
// lives in curve_sample.h, instantiated here at three pieces, and reeds_shepp.hip shares it.
#include <cmath>
#include "localplan.h"
#include "traj_sample.h"
#include "curve_sample.h"

namespace {

constexpr int kCh = 64;   // points per round (one per lane)
constexpr int kRow = 3;   // doubles per point: x, y, yaw
constexpr int kMaxPieces = 3;
constexpr int kStepsCostOnly = 65536;  // table entries of a launch that stores no rows (longer pieces: added on)
constexpr double kMaxSteps = 16777216.0;  // (t + p + q) / step beyond this is refused per pair (as polytraj3d.hip)
constexpr double kMaxAngle = 64.0;        // |theta|, |alpha|, |beta| beyond this are no angles (see the solve kernel)
constexpr double kPi = lp::kPi;
constexpr double kInf = __builtin_huge_val();

// the three modes of word w (LSL, RSR, LSR, RSL, RLR, LRL), two bits each, six bits a word
constexpr uint64_t word_code(int a, int b, int c) { return (uint64_t)(a | (b << 2) | (c << 4)); }
constexpr uint64_t kWordModes = word_code(MODE_L, MODE_S, MODE_L) | word_code(MODE_R, MODE_S, MODE_R) << 6 |
                                word_code(MODE_L, MODE_S, MODE_R) << 12 | word_code(MODE_R, MODE_S, MODE_L) << 18 |
                                word_code(MODE_R, MODE_L, MODE_R) << 24 | word_code(MODE_L, MODE_R, MODE_L) << 30;
__device__ __forceinline__ int word_mode(int w, int j) { return (int)((kWordModes >> (6 * w + 2 * j)) & 3u); }

// Curve.mod2pi (curve.py:51-55)
__device__ __forceinline__ double mod2pi(double th) { return th - 2.0 * kPi * floor(th / kPi / 2.0); }
// Curve.pi2pi (curve.py:41-49)
__device__ __forceinline__ double pi2pi(double th)
{
    while (th > kPi) th -= 2.0 * kPi;
    while (th < -kPi) th += 2.0 * kPi;
    return th;
}

struct dubins_frame {
    double theta, dist, alpha, beta;
};
// generation()'s coordinate transformation (:253-261)
__device__ __forceinline__ dubins_frame make_frame(const double* s, const double* g, double max_curv)
{
    dubins_frame f;
    const double gx = g[0] - s[0], gy = g[1] - s[1];
    f.theta = mod2pi(atan2(gy, gx));
    f.dist = lp::py_hypot(gx, gy) * max_curv;
    f.alpha = mod2pi(s[2] - f.theta);
    f.beta = mod2pi(g[2] - f.theta);
    return f;
}

struct dubins_best {
    int word;  // 0..5, -1: no word (the reference raises)
    double t, p, q, cost;
};

__device__ __forceinline__ void take(dubins_best& b, int w, bool feasible, double t, double p, double q)
{
    const double cost = fabs(t) + fabs(p) + fabs(q);
    if (feasible && b.cost > cost) {
        b.word = w;
        b.t = t;
        b.p = p;
        b.q = q;
        b.cost = cost;
    }
}

// The six words in the reference's order (:38-205, :264-273).  The reference calls atan2 with the same
// arguments in LSL and LRL, and in RSR and RLR: one call each here.
__device__ __forceinline__ dubins_best solve_words(const dubins_frame& f)
{
    const double alpha = f.alpha, beta = f.beta, d = f.dist;
    const double sa = sin(alpha), sb = sin(beta), ca = cos(alpha), cb = cos(beta), cab = cos(alpha - beta);
    const double d2 = d * d;
    dubins_best b;
    b.word = -1;
    b.t = b.p = b.q = __builtin_nan("");
    b.cost = kInf;
    const double at_l = atan2(cb - ca, d + sa - sb);   // LSL, LRL (-ca + cb is the same sum)
    const double at_r = atan2(ca - cb, d - sa + sb);   // RSR, RLR
    {   // LSL
        const double pp = 2 + d2 - 2 * cab + 2 * d * (sa - sb);
        take(b, 0, !(pp < 0), mod2pi(-alpha + at_l), sqrt(pp), mod2pi(beta - at_l));
    }
    {   // RSR
        const double pp = 2 + d2 - 2 * cab + 2 * d * (sb - sa);
        take(b, 1, !(pp < 0), mod2pi(alpha - at_r), sqrt(pp), mod2pi(-beta + at_r));
    }
    {   // LSR
        const double pp = -2 + d2 + 2 * cab + 2 * d * (sa + sb);
        const double p = sqrt(pp);
        const double a1 = atan2(-ca - cb, d + sa + sb), a2 = atan2(-2.0, p);
        take(b, 2, !(pp < 0), mod2pi(-alpha + a1 - a2), p, mod2pi(-beta + a1 - a2));
    }
    {   // RSL
        const double pp = -2 + d2 + 2 * cab - 2 * d * (sa + sb);
        const double p = sqrt(pp);
        const double a1 = atan2(ca + cb, d - sa - sb), a2 = atan2(2.0, p);
        take(b, 3, !(pp < 0), mod2pi(alpha - a1 + a2), p, mod2pi(beta - a1 + a2));
    }
    {   // RLR and LRL share p (the reference writes the same expression in both)
        const double pc = (6.0 - d2 + 2.0 * cab + 2.0 * d * (sa - sb)) / 8.0;
        const bool ok = !(fabs(pc) > 1.0);
        const double p = mod2pi(2 * kPi - acos(pc));
        const double t_rlr = mod2pi(alpha - at_r + p / 2.0);
        take(b, 4, ok, t_rlr, p, mod2pi(alpha - beta - t_rlr + p));
        const double t_lrl = mod2pi(-alpha + at_l + p / 2.0);
        take(b, 5, ok, t_lrl, p, mod2pi(beta - alpha - t_lrl + p));
    }
    return b;
}

__device__ __forceinline__ void word_pieces(curve_pieces<kMaxPieces>& P, int word, double t, double p, double q)
{
    P.mode[0] = word_mode(word, 0);
    P.mode[1] = word_mode(word, 1);
    P.mode[2] = word_mode(word, 2);
    P.len[0] = t;
    P.len[1] = p;
    P.len[2] = q;
}

template <bool MATRIX>
__global__ __launch_bounds__(256) void dubins_solve_kernel(pmp_dubins_params C, size_t n, const double* __restrict__ starts,
                                                           const double* __restrict__ goals, size_t B,
                                                           const double* __restrict__ R, int nr, int point_cap,
                                                           int with_points, uint8_t* __restrict__ word_out,
                                                           double* __restrict__ tpq_out, double* __restrict__ cost_out,
                                                           int32_t* __restrict__ np_out, int32_t* __restrict__ st_out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t ia = MATRIX ? i / B : i, ib = MATRIX ? i % B : i;
    const double s[3] = {starts[3 * ia], starts[3 * ia + 1], starts[3 * ia + 2]};
    const double g[3] = {goals[3 * ib], goals[3 * ib + 1], goals[3 * ib + 2]};
    const dubins_frame f = make_frame(s, g, C.max_curv);
    const dubins_best b = solve_words(f);
    word_out[i] = (uint8_t)(b.word < 0 ? 255 : b.word);
    cost_out[i] = b.cost;
    if (MATRIX) return;
    tpq_out[3 * i] = b.t;
    tpq_out[3 * i + 1] = b.p;
    tpq_out[3 * i + 2] = b.q;
    // the reference raises: no word (sum() of None: non-finite poses), int() of a non-finite quotient, or
    // more points than the int(sum / step) + 6 slots of its lists; or its pi2pi never ends: a coordinate or
    // yaw so large that mod2pi leaves no angle in [0, 2 pi] (from 1e17 on its error exceeds a turn)
    const double slots = ((0.0 + b.t) + b.p + b.q) / C.step;
    const bool angles = fabs(f.theta) <= kMaxAngle && fabs(f.alpha) <= kMaxAngle && fabs(f.beta) <= kMaxAngle;
    if (b.word < 0 || !(fabs(slots) < kInf) || !angles) {
        np_out[i] = 0;
        st_out[i] = PMP_REF_RAISES;
        return;
    }
    if (!(slots < kMaxSteps)) {  // more steps than any buffer holds: nothing is counted
        np_out[i] = 0;
        st_out[i] = PMP_PATH_OVERFLOW;
        return;
    }
    curve_pieces<kMaxPieces> P;
    word_pieces(P, b.word, b.t, b.p, b.q);
    lay_pieces(P, 3, f.alpha, R, nr, C.step, C.max_curv);
    if ((double)P.total > trunc(slots) + 6.0) {
        np_out[i] = 0;
        st_out[i] = PMP_REF_RAISES;
        return;
    }
    const int cnt = stripped_count(P, 3, f.alpha, R, nr, C.step, C.max_curv);
    np_out[i] = cnt;
    st_out[i] = with_points && cnt > point_cap ? PMP_PATH_OVERFLOW : PMP_FOUND;
}

__global__ __launch_bounds__(64) void dubins_sample_kernel(pmp_dubins_params C, int n, const double* __restrict__ starts,
                                                           const double* __restrict__ goals, const double* __restrict__ R,
                                                           int nr, const uint8_t* __restrict__ word_in,
                                                           const double* __restrict__ tpq_in,
                                                           const int32_t* __restrict__ np_in, int point_cap,
                                                           double* __restrict__ pts_out)
{
    __shared__ __attribute__((aligned(16))) double stage[kCh * kRow];
    const int q = blockIdx.x;
    const int lane = lane_id();
    if (q >= n) return;
    const int count = np_in[q];
    const int nrow_all = count < point_cap ? count : point_cap;
    const int word = word_in[q];
    if (nrow_all <= 0 || word > 5) return;
    const double s[3] = {starts[3 * (size_t)q], starts[3 * (size_t)q + 1], starts[3 * (size_t)q + 2]};
    const double g[3] = {goals[3 * (size_t)q], goals[3 * (size_t)q + 1], goals[3 * (size_t)q + 2]};
    const dubins_frame f = make_frame(s, g, C.max_curv);
    curve_pieces<kMaxPieces> P;
    word_pieces(P, word, tpq_in[3 * (size_t)q], tpq_in[3 * (size_t)q + 1], tpq_in[3 * (size_t)q + 2]);
    lay_pieces(P, 3, f.alpha, R, nr, C.step, C.max_curv);
    const double ct = cos(f.theta), sn = sin(f.theta);
    double* pts = pts_out + (size_t)q * point_cap * kRow;
    for (int base = 0; base < nrow_all; base += kCh) {
        const int nrow = nrow_all - base < kCh ? nrow_all - base : kCh;
        if (lane < nrow) {
            // rows < point_cap <= nr - 1: every step of theirs is in the table
            const pose o = local_point(P, 3, base + lane, f.alpha, R, nr, C.step, C.max_curv);
            double* r = stage + lane * kRow;
            r[0] = (ct * o.x - sn * o.y) + s[0];
            r[1] = (sn * o.x + ct * o.y) + s[1];
            r[2] = pi2pi(o.yaw + f.theta);
        }
        __syncthreads();
        traj_store_rows<kRow>(pts, stage, base, nrow, lane);
        __syncthreads();
    }
}

int check_params(pmp_ctx* ctx, const char* fn, const pmp_dubins_params* prm)
{
    if (!prm) return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": null params");
    // the reference never leaves its loop (step) or divides by zero (max_curv) on these
    if (!std::isfinite(prm->step) || !(prm->step > 0) || !std::isfinite(prm->max_curv) || !(prm->max_curv > 0))
        return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": step and max_curv must be > 0 and finite");
    return PMP_OK;
}

}  // namespace

extern "C" int pmp_dubins_batch(pmp_ctx* ctx, void* stream, const pmp_dubins_params* prm, int n, const double* start_xyyaw,
                                const double* goal_xyyaw, uint8_t* word, double* tpq, double* cost, int32_t* n_points,
                                int point_cap, double* points, int32_t* status)
{
    const char* fn = "pmp_dubins_batch";
    if (!ctx) return PMP_EINVAL;
    if (int rc = check_params(ctx, fn, prm)) return rc;
    if (n < 0 || point_cap < 1) return pmp_set_err(ctx, PMP_EINVAL, "pmp_dubins_batch: bad n/point_cap");
    if (n == 0) return PMP_OK;
    if (!start_xyyaw || !goal_xyyaw || !word || !tpq || !cost || !n_points || !status)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_dubins_batch: null pointer argument");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    // R[0 .. nr - 1]: a stored row i < point_cap is at most step i of its piece
    const int nr = (points ? point_cap : std::min(point_cap, kStepsCostOnly)) + 1;
    double* R = (double*)pmp_scratch(ctx, SCR_DUBINS_STEPS, (size_t)nr * 8);
    if (!R) return PMP_ENOMEM;
    hipLaunchKernelGGL(curve_steps_kernel, dim3(1), dim3(64), 0, s, prm->step, nr, R);
    hipLaunchKernelGGL(dubins_solve_kernel<false>, dim3((unsigned)(((size_t)n + 255) / 256)), dim3(256), 0, s, *prm, (size_t)n, start_xyyaw,
                       goal_xyyaw, (size_t)1, R, nr, point_cap, points ? 1 : 0, word, tpq, cost, n_points, status);
    if (points)
        hipLaunchKernelGGL(dubins_sample_kernel, dim3(n), dim3(64), 0, s, *prm, n, start_xyyaw, goal_xyyaw, R, nr, word,
                           tpq, n_points, point_cap, points);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}

extern "C" int pmp_dubins_cost_matrix(pmp_ctx* ctx, void* stream, const pmp_dubins_params* prm, int A,
                                      const double* start_xyyaw, int B, const double* goal_xyyaw, double* cost,
                                      uint8_t* word)
{
    const char* fn = "pmp_dubins_cost_matrix";
    if (!ctx) return PMP_EINVAL;
    if (int rc = check_params(ctx, fn, prm)) return rc;
    if (A < 0 || B < 0) return pmp_set_err(ctx, PMP_EINVAL, "pmp_dubins_cost_matrix: bad A/B");
    if (A == 0 || B == 0) return PMP_OK;
    if (!start_xyyaw || !goal_xyyaw || !cost || !word)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_dubins_cost_matrix: null pointer argument");
    const size_t n = (size_t)A * (size_t)B;
    if ((n + 255) / 256 > 0x7fffffffull) return pmp_set_err(ctx, PMP_EINVAL, "pmp_dubins_cost_matrix: A x B too large");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(dubins_solve_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *prm,
                       n, start_xyyaw, goal_xyyaw, (size_t)B, nullptr, 0, 0, 0, word, nullptr, cost, nullptr, nullptr);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}
