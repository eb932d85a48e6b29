// Batched ReedsShepp.generation() (curve_generation/reeds_shepp.py:37-674, curve.py:41-49) for gfx950: the
// car that can reverse, the steering function and distance metric of the nonholonomic sampling planners
// for parking-style manoeuvres.
//
// Three kernels, all f64 in the reference's operation order (-ffp-contract=off).  sin, cos, tan, asin, acos
// and atan2 are crmath.h's, rounded as the exact value rounds, which is what glibc returns in all but about
// one call in a thousand: the reference decides its point count on `x == 0.0` of a local x that is 0
// mathematically whenever the goal lies abeam of the start, and the device libm's ulp changed that count
// in two of 325 fixture cases.  hypot is CPython's (localplan.h); sqrt and the division round correctly.
//  1. steps: curve_sample.h's table R[k] of the repeated sum `length += d_length` (:651-655).
//  2. solve: one lane per pose pair.  The frame x, y, phi (:621-627), then the 46 candidates in the
//     reference's order, called slots 0..45 here:
//        0- 1  SCS    (:235-258)  SLS on (x, y, phi) and its reflection
//        2- 9  CCC    (:260-319)  LRL on the four reflections, then the same four on the backwards (xb, yb)
//       10-17  CSC    (:321-376)  LSL x 4, LSR x 4
//       18-25  CCCC   (:378-434)  LRLRn x 4, LRLRp x 4
//       26-41  CCSC   (:436-536)  LRSL x 4, LRSR x 4, then each x 4 on (xb, yb)
//       42-45  CCSCC  (:538-573)  LRSLR x 4
//     The four reflections are (x, y, phi), (-x, y, -phi), (x, -y, -phi), (-x, -y, phi): time-flip is bit 0,
//     reflect is bit 1.  One family at a time with only the best candidate live; the reflections are a
//     rolled loop, so the kernel holds one body of each primitive (two of those with a backwards form).
//     sin(phi) and cos(phi) are computed once: sin(-phi) = -sin(phi) and cos(-phi) = cos(phi) exactly, and
//     x - sin(-phi) is x + sin(phi) by IEEE's definition of subtraction, so the primitives see the
//     reference's arguments, signed zeros included (atan2(0.0, -0.0) = pi against atan2(0.0, 0.0) = 0
//     decides which CCC slot of a pair of equal poses costs 0 and which 2 pi).
//     The first strictly cheapest slot wins (:633-637); then, as in dubins.hip, each piece's count by
//     binary search in R, the point count 1 + sum(count + 1) less the trailing points whose local x is
//     exactly 0.0 (:664-667).  In the cost-matrix form pair n is (starts[n / B], goals[n % B]), decoded
//     here, and nothing is counted.
//  3. sample: one wave64 per pair, 64 points a round, curve_sample.h's local_point from the local start
//     pose (0, 0, 0); the transformation back (:670-672) in the reference's operation order; the rows
//     (x, y, yaw) go through an LDS stage so that the wave stores them as one contiguous run.
#include <cmath>
#include "localplan.h"
#include "traj_sample.h"
#include "curve_sample.h"
#include "crmath.h"

namespace {

constexpr int kCh = 64;   // points per round (one per lane)
constexpr int kRow = 3;   // doubles per point: x, y, yaw
constexpr int kMaxPieces = 5;
constexpr int kSlots = 46;
constexpr int kStepsCostOnly = 65536;  // table entries of a launch that stores no rows (longer pieces: added on)
constexpr double kMaxSteps = 16777216.0;  // cost / step beyond this is refused per pair (as dubins.hip)
// |syaw| or |gyaw - syaw| beyond this: refused.  M() below is the reference's loop, |phi| / 2 pi rounds of
// it, and from about 1e16 on (where phi - 2 pi == phi) it never ends; neither does it for an infinite yaw.
constexpr double kMaxAngle = 64.0;
constexpr double kPi = lp::kPi;
constexpr double kHalfPi = 0.5 * kPi;
constexpr double kInf = __builtin_huge_val();

// sin and cos of the sampler, rounded as glibc rounds them (crmath.h)
struct cr_trig {
    static __device__ __forceinline__ void sincos(double x, double& s, double& c) { crm::sincos(x, s, c); }
};

// The word of each slot: two bits a mode, five modes, then the piece count
constexpr uint16_t W(int a, int b, int c) { return (uint16_t)(a | b << 2 | c << 4 | 3 << 10); }
constexpr uint16_t W(int a, int b, int c, int d) { return (uint16_t)(a | b << 2 | c << 4 | d << 6 | 4 << 10); }
constexpr uint16_t W(int a, int b, int c, int d, int e) { return (uint16_t)(a | b << 2 | c << 4 | d << 6 | e << 8 | 5 << 10); }
constexpr int L = MODE_L, S = MODE_S, R_ = MODE_R;
__device__ const uint16_t kSlotWord[kSlots] = {
    W(S, L, S), W(S, R_, S),
    W(L, R_, L), W(L, R_, L), W(R_, L, R_), W(R_, L, R_), W(L, R_, L), W(L, R_, L), W(R_, L, R_), W(R_, L, R_),
    W(L, S, L), W(L, S, L), W(R_, S, R_), W(R_, S, R_), W(L, S, R_), W(L, S, R_), W(R_, S, L), W(R_, S, L),
    W(L, R_, L, R_), W(L, R_, L, R_), W(R_, L, R_, L), W(R_, L, R_, L),
    W(L, R_, L, R_), W(L, R_, L, R_), W(R_, L, R_, L), W(R_, L, R_, L),
    W(L, R_, S, L), W(L, R_, S, L), W(R_, L, S, R_), W(R_, L, S, R_),
    W(L, R_, S, R_), W(L, R_, S, R_), W(R_, L, S, L), W(R_, L, S, L),
    W(L, S, R_, L), W(L, S, R_, L), W(R_, S, L, R_), W(R_, S, L, R_),
    W(R_, S, R_, L), W(R_, S, R_, L), W(L, S, L, R_), W(L, S, L, R_),
    W(L, R_, S, L, R_), W(L, R_, S, L, R_), W(R_, L, S, R_, L), W(R_, L, S, R_, L)};
__device__ __forceinline__ int slot_pieces(int slot) { return kSlotWord[slot] >> 10; }
__device__ __forceinline__ int slot_mode(int slot, int j) { return (kSlotWord[slot] >> (2 * j)) & 3; }

// ReedsShepp.M = Curve.pi2pi (:55-65, curve.py:41-49): the reference's loops, bounded by kMaxAngle
__device__ __forceinline__ double M(double th)
{
    while (th > kPi) th -= 2.0 * kPi;
    while (th < -kPi) th += 2.0 * kPi;
    return th;
}
// ReedsShepp.R (:37-53)
__device__ __forceinline__ void R(double x, double y, double& r, double& theta)
{
    r = lp::py_hypot(x, y);
    theta = crm::atan2(y, x);
}

// What a primitive is called with: x, y, phi of one reflection, and sin(phi), cos(phi) as the reference
// computes them from that phi
struct rs_arg {
    double x, y, phi, s, c;
};

// Reflection r of (x, y, phi): bit 0 time-flip (-x, -phi), bit 1 reflect (-y, -phi)
__device__ __forceinline__ rs_arg reflect(double x, double y, double phi, double s, double c, int r)
{
    const bool neg = ((r ^ (r >> 1)) & 1) != 0;
    rs_arg a;
    a.x = (r & 1) ? -x : x;
    a.y = (r & 2) ? -y : y;
    a.phi = neg ? -phi : phi;
    a.s = neg ? -s : s;
    a.c = c;
    return a;
}

// Straight-Left-Straight (:81-100)
__device__ __forceinline__ bool SLS(const rs_arg& a, double& t, double& u, double& v)
{
    const double phi = M(a.phi);
    if (a.y > 0.0 && 0.0 < phi && phi < kPi * 0.99) {
        const double xd = -a.y / crm::tan(phi) + a.x;
        t = xd - crm::tan(phi / 2.0);
        u = phi;
        v = sqrt((a.x - xd) * (a.x - xd) + a.y * a.y) - crm::tan(phi / 2.0);
        return true;
    } else if (a.y < 0.0 && 0.0 < phi && phi < kPi * 0.99) {
        const double xd = -a.y / crm::tan(phi) + a.x;
        t = xd - crm::tan(phi / 2.0);
        u = phi;
        v = -sqrt((a.x - xd) * (a.x - xd) + a.y * a.y) - crm::tan(phi / 2.0);
        return true;
    }
    return false;
}

// L+R-L- (:102-116)
__device__ __forceinline__ bool LRL(const rs_arg& a, double& t, double& u, double& v)
{
    double r, theta;
    R(a.x - a.s, a.y - 1.0 + a.c, r, theta);
    if (r <= 4.0) {
        u = -2.0 * crm::asin(0.25 * r);
        t = M(theta + 0.5 * u + kPi);
        v = M(a.phi - t + u);
        if (t >= 0.0 && u <= 0.0) return true;
    }
    return false;
}

// L+S+L+ (:118-129)
__device__ __forceinline__ bool LSL(const rs_arg& a, double& t, double& u, double& v)
{
    R(a.x - a.s, a.y - 1.0 + a.c, u, t);
    if (t >= 0.0) {
        v = M(a.phi - t);
        if (v >= 0.0) return true;
    }
    return false;
}

// L+S+R+ (:131-146)
__device__ __forceinline__ bool LSR(const rs_arg& a, double& t, double& u, double& v)
{
    double r, theta;
    R(a.x + a.s, a.y - 1.0 - a.c, r, theta);
    r = r * r;
    if (r >= 4.0) {
        u = sqrt(r - 4.0);
        t = M(theta + crm::atan2(2.0, u));
        v = M(t - a.phi);
        if (t >= 0.0 && v >= 0.0) return true;
    }
    return false;
}

// _calTauOmega (:725-736)
__device__ __forceinline__ void cal_tau_omega(double u, double v, double xi, double eta, double phi, double& tau,
                                              double& omega)
{
    const double delta = M(u - v);
    double su, cu, sd, cd;
    crm::sincos(u, su, cu);
    crm::sincos(delta, sd, cd);
    const double A = su - sd;
    const double B = cu - cd - 1.0;
    const double t1 = crm::atan2(eta * A - xi * B, xi * A + eta * B);
    const double t2 = 2.0 * (cd - cu - cu) + 3.0;  // cos(v) is cos(u): v is u or -u
    tau = t2 < 0 ? M(t1 + kPi) : M(t1);
    omega = M(tau - u + v - phi);
}

// L+R+L-R- (:148-162)
__device__ __forceinline__ bool LRLRn(const rs_arg& a, double& t, double& u, double& v)
{
    const double xi = a.x + a.s, eta = a.y - 1.0 - a.c;
    const double rho = 0.25 * (2.0 + sqrt(xi * xi + eta * eta));
    if (rho <= 1.0) {
        u = crm::acos(rho);
        cal_tau_omega(u, -u, xi, eta, a.phi, t, v);
        if (t >= 0.0 && v <= 0.0) return true;
    }
    return false;
}

// L+R-L-R+ (:164-179)
__device__ __forceinline__ bool LRLRp(const rs_arg& a, double& t, double& u, double& v)
{
    const double xi = a.x + a.s, eta = a.y - 1.0 - a.c;
    const double rho = (20.0 - xi * xi - eta * eta) / 16.0;
    if (0.0 <= rho && rho <= 1.0) {
        u = -crm::acos(rho);
        if (u >= -0.5 * kPi) {
            cal_tau_omega(u, u, xi, eta, a.phi, t, v);
            if (t >= 0.0 && v >= 0.0) return true;
        }
    }
    return false;
}

// L+R-(pi/2)S-R- (:181-196)
__device__ __forceinline__ bool LRSR(const rs_arg& a, double& t, double& u, double& v)
{
    const double xi = a.x + a.s, eta = a.y - 1.0 - a.c;
    double rho, theta;
    R(-eta, xi, rho, theta);
    if (rho >= 2.0) {
        t = theta;
        u = 2.0 - rho;
        v = M(t + 0.5 * kPi - a.phi);
        if (t >= 0.0 && u <= 0.0 && v <= 0.0) return true;
    }
    return false;
}

// L+R-(pi/2)S-L- (:198-214)
__device__ __forceinline__ bool LRSL(const rs_arg& a, double& t, double& u, double& v)
{
    const double xi = a.x - a.s, eta = a.y - 1.0 + a.c;
    double rho, theta;
    R(xi, eta, rho, theta);
    if (rho >= 2.0) {
        const double r = sqrt(rho * rho - 4.0);
        u = 2.0 - r;
        t = M(theta + crm::atan2(r, -2.0));
        v = M(a.phi - 0.5 * kPi - t);
        if (t >= 0.0 && u <= 0.0 && v <= 0.0) return true;
    }
    return false;
}

// L+R-(pi/2)S-L-(pi/2)R+ (:216-233; R()'s angle is not used there)
__device__ __forceinline__ bool LRSLR(const rs_arg& a, double& t, double& u, double& v)
{
    const double xi = a.x + a.s, eta = a.y - 1.0 - a.c;
    const double r = lp::py_hypot(xi, eta);
    if (r >= 2.0) {
        u = 4.0 - sqrt(r * r - 4.0);
        if (u <= 0.0) {
            t = M(crm::atan2((4.0 - u) * xi - 2.0 * eta, -2.0 * xi + (u - 4.0) * eta));
            v = M(t - a.phi);
            if (t >= 0.0 && v >= 0.0) return true;
        }
    }
    return false;
}

struct rs_best {
    int slot;  // 0..45, -1: no candidate below inf (the reference raises)
    double l[kMaxPieces];  // NaN beyond the word's pieces
    double cost;
};

// One candidate: path_length = sum(|l|) as Python's sum adds it (:75), the first strictly shortest wins
// (:636).  flip: the time-flipped forms negate every length.  sc: this pair's slot_costs row, or null.
template <int NP>
__device__ __forceinline__ void take(rs_best& b, double* __restrict__ sc, int slot, bool ok, bool flip, double l0,
                                     double l1, double l2, double l3 = 0.0, double l4 = 0.0)
{
    const double nan = __builtin_nan("");
    double cost = 0.0 + fabs(l0);
    cost += fabs(l1);
    cost += fabs(l2);
    if (NP > 3) cost += fabs(l3);
    if (NP > 4) cost += fabs(l4);
    if (sc) sc[slot] = ok ? cost : nan;
    if (ok && cost < b.cost) {
        b.slot = slot;
        b.cost = cost;
        b.l[0] = flip ? -l0 : l0;
        b.l[1] = flip ? -l1 : l1;
        b.l[2] = flip ? -l2 : l2;
        b.l[3] = NP > 3 ? (flip ? -l3 : l3) : nan;
        b.l[4] = NP > 4 ? (flip ? -l4 : l4) : nan;
    }
}

// The 46 candidates of generation() (:629-637) for the frame (x, y, phi)
__device__ __forceinline__ rs_best solve_slots(double x, double y, double phi, double* __restrict__ sc)
{
    rs_best b;
    b.slot = -1;
    b.cost = kInf;
#pragma unroll
    for (int j = 0; j < kMaxPieces; j++) b.l[j] = __builtin_nan("");
    double s, c;
    crm::sincos(phi, s, c);
    // the backwards transform (:295-297, :492-494)
    const double xb = x * c + y * s, yb = x * s - y * c;
    double t = 0.0, u = 0.0, v = 0.0;
    // SCS: (x, y, phi) and the reflection (x, -y, -phi)
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        const bool ok = SLS(reflect(x, y, phi, s, c, 2 * k), t, u, v);
        take<3>(b, sc, k, ok, false, t, u, v);
    }
    // CCC: LRL, then LRL on (xb, yb) with the lengths reversed
#pragma unroll 1
    for (int k = 0; k < 8; k++) {
        const bool back = k >= 4;
        const bool ok = LRL(reflect(back ? xb : x, back ? yb : y, phi, s, c, k & 3), t, u, v);
        take<3>(b, sc, 2 + k, ok, (k & 1) != 0, back ? v : t, u, back ? t : v);
    }
    // CSC
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        const bool ok = LSL(reflect(x, y, phi, s, c, k), t, u, v);
        take<3>(b, sc, 10 + k, ok, (k & 1) != 0, t, u, v);
    }
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        const bool ok = LSR(reflect(x, y, phi, s, c, k), t, u, v);
        take<3>(b, sc, 14 + k, ok, (k & 1) != 0, t, u, v);
    }
    // CCCC: [t, u, -u, v] and [t, u, u, v]
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        const bool ok = LRLRn(reflect(x, y, phi, s, c, k), t, u, v);
        take<4>(b, sc, 18 + k, ok, (k & 1) != 0, t, u, -u, v);
    }
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        const bool ok = LRLRp(reflect(x, y, phi, s, c, k), t, u, v);
        take<4>(b, sc, 22 + k, ok, (k & 1) != 0, t, u, u, v);
    }
    // CCSC: [t, -pi/2, u, v] of LRSL and of LRSR, then [v, u, -pi/2, t] of each on (xb, yb)
#pragma unroll 1
    for (int k = 0; k < 16; k++) {
        const bool back = k >= 8;
        const rs_arg a = reflect(back ? xb : x, back ? yb : y, phi, s, c, k & 3);
        const bool ok = (k & 4) ? LRSR(a, t, u, v) : LRSL(a, t, u, v);
        take<4>(b, sc, 26 + k, ok, (k & 1) != 0, back ? v : t, back ? u : -kHalfPi, back ? -kHalfPi : u, back ? t : v);
    }
    // CCSCC
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        const bool ok = LRSLR(reflect(x, y, phi, s, c, k), t, u, v);
        take<5>(b, sc, 42 + k, ok, (k & 1) != 0, t, -kHalfPi, u, -kHalfPi, v);
    }
    return b;
}

__device__ __forceinline__ void word_pieces(curve_pieces<kMaxPieces>& P, int slot, const double* __restrict__ l)
{
#pragma unroll
    for (int j = 0; j < kMaxPieces; j++) {
        P.mode[j] = slot_mode(slot, j);
        P.len[j] = l[j];
    }
}

template <bool MATRIX>
__global__ __launch_bounds__(256) void rs_solve_kernel(pmp_reeds_shepp_params C, size_t n, const double* __restrict__ starts,
                                                       const double* __restrict__ goals, size_t B,
                                                       const double* __restrict__ Rt, int nr, int point_cap,
                                                       int with_points, uint8_t* __restrict__ slot_out,
                                                       double* __restrict__ len_out, double* __restrict__ cost_out,
                                                       double* __restrict__ sc_out, int32_t* __restrict__ np_out,
                                                       int32_t* __restrict__ st_out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t ia = MATRIX ? i / B : i, ib = MATRIX ? i % B : i;
    const double sx = starts[3 * ia], sy = starts[3 * ia + 1], syaw = starts[3 * ia + 2];
    // the coordinate transformation (:621-627); phi stays unwrapped, as the reference leaves it
    const double dx = goals[3 * ib] - sx, dy = goals[3 * ib + 1] - sy, phi = goals[3 * ib + 2] - syaw;
    const bool angles = fabs(syaw) <= kMaxAngle && fabs(phi) <= kMaxAngle;  // false for a NaN too
    double* sc = MATRIX || !sc_out ? nullptr : sc_out + kSlots * i;
    rs_best b;
    if (angles) {
        double cs, sn;
        crm::sincos(syaw, sn, cs);
        const double x = (cs * dx + sn * dy) * C.max_curv;
        const double y = (-sn * dx + cs * dy) * C.max_curv;
        b = solve_slots(x, y, phi, sc);
    } else {
        b.slot = -1;
        b.cost = kInf;
        for (int j = 0; j < kMaxPieces; j++) b.l[j] = __builtin_nan("");
        if (sc)
            for (int j = 0; j < kSlots; j++) sc[j] = __builtin_nan("");
    }
    slot_out[i] = (uint8_t)(b.slot < 0 ? 255 : b.slot);
    cost_out[i] = b.cost / C.max_curv;  // as generation() returns it (:674)
    if (MATRIX) return;
    for (int j = 0; j < kMaxPieces; j++) len_out[kMaxPieces * i + j] = b.l[j];
    // the reference raises: no candidate below inf (a non-finite pose) and int(inf / step) (:640), or more
    // points than the int(cost / step) + len(lengths) + 3 slots of its lists; or its M() never ends
    const double slots = b.cost / C.step;
    if (b.slot < 0 || !(slots < kInf)) {
        np_out[i] = 0;
        st_out[i] = PMP_REF_RAISES;
        return;
    }
    if (!(slots < kMaxSteps)) {  // more steps than any buffer holds: nothing is counted
        np_out[i] = 0;
        st_out[i] = PMP_PATH_OVERFLOW;
        return;
    }
    const int np = slot_pieces(b.slot);
    curve_pieces<kMaxPieces> P;
    word_pieces(P, b.slot, b.l);
    lay_pieces<kMaxPieces, cr_trig>(P, np, 0.0, Rt, nr, C.step, C.max_curv);
    if ((double)P.total > trunc(slots) + (double)np + 3.0) {
        np_out[i] = 0;
        st_out[i] = PMP_REF_RAISES;
        return;
    }
    const int cnt = stripped_count<kMaxPieces, cr_trig>(P, np, 0.0, Rt, nr, C.step, C.max_curv);
    np_out[i] = cnt;
    st_out[i] = with_points && cnt > point_cap ? PMP_PATH_OVERFLOW : PMP_FOUND;
}

__global__ __launch_bounds__(64) void rs_sample_kernel(pmp_reeds_shepp_params C, int n, const double* __restrict__ starts,
                                                       const double* __restrict__ Rt, int nr,
                                                       const uint8_t* __restrict__ slot_in,
                                                       const double* __restrict__ len_in,
                                                       const int32_t* __restrict__ np_in, int point_cap,
                                                       double* __restrict__ pts_out)
{
    __shared__ __attribute__((aligned(16))) double stage[kCh * kRow];
    const int q = blockIdx.x;
    const int lane = lane_id();
    if (q >= n) return;
    const int count = np_in[q];
    const int nrow_all = count < point_cap ? count : point_cap;
    const int slot = slot_in[q];
    if (nrow_all <= 0 || slot >= kSlots) return;
    const double sx = starts[3 * (size_t)q], sy = starts[3 * (size_t)q + 1], syaw = starts[3 * (size_t)q + 2];
    const int np = slot_pieces(slot);
    curve_pieces<kMaxPieces> P;
    word_pieces(P, slot, len_in + kMaxPieces * (size_t)q);
    lay_pieces<kMaxPieces, cr_trig>(P, np, 0.0, Rt, nr, C.step, C.max_curv);
    double cm, sm;
    crm::sincos(-syaw, sm, cm);
    double* pts = pts_out + (size_t)q * point_cap * kRow;
    for (int base = 0; base < nrow_all; base += kCh) {
        const int nrow = nrow_all - base < kCh ? nrow_all - base : kCh;
        if (lane < nrow) {
            // rows < point_cap <= nr - 1: every step of theirs is in the table
            const pose o = local_point<kMaxPieces, cr_trig>(P, np, base + lane, 0.0, Rt, nr, C.step, C.max_curv);
            double* r = stage + lane * kRow;
            r[0] = (cm * o.x + sm * o.y) + sx;
            r[1] = (-sm * o.x + cm * o.y) + sy;
            r[2] = M(o.yaw + syaw);
        }
        __syncthreads();
        traj_store_rows<kRow>(pts, stage, base, nrow, lane);
        __syncthreads();
    }
}

int check_params(pmp_ctx* ctx, const char* fn, const pmp_reeds_shepp_params* prm)
{
    if (!prm) return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": null params");
    // the reference never leaves its loop (step) or divides by zero (max_curv) on these
    if (!std::isfinite(prm->step) || !(prm->step > 0) || !std::isfinite(prm->max_curv) || !(prm->max_curv > 0))
        return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": step and max_curv must be > 0 and finite");
    return PMP_OK;
}

}  // namespace

extern "C" int pmp_reeds_shepp_batch(pmp_ctx* ctx, void* stream, const pmp_reeds_shepp_params* prm, int n,
                                     const double* start_xyyaw, const double* goal_xyyaw, uint8_t* slot, double* lengths,
                                     double* cost, double* slot_costs, int32_t* n_points, int point_cap, double* points,
                                     int32_t* status)
{
    const char* fn = "pmp_reeds_shepp_batch";
    if (!ctx) return PMP_EINVAL;
    if (int rc = check_params(ctx, fn, prm)) return rc;
    if (n < 0 || point_cap < 1) return pmp_set_err(ctx, PMP_EINVAL, "pmp_reeds_shepp_batch: bad n/point_cap");
    if (n == 0) return PMP_OK;
    if (!start_xyyaw || !goal_xyyaw || !slot || !lengths || !cost || !n_points || !status)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_reeds_shepp_batch: null pointer argument");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    // R[0 .. nr - 1]: a stored row i < point_cap is at most step i of its piece
    const int nr = (points ? point_cap : std::min(point_cap, kStepsCostOnly)) + 1;
    double* Rt = (double*)pmp_scratch(ctx, SCR_RS_STEPS, (size_t)nr * 8);
    if (!Rt) return PMP_ENOMEM;
    hipLaunchKernelGGL(curve_steps_kernel, dim3(1), dim3(64), 0, s, prm->step, nr, Rt);
    hipLaunchKernelGGL(rs_solve_kernel<false>, dim3((unsigned)(((size_t)n + 255) / 256)), dim3(256), 0, s, *prm, (size_t)n,
                       start_xyyaw, goal_xyyaw, (size_t)1, Rt, nr, point_cap, points ? 1 : 0, slot, lengths, cost, slot_costs,
                       n_points, status);
    if (points)
        hipLaunchKernelGGL(rs_sample_kernel, dim3(n), dim3(64), 0, s, *prm, n, start_xyyaw, Rt, nr, slot, lengths, n_points,
                           point_cap, points);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}

extern "C" int pmp_reeds_shepp_cost_matrix(pmp_ctx* ctx, void* stream, const pmp_reeds_shepp_params* prm, int A,
                                           const double* start_xyyaw, int B, const double* goal_xyyaw, double* cost,
                                           uint8_t* slot)
{
    const char* fn = "pmp_reeds_shepp_cost_matrix";
    if (!ctx) return PMP_EINVAL;
    if (int rc = check_params(ctx, fn, prm)) return rc;
    if (A < 0 || B < 0) return pmp_set_err(ctx, PMP_EINVAL, "pmp_reeds_shepp_cost_matrix: bad A/B");
    if (A == 0 || B == 0) return PMP_OK;
    if (!start_xyyaw || !goal_xyyaw || !cost || !slot)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_reeds_shepp_cost_matrix: null pointer argument");
    const size_t n = (size_t)A * (size_t)B;
    if ((n + 255) / 256 > 0x7fffffffull)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_reeds_shepp_cost_matrix: A x B too large");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(rs_solve_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *prm, n,
                       start_xyyaw, goal_xyyaw, (size_t)B, nullptr, 0, 0, 0, slot, nullptr, cost, nullptr, nullptr, nullptr);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}
