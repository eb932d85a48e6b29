// Batched SplineTrajectory3D.generate() / evaluate() / resample() / reparameterize_constant_speed() for
// gfx950 (trajectory/spline_trajectory.py:16-392, trajectory_base.py:193-216, :245-261): the `spline`
// choice after 3D planning (examples/3d_example.py:100-133), for smoothing_factor = 0.
//
// With s = 0 scipy's UnivariateSpline (FITPACK curfit) searches no knots: it places them by a fixed rule
// and returns the interpolating spline on them, which is unique.  One wave64 per path:
//  1. waypoints into LDS (from the f64 list, or decoded from the cell ids a 3D grid planner left on the
//     device); chords lane-parallel, the centripetal parameter's running sum on lane 0 (:60-77);
//  2. k = min(spline_degree, n - 1); knots: k + 1 copies of u[0], the interior knots
//     u[(k+1)/2 : n-(k+1)/2] (odd k) or (u[j] + u[j+1]) / 2 for j = k/2 .. n-k/2-2 (even k), k + 1
//     copies of u[n-1];
//  3. the n x n collocation system B_j(u_i) c_j = p_i, k + 1 non-zeros a row (row i holds the basis of
//     the knot span of u_i, columns off[i] .. off[i] + k), solved for the three axes from one
//     elimination without pivoting (the matrix is totally positive).  Operation order:
//       for c = 0 .. n-2, every row r = c+1 .. c+k with off[r] <= c:
//         m = A[r][c] / A[c][c];  A[r][j] = A[r][j] - m A[c][j] for j = c+1 .. off[c]+k;  b[r] = b[r] - m b[c]
//       for i = n-1 .. 0:  s = b[i];  s = s - A[i][j] x[j] for j = i+1 .. off[i]+k ascending;  x[i] = s / A[i][i]
//     (one lane per (r, j) in the elimination, one lane per axis in the back substitution);
//  4. derivative coefficients c'_i = (c_{i+1} - c_i) k / (t_{i+k+1} - t_{i+1}), once and twice;
//  5. the 500-sample time parameterisation (:154-203), 64 samples a round, the neighbouring sample from
//     the neighbouring lane, times[] summed left to right on lane 0;
//  6. the sampling loop (:216-263) runs twice: the first pass stores nothing and reduces the two
//     ratios of _enforce_constraints (:304-323), the second stores the scaled rows with yaw and yaw rate
//     (traj_sample.h) through an LDS stage as contiguous runs.  evaluate(t), resample(dt) and the
//     constant-speed reparameterisation replace the second pass.
// The basis functions are de Boor's recursion (FITPACK fpbspl); its stages k-2, k-1 and k are the bases
// of q'', q' and q on the same span, so one walk serves all three.  Plain IEEE doubles,
// -ffp-contract=off.
#include "pmp_internal.h"
#include "traj_entry.h"
#include "traj_sample.h"

namespace {

constexpr int kCh = 64;        // points per round (one per lane)
constexpr int kRow = 12;       // doubles per point
constexpr int kNs = 500;       // samples of the time parameterisation (:162)
constexpr int kNarc = 1000;    // samples of the arc-length table (:122)
constexpr int kBand = 6;       // doubles per collocation row (k + 1 <= 6)
constexpr int kMaxWp = 500;    // waypoints whose LDS block (below) fits 64 KiB
constexpr double kMaxSteps = 16777216.0;  // total_time / dt beyond this is refused per path

// C0 C1 C2 [3][nmax] each | U [nmax] | T [nmax + 6] | off [nmax] i32 | TM [kNs] | ARC [kNarc] | stage | tq | meta.
// The collocation band [nmax][kBand] lives in C1 | C2 until the derivative coefficients replace it.
__host__ __device__ constexpr size_t lds_doubles(int nmax)
{
    return 10 * (size_t)nmax + (nmax + 6) + (nmax / 2 + 1) + kNs + kNarc + kCh * kRow + kCh + 2;
}
static_assert(8 * lds_doubles(kMaxWp) <= 64 * 1024, "LDS block");

__device__ __forceinline__ double inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// np.linspace(0, 1, ns)[i]
__device__ __forceinline__ double lin01(int ns, int i) { return i == ns - 1 ? 1.0 : (double)i * (1.0 / (double)(ns - 1)); }

__device__ __forceinline__ double norm3(double a, double b, double c) { return __dsqrt_rn((a * a + b * b) + c * c); }

struct Bsp {
    const double* t;  // knots [n + k + 1]
    const double* c0; // coefficients [3][nmax] of q, q', q''
    const double* c1;
    const double* c2;
    int n, k, nmax;
};

// the knot span of x: the largest s in [k, n - 1] with t[s] <= x (FITPACK splev's search)
__device__ __forceinline__ int bsp_span(const Bsp& B, double x)
{
    int lo = B.k, hi = B.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (B.t[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// de Boor's recursion on span s (fpbspl): after stage j, h[0..j] are the degree-j basis functions
// B_{s-j..s}.  Stages k-2, k-1 and k give q'', q' and q per axis as sums of coefficient x basis, ascending
// (splev); row (nullable) gets the degree-k basis, a collocation row.  The stage is a template argument
// so that every index into h is a constant and h stays in registers.
template <int J>
__device__ __forceinline__ void bsp_dot(const double* c, int nmax, const double (&h)[6], double (&o)[3])
{
#pragma unroll
    for (int d = 0; d < 3; d++) {
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i <= J; i++) sum = sum + c[d * nmax + i] * h[i];
        o[d] = sum;
    }
}

template <int J, bool kPos, bool kD1, bool kD2>
__device__ __forceinline__ void bsp_stage(const Bsp& B, double x, int s, double (&h)[6], double (&pos)[3],
                                          double (&q1)[3], double (&q2)[3], double* row)
{
    if constexpr (J <= 5) {
        const int k = B.k;
        if (J <= k) {
            if constexpr (J >= 1) {
                double hh[J];
#pragma unroll
                for (int i = 0; i < J; i++) hh[i] = h[i];
                h[0] = 0.0;
#pragma unroll
                for (int i = 0; i < J; i++) {
                    const double tr = B.t[s + 1 + i], tl = B.t[s + 1 + i - J];
                    const double g = hh[i] / (tr - tl);
                    h[i] = h[i] + g * (tr - x);
                    h[i + 1] = g * (x - tl);
                }
            }
            // selects between values, never between the arrays: those would put them in memory
            const bool p = kPos && J == k, a = kD1 && J == k - 1, b = kD2 && J == k - 2;
            if (p || a || b) {
                const double *c0 = B.c0, *c1 = B.c1, *c2 = B.c2;
                double sum[3];
                bsp_dot<J>((p ? c0 : (a ? c1 : c2)) + (s - k), B.nmax, h, sum);
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    pos[d] = p ? sum[d] : pos[d];
                    q1[d] = a ? sum[d] : q1[d];
                    q2[d] = b ? sum[d] : q2[d];
                }
            }
            if (row && J == k) {
#pragma unroll
                for (int i = 0; i < kBand; i++) row[i] = i <= J ? h[i] : 0.0;
            }
            bsp_stage<J + 1, kPos, kD1, kD2>(B, x, s, h, pos, q1, q2, row);
        }
    }
}

template <bool kPos, bool kD1, bool kD2>
__device__ __forceinline__ void bsp_eval(const Bsp& B, double x, double (&pos)[3], double (&q1)[3], double (&q2)[3],
                                         double* row = nullptr)
{
    double h[6] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int d = 0; d < 3; d++) pos[d] = q1[d] = q2[d] = 0.0;
    bsp_stage<0, kPos, kD1, kD2>(B, x, bsp_span(B, x), h, pos, q1, q2, row);
}

// interp1d(xs, np.linspace(0, 1, ns), kind='linear', fill_value='extrapolate')(x), then np.clip(., 0, 1)
__device__ __forceinline__ double interp01(const double* xs, int ns, double x)
{
    const int h = traj_interp_upper(xs, ns, x), l0 = h - 1;
    const double xl = xs[l0], xh = xs[h], yl = lin01(ns, l0), yh = lin01(ns, h);
    const double u = (yh - yl) / (xh - xl) * (x - xl) + yl;
    return u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

enum { kGenerate = 0, kEvaluate = 1, kConstSpeed = 2 };

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void splinetraj3d_kernel(
    pmp_splinetraj_params C, int nq, const double* __restrict__ path, const int32_t* __restrict__ off,
    const int32_t* __restrict__ cells, const int32_t* __restrict__ path_len, int path_cap, int Y, int Z, int nmax,
    int point_cap, double* __restrict__ pts_out, int32_t* __restrict__ np_out, double* __restrict__ total_out,
    int32_t* __restrict__ st_out, const double* __restrict__ eval_t, int n_eval, double sample_dt, int constant_speed)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int q = blockIdx.x;
    const int lane = lane_id();
    if (q >= nq) return;
    int wp_cap;
    const int n = traj_waypoint_count(q, off, cells, path_len, path_cap, nmax, wp_cap);
    double* C0 = sm;  // the waypoints, then the spline's coefficients
    double* C1 = C0 + 3 * (size_t)nmax;
    double* C2 = C1 + 3 * (size_t)nmax;
    double* U = C2 + 3 * (size_t)nmax;
    double* T = U + nmax;
    int* roff = (int*)(T + nmax + 6);
    double* tab = (double*)roff + (nmax / 2 + 1);  // times[] and the arc-length table
    double* stage = tab + kNs + kNarc;
    double* tq = stage + kCh * kRow;
    int* meta = (int*)(tq + kCh);
    auto refuse = [&](int st) { traj_refuse(lane, q, st, st_out, np_out, total_out); };
    // n < 3: two waypoints give k = 1, whose derivative(2) raises (:120); k = 1 likewise
    const int k = C.spline_degree < n - 1 ? C.spline_degree : n - 1;
    if (n < 3 || k < 2 || n > wp_cap) {
        refuse(n > wp_cap ? PMP_CAP_OVERFLOW : PMP_REF_RAISES);
        return;
    }
    traj_load_waypoints(C0, nmax, n, q, lane, path, off, cells, path_cap, Y, Z);
    __syncthreads();
    // _compute_centripetal_parameterization (:60-77) and get_path_length (trajectory_base.py:144-149)
    for (int i = lane + 1; i < n; i += 64) {
        const double ch = norm3(C0[i] - C0[i - 1], C0[nmax + i] - C0[nmax + i - 1], C0[2 * nmax + i] - C0[2 * nmax + i - 1]);
        C1[i] = ch;
        U[i] = __dsqrt_rn(ch);
    }
    __syncthreads();
    if (lane == 0) {
        double acc = 0.0, len = 0.0;
        U[0] = 0.0;
        for (int i = 1; i < n; i++) {
            acc = acc + U[i];
            len = len + C1[i];
            U[i] = acc;
        }
        C1[0] = len;
    }
    __syncthreads();
    const double path_length = C1[0];
    {
        const double dn = U[n - 1];
        __syncthreads();
        bool bad = false;
        for (int i = lane; i < n; i += 64) {
            const double u = U[i] / dn;
            // scipy: x must be strictly increasing if s = 0 (repeated consecutive waypoints)
            if (i + 1 < n) bad |= !(U[i + 1] / dn - u > 0.0);
            C2[i] = u;
        }
        __syncthreads();
        for (int i = lane; i < n; i += 64) U[i] = C2[i];
        if (ballot(bad) || !(dn > 0.0) || !(dn < inf())) {
            refuse(PMP_REF_RAISES);
            return;
        }
    }
    __syncthreads();
    // knots
    for (int i = lane; i < n + k + 1; i += 64) {
        double v;
        if (i <= k) v = U[0];
        else if (i >= n) v = U[n - 1];
        else if (k & 1) v = U[i - k - 1 + (k + 1) / 2];
        else {
            const int j = i - k - 1 + k / 2;
            v = (U[j] + U[j + 1]) / 2.0;
        }
        T[i] = v;
    }
    __syncthreads();
    Bsp B;
    B.t = T;
    B.c0 = C0;
    B.c1 = C1;
    B.c2 = C2;
    B.n = n;
    B.k = k;
    B.nmax = nmax;
    // collocation rows
    double* A = C1;  // [n][kBand], through C2
    for (int i = lane; i < n; i += 64) {
        const double x = U[i];
        double pos[3], q1[3], q2[3];
        roff[i] = bsp_span(B, x) - k;
        bsp_eval<false, false, false>(B, x, pos, q1, q2, A + i * kBand);
    }
    __syncthreads();
    // elimination (the order in the header comment): lane = (row below the pivot, column or axis)
    {
        const int rr = lane >> 3, jj = lane & 7;
        for (int c = 0; c + 1 < n; c++) {
            const int r = c + 1 + rr;
            if (rr < k && r < n && roff[r] <= c) {
                const int oc = roff[c], orr = roff[r];
                const double m = A[r * kBand + c - orr] / A[c * kBand + c - oc];
                if (jj < 5) {
                    const int col = c + 1 + jj;
                    if (col <= oc + k) A[r * kBand + col - orr] = A[r * kBand + col - orr] - m * A[c * kBand + col - oc];
                } else {
                    const int d = jj - 5;
                    C0[d * nmax + r] = C0[d * nmax + r] - m * C0[d * nmax + c];
                }
            }
            __syncthreads();
        }
    }
    if (lane < 3) {
        double* x = C0 + lane * nmax;
        for (int i = n - 1; i >= 0; i--) {
            const int oi = roff[i];
            double s = x[i];
            for (int j = i + 1; j <= oi + k; j++) s = s - A[i * kBand + j - oi] * x[j];
            x[i] = s / A[i * kBand + i - oi];
        }
    }
    __syncthreads();
    // spline.derivative(1), spline.derivative(2) (scipy splder)
    for (int e = lane; e < 3 * (n - 1); e += 64) {
        const int d = e / (n - 1), i = e - d * (n - 1);
        C1[d * nmax + i] = (C0[d * nmax + i + 1] - C0[d * nmax + i]) * (double)k / (T[i + k + 1] - T[i + 1]);
    }
    __syncthreads();
    for (int e = lane; e < 3 * (n - 2); e += 64) {
        const int d = e / (n - 2), i = e - d * (n - 2);
        C2[d * nmax + i] = (C1[d * nmax + i + 1] - C1[d * nmax + i]) * (double)(k - 1) / (T[i + k + 1] - T[i + 2]);
    }
    __syncthreads();

    // ---- the two sample tables, 64 samples a round, the previous sample from the neighbouring lane:
    // times[] of _compute_time_parameterization (:154-203), and for the constant-speed mode the
    // arc-length table of _compute_arc_length_parameterization (:122-152); both summed on lane 0
    double* TM = tab;
    double* ARC = tab + kNs;
    const double vclip = fmin(fmin(fabs(C.max_velocity[0]), fabs(C.max_velocity[1])), fabs(C.max_velocity[2]));
    for (int tb = 0; tb < (constant_speed ? 2 : 1); tb++) {
        const int ns = tb ? kNarc : kNs;
        double* X = tb ? ARC : TM;
        double cpos[3] = {0.0, 0.0, 0.0}, cvel = 0.0;  // the previous round's last sample (wave-uniform)
        for (int base = 0; base < ns; base += kCh) {
            const int i = base + lane;
            double pos[3], q1[3], q2[3];
            bsp_eval<true, true, false>(B, lin01(ns, i < ns ? i : ns - 1), pos, q1, q2);
            const double speed = norm3(q1[0], q1[1], q1[2]);
            const double vel = speed > 0.0 ? (vclip < speed ? vclip : speed) : 0.0;
            double ppos[3], pvel = __shfl_up(vel, 1);
#pragma unroll
            for (int d = 0; d < 3; d++) ppos[d] = __shfl_up(pos[d], 1);
            if (lane == 0) {
                pvel = cvel;
#pragma unroll
                for (int d = 0; d < 3; d++) ppos[d] = cpos[d];
            }
            if (i >= 1 && i < ns) {
                const double ds = norm3(pos[0] - ppos[0], pos[1] - ppos[1], pos[2] - ppos[2]);
                const double avg = (vel + pvel) / 2.0;
                X[i] = tb ? ds : (avg > 0.0 ? ds / avg : 0.1);
            }
            cvel = rl_f64(vel, 63);
#pragma unroll
            for (int d = 0; d < 3; d++) cpos[d] = rl_f64(pos[d], 63);
        }
        __syncthreads();
        if (lane == 0) {
            double acc = 0.0;
            X[0] = 0.0;
            for (int i = 1; i < ns; i++) {
                acc = acc + X[i];
                X[i] = acc;
            }
        }
        __syncthreads();
    }
    if (constant_speed) {
        const double al = ARC[kNarc - 1];
        __syncthreads();
        if (al > 0.0)
            for (int i = lane; i < kNarc; i += 64) ARC[i] = ARC[i] / al;
        __syncthreads();
    }
    const double T0 = TM[kNs - 1];
    const int mode = constant_speed ? kConstSpeed : (eval_t || sample_dt > 0.0 ? kEvaluate : kGenerate);
    double* pts = pts_out + (size_t)q * point_cap * kRow;

    // ---- two passes of one sampling loop.  Pass 0 is generate()'s loop (:216-263) storing nothing: it
    // reduces the two ratios of _enforce_constraints (:304-323), which every mode needs before a row is
    // final.  Pass 1 stores rows: generate()'s again, scaled, with yaw; or evaluate(t) (:273-302) at
    // eval_t / at resample()'s repeated sum; or reparameterize_constant_speed()'s loop (:350-392).
    double scale = 1.0, total = T0, cs = 0.0;
    bool scaled = false;
    int count = 0;
    for (int pass = 0; pass < 2; pass++) {
        const bool gen = pass == 0 || mode == kGenerate;
        const double dt = gen || mode == kConstSpeed || eval_t ? C.min_time_step : sample_dt;
        const double* et = gen ? nullptr : eval_t;
        const double bound = gen ? T0 : total;  // the loop's total_time
        if (!(bound < inf()) || (!et && !(bound / dt < kMaxSteps))) {
            refuse(!(bound < inf()) ? PMP_REF_RAISES : PMP_PATH_OVERFLOW);
            if (lane == 0) total_out[q] = bound;
            return;
        }
        const double du = bound > 0.0 ? 1.0 / bound : 0.0;
        double t = 0.0, last_t = -1.0, rv = 0.0, ra = 0.0;
        bool done = false;
        traj_prev pv;
        count = 0;
        while (!done) {
            const traj_round r = traj_round_head(lane, et, n_eval, count, dt, bound, t, last_t, tq, meta, point_cap);
            const int kk = r.k;
            done = r.done;
            // the final point of generate() (:250-263) and of the constant-speed loop (:382-392): u = 1, at rest
            const bool app = (gen || mode == kConstSpeed) && r.appended && lane == kk - 1;
            const int nrow = pass == 0 ? kk : r.nrow;  // the first pass stores nothing: it sees every point
            double my_t = 0.0, vx = 0.0, vy = 0.0;
            double* o = stage + lane * kRow;
            if (lane < nrow) {
                double tc = tq[lane], u;
                if (gen) u = interp01(TM, kNs, tc);
                else if (mode == kEvaluate) {
                    tc = tc < 0.0 ? 0.0 : (tc > bound ? bound : tc);
                    u = bound > 0.0 ? tc / bound : 0.0;
                    u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
                } else u = interp01(ARC, kNarc, bound > 0.0 ? tc / bound : 0.0);
                if (app) u = 1.0;
                double pos[3], v[3], a[3];
                bsp_eval<true, true, true>(B, u, pos, v, a);
                if (!gen && mode == kConstSpeed) {
                    const double nv = norm3(v[0], v[1], v[2]);
#pragma unroll
                    for (int d = 0; d < 3; d++) {
                        v[d] = nv > 0.0 ? (v[d] / nv) * cs : 0.0;
                        a[d] = 0.0;
                    }
                } else {
#pragma unroll
                    for (int d = 0; d < 3; d++) {
                        v[d] = v[d] * du;
                        a[d] = a[d] * (du * du);
                    }
                }
                if (app) {
#pragma unroll
                    for (int d = 0; d < 3; d++) {
                        v[d] = 0.0;
                        a[d] = 0.0;
                    }
                }
                if (pass == 0) {
#pragma unroll
                    for (int d = 0; d < 3; d++) {
                        const double x = fabs(v[d]) / C.max_velocity[d], y = fabs(a[d]) / C.max_acceleration[d];
                        rv = x > rv ? x : rv;
                        ra = y > ra ? y : ra;
                    }
                } else {
                    const bool sc = gen && scaled;
                    my_t = sc ? tc * scale : tc;
                    o[0] = my_t;
#pragma unroll
                    for (int d = 0; d < 3; d++) {
                        o[1 + d] = pos[d];
                        o[4 + d] = sc ? v[d] / scale : v[d];
                        o[7 + d] = sc ? a[d] / (scale * scale) : a[d];
                    }
                    vx = o[4];
                    vy = o[5];
                }
            }
            if (pass == 1) {
                double yaw_col, rate_col;
                traj_yaw_tail(lane, nrow, mode == kGenerate, vx, vy, my_t, pv, yaw_col, rate_col);
                if (lane < nrow) {
                    o[10] = yaw_col;
                    o[11] = rate_col;
                }
                __syncthreads();
                traj_store_rows<kRow>(pts, stage, count, nrow, lane);
            }
            count += kk;
            __syncthreads();
        }
        if (pass == 0) {
            rv = wave_max(rv);
            ra = wave_max(ra);
            scaled = rv > 1.0 || ra > 1.0;
            if (scaled) {
                const double sa = __dsqrt_rn(ra);
                scale = sa > rv ? sa : rv;
                total = T0 * scale;
            }
            if (mode == kConstSpeed) {
                // constant_speed and the new total_time (:336-344)
                const double want = total > 0.0 ? path_length / total : 1.0;
                const double vmin = fmin(fmin(C.max_velocity[0], C.max_velocity[1]), C.max_velocity[2]);
                cs = vmin < want ? vmin : want;
                total = path_length / cs;
            }
        }
    }
    if (lane == 0) {
        total_out[q] = total;
        np_out[q] = count;
        st_out[q] = count > point_cap ? PMP_PATH_OVERFLOW : PMP_FOUND;
    }
}

}  // namespace

extern "C" int pmp_splinetraj3d_max_waypoints(void) { return kMaxWp; }

extern "C" int pmp_splinetraj3d_batch(pmp_ctx* ctx, void* stream, const pmp_splinetraj_params* prm, int nq,
                                      const double* path_xyz, const int32_t* path_off, const int32_t* cells,
                                      const int32_t* path_len, int path_cap, int X, int Y, int Z, int max_waypoints,
                                      int point_cap, double* points, int32_t* n_points, double* total_time,
                                      int32_t* status, const double* eval_t, int n_eval, double sample_dt,
                                      int constant_speed)
{
    const char* fn = "pmp_splinetraj3d_batch";
    if (!ctx) return PMP_EINVAL;
    if (!prm || nq < 0 || max_waypoints < 3)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_splinetraj3d_batch: bad params/nq/max_waypoints");
    if (max_waypoints > kMaxWp)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_splinetraj3d_batch: max_waypoints too large for the LDS block (<= 500)");
    if (prm->spline_degree < 1 || prm->spline_degree > 5)  // scipy: k should be 1 <= k <= 5
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_splinetraj3d_batch: spline_degree must be 1..5");
    // the reference divides by zero (NaN ratios) or never leaves its sampling loop on these
    const double vmin = std::min(std::min(std::fabs(prm->max_velocity[0]), std::fabs(prm->max_velocity[1])),
                                 std::fabs(prm->max_velocity[2]));
    const double amin = std::min(std::min(prm->max_acceleration[0], prm->max_acceleration[1]), prm->max_acceleration[2]);
    if (!finite3(prm->max_velocity) || !finite3(prm->max_acceleration) || !(vmin > 0) || !(amin > 0))
        return pmp_set_err(ctx, PMP_EINVAL,
                           "pmp_splinetraj3d_batch: constraints must be finite, min|max_velocity| > 0, min(max_acceleration) > 0");
    if (int rc = traj_check_sampling(ctx, fn, point_cap, eval_t, n_eval, prm->min_time_step, sample_dt)) return rc;
    if ((eval_t != nullptr) + (sample_dt > 0) + (constant_speed != 0) > 1)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_splinetraj3d_batch: eval_t, sample_dt and constant_speed exclude each other");
    if (nq == 0) return PMP_OK;
    bool form_cells;
    if (int rc = traj_check_paths(ctx, fn, path_xyz, path_off, cells, path_len, path_cap, X, Y, Z, form_cells)) return rc;
    if (!points || !n_points || !total_time || !status)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_splinetraj3d_batch: null pointer argument");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(splinetraj3d_kernel, dim3(nq), dim3(64), 8 * lds_doubles(max_waypoints), (hipStream_t)stream, *prm,
                       nq, form_cells ? nullptr : path_xyz, form_cells ? nullptr : path_off, form_cells ? cells : nullptr,
                       form_cells ? path_len : nullptr, path_cap, Y, Z, max_waypoints, point_cap, points, n_points,
                       total_time, status, eval_t, n_eval, sample_dt, constant_speed);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}
