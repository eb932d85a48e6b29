// Batched particle-swarm planning for gfx950: PSO.plan() (global_planner/evolutionary_search/pso.py:77-123) after
// initializePositions(), on the reference's BSpline(step=0.01, k=4).  All f64, -ffp-contract=off.
//
// One workgroup per plan, `waves` wave64s in it.  The swarm's state (integer positions, f64 velocities, fitness
// and best fitness per particle), a candidate copy of it, the global best and one B-spline state per wave
// (bspline_dev.h) live in LDS, sized by the launch.
//
// The reference's swarm is asynchronous: particles are updated in index order, and one whose best fitness
// exceeds the global best's replaces it at once, so later particles of the same iteration steer towards the new
// best.  Here an iteration evaluates speculatively.  A round evaluates every particle not yet committed against
// the global best as it stands, one particle per wave at a time (velocity and position update on the lanes,
// the stable sort by x, de-duplication, the curve, the collision count over the sample pairs, the fitness),
// into the candidate copy.  Wave 0 then scans in index order for the first particle whose new best fitness
// beats the global best; the candidates up to and including it are committed, the global best is replaced, and
// the particles after it are evaluated again in another round from their committed (pre-iteration) state.
// A particle's draws sit at fixed offsets of the stream, so a repeated evaluation reads the same ones.  The
// result is the sequential algorithm's for any number of waves; repeats counts the evaluations thrown away.
//
// Particle.best_pos is the same list as Particle.position in the reference (pso.py:102-104, :280), so the
// cognitive term is w_cognitive * rand1 * 0: it is computed as that (the sign of the zero counts), and rand1
// is still drawn.
#include <cmath>
#define BS_SYNC() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront")
#include "bspline_dev.h"
#include "grid2d.h"

namespace {

using namespace bsdev;

constexpr int kDeg = 4;            // BSpline(step=0.01, k=4), centripetal, interpolation (pso.py:61)
constexpr int kSamples = 100;      // int(1 / 0.01)
constexpr int kMaxPoints = 62;     // point_num: with start and goal one waypoint per lane
constexpr int kMaxWaves = 16;
constexpr int kDefaultWaves = 16;  // measured: DESIGN.md 3.12 (256 default plans: 130 ms at 16, 172 ms at 8)
constexpr size_t kLdsBytes = 160 * 1024;  // one CU's LDS

// The LDS of one plan: doubles first, then int32
struct pso_layout {
    size_t hd, vel, cvel, fit, best, cfit, bs, pos, cpos, gpos, bytes;  // byte offsets
    int bs_doubles;
    __host__ __device__ pso_layout(int np, int pn, int waves)
    {
        const size_t pp = (size_t)np * pn * 2, e = (size_t)even(np);
        bs_doubles = bs_layout(pn + 2, kDeg).total;
        size_t o = 0;
        hd = o; o += 8 * 8;  // [0] the global best's fitness; ints from [1]: hit, bad
        vel = o; o += pp * 8;
        cvel = o; o += pp * 8;
        fit = o; o += e * 8;
        best = o; o += e * 8;
        cfit = o; o += e * 8;
        bs = o; o += (size_t)waves * bs_doubles * 8;
        pos = o; o += pp * 4;
        cpos = o; o += pp * 4;
        gpos = o; o += (size_t)even(pn * 2) * 4;
        bytes = (o + 15) & ~(size_t)15;
    }
};

struct pso_io {
    const uint32_t* occ;
    const int32_t *start, *goal, *init;
    const double* rnd;
    long long rnd_stride;
    int32_t *status, *best_pos;
    double *best_fit, *history;
    int32_t* pos;
    double *vel, *fit, *pbest, *rows, *length;
    long long* repeats;
    int32_t* trace_pos;
    double* trace_fit;
};

// PSO.isCollision (pso.py:295-356) of the round()ed samples a -> b over the bit grid: true where an endpoint is
// an obstacle or out of range, else the class's own Bresenham walk, its three branches in its order and its
// termination test (x == x2 on the x-major branch, y == y2 on the other).  e > tau with tau = (d_y - d_x) / 2
// is compared as 2 e against d_y - d_x: the same decision in integers.  A cell outside the grid is in no
// obstacle set.  The walk is bounded by d_x + d_y + 1 steps, which the reference's loop never reaches.
__device__ inline bool pso_collision(const uint32_t* occ, int W, int H, double ax, double ay, double bx, double by)
{
    const double r0 = rint(ax), r1 = rint(ay), r2 = rint(bx), r3 = rint(by);  // Python's round(): half to even
    if (!(r0 >= 0 && r0 < W && r1 >= 0 && r1 < H && r2 >= 0 && r2 < W && r3 >= 0 && r3 < H)) return true;
    const int x1 = (int)r0, y1 = (int)r1, x2 = (int)r2, y2 = (int)r3;
    if (grid2d::occ_bit(occ, H, x1, y1) || grid2d::occ_bit(occ, H, x2, y2)) return true;
    const int dx = abs(x2 - x1), dy = abs(y2 - y1);
    const int sx = x2 > x1 ? 1 : (x2 < x1 ? -1 : 0), sy = y2 > y1 ? 1 : (y2 < y1 ? -1 : 0);
    const bool xmaj = dx > dy;
    const int tau2 = xmaj ? dy - dx : dx - dy;
    int x = x1, y = y1, e = 0;
    for (int it = 0; it < dx + dy + 1; it++) {
        if (xmaj ? x == x2 : y == y2) return false;
        if (2 * e > tau2) {
            if (xmaj) { x += sx; e -= dy; } else { y += sy; e -= dx; }
        } else if (2 * e < tau2) {
            if (xmaj) { y += sy; e += dx; } else { x += sx; e += dy; }
        } else {
            x += sx;
            y += sy;
            e += xmaj ? dx - dy : dy - dx;
        }
        if (x >= 0 && x < W && y >= 0 && y < H && grid2d::occ_bit(occ, H, x, y)) return true;
    }
    return false;
}

// calFitnessValue (pso.py:186-212) of the pn points at pos by one wave on its B-spline state bsm: every lane
// returns the fitness, inf where the reference's run() raises (fewer than k + 1 points after the
// de-duplication, or a singular collocation matrix).  rows [kSamples][2] (nullable) and *len receive the curve.
__device__ __noinline__ double pso_fitness(double* bsm, const int* pos, int pn, int sx, int sy, int gx, int gy, const uint32_t* occ,
                              int W, int H, double* rows, double* len, int lane)
{
    bs_cfg C;
    C.k = kDeg;
    C.dim = 2;
    C.nm = pn + 2;
    C.param_mode = PMP_BSPLINE_CENTRIPETAL;
    C.approx = false;
    C.three_d = false;
    const bs_layout L(pn + 2, kDeg);
    double *D = bsm + L.D, *par = bsm + L.par, *knot = bsm + L.knot, *band = bsm + L.band, *seg = bsm + L.seg;
    double* stage = bsm + L.stage;
    // [start] + position + [goal], first occurrences kept (sorted(set(points), key=points.index))
    const int tot = pn + 2;
    int x = 0, y = 0;
    if (lane == 0) {
        x = sx;
        y = sy;
    } else if (lane <= pn) {
        x = pos[2 * (lane - 1)];
        y = pos[2 * (lane - 1) + 1];
    } else if (lane == pn + 1) {
        x = gx;
        y = gy;
    }
    bool dup = false;
    for (int i = 0; i < tot; i++) {
        const int xi = __shfl(x, i), yi = __shfl(y, i);
        if (i < lane && xi == x && yi == y) dup = true;
    }
    const bool keep = lane < tot && !dup;
    const uint64_t mask = ballot(keep);
    const int n = __popcll(mask);
    BS_SYNC();  // the evaluation before this one has read its D
    if (keep) {
        const int idx = __popcll(mask & ((1ull << lane) - 1ull));
        D[idx * 2] = (double)x;
        D[idx * 2 + 1] = (double)y;
    }
    BS_SYNC();
    *len = qnan();
    if (n < kDeg + 1) return kInf;
    bs_params(C, D, n, par, seg, lane);
    bs_knots(C, par, n, knot, lane);
    if (bs_poisoned(par, knot, n, kDeg, lane)) return kInf;  // distinct points: never
    if (bs_interpolate(C, D, n, par, knot, band, lane)) return kInf;
    int hits = 0;
    const double length = bs_rows(C, knot, D, n, kSamples, false, stage, rows, lane,
                                  [&](bool has, const double* p, const double* prev) {
                                      if (has && pso_collision(occ, W, H, prev[0], prev[1], p[0], p[1])) hits++;
                                  });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o);
    *len = length;
    return 100000.0 / (length + (double)(50000 * hits));
}

__global__ __launch_bounds__(64 * kMaxWaves) void pso_kernel(pmp_pso_params P, int waves, int n_plans, pso_io io)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smb[];
    const int q = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = lane_id(), wave = tid >> 6;
    if (q >= n_plans) return;
    const int np = P.n_particles, pn = P.point_num, W = P.x_range, H = P.y_range, pp = pn * 2;
    const pso_layout L(np, pn, waves);
    double* hd = (double*)(smb + L.hd);
    int* ihd = (int*)(hd + 1);
    double *vel = (double*)(smb + L.vel), *cvel = (double*)(smb + L.cvel), *fit = (double*)(smb + L.fit);
    double *best = (double*)(smb + L.best), *cfit = (double*)(smb + L.cfit);
    double* bsm = (double*)(smb + L.bs) + (size_t)wave * L.bs_doubles;
    int *pos = (int*)(smb + L.pos), *cpos = (int*)(smb + L.cpos), *gpos = (int*)(smb + L.gpos);
    const int sx = io.start[2 * q], sy = io.start[2 * q + 1], gx = io.goal[2 * q], gy = io.goal[2 * q + 1];
    const int32_t* init = io.init + (size_t)q * np * pp;
    const double* rnd = io.rnd + (size_t)q * io.rnd_stride;
    double* hist = io.history + (size_t)q * P.max_iter;
    double dummy;

    if (tid == 0) {
        ihd[0] = 0;
        ihd[1] = 0;
    }
    __syncthreads();
    bool bad = false;
    for (int i = tid; i < np * pp; i += nt) {
        const int v = init[i];
        bad = bad || v < 0 || v >= ((i & 1) ? H : W);
        pos[i] = v;
        vel[i] = 0.0;
    }
    if (bad) atomicOr(&ihd[1], 1);
    __syncthreads();
    if (ihd[1]) {  // the entry refuses such a launch; a position that changed since is not run
        if (tid == 0) {
            io.status[q] = PMP_REF_RAISES;
            io.best_fit[q] = qnan();
            io.length[q] = qnan();
            io.repeats[q] = 0;
        }
        return;
    }
    // the initial fitness of every particle, then plan()'s scan for the first best (pso.py:92-107)
    for (int p = wave; p < np; p += waves) {
        const double f = pso_fitness(bsm, pos + (size_t)p * pp, pn, sx, sy, gx, gy, io.occ, W, H, nullptr, &dummy, lane);
        if (lane == 0) {
            fit[p] = f;
            best[p] = f;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int b = 0;
        for (int p = 1; p < np; p++)
            if (fit[p] > fit[b]) b = p;
        hd[0] = fit[b];
        ihd[2] = b;
    }
    __syncthreads();
    for (int i = tid; i < pp; i += nt) gpos[i] = pos[(size_t)ihd[2] * pp + i];
    __syncthreads();

    const double scale_x = W > H ? (double)W / (double)H : 1.0, scale_y = W > H ? 1.0 : (double)H / (double)W;
    const double vhi = P.max_speed, vlo = 0.0 - P.max_speed;  // -max_speed of an int: no negative zero
    long long repeats = 0;
    for (int it = 0; it < P.max_iter; it++) {
        int first = 0;
        while (first < np) {
            for (int p = first + wave; p < np; p += waves) {
                const int* sp = pos + (size_t)p * pp;
                const double* sv = vel + (size_t)p * pp;
                int* cp = cpos + (size_t)p * pp;
                double* cv = cvel + (size_t)p * pp;
                int nx = 0, ny = 0;
                if (lane < pn) {  // updateParticleVelocity / updateParticlePosition of point `lane`
                    const double* d = rnd + (((size_t)it * np + p) * pn + lane) * 2;
                    const double rand1 = d[0], rand2 = d[1];
                    const int px = sp[2 * lane], py = sp[2 * lane + 1];
                    double vx = P.w_inertial * sv[2 * lane] + P.w_cognitive * rand1 * 0.0 +
                                P.w_social * rand2 * (double)(gpos[2 * lane] - px);
                    double vy = P.w_inertial * sv[2 * lane + 1] + P.w_cognitive * rand1 * 0.0 +
                                P.w_social * rand2 * (double)(gpos[2 * lane + 1] - py);
                    if (W > H) vx *= scale_x;
                    else vy *= scale_y;
                    if (vx < vlo) vx = vlo;
                    if (vx > vhi) vx = vhi;
                    if (vy < vlo) vy = vlo;
                    if (vy > vhi) vy = vhi;
                    cv[2 * lane] = vx;
                    cv[2 * lane + 1] = vy;
                    double fx = (double)px + trunc(vx), fy = (double)py + trunc(vy);  // int(): towards zero
                    if (fx < 0.0) fx = 0.0;
                    if (fx > (double)(W - 1)) fx = (double)(W - 1);
                    if (fy < 0.0) fy = 0.0;
                    if (fy > (double)(H - 1)) fy = (double)(H - 1);
                    nx = (int)fx;
                    ny = (int)fy;
                }
                // position.sort(key=x): stable, by x only; the velocities keep their index
                int rank = 0;
                for (int j = 0; j < pn; j++) {
                    const int xj = __shfl(nx, j);
                    if (xj < nx || (xj == nx && j < lane)) rank++;
                }
                if (lane < pn) {
                    cp[2 * rank] = nx;
                    cp[2 * rank + 1] = ny;
                }
                BS_SYNC();
                const double f = pso_fitness(bsm, cp, pn, sx, sy, gx, gy, io.occ, W, H, nullptr, &dummy, lane);
                if (lane == 0) cfit[p] = f;
            }
            __syncthreads();
            // the first particle, in index order, whose new best fitness beats the global best
            if (wave == 0) {
                int hit = np;
                const double gf = hd[0];
                for (int base = first; base < np && hit == np; base += 64) {
                    const int p = base + lane;
                    bool b = false;
                    if (p < np) {
                        const double f = cfit[p], nb = f > best[p] ? f : best[p];
                        b = nb > gf;
                    }
                    const uint64_t m = ballot(b);
                    if (m) hit = base + __builtin_ctzll(m);
                }
                if (lane == 0) ihd[0] = hit;
            }
            __syncthreads();
            const int hit = ihd[0], last = hit < np ? hit : np - 1;
            for (int i = first * pp + tid; i < (last + 1) * pp; i += nt) {
                pos[i] = cpos[i];
                vel[i] = cvel[i];
            }
            for (int p = first + tid; p <= last; p += nt) {
                const double f = cfit[p];
                fit[p] = f;
                if (f > best[p]) best[p] = f;
                if (p == hit) hd[0] = best[p];
            }
            if (hit < np) {
                for (int i = tid; i < pp; i += nt) gpos[i] = cpos[(size_t)hit * pp + i];
                repeats += np - 1 - hit;
            }
            first = last + 1;
            __syncthreads();
        }
        if (tid == 0) hist[it] = hd[0];
        if (io.trace_pos) {
            int32_t* tp = io.trace_pos + ((size_t)q * P.max_iter + it) * np * pp;
            double* tf = io.trace_fit + ((size_t)q * P.max_iter + it) * np;
            for (int i = tid; i < np * pp; i += nt) tp[i] = pos[i];
            for (int i = tid; i < np; i += nt) tf[i] = fit[i];
        }
    }
    for (int i = tid; i < np * pp; i += nt) {
        io.pos[(size_t)q * np * pp + i] = pos[i];
        io.vel[(size_t)q * np * pp + i] = vel[i];
    }
    for (int i = tid; i < np; i += nt) {
        io.fit[(size_t)q * np + i] = fit[i];
        io.pbest[(size_t)q * np + i] = best[i];
    }
    for (int i = tid; i < pp; i += nt) io.best_pos[(size_t)q * pp + i] = gpos[i];
    const double gf = hd[0];
    if (tid == 0) {
        io.best_fit[q] = gf;
        io.status[q] = gf < kInf ? PMP_FOUND : PMP_REF_RAISES;
        io.repeats[q] = repeats;
    }
    // the best particle's curve (pso.py:119-123); where its fitness is inf the reference raises here
    if (wave == 0) {
        double* rows = io.rows + (size_t)q * kSamples * 2;
        double len;
        const double f = pso_fitness(bsm, gpos, pn, sx, sy, gx, gy, io.occ, W, H, rows, &len, lane);
        if (!(f < kInf))
            for (int i = lane; i < kSamples * 2; i += 64) rows[i] = qnan();
        if (lane == 0) io.length[q] = len;
    }
}

}  // namespace

extern "C" int pmp_pso_default_waves(void) { return kDefaultWaves; }

extern "C" int pmp_pso_batch(pmp_ctx* ctx, void* stream, const pmp_pso_params* prm, const uint32_t* occ_bits, int n_plans,
                             const int32_t* start, const int32_t* goal, const int32_t* init_positions,
                             const int32_t* init_bounds, const double* rnd, int64_t rnd_stride, int32_t* status,
                             int32_t* best_position, double* best_fitness, double* fitness_history, int32_t* positions,
                             double* velocities, double* fitness, double* particle_best_fitness, double* points,
                             double* length, int64_t* repeats, int32_t* trace_positions, double* trace_fitness)
{
    const std::string fn = "pmp_pso_batch";
    if (!ctx) return PMP_EINVAL;
    if (!prm) return pmp_set_err(ctx, PMP_EINVAL, fn + ": null params");
    if (prm->x_range < 1 || prm->y_range < 1) return pmp_set_err(ctx, PMP_EINVAL, fn + ": bad x_range / y_range");
    if (prm->n_particles < 1) return pmp_set_err(ctx, PMP_EINVAL, fn + ": n_particles must be >= 1");
    if (prm->point_num < 1 || prm->point_num > kMaxPoints)
        return pmp_set_err(ctx, PMP_EINVAL, fn + ": point_num must be 1..62 (a curve has at most 64 waypoints)");
    if (prm->max_iter < 0) return pmp_set_err(ctx, PMP_EINVAL, fn + ": max_iter must be >= 0");
    if (!std::isfinite(prm->w_inertial) || !std::isfinite(prm->w_cognitive) || !std::isfinite(prm->w_social))
        return pmp_set_err(ctx, PMP_EINVAL, fn + ": the weights must be finite");
    if (!(prm->max_speed >= 0)) return pmp_set_err(ctx, PMP_EINVAL, fn + ": max_speed must be >= 0");
    if (prm->waves < 0 || prm->waves > kMaxWaves) return pmp_set_err(ctx, PMP_EINVAL, fn + ": waves must be 0 (default) .. 16");
    if (n_plans < 0) return pmp_set_err(ctx, PMP_EINVAL, fn + ": bad n_plans");
    if (n_plans == 0) return PMP_OK;
    const int64_t draws = 2ll * prm->point_num * prm->n_particles * prm->max_iter;
    if ((int64_t)prm->n_particles * prm->point_num > (1 << 24) || draws < 0)
        return pmp_set_err(ctx, PMP_EINVAL, fn + ": the swarm does not fit the workgroup's LDS");
    if (rnd_stride < draws)
        return pmp_set_err(ctx, PMP_EINVAL, fn + ": the stream is shorter than 2 point_num n_particles max_iter draws");
    if (!occ_bits || !start || !goal || !init_positions || !init_bounds || (!rnd && draws > 0) || !status || !best_position ||
        !best_fitness || (!fitness_history && prm->max_iter > 0) || !positions || !velocities || !fitness ||
        !particle_best_fitness || !points || !length || !repeats || (!trace_positions != !trace_fitness))
        return pmp_set_err(ctx, PMP_EINVAL, fn + ": null pointer argument");
    if (init_bounds[0] < 0 || init_bounds[1] < 0 || init_bounds[2] >= prm->x_range || init_bounds[3] >= prm->y_range)
        return pmp_set_err(ctx, PMP_EINVAL, fn + ": an initial position lies outside the grid");
    // the default: kDefaultWaves, no more than there are particles, and as many as the LDS holds beside the swarm
    int waves = prm->waves ? prm->waves : (prm->n_particles < kDefaultWaves ? prm->n_particles : kDefaultWaves);
    while (!prm->waves && waves > 1 && pso_layout(prm->n_particles, prm->point_num, waves).bytes > kLdsBytes) waves--;
    const pso_layout L(prm->n_particles, prm->point_num, waves);
    if (L.bytes > kLdsBytes)
        return pmp_set_err(ctx, PMP_EINVAL, fn + ": the swarm does not fit the workgroup's LDS (" + std::to_string(L.bytes) +
                                                " of " + std::to_string(kLdsBytes) + " bytes; fewer waves leave more)");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    pso_io io;
    io.occ = occ_bits;
    io.start = start;
    io.goal = goal;
    io.init = init_positions;
    io.rnd = rnd;
    io.rnd_stride = rnd_stride;
    io.status = status;
    io.best_pos = best_position;
    io.best_fit = best_fitness;
    io.history = fitness_history;
    io.pos = positions;
    io.vel = velocities;
    io.fit = fitness;
    io.pbest = particle_best_fitness;
    io.rows = points;
    io.length = length;
    io.repeats = (long long*)repeats;
    io.trace_pos = trace_positions;
    io.trace_fit = trace_fitness;
    hipLaunchKernelGGL(pso_kernel, dim3(n_plans), dim3(64 * waves), L.bytes, (hipStream_t)stream, *prm, waves, n_plans, io);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}
