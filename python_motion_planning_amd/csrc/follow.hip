// Batched path-following planners for gfx950: whole PID.plan (local_planner/pid.py:55-158), APF.plan
// (apf.py:50-144) and RPP.plan (rpp.py:51-147) iterations.
//
// The loop is track.hip's: four agents per wave64, one per 16-lane DPP row; reachGoal,
// getLookaheadPoint on the row, the rotate-or-move branch, a controller, Robot.kinematic.  An
// agent's scalar work runs on all 16 lanes of its row (same inputs, same result).
//
// Obstacle term (APF.getRepulsiveForce, RPP.applyObstacleConstraint).  The reference takes a cdist
// from the robot to every obstacle cell at every step.  Only cells nearer than d_0 (APF:
// 1/D - 1/d_0 > 0) or scaling_dist (RPP: min D < scaling_dist) can matter, so the row scans the
// window of cells [floor(p - d), ceil(p + d)]^2 of the occupancy bit grid, clipped to the grid's box
// (cells outside it are free), window cell k = ix * ny + iy on lane k % 16, and reduces over the row:
// a minimum for RPP, two sums for APF.  D = sqrt(dx dx + dy dy) as scipy's euclidean cdist (no
// hypot, no fma).  APF's sum runs in that window order (lane partial sums, then a rotation tree), not
// in the reference's list(set) order: the terms are the same, at most a handful per step.
// The scan is entered by the whole wave with the rows that need it flagged (`need`, row-uniform, as
// mpc_rows): the other rows get an empty window and keep their lanes converged through it.
#include "localplan.h"
#include "rowlane.h"

namespace {

constexpr int kWave = 64;
constexpr int kRows = 4;  // agents per wave

// numpy.linalg.norm of a 2-vector: sqrt(x.dot(x)), the dot product's second term fused by the BLAS kernel
__device__ __forceinline__ double norm2(double x, double y) { return sqrt(fma(y, y, x * x)); }

struct ObsTerm {
    double dmin;    // min D over the window's obstacle cells (inf: none)
    double sx, sy;  // APF: sum of (1/D - 1/d_0) (1/D)^2 (p - cell) over cells with 1/D - 1/d_0 > 0
};

// The obstacle scan for the agents of the wave's four rows, called by the whole wave; `need`
// (row-uniform) selects the rows whose agent uses it now.
template <bool APF>
__device__ __forceinline__ ObsTerm obstacle_rows(bool need, const uint32_t* __restrict__ occ, int ox, int oy, int W,
                                                 int H, double px, double py, double d, double inv_d0)
{
    const int v = lane_id() & 15;
    int x0 = 0, y0 = 0, nx = 0, ny = 0;
    if (need) {
        // clip in double before the conversion (a huge d, or a NaN position, stays inside the box)
        const double bx0 = (double)ox, bx1 = (double)ox + (double)(W - 1);
        const double by0 = (double)oy, by1 = (double)oy + (double)(H - 1);
        const double fx0 = fmax(floor(px - d), bx0), fx1 = fmin(ceil(px + d), bx1);
        const double fy0 = fmax(floor(py - d), by0), fy1 = fmin(ceil(py + d), by1);
        if (fx0 <= fx1 && fy0 <= fy1) {
            x0 = (int)fx0;
            y0 = (int)fy0;
            nx = (int)fx1 - x0 + 1;
            ny = (int)fy1 - y0 + 1;
        }
    }
    const int n = nx * ny;
    ObsTerm T;
    T.dmin = INFINITY;
    T.sx = T.sy = 0.0;
#pragma unroll 1
    for (int k = v; k < n; k += 16) {
        const int ix = k / ny, iy = k - ix * ny;
        const int cx = x0 + ix, cy = y0 + iy;
        const uint32_t c = (uint32_t)(cx - ox) * (uint32_t)H + (uint32_t)(cy - oy);  // inside the box by the clip
        if (!((occ[c >> 5] >> (c & 31u)) & 1u)) continue;
        const double dx = (double)cx - px, dy = (double)cy - py;
        const double D = sqrt(dx * dx + dy * dy);
        if (APF) {
            const double iD = 1.0 / D;
            const double g = iD - inv_d0;
            if (g > 0) {
                const double c2 = g * (iD * iD);
                T.sx += c2 * (px - (double)cx);
                T.sy += c2 * (py - (double)cy);
            }
        } else {
            T.dmin = fmin(T.dmin, D);
        }
    }
    if (APF) {
        T.sx = sum16(T.sx);
        T.sy = sum16(T.sy);
    } else {
        T.dmin = min16(T.dmin);
    }
    return T;
}

// `iters` iterations of PID.plan / APF.plan / RPP.plan for agent 4 * block + row.  Control flow is
// per row; the obstacle scan is entered by the whole wave with the rows that use it flagged.
template <int KIND>
__global__ __launch_bounds__(kWave) void follow_kernel(const uint32_t* __restrict__ occ, int ox, int oy, int W, int H,
                                                       pmp_lp_params P, pmp_follow_params F, int na,
                                                       double* __restrict__ state, double* __restrict__ pid_state,
                                                       const double* __restrict__ goal,
                                                       const double* __restrict__ path_xy,
                                                       const int32_t* __restrict__ path_off, int iters,
                                                       double* __restrict__ u_out, int32_t* __restrict__ status_out,
                                                       int32_t* __restrict__ nsteps_out, double* __restrict__ hist_pose,
                                                       double* __restrict__ hist_look)
{
    const int v = threadIdx.x & 15;
    const int ai = blockIdx.x * kRows + (threadIdx.x >> 4);
    const bool valid = ai < na;
    const int a = valid ? ai : na - 1;  // rows past the batch read a real agent and write nothing
    const double* path = path_xy + 2 * (size_t)path_off[a];
    const int Pn = path_off[a + 1] - path_off[a];
    const double gl[3] = {goal[3 * a], goal[3 * a + 1], goal[3 * a + 2]};
    double st[5];
    for (int k = 0; k < 5; k++) st[k] = state[5 * a + k];
    double e_v = 0.0, i_v = 0.0, e_w = 0.0, i_w = 0.0;  // PID integrators (pid.py:40-41)
    if (KIND == PMP_FOLLOW_PID) {
        e_v = pid_state[4 * a]; i_v = pid_state[4 * a + 1];
        e_w = pid_state[4 * a + 2]; i_w = pid_state[4 * a + 3];
    }
    const double dt = P.dt;
    const double inv_d0 = 1.0 / F.d_0;
    int status = 0, steps = 0;
    bool live = valid;  // row-uniform: the agent still iterates
    double u0 = st[3], u1 = st[4];
    for (int it = 0; it < iters; it++) {
        if (!ballot(live)) break;
        // base-class regularisers (local_planner.py:172-206)
#define LINREG(vd) lp::clampd(st[3] + lp::clampd((vd) - st[3], P.min_v_inc, P.max_v_inc), P.min_v, P.max_v)
#define ANGREG(wd) lp::clampd(st[4] + lp::clampd((wd) - st[4], P.min_w_inc, P.max_w_inc), P.min_w, P.max_w)
        bool need = false;  // the row's agent uses the obstacle term in this iteration
        double pt[2] = {0, 0}, lookahead_k = 0.0;
        if (live) {
            double theta_trj = 0, kappa = 0;
            if (lp::reach_goal(st, gl, P)) {
                status = PMP_FOUND + 1;
                live = false;
            } else if (lookahead_row(path, Pn, st[0], st[1], st[3], P, pt, &theta_trj, &kappa)) {
                status = PMP_REF_RAISES;
                live = false;
            } else if (KIND == PMP_FOLLOW_APF) {
                need = true;  // getRepulsiveForce precedes the branch (apf.py:66)
            } else {
                // PID's own (pid.py:114-158); the integrators move only where the reference calls them
                auto pid_lin = [&](double v_d) {
                    const double e = v_d - st[3];
                    i_v += e * dt;
                    const double d_v = (e - e_v) / dt;
                    e_v = e;
                    const double inc = lp::clampd(F.k_v_p * e + F.k_v_i * i_v + F.k_v_d * d_v, P.min_v_inc, P.max_v_inc);
                    return lp::clampd(st[3] + inc, P.min_v, P.max_v);
                };
                auto pid_ang = [&](double w_d) {
                    const double e = w_d - st[4];
                    i_w += e * dt;
                    const double d_w = (e - e_w) / dt;
                    e_w = e;
                    const double inc = lp::clampd(F.k_w_p * e + F.k_w_i * i_w + F.k_w_d * d_w, P.min_w_inc, P.max_w_inc);
                    return lp::clampd(st[4] + inc, P.min_w, P.max_w);
                };
                const double ang = atan2(pt[1] - st[1], pt[0] - st[0]);  // angle(robot.position, lookahead_pt)
                double theta_d = ang;
                if (KIND == PMP_FOLLOW_PID) {  // pid.py:73-79
                    double theta_err = ang;
                    if (fabs(theta_err - theta_trj) > lp::kPi) {
                        if (theta_err > theta_trj) theta_trj += 2 * lp::kPi;
                        else theta_err += 2 * lp::kPi;
                    }
                    theta_d = F.k_theta * theta_err + (1 - F.k_theta) * theta_trj;
                } else {  // rpp.py:71-73
                    lookahead_k = 2 * sin(ang - st[2]) / lp::lookahead_dist(st[3], P);
                }
                double e_theta = lp::regularize_angle(st[2] - gl[2]);
                if (!(lp::py_hypot(gl[0] - st[0], gl[1] - st[1]) > P.goal_dist_tol)) {
                    u0 = 0.0;
                    if (!(fabs(e_theta) > P.rotate_tol)) u1 = 0.0;
                    else u1 = KIND == PMP_FOLLOW_PID ? pid_ang(e_theta / dt) : ANGREG(e_theta / dt);
                } else {
                    e_theta = lp::regularize_angle(theta_d - st[2]);
                    if (fabs(e_theta) > P.rotate_tol) {
                        u0 = 0.0;
                        u1 = KIND == PMP_FOLLOW_PID ? pid_ang(e_theta / dt) : ANGREG(e_theta / dt);
                    } else if (KIND == PMP_FOLLOW_PID) {
                        const double v_d = lp::py_hypot(st[0] - pt[0], st[1] - pt[1]) / dt;
                        u0 = pid_lin(v_d);
                        u1 = pid_ang(e_theta / dt);
                    } else if (lookahead_k == 0.0) {
                        status = PMP_REF_RAISES;  // 1.0 / curvature (rpp.py:125): ZeroDivisionError
                        live = false;
                    } else {
                        need = true;
                    }
                }
            }
        }
        if (KIND != PMP_FOLLOW_PID) {
            if (ballot(need)) {
                const ObsTerm T = obstacle_rows<KIND == PMP_FOLLOW_APF>(
                    need, occ, ox, oy, W, H, st[0], st[1], KIND == PMP_FOLLOW_APF ? F.d_0 : F.scaling_dist, inv_d0);
                if (need && KIND == PMP_FOLLOW_APF) {
                    // forces (apf.py:110-144) and the desired velocity (apf.py:71-75)
                    double rx = T.sx, ry = T.sy;
                    if (!(rx == 0.0 && ry == 0.0)) {
                        const double n = norm2(rx, ry);
                        rx = rx / n;
                        ry = ry / n;
                    }
                    double ax = pt[0] - st[0], ay = pt[1] - st[1];
                    if (!(ax == 0.0 && ay == 0.0)) {
                        const double n = norm2(ax, ay);
                        ax = ax / n;
                        ay = ay / n;
                    }
                    const double fx = F.zeta * ax + F.eta * rx, fy = F.zeta * ay + F.eta * ry;
                    double sn, cs;
                    sincos(st[2], &sn, &cs);
                    double nvx = st[3] * cs + fx, nvy = st[3] * sn + fy;
                    const double n = norm2(nvx, nvy);
                    nvx = nvx / n * P.max_v;
                    nvy = nvy / n * P.max_v;
                    const double theta_d = atan2(nvy, nvx);
                    double e_theta = lp::regularize_angle(st[2] - gl[2]);
                    if (!(lp::py_hypot(gl[0] - st[0], gl[1] - st[1]) > P.goal_dist_tol)) {
                        u0 = 0.0;
                        u1 = fabs(e_theta) > P.rotate_tol ? ANGREG(e_theta / dt) : 0.0;
                    } else {
                        e_theta = lp::regularize_angle(theta_d - st[2]);
                        if (fabs(e_theta) > P.rotate_tol) {
                            u0 = 0.0;
                            u1 = ANGREG(e_theta / dt);
                        } else {
                            u0 = LINREG(norm2(nvx, nvy));
                            u1 = ANGREG(e_theta / dt);
                        }
                    }
                }
                if (need && KIND == PMP_FOLLOW_RPP) {
                    // applyCurvatureConstraint / applyObstacleConstraint (rpp.py:114-147)
                    const double radius = fabs(1.0 / lookahead_k);
                    const double curv_vel = radius < F.regulated_radius_min ? P.max_v * (radius / F.regulated_radius_min) : P.max_v;
                    const double cost_vel = T.dmin < F.scaling_dist ? P.max_v * F.scaling_gain * T.dmin / F.scaling_dist : P.max_v;
                    const double v_d = cost_vel < curv_vel ? cost_vel : curv_vel;  // min(curv_vel, cost_vel)
                    u0 = LINREG(v_d);
                    u1 = ANGREG(v_d * lookahead_k);
                }
            }
        }
#undef LINREG
#undef ANGREG
        if (live) {
            if (v == 0 && hist_pose) {
                double* hp = hist_pose + ((size_t)a * iters + it) * 3;
                hp[0] = st[0]; hp[1] = st[1]; hp[2] = st[2];
            }
            if (v == 0 && hist_look) {  // lookahead_pts.append(lookahead_pt) (rpp.py:94)
                double* hl = hist_look + ((size_t)a * iters + it) * 2;
                hl[0] = pt[0]; hl[1] = pt[1];
            }
            // Robot.kinematic -> lookforward (agent.py:68-116)
            double sn, cs;
            sincos(st[2], &sn, &cs);
            const double nx = st[0] + (dt * cs) * u0, ny = st[1] + (dt * sn) * u0, nth = st[2] + dt * u1;
            st[0] = nx; st[1] = ny; st[2] = nth; st[3] = u0; st[4] = u1;
            steps++;
        }
    }
    if (valid && v == 0) {
        for (int k = 0; k < 5; k++) state[5 * a + k] = st[k];
        if (KIND == PMP_FOLLOW_PID) {
            pid_state[4 * a] = e_v; pid_state[4 * a + 1] = i_v;
            pid_state[4 * a + 2] = e_w; pid_state[4 * a + 3] = i_w;
        }
        u_out[2 * a] = u0;
        u_out[2 * a + 1] = u1;
        status_out[a] = status;
        nsteps_out[a] = steps;
    }
}

}  // namespace

extern "C" int pmp_follow_step_batch(pmp_ctx* ctx, void* stream, int kind, const uint32_t* occ_bits, int ox, int oy,
                                     int W, int H, const pmp_lp_params* lp, const pmp_follow_params* fp, int na,
                                     double* state, double* pid_state, const double* goal, const double* path_xy,
                                     const int32_t* path_off, int iters, double* u, int32_t* status, int32_t* n_steps,
                                     double* hist_pose, double* hist_lookahead)
{
    if (!ctx) return PMP_EINVAL;
    if (!lp || !fp || na < 0 || iters < 1 ||
        (kind != PMP_FOLLOW_PID && kind != PMP_FOLLOW_APF && kind != PMP_FOLLOW_RPP))
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_follow_step_batch: bad kind/params/na/iters");
    if (kind == PMP_FOLLOW_PID && !pid_state)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_follow_step_batch: PID needs pid_state");
    if (kind != PMP_FOLLOW_PID) {
        if (!occ_bits || W < 1 || H < 1 || W > 8192 || H > 8192)
            return pmp_set_err(ctx, PMP_EINVAL, "pmp_follow_step_batch: APF / RPP need occ_bits with 1 <= W, H <= 8192");
        if (kind == PMP_FOLLOW_APF && !(fp->d_0 > 0))
            return pmp_set_err(ctx, PMP_EINVAL, "pmp_follow_step_batch: d_0 must be > 0");
        if (kind == PMP_FOLLOW_RPP && !(fp->scaling_dist >= 0))
            return pmp_set_err(ctx, PMP_EINVAL, "pmp_follow_step_batch: scaling_dist must be >= 0");
    }
    if (na == 0) return PMP_OK;
    if (!state || !goal || !path_xy || !path_off || !u || !status || !n_steps)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_follow_step_batch: null pointer argument");
    if (!(lp->dt > 0)) return pmp_set_err(ctx, PMP_EINVAL, "pmp_follow_step_batch: dt must be > 0");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const dim3 grid((na + kRows - 1) / kRows);
    hipStream_t s = (hipStream_t)stream;
#define PMP_FOLLOW_LAUNCH(K)                                                                                      \
    hipLaunchKernelGGL(follow_kernel<K>, grid, dim3(kWave), 0, s, occ_bits, ox, oy, W, H, *lp, *fp, na, state,    \
                       pid_state, goal, path_xy, path_off, iters, u, status, n_steps, hist_pose, hist_lookahead)
    if (kind == PMP_FOLLOW_PID) PMP_FOLLOW_LAUNCH(PMP_FOLLOW_PID);
    else if (kind == PMP_FOLLOW_APF) PMP_FOLLOW_LAUNCH(PMP_FOLLOW_APF);
    else PMP_FOLLOW_LAUNCH(PMP_FOLLOW_RPP);
#undef PMP_FOLLOW_LAUNCH
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}
