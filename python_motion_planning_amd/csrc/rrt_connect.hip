// Batched RRT-Connect for gfx950 (global_planner/sample_search/rrt_connect.py:42-147 over rrt.py:92-130
// and sample_search.py:27-135): one 64-lane wave per query, kQW queries per workgroup.  A plan is a few
// hundred nodes and under a thousand collision tests -- many tiny sequential searches, so the batch
// fills the device and a query needs no workgroup barrier: after the obstacle load the waves of a
// workgroup never meet again.
//
// Tree 0 is rooted at the start, tree 1 at the goal; `fw` names the one that is sample_list_f.  Per
// iteration (all decisions wave-uniform, results identical to the reference's sequential loop):
//  1. sample from the query's np.random stream (generateRandomNode, rrt.py:92-103: one draw for the
//     goal, else three; no `in sample_list` skip in rrt_connect.py);
//  2. nearest node of the forward tree = first argmin of the exact CPython hypot (rrt.py:117-118): a
//     plain f64 pass, the nodes spread over the lanes, and a wave lexicographic (value, index) minimum;
//  3. steer (hypot, atan2, min(max_dist, d), cos, sin, g = g_near + d) and isCollision(new, near), the
//     obstacle items spread over the lanes (coll_item: rrt.hip's item set and operation order);
//  4. insert.  A sample at distance exactly 0 from its nearest node (the goal sampled while the
//     goal-rooted tree is forward) steers to that node's own key: the dict entry is replaced in place,
//     its parent its own coordinates, g + 0.0.  A steered node landing exactly on another existing key
//     (probability ~2^-50 per insert) is appended instead of replacing it, as plain RRT does;
//  5. the same nearest / steer / test from the backward tree towards node_new (rrt_connect.py:64), then
//     the greedy extension (rrt_connect.py:69-85): equal coordinates end the plan, else one steered
//     step of min(max_dist, dist) towards node_new is appended on a free segment; a collision breaks;
//  6. the trees swap roles when len(b) < len(f) (rrt_connect.py:87), every iteration;
//  7. on equality: cost = the meeting node's g in both trees, the path start -> meeting node -> goal
//     (extractPath, rrt_connect.py:92-126).
// Every loop is bounded: inserts and the greedy loop by the tree capacity, the parent walks by the
// tree sizes, the path by path_cap.
//
// Each tree's first kLdsNodes nodes (x, y, g) sit in LDS beside the HBM arrays that are the output;
// the scan reads the rest from HBM.  Parents are only read by the final walk and live in HBM alone.
#include "localplan.h"
#include "rrt_obstacles.h"  // in_box, inter_rect, inter_circle

namespace {

constexpr int kQW = 4;            // queries (waves) per workgroup
constexpr int kNT = 64 * kQW;
// Nodes of each tree kept in LDS: 4 queries x 2 trees x 160 nodes x 24 B = 30,720 B static, so four
// workgroups (16 waves) share a CU's 160 KiB with up to 9.5 KiB of obstacles each; README trees
// (at most 147 nodes each over seeds 0..15) stay inside it.  The registers, not the LDS, set the
// residency: 212 VGPRs (the f64 atan2 / sincos / hypot chain) hold two workgroups per CU, and builds
// forced to 168 or 128 VGPRs spill and are no faster
constexpr int kLdsNodes = 160;
constexpr int kMaxObs = 256;   // per obstacle kind
constexpr int kMaxBnd = 8;

struct RcArgs {
    pmp_rrt_params P;
    const double *rect, *circ, *bnd;
    int nr, nc, nb;
    const double *start, *goal;
    int nq;
    const double* rnd;
    int64_t stride;
    int cap;
    double *txy, *tg;
    int32_t* tpar;
    int32_t *n_nodes, *forward, *boundary;
    double* cost;
    int32_t* path_len;
    double* path;
    int path_cap;
    int32_t* iters;
    int64_t* draws;
    int32_t* status;
    int64_t* counters;  // nullable [nq][4]
};

struct RcShared {
    double x[kQW][2][kLdsNodes], y[kQW][2][kLdsNodes], g[kQW][2][kLdsNodes];
};

// the map's obstacles in the workgroup's dynamic LDS: rects (4 doubles each), circles (3), boundary (4)
struct Obs {
    const double *rect, *circ, *bnd;
    int nr, nc, nb;
    double d;  // inflation
};

}  // namespace
extern __shared__ __attribute__((aligned(16))) unsigned char rc_lds_dyn[];
namespace {

__host__ __device__ inline int obs_bytes(int nr, int nc, int nb) { return ((4 * nr + 3 * nc + 4 * nb) * 8 + 15) & ~15; }

// collision test item `it` of isCollision(p1, p2) -- rrt.hip's coll_item over this kernel's obstacle
// pointers: inside(p1) circles / rects / boundary, inside(p2) ..., rect crossings, circle crossings
// (sample_search.py:27-49), each behind an exact bounding-box rejection (|dx| > r + d already implies
// hypot > r + d; a segment whose bbox misses the inflated rect fails every "rapid repulsion" pair test)
__device__ inline bool coll_item(const Obs& O, int it, double x1, double y1, double x2, double y2)
{
    const int nr = O.nr, nc = O.nc, nb = O.nb;
    const double d = O.d;
    const int per = nc + nr + nb;
    double x = x1, y = y1;
    if (it >= per && it < 2 * per) { it -= per; x = x2; y = y2; }
    if (it < per) {
        if (it < nc) {
            const double* c = &O.circ[3 * it];
            const double rr = c[2] + d;
            if (fabs(x - c[0]) > rr || fabs(y - c[1]) > rr) return false;
            return lp::py_hypot(x - c[0], y - c[1]) <= rr;
        }
        it -= nc;
        if (it < nr) return in_box(&O.rect[4 * it], d, x, y);
        return in_box(&O.bnd[4 * (it - nr)], d, x, y);
    }
    it -= 2 * per;
    const double bx0 = fmin(x1, x2), bx1 = fmax(x1, x2), by0 = fmin(y1, y2), by1 = fmax(y1, y2);
    if (it < nr) {
        const double* r = &O.rect[4 * it];
        if (bx1 < r[0] - d || bx0 > r[0] + r[2] + d || by1 < r[1] - d || by0 > r[1] + r[3] + d) return false;
        return inter_rect(r, d, x1, y1, x2, y2);
    }
    it -= nr;
    const double* c = &O.circ[3 * it];
    // the projected point lies within the segment's bbox (up to rounding): a gap of more than
    // r + d (with slack for the rounding) rules the circle out
    const double rr = (c[2] + d) * (1.0 + 1e-12) + 1e-12;
    if (bx1 < c[0] - rr || bx0 > c[0] + rr || by1 < c[1] - rr || by0 > c[1] + rr) return false;
    return inter_circle(c, d, x1, y1, x2, y2);
}

// one wave's isCollision(p1, p2); wave-uniform result
__device__ bool collision_wave(const Obs& O, double x1, double y1, double x2, double y2)
{
    bool hit = false;
    const int items = 2 * (O.nc + O.nr + O.nb) + O.nr + O.nc;
    for (int it = lane_id(); it < items; it += 64) hit |= coll_item(O, it, x1, y1, x2, y2);
    return ballot(hit) != 0;
}

// lexicographic minimum of (v, i) over the wave: every lane gets it
__device__ __forceinline__ void wave_min_di(double& v, int& i)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

// one tree of one query: nodes 0 .. kLdsNodes-1 in LDS (and in HBM), the rest in HBM only
struct Tree {
    double *lx, *ly, *lg;  // LDS
    double *xy, *g;        // HBM [cap][2], [cap]
    int32_t* par;          // HBM [cap]
};

// Lane 0 writes node `slot` (slot < cap); every lane may read it afterwards.  A node beyond the LDS
// part is read back from HBM by other lanes of this wave: the device-scope fence completes the store
// and drops the lanes' cached line.
__device__ __forceinline__ void node_store(const Tree& T, int slot, double x, double y, double g, int parent)
{
    if (lane_id() == 0) {
        if (slot < kLdsNodes) { T.lx[slot] = x; T.ly[slot] = y; T.lg[slot] = g; }
        T.xy[2 * slot] = x; T.xy[2 * slot + 1] = y; T.g[slot] = g; T.par[slot] = parent;
    }
    if (slot < kLdsNodes) __threadfence_block();
    else __threadfence();
}

// First argmin of hypot(nd - node) over a tree of n nodes (rrt.py:117-118): each lane's nodes in
// increasing j (a strict < keeps its first), then the wave's (value, index) minimum
__device__ __forceinline__ int nearest(const Tree& T, int n, double px, double py)
{
    double best = INFINITY;
    int near = 0x7fffffff;
    const int nl = n < kLdsNodes ? n : kLdsNodes;
    for (int j = lane_id(); j < nl; j += 64) {
        const double e = lp::py_hypot(T.lx[j] - px, T.ly[j] - py);
        if (e < best) { best = e; near = j; }
    }
    for (int j = kLdsNodes + lane_id(); j < n; j += 64) {
        const double e = lp::py_hypot(T.xy[2 * j] - px, T.xy[2 * j + 1] - py);
        if (e < best) { best = e; near = j; }
    }
    wave_min_di(best, near);
    near = uni(near);
    return near < n ? near : 0;  // (no finite distance at all -- NaN inputs: stay inside the tree)
}

__global__ __launch_bounds__(kNT) void rrt_connect_kernel(RcArgs A)
{
    __shared__ RcShared S;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int nr = A.nr, nc = A.nc, nb = A.nb;
    {
        double* ob = (double*)rc_lds_dyn;
        for (int i = tid; i < 4 * nr; i += kNT) ob[i] = A.rect[i];
        for (int i = tid; i < 3 * nc; i += kNT) ob[4 * nr + i] = A.circ[i];
        for (int i = tid; i < 4 * nb; i += kNT) ob[4 * nr + 3 * nc + i] = A.bnd[i];
    }
    __syncthreads();  // the only workgroup barrier: from here on each wave runs its own query
    const int q = blockIdx.x * kQW + w;
    if (q >= A.nq) return;
    const pmp_rrt_params P = A.P;
    Obs O;
    O.rect = (const double*)rc_lds_dyn;
    O.circ = O.rect + 4 * nr;
    O.bnd = O.circ + 3 * nc;
    O.nr = nr; O.nc = nc; O.nb = nb; O.d = P.delta;
    const int cap = A.cap;
    auto tree_of = [&](int t) {
        Tree T;
        T.lx = S.x[w][t]; T.ly = S.y[w][t]; T.lg = S.g[w][t];
        T.xy = A.txy + ((size_t)q * 2 + t) * cap * 2;
        T.g = A.tg + ((size_t)q * 2 + t) * cap;
        T.par = A.tpar + ((size_t)q * 2 + t) * cap;
        return T;
    };
    const double* rnd = A.rnd + (size_t)q * A.stride;
    const double gx = A.goal[2 * q], gy = A.goal[2 * q + 1];
    node_store(tree_of(0), 0, A.start[2 * q], A.start[2 * q + 1], 0.0, 0);
    node_store(tree_of(1), 0, gx, gy, 0.0, 0);
    const double lox = P.delta, rgx = (P.x_range - P.delta) - P.delta;
    const double loy = P.delta, rgy = (P.y_range - P.delta) - P.delta;
    // nF / nB: the node counts of the forward (tree fw) and the backward tree
    int nF = 1, nB = 1, fw = 0, status = PMP_NO_PATH, it = 0;
    int b0 = -1, b1 = -1;
    int64_t cur = 0;
    int64_t c_scan = 0, c_tests = 0, c_greedy = 0;
    while (it < P.sample_num) {
        // ---- 1. sample ----
        if (cur + 3 > A.stride) { status = PMP_CAP_OVERFLOW; break; }
        it++;
        double px = gx, py = gy;  // the point steered towards: the sample, then node_new
        if (rnd[cur++] > P.goal_sample_rate) {
            px = lox + rgx * rnd[cur++];
            py = loy + rgy * rnd[cur++];
        }
        // One copy of nearest / steer / test / insert serves the three places the reference steers
        // from: phase 0 getNearest(sample_list_f, node_rand), phase 1 getNearest(sample_list_b,
        // node_new), phase 2 a greedy step from node_new_b (no scan: the node steered from is known).
        // A collision ends the iteration in every phase (getNearest returns None; the greedy loop
        // breaks).  Every pass of phase 2 appends a node or leaves, so cap + 2 passes bound the loop.
        int phase = 0, slot = -1, bs = -1;
        double bx = 0.0, by = 0.0, bg = 0.0;  // node_new_b
        for (int s = 0; s < cap + 3; s++) {
            const bool back = phase > 0;
            const Tree T = tree_of(back ? fw ^ 1 : fw);
            int n = back ? nB : nF;
            int near = bs;
            double ex = bx, ey = by, eg = bg;
            if (phase < 2) {
                near = nearest(T, n, px, py);
                c_scan += n;
                if (near < kLdsNodes) { ex = T.lx[near]; ey = T.ly[near]; eg = T.lg[near]; }
                else { ex = T.xy[2 * near]; ey = T.xy[2 * near + 1]; eg = T.g[near]; }
            } else {
                if (bx == px && by == py) {  // node_new_b == node_new: Node.__eq__ compares the coordinates
                    status = PMP_FOUND;
                    b0 = fw ? bs : slot;
                    b1 = fw ? slot : bs;
                    break;
                }
                c_greedy++;
            }
            // steer (rrt.py:121-125, rrt_connect.py:75-79); hypot takes its arguments through fabs, so
            // dist(node_new, node_new_b) and dist(node_near, node) are this one expression
            const double d0 = lp::py_hypot(px - ex, py - ey);
            const double theta = atan2(py - ey, px - ex);
            const double d = P.max_dist < d0 ? P.max_dist : d0;
            double st, ct;
            sincos(theta, &st, &ct);  // one range reduction; the same bits as cos / sin (tools/sincos_check.hip)
            const double ox = ex + d * ct, oy = ey + d * st, og = eg + d;
            c_tests++;
            if (collision_wave(O, ox, oy, ex, ey)) break;
            int sl = near;  // d0 == 0: node_new.current is node_near's key, the dict entry is replaced in place
            if (d0 != 0.0) {
                if (n >= cap) { status = PMP_CAP_OVERFLOW; break; }
                sl = n++;
            }
            node_store(T, sl, ox, oy, og, near);
            if (back) nB = n;
            else nF = n;
            if (phase == 0) {
                slot = sl;
                px = ox;
                py = oy;
            } else {
                bs = sl; bx = ox; by = oy; bg = og;
            }
            phase = phase < 2 ? phase + 1 : 2;
        }
        if (status != PMP_NO_PATH) break;
        // ---- 6. the smaller tree becomes the forward one ----
        if (nB < nF) {
            const int t = nF;
            nF = nB;
            nB = t;
            fw ^= 1;
        }
    }
    // ---- 7. extractPath (rrt_connect.py:92-126) ----
    __threadfence();  // lane 0 reads parents and nodes it wrote to HBM
    const int n0 = fw ? nB : nF, n1 = fw ? nF : nB;
    if (lane == 0) {
        const Tree T[2] = {tree_of(0), tree_of(1)};
        double c = 0.0;
        int plen = 0;
        if (status == PMP_FOUND) {
            c = T[0].g[b0] + T[1].g[b1];
            double* out = A.path + (size_t)q * A.path_cap * 2;
            // the start-rooted walk, counted first (at most n0 nodes) and then written root first
            int k0 = 0, v = b0;
            bool reached = false;
            for (int s = 0; s < n0; s++) {
                k0++;
                if (v == 0) { reached = true; break; }
                v = T[0].par[v];
            }
            if (reached) {
                v = b0;
                for (int s = k0 - 1; s >= 0; s--) {
                    if (s < A.path_cap) { out[2 * s] = T[0].xy[2 * v]; out[2 * s + 1] = T[0].xy[2 * v + 1]; }
                    v = T[0].par[v];
                }
                plen = k0;
                // the goal-rooted walk, without the meeting node
                v = b1;
                reached = v == 0;
                for (int s = 0; !reached && s < n1; s++) {
                    v = T[1].par[v];
                    if (plen < A.path_cap) { out[2 * plen] = T[1].xy[2 * v]; out[2 * plen + 1] = T[1].xy[2 * v + 1]; }
                    plen++;
                    reached = v == 0;
                }
            }
            if (!reached) { status = PMP_REF_RAISES; plen = 0; }  // a parent cycle: the reference never returns
            else if (plen > A.path_cap) status = PMP_PATH_OVERFLOW;
        }
        A.n_nodes[2 * q] = n0;
        A.n_nodes[2 * q + 1] = n1;
        A.forward[q] = fw;
        A.boundary[2 * q] = b0;
        A.boundary[2 * q + 1] = b1;
        A.cost[q] = c;
        A.path_len[q] = plen;
        A.iters[q] = it;
        A.draws[q] = cur;
        A.status[q] = status;
        if (A.counters) {
            A.counters[4 * q] = it;
            A.counters[4 * q + 1] = c_scan;
            A.counters[4 * q + 2] = c_tests;
            A.counters[4 * q + 3] = c_greedy;
        }
    }
}

}  // namespace

extern "C" int pmp_rrt_connect_lds_nodes(void) { return kLdsNodes; }

extern "C" int pmp_rrt_connect_batch(pmp_ctx* ctx, void* stream, const pmp_rrt_params* p, const double* rect, int nr,
                                     const double* circ, int nc, const double* bnd, int nb, const double* start_xy,
                                     const double* goal_xy, int nq, const double* rnd, int64_t rnd_stride, int tree_cap,
                                     double* tree_xy, double* tree_g, int32_t* tree_parent, int32_t* n_nodes,
                                     int32_t* forward, int32_t* boundary, double* cost, int32_t* path_len,
                                     double* path_xy, int path_cap, int32_t* iters, int64_t* draws, int32_t* status,
                                     int64_t* counters)
{
    if (!ctx) return PMP_EINVAL;
    if (!p || nq < 0 || nr < 0 || nc < 0 || nb < 0 || nr > kMaxObs || nc > kMaxObs || nb > kMaxBnd)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_rrt_connect_batch: bad params or obstacle counts (<= 256 rects, 256 circles, 8 boundary)");
    if (p->sample_num < 0 || tree_cap < 2 || tree_cap > (1 << 28) || rnd_stride < 1 || path_cap < 0 || !(p->delta >= 0) || !(p->max_dist >= 0))
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_rrt_connect_batch: bad sample_num / tree_cap / rnd_stride / path_cap");
    if (nq == 0) return PMP_OK;
    if ((nr && !rect) || (nc && !circ) || (nb && !bnd) || !start_xy || !goal_xy || !rnd || !tree_xy || !tree_g ||
        !tree_parent || !n_nodes || !forward || !boundary || !cost || !path_len || (path_cap && !path_xy) || !iters ||
        !draws || !status)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_rrt_connect_batch: null pointer argument");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    RcArgs A;
    A.P = *p;
    A.rect = rect; A.circ = circ; A.bnd = bnd;
    A.nr = nr; A.nc = nc; A.nb = nb;
    A.start = start_xy; A.goal = goal_xy; A.nq = nq;
    A.rnd = rnd; A.stride = rnd_stride; A.cap = tree_cap;
    A.txy = tree_xy; A.tg = tree_g; A.tpar = tree_parent;
    A.n_nodes = n_nodes; A.forward = forward; A.boundary = boundary;
    A.cost = cost; A.path_len = path_len; A.path = path_xy; A.path_cap = path_cap;
    A.iters = iters; A.draws = draws; A.status = status; A.counters = counters;
    hipLaunchKernelGGL(rrt_connect_kernel, dim3((nq + kQW - 1) / kQW), dim3(kNT), (size_t)obs_bytes(nr, nc, nb),
                       (hipStream_t)stream, A);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}
