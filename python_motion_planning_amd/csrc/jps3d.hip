// Batched 3D Jump Point Search for gfx950, exact with the reference JPS3D.plan
// (global_planner/graph_search/jps3d.py:42-88) over Grid3D's 26 motions (utils/environment/env3d.py:56-70)
// with GraphSearcher3D.isCollision (graph_search_3d.py:66-107, Python-int coordinates).
//
// The outer loop is AStar3D's with another neighbour set: the (f, h, counter) tuple heap (a total
// order, so the heap shape is free; heap16.h with grid3d.h's Key3), a pop skipped when CLOSED holds
// the cell with g <= the popped g (:59-60), CLOSED overwritten before the goal test (:62-68), the 26
// jump() results computed first, each dropped when CLOSED holds its cell with g <= the new g
// (:75-81), the survivors pushed in motion order with consecutive counters (:83-85).
// g(jp) = g(node) + math.sqrt of the integer square distance node -> jp (_mk_qnode, :158-160).
//
// jump(c, d) (:96-155) is evaluated in its collapsed form.  n_k = c + k d; a step n_{k-1} -> n_k
// stops the ray when n_k is outside the grid, n_{k-1} or n_k is occupied, or (diagonal d) one of the
// corner cells n_{k-1} + d_a e_a is occupied (isCollision); forced(n, d) is the table of :164-244.
//   axis:  the first n_k before the stop with n_k == goal or forced(n_k, d);
//   plane diagonal: n_k is primary when it is the goal, forced, or an axis jump from it along a
//          non-zero component of d finds something; the reference also recurses along d itself from
//          every step (:147-151), so its result is n_1 when any primary step lies before the stop;
//   space diagonal: the first n_k before the stop that is the goal, forced, or from which one of the
//          three axis jumps or three plane-diagonal jumps finds something.
// Cells outside the grid never matter: the only (blocked, free) pairs with a blocked cell outside
// the grid have their free cell outside too, so "occupied or outside" serves both tests.
//
// One wave64 per query (persistent workers pulling an atomic queue, longest-first order as
// pmp_graph3d_batch).  Lane mapping of an expansion: the 26 rays run one after another, the steps of
// a ray on the lanes -- lane k tests step k + 1 (rounds of 64 for longer rays): one ballot of "this
// step stops" gives the first stop, the lanes before it test "this step is a hit" (axis rays: bit
// tests only; diagonal rays: the step's sub-jumps as serial scans on the step's lane, bounded by the
// grid side, early exit), a second ballot gives the first hit.  Lane m keeps ray m's result; the
// CLOSED test, the key and the batch push then run on lanes 0..25 as in astar3d.hip.
// Per-worker HBM state, reset per query: u32 CLOSED parent per cell (~0 = not CLOSED), f64 CLOSED g
// per cell, u32 parent of push #seq (a jump point's parent is the node that pushed it).
#include <algorithm>
#include "grid3d.h"

namespace {

using namespace grid3d;

// occupancy of a voxel, true outside the grid: from the bitmap staged in LDS or from HBM
template <bool OCC_LDS>
struct Occ {
    const uint32_t* g;
    const lds_w32* l;
    int X, Y, Z;
    __device__ __forceinline__ bool operator()(int x, int y, int z) const
    {
        return OCC_LDS ? occ3l(l, X, Y, Z, x, y, z) != 0u : occ3(g, X, Y, Z, x, y, z);
    }
};

struct V3 {
    int x, y, z;
};

// _has_forced_neighbor (jps3d.py:164-244) at cell n for direction d: some (blocked, free) pair holds
template <class O>
__host__ __device__ inline bool forced3(const O& o, V3 n, V3 d)
{
    // blocked(n + b) and free(n + f)
    auto P = [&](int bx, int by, int bz, int fx, int fy, int fz) -> bool {
        return o(n.x + bx, n.y + by, n.z + bz) && !o(n.x + fx, n.y + fy, n.z + fz);
    };
    const int nz = (d.x != 0) + (d.y != 0) + (d.z != 0);
    if (nz == 1) {  // the four face neighbours off the axis, each with the cell one step on (:186-208)
        bool f = false;
        if (d.x == 0) f = f || P(1, 0, 0, 1 + d.x, d.y, d.z) || P(-1, 0, 0, -1 + d.x, d.y, d.z);
        if (d.y == 0) f = f || P(0, 1, 0, d.x, 1 + d.y, d.z) || P(0, -1, 0, d.x, -1 + d.y, d.z);
        if (d.z == 0) f = f || P(0, 0, 1, d.x, d.y, 1 + d.z) || P(0, 0, -1, d.x, d.y, -1 + d.z);
        return f;
    }
    if (nz == 2) {  // 2D rules in the plane of motion (:211-229)
        if (d.z == 0) return P(-d.x, 0, 0, -d.x, d.y, 0) || P(0, -d.y, 0, d.x, -d.y, 0);
        if (d.y == 0) return P(-d.x, 0, 0, -d.x, 0, d.z) || P(0, 0, -d.z, d.x, 0, -d.z);
        return P(0, -d.y, 0, 0, -d.y, d.z) || P(0, 0, -d.z, 0, d.y, -d.z);
    }
    // space diagonal (:232-242)
    return P(-d.x, 0, 0, -d.x, d.y, 0) || P(0, -d.y, 0, d.x, -d.y, 0) || P(0, 0, -d.z, d.x, 0, -d.z);
}

// the step p -> p + d stops the ray (jps3d.py:110-116 with isCollision, graph_search_3d.py:66-107)
template <class O>
__host__ __device__ inline bool step_stops(const O& o, V3 p, V3 d)
{
    if (o(p.x + d.x, p.y + d.y, p.z + d.z) || o(p.x, p.y, p.z)) return true;
    const int nz = (d.x != 0) + (d.y != 0) + (d.z != 0);
    if (nz < 2) return false;
    return (d.x != 0 && o(p.x + d.x, p.y, p.z)) || (d.y != 0 && o(p.x, p.y + d.y, p.z)) ||
           (d.z != 0 && o(p.x, p.y, p.z + d.z));
}

__host__ __device__ inline bool same(V3 a, V3 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

// an axis jump from the free cell c finds something: serial scan, at most one grid side long
template <class O>
__host__ __device__ inline bool axis_hit(const O& o, V3 goal, V3 c, V3 d)
{
    for (;;) {
        c.x += d.x;
        c.y += d.y;
        c.z += d.z;
        if (o(c.x, c.y, c.z)) return false;  // occupied or outside the grid; the cell before is free
        if (same(c, goal) || forced3(o, c, d)) return true;
    }
}

// the step n of a plane-diagonal ray d is primary: goal, forced, or an axis jump along a component of d
template <class O>
__host__ __device__ inline bool primary2(const O& o, V3 goal, V3 n, V3 d)
{
    if (same(n, goal) || forced3(o, n, d)) return true;
    if (d.x != 0 && axis_hit(o, goal, n, V3{d.x, 0, 0})) return true;
    if (d.y != 0 && axis_hit(o, goal, n, V3{0, d.y, 0})) return true;
    return d.z != 0 && axis_hit(o, goal, n, V3{0, 0, d.z});
}

// a plane-diagonal jump from c finds something: a primary step before the ray stops
template <class O>
__host__ __device__ inline bool plane_hit(const O& o, V3 goal, V3 c, V3 d)
{
    for (;;) {
        if (step_stops(o, c, d)) return false;
        c.x += d.x;
        c.y += d.y;
        c.z += d.z;
        if (primary2(o, goal, c, d)) return true;
    }
}

// the step n of a space-diagonal ray d ends the jump (jps3d.py:127-152)
template <class O>
__host__ __device__ inline bool hit3(const O& o, V3 goal, V3 n, V3 d)
{
    if (primary2(o, goal, n, d)) return true;  // goal, forced, the three axis jumps
    return plane_hit(o, goal, n, V3{d.x, d.y, 0}) || plane_hit(o, goal, n, V3{d.x, 0, d.z}) ||
           plane_hit(o, goal, n, V3{0, d.y, d.z});
}

// "step n of a ray along d is a hit", by the number of non-zero components of d (wave-uniform)
template <class O>
__host__ __device__ inline bool step_hit(const O& o, V3 goal, V3 n, V3 d, int nz)
{
    if (nz == 1) return same(n, goal) || forced3(o, n, d);
    if (nz == 2) return primary2(o, goal, n, d);
    return hit3(o, goal, n, d);
}

template <bool OCC_LDS>
__global__ __launch_bounds__(64) void jps3d_kernel(
    const uint32_t* __restrict__ occ_all, int per_query, int X, int Y, int Z, int heuristic,
    const int32_t* __restrict__ start_xyz, const int32_t* __restrict__ goal_xyz, int nq, double* __restrict__ cost_out,
    int32_t* __restrict__ path_len_out, uint32_t* __restrict__ path_out, int path_cap, int32_t* __restrict__ nexp_out,
    uint32_t* __restrict__ expand_out, uint32_t* __restrict__ expand_parent, double* __restrict__ expand_g, int expand_cap,
    int64_t* __restrict__ counters, int32_t* __restrict__ status_out, int* __restrict__ queue, uint4* __restrict__ spill_all,
    int heap_cap, int lds_cap, double* __restrict__ cg_all, uint32_t* __restrict__ cpar_all, uint32_t* __restrict__ ppar_all,
    uint32_t ppar_cap, const int32_t* __restrict__ order, int prio_n)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = lane_id();
    const int worker = blockIdx.x;
    const size_t ncell = (size_t)X * Y * Z;
    const size_t words = (ncell + 31) / 32;
    const size_t spill_n = (size_t)(heap_cap > lds_cap ? heap_cap - lds_cap : 0);
    heap16::Heap hp =
        heap16::make_heap<true>(smem, lds_cap, spill_all + (size_t)worker * spill_n * 2, spill_n);  // 32 B records
    lds_w32* occl = (lds_w32*)(smem + (size_t)heap16::lds_entry_bytes<true>() * lds_cap);  // OCC_LDS: the query's bitmap
    double* cg = cg_all + (size_t)worker * ncell;                // CLOSED g
    uint32_t* cpar = cpar_all + (size_t)worker * ncell;          // CLOSED parent cell, ~0 = not CLOSED
    uint32_t* ppar = ppar_all + (size_t)worker * ppar_cap;       // parent of push #seq
    int pop_jl, pop_ol;
    heap16::pop_lane_consts(lane, pop_jl, pop_ol);
    const heap16::Walk6 pop_w = heap16::walk6_consts(lane, pop_jl, pop_ol);

    for (;;) {
        const int qi = next_query(queue, lane);
        if (qi >= nq) break;
        const int q = uni(order ? order[qi] : qi);
        if (qi < prio_n) __builtin_amdgcn_s_setprio(3);  // the longest queries set the launch's tail
        else __builtin_amdgcn_s_setprio(0);
        const uint32_t* occ = occ_all + (per_query ? (size_t)q * words : 0);
        if (OCC_LDS)
            for (size_t i = lane; i < words; i += 64) occl[i] = occ[i];
        for (size_t i = lane; i < ncell; i += 64) cpar[i] = ~0u;
        heap16::wsync();
        const Occ<OCC_LDS> o{occ, occl, X, Y, Z};
        const int sx = start_xyz[3 * q], sy = start_xyz[3 * q + 1], sz = start_xyz[3 * q + 2];
        Key3 qc;
        qc.gx = goal_xyz[3 * q];
        qc.gy = goal_xyz[3 * q + 1];
        qc.gz = goal_xyz[3 * q + 2];
        qc.heur = heuristic;
        qc.Y = Y;
        qc.Z = Z;
        const V3 goal{qc.gx, qc.gy, qc.gz};
        const bool s_in = (unsigned)sx < (unsigned)X && (unsigned)sy < (unsigned)Y && (unsigned)sz < (unsigned)Z;
        const bool g_in = (unsigned)qc.gx < (unsigned)X && (unsigned)qc.gy < (unsigned)Y && (unsigned)qc.gz < (unsigned)Z;
        const uint32_t st_c = ((uint32_t)sx * (uint32_t)Y + (uint32_t)sy) * (uint32_t)Z + (uint32_t)sz;
        if (!s_in || !g_in) {  // every lane stores the same values (no lane-0 block before the continue)
            status_out[q] = PMP_NO_PATH;
            cost_out[q] = __builtin_inf();
            path_len_out[q] = 0;
            nexp_out[q] = s_in ? 1 : 0;
            if (s_in && expand_out) {
                expand_out[(size_t)q * expand_cap] = st_c;
                if (expand_parent) expand_parent[(size_t)q * expand_cap] = st_c;
                if (expand_g) expand_g[(size_t)q * expand_cap] = 0.0;
            }
            if (counters) { counters[4 * q] = 1; counters[4 * q + 1] = 1; counters[4 * q + 2] = s_in; counters[4 * q + 3] = 1; }
            continue;
        }
        const uint32_t goal_xyz24 = ((uint32_t)qc.gx << 16) | ((uint32_t)qc.gy << 8) | (uint32_t)qc.gz;
        Ent root;  // start: g = 0, h = heuristic(start), counter 0 (jps3d.py:34-35,51); its parent is itself
        root.g = 0.0;
        root.a = 0u;
        root.b = ((((uint32_t)sx << 16) | ((uint32_t)sy << 8) | (uint32_t)sz) << 5) | 26u;
        qc.set_f(root);
        if (lane == 0) {
            heap16::store<true, true>(hp, 0, root);
            ppar[0] = st_c;
        }
        heap16::wsync();
        int n = 1;
        uint32_t seq = 1;
        int64_t npush = 1, npop = 0, niter = 0;
        int nexp = 0, maxn = 1, st = PMP_NO_PATH, plen = 0;
        double goal_cost = __builtin_inf();

        while (n > 0) {
            const Ent node = root;
            npop++;
            n -= 1;
            const int x = (int)((node.b >> 21) & 255u), y = (int)((node.b >> 13) & 255u), z = (int)((node.b >> 5) & 255u);
            const uint32_t lin = ((uint32_t)x * (uint32_t)Y + (uint32_t)y) * (uint32_t)Z + (uint32_t)z;
            // HBM round issued before the pop: the node's CLOSED state and the popped entry's parent
            const uint32_t scp = cpar[lin];
            const double scg = cg[lin];
            const uint32_t npar = ppar[node.a < ppar_cap ? node.a : 0u];
            if (n > 0) {
                if (n < lds_cap) heap16::pop<Key3, false, true>(hp, qc, n, root, lane, pop_jl, pop_ol, pop_w);
                else heap16::pop<Key3, true, true>(hp, qc, n, root, lane, pop_jl, pop_ol, pop_w);
            }
            const bool sclosed = rl_u32(scp, 0) != ~0u;
            if (sclosed && node.g >= rl_f64(scg, 0)) continue;  // :59-60
            niter++;
            if (lane == 0) {  // CLOSED[node.current] = node (:62)
                if (!sclosed && expand_out && nexp < expand_cap) expand_out[(size_t)q * expand_cap + nexp] = lin;
                cpar[lin] = npar;
                cg[lin] = node.g;
            }
            if (!sclosed) nexp++;
            heap16::wsync();
            if (((node.b >> 5) & 0xFFFFFFu) == goal_xyz24) {  // goal (:65-68): extractPath via CLOSED parents (:248-261)
                st = PMP_FOUND;
                if (lane == 0) {
                    uint32_t c = lin;
                    int len = 1;
                    double cost = 0.0;
                    while (c != st_c && len <= (int)ncell) {
                        const uint32_t p = cpar[c];
                        const int ddx = (int)(c / ((uint32_t)Y * Z)) - (int)(p / ((uint32_t)Y * Z));
                        const int ddy = (int)((c / (uint32_t)Z) % (uint32_t)Y) - (int)((p / (uint32_t)Z) % (uint32_t)Y);
                        const int ddz = (int)(c % (uint32_t)Z) - (int)(p % (uint32_t)Z);
                        cost += dist3(ddx, ddy, ddz);
                        c = p;
                        len++;
                    }
                    goal_cost = cost;
                    plen = len;
                    if (len <= path_cap) {
                        uint32_t* pth = path_out + (size_t)q * path_cap;
                        c = lin;
                        for (int i = len - 1; i >= 0; i--) {
                            pth[i] = c;
                            if (i == 0) break;
                            c = cpar[c];
                        }
                    }
                }
                break;
            }
            // ---- the 26 jumps (:74-81): rays one after another, steps on the lanes; lane m keeps ray m's result
            bool has = false;
            int jx = x, jy = y, jz = z;
            for (int m = 0; m < 26; m++) {
                const V3 d{c_m3.m[m][0], c_m3.m[m][1], c_m3.m[m][2]};
                const int nz = (d.x != 0) + (d.y != 0) + (d.z != 0);
                int found = 0;  // the hit's step number, 0 = None
                for (int base = 0;; base += 64) {
                    const int k = base + lane;  // this lane tests the step n_k -> n_{k+1}
                    const V3 p{x + k * d.x, y + k * d.y, z + k * d.z};
                    const uint64_t sm = ballot(step_stops(o, p, d));
                    const int fs = sm ? __ffsll((long long)sm) - 1 : 64;  // lanes before the first stop are on the ray
                    bool h = false;
                    if (lane < fs) h = step_hit(o, goal, V3{p.x + d.x, p.y + d.y, p.z + d.z}, d, nz);
                    const uint64_t hm = ballot(h);
                    if (hm) found = base + __ffsll((long long)hm);
                    if (hm || sm) break;  // a ray leaves the grid within 256 steps, which stops it
                }
                // a plane diagonal's own recursion returns the adjacent cell whenever anything lies ahead
                if (found && nz == 2) found = 1;
                if (lane == m) {
                    has = found != 0;
                    jx = x + found * d.x;
                    jy = y + found * d.y;
                    jz = z + found * d.z;
                }
            }
            // ---- candidates on lanes 0..25: CLOSED test (:79-80), g and key (_mk_qnode)
            const uint32_t jlin = ((uint32_t)jx * (uint32_t)Y + (uint32_t)jy) * (uint32_t)Z + (uint32_t)jz;
            const uint32_t jcp = cpar[jlin];
            const double jcg = cg[jlin];
            const double g1 = node.g + dist3(jx - x, jy - y, jz - z);
            const bool ok = has && !(jcp != ~0u && g1 >= jcg);
            const uint64_t okm = ballot(ok);
            const int nok = __popcll(okm);
            npush += nok;
            if (nok) {
                if (seq + (uint32_t)nok > ppar_cap || n + nok > heap_cap) {
                    st = PMP_CAP_OVERFLOW;
                    break;
                }
                Ent it;
                it.g = g1;
                it.a = seq + (uint32_t)__popcll(okm & ((1ull << lane) - 1ull));  // the reference's push counter
                it.b = ((((uint32_t)jx & 255u) << 16) | (((uint32_t)jy & 255u) << 8) | ((uint32_t)jz & 255u)) << 5 | (uint32_t)(lane & 31);
                qc.set_f(it);
                if (ok) ppar[it.a] = lin;
                n = heap16::push_batch(hp, qc, n, okm, it, root, lane);
                seq += (uint32_t)nok;
                if (n > maxn) maxn = n;
            }
        }
        heap16::wsync();
        // the final CLOSED parent and g of the cells in first-insertion order
        if (expand_out && (expand_parent || expand_g)) {
            const int ne = nexp < expand_cap ? nexp : expand_cap;
            for (int i = lane; i < ne; i += 64) {
                const uint32_t c = expand_out[(size_t)q * expand_cap + i];
                if (expand_parent) expand_parent[(size_t)q * expand_cap + i] = cpar[c];
                if (expand_g) expand_g[(size_t)q * expand_cap + i] = cg[c];
            }
        }
        if (lane == 0) {
            int s = st;
            if (s == PMP_FOUND && plen > path_cap) s = PMP_PATH_OVERFLOW;
            status_out[q] = s;
            cost_out[q] = st == PMP_FOUND ? goal_cost : __builtin_inf();
            path_len_out[q] = st == PMP_FOUND ? plen : 0;
            nexp_out[q] = nexp;
            if (counters) {
                counters[4 * q + 0] = npush;
                counters[4 * q + 1] = npop;
                counters[4 * q + 2] = niter;
                counters[4 * q + 3] = maxn;
            }
        }
        heap16::wsync();
    }
}

}  // namespace

extern "C" int pmp_jps3d_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int per_query, int X, int Y, int Z,
                               int heuristic, const int32_t* start_xyz, const int32_t* goal_xyz, int nq, double* cost,
                               int32_t* path_len, uint32_t* path, int path_cap, int32_t* n_expanded, uint32_t* expand,
                               uint32_t* expand_parent, double* expand_g, int expand_cap, int64_t* counters,
                               int32_t* status)
{
    if (!ctx) return PMP_EINVAL;
    if (X < 1 || Y < 1 || Z < 1 || X > kMaxDim3 || Y > kMaxDim3 || Z > kMaxDim3)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_jps3d_batch: X, Y, Z must be in [1, 256]");
    if (heuristic != 0 && heuristic != 1) return pmp_set_err(ctx, PMP_EINVAL, "pmp_jps3d_batch: heuristic must be 0 or 1");
    if (nq < 0 || path_cap < 1 || (expand && expand_cap < 1))
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_jps3d_batch: bad nq/path_cap/expand_cap");
    if (!expand && (expand_parent || expand_g))
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_jps3d_batch: expand_parent / expand_g need expand");
    if (nq == 0) return PMP_OK;
    if (!occ_bits || !start_xyz || !goal_xyz || !cost || !path_len || !path || !n_expanded || !status)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_jps3d_batch: null pointer argument");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t ncell = (size_t)X * Y * Z;
    // workers, LDS heap share and scratch budget as pmp_graph3d_batch (astar3d.hip)
    const int per_cu = pmp_workers_per_cu(ctx, 16, nq);
    int workers = 256 * per_cu;
    if (workers > nq) workers = nq;
    constexpr int kEnt = heap16::lds_entry_bytes<true>(), kSpill = heap16::spill_entry_bytes<true>();
    size_t hc = 26 * ncell + 8;
    if (hc > (size_t)(1 << 22)) hc = (size_t)1 << 22;
    const int heap_cap = (int)hc;
    const pmp_lds_plan lp = pmp_plan_lds(ctx, per_cu, (ncell + 31) / 32, kOccLdsWords, kEnt, heap_cap);
    if (!lp.ok)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_jps3d_batch: workers / resident per CU leave no LDS heap share");
    const size_t spill_n = lp.spill_n;
    // the parent of every push, indexed by the push counter (a query that pushes more stops with PMP_CAP_OVERFLOW)
    const uint32_t ppar_cap = (uint32_t)std::min<size_t>(64 * ncell + 64, (size_t)1 << 24);
    {
        const size_t per_worker = spill_n * kSpill + ncell * 8 + ((size_t)ncell + ppar_cap) * 4;
        const size_t fit = kScratchBudget3 / per_worker;
        if (fit < 1) return pmp_set_err(ctx, PMP_ENOMEM, "pmp_jps3d_batch: one worker exceeds the scratch budget");
        if ((size_t)workers > fit) workers = (int)fit;
    }
    uint4* spill = (uint4*)pmp_scratch(ctx, SCR_AUX1, (size_t)workers * spill_n * kSpill + 16);
    double* cg = (double*)pmp_scratch(ctx, SCR_AUX3, (size_t)workers * ncell * 8 + 16);
    uint32_t* tpar = (uint32_t*)pmp_scratch(ctx, SCR_AUX4, (size_t)workers * (ncell + ppar_cap) * 4 + 16);
    int* queue = (int*)pmp_scratch(ctx, SCR_AUX0, 256);
    if (!spill || !cg || !tpar || !queue) return PMP_ENOMEM;
    hipStream_t s = (hipStream_t)stream;
    PMP_HIP_CHECK(ctx, hipMemsetAsync(queue, 0, 16, s));
    int32_t* order = nullptr;
    {
        const int ext[3] = {X, Y, Z};
        const int rc = pmp_lpt_order(ctx, s, 3, start_xyz, goal_xyz, nq, ext, workers, &order);
        if (rc) return rc;
    }
    auto kern = lp.occ_lds ? jps3d_kernel<true> : jps3d_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(workers), dim3(64), (size_t)lp.lds_cap * kEnt + lp.occ_bytes, s, occ_bits, per_query, X, Y, Z,
                       heuristic, start_xyz, goal_xyz, nq, cost, path_len, path, path_cap, n_expanded, expand, expand_parent,
                       expand_g, expand_cap, counters, status, queue, spill, heap_cap, lp.lds_cap, cg, tpar,
                       tpar + (size_t)workers * ncell, ppar_cap, (const int32_t*)order, order ? ctx->astar_prio_n : 0);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}
