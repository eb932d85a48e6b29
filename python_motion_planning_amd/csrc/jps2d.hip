// Batched 2D Jump Point Search for gfx950, exact with the reference JPS.plan
// (global_planner/graph_search/jps.py:38-83) over Grid's 8 motions (utils/environment/env.py:52-55),
// including CPython heapq's tie behaviour under Node.__lt__ (utils/environment/node.py:51-54).
//
// The outer loop (:52-83): heappop; a pop whose cell is in CLOSED is skipped (no g comparison); the
// goal test; the 8 jump() results in motion order, each kept when its cell is not in CLOSED, pushed in
// that order until the goal has been pushed; then CLOSED[node.current] = node.  OPEN may hold several
// entries of a cell.  g(jp) adds the motion's cost once per step of the jump (Node.__add__ at every
// recursion level, :97): k dependent f64 additions.  h is GraphSearcher.h on integer differences,
// f = g + h, and an entry is less than another when f < f' or (f == f' and h < h').
//
// jump(c, d) (:85-121) is evaluated in its collapsed form.  n_k = c + k d, cells outside the grid
// count as obstacles (equal to the reference on grids whose border cells are obstacles):
//   axis ray:     the first n_k that is the goal or forced (detectForceNeighbor, :123-164), nothing
//                 once some n_k is an obstacle (the obstacle test comes before the goal test);
//   diagonal ray: the first n_k before an obstacle n_k that is the goal, a cell from which the axis
//                 ray along (d_x, 0) or (0, d_y) returns something, or forced.  No corner test.
// The reference's RecursionError on rays deeper than Python's recursion limit is not reproduced.
//
// Ray scan.  A pre-kernel writes two row-padded copies of the occupancy into context scratch, one
// per axis: A[x] holds column x's cells along y, B[y] holds row y's cells along x, each row a whole
// number of words with at least one padding bit, the padding set (outside = obstacle).  An axis ray
// is then a walk over words: obstacle = row(r), forced along +c = (row(r+1) & ~(row(r+1) >> 1)) |
// (row(r-1) & ~(row(r-1) >> 1)) with the neighbour word's carry, the goal one more bit, the first
// set bit by ffs / clz.  The four axis rays of an expansion run on lanes 0..3; the four diagonal
// rays run at once on the four 16-lane groups of the wave, lane i of a group testing step 16 r + i + 1
// in round r: a ballot of "n_k is an obstacle" bounds the ray, the lanes before it do their two axis
// sub-scans with the word walk, a second ballot gives the first hit.  Grids whose two copies fit
// kOccLdsWords are staged in LDS.
//
// Heap.  CPython's array element for element (Lib/heapq.py).  heappush: the ancestors of the new
// position load in one round on the lanes; those the item is less than are a suffix of the root
// path (the path is sorted), so a ballot popcount gives how many move down.  heappop: the _siftup
// walk to a leaf is a wave-uniform loop over the levels (lane i keeps level i's child); the final
// array of _siftup + _siftdown moves the children up while !(last < child) and drops `last` at the
// first child it is less than, again one ballot.  Entries are 16 B (f, h's integer order key, push
// number) in LDS, positions >= lds_cap in a per-worker HBM spill.
//
// One wave64 per query, persistent workers pulling an atomic queue, longest-first order (lpt_order.hip)
// and raised priority as the A* engines.  Per-worker HBM state: g, cell and parent cell of push #seq, the
// query's CLOSED list (push numbers, in insertion order), one CLOSED bit per cell and the CLOSED push
// number per cell (read only where the bit is set).  The bits are zero between queries: a query
// clears them by walking its own CLOSED list.
#include <algorithm>
#include <cmath>
#include "pmp_internal.h"
#include "astar2d_entry.h"

namespace {

constexpr int kMaxDim = 8192;
constexpr double kSqrt2 = 1.4142135623730951;  // math.sqrt(2), the diagonal motions' cost (env.py:52-55)
constexpr int kOccLdsWords = 4096;             // both padded copies staged in LDS up to this size
constexpr int kEnt = 16;                       // bytes of a heap entry
constexpr size_t kScratchBudget = (size_t)96 << 30;  // workers are reduced to fit

// motions (mot_x, mot_y: even = axis, odd = diagonal) and lds_u32 come from astar2d_entry.h
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4 lds_u4;

__device__ __forceinline__ void wsync() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// ---- the padded copies ------------------------------------------------------------------------
__host__ __device__ inline int row_words(int n) { return n / 32 + 1; }  // >= 1 padding bit

// word t of the copies: A (W rows of SA words) then B (H rows of SB words)
__global__ void jps2d_rows(const uint32_t* __restrict__ occ, int W, int H, uint32_t* __restrict__ out)
{
    const int SA = row_words(H), SB = row_words(W);
    const size_t nA = (size_t)W * SA, nB = (size_t)H * SB;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nA + nB) return;
    const bool a = t < nA;
    const size_t u = a ? t : t - nA;
    const int r = (int)(u / (size_t)(a ? SA : SB)), w = (int)(u % (size_t)(a ? SA : SB));
    uint32_t v = 0u;
    for (int b = 0; b < 32; b++) {
        const int c = 32 * w + b;
        bool o = true;
        if (c < (a ? H : W)) {
            const uint32_t ci = a ? (uint32_t)r * (uint32_t)H + (uint32_t)c : (uint32_t)c * (uint32_t)H + (uint32_t)r;
            o = ((occ[ci >> 5] >> (ci & 31u)) & 1u) != 0u;
        }
        v |= (o ? 1u : 0u) << b;
    }
    out[t] = v;
}

// one padded copy: n rows of `stride` words, from LDS or HBM; everything outside reads as obstacle
template <bool L>
struct Rows {
    const uint32_t* g;
    const lds_u32* l;
    int n, stride;
    __device__ __forceinline__ uint32_t word(int r, int w) const
    {
        if ((unsigned)r >= (unsigned)n || (unsigned)w >= (unsigned)stride) return ~0u;
        const int i = r * stride + w;
        return L ? l[i] : g[i];
    }
    __device__ __forceinline__ bool bit(int r, int c) const { return ((word(r, c >> 5) >> (c & 31)) & 1u) != 0u; }
};

// The axis ray from the cell (r, c0) of a copy along s = +-1 in its column coordinate: the number of
// steps to the first cell that is the goal (gr, gc) or forced, 0 when an obstacle comes first.
template <bool L>
__device__ inline int axis_scan(const Rows<L>& R, int r, int c0, int s, int gr, int gc)
{
    int w = c0 >> 5;
    uint32_t mask = s > 0 ? ((~0u << (c0 & 31)) << 1) : ((1u << (c0 & 31)) - 1u);  // the word's cells beyond c0
    for (;;) {
        if ((unsigned)w >= (unsigned)R.stride) return 0;
        const uint32_t b = R.word(r, w), u = R.word(r + 1, w), l = R.word(r - 1, w);
        const uint32_t un = R.word(r + 1, w + s), ln = R.word(r - 1, w + s);
        // forced at c (:137-153): a side cell is an obstacle and the side cell one step on is not
        const uint32_t us = s > 0 ? (u >> 1) | (un << 31) : (u << 1) | (un >> 31);
        const uint32_t ls = s > 0 ? (l >> 1) | (ln << 31) : (l << 1) | (ln >> 31);
        uint32_t hit = (u & ~us) | (l & ~ls);
        if (r == gr && (gc >> 5) == w) hit |= 1u << (gc & 31);
        const uint32_t m = (b | hit) & mask;
        if (m) {
            const int p = s > 0 ? __ffs((int)m) - 1 : 31 - __clz((int)m);
            if ((b >> p) & 1u) return 0;  // the obstacle test comes first (:102-107)
            return abs(32 * w + p - c0);
        }
        w += s;
        mask = ~0u;
    }
}

// ---- the heap ---------------------------------------------------------------------------------
struct Ent {
    double f;
    uint32_t hk, seq;
};
struct Heap {
    lds_u4* l;
    u32x4* s;
    int lds_cap;
};
__device__ __forceinline__ Ent hld(const Heap& h, int p)
{
    u32x4 v;
    if (p < h.lds_cap) v = h.l[p];
    else v = h.s[p - h.lds_cap];
    Ent e;
    e.f = __longlong_as_double(((uint64_t)v.y << 32) | v.x);
    e.hk = v.z;
    e.seq = v.w;
    return e;
}
__device__ __forceinline__ void hst(const Heap& h, int p, const Ent& e)
{
    const uint64_t b = (uint64_t)__double_as_longlong(e.f);
    const u32x4 v = {(uint32_t)b, (uint32_t)(b >> 32), e.hk, e.seq};
    if (p < h.lds_cap) h.l[p] = v;
    else h.s[p - h.lds_cap] = v;
}
// Node.__lt__ (node.py:51-54); the order of h is the order of its integer key
__device__ __forceinline__ bool ent_lt(const Ent& a, const Ent& b)
{
    return (a.f < b.f) | ((a.f == b.f) & (a.hk < b.hk));
}

// heapq.heappush on a heap of n entries (wave-uniform `it`): append, _siftdown(heap, 0, n)
__device__ inline void heap_push(const Heap& h, int n, const Ent& it, int lane)
{
    // lane j >= 1 takes the j-th ancestor of position n (lane 0 the position itself)
    int pos = n, child = n;
    bool have = lane == 0;
    if (lane >= 1 && lane < 32) {
        const uint32_t a = ((uint32_t)n + 1u) >> lane;  // 1-based ancestor index, 0 = above the root
        have = a != 0u;
        pos = (int)a - 1;
        child = (int)((((uint32_t)n + 1u) >> (lane - 1)) - 1u);
    }
    Ent e = it;
    if (lane >= 1 && have) e = hld(h, pos);
    const uint64_t mv = ballot(lane >= 1 && have && ent_lt(it, e));  // a suffix of the root path
    const int m = __popcll(mv);
    wsync();
    if (lane >= 1 && lane <= m) hst(h, child, e);
    if (lane == m) hst(h, pos, it);
    wsync();
}

// heapq.heappop on a heap of n >= 1 entries: returns heap[0]; the array becomes CPython's
__device__ inline Ent heap_pop(const Heap& h, int n, int lane)
{
    const Ent last = hld(h, n - 1);
    if (n == 1) return last;
    const Ent ret = hld(h, 0);
    const int end = n - 1;
    // _siftup's walk: lane i keeps the level-i child on the path and the position it would move to
    int pos = 0, lvl = 0, myto = 0;
    Ent c = last;
    for (int cp = 1; cp < end; cp = 2 * pos + 1) {
        Ent e = hld(h, cp);
        const int rp = cp + 1;
        if (rp < end) {
            const Ent er = hld(h, rp);
            if (!ent_lt(e, er)) {
                cp = rp;
                e = er;
            }
        }
        lvl++;
        if (lane == lvl) {
            c = e;
            myto = pos;
        }
        pos = cp;
    }
    // the children move up while !(last < child); `last` lands where the first one it is less than was
    const uint64_t lt = ballot(lane >= 1 && lane <= lvl && ent_lt(last, c));
    const int t = lt ? __ffsll((long long)lt) - 1 : lvl + 1;
    wsync();
    if (lane >= 1 && lane < t) hst(h, myto, c);
    const int lp = (int)rl_u32((uint32_t)myto, t <= lvl ? t : 0);  // p_{t-1}
    if (lane == 0) hst(h, t <= lvl ? lp : pos, last);
    wsync();
    return ret;
}

// ---- the search -------------------------------------------------------------------------------
template <bool OCC_LDS>
__global__ __launch_bounds__(64) void jps2d_kernel(
    const uint32_t* __restrict__ rows, int W, int H, int heuristic, const int32_t* __restrict__ start_xy,
    const int32_t* __restrict__ goal_xy, int nq, double* __restrict__ cost_out, int32_t* __restrict__ path_len_out,
    uint32_t* __restrict__ path_out, int path_cap, int32_t* __restrict__ nexp_out, uint32_t* __restrict__ expand_out,
    uint32_t* __restrict__ expand_parent, double* __restrict__ expand_g, int expand_cap, int64_t* __restrict__ counters,
    int32_t* __restrict__ status_out, int* __restrict__ queue, uint4* __restrict__ spill_all, int push_cap, int lds_cap,
    double* __restrict__ sg_all, uint32_t* __restrict__ su_all, uint32_t* __restrict__ cell_all, size_t cbit_words,
    const int32_t* __restrict__ order, int prio_n)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = lane_id();
    const int worker = blockIdx.x;
    const size_t ncell = (size_t)W * H;
    const int SA = row_words(H), SB = row_words(W);
    const size_t nA = (size_t)W * SA, nB = (size_t)H * SB;
    const size_t spill_n = (size_t)(push_cap > lds_cap ? push_cap - lds_cap : 0);
    Heap hp;
    hp.l = (lds_u4*)smem;
    hp.s = (u32x4*)spill_all + (size_t)worker * spill_n;
    hp.lds_cap = lds_cap;
    lds_u32* occl = (lds_u32*)(smem + (size_t)kEnt * lds_cap);
    if (OCC_LDS) {
        for (size_t i = lane; i < nA + nB; i += 64) occl[i] = rows[i];
        wsync();
    }
    const Rows<OCC_LDS> RA{rows, occl, W, SA}, RB{rows + nA, occl + nA, H, SB};
    double* sg = sg_all + (size_t)worker * push_cap;                       // g of push #seq
    uint32_t* scell = su_all + (size_t)worker * 3 * (size_t)push_cap;      // its cell
    uint32_t* spar = scell + push_cap;                                     // its parent cell
    uint32_t* clist = spar + push_cap;                                     // CLOSED: push numbers in insertion order
    uint32_t* cbit = cell_all + (size_t)worker * cbit_words;               // CLOSED bit per cell
    uint32_t* cseq = cell_all + (size_t)gridDim.x * cbit_words + (size_t)worker * ncell;  // CLOSED push number (bit set)

    for (;;) {
        const int qi = next_query(queue, lane);
        if (qi >= nq) break;
        const int q = uni(order ? order[qi] : qi);
        if (qi < prio_n) __builtin_amdgcn_s_setprio(3);  // the longest queries set the launch's tail
        else __builtin_amdgcn_s_setprio(0);
        const int sx = start_xy[2 * q], sy = start_xy[2 * q + 1];
        const int gx = goal_xy[2 * q], gy = goal_xy[2 * q + 1];
        const bool s_in = (unsigned)sx < (unsigned)W && (unsigned)sy < (unsigned)H;
        const bool g_in = (unsigned)gx < (unsigned)W && (unsigned)gy < (unsigned)H;
        if (!s_in || !g_in) {  // every lane stores the same values
            status_out[q] = PMP_NO_PATH;
            cost_out[q] = 0.0;
            path_len_out[q] = 0;
            nexp_out[q] = 0;
            if (counters) { counters[4 * q] = 0; counters[4 * q + 1] = 0; counters[4 * q + 2] = 0; counters[4 * q + 3] = 0; }
            continue;
        }
        const uint32_t st_c = (uint32_t)sx * (uint32_t)H + (uint32_t)sy;
        const uint32_t goal_c = (uint32_t)gx * (uint32_t)H + (uint32_t)gy;
        if (lane == 0) {  // the start: g = 0, h = 0 (Planner.__init__), its parent is itself
            Ent root;
            root.f = 0.0;
            root.hk = 0u;
            root.seq = 0u;
            hst(hp, 0, root);
            sg[0] = 0.0;
            scell[0] = st_c;
            spar[0] = st_c;
        }
        wsync();
        int n = 1, nexp = 0, maxn = 1, st = PMP_NO_PATH, plen = 0;
        uint32_t seq = 1;
        int64_t npush = 1, npop = 0;
        double goal_cost = 0.0;

        while (n > 0) {
            const Ent top = heap_pop(hp, n, lane);
            n -= 1;
            npop++;
            const uint32_t cell = scell[top.seq];
            const double node_g = sg[top.seq];
            if ((cbit[cell >> 5] >> (cell & 31u)) & 1u) continue;  // :56-57
            const int x = (int)(cell / (uint32_t)H), y = (int)(cell % (uint32_t)H);
            if (cell != goal_c) {
                // ---- the four axis rays on lanes 0..3 (motions 0, 2, 4, 6)
                int ka = 0;
                if (lane < 4) {
                    const int dx = mot_x(2 * lane), dy = mot_y(2 * lane);
                    ka = dx != 0 ? axis_scan(RB, y, x, dx, gy, gx) : axis_scan(RA, x, y, dy, gx, gy);
                }
                // ---- the four diagonal rays on the four 16-lane groups (motions 1, 3, 5, 7)
                const int grp = lane >> 4, li = lane & 15;
                const int dx = mot_x(2 * grp + 1), dy = mot_y(2 * grp + 1);
                int kd = 0;
                bool done = false;
                for (int base = 0;; base += 16) {
                    const int k = base + li + 1;
                    const int nx = x + k * dx, ny = y + k * dy;
                    const uint64_t sm = ballot(!done && RA.bit(nx, ny));  // obstacle or outside: the ray ends
                    const uint32_t gsm = (uint32_t)(sm >> (16 * grp)) & 0xFFFFu;
                    const int fs = gsm ? __ffs((int)gsm) - 1 : 16;
                    bool hit = false;
                    if (!done && li < fs) {
                        hit = (nx == gx && ny == gy) ||                                         // :106-107
                              (RA.bit(nx - dx, ny) && !RA.bit(nx - dx, ny + dy)) ||             // :156-162
                              (RA.bit(nx, ny - dy) && !RA.bit(nx + dx, ny - dy));
                        if (!hit) hit = axis_scan(RB, ny, nx, dx, gy, gx) != 0;                 // :112-115
                        if (!hit) hit = axis_scan(RA, nx, ny, dy, gx, gy) != 0;
                    }
                    const uint64_t hm = ballot(hit);
                    const uint32_t ghm = (uint32_t)(hm >> (16 * grp)) & 0xFFFFu;
                    if (!done) {
                        if (ghm) kd = base + __ffs((int)ghm);
                        done = ghm != 0u || gsm != 0u;
                    }
                    if (ballot(!done) == 0ull) break;  // a ray leaves the grid, which ends it
                }
                // ---- lane m keeps motion m's jump point: CLOSED test (:69), g, h (:70-71)
                const int ks = __shfl(ka, (lane >> 1) & 3), kg = __shfl(kd, ((lane >> 1) & 3) * 16);
                const int k = lane < 8 ? ((lane & 1) ? kg : ks) : 0;
                const int jx = x + k * mot_x(lane & 7), jy = y + k * mot_y(lane & 7);
                const uint32_t jc = (uint32_t)jx * (uint32_t)H + (uint32_t)jy;
                bool ok = k > 0;
                if (ok) ok = ((cbit[jc >> 5] >> (jc & 31u)) & 1u) == 0u;
                uint64_t okm = ballot(ok);
                const uint64_t gm = ballot(ok && jc == goal_c);
                if (gm) okm &= (2ull << (__ffsll((long long)gm) - 1)) - 1ull;  // nothing is pushed after the goal (:78-80)
                ok = ok && ((okm >> lane) & 1ull);
                const int nok = __popcll(okm);
                if (nok) {
                    if (seq + (uint32_t)nok > (uint32_t)push_cap) {
                        st = PMP_CAP_OVERFLOW;
                        break;
                    }
                    Ent it;
                    it.f = 0.0;
                    it.hk = 0u;
                    it.seq = seq + (uint32_t)__popcll(okm & ((1ull << lane) - 1ull));
                    if (ok) {
                        double g1 = node_g;
                        const double mc = (lane & 1) ? kSqrt2 : 1.0;
                        for (int i = 0; i < k; i++) g1 += mc;  // Node.__add__ once per step (:97)
                        const int hx = abs(gx - jx), hy = abs(gy - jy);
                        it.hk = heuristic ? (uint32_t)(hx + hy) : (uint32_t)(hx * hx + hy * hy);
                        it.f = g1 + (heuristic ? (double)it.hk : __dsqrt_rn((double)it.hk));
                        sg[it.seq] = g1;
                        scell[it.seq] = jc;
                        spar[it.seq] = cell;
                    }
                    wsync();
                    for (uint64_t pm = okm; pm; pm &= pm - 1ull) {
                        const int m = __ffsll((long long)pm) - 1;
                        Ent e;
                        e.f = rl_f64(it.f, m);
                        e.hk = rl_u32(it.hk, m);
                        e.seq = rl_u32(it.seq, m);
                        heap_push(hp, n, e, lane);
                        n++;
                    }
                    seq += (uint32_t)nok;
                    npush += nok;
                    if (n > maxn) maxn = n;
                }
            }
            if (lane == 0) {  // CLOSED[node.current] = node (:61, :82)
                cbit[cell >> 5] |= 1u << (cell & 31u);
                cseq[cell] = top.seq;
                clist[nexp] = top.seq;
            }
            nexp++;
            wsync();
            if (cell == goal_c) {  // extractPath (a_star.py:98-117): hypot per leg, accumulated goal -> start
                st = PMP_FOUND;
                if (lane == 0) {
                    uint32_t c = cell;
                    int len = 1;
                    double cost = 0.0;
                    while (c != st_c && len <= nexp) {
                        const uint32_t p = spar[cseq[c]];
                        const int ddx = (int)(c / (uint32_t)H) - (int)(p / (uint32_t)H);
                        const int ddy = (int)(c % (uint32_t)H) - (int)(p % (uint32_t)H);
                        cost += __dsqrt_rn((double)(ddx * ddx + ddy * ddy));
                        c = p;
                        len++;
                    }
                    goal_cost = cost;
                    plen = len;
                    if (len <= path_cap) {
                        uint32_t* pth = path_out + (size_t)q * path_cap;
                        c = cell;
                        for (int i = 0; i < len; i++) {
                            pth[i] = c;
                            c = spar[cseq[c]];
                        }
                    }
                }
                break;
            }
        }
        wsync();
        // the CLOSED records in insertion order, and the query's CLOSED bits cleared for the next one
        for (int i = lane; i < nexp; i += 64) {
            const uint32_t sq = clist[i];
            const uint32_t c = scell[sq];
            if (expand_out && i < expand_cap) {
                expand_out[(size_t)q * expand_cap + i] = c;
                if (expand_parent) expand_parent[(size_t)q * expand_cap + i] = spar[sq];
                if (expand_g) expand_g[(size_t)q * expand_cap + i] = sg[sq];
            }
            atomicAnd(&cbit[c >> 5], ~(1u << (c & 31u)));
        }
        if (lane == 0) {
            int s = st;
            if (s == PMP_FOUND && plen > path_cap) s = PMP_PATH_OVERFLOW;
            status_out[q] = s;
            cost_out[q] = st == PMP_FOUND ? goal_cost : 0.0;
            path_len_out[q] = st == PMP_FOUND ? plen : 0;
            nexp_out[q] = nexp;
            if (counters) {
                counters[4 * q + 0] = npush;
                counters[4 * q + 1] = npop;
                counters[4 * q + 2] = nexp;
                counters[4 * q + 3] = maxn;
            }
        }
        wsync();
    }
}

}  // namespace

extern "C" int pmp_jps2d_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int W, int H, int heuristic,
                               const int32_t* start_xy, const int32_t* goal_xy, int nq, double* cost,
                               int32_t* path_len, uint32_t* path, int path_cap, int32_t* n_expanded,
                               uint32_t* expand, uint32_t* expand_parent, double* expand_g, int expand_cap,
                               int push_cap, int64_t* counters, int32_t* status)
{
    if (!ctx) return PMP_EINVAL;
    if (W < 1 || H < 1 || W > kMaxDim || H > kMaxDim)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_jps2d_batch: W, H must be in [1, 8192]");
    if (heuristic != 0 && heuristic != 1) return pmp_set_err(ctx, PMP_EINVAL, "pmp_jps2d_batch: heuristic must be 0 or 1");
    if (nq < 0 || path_cap < 1 || (expand && expand_cap < 1) || push_cap < 0)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_jps2d_batch: bad nq/path_cap/expand_cap/push_cap");
    if (!expand && (expand_parent || expand_g))
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_jps2d_batch: expand_parent / expand_g need expand");
    if (nq == 0) return PMP_OK;
    if (!occ_bits || !start_xy || !goal_xy || !cost || !path_len || !path || !n_expanded || !status)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_jps2d_batch: null pointer argument");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t ncell = (size_t)W * H;
    // every push is kept (its g, cell and parent), so the push capacity is the heap's too: by default
    // 8 per cell (a cell closes once and pushes at most 8) up to 2^20
    if (push_cap == 0) push_cap = (int)std::min<size_t>(8 * ncell + 8, (size_t)1 << 20);
    if (push_cap < 16) push_cap = 16;
    int workers = 256 * pmp_workers_per_cu(ctx, 8, nq);
    if (workers > nq) workers = nq;
    const size_t cbit_words = (ncell + 31) / 32;
    {  // the scratch budget bounds the workers (the heap counted without its LDS part)
        const size_t per_worker = (size_t)push_cap * (kEnt + 20) + (cbit_words + ncell) * 4;
        const size_t fit = kScratchBudget / per_worker;
        if (fit < 1) return pmp_set_err(ctx, PMP_ENOMEM, "pmp_jps2d_batch: one worker exceeds the scratch budget");
        if ((size_t)workers > fit) workers = (int)fit;
    }
    const int per_cu = (workers + 255) / 256;  // of the workers that run: each one's LDS share
    const size_t nrows = (size_t)W * row_words(H) + (size_t)H * row_words(W);
    // the two padded copies are this planner's occupancy: in LDS when the share holds them beside a heap
    const pmp_lds_plan lp = pmp_plan_lds(ctx, per_cu, nrows, kOccLdsWords, kEnt, push_cap);
    if (!lp.ok)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_jps2d_batch: workers / resident per CU leave no LDS heap share");
    uint4* spill = (uint4*)pmp_scratch(ctx, SCR_AUX1, (size_t)workers * lp.spill_n * kEnt + 16);
    double* sg = (double*)pmp_scratch(ctx, SCR_AUX3, (size_t)workers * push_cap * 8 + 16);
    uint32_t* su = (uint32_t*)pmp_scratch(ctx, SCR_AUX4, (size_t)workers * push_cap * 12 + 16);
    uint32_t* cells = (uint32_t*)pmp_scratch(ctx, SCR_AUX2, (size_t)workers * (cbit_words + ncell) * 4 + 16);
    uint32_t* rows = (uint32_t*)pmp_scratch(ctx, SCR_BITS, nrows * 4 + 16);
    int* queue = (int*)pmp_scratch(ctx, SCR_AUX0, 256);
    if (!spill || !sg || !su || !cells || !rows || !queue) return PMP_ENOMEM;
    hipStream_t s = (hipStream_t)stream;
    PMP_HIP_CHECK(ctx, hipMemsetAsync(queue, 0, 16, s));
    // the CLOSED bits of every worker start clear (each query clears its own afterwards)
    PMP_HIP_CHECK(ctx, hipMemsetAsync(cells, 0, (size_t)workers * cbit_words * 4, s));
    hipLaunchKernelGGL(jps2d_rows, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, s, occ_bits, W, H, rows);
    int32_t* order = nullptr;
    {
        const int ext[2] = {W, H};
        const int rc = pmp_lpt_order(ctx, s, 2, start_xy, goal_xy, nq, ext, workers, &order);
        if (rc) return rc;
    }
    auto kern = lp.occ_lds ? jps2d_kernel<true> : jps2d_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(workers), dim3(64), (size_t)lp.lds_cap * kEnt + lp.occ_bytes, s, rows, W, H, heuristic, start_xy,
                       goal_xy, nq, cost, path_len, path, path_cap, n_expanded, expand, expand_parent, expand_g,
                       expand_cap, counters, status, queue, spill, push_cap, lp.lds_cap, sg, su, cells, cbit_words,
                       (const int32_t*)order, order ? ctx->astar_prio_n : 0);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}
