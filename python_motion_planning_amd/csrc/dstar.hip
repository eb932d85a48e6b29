// Batched D* (plan + OnPress replanning) for gfx950, exact with DStar.plan (global_planner/graph_search/d_star.py:75-291)
// over Grid with GraphSearcher.isCollision (graph_search.py:61-87).
//
// The reference's OPEN is a Python list: insert appends (duplicates allowed, :236-248), min_state is
// the FIRST entry of minimal k in list order (:220-227), delete removes the first occurrence
// (:250-259).  All entries of one node share that node's k, so the popped entry is the earliest
// remaining entry of the node minimising (k, first entry position) -- a strict total order.  The
// kernel keeps:
//   per cell (32 B): h, k, first/last remaining entry, parent cell, entry count | tag << 24;
//   per entry: the next entry of the same node (a FIFO per node, positions = append counter);
//   a lazy min-heap (heap16.h) of (k, first position, cell), validated on pop against the cell.
// plan() is followed by any number of OnPress(x, y) calls (:102-134) without the figure: add the
// obstacle to the worker's copy of the grid, walk from the start along the parents and modify()
// (:262-274) where an edge collides -- processState on the kept OPEN / cell states.
// processState (:158-218) runs on one wave: lanes 0..7 are the 8 motions (env.py:52-55) in order,
// the RAISE scan is a scalar loop, the LOWER/else decisions are per lane, and appended entries
// take their positions by lane-order prefix counts, exactly the reference's append order.
#include <algorithm>
#include "heap16.h"

namespace {

__device__ __constant__ int c_dmx[8] = {-1, -1, 0, 1, 1, 1, 0, -1};
__device__ __constant__ int c_dmy[8] = {0, 1, 1, 1, 0, -1, -1, -1};

constexpr uint32_t T_NEW = 0, T_OPEN = 1, T_CLOSED = 2;

struct __attribute__((aligned(16))) DCell {
    double h, k;
    int32_t first, last, parent;
    uint32_t cnt_t;  // entry count (24 bits) | tag << 24
};

using heap16::Ent;  // g = k, a = first entry position, b = cell

struct KeyD {
    static constexpr bool kStoredF = false;
    __device__ __forceinline__ void derive(Ent& e) const { e.f = e.g; e.hk = 0u; }
    static __device__ __forceinline__ bool lt(const Ent& x, const Ent& y)
    {
        return (x.g < y.g) | ((x.g == y.g) & (x.a < y.a));
    }
};

// branch-free: the word is loaded for any (x, y) (index 0 outside the grid), so the several
// occupancy reads of one collision test issue together instead of one round trip each
__device__ __forceinline__ uint32_t occ2(const uint32_t* occ, int W, int H, int x, int y)
{
    const bool in = (unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H;
    const uint32_t c = in ? (uint32_t)x * (uint32_t)H + (uint32_t)y : 0u;
    return (in ? 0u : 1u) | ((occ[c >> 5] >> (c & 31)) & 1u);
}

__device__ __forceinline__ DCell load_cell(const DCell* cells, int c)
{
    const uint4* p = reinterpret_cast<const uint4*>(cells + c);
    const uint4 a = p[0], b = p[1];
    DCell r;
    r.h = __hiloint2double((int)a.y, (int)a.x);
    r.k = __hiloint2double((int)a.w, (int)a.z);
    r.first = (int32_t)b.x;
    r.last = (int32_t)b.y;
    r.parent = (int32_t)b.z;
    r.cnt_t = b.w;
    return r;
}

__device__ __forceinline__ void store_cell(DCell* cells, int c, const DCell& v)
{
    uint4* p = reinterpret_cast<uint4*>(cells + c);
    const uint64_t hb = (uint64_t)__double_as_longlong(v.h), kb = (uint64_t)__double_as_longlong(v.k);
    p[0] = make_uint4((uint32_t)hb, (uint32_t)(hb >> 32), (uint32_t)kb, (uint32_t)(kb >> 32));
    p[1] = make_uint4((uint32_t)v.first, (uint32_t)v.last, (uint32_t)v.parent, v.cnt_t);
}

__device__ __forceinline__ uint32_t cnt_of(uint32_t ct) { return ct & 0xFFFFFFu; }
__device__ __forceinline__ uint32_t tag_of(uint32_t ct) { return ct >> 24; }

__device__ __forceinline__ DCell rl_cell(const DCell& v, int lane)
{
    DCell r;
    r.h = rl_f64(v.h, lane);
    r.k = rl_f64(v.k, lane);
    r.first = (int32_t)rl_u32((uint32_t)v.first, lane);
    r.last = (int32_t)rl_u32((uint32_t)v.last, lane);
    r.parent = (int32_t)rl_u32((uint32_t)v.parent, lane);
    r.cnt_t = rl_u32(v.cnt_t, lane);
    return r;
}

// Per-query search state of one wave (wave-uniform scalars)
struct Search2 {
    heap16::Heap hp;
    DCell* cells;
    int32_t* nxt;
    int heap_cap, lds_cap, entry_cap;
    int n;              // heap elements (valid + stale)
    int64_t open;       // len(OPEN) (entries, duplicates included)
    int ne;             // entries appended so far (list positions)
    int64_t np;         // processState calls (len(EXPAND), a None entry included)
    Ent root;
    int start;
    int goal_slot, goal_cell;  // start == goal: the goal object lives in slot W*H (d_star.py:66-68)
    bool start_closed;  // self.start.t == 'CLOSED'
    bool overflow;
    int raise_cell;     // PS_RAISE: the border node whose getNeighbor raised KeyError
};

// processState outcome: EMPTY = OPEN was empty (the reference appends None to EXPAND, returns -1),
// DONE = processed and OPEN is non-empty (min_k is S.root after clean_top), EMPTIED = processed and
// OPEN is empty (the reference's `return self.min_k` raises AttributeError), OVER = a cap was hit,
// RAISE = getNeighbor of a node on the grid's border looked up an out-of-grid cell (KeyError)
enum { PS_EMPTY = 0, PS_DONE = 1, PS_EMPTIED = 2, PS_OVER = 3, PS_RAISE = 4 };

struct D2 {
    const uint32_t* occ;  // the shared grid, or the worker's working copy (OnPress adds obstacles)
    int W, H;
    Search2& S;
    int lane, pop_jl, pop_ol;
    int mdx, mdy;
    double mcost;
    KeyD key;
    heap16::Walk6 pop_w{0ull, 0ull};  // set after construction (walk6_consts)

    __device__ __forceinline__ void push(const Ent& it0)
    {
        if (S.n >= S.heap_cap) { S.overflow = true; return; }
        Ent it = it0;
        key.derive(it);
        if (S.n == 0) {
            if (lane == 0) heap16::store<true>(S.hp, 0, it);
            S.root = it;
            heap16::wsync();
        } else if (S.n < S.lds_cap) {
            heap16::push<KeyD, false>(S.hp, key, S.n, it, S.root, lane);
        } else {
            heap16::push<KeyD, true>(S.hp, key, S.n, it, S.root, lane);
        }
        S.n += 1;
    }

    __device__ __forceinline__ void pop_top()
    {
        S.n -= 1;
        if (S.n > 0) {
            if (S.n < S.lds_cap) heap16::pop<KeyD, false, true>(S.hp, key, S.n, S.root, lane, pop_jl, pop_ol, pop_w);
            else heap16::pop<KeyD, true, true>(S.hp, key, S.n, S.root, lane, pop_jl, pop_ol, pop_w);
        }
    }

    // drop heap tops that do not match their cell's (k, first entry); S.root is then min_state and
    // `c` its cell (valid when the loop returned early)
    __device__ __forceinline__ void clean_top(DCell& c)
    {
        while (S.open > 0 && S.n > 0) {
            c = load_cell(S.cells, (int)S.root.b);
            if (cnt_of(c.cnt_t) > 0 && (uint32_t)c.first == S.root.a && c.k == S.root.g) return;
            pop_top();
        }
    }
    __device__ __forceinline__ void clean_top()
    {
        DCell c;
        clean_top(c);
    }

    // insert(node, h_new) (:236-248) on a wave-uniform cell: always appends an entry
    __device__ __forceinline__ void insert_uniform(int X, double hnew)
    {
        if (S.ne + 1 > S.entry_cap) { S.overflow = true; return; }
        DCell c = load_cell(S.cells, X);
        const uint32_t t = tag_of(c.cnt_t);
        if (t == T_NEW) c.k = hnew;
        else if (t == T_OPEN) c.k = fmin(c.k, hnew);
        else c.k = fmin(c.h, hnew);
        c.h = hnew;
        const int e = S.ne++;
        const uint32_t cnt = cnt_of(c.cnt_t);
        if (lane == 0) {
            if (cnt == 0) c.first = e;
            else S.nxt[c.last] = e;
            S.nxt[e] = -1;
        }
        if (cnt == 0) c.first = e;
        c.last = e;
        c.cnt_t = (T_OPEN << 24) | (cnt + 1u);
        if (lane == 0) store_cell(S.cells, X, c);
        S.open += 1;
        if (X == S.start) S.start_closed = false;
        heap16::wsync();
        Ent it;
        it.g = c.k;
        it.a = (uint32_t)c.first;
        it.b = (uint32_t)X;
        push(it);
    }

    __device__ __forceinline__ int process_state()
    {
        // ---- min_state: the earliest entry of the node minimising (k, first entry) ----
        DCell xc;  // the popped node's cell: clean_top's load (the heap pop does not touch cells)
        clean_top(xc);
        S.np++;  // EXPAND.append(node), None included (:165-167)
        if (S.open == 0) return PS_EMPTY;
        if (S.n == 0) return PS_OVER;  // cannot happen while S.open > 0
        const Ent top = S.root;
        const int X = (int)top.b;
        // the neighbours' cells load now, beside the heap pop (lanes 0..7, any in-grid neighbour;
        // getNeighbor's collision test only decides below whether a lane uses its cell)
        const int Xc0 = X == S.goal_slot ? S.goal_cell : X;
        const int x = Xc0 / H, y = Xc0 % H;
        // getNeighbor (:276-291) looks up self.map[node + motion] for all 8 motions before any
        // collision test, and self.map holds the in-grid cells only (env.py:34-35): processing a node
        // on the grid's border raises KeyError (only on a grid whose border cells are not walls)
        if (x == 0 || y == 0 || x == W - 1 || y == H - 1) {
            S.raise_cell = Xc0;
            return PS_RAISE;
        }
        const int nx = x + mdx, ny = y + mdy;
        const bool nin = lane < 8 && (unsigned)nx < (unsigned)W && (unsigned)ny < (unsigned)H;
        const int Y = nin ? nx * H + ny : 0;
        DCell yc = load_cell(S.cells, Y);
        uint32_t coll = occ2(occ, W, H, x, y) | occ2(occ, W, H, nx, ny);
        if (mdx != 0 && mdy != 0) coll = coll | occ2(occ, W, H, x, ny) | occ2(occ, W, H, nx, y);
        pop_top();
        const int Xc = X == S.goal_slot ? S.goal_cell : X;  // node.current
        const double k_old = xc.k;
        // delete (:250-259): CLOSED if OPEN, drop the first entry
        {
            uint32_t tg = tag_of(xc.cnt_t);
            if (tg == T_OPEN) tg = T_CLOSED;
            const int e = xc.first;
            xc.first = S.nxt[e];
            xc.cnt_t = (tg << 24) | (cnt_of(xc.cnt_t) - 1u);
            if (cnt_of(xc.cnt_t) == 0) xc.last = -1;
            S.open -= 1;
        }
        // ---- neighbours (getNeighbor, :276-291): lanes 0..7 in motion order ----
        const bool nb = lane < 8 && coll == 0u;
        const uint64_t nbm = ballot(nb) & 0xFFull;
        // RAISE (:177-183): scalar scan in motion order
        double hX = xc.h;
        int pX = xc.parent;
        if (k_old < hX) {
            for (uint64_t m = nbm; m; m &= m - 1) {
                const int l = __ffsll((long long)m) - 1;
                const double hy = rl_f64(yc.h, l);
                const double c = (l & 1) ? 1.4142135623730951 : 1.0;
                if (hy <= k_old && hX > hy + c) {
                    pX = (int)rl_u32((uint32_t)Y, l);
                    hX = hy + c;
                }
            }
        }
        // LOWER / else (:185-217): one decision per lane; kind 1 = insert(node_n, h_new), 2 = insert(node, h)
        int kind = 0;
        double hnew = 0.0;
        bool setpar = false;
        if (nb) {
            const uint32_t ty = tag_of(yc.cnt_t);
            const bool par_is_x = yc.parent == Xc;
            const double hc = hX + mcost;
            if (k_old == hX) {
                if (ty == T_NEW || (par_is_x && yc.h != hc) || (!par_is_x && yc.h > hc)) {
                    kind = 1; hnew = hc; setpar = true;
                }
            } else {
                if (ty == T_NEW || (par_is_x && yc.h != hc)) {
                    kind = 1; hnew = hc; setpar = true;
                } else if (!par_is_x && yc.h > hc) {
                    kind = 2;
                } else if (!par_is_x && hX > yc.h + mcost && ty == T_CLOSED && yc.h > k_old) {
                    kind = 1; hnew = yc.h;
                }
            }
        }
        const uint64_t insm = ballot(kind != 0);
        const int nins = __popcll(insm);
        if (S.ne + nins > S.entry_cap) return PS_OVER;
        const int myE = S.ne + __popcll(insm & ((1ull << lane) - 1ull));
        // insert(node_n, h_new) (:236-248) for lanes of kind 1 (distinct cells, independent)
        if (kind == 1) {
            const uint32_t ty = tag_of(yc.cnt_t);
            if (ty == T_NEW) yc.k = hnew;
            else if (ty == T_OPEN) yc.k = fmin(yc.k, hnew);
            else yc.k = fmin(yc.h, hnew);
            yc.h = hnew;
            if (setpar) yc.parent = Xc;
            const uint32_t cnt = cnt_of(yc.cnt_t);
            if (cnt == 0) yc.first = myE;
            else S.nxt[yc.last] = myE;
            S.nxt[myE] = -1;
            yc.last = myE;
            yc.cnt_t = (T_OPEN << 24) | (cnt + 1u);
            store_cell(S.cells, Y, yc);
        }
        // insert(node, node.h) for lanes of kind 2, in lane order (node is CLOSED here, so
        // k = min(h, h) = h the first time and min(k, h) = h after)
        const uint64_t xm = ballot(kind == 2);
        if (xm) {
            if (lane == 0) {
                uint32_t cnt = cnt_of(xc.cnt_t);
                for (uint64_t m = xm; m; m &= m - 1) {
                    const int l = __ffsll((long long)m) - 1;
                    const int e = S.ne + __popcll(insm & ((1ull << l) - 1ull));
                    if (cnt == 0) xc.first = e;
                    else S.nxt[xc.last] = e;
                    S.nxt[e] = -1;
                    xc.last = e;
                    cnt++;
                }
                xc.cnt_t = (T_OPEN << 24) | cnt;
            }
            xc.first = (int32_t)rl_u32((uint32_t)xc.first, 0);
            xc.last = (int32_t)rl_u32((uint32_t)xc.last, 0);
            xc.cnt_t = rl_u32(xc.cnt_t, 0);
            xc.k = hX;
        }
        xc.h = hX;
        xc.parent = pX;
        if (lane == 0) store_cell(S.cells, X, xc);
        S.ne += nins;
        S.open += nins;
        heap16::wsync();
        // heap pushes: every re-keyed cell (stale elements are skipped on pop), stored together and
        // sifted up only where below the parent (heap16::push_batch; the key is a total order)
        {
            const uint64_t pm = ballot(kind == 1);
            if (pm) {
                if (S.n + __popcll(pm) > S.heap_cap) {
                    S.overflow = true;
                } else {
                    Ent it;
                    it.g = yc.k;
                    it.a = (uint32_t)yc.first;
                    it.b = (uint32_t)Y;
                    key.derive(it);
                    S.n = heap16::push_batch(S.hp, key, S.n, pm, it, S.root, lane);
                }
            }
        }
        if (!S.overflow && cnt_of(xc.cnt_t) > 0) {
            Ent it;
            it.g = xc.k;
            it.a = (uint32_t)xc.first;
            it.b = (uint32_t)X;
            push(it);
        }
        if (S.overflow) return PS_OVER;
        // start.t after this processState
        if (X == S.start) S.start_closed = tag_of(xc.cnt_t) == T_CLOSED;
        if (ballot(kind == 1 && Y == S.start)) S.start_closed = false;
        return S.open == 0 ? PS_EMPTIED : PS_DONE;
    }
};

__device__ __forceinline__ bool coll2(const uint32_t* occ, int W, int H, int a, int b)
{
    const int x1 = a / H, y1 = a % H, x2 = b / H, y2 = b % H;
    uint32_t c = occ2(occ, W, H, x1, y1) | occ2(occ, W, H, x2, y2);
    if (x1 != x2 && y1 != y2) c = c | occ2(occ, W, H, x1, y2) | occ2(occ, W, H, x2, y1);
    return c;
}

// GraphSearcher.cost (graph_search.py:46-59): inf on collision, else Planner.dist of neighbours
__device__ __forceinline__ double cost2(const uint32_t* occ, int W, int H, int a, int b)
{
    if (coll2(occ, W, H, a, b)) return __builtin_inf();
    return (a / H != b / H && a % H != b % H) ? 1.4142135623730951 : 1.0;
}

// DStar.plan (:75-89) and then npress OnPress(x, y) calls (:102-134) per query.  Round r (0 = plan)
// writes cost / path / len(EXPAND) / status at [q][r]; presses at [q][npress][2].
__device__ __forceinline__ void dstar_run(const uint32_t* __restrict__ occ_in, int W, int H,
                                                   const int32_t* __restrict__ start_xy, const int32_t* __restrict__ goal_xy,
                                                   int nq, const int32_t* __restrict__ presses, int npress,
                                                   double* __restrict__ cost_out, int32_t* __restrict__ path_len_out,
                                                   int32_t* __restrict__ path_out, int path_cap,
                                                   int64_t* __restrict__ nproc_out, int32_t* __restrict__ status_out,
                                                   int64_t max_process, int* __restrict__ queue, uint4* __restrict__ spill_all,
                                                   int heap_cap, int lds_cap, DCell* __restrict__ cells_all,
                                                   int32_t* __restrict__ next_all, int entry_cap, uint32_t* __restrict__ occw_all,
                                                   int* __restrict__ ovf, int retry)
{
    // ovf (nullable): [0] queries whose heap / entry list outgrew this launch's capacity, [1] the
    // re-run's queue, [2..] their indices.  retry = 0: the first pass (appends to it); 1: the re-run
    // at the bound over that list
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = lane_id();
    const int worker = blockIdx.x;
    const int ncell = W * H;
    const int words = (ncell + 31) / 32;
    const size_t spill_n = (size_t)(heap_cap > lds_cap ? heap_cap - lds_cap : 0);
    Search2 S;
    S.hp = heap16::make_heap(smem, lds_cap, spill_all + (size_t)worker * spill_n, spill_n);
    S.cells = cells_all + (size_t)worker * (size_t)(ncell + 1);
    S.nxt = next_all + (size_t)worker * entry_cap;
    S.heap_cap = heap_cap;
    S.lds_cap = lds_cap;
    S.entry_cap = entry_cap;
    uint32_t* occw = npress > 0 ? occw_all + (size_t)worker * (size_t)words : nullptr;
    D2 d{npress > 0 ? (const uint32_t*)occw : occ_in, W, H, S, lane, 0, 0, c_dmx[lane & 7], c_dmy[lane & 7],
         (lane & 1) ? 1.4142135623730951 : 1.0, KeyD()};  // Planner.dist = hypot(1, 1) / hypot(1, 0)
    heap16::pop_lane_consts(lane, d.pop_jl, d.pop_ol);
    d.pop_w = heap16::walk6_consts(lane, d.pop_jl, d.pop_ol);
    const int R1 = npress + 1;

    for (;;) {
        int q;
        if (retry) {
            const int qi = next_query(ovf + 1, lane);
            if (qi >= uni(ovf[0])) break;
            q = uni(ovf[2 + qi]);
        } else {
            q = next_query(queue, lane);
            if (q >= nq) break;
        }
        bool hover = false;  // the heap / entry list outgrew the capacity (the re-run's case)
        const int sx = uni(start_xy[2 * q]), sy = uni(start_xy[2 * q + 1]);
        const int gx = uni(goal_xy[2 * q]), gy = uni(goal_xy[2 * q + 1]);
        if ((unsigned)sx >= (unsigned)W || (unsigned)sy >= (unsigned)H || (unsigned)gx >= (unsigned)W ||
            (unsigned)gy >= (unsigned)H) {
            // every lane stores the same values (no lane-0 block before the continue)
            for (int r = 0; r < R1; r++) {
                status_out[(size_t)q * R1 + r] = r == 0 ? PMP_REF_RAISES : -1;
                cost_out[(size_t)q * R1 + r] = 0.0;
                path_len_out[(size_t)q * R1 + r] = 0;
                nproc_out[(size_t)q * R1 + r] = 0;
            }
            continue;
        }
        if (occw) {
            for (int w = lane; w < words; w += 64) occw[w] = occ_in[w];
        }
        const int start = sx * H + sy, goal = gx * H + gy;
        // DStar.__init__ (:55-70): every cell NEW with h = k = inf, goal h = 0, insert(goal, 0)
        {
            DCell v;
            v.h = __builtin_inf();
            v.k = __builtin_inf();
            v.first = v.last = v.parent = -1;
            v.cnt_t = T_NEW << 24;
            for (int c = lane; c <= ncell; c += 64) store_cell(S.cells, c, v);
            heap16::wsync();
            if (lane == 0) {
                v.h = 0.0;
                store_cell(S.cells, start == goal ? ncell : goal, v);
            }
            heap16::wsync();
        }
        S.n = 0;
        S.open = 0;
        S.ne = 0;
        S.np = 0;
        S.start = start;
        S.goal_cell = goal;
        S.goal_slot = start == goal ? ncell : goal;
        S.start_closed = false;
        S.overflow = false;
        d.insert_uniform(S.goal_slot, 0.0);
        // ---- plan(): processState until the start is CLOSED (:84-87)
        int st = PMP_FOUND;
        int plen0 = 0;  // round 0's path_len when it raises: -2 = getNeighbor's KeyError (path[0] = the node)
        for (;;) {
            const int ps = d.process_state();
            if (ps == PS_OVER) { st = PMP_CAP_OVERFLOW; hover = true; break; }
            if (ps == PS_RAISE) { st = PMP_REF_RAISES; plen0 = -2; break; }
            if (ps != PS_DONE) { st = PMP_REF_RAISES; break; }  // min_k of an empty OPEN (:234)
            if (S.start_closed) break;
            if (max_process > 0 && S.np >= max_process) { st = PMP_CAP_OVERFLOW; break; }
        }
        for (int r = 0; r <= npress; r++) {
            int rst = st;
            double cost = 0.0;
            int plen = 0;
            int32_t* pth = path_out + ((size_t)q * R1 + r) * (size_t)path_cap;
            if (r == 0) {
                if (plen0 == -2) {
                    plen = -2;
                    if (lane == 0) pth[0] = S.raise_cell;
                }
                if (st == PMP_FOUND && lane == 0) {
                    // extractPath (:136-156): start -> goal through parents, cost via GraphSearcher.cost
                    int c = start;
                    pth[0] = c;
                    plen = 1;
                    while (c != goal) {
                        const int p = load_cell(S.cells, c).parent;
                        if (p < 0 || plen > ncell) { rst = PMP_REF_RAISES; break; }
                        cost += cost2(d.occ, W, H, c, p);
                        c = p;
                        if (plen < path_cap) pth[plen] = c;
                        plen++;
                    }
                    if (rst == PMP_FOUND && plen > path_cap) rst = PMP_PATH_OVERFLOW;
                }
                rst = uni(rst);
            } else if (st != PMP_FOUND) {
                rst = -1;  // not run: an earlier call raised or hit a cap
            } else {
                // OnPress(x, y) (:102-134) without the figure
                const int px = uni(presses[((size_t)q * npress + (r - 1)) * 2]);
                const int py = uni(presses[((size_t)q * npress + (r - 1)) * 2 + 1]);
                if (px < 0 || px > W - 1 || py < 0 || py > H - 1 || occ2(d.occ, W, H, px, py)) {
                    rst = PMP_NO_PATH;  // "Please choose right area!" / already an obstacle: nothing happens
                } else {
                    heap16::wsync();
                    if (lane == 0) {
                        const uint32_t c = (uint32_t)(px * H + py);
                        occw[c >> 5] |= 1u << (c & 31);
                    }
                    heap16::wsync();
                    S.np = 0;  // self.EXPAND = []
                    int node = start;
                    const int64_t bound = 4 * (int64_t)ncell + 4;
                    int64_t steps = 0;
                    while (node != goal) {
                        if (++steps > bound) { rst = PMP_CAP_OVERFLOW; break; }
                        const int p = load_cell(S.cells, node).parent;
                        if (p < 0) { rst = PMP_REF_RAISES; plen = -1; break; }  // self.map[None]: KeyError
                        if (coll2(d.occ, W, H, node, p)) {
                            // modify(node, node_parent) (:262-274): cost is inf (they collide)
                            if (tag_of(load_cell(S.cells, node).cnt_t) == T_CLOSED)
                                d.insert_uniform(node, load_cell(S.cells, p).h + __builtin_inf());
                            for (;;) {
                                const int ps = S.overflow ? PS_OVER : d.process_state();
                                if (ps == PS_OVER) { rst = PMP_CAP_OVERFLOW; hover = true; break; }
                                if (ps == PS_RAISE) {  // getNeighbor's KeyError: path_len -2, path[0] = the node
                                    rst = PMP_REF_RAISES;
                                    plen = -2;
                                    if (lane == 0) pth[0] = S.raise_cell;
                                    break;
                                }
                                if (ps == PS_EMPTIED) { rst = PMP_REF_RAISES; break; }
                                // an OPEN empty on entry makes processState return -1 forever: the
                                // reference's loop never ends
                                if (ps == PS_EMPTY) { rst = PMP_CAP_OVERFLOW; break; }
                                if (max_process > 0 && S.np >= max_process) { rst = PMP_CAP_OVERFLOW; break; }
                                // k_min >= node.h
                                d.clean_top();
                                if (S.root.g >= load_cell(S.cells, node).h) break;
                            }
                            if (rst != PMP_FOUND) break;
                            continue;
                        }
                        if (lane == 0 && plen < path_cap) pth[plen] = node;
                        plen++;
                        cost += cost2(d.occ, W, H, node, p);
                        node = p;
                    }
                    if (rst == PMP_FOUND && plen > path_cap) rst = PMP_PATH_OVERFLOW;
                    plen = uni(plen);
                }
                if (rst == PMP_REF_RAISES || rst == PMP_CAP_OVERFLOW) st = rst;
            }
            if (lane == 0) {
                status_out[(size_t)q * R1 + r] = rst;
                cost_out[(size_t)q * R1 + r] = cost;
                path_len_out[(size_t)q * R1 + r] = plen;
                nproc_out[(size_t)q * R1 + r] = rst == -1 ? 0 : S.np;  // a no-op press keeps EXPAND
            }
        }
        if (!retry && ovf && hover && lane == 0) {  // the re-run overwrites every output of q
            const int i = atomicAdd(ovf, 1);
            ovf[2 + i] = q;
        }
        heap16::wsync();
    }
}

// the first pass and the re-run at the bound, as two kernels (so a profile keys them apart)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void dstar_kernel(const uint32_t* __restrict__ occ_in, int W, int H,
                                                   const int32_t* __restrict__ start_xy, const int32_t* __restrict__ goal_xy,
                                                   int nq, const int32_t* __restrict__ presses, int npress,
                                                   double* __restrict__ cost_out, int32_t* __restrict__ path_len_out,
                                                   int32_t* __restrict__ path_out, int path_cap,
                                                   int64_t* __restrict__ nproc_out, int32_t* __restrict__ status_out,
                                                   int64_t max_process, int* __restrict__ queue, uint4* __restrict__ spill_all,
                                                   int heap_cap, int lds_cap, DCell* __restrict__ cells_all,
                                                   int32_t* __restrict__ next_all, int entry_cap, uint32_t* __restrict__ occw_all,
                                                   int* __restrict__ ovf)
{
    dstar_run(occ_in, W, H, start_xy, goal_xy, nq, presses, npress, cost_out, path_len_out, path_out, path_cap, nproc_out, status_out, max_process, queue, spill_all, heap_cap, lds_cap, cells_all, next_all, entry_cap, occw_all, ovf, 0);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void dstar_rerun_kernel(const uint32_t* __restrict__ occ_in, int W, int H,
                                                   const int32_t* __restrict__ start_xy, const int32_t* __restrict__ goal_xy,
                                                   int nq, const int32_t* __restrict__ presses, int npress,
                                                   double* __restrict__ cost_out, int32_t* __restrict__ path_len_out,
                                                   int32_t* __restrict__ path_out, int path_cap,
                                                   int64_t* __restrict__ nproc_out, int32_t* __restrict__ status_out,
                                                   int64_t max_process, int* __restrict__ queue, uint4* __restrict__ spill_all,
                                                   int heap_cap, int lds_cap, DCell* __restrict__ cells_all,
                                                   int32_t* __restrict__ next_all, int entry_cap, uint32_t* __restrict__ occw_all,
                                                   int* __restrict__ ovf)
{
    dstar_run(occ_in, W, H, start_xy, goal_xy, nq, presses, npress, cost_out, path_len_out, path_out, path_cap, nproc_out, status_out, max_process, queue, spill_all, heap_cap, lds_cap, cells_all, next_all, entry_cap, occw_all, ovf, 1);
}

}  // namespace

extern "C" int pmp_dstar2d_onpress_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int W, int H,
                                         const int32_t* start_xy, const int32_t* goal_xy, int nq, const int32_t* presses,
                                         int npress, double* cost, int32_t* path_len, int32_t* path, int path_cap,
                                         int64_t* n_process, int32_t* status, int64_t max_process)
{
    if (!ctx) return PMP_EINVAL;
    if (W < 1 || H < 1 || (int64_t)W * H > (1 << 26))
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_dstar2d_batch: W*H must be in [1, 2^26]");
    if (nq < 0 || path_cap < 1 || npress < 0 || (npress > 0 && !presses))
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_dstar2d_batch: bad nq/path_cap/npress/presses");
    if (nq == 0) return PMP_OK;
    if (!occ_bits || !start_xy || !goal_xy || !cost || !path_len || !path || !n_process || !status)
        return pmp_set_err(ctx, PMP_EINVAL, "pmp_dstar2d_batch: null pointer argument");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t ncell = (size_t)W * H;
    const size_t words = (ncell + 31) / 32;
    // per worker: 32 B cell state, 4 B per entry and 16 B per heap element beyond the LDS part.  The
    // bound is 4 entries / heap elements per cell; the first pass takes ctx->dstar_first_cap (default
    // one per cell: a third of the scratch, twice the workers at 512^2 within the budget), and a second
    // launch re-runs at the bound the queries whose heap or entry list outgrew it
    const size_t hb = 4 * ncell + 64;
    const int cap_full = (int)(hb > (size_t)(1 << 26) ? (size_t)(1 << 26) : hb);
    const size_t h1 = ctx->dstar_first_cap > 0 ? (size_t)ctx->dstar_first_cap : ncell + 64;
    const int cap1 = (int)std::min(h1, (size_t)cap_full);
    const bool two = cap1 < cap_full;
    const int per_cu = pmp_workers_per_cu(ctx, 16, nq);
    int lds_cap = (((160 * 1024) / pmp_lds_share(ctx, per_cu) - 256) / 16) & ~15;
    if (lds_cap > cap1) lds_cap = (cap1 + 15) & ~15;
    auto spill_of = [&](int cap) { return cap > lds_cap ? (size_t)(cap - lds_cap) : (size_t)0; };
    auto per_worker = [&](int cap) {
        return (ncell + 1) * sizeof(DCell) + (size_t)cap * 4 + spill_of(cap) * 16 + 4096 + (npress > 0 ? words * 4 : 0);
    };
    int workers = 256 * per_cu;
    const size_t budget = (size_t)48 << 30;  // per-context scratch of the workers
    const size_t max_workers = budget / per_worker(cap1);
    if ((size_t)workers > max_workers) workers = (int)(max_workers > 0 ? max_workers : 1);
    if (workers > nq) workers = nq;
    // the re-run: one worker per CU at most, within the first pass's allocations where they suffice
    int rw = 0;
    if (two) {
        rw = std::min(nq, 256);
        const size_t mw = budget / per_worker(cap_full);
        if ((size_t)rw > mw) rw = (int)(mw > 0 ? mw : 1);
    }
    const size_t spill_b = std::max((size_t)workers * spill_of(cap1), (size_t)rw * spill_of(cap_full)) * 16 + 16;
    const size_t cells_b = (size_t)std::max(workers, rw) * (ncell + 1) * sizeof(DCell) + 16;
    const size_t nxt_b = std::max((size_t)workers * cap1, (size_t)rw * cap_full) * 4 + 16;
    uint4* spill = (uint4*)pmp_scratch(ctx, SCR_AUX1, spill_b);
    DCell* cells = (DCell*)pmp_scratch(ctx, SCR_AUX2, cells_b);
    int32_t* nxt = (int32_t*)pmp_scratch(ctx, SCR_AUX3, nxt_b);
    int* queue = (int*)pmp_scratch(ctx, SCR_AUX0, 256);
    uint32_t* occw = npress > 0 ? (uint32_t*)pmp_scratch(ctx, SCR_AUX4, (size_t)std::max(workers, rw) * words * 4 + 16) : nullptr;
    int* ovf = two ? (int*)pmp_scratch(ctx, SCR_DSTAR_OVF, ((size_t)nq + 2) * 4 + 16) : nullptr;
    if (!spill || !cells || !nxt || !queue || (npress > 0 && !occw) || (two && !ovf)) return PMP_ENOMEM;
    hipStream_t s = (hipStream_t)stream;
    PMP_HIP_CHECK(ctx, hipMemsetAsync(queue, 0, 16, s));
    if (two) PMP_HIP_CHECK(ctx, hipMemsetAsync(ovf, 0, 8, s));
    hipLaunchKernelGGL(dstar_kernel, dim3(workers), dim3(64), (size_t)lds_cap * 16, s, occ_bits, W, H, start_xy, goal_xy,
                       nq, presses, npress, cost, path_len, path, path_cap, n_process, status, max_process, queue, spill,
                       cap1, lds_cap, cells, nxt, cap1, occw, ovf);
    if (two)
        hipLaunchKernelGGL(dstar_rerun_kernel, dim3(rw), dim3(64), (size_t)lds_cap * 16, s, occ_bits, W, H, start_xy, goal_xy,
                           nq, presses, npress, cost, path_len, path, path_cap, n_process, status, max_process, queue,
                           spill, cap_full, lds_cap, cells, nxt, cap_full, occw, ovf);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}

extern "C" int pmp_dstar2d_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int W, int H,
                                 const int32_t* start_xy, const int32_t* goal_xy, int nq, double* cost,
                                 int32_t* path_len, int32_t* path, int path_cap, int64_t* n_process, int32_t* status,
                                 int64_t max_process)
{
    return pmp_dstar2d_onpress_batch(ctx, stream, occ_bits, W, H, start_xy, goal_xy, nq, nullptr, 0, cost, path_len, path,
                                     path_cap, n_process, status, max_process);
}
