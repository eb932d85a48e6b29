// The A* 2D heap entry, shared by the three engines (astar2d.hip, astar2d_mq.hip, astar2d_sq.hip).
// The host re-runs a query that overflowed one engine's heap on another, so all three must build
// bit-identical heaps: the entry code, its accessors, the h order key and Node.__lt__ are defined
// here alone.  What differs per engine stays in its file: h_of_key (the multi-query engine's
// sqrt_int_rn against __dsqrt_rn), the heap structs and the choice-bit storage.
//
// Heap entry (12 B in LDS as SoA: f64 f[] | u32 cm[]):
//   cm = dx << 18 | dy << 4 | dir, with (dx, dy) = goal - cell as 14-bit two's-complement fields and
//   dir = the motion index (env.py:52-55) that reached the cell from its parent, 8 = start.  The
//   start entry stores (dx, dy) = (0, 0): its h is 0 (planner.py:15); its real cell is the query's.
#pragma once
#include "pmp_internal.h"

// motions in the order of env.py:52-55: (-1,0),(-1,1),(0,1),(1,1),(1,0),(1,-1),(0,-1),(-1,-1),
// as 2-bit fields of (m + 1); even = axis, odd = diagonal (jps2d.hip walks the same table)
constexpr uint32_t kMx1 = 0x1A90u, kMy1 = 0x01A9u;
__device__ __forceinline__ int mot_x(int d) { return (int)((kMx1 >> (2 * d)) & 3u) - 1; }
__device__ __forceinline__ int mot_y(int d) { return (int)((kMy1 >> (2 * d)) & 3u) - 1; }

// HEUR (a template parameter, so key computations carry no runtime branch): bits 0-1 = the
// heuristic -- 0 euclidean, 1 manhattan (GraphSearcher.h, graph_search.py:41-44), 2 zero (Dijkstra's
// node_n.h = 0, dijkstra.py:74); bit 2 = the Theta* entry layout: a 5-bit code instead of the 4-bit
// dir (0..7 the pusher's motion, 8 the start, 16 + motion = "path 2": the parent is the pusher's own
// parent, theta_star.py:104-108) and a 13-bit dy field (H <= 4096).  The single-query engine has no
// Theta* variant: its plain HEUR (0..2) selects the 4-bit layout.
constexpr int kThetaLayout = 4;
template <int HEUR> constexpr int hkind() { return HEUR & 3; }
template <int HEUR> constexpr int dbits() { return (HEUR & kThetaLayout) ? 5 : 4; }
template <int HEUR>
__device__ __forceinline__ uint32_t pack_cm(int dx, int dy, int dir)
{
    constexpr int S = dbits<HEUR>();
    return ((uint32_t)dx << 18) | (((uint32_t)dy & ((1u << (18 - S)) - 1u)) << S) | (uint32_t)dir;
}
template <int HEUR> __device__ __forceinline__ int cm_dx(uint32_t cm) { return (int)cm >> 18; }
template <int HEUR> __device__ __forceinline__ int cm_dy(uint32_t cm) { return (int)(cm << 14) >> (14 + dbits<HEUR>()); }
template <int HEUR> __device__ __forceinline__ int cm_dir(uint32_t cm) { return (int)(cm & ((1u << dbits<HEUR>()) - 1u)); }

// The order key of h: h order == hkey order (dx^2 + dy^2, or |dx| + |dy|), four integer ops from cm.
template <int HEUR>
__device__ __forceinline__ uint32_t hkey(uint32_t cm)
{
    if (hkind<HEUR>() == 2) return 0u;
    const int dx = cm_dx<HEUR>(cm), dy = cm_dy<HEUR>(cm);
    if (hkind<HEUR>() == 1) return (uint32_t)(abs(dx) + abs(dy));
    return (uint32_t)(__mul24(dx, dx) + __mul24(dy, dy));
}

// Node.__lt__ (node.py:51-54) on (f, hkey) pairs -- evaluated without short-circuit branches
__device__ __forceinline__ bool key_lt(double fa, uint32_t ka, double fb, uint32_t kb)
{
    return (fa < fb) | ((fa == fb) & (ka < kb));
}

typedef __attribute__((address_space(3))) double lds_f64;
typedef __attribute__((address_space(3))) uint32_t lds_u32;

// per lane: bit `lane` of mask ? a : b, as one v_cndmask (left to itself the compiler lowers such a
// select through 0/1 VGPRs, or predicates a load into registers another load still owns)
__device__ __forceinline__ uint32_t sel_lanes(uint64_t mask, uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, %2, %1, %3" : "=v"(r) : "v"(a), "v"(b), "s"(mask));
    return r;
}

// LDS atomic masked OR: word = (word & ~mask) | val, no return value (nothing waits on it).  LDS
// operations of one wave complete in order, so later ds_reads of the word see it.
__device__ __forceinline__ void ds_mskor(lds_u32* w, uint32_t mask, uint32_t val)
{
    asm volatile("ds_mskor_b32 %0, %1, %2" ::"v"((uint32_t)(uintptr_t)w), "v"(mask), "v"(val) : "memory");
}

// Orders this wave's LDS and HBM accesses across its lanes.  A wave's memory operations are
// performed in order, so wavefront scope needs no s_waitcnt (LLVM AMDGPU memory model): this is a
// compiler barrier only and never stalls on outstanding HBM stores.
__device__ __forceinline__ void wave_sync_mem() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }
