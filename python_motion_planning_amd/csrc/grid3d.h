// Grid helpers shared by the one-wave-per-query 3D kernels.  All four planners (astar3d.hip,
// jps3d.hip, dstar3d.hip, lpa3d.hip) take Grid3D's 26 motions, Planner3D.dist, the dimension limit
// and the LDS word type from here; astar3d.hip and jps3d.hip also the (f, h, counter) heap key, the
// occupancy bit of a voxel (from HBM or from the bitmap staged in LDS), the LDS occupancy threshold
// and the per-context scratch budget (dstar3d.hip and lpa3d.hip keep their own occupancy structs,
// threshold and budget).  The longest-first pre-pass the launchers use is pmp_lpt_order
// (lpt_order.hip), their workers per CU and LDS heap plan pmp_workers_per_cu and pmp_plan_lds
// (all three declared in pmp_internal.h).
#pragma once
#include "heap16.h"

namespace grid3d {

constexpr int kMaxDim3 = 256;

// Grid3D.motions (env3d.py:56-70), in the reference's order: kM3 for compile-time use (indexed by
// unrolled loop counters), c_m3 the same table in constant memory (indexed by a lane's motion)
struct Motions3 {
    int8_t m[26][3];
};
constexpr Motions3 kM3 = {{
    {-1, 0, 0}, {-1, 1, 0}, {0, 1, 0}, {1, 1, 0}, {1, 0, 0}, {1, -1, 0}, {0, -1, 0}, {-1, -1, 0},
    {0, 0, 1}, {0, 0, -1},
    {-1, 0, 1}, {-1, 1, 1}, {0, 1, 1}, {1, 1, 1}, {1, 0, 1}, {1, -1, 1}, {0, -1, 1}, {-1, -1, 1},
    {-1, 0, -1}, {-1, 1, -1}, {0, 1, -1}, {1, 1, -1}, {1, 0, -1}, {1, -1, -1}, {0, -1, -1}, {-1, -1, -1}}};
alignas(16) static __device__ __constant__ Motions3 c_m3 = kM3;  // aligned like an array of its size

using heap16::Ent;  // g = path cost, a = push counter, b = cm; derived f = g + h, hk = h order key

// (f, h, counter) tuple order of a_star3d.py:40,75.  f = tentative_g + h is computed once, at the
// push (set_f), and stored beside the entry; h's order key (an integer) is rebuilt from the cell.
struct Key3 {
    static constexpr bool kStoredF = true;
    int gx, gy, gz;
    int heur;  // 0 euclidean, 1 manhattan, 2 zero (Dijkstra3D: h = 0, dijkstra3d.py:34,83)
    int Y, Z;

    __device__ __forceinline__ uint32_t hkey(uint32_t b) const
    {
        const int x = (int)((b >> 21) & 255u), y = (int)((b >> 13) & 255u), z = (int)((b >> 5) & 255u);
        const int dx = abs(gx - x), dy = abs(gy - y), dz = abs(gz - z);
        return heur == 2 ? 0u : (heur == 1 ? (uint32_t)(dx + dy + dz) : (uint32_t)(dx * dx + dy * dy + dz * dz));
    }
    __device__ __forceinline__ void derive(Ent& e) const { e.hk = hkey(e.b); }
    // f = g + h exactly as node_n.g + node_n.h (math.sqrt of the integer square sum for euclidean)
    __device__ __forceinline__ void set_f(Ent& e) const
    {
        e.hk = hkey(e.b);
        e.f = heur == 2 ? e.g : (heur == 1 ? e.g + (double)e.hk : e.g + __dsqrt_rn((double)e.hk));
    }

    static __device__ __forceinline__ bool lt(const Ent& a, const Ent& b)
    {
        return (a.f < b.f) | ((a.f == b.f) & ((a.hk < b.hk) | ((a.hk == b.hk) & (a.a < b.a))));
    }
};

__device__ __forceinline__ bool occ3(const uint32_t* occ, int X, int Y, int Z, int x, int y, int z)
{
    if ((unsigned)x >= (unsigned)X || (unsigned)y >= (unsigned)Y || (unsigned)z >= (unsigned)Z) return true;
    const uint32_t c = ((uint32_t)x * (uint32_t)Y + (uint32_t)y) * (uint32_t)Z + (uint32_t)z;
    return (occ[c >> 5] >> (c & 31)) & 1u;
}

typedef __attribute__((address_space(3))) uint32_t lds_w32;

// occupancy bit, blocked outside the grid, from the per-query bitmap staged in LDS
__device__ __forceinline__ uint32_t occ3l(const lds_w32* occ, int X, int Y, int Z, int x, int y, int z)
{
    if ((unsigned)x >= (unsigned)X || (unsigned)y >= (unsigned)Y || (unsigned)z >= (unsigned)Z) return 1u;
    const uint32_t c = ((uint32_t)x * (uint32_t)Y + (uint32_t)y) * (uint32_t)Z + (uint32_t)z;
    return (occ[c >> 5] >> (c & 31)) & 1u;
}

constexpr int kOccLdsWords = 1024;  // grids up to 32768 cells keep their occupancy in LDS (4 KiB)

__device__ __forceinline__ double dist3(int dx, int dy, int dz)  // Planner3D.dist (planner3d.py:22-27)
{
    return __dsqrt_rn((double)(dx * dx + dy * dy + dz * dz));
}

// per-context scratch budget of the 3D planners (heap spill + closed state + any-voxel parents per worker)
// 48 GiB: the 20-per-CU 5,120 workers at C5 (2.09-2.11 M plans/s); 32 GiB fitted ~4,870 (2.05 M,
// tools/calls/r6_call53.sh)
constexpr size_t kScratchBudget3 = (size_t)48 << 30;

}  // namespace grid3d
