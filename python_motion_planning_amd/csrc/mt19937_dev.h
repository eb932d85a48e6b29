// MT19937 as CPython's `random` runs it (Modules/_randommodule.c: genrand_uint32, random_random), for one
// wave64 whose 624 state words lie in LDS: the twist, the tempering and random.random()'s double.  Nothing
// else: seeding stays on the host, the state comes from random.getstate().
//
// The twist is mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ (y & 1 ? 0x9908b0df : 0) with
// y = (mt[k] & 0x80000000) | (mt[(k + 1) % 624] & 0x7fffffff), for k ascending.  Word k reads k + 1 before it
// is replaced, k + 397 before it is replaced while k < 227, and the replaced k - 227 from then on; the last
// word reads the replaced word 0.  So the three spans 0..226, 227..453, 454..623 depend on each other only
// through words at least 227 back, and 64 consecutive words can be done at once as long as a chunk reads all
// its inputs before it writes: ten chunks of 64, ascending.
#pragma once
#include <cstdint>

namespace mtdev {

constexpr int kN = 624;
constexpr int kM = 397;
constexpr int kStateWords = kN + 1;  // the words and the index, as random.getstate()[1]

__device__ __forceinline__ void mt_sync() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// All 64 lanes of the wave call this together.
__device__ inline void twist(uint32_t* mt, int lane)
{
    for (int base = 0; base < kN; base += 64) {
        const int k = base + lane;
        uint32_t v = 0;
        if (k < kN) {
            const int k1 = k + 1 == kN ? 0 : k + 1;
            const int km = k + kM >= kN ? k + kM - kN : k + kM;
            const uint32_t y = (mt[k] & 0x80000000u) | (mt[k1] & 0x7fffffffu);
            v = mt[km] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        mt_sync();
        if (k < kN) mt[k] = v;
        mt_sync();
    }
}

// genrand_uint32: idx is wave-uniform, 0..624 (624: twist first).  Every lane returns the word.
__device__ __forceinline__ uint32_t next_u32(uint32_t* mt, int& idx, int lane)
{
    if (idx >= kN) {
        twist(mt, lane);
        idx = 0;
    }
    uint32_t y = mt[idx++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// random.random(): (a * 2^26 + b) / 2^53 from the top 27 and 26 bits of two outputs; exact in f64
__device__ __forceinline__ double next_double(uint32_t* mt, int& idx, int lane)
{
    const uint32_t a = next_u32(mt, idx, lane) >> 5;
    const uint32_t b = next_u32(mt, idx, lane) >> 6;
    return ((double)a * 67108864.0 + (double)b) * (1.0 / 9007199254740992.0);
}

}  // namespace mtdev
