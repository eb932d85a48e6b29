// Longest-first schedule of a batch: counting sort of the queries by descending start-goal distance
// (a query's expansions grow ~ with distance^2, so the longest queries start first and the short ones
// fill the tail).  The one pre-pass of every persistent-worker planner, 2D (astar2d.hip, jps2d.hip) and
// 3D (astar3d.hip, jps3d.hip, dstar3d.hip, lpa3d.hip).
#include <cmath>
#include "pmp_internal.h"

namespace {

// in double (endpoints may lie far outside the grid: the kernels report those queries, this
// pre-pass must only stay in range), clamped to the histogram [0, nb - 1] by the callers
template <int DIMS>
__device__ __forceinline__ int lpt_key(const int32_t* s, const int32_t* g, int q)
{
    const double dx = (double)s[DIMS * q] - g[DIMS * q], dy = (double)s[DIMS * q + 1] - g[DIMS * q + 1];
    double d2 = dx * dx + dy * dy;
    if constexpr (DIMS == 3) {
        const double dz = (double)s[3 * q + 2] - g[3 * q + 2];
        d2 = d2 + dz * dz;
    }
    const double d = __dsqrt_rn(d2);
    return d < 2147483647.0 ? (int)d : 2147483647;
}

template <int DIMS>
__global__ void lpt_hist(const int32_t* s, const int32_t* g, int nq, int nb, int* hist)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq) atomicAdd(&hist[min(lpt_key<DIMS>(s, g, q), nb - 1)], 1);
}

// offsets[k] = number of queries with a larger key (descending order); one thread, nb <= 16384
__global__ void lpt_scan(int nb, int* hist)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int run = 0;
    for (int k = nb - 1; k >= 0; k--) {
        const int c = hist[k];
        hist[k] = run;
        run += c;
    }
}

template <int DIMS>
__global__ void lpt_scatter(const int32_t* s, const int32_t* g, int nq, int nb, int* offs, int32_t* order)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq) order[atomicAdd(&offs[min(lpt_key<DIMS>(s, g, q), nb - 1)], 1)] = q;
}

}  // namespace

int pmp_lpt_order(pmp_ctx* ctx, hipStream_t s, int dims, const int32_t* start, const int32_t* goal, int nq,
                  const int* extent, int workers, int32_t** order)
{
    *order = nullptr;
    if (!ctx->astar_lpt || nq <= workers) return PMP_OK;
    double diag2 = 0.0;
    for (int i = 0; i < dims; i++) diag2 += (double)extent[i] * extent[i];
    const int nb = (int)ceil(sqrt(diag2)) + 1;
    int* hist = (int*)pmp_scratch(ctx, SCR_PDIR, sizeof(int) * ((size_t)nb + (size_t)nq));
    if (!hist) return PMP_ENOMEM;
    int32_t* ord = hist + nb;
    PMP_HIP_CHECK(ctx, hipMemsetAsync(hist, 0, sizeof(int) * (size_t)nb, s));
    const dim3 grid((nq + 255) / 256), block(256);
    auto hist_k = dims == 3 ? lpt_hist<3> : lpt_hist<2>;
    auto scatter_k = dims == 3 ? lpt_scatter<3> : lpt_scatter<2>;
    hipLaunchKernelGGL(hist_k, grid, block, 0, s, start, goal, nq, nb, hist);
    hipLaunchKernelGGL(lpt_scan, dim3(1), dim3(64), 0, s, nb, hist);
    hipLaunchKernelGGL(scatter_k, grid, block, 0, s, start, goal, nq, nb, hist, ord);
    *order = ord;
    return PMP_OK;
}
