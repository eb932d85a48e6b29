// libdevfn_probe.so: the shared device functions of the 2D grid planners, evaluated on their own (test
// infrastructure only, like pmp_oracle.c).  It includes the product's headers, so it runs the very
// functions the kernels inline, compiled with the product's flags; it holds no planner.  Every entry
// point takes device pointers and a stream, launches one kernel that evaluates pure functions, and
// writes nothing but its own output arrays (out[i] for i < n).  Returns the hipError_t of the launch.
// tests/test_devfn_gpu.py drives it through ctypes with torch tensors as buffers.
#include "../python_motion_planning_amd/csrc/astar2d_entry.h"

namespace {

// out[0] = how many k of [lo, lo + n) have sqrt_int_rn(k) != __dsqrt_rn((double)k) bit for bit;
// out[1 + j] = the j-th one found (j < 16, in the order the atomics land).  The host zeroes out[0..16].
__global__ void sqrt_sweep_kernel(uint32_t lo, unsigned long long n, unsigned long long* out)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t k = lo + (uint32_t)i;
        const long long a = __double_as_longlong(sqrt_int_rn(k));
        const long long b = __double_as_longlong(__dsqrt_rn((double)k));
        if (a != b) {
            const unsigned long long j = atomicAdd(&out[0], 1ull);
            if (j < 16) out[1 + j] = k;
        }
    }
}

// out[i] = sqrt_int_rn(k[i]); ref[i] = __dsqrt_rn((double)k[i])
__global__ void sqrt_values_kernel(const uint32_t* k, int n, double* out, double* ref)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = sqrt_int_rn(k[i]);
    ref[i] = __dsqrt_rn((double)k[i]);
}

// cm[i] = pack_cm<HEUR>(dx[i], dy[i], dir[i]); back[3 i ..] = cm_dx, cm_dy, cm_dir of it; hk[i] = hkey of it
template <int HEUR>
__global__ void entry_kernel(const int32_t* dx, const int32_t* dy, const int32_t* dir, int n, uint32_t* cm, int32_t* back,
                             uint32_t* hk)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = pack_cm<HEUR>(dx[i], dy[i], dir[i]);
    cm[i] = c;
    back[3 * i] = cm_dx<HEUR>(c);
    back[3 * i + 1] = cm_dy<HEUR>(c);
    back[3 * i + 2] = cm_dir<HEUR>(c);
    hk[i] = hkey<HEUR>(c);
}

// out[x * H + y] = cst_idx(x, y, cst_tiles_y(H)) (which = 0) or g_idx(x, y, g_tiles_y(H)) (which = 1)
__global__ void tile_kernel(int which, int W, int H, uint32_t* out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W * H) return;
    const int x = i / H, y = i % H;
    out[i] = which == 0 ? cst_idx(x, y, cst_tiles_y(H)) : g_idx(x, y, g_tiles_y(H));
}

int launched() { return (int)hipGetLastError(); }

}  // namespace

extern "C" int devfn_sqrt_sweep(void* stream, uint32_t lo, unsigned long long n, unsigned long long* out17)
{
    if (!out17 || (unsigned long long)lo + n > (1ull << 31)) return -1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(sqrt_sweep_kernel, dim3(256 * 8), dim3(256), 0, (hipStream_t)stream, lo, n, out17);
    return launched();
}

extern "C" int devfn_sqrt_values(void* stream, const uint32_t* k, int n, double* out, double* ref)
{
    if (!k || !out || !ref || n < 0) return -1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(sqrt_values_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, k, n, out, ref);
    return launched();
}

// heur: the HEUR template value of astar2d_entry.h (0 euclidean, 1 manhattan, 2 zero; + 4 = the Theta* layout)
extern "C" int devfn_entry(void* stream, int heur, const int32_t* dx, const int32_t* dy, const int32_t* dir, int n,
                           uint32_t* cm, int32_t* back, uint32_t* hk)
{
    if (!dx || !dy || !dir || !cm || !back || !hk || n < 0) return -1;
    if (n == 0) return 0;
    constexpr int TL = kThetaLayout;
    auto kern = heur == 0 ? entry_kernel<0> : heur == 1 ? entry_kernel<1> : heur == 2 ? entry_kernel<2>
              : heur == TL ? entry_kernel<TL> : heur == (TL | 1) ? entry_kernel<TL | 1>
              : heur == (TL | 2) ? entry_kernel<TL | 2> : nullptr;
    if (!kern) return -1;
    hipLaunchKernelGGL(kern, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, dx, dy, dir, n, cm, back, hk);
    return launched();
}

extern "C" int devfn_tile_index(void* stream, int which, int W, int H, uint32_t* out)
{
    if (!out || (which != 0 && which != 1) || W < 1 || H < 1 || W > 8192 || H > 8192) return -1;
    const int n = W * H;
    hipLaunchKernelGGL(tile_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, which, W, H, out);
    return launched();
}

// the slot sizes the launchers allocate for those index maps (host functions of pmp_internal.h)
extern "C" unsigned long long devfn_cst_tiled_bytes(int W, int H) { return cst_tiled_bytes(W, H); }
extern "C" unsigned long long devfn_g_slot_cells(int W, int H) { return g_slot_cells(W, H); }
