// Batched ant-colony planning for gfx950: ACO.plan() (global_planner/evolutionary_search/aco.py:65-166).  All
// f64, -ffp-contract=off, denormals kept (the compiler's default for f64).
//
// One wave64 per plan, `waves` of them per workgroup; the waves of a workgroup share nothing but the launch.
// Every draw's position in the random stream depends on all earlier draws, so a plan is sequential over
// iterations, ants and steps, and the generator itself runs in the kernel (mt19937_dev.h): its 624 words and
// the current ant's visited bitmap are the wave's LDS.  The pheromone double[W H][8] (cell, motion index: a
// cell's eight edges are one 64-byte line), the iteration's ant paths (uint16 cell ids) and their lengths are
// per-plan scratch in global memory.
//
// The reference's only powers are pheromone ** alpha and (1 / h) ** beta.  The second is tabulated on the host
// by CPython's own ** (heur); the first is x ** 1.0 = x or x ** 0.0 = 1.0 for the two alphas the entry takes.
// What is left is *, +, / and < on doubles, in the reference's order: the walk is the reference's bit for bit.
//
// A step: lanes 0..7 load the eight edges' pheromone, the neighbours' heuristic and visited bits at once; the
// left-to-right sums (prob_sum, then the running cp of the quotients) are taken in motion order from the
// lanes' terms; one draw; bisect_left over the candidates' cp as the reference's binary search, on the
// ballot of cp < r.  Evaporation, the deposit along a path, the bitmap clear and the twist are wave-wide.
#include <climits>
#include <cmath>
#include "pmp_internal.h"
#include "mt19937_dev.h"

namespace {

using namespace mtdev;

constexpr int kMaxWaves = 8;
constexpr int kDefaultWaves = 2;  // measured: DESIGN.md 3.13 (4096 default plans: 795 ms at 2, 797 at 4, 796 at 8, 916 at 1)
constexpr int kMaxCells = 65536;  // cell ids are uint16 in the path scratch; 8 KiB of visited bits

// env.motions (env.py:49-53): dx + 1 and dy + 1 of motion m, two bits each
constexpr uint32_t kDx = 0x1A90u, kDy = 0x01A9u;
__host__ __device__ __forceinline__ int motion_dx(int m) { return (int)((kDx >> (2 * m)) & 3u) - 1; }
__host__ __device__ __forceinline__ int motion_dy(int m) { return (int)((kDy >> (2 * m)) & 3u) - 1; }

enum : int { kBadBorder = 1, kBadHeur = 2, kBadEndpoint = 4, kBadTable = 8, kBadIndex = 16 };

__device__ __forceinline__ bool occ_at(const uint32_t* occ, uint32_t ci) { return ((occ[ci >> 5] >> (ci & 31u)) & 1u) != 0u; }

// The prologue: moves[cell] = the 8-bit mask of motions m for which isCollision(cell, cell + motions[m]) is
// false (evolutionary_search.py:61-87: target free and, for a diagonal, both side cells free; obstacles get 0),
// and the checks the entry refuses a launch by, OR-ed into *flags.
__global__ void aco_prologue(const uint32_t* occ, int W, int H, uint8_t* moves, const int32_t* start, const int32_t* goal,
                             int n_plans, const double* heur, int n_tables, const int32_t* heur_of, const uint32_t* mt_in,
                             int* flags)
{
    const int cells = W * H;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, gsz = (size_t)gridDim.x * blockDim.x;
    int bad = 0;
    for (size_t c = gid; c < (size_t)cells; c += gsz) {
        const int x = (int)(c / H), y = (int)(c % H);
        uint32_t mask = 0;
        if (!occ_at(occ, (uint32_t)c)) {
            if (x == 0 || y == 0 || x == W - 1 || y == H - 1) {
                bad |= kBadBorder;
            } else {
                for (int m = 0; m < 8; m++) {
                    const int dx = motion_dx(m), dy = motion_dy(m);
                    bool hit = occ_at(occ, (uint32_t)((x + dx) * H + y + dy));
                    if (dx != 0 && dy != 0)
                        hit = hit || occ_at(occ, (uint32_t)(x * H + y + dy)) || occ_at(occ, (uint32_t)((x + dx) * H + y));
                    if (!hit) mask |= 1u << m;
                }
            }
        }
        moves[c] = (uint8_t)mask;
    }
    for (size_t i = gid; i < (size_t)n_tables * cells; i += gsz)
        if (!occ_at(occ, (uint32_t)(i % cells)) && !std::isfinite(heur[i])) bad |= kBadHeur;
    for (size_t q = gid; q < (size_t)n_plans; q += gsz) {
        const int sx = start[2 * q], sy = start[2 * q + 1], gx = goal[2 * q], gy = goal[2 * q + 1];
        if (sx < 0 || sx >= W || sy < 0 || sy >= H || gx < 0 || gx >= W || gy < 0 || gy >= H ||
            occ_at(occ, (uint32_t)(sx * H + sy)) || occ_at(occ, (uint32_t)(gx * H + gy)))
            bad |= kBadEndpoint;
        if (heur_of[q] < 0 || heur_of[q] >= n_tables) bad |= kBadTable;
        if (mt_in[q * (size_t)kStateWords + kN] > (uint32_t)kN) bad |= kBadIndex;
    }
    if (bad) atomicOr(flags, bad);
}

struct aco_io {
    const uint8_t* moves;
    const int32_t *start, *goal;
    const double* heur;
    const int32_t* heur_of;
    const uint32_t* mt_in;
    int32_t *status, *best_len, *best_path, *n_cost, *cost_list;
    long long* draws;
    uint32_t* mt_out;
    int32_t *ant_found, *ant_len;  // the trace, or null
    double* pher;
    uint16_t* paths;
    int32_t* lens;
};

__device__ __forceinline__ void global_sync() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// cap = ceil(max_steps) + 1: the entries of a path; wave_words: the LDS words of one wave
__global__ __launch_bounds__(64 * kMaxWaves) void aco_kernel(pmp_aco_params P, int waves, int n_plans, int cap,
                                                             int vis_words, int wave_words, aco_io io)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int q = (int)blockIdx.x * waves + wave;
    if (q >= n_plans) return;  // the waves of a workgroup never meet at a barrier
    uint32_t* mt = sm + (size_t)wave * wave_words;
    uint32_t* vis = mt + kN;
    const int W = P.x_range, H = P.y_range, cells = W * H, K = cap - 1;
    const int s = uni(io.start[2 * q] * H + io.start[2 * q + 1]), g = uni(io.goal[2 * q] * H + io.goal[2 * q + 1]);
    const uint8_t* moves = io.moves;
    const double* heur = io.heur + (size_t)uni(io.heur_of[q]) * cells;
    double* pher = io.pher + (size_t)q * cells * 8;
    uint16_t* paths = io.paths + (size_t)q * P.n_ants * cap;
    int32_t* lens = io.lens + (size_t)q * P.n_ants;
    int32_t* best_path = io.best_path + (size_t)q * cap;
    int32_t* cost_list = io.cost_list + (size_t)q * P.max_iter;
    const bool use_pher = P.alpha != 0.0;
    const int my_off = motion_dx(lane & 7) * H + motion_dy(lane & 7);

    const uint32_t* mt_in = io.mt_in + (size_t)q * kStateWords;
    for (int i = lane; i < kN; i += 64) mt[i] = mt_in[i];
    int idx = uni((int)mt_in[kN]);
    if (idx > kN) idx = kN;  // the entry refuses such a state
    for (int e = lane; e < cells * 8; e += 64) pher[e] = ((moves[e >> 3] >> (e & 7)) & 1) ? 1.0 : 0.0;
    global_sync();
    mt_sync();

    long long draws = 0;
    int mn = INT_MAX, n_cost = 0, best_len = 0;
    bool index_error = false;
    for (int it = 0; it < P.max_iter && !index_error; it++) {
        for (int a = 0; a < P.n_ants && !index_error; a++) {
            for (int i = lane; i < vis_words; i += 64) vis[i] = 0u;
            uint16_t* path = paths + (size_t)a * cap;
            int c = s, len = 0, steps = 0;
            bool found = false;
            while (steps < K) {
                mt_sync();
                if (lane == 0) {
                    path[len] = (uint16_t)c;
                    vis[c >> 5] |= 1u << (c & 31);
                }
                len++;
                mt_sync();
                // the eight neighbours on lanes 0..7: c is a free cell, which the entry's border rule makes an
                // interior one, so every neighbour is a cell of the grid; clamped all the same
                int nb = c + my_off;
                nb = nb < 0 ? 0 : (nb >= cells ? cells - 1 : nb);
                double ph = 0.0, he = 0.0;
                uint32_t vw = 0u, mv = 0u;
                if (lane < 8) {
                    mv = moves[c];
                    he = heur[nb];
                    if (use_pher) ph = pher[(size_t)c * 8 + lane];
                    vw = vis[nb >> 5];
                }
                const bool open = lane < 8 && ((mv >> lane) & 1u) && !((vw >> (nb & 31)) & 1u);
                const uint32_t cand = (uint32_t)ballot(open);
                if (ballot(open && nb == g)) {  // the candidates collected before it are dropped without a draw
                    if (lane == 0) path[len] = (uint16_t)g;
                    len++;
                    found = true;
                    break;
                }
                const double t = use_pher ? ph * he : he;
                double ps = 0.0;
#pragma unroll
                for (int m = 0; m < 8; m++) {
                    const double tm = rl_f64(t, m);
                    ps = ((cand >> m) & 1u) ? ps + tm : ps;
                }
                if (ps == 0.0) break;  // a dead end, or every term underflowed
                const double qv = t / ps;
                double p0 = 0.0, cp = 0.0;
#pragma unroll
                for (int m = 0; m < 8; m++) {
                    const double qm = rl_f64(qv, m);
                    p0 = ((cand >> m) & 1u) ? p0 + qm : p0;
                    if (lane == m) cp = p0;
                }
                const double r = next_double(mt, idx, lane);
                draws++;
                // bisect_left(cp, r) over the candidates in motion order: bit k of lt = cp[k] < r
                const uint32_t less = (uint32_t)ballot(lane < 8 && cp < r) & cand;
                uint32_t lt = 0u;
                int n = 0;
#pragma unroll
                for (int m = 0; m < 8; m++)
                    if ((cand >> m) & 1u) {
                        lt |= ((less >> m) & 1u) << n;
                        n++;
                    }
                int lo = 0, hi = n;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if ((lt >> mid) & 1u) lo = mid + 1;
                    else hi = mid;
                }
                if (lo == n) {  // r > cp[-1]: the reference's list index raises
                    index_error = true;
                    break;
                }
                uint32_t rest = cand;
                for (int i = 0; i < lo; i++) rest &= rest - 1u;
                const int m = __builtin_ctz(rest);
                c += motion_dx(m) * H + motion_dy(m);
                steps++;
            }
            if (lane == 0) lens[a] = found ? len : -len;
            if (io.ant_found && lane == 0) {
                const size_t o = ((size_t)q * P.max_iter + it) * P.n_ants + a;
                io.ant_found[o] = found ? 1 : 0;
                io.ant_len[o] = len;
            }
        }
        if (index_error) break;
        global_sync();
        // pheromone deterioration, then the successful ants' deposits in ant order (aco.py:137-149)
        for (int e = lane; e < cells * 8; e += 64)
            if ((moves[e >> 3] >> (e & 7)) & 1) pher[e] = pher[e] * P.one_minus_rho;
        global_sync();
        int bpl = INT_MAX, bp = -1;
        for (int a = 0; a < P.n_ants; a++) {
            const int L = uni(lens[a]);
            if (L <= 0) continue;
            if (L < bpl) {
                bpl = L;
                bp = a;
            }
            const double add = P.Q / (double)L;
            const uint16_t* path = paths + (size_t)a * cap;
            for (int i = lane; i < L - 1; i += 64) {  // no cell twice in a path: the edges are distinct
                const int c1 = path[i], d = (int)path[i + 1] - c1;
                const int m = d == -H ? 0 : d == 1 - H ? 1 : d == 1 ? 2 : d == H + 1 ? 3 : d == H ? 4 : d == H - 1 ? 5 : d == -1 ? 6 : 7;
                double* e = pher + (size_t)c1 * 8 + m;
                *e = *e + add;
            }
            global_sync();
        }
        if (bpl < INT_MAX && bpl < mn) mn = bpl;
        if (mn < INT_MAX) {
            if (lane == 0) cost_list[n_cost] = mn;
            n_cost++;
            if (bpl < INT_MAX && bpl <= mn) {  // a later tie wins
                const uint16_t* path = paths + (size_t)bp * cap;
                for (int i = lane; i < bpl; i += 64) best_path[i] = path[i];
                best_len = bpl;
            }
        }
        global_sync();
    }
    mt_sync();
    uint32_t* mout = io.mt_out + (size_t)q * kStateWords;
    for (int i = lane; i < kN; i += 64) mout[i] = mt[i];
    if (lane == 0) {
        mout[kN] = (uint32_t)idx;
        io.status[q] = index_error ? PMP_REF_INDEX_ERROR : (best_len > 0 ? PMP_FOUND : PMP_NO_PATH);
        io.best_len[q] = best_len;
        io.n_cost[q] = n_cost;
        io.draws[q] = draws;
    }
}

__global__ void mt_doubles_kernel(const uint32_t* state_in, long long n, double* out, uint32_t* state_out)
{
    __shared__ uint32_t mt[kN];
    const int lane = lane_id();
    for (int i = lane; i < kN; i += 64) mt[i] = state_in[i];
    int idx = uni((int)state_in[kN]);
    if (idx > kN) idx = kN;
    mt_sync();
    for (long long i = 0; i < n; i++) {
        const double r = next_double(mt, idx, lane);
        if (lane == 0) out[i] = r;
    }
    mt_sync();
    for (int i = lane; i < kN; i += 64) state_out[i] = mt[i];
    if (lane == 0) state_out[kN] = (uint32_t)idx;
}

}  // namespace

extern "C" int pmp_aco_default_waves(void) { return kDefaultWaves; }
extern "C" int pmp_aco_max_waves(void) { return kMaxWaves; }

extern "C" int pmp_aco_path_cap(int x_range, int y_range)
{
    if (x_range < 1 || y_range < 1 || (int64_t)x_range * y_range > kMaxCells) return 0;
    // steps < x_range * y_range / 2 + max(x_range, y_range), a float: ceil of it choices, and the goal
    return (x_range * y_range + 1) / 2 + (x_range > y_range ? x_range : y_range) + 1;
}

extern "C" int pmp_aco_batch(pmp_ctx* ctx, void* stream, const pmp_aco_params* prm, const uint32_t* occ_bits, int n_plans,
                             const int32_t* starts, const int32_t* goals, const double* heur, int n_tables,
                             const int32_t* heur_of, const uint32_t* mt_state_in, int32_t* status, int32_t* best_len,
                             int32_t* best_path, int32_t* n_cost, int32_t* cost_list, int64_t* draws,
                             uint32_t* mt_state_out, int32_t* ant_found, int32_t* ant_len, double* pheromone,
                             uint16_t* paths, int32_t* ant_scratch)
{
    const std::string fn = "pmp_aco_batch";
    if (!ctx) return PMP_EINVAL;
    if (!prm) return pmp_set_err(ctx, PMP_EINVAL, fn + ": null params");
    if (prm->x_range < 1 || prm->y_range < 1) return pmp_set_err(ctx, PMP_EINVAL, fn + ": bad x_range / y_range");
    if ((int64_t)prm->x_range * prm->y_range > kMaxCells)
        return pmp_set_err(ctx, PMP_EINVAL, fn + ": grids above 65,536 cells are not taken");
    if (!(prm->alpha == 0.0 || prm->alpha == 1.0))
        return pmp_set_err(ctx, PMP_EINVAL, fn + ": alpha must be 0.0 or 1.0 (no bit-reproducible device pow)");
    if (prm->n_ants < 1) return pmp_set_err(ctx, PMP_EINVAL, fn + ": n_ants must be >= 1");
    if (prm->max_iter < 0) return pmp_set_err(ctx, PMP_EINVAL, fn + ": max_iter must be >= 0");
    if (!std::isfinite(prm->one_minus_rho) || !std::isfinite(prm->Q))
        return pmp_set_err(ctx, PMP_EINVAL, fn + ": one_minus_rho and Q must be finite");
    if (prm->waves < 0 || prm->waves > kMaxWaves) return pmp_set_err(ctx, PMP_EINVAL, fn + ": waves must be 0 (default) .. 8");
    if (n_plans < 0 || n_tables < 0) return pmp_set_err(ctx, PMP_EINVAL, fn + ": bad n_plans / n_tables");
    if (n_plans == 0) return PMP_OK;
    if (n_tables < 1) return pmp_set_err(ctx, PMP_EINVAL, fn + ": no heuristic table");
    if (!occ_bits || !starts || !goals || !heur || !heur_of || !mt_state_in || !status || !best_len || !best_path || !n_cost ||
        (!cost_list && prm->max_iter > 0) || !draws || !mt_state_out || (!ant_found != !ant_len) || !pheromone || !paths ||
        !ant_scratch)
        return pmp_set_err(ctx, PMP_EINVAL, fn + ": null pointer argument");
    const int W = prm->x_range, H = prm->y_range, cells = W * H, cap = pmp_aco_path_cap(W, H);
    hipStream_t s = (hipStream_t)stream;
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    // moves[cells] and the flag word behind it
    const size_t flag_off = ((size_t)cells + 15) & ~(size_t)15;
    uint8_t* moves = (uint8_t*)pmp_scratch(ctx, SCR_AUX0, flag_off + 16);
    if (!moves) return PMP_ENOMEM;
    int* flags = (int*)(moves + flag_off);
    PMP_HIP_CHECK(ctx, hipMemsetAsync(flags, 0, sizeof(int), s));
    const size_t work = std::max((size_t)n_tables * cells, (size_t)n_plans);
    const int blocks = (int)std::min<size_t>((work + 255) / 256, 4096);
    hipLaunchKernelGGL(aco_prologue, dim3(blocks), dim3(256), 0, s, occ_bits, W, H, moves, starts, goals, n_plans, heur,
                       n_tables, heur_of, mt_state_in, flags);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    // the refusals that depend on device data: one word back, one wait on the stream
    int bad = 0;
    PMP_HIP_CHECK(ctx, hipMemcpyAsync(&bad, flags, sizeof(int), hipMemcpyDeviceToHost, s));
    PMP_HIP_CHECK(ctx, hipStreamSynchronize(s));
    if (bad & kBadBorder)
        return pmp_set_err(ctx, PMP_EINVAL, fn + ": a free cell on the grid's border (the reference's ant steps outside the "
                                                 "grid there and dies with KeyError)");
    if (bad & kBadEndpoint) return pmp_set_err(ctx, PMP_EINVAL, fn + ": a start or goal outside the grid or in an obstacle");
    if (bad & kBadTable) return pmp_set_err(ctx, PMP_EINVAL, fn + ": heur_of names no table");
    if (bad & kBadHeur) return pmp_set_err(ctx, PMP_EINVAL, fn + ": a non-finite heuristic entry for a free cell");
    if (bad & kBadIndex) return pmp_set_err(ctx, PMP_EINVAL, fn + ": an MT19937 index above 624");
    const int waves = prm->waves ? prm->waves : kDefaultWaves;
    const int vis_words = (cells + 31) / 32;
    const int wave_words = (kN + vis_words + 3) & ~3;
    aco_io io;
    io.moves = moves;
    io.start = starts;
    io.goal = goals;
    io.heur = heur;
    io.heur_of = heur_of;
    io.mt_in = mt_state_in;
    io.status = status;
    io.best_len = best_len;
    io.best_path = best_path;
    io.n_cost = n_cost;
    io.cost_list = cost_list;
    io.draws = (long long*)draws;
    io.mt_out = mt_state_out;
    io.ant_found = ant_found;
    io.ant_len = ant_len;
    io.pher = pheromone;
    io.paths = paths;
    io.lens = ant_scratch;
    hipLaunchKernelGGL(aco_kernel, dim3((n_plans + waves - 1) / waves), dim3(64 * waves), (size_t)waves * wave_words * 4, s,
                       *prm, waves, n_plans, cap, vis_words, wave_words, io);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}

extern "C" int pmp_mt19937_doubles(pmp_ctx* ctx, void* stream, const uint32_t* state_in, int64_t n, double* out,
                                   uint32_t* state_out)
{
    const std::string fn = "pmp_mt19937_doubles";
    if (!ctx) return PMP_EINVAL;
    if (n < 0) return pmp_set_err(ctx, PMP_EINVAL, fn + ": bad n");
    if (!state_in || !state_out || (!out && n > 0)) return pmp_set_err(ctx, PMP_EINVAL, fn + ": null pointer argument");
    PMP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(mt_doubles_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state_in, (long long)n, out, state_out);
    PMP_HIP_CHECK(ctx, hipGetLastError());
    return PMP_OK;
}
