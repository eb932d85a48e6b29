// Host side of the trajectory entries that take a path either as f64 waypoints or as a 3D grid planner's
// cell ids (pmp_polytraj3d_batch, pmp_splinetraj3d_batch): the argument checks they share.  `fn` is the
// entry's name, the start of every message.  Checks of the kind (constraints, degree, the LDS limit) stay
// in the entry's file.
#pragma once
#include <cmath>
#include <string>
#include "pmp_internal.h"

inline bool finite3(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// How the points are sampled: the buffer, evaluate()'s times, generate()'s and resample()'s steps (the
// reference never leaves its sampling loop on a step that is not positive)
inline int traj_check_sampling(pmp_ctx* ctx, const char* fn, int point_cap, const double* eval_t, int n_eval,
                               double min_time_step, double sample_dt)
{
    if (point_cap < 1 || n_eval < 0 || (eval_t && n_eval < 1))
        return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": bad point_cap/n_eval");
    if (!std::isfinite(min_time_step) || !(min_time_step > 0) || !std::isfinite(sample_dt) || sample_dt < 0)
        return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": min_time_step must be > 0 and sample_dt >= 0, finite");
    return PMP_OK;
}

// Where the paths come from: exactly one of the two forms; cells: set to which
inline int traj_check_paths(pmp_ctx* ctx, const char* fn, const double* path_xyz, const int32_t* path_off,
                            const int32_t* cell_ids, const int32_t* path_len, int path_cap, int X, int Y, int Z,
                            bool& cells)
{
    const bool form_xyz = path_xyz && path_off;
    cells = cell_ids && path_len;
    if (form_xyz == cells)
        return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": give either path_xyz + path_off or cells + path_len");
    if (cells && (path_cap < 1 || X < 1 || Y < 1 || Z < 1 || (int64_t)X * Y * Z > INT32_MAX))
        return pmp_set_err(ctx, PMP_EINVAL, std::string(fn) + ": bad path_cap or grid size");
    return PMP_OK;
}
