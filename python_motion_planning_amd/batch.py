"""Batched entry points over the C-ABI (include/pmp.h).  Inputs/outputs are torch device tensors.

These are the calls the drop-in planner classes, the bench and the parity tests go through;
each one launches the gfx950 kernels of libpmp_hip.so asynchronously on the current stream.

The grid-search and sampling wrappers are each: intake, allocate, one C call, _lib.check, extras, return.
What they share is here once: _open (torch, library, context), _occ2d / _occ3d_bits (occupancy intake),
_endpoints (start / goal upload), _records (the cost / path_len / path / count / status block and its
optional blocks), _manhattan and _path_cap; the sampling trio has _sample_inputs and _tree_outputs.  The C
call stays written out in each wrapper: its argument order is the ABI.  query0 is the read-back of the
drop-in classes.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib
from .env import pack_bits


def _dev(torch, a, dtype):
    if isinstance(a, torch.Tensor):
        return a.to(device="cuda", dtype=dtype).contiguous()
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def occ_bits_device(occ, torch=None):
    """uint8 [W, H] (x-major) numpy occupancy -> bit-packed uint32 device tensor (as int32)."""
    torch = torch or _lib.device_check()
    words = pack_bits(occ)
    return torch.as_tensor(words.view(np.int32), device="cuda")


def _open():
    """(torch, the loaded library, the context): raises PMPError without a HIP device."""
    return _lib.device_check(), _lib.load_library(), _lib.context()


def _occ2d(torch, occ, occ_bits=None):
    """(occ_bits, W, H) of a 2D occupancy: a uint8 [W, H] array (x-major), a Grid, or, with occ_bits
    given (device words, used as they are), anything with the shape: (W, H) itself or the array."""
    if occ_bits is not None:
        W, H = (occ if isinstance(occ, tuple) else occ.shape)[:2]
    elif hasattr(occ, "occupancy_words"):  # a Grid
        W, H = occ.x_range, occ.y_range
        occ_bits = torch.as_tensor(occ.occupancy_words().view(np.int32), device="cuda")
    else:
        occ = np.asarray(occ)
        W, H = occ.shape[:2]
        occ_bits = occ_bits_device(occ, torch)
    return occ_bits, int(W), int(H)


def _occ3d_bits(torch, occ, occ_bits=None):
    """(device words, per_query, (X, Y, Z)) of a shared [X, Y, Z] or per-query [nq, X, Y, Z] grid; with
    occ_bits given, `occ` only supplies the shape."""
    shape = tuple(occ) if isinstance(occ, tuple) else np.asarray(occ).shape
    per_query = len(shape) == 4
    if occ_bits is None:
        occ = np.asarray(occ)
        words = np.stack([pack_bits(o) for o in occ]) if per_query else pack_bits(occ)
        occ_bits = torch.as_tensor(np.ascontiguousarray(words).view(np.int32), device="cuda")
    return occ_bits, per_query, tuple(int(d) for d in shape[-3:])


def _endpoints(torch, starts, goals, d, dtype):
    """(s, g, nq): starts and goals as [nq, d] device tensors of dtype."""
    s = _dev(torch, starts, dtype).reshape(-1, d)
    return s, _dev(torch, goals, dtype).reshape(-1, d), int(s.shape[0])


def _manhattan(heuristic: str) -> int:
    """The C entries' heuristic flag: 1 = manhattan, 0 = euclidean."""
    return 1 if heuristic == "manhattan" else 0


def _path_cap(path_cap, cells, bound=1 << 16):
    """The caller's path_cap, else room for every cell once, up to bound (None: unbounded)."""
    if path_cap is not None:
        return int(path_cap)
    return cells + 1 if bound is None else min(cells + 1, bound)


# the per-query blocks a wrapper may attach: dtype and width (None: the capacity the wrapper gives)
_OPTIONAL = dict(expand=("int32", None), expand_parent=("int32", None), expand_g=("float64", None),
                 counters=("int64", 4))


def _records(torch, lead, path_cap, count="n_expanded", count_dtype="int32", path_lead=None, **optional):
    """The record block of a grid planner: cost f64, status i32 and the count column of shape lead ((nq,),
    or (nq, R) with a record per round), path_len i32 and path i32 [.., path_cap] of shape path_lead (lead
    unless given).  optional: name=capacity (counters=flag) for each per-query block the wrapper has
    (_OPTIONAL), [nq, capacity] or None when that is 0 / False.  Nothing is initialised: the kernels write
    every record.  Sizes go to torch.empty as separate integers: that overload parses faster than a tuple,
    and on a small batch these allocations are most of the wrapper's host time."""
    path_lead = lead if path_lead is None else path_lead
    out = dict(cost=torch.empty(*lead, dtype=torch.float64, device="cuda"),
               path_len=torch.empty(*path_lead, dtype=torch.int32, device="cuda"),
               path=torch.empty(*path_lead, path_cap, dtype=torch.int32, device="cuda"),
               status=torch.empty(*lead, dtype=torch.int32, device="cuda"))
    out[count] = torch.empty(*lead, dtype=getattr(torch, count_dtype), device="cuda")
    for k, cap in optional.items():
        dtype, width = _OPTIONAL[k]
        out[k] = torch.empty(lead[0], width or cap, dtype=getattr(torch, dtype), device="cuda") if cap else None
    return out


def query0(r, key, n, k=None):
    """The first n entries of query 0's `key` (of its round or tree k, where it has them) in a result dict,
    as numpy: what the drop-in classes read back."""
    return r[key][((0,) if k is None else (0, k)) + (slice(n),)].cpu().numpy()


def astar2d_batch(occ, starts, goals, heuristic: str = "euclidean", path_cap: int | None = None,
                  expand_cap: int = 0, counters: bool = False, occ_bits=None, reserve_slots: int | None = None,
                  heap_cap: int = 0, retry_overflow: bool = True, algo: str = "astar"):
    """Batched AStar.plan (a_star.py:39-83); algo "dijkstra" / "gbfs" run Dijkstra.plan
    (dijkstra.py:36-85) / GBFS.plan (gbfs.py:36-86) on the same kernel (pmp_graph2d_batch).

    occ: numpy uint8 [W, H] (or pass occ=(W, H) with a prebuilt `occ_bits` device tensor).
    starts, goals: [nq, 2] int (numpy or device tensors).
    Returns dict of device tensors: cost f64 [nq], path_len i32 [nq], path i32 [nq, path_cap]
    (cell ids x*H+y, goal first), n_expanded i32, status i32, optional expand / counters.

    A query whose heap outgrows the reserved capacity stops with STATUS_CAP_OVERFLOW; with
    retry_overflow those queries are planned again on the GPU with the full bound (8 W H + 8
    entries) on fewer workers -- one host sync to read the statuses.
    """
    torch, L, ctx = _open()
    occ_bits, W, H = _occ2d(torch, occ, occ_bits)
    s, g, nq = _endpoints(torch, starts, goals, 2, torch.int32)
    path_cap = _path_cap(path_cap, W * H)
    out = _records(torch, (nq,), path_cap, expand=expand_cap, counters=counters)
    if reserve_slots:
        _lib.check(ctx, L.pmp_astar2d_reserve(ctx, W, H, int(reserve_slots), int(heap_cap)), "pmp_astar2d_reserve")
    rc = L.pmp_graph2d_batch(ctx, _lib.stream_ptr(), _lib.ALGOS[algo], occ_bits.data_ptr(), W, H,
                             _manhattan(heuristic), s.data_ptr(), g.data_ptr(), nq,
                             out["cost"].data_ptr(), out["path_len"].data_ptr(), out["path"].data_ptr(), path_cap,
                             out["n_expanded"].data_ptr(), _lib.ptr(out["expand"]), int(expand_cap),
                             _lib.ptr(out["counters"]), out["status"].data_ptr())
    _lib.check(ctx, rc, "pmp_graph2d_batch")
    if retry_overflow:
        redo = torch.nonzero(out["status"] == _lib.STATUS_CAP_OVERFLOW).flatten()
        if redo.numel():
            r = astar2d_full_bound((W, H), s[redo], g[redo], heuristic, path_cap, expand_cap, counters, occ_bits,
                                   algo=algo)
            for k in ("cost", "path_len", "path", "n_expanded", "status", "expand", "counters"):
                if out[k] is not None:
                    out[k][redo] = r[k]
    out["W"], out["H"] = W, H
    return out


def astar2d_full_bound(occ, starts, goals, heuristic="euclidean", path_cap=None, expand_cap=0, counters=False,
                       occ_bits=None, algo="astar"):
    """The overflow re-plan: the queries (a few) planned with the full heap bound (8 W H + 8 entries,
    which no search exceeds) on at most 256 workers, then the context's geometry restored as it was --
    the host's own reservation (its explicit heap_cap, or the default when it asked for none, so the
    engine choice of later batches is unchanged) or launch-sized scratch."""
    W, H = (int(v) for v in (occ if isinstance(occ, tuple) else occ.shape)[:2])
    L, ctx = _lib.load_library(), _lib.context()
    nq = int(starts.shape[0])
    geo = np.zeros(6, np.int32)  # the geometry in force, restored after the re-run
    _lib.check(ctx, L.pmp_astar2d_geometry(ctx, geo.ctypes.data), "pmp_astar2d_geometry")
    _lib.check(ctx, L.pmp_astar2d_reserve(ctx, W, H, max(1, min(nq, 256)), 8 * W * H + 8), "pmp_astar2d_reserve")
    try:
        return astar2d_batch(occ if occ_bits is None else (W, H), starts, goals, heuristic, path_cap, expand_cap,
                             counters, occ_bits, retry_overflow=False, algo=algo)
    finally:
        if geo[5] or not geo[0]:  # sized by the launches: keep it that way (grows with the batches)
            _lib.check(ctx, L.pmp_astar2d_reserve_auto(ctx), "pmp_astar2d_reserve_auto")
        else:  # the host's own reservation, with the capacity it asked for (0 = the default)
            cap = int(geo[3]) if geo[4] & 2 else 0
            _lib.check(ctx, L.pmp_astar2d_reserve(ctx, int(geo[0]), int(geo[1]), int(geo[2]), cap),
                       "pmp_astar2d_reserve")


_ONE = {}


class SingleQuery:
    """One drop-in query (AStar.plan, a_star.py:39-83) with one host round trip: start/goal go up in
    one pinned copy, the kernel writes (status, n_expanded, path_len | path | CLOSED records) into one
    int32 device block, and the block comes back in one pinned copy and one stream sync.  The
    buffers are kept per (context, capacities) and reused call after call."""

    def __init__(self, torch, path_cap: int, expand_cap: int) -> None:
        self.path_cap, self.expand_cap = path_cap, expand_cap
        n = 4 + path_cap + expand_cap
        self.dev = torch.empty(n, dtype=torch.int32, device="cuda")
        self.host = torch.empty(n, dtype=torch.int32, pin_memory=True)
        self.sg_host = torch.empty(4, dtype=torch.int32, pin_memory=True)
        self.sg_dev = torch.empty(4, dtype=torch.int32, device="cuda")
        self.cost = torch.empty(1, dtype=torch.float64, device="cuda")

    def launch(self, torch, W: int, H: int, occ_bits, start, goal, heuristic: str, algo: str) -> None:
        L, ctx = _lib.load_library(), _lib.context()
        self.sg_host.numpy()[:] = (start[0], start[1], goal[0], goal[1])
        self.sg_dev.copy_(self.sg_host, non_blocking=True)
        d, pc = self.dev.data_ptr(), self.path_cap
        rc = L.pmp_graph2d_batch(ctx, _lib.stream_ptr(), _lib.ALGOS[algo], occ_bits.data_ptr(), W, H,
                                 _manhattan(heuristic), self.sg_dev.data_ptr(),
                                 self.sg_dev.data_ptr() + 8, 1, self.cost.data_ptr(), d + 8, d + 16, pc, d + 4,
                                 d + 16 + 4 * pc, self.expand_cap, None, d)
        _lib.check(ctx, rc, "pmp_graph2d_batch")
        self.host.copy_(self.dev, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()

    def result(self):
        """(status, n_expanded, path cells goal->start, CLOSED records) as numpy, after the sync."""
        self.event.synchronize()
        h = self.host.numpy()
        st, nexp, plen = int(h[0]), int(h[1]), int(h[2])
        path = h[4: 4 + min(max(plen, 0), self.path_cap)].copy()
        exp = h[4 + self.path_cap: 4 + self.path_cap + min(max(nexp, 0), self.expand_cap)].view(np.uint32).copy()
        return st, nexp, plen, path, exp


def single_query(torch, path_cap: int, expand_cap: int) -> SingleQuery:
    key = (_lib.context(), path_cap, expand_cap)
    q = _ONE.get(key)
    if q is None:
        if len(_ONE) > 16:
            _ONE.clear()
        q = _ONE[key] = SingleQuery(torch, path_cap, expand_cap)
    return q


_RECORDS = ("cost", "path_len", "path", "n_expanded", "status")


def astar2d_sharded(occ, starts, goals, dist=None, path_cap: int | None = None, algo: str = "astar", **kw):
    """One batch of 2D grid queries split over all ranks of the process group `dist` (one GPU each):
    every rank plans its longest-first round-robin share on its own GPU with astar2d_batch and every
    rank returns the full batch's records (cost, path_len, path, n_expanded, status) in input order,
    gathered with one all_gather per field over RCCL.  dist=None: one rank."""
    from . import shard

    torch = _lib.device_check()
    occ_bits, W, H = _occ2d(torch, occ)

    def plan(s, g):
        r = astar2d_batch((W, H), s, g, path_cap=path_cap, occ_bits=occ_bits, algo=algo, **kw)
        return {k: r[k] for k in _RECORDS}

    return shard.run_sharded(dist, plan, np.asarray(starts), np.asarray(goals), device="cuda")


def astar3d_sharded(occ, starts, goals, dist=None, path_cap: int | None = None, algo: str = "astar", **kw):
    """astar2d_sharded for AStar3D (C5: 8192 queries over the node's GPUs).  occ: shared [X,Y,Z] or
    per-query [nq,X,Y,Z] grids (per-query grids are sliced with the rank's queries)."""
    from . import shard

    _lib.device_check()
    occ_np = np.asarray(occ)
    s_all, g_all = np.asarray(starts), np.asarray(goals)
    per_query = occ_np.ndim == 4
    world = dist.get_world_size() if dist is not None else 1
    rank = dist.get_rank() if dist is not None else 0
    idx = shard.lpt_deal(shard.octile(s_all, g_all), world, rank)
    r = astar3d_batch(occ_np[idx] if per_query else occ_np, s_all[idx], g_all[idx], path_cap=path_cap, algo=algo, **kw)
    return shard.all_gather_rows(dist, idx, {k: r[k] for k in _RECORDS}, len(s_all), device="cuda")


def obstacle_grid(obstacles):
    """Obstacle set of (x, y) integer tuples -> (ox, oy, occ[W, H]) covering its bounding box."""
    if not obstacles:
        return 0, 0, np.zeros((1, 1), np.uint8)
    a = np.fromiter((c for t in obstacles for c in t), np.int64, count=2 * len(obstacles)).reshape(-1, 2)
    ox, oy = int(a[:, 0].min()), int(a[:, 1].min())
    W, H = int(a[:, 0].max()) - ox + 1, int(a[:, 1].max()) - oy + 1
    occ = np.zeros((W, H), np.uint8)
    occ[a[:, 0] - ox, a[:, 1] - oy] = 1
    return ox, oy, occ


def pack_paths(paths):
    """list of [P_i, 2] paths -> (path_xy [sum P, 2] f64, path_off [n+1] i32) numpy arrays."""
    off = np.zeros(len(paths) + 1, np.int32)
    for i, p in enumerate(paths):
        off[i + 1] = off[i] + len(p)
    xy = np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in paths]) if off[-1] else np.zeros((0, 2))
    return xy, off


def dwa_step_batch(grid, lp_params, dwa_params, state, goal, path_xy, path_off, iters: int = 1,
                   want_eval: bool = False, want_traj: bool = False, want_hist: bool = False, parts: int = 0):
    """Batched DWA.plan iterations (dwa.py:72-93) on the gfx950 kernel dwa.hip.

    grid: (ox, oy, occ[W, H]) from obstacle_grid() (or with occ already a device bit tensor plus W, H).
    lp_params: _lib.LPParams; dwa_params: _lib.DWAParams.
    state [na, 5] f64 device tensor, updated in place; goal [na, 3]; path_xy / path_off from pack_paths().
    parts: workgroups per agent (pmp_dwa_set_split: 0 auto, 1 one per agent, k); results are identical.
    Returns dict of device tensors (u, best, status, n_steps, optional hist_pose, eval, best_traj).
    """
    torch = _lib.device_check()
    L = _lib.load_library()
    ctx = _lib.context()
    ox, oy, occ = grid[:3]
    if isinstance(occ, np.ndarray):
        W, H = occ.shape
        occ_bits = occ_bits_device(occ, torch)
    else:
        occ_bits, (W, H) = occ, grid[3]
    na = int(state.shape[0])
    goal = _dev(torch, goal, torch.float64).reshape(-1, 3)
    path_xy = _dev(torch, path_xy, torch.float64).reshape(-1, 2)
    path_off = _dev(torch, path_off, torch.int32)
    H_steps = int(dwa_params.predict_time / lp_params.dt)
    out = dict(u=torch.empty((na, 2), dtype=torch.float64, device="cuda"),
               best=torch.empty(na, dtype=torch.int32, device="cuda"),
               status=torch.empty(na, dtype=torch.int32, device="cuda"),
               n_steps=torch.empty(na, dtype=torch.int32, device="cuda"))
    out["hist_pose"] = torch.zeros((na, iters, 3), dtype=torch.float64, device="cuda") if want_hist else None
    out["eval"] = torch.zeros((na, 4096, 3), dtype=torch.float64, device="cuda") if want_eval else None
    out["best_traj"] = (torch.zeros((na, iters, max(H_steps, 1), 5), dtype=torch.float64, device="cuda")
                        if want_traj else None)
    _lib.check(ctx, L.pmp_dwa_set_split(ctx, int(parts)), "pmp_dwa_set_split")
    rc = L.pmp_dwa_step_batch(ctx, _lib.stream_ptr(), occ_bits.data_ptr(),
                              ox, oy, W, H, ctypes.byref(lp_params), ctypes.byref(dwa_params), na, state.data_ptr(),
                              goal.data_ptr(), path_xy.data_ptr(), path_off.data_ptr(), int(iters),
                              out["u"].data_ptr(), out["best"].data_ptr(), out["status"].data_ptr(),
                              out["n_steps"].data_ptr(), _lib.ptr(out["hist_pose"]), _lib.ptr(out["eval"]),
                              _lib.ptr(out["best_traj"]))
    _lib.check(ctx, rc, "pmp_dwa_step_batch")
    return out


def lqr_control_batch(lp_params, lqr_params, s, s_d, u_r, robot_vw):
    """Batched LQR.lqrControl (lqr.py:103-145).  s, s_d [n,3], u_r [n,2], robot_vw [n,2] (the
    robot's current v, w).  Returns u [n,2] (device tensor)."""
    torch = _lib.device_check()
    L = _lib.load_library()
    ctx = _lib.context()
    s = _dev(torch, s, torch.float64).reshape(-1, 3)
    n = int(s.shape[0])
    s_d = _dev(torch, s_d, torch.float64).reshape(-1, 3)
    u_r = _dev(torch, u_r, torch.float64).reshape(-1, 2)
    vw = _dev(torch, robot_vw, torch.float64).reshape(-1, 2)
    u = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    rc = L.pmp_lqr_control_batch(ctx, _lib.stream_ptr(), ctypes.byref(lp_params),
                                 ctypes.byref(lqr_params), n, s.data_ptr(), s_d.data_ptr(), u_r.data_ptr(),
                                 vw.data_ptr(), u.data_ptr())
    _lib.check(ctx, rc, "pmp_lqr_control_batch")
    return u


def mpc_control_batch(lp_params, mpc_params, s, s_d, u_r, u_p, robot_vw, want_qp: bool = False):
    """Batched MPC.mpcControl (mpc.py:111-214).  u_p [n,2] device tensor updated in place (the new
    u_p the reference returns).  Returns dict: u [n,2], iters, status, and with want_qp the assembled
    QP (H [n,2m,2m], g [n,2m], lu [n,2,4m]) and its solution du [n,2m]."""
    torch = _lib.device_check()
    L = _lib.load_library()
    ctx = _lib.context()
    s = _dev(torch, s, torch.float64).reshape(-1, 3)
    n = int(s.shape[0])
    nv = 2 * int(mpc_params.m)
    s_d = _dev(torch, s_d, torch.float64).reshape(-1, 3)
    u_r = _dev(torch, u_r, torch.float64).reshape(-1, 2)
    vw = _dev(torch, robot_vw, torch.float64).reshape(-1, 2)
    f64 = dict(dtype=torch.float64, device="cuda")
    out = dict(u=torch.empty((n, 2), **f64), iters=torch.empty(n, dtype=torch.int32, device="cuda"),
               status=torch.empty(n, dtype=torch.int32, device="cuda"))
    out.update(H=torch.zeros((n, nv, nv), **f64), g=torch.zeros((n, nv), **f64), lu=torch.zeros((n, 2, 2 * nv), **f64),
               du=torch.zeros((n, nv), **f64)) if want_qp else out.update(H=None, g=None, lu=None, du=None)
    rc = L.pmp_mpc_control_batch(ctx, _lib.stream_ptr(), ctypes.byref(lp_params),
                                 ctypes.byref(mpc_params), n, s.data_ptr(), s_d.data_ptr(), u_r.data_ptr(),
                                 u_p.data_ptr(), vw.data_ptr(), out["u"].data_ptr(), _lib.ptr(out["H"]),
                                 _lib.ptr(out["g"]), _lib.ptr(out["lu"]), _lib.ptr(out["du"]), out["iters"].data_ptr(),
                                 out["status"].data_ptr())
    _lib.check(ctx, rc, "pmp_mpc_control_batch")
    return out


def track_step_batch(kind: str, lp_params, state, goal, path_xy, path_off, iters: int = 1, lqr_params=None,
                     mpc_params=None, u_p=None, want_hist: bool = False):
    """Batched LQR.plan / MPC.plan iterations (lqr.py:58-86, mpc.py:66-94), kind "lqr" or "mpc".
    state [na,5] f64 device tensor (updated in place); u_p [na,2] device tensor (MPC, in place).
    Returns dict of device tensors (u, status, n_steps, admm_iters, optional hist_pose)."""
    torch = _lib.device_check()
    L = _lib.load_library()
    ctx = _lib.context()
    k = {"lqr": _lib.TRACK_LQR, "mpc": _lib.TRACK_MPC}[kind]
    na = int(state.shape[0])
    goal = _dev(torch, goal, torch.float64).reshape(-1, 3)
    path_xy = _dev(torch, path_xy, torch.float64).reshape(-1, 2)
    path_off = _dev(torch, path_off, torch.int32)
    if k == _lib.TRACK_MPC and u_p is None:
        raise ValueError("MPC needs the carried u_p tensor [na, 2]")
    out = dict(u=torch.empty((na, 2), dtype=torch.float64, device="cuda"),
               status=torch.empty(na, dtype=torch.int32, device="cuda"),
               n_steps=torch.empty(na, dtype=torch.int32, device="cuda"),
               admm_iters=torch.empty(na, dtype=torch.int32, device="cuda"))
    out["hist_pose"] = torch.zeros((na, iters, 3), dtype=torch.float64, device="cuda") if want_hist else None
    rc = L.pmp_track_step_batch(ctx, _lib.stream_ptr(), k, ctypes.byref(lp_params),
                                ctypes.byref(lqr_params) if lqr_params is not None else None,
                                ctypes.byref(mpc_params) if mpc_params is not None else None, na, state.data_ptr(),
                                _lib.ptr(u_p), goal.data_ptr(), path_xy.data_ptr(), path_off.data_ptr(), int(iters),
                                out["u"].data_ptr(), out["status"].data_ptr(), out["n_steps"].data_ptr(),
                                _lib.ptr(out["hist_pose"]), out["admm_iters"].data_ptr())
    _lib.check(ctx, rc, "pmp_track_step_batch")
    return out


def follow_step_batch(kind: str, grid, lp_params, follow_params, state, goal, path_xy, path_off, iters: int = 1,
                      pid_state=None, want_hist: bool = False, want_lookahead: bool = False):
    """Batched PID.plan / APF.plan / RPP.plan iterations (pid.py:55-99, apf.py:50-95, rpp.py:51-99) on
    the gfx950 kernel follow.hip, kind "pid", "apf" or "rpp".

    grid: (ox, oy, occ[W, H]) from obstacle_grid() (or with occ already a device bit tensor plus (W, H));
    may be None for PID, which reads no obstacles.  lp_params: _lib.LPParams; follow_params: _lib.FollowParams.
    state [na,5] f64 device tensor (updated in place); pid_state [na,4] f64 device tensor (PID: e_v, i_v,
    e_w, i_w, in place).  Returns dict of device tensors (u, status, n_steps, optional hist_pose
    [na,iters,3] and lookahead [na,iters,2])."""
    torch = _lib.device_check()
    L = _lib.load_library()
    ctx = _lib.context()
    k = _lib.FOLLOW_KINDS[kind]
    occ_bits, ox, oy, W, H = None, 0, 0, 0, 0
    if grid is not None:
        ox, oy, occ = grid[:3]
        if isinstance(occ, np.ndarray):
            W, H = occ.shape
            occ_bits = occ_bits_device(occ, torch)
        else:
            occ_bits, (W, H) = occ, grid[3]
    elif k != _lib.FOLLOW_PID:
        raise ValueError(f"{kind} needs the obstacle grid")
    if k == _lib.FOLLOW_PID and pid_state is None:
        raise ValueError("PID needs the carried pid_state tensor [na, 4]")
    na = int(state.shape[0])
    goal = _dev(torch, goal, torch.float64).reshape(-1, 3)
    path_xy = _dev(torch, path_xy, torch.float64).reshape(-1, 2)
    path_off = _dev(torch, path_off, torch.int32)
    out = dict(u=torch.empty((na, 2), dtype=torch.float64, device="cuda"),
               status=torch.empty(na, dtype=torch.int32, device="cuda"),
               n_steps=torch.empty(na, dtype=torch.int32, device="cuda"))
    out["hist_pose"] = torch.zeros((na, iters, 3), dtype=torch.float64, device="cuda") if want_hist else None
    out["lookahead"] = torch.zeros((na, iters, 2), dtype=torch.float64, device="cuda") if want_lookahead else None
    rc = L.pmp_follow_step_batch(ctx, _lib.stream_ptr(), k, _lib.ptr(occ_bits), int(ox), int(oy), int(W), int(H),
                                 ctypes.byref(lp_params), ctypes.byref(follow_params), na, state.data_ptr(),
                                 _lib.ptr(pid_state), goal.data_ptr(), path_xy.data_ptr(), path_off.data_ptr(),
                                 int(iters), out["u"].data_ptr(), out["status"].data_ptr(), out["n_steps"].data_ptr(),
                                 _lib.ptr(out["hist_pose"]), _lib.ptr(out["lookahead"]))
    _lib.check(ctx, rc, "pmp_follow_step_batch")
    return out


def dstar2d_batch(occ, starts, goals, path_cap: int | None = None, max_process: int = 0):
    """Batched DStar.plan (d_star.py:75-156) on one Grid.  occ uint8 [W, H] (x-major).
    Returns dict of device tensors: cost, path_len, path [nq, path_cap] (cells x*H+y, start -> goal),
    n_process (processState calls), status (4 = the reference raises: start unreachable)."""
    torch, L, ctx = _open()
    occ_bits, W, H = _occ2d(torch, occ)
    s, g, nq = _endpoints(torch, starts, goals, 2, torch.int32)
    path_cap = _path_cap(path_cap, W * H, None)
    out = _records(torch, (nq,), path_cap, "n_process", "int64")
    rc = L.pmp_dstar2d_batch(ctx, _lib.stream_ptr(), occ_bits.data_ptr(), W, H,
                             s.data_ptr(), g.data_ptr(), nq, out["cost"].data_ptr(), out["path_len"].data_ptr(),
                             out["path"].data_ptr(), path_cap, out["n_process"].data_ptr(), out["status"].data_ptr(),
                             int(max_process))
    _lib.check(ctx, rc, "pmp_dstar2d_batch")
    return out


def dstar2d_onpress_batch(occ, starts, goals, presses, path_cap: int | None = None, max_process: int = 0):
    """Batched DStar.plan followed by one DStar.OnPress per press (d_star.py:75-134) on one Grid,
    pmp_dstar2d_onpress_batch.  presses [nq, npress, 2] int cells (x, y).
    Returns dict of device tensors, per call r (0 = plan): cost [nq, R], path_len [nq, R],
    path [nq, R, path_cap] (cells x*H+y; plan start -> goal, presses the walk without the goal),
    n_process [nq, R] (len(EXPAND)), status [nq, R] (include/pmp.h)."""
    torch, L, ctx = _open()
    occ_bits, W, H = _occ2d(torch, occ)
    s, g, nq = _endpoints(torch, starts, goals, 2, torch.int32)
    pr = _dev(torch, presses, torch.int32)
    if pr.dim() != 3 or pr.shape[0] != nq or pr.shape[2] != 2:
        raise ValueError("presses must be [nq, npress, 2]")
    R = int(pr.shape[1]) + 1
    path_cap = 4 * W * H + 8 if path_cap is None else int(path_cap)  # a walk can visit a cell more than once
    out = _records(torch, (nq, R), path_cap, "n_process", "int64")
    rc = L.pmp_dstar2d_onpress_batch(ctx, _lib.stream_ptr(), occ_bits.data_ptr(), W, H, s.data_ptr(), g.data_ptr(), nq,
                                     pr.data_ptr(), R - 1, out["cost"].data_ptr(), out["path_len"].data_ptr(),
                                     out["path"].data_ptr(), path_cap, out["n_process"].data_ptr(),
                                     out["status"].data_ptr(), int(max_process))
    _lib.check(ctx, rc, "pmp_dstar2d_onpress_batch")
    return out


def lpastar2d_batch(occ, starts, goals, heuristic: str = "euclidean", path_cap: int = 1001, counters: bool = False,
                    lite: bool = False):
    """Batched LPAStar.plan (lpa_star.py:78-87: computeShortestPath + extractPath) on one Grid;
    lite=True runs DStarLite.plan (d_star_lite.py:14-187, pmp_dstarlite2d_batch).
    occ uint8 [W, H] (x-major).  Returns dict of device tensors: cost, path_len, path [nq, path_cap]
    (cells x*H+y, start -> goal), n_expanded (len(EXPAND)), status (1 = extractPath gave up after
    1000 steps, 4 = the reference raises), optional counters [nq, 4]."""
    torch, L, ctx = _open()
    occ_bits, W, H = _occ2d(torch, occ)
    s, g, nq = _endpoints(torch, starts, goals, 2, torch.int32)
    path_cap = int(path_cap)
    out = _records(torch, (nq,), path_cap, counters=counters)
    fn = L.pmp_dstarlite2d_batch if lite else L.pmp_lpastar2d_batch
    rc = fn(ctx, _lib.stream_ptr(), occ_bits.data_ptr(), W, H, _manhattan(heuristic), s.data_ptr(), g.data_ptr(), nq,
            out["cost"].data_ptr(), out["path_len"].data_ptr(), out["path"].data_ptr(), path_cap,
            out["n_expanded"].data_ptr(), _lib.ptr(out["counters"]), out["status"].data_ptr())
    _lib.check(ctx, rc, "pmp_dstarlite2d_batch" if lite else "pmp_lpastar2d_batch")
    return out


def lpastar2d_replan_batch(occ, starts, goals, toggles, heuristic: str = "euclidean", path_cap: int = 1001,
                           counters: bool = False, lite: bool = False):
    """LPAStar.plan() then one LPAStar.OnPress edit (lpa_star.py:101-137) per toggle, each followed by
    plan() on the kept state, for every query (pmp_lpastar2d_replan_batch); lite=True: DStarLite.plan()
    then DStarLite.OnPress per toggle (d_star_lite.py:61-97, pmp_dstarlite2d_replan_batch).  toggles [nq, nt, 2].
    Returns cost / n_expanded / status [nq, nt + 1] (status -1 = not run) and the last plan's path."""
    torch, L, ctx = _open()
    occ_bits, W, H = _occ2d(torch, occ)
    s, g, nq = _endpoints(torch, starts, goals, 2, torch.int32)
    t = _dev(torch, toggles, torch.int32).reshape(nq, -1, 2)
    nt = int(t.shape[1])
    if nt < 1:
        raise ValueError("lpastar2d_replan_batch needs at least one toggle per query")
    if bool(((t[..., 0] < 0) | (t[..., 0] >= W) | (t[..., 1] < 0) | (t[..., 1] >= H)).any()):
        raise ValueError("toggle cells must lie in the grid (OnPress rejects others, lpa_star.py:108-109)")
    path_cap = int(path_cap)
    # a record per plan, but only the last plan's path
    out = _records(torch, (nq, nt + 1), path_cap, path_lead=(nq,), counters=counters)
    fn = L.pmp_dstarlite2d_replan_batch if lite else L.pmp_lpastar2d_replan_batch
    rc = fn(ctx, _lib.stream_ptr(), occ_bits.data_ptr(), W, H, _manhattan(heuristic), s.data_ptr(), g.data_ptr(), nq,
            t.data_ptr(), nt, out["cost"].data_ptr(), out["n_expanded"].data_ptr(), out["status"].data_ptr(),
            out["path_len"].data_ptr(), out["path"].data_ptr(), path_cap, _lib.ptr(out["counters"]))
    _lib.check(ctx, rc, "pmp_dstarlite2d_replan_batch" if lite else "pmp_lpastar2d_replan_batch")
    return out


def map_arrays(env, torch=None):
    """Map obstacle lists (env.py:83-117) -> device f64 tensors rect [nr,4], circ [nc,3], bnd [nb,4]."""
    torch = torch or _lib.device_check()

    def t(lst, k):
        a = np.asarray(lst if lst else np.zeros((0, k)), np.float64).reshape(-1, k)
        return torch.as_tensor(np.ascontiguousarray(a), device="cuda")

    return t(env.obs_rect, 4), t(env.obs_circ, 3), t(env.boundary, 4)


def _sample_inputs(torch, env, starts, goals, rnd, sample_num, delta, max_dist, radius, goal_sample_rate, star):
    """What the three sampling wrappers take in: the Map's obstacle arrays, the endpoints and the random
    streams on the device, and the RRTParams.  Returns (head, keep, nq, rnd): head is what their C entries
    take after the context and the stream, from the parameters to the goals; keep = (rect, circ, bnd, s, g)
    are the tensors head points into, to be held until the launch; rnd is [nq, stride]."""
    rect, circ, bnd = map_arrays(env, torch)
    s, g, nq = _endpoints(torch, starts, goals, 2, torch.float64)
    rnd = _dev(torch, rnd, torch.float64).reshape(nq, -1)
    P = _lib.RRTParams(float(env.x_range), float(env.y_range), float(delta), float(max_dist), float(radius),
                       float(goal_sample_rate), int(sample_num), int(star))
    head = (ctypes.byref(P), rect.data_ptr(), int(rect.shape[0]), circ.data_ptr(), int(circ.shape[0]), bnd.data_ptr(),
            int(bnd.shape[0]), s.data_ptr(), g.data_ptr())
    return head, (rect, circ, bnd, s, g), nq, rnd


def _tree_outputs(torch, nq, trees, cap, path_cap, counters):
    """What the three sampling wrappers give back: the tree block with the per-tree leading shape `trees`
    (() for one tree per query, (2,) for RRT-Connect's pair), the path and the per-query scalars."""
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    return dict(tree_xy=torch.empty(nq, *trees, cap, 2, **f64), tree_g=torch.empty(nq, *trees, cap, **f64),
                tree_parent=torch.empty(nq, *trees, cap, **i32), n_nodes=torch.empty(nq, *trees, **i32),
                path_len=torch.empty(nq, **i32), path=torch.empty(nq, max(path_cap, 1), 2, **f64),
                draws=torch.empty(nq, dtype=torch.int64, device="cuda"), status=torch.empty(nq, **i32),
                counters=torch.zeros(nq, 4, dtype=torch.int64, device="cuda") if counters else None)


def rrt_batch(env, starts, goals, rnd, sample_num: int, star: bool = True, max_dist: float = 0.5,
              radius: float = 10.0, goal_sample_rate: float = 0.05, delta: float = 0.5, path_cap: int | None = None,
              counters: bool = False):
    """Batched RRT / RRT* plans (rrt.py:49-151, rrt_star.py:43-76) on one Map.
    rnd: [nq, stride] f64 random streams (RandomState.random_sample order; 3*sample_num+1 per query).
    Returns dict of device tensors: tree_xy [nq,cap,2], tree_g, tree_parent, n_nodes, cost, path_len,
    path [nq,path_cap,2] (goal -> start), draws, status."""
    torch, L, ctx = _open()
    head, keep, nq, rnd = _sample_inputs(torch, env, starts, goals, rnd, sample_num, delta, max_dist, radius,
                                         goal_sample_rate, bool(star))
    cap = int(sample_num) + 2
    path_cap = cap if path_cap is None else int(path_cap)
    out = _tree_outputs(torch, nq, (), cap, path_cap, counters)
    out["cost"] = torch.empty(nq, dtype=torch.float64, device="cuda")
    rc = L.pmp_rrt_batch(ctx, _lib.stream_ptr(), *head, nq, rnd.data_ptr(), int(rnd.shape[1]), cap,
                         out["tree_xy"].data_ptr(), out["tree_g"].data_ptr(), out["tree_parent"].data_ptr(),
                         out["n_nodes"].data_ptr(), out["cost"].data_ptr(), out["path_len"].data_ptr(),
                         out["path"].data_ptr(), path_cap, out["draws"].data_ptr(), out["status"].data_ptr(),
                         _lib.ptr(out["counters"]))
    _lib.check(ctx, rc, "pmp_rrt_batch")
    return out


def ellipse_constants(starts, goals) -> np.ndarray:
    """[nq, 5] per query: the centre, cos / sin of theta and c of Ellipse.transform
    (informed_rrt.py:20-33, 67-69), each with the reference's own scalar numpy expression (np.arctan2
    differs from libm's atan2 in the last bit of some inputs, so theta is not recomputed on the device)."""
    s = np.asarray(starts, np.float64).reshape(-1, 2)
    g = np.asarray(goals, np.float64).reshape(-1, 2)
    out = np.empty((len(s), 5), np.float64)
    for q, (p1, p2) in enumerate(zip(s.tolist(), g.tolist())):
        theta = -np.arctan2(p2[1] - p1[1], p2[0] - p1[0])
        out[q] = ((p1[0] + p2[0]) / 2, (p1[1] + p2[1]) / 2, np.cos(theta), np.sin(theta),
                  math.hypot(p2[0] - p1[0], p2[1] - p1[1]) / 2)
    return out


def informed_rrt_batch(env, starts, goals, rnd, sample_num: int, max_dist: float = 0.5, radius: float = 12.0,
                       delta: float = 0.5, goal_sample_rate: float = 0.05, path_cap: int | None = None,
                       counters: bool = False):
    """Batched Informed RRT* plans (informed_rrt.py:74-152) on one Map.
    rnd: [nq, stride] f64 random streams (RandomState.random_sample order).  The ellipse sampler's draw
    count is unbounded: a query that reaches the end of its stream reports status 3 (re-run it with a
    longer stream; 4*sample_num+64 is enough for most).
    Returns dict of device tensors: tree_xy [nq,cap,2], tree_g, tree_parent, n_nodes, best_cost (inf:
    never connected), n_finds, goal_slot (-1: never connected), path_len, path [nq,path_cap,2] (the best
    connection's, goal -> start), draws, status."""
    torch, L, ctx = _open()
    head, keep, nq, rnd = _sample_inputs(torch, env, starts, goals, rnd, sample_num, delta, max_dist, radius,
                                         goal_sample_rate, 1)
    s, g = keep[3:]
    ell = torch.as_tensor(ellipse_constants(s.cpu().numpy(), g.cpu().numpy()), device="cuda")
    cap = int(sample_num) + 2
    path_cap = cap if path_cap is None else int(path_cap)
    out = _tree_outputs(torch, nq, (), cap, path_cap, counters)
    out.update(best_cost=torch.empty(nq, dtype=torch.float64, device="cuda"),
               n_finds=torch.empty(nq, dtype=torch.int32, device="cuda"),
               goal_slot=torch.empty(nq, dtype=torch.int32, device="cuda"))
    rc = L.pmp_informed_rrt_batch(ctx, _lib.stream_ptr(), *head, ell.data_ptr(), nq, rnd.data_ptr(), int(rnd.shape[1]),
                                  cap, out["tree_xy"].data_ptr(), out["tree_g"].data_ptr(),
                                  out["tree_parent"].data_ptr(), out["n_nodes"].data_ptr(),
                                  out["best_cost"].data_ptr(), out["n_finds"].data_ptr(), out["goal_slot"].data_ptr(),
                                  out["path_len"].data_ptr(), out["path"].data_ptr(), path_cap,
                                  out["draws"].data_ptr(), out["status"].data_ptr(), _lib.ptr(out["counters"]))
    _lib.check(ctx, rc, "pmp_informed_rrt_batch")
    return out


RRT_CONNECT_DEFAULT_CAP = 2048


def rrt_connect_lds_nodes() -> int:
    """Nodes of each tree rrt_connect.hip keeps in LDS (larger trees continue in HBM)."""
    return int(_lib.load_library().pmp_rrt_connect_lds_nodes())


def rrt_connect_batch(env, starts, goals, rnd, sample_num: int, max_dist: float = 0.5, goal_sample_rate: float = 0.05,
                      delta: float = 0.5, cap: int | None = None, path_cap: int | None = None, counters: bool = False):
    """Batched RRT-Connect plans (rrt_connect.py:42-147) on one Map.
    rnd: [nq, stride] f64 random streams (RandomState.random_sample order; 3*sample_num per query suffice).
    cap: nodes per tree, default 2048 -- the reference's runs on the README map need up to 150 and C3 with
    max_dist 0.5 about 1,100.  An iteration adds one node plus its greedy steps, so sample_num does not
    bound a tree: a query that outgrows cap reports status 3 (re-run it with a larger one; RRTConnect.plan
    doubles it).  Memory is nq x 2 x cap x 28 B.  path_cap defaults to 2 * cap, which holds any path.
    Returns dict of device tensors: tree_xy [nq,2,cap,2], tree_g, tree_parent [nq,2,cap] (tree 0 rooted at
    the start, tree 1 at the goal), n_nodes [nq,2], forward, boundary [nq,2], cost, path_len, path
    [nq,path_cap,2] (start -> goal), iters, draws, status."""
    torch, L, ctx = _open()
    head, keep, nq, rnd = _sample_inputs(torch, env, starts, goals, rnd, sample_num, delta, max_dist, 0.0,
                                         goal_sample_rate, 0)
    cap = RRT_CONNECT_DEFAULT_CAP if cap is None else int(cap)
    path_cap = 2 * cap if path_cap is None else int(path_cap)
    out = _tree_outputs(torch, nq, (2,), cap, path_cap, counters)
    i32 = dict(dtype=torch.int32, device="cuda")
    out.update(cost=torch.empty(nq, dtype=torch.float64, device="cuda"), forward=torch.empty(nq, **i32),
               boundary=torch.empty(nq, 2, **i32), iters=torch.empty(nq, **i32))
    rc = L.pmp_rrt_connect_batch(ctx, _lib.stream_ptr(), *head, nq, rnd.data_ptr(), int(rnd.shape[1]), cap,
                                 out["tree_xy"].data_ptr(), out["tree_g"].data_ptr(), out["tree_parent"].data_ptr(),
                                 out["n_nodes"].data_ptr(), out["forward"].data_ptr(), out["boundary"].data_ptr(),
                                 out["cost"].data_ptr(), out["path_len"].data_ptr(), out["path"].data_ptr(), path_cap,
                                 out["iters"].data_ptr(), out["draws"].data_ptr(), out["status"].data_ptr(),
                                 _lib.ptr(out["counters"]))
    _lib.check(ctx, rc, "pmp_rrt_connect_batch")
    return out


def astar3d_batch(occ, starts, goals, heuristic: str = "euclidean", path_cap: int | None = None,
                  expand_cap: int = 0, counters: bool = False, algo: str = "astar"):
    """Batched AStar3D.plan (a_star3d.py:33-106); algo "dijkstra" / "gbfs" run Dijkstra3D.plan
    (dijkstra3d.py:39-87) / GBFS3D.plan (gbfs3d.py:34-82) on the same kernel (pmp_graph3d_batch).

    occ: uint8 [X, Y, Z] shared grid or [nq, X, Y, Z] per-query grids (numpy).
    Returns dict of device tensors: cost (inf if unreachable), path_len, path [nq, path_cap]
    (cells (x*Y+y)*Z+z, start -> goal), n_expanded (len(CLOSED)), status, optional expand / counters.
    """
    torch, L, ctx = _open()
    occ_bits, per_query, (X, Y, Z) = _occ3d_bits(torch, occ)
    s, g, nq = _endpoints(torch, starts, goals, 3, torch.int32)
    path_cap = _path_cap(path_cap, X * Y * Z)
    out = _records(torch, (nq,), path_cap, expand=expand_cap, counters=counters)
    rc = L.pmp_graph3d_batch(ctx, _lib.stream_ptr(), _lib.ALGOS[algo], occ_bits.data_ptr(), int(per_query),
                             X, Y, Z, _manhattan(heuristic), s.data_ptr(), g.data_ptr(), nq,
                             out["cost"].data_ptr(), out["path_len"].data_ptr(), out["path"].data_ptr(), path_cap,
                             out["n_expanded"].data_ptr(), _lib.ptr(out["expand"]), int(expand_cap),
                             _lib.ptr(out["counters"]), out["status"].data_ptr())
    _lib.check(ctx, rc, "pmp_graph3d_batch")
    out["dims"] = (X, Y, Z)
    return out


def jps3d_batch(occ, starts, goals, heuristic: str = "euclidean", path_cap: int | None = None,
                expand_cap: int = 0, counters: bool = False):
    """Batched JPS3D.plan (jps3d.py:42-88) on pmp_jps3d_batch (csrc/jps3d.hip).

    occ: uint8 [X, Y, Z] shared grid or [nq, X, Y, Z] per-query grids (numpy).
    Returns astar3d_batch's dict (the path lists jump points only; n_expanded = len(CLOSED)) and, with
    expand_cap != 0, expand_parent / expand_g [nq, expand_cap]: the final CLOSED parent cell and g of
    the cells in `expand`.
    """
    torch, L, ctx = _open()
    occ_bits, per_query, (X, Y, Z) = _occ3d_bits(torch, occ)
    s, g, nq = _endpoints(torch, starts, goals, 3, torch.int32)
    path_cap = _path_cap(path_cap, X * Y * Z)
    out = _records(torch, (nq,), path_cap, expand=expand_cap, expand_parent=expand_cap, expand_g=expand_cap,
                   counters=counters)
    rc = L.pmp_jps3d_batch(ctx, _lib.stream_ptr(), occ_bits.data_ptr(), int(per_query), X, Y, Z,
                           _manhattan(heuristic), s.data_ptr(), g.data_ptr(), nq,
                           out["cost"].data_ptr(), out["path_len"].data_ptr(), out["path"].data_ptr(), path_cap,
                           out["n_expanded"].data_ptr(), _lib.ptr(out["expand"]), _lib.ptr(out["expand_parent"]),
                           _lib.ptr(out["expand_g"]), int(expand_cap), _lib.ptr(out["counters"]),
                           out["status"].data_ptr())
    _lib.check(ctx, rc, "pmp_jps3d_batch")
    out["dims"] = (X, Y, Z)
    return out


def jps2d_batch(occ, starts, goals, heuristic: str = "euclidean", path_cap: int | None = None,
                expand_cap: int = 0, push_cap: int = 0, counters: bool = False, occ_bits=None):
    """Batched JPS.plan (jps.py:38-83) on pmp_jps2d_batch (csrc/jps2d.hip).

    occ: a Grid or a numpy uint8 [W, H] occupancy shared by the queries (or occ=(W, H) with a prebuilt
    `occ_bits` device tensor).  starts, goals: [nq, 2] int.
    Returns dict of device tensors: cost f64 [nq] (0 without a path), path_len i32 [nq], path i32
    [nq, path_cap] (cell ids x*H + y of the jump points, goal first), n_expanded i32 (len(CLOSED)),
    status i32 (0 found, 1 no path, 2 path_cap overflow, 3 push_cap overflow), and with expand_cap != 0
    expand / expand_parent / expand_g [nq, expand_cap]: the CLOSED cells in insertion order, each
    node's parent cell and g; optional counters i64 [nq, 4] (pushes, pops, expansions, max heap size).
    push_cap: pushes (and heap entries) kept per query, 0 = the kernel's default.
    """
    torch, L, ctx = _open()
    occ_bits, W, H = _occ2d(torch, occ, occ_bits)
    s, g, nq = _endpoints(torch, starts, goals, 2, torch.int32)
    path_cap = _path_cap(path_cap, W * H, 1 << 12)
    out = _records(torch, (nq,), path_cap, expand=expand_cap, expand_parent=expand_cap, expand_g=expand_cap,
                   counters=counters)
    rc = L.pmp_jps2d_batch(ctx, _lib.stream_ptr(), occ_bits.data_ptr(), W, H, _manhattan(heuristic),
                           s.data_ptr(), g.data_ptr(), nq, out["cost"].data_ptr(), out["path_len"].data_ptr(),
                           out["path"].data_ptr(), path_cap, out["n_expanded"].data_ptr(), _lib.ptr(out["expand"]),
                           _lib.ptr(out["expand_parent"]), _lib.ptr(out["expand_g"]), int(expand_cap), int(push_cap),
                           _lib.ptr(out["counters"]), out["status"].data_ptr())
    _lib.check(ctx, rc, "pmp_jps2d_batch")
    out["W"], out["H"] = W, H
    return out


def dstar3d_batch(occ, starts, goals, blocks=None, path_cap: int | None = None, expand_cap: int = 0,
                  max_process: int = 0, occ_bits=None):
    """Batched DStar3D (d_star3d.py:60-281): plan() and then one apply_dynamic_obstacles() per round
    of `blocks` [nq, nrounds, nblk, 3] (int voxels; outside the grid = ignored), on pmp_dstar3d_batch.

    occ: uint8 [X, Y, Z] shared grid or [nq, X, Y, Z] per-query grids (numpy).
    Returns dict of device tensors, per round r (0 = plan): cost [nq, R], path_len [nq, R],
    path [nq, R, path_cap] (voxels (x*Y+y)*Z+z, start -> goal), n_process [nq, R] (len(EXPAND)),
    status [nq, R] (include/pmp.h), optional expand [nq, expand_cap] (plan()'s EXPAND voxels).
    occ_bits: optional device words of `occ` already packed (occ may then be just its shape)."""
    torch, L, ctx = _open()
    occ_bits, per_query, (X, Y, Z) = _occ3d_bits(torch, occ, occ_bits)
    s, g, nq = _endpoints(torch, starts, goals, 3, torch.int32)
    if blocks is None:
        nr, nb, b = 0, 0, None
    else:
        b = _dev(torch, blocks, torch.int32)
        if b.dim() != 4 or b.shape[0] != nq or b.shape[3] != 3:
            raise ValueError("blocks must be [nq, nrounds, nblk, 3]")
        nr, nb = int(b.shape[1]), int(b.shape[2])
    path_cap = _path_cap(path_cap, X * Y * Z)
    out = _records(torch, (nq, nr + 1), path_cap, "n_process", "int64", expand=expand_cap)
    rc = L.pmp_dstar3d_batch(ctx, _lib.stream_ptr(), occ_bits.data_ptr(), int(per_query), X, Y, Z, s.data_ptr(),
                             g.data_ptr(), nq, _lib.ptr(b), nr, nb, out["cost"].data_ptr(), out["path_len"].data_ptr(),
                             out["path"].data_ptr(), path_cap, out["n_process"].data_ptr(), out["status"].data_ptr(),
                             _lib.ptr(out["expand"]), int(expand_cap), int(max_process))
    _lib.check(ctx, rc, "pmp_dstar3d_batch")
    out["dims"] = (X, Y, Z)
    return out


def lpastar3d_batch(occ, starts, goals, changes=None, heuristic: str = "euclidean", path_cap: int | None = None,
                    counters: bool = False, max_expansions: int = 0, occ_bits=None):
    """Batched LPAStar3D (lpa_star3d.py:40-225): plan() and then one apply_change() per row of
    `changes` [nq, nr, 4] = (x, y, z, mode) with mode 0 = blocked None (toggle), 1 = True, 2 = False,
    on pmp_lpastar3d_batch.  occ: uint8 [X, Y, Z] shared or [nq, X, Y, Z] per-query grids.
    Returns dict of device tensors per call r (0 = plan): cost [nq, R], path_len [nq, R],
    path [nq, R, path_cap] (voxels (x*Y+y)*Z+z, start -> goal), n_expanded [nq, R] (len(EXPAND)),
    status [nq, R] (include/pmp.h), optional counters [nq, 4].
    occ_bits: optional device words of `occ` already packed (occ may then be just its shape)."""
    torch, L, ctx = _open()
    occ_bits, per_query, (X, Y, Z) = _occ3d_bits(torch, occ, occ_bits)
    s, g, nq = _endpoints(torch, starts, goals, 3, torch.int32)
    if changes is None:
        nr, ch = 0, None
    else:
        ch = _dev(torch, changes, torch.int32)
        if ch.dim() != 3 or ch.shape[0] != nq or ch.shape[2] != 4:
            raise ValueError("changes must be [nq, nr, 4]")
        nr = int(ch.shape[1])
    path_cap = _path_cap(path_cap, X * Y * Z)
    out = _records(torch, (nq, nr + 1), path_cap, "n_expanded", "int64", counters=counters)
    rc = L.pmp_lpastar3d_batch(ctx, _lib.stream_ptr(), occ_bits.data_ptr(), int(per_query), X, Y, Z,
                               _manhattan(heuristic), s.data_ptr(), g.data_ptr(), nq, _lib.ptr(ch), nr,
                               out["cost"].data_ptr(), out["path_len"].data_ptr(), out["path"].data_ptr(), path_cap,
                               out["n_expanded"].data_ptr(), out["status"].data_ptr(), _lib.ptr(out["counters"]),
                               int(max_expansions))
    _lib.check(ctx, rc, "pmp_lpastar3d_batch")
    out["dims"] = (X, Y, Z)
    return out


def _xyz_arrays(paths):
    return [np.asarray(p, np.float64).reshape(-1, 3) for p in paths]


def _traj3d_batch(torch, arrs, cells, row, min_wp, wp_limit, max_waypoints, eval_t, point_cap, estimate, call,
                  retry_overflow, merge=(), per_path=None):
    """What totp3d_batch, polytraj3d_batch and splinetraj3d_batch share: the two path sources, the eval_t
    upload, the common outputs and the overflow retry.
    arrs: list of [n, 3] f64 arrays (_xyz_arrays), packed to (flat [sum n, 3], off [nq + 1] i32); or None
    with cells=(path [nq, path_cap], path_len, (X, Y, Z)).  row: doubles per point.  The launch's max_waypoints is
    the one given, else the longest path's, at least min_wp and at most wp_limit (None: no limit).
    estimate(arrs, wp) -> the first point_cap when none is given and there is no eval_t (arrs: the waypoint
    arrays, or None in the cells form, where no path has more than wp waypoints).
    call(o, a, src, nmax, ev, pp) adds the kind's outputs to o (points [m, pc, row], n_points, total_time,
    status) and launches its C entry on m paths: a is the path tensor, src the entry's eight path-source
    arguments (path_xyz, path_off, cells, path_len, path_cap, X, Y, Z), nmax its max_waypoints, ev its
    (eval_t, n_eval), pp the per_path inputs {name: (array or None, shape of one path's)} as f64 device
    tensors of those m paths.
    Paths whose points overflow the first cap are run again with the largest count among them: their rows,
    n_points, total_time, status and the outputs named in merge replace the first run's; points grows to that
    count, NaN where the first run had no row.  Returns (out, off): off is the host offsets, None in the
    cells form."""
    et = None if eval_t is None else torch.as_tensor(np.asarray(eval_t, np.float64).ravel(), device="cuda")
    ev = (_lib.ptr(et), 0 if et is None else int(et.numel()))

    def pack(arrs):
        off = np.zeros(len(arrs) + 1, np.int32)
        off[1:] = np.cumsum([len(a) for a in arrs])
        flat = torch.as_tensor(np.concatenate(arrs) if arrs else np.zeros((0, 3)), device="cuda")
        return flat, torch.as_tensor(off, device="cuda"), off

    if cells is None:
        nq = len(arrs)
        a, b, off = pack(arrs)
        tail = (0, 0, 0, 0)
        wp = max((len(p) for p in arrs), default=min_wp)
    else:
        off = None
        a = _dev(torch, cells[0], torch.int32)
        b = _dev(torch, cells[1], torch.int32).reshape(-1)
        nq = int(a.shape[0])
        tail = (int(a.shape[1]),) + tuple(int(v) for v in cells[2])
        wp = int(b.max().item()) if max_waypoints is None and nq else min_wp
    if max_waypoints is not None:
        nmax = int(max_waypoints)
    else:
        nmax = max(min_wp, wp) if wp_limit is None else min(max(min_wp, wp), wp_limit)
    if point_cap is None:
        point_cap = ev[1] + 1 if et is not None else estimate(arrs, max(wp, int(max_waypoints or 0)))
    point_cap = int(point_cap)
    pp = {k: None if v is None else _dev(torch, v, torch.float64).reshape((nq,) + shape)
          for k, (v, shape) in (per_path or {}).items()}

    def launch(a, b, pp, pc):
        m = int(b.shape[0]) - 1 if cells is None else int(b.shape[0])
        f64 = dict(dtype=torch.float64, device="cuda")
        i32 = dict(dtype=torch.int32, device="cuda")
        o = dict(points=torch.empty((m, pc, row), **f64), n_points=torch.empty(m, **i32),
                 total_time=torch.empty(m, **f64), status=torch.empty(m, **i32))
        ptrs = (a.data_ptr(), b.data_ptr())
        src = (ptrs + (None, None) if cells is None else (None, None) + ptrs) + tail
        call(o, a, src, nmax, ev, pp)
        return o

    def rerun(redo, idx, pc):
        sa, sb = pack([arrs[i] for i in redo])[:2] if cells is None else (a[idx].contiguous(), b[idx].contiguous())
        return launch(sa, sb, {k: None if v is None else v[idx].contiguous() for k, v in pp.items()}, pc)

    out = launch(a, b, pp, point_cap)
    if retry_overflow and nq:
        _retry_overflowed(torch, out, nq, point_cap, row, rerun, ("total_time",) + tuple(merge))
    return out, off


def _retry_overflowed(torch, out, nq, point_cap, row, rerun, merge=()):
    """The single overflow retry of the wrappers that return point rows (the trajectory generators,
    dubins_batch).  out: the first launch's outputs with points [nq, point_cap, row], n_points and status.
    The items whose points overflowed point_cap are run again by rerun(redo, idx, pc) -> the same outputs
    for those items alone (redo: their indices on the host, idx: on the device, pc: the largest count among
    them); their rows, n_points, status and the outputs named in merge replace the first run's in out, and
    points grows to pc, NaN where the first run had no row."""
    st = out["status"].cpu().numpy()
    npt = out["n_points"].cpu().numpy()
    redo = np.nonzero((st == _lib.STATUS_PATH_OVERFLOW) & (npt > point_cap))[0]
    if len(redo):
        pc = int(npt[redo].max())
        idx = torch.as_tensor(redo, device="cuda", dtype=torch.long)
        r = rerun(redo, idx, pc)
        big = torch.full((nq, pc, row), float("nan"), dtype=torch.float64, device="cuda")
        big[:, :point_cap] = out["points"]
        big[idx] = r["points"]
        out["points"] = big
        for k in ("n_points", "status") + tuple(merge):
            out[k][idx] = r[k]


def totp3d_batch(paths, params, point_cap: int | None = None, eval_t=None, retry_overflow: bool = True):
    """Batched TimeOptimalTrajectory3D(path, constraints, path_resolution).generate()
    (trajectory/time_optimal_trajectory.py:260-302) on pmp_totp3d_batch.  paths: list of [n, 3]
    waypoint arrays (reference order); params: _lib.TotpParams.  With eval_t (1-D times), evaluate(t)
    (:304-335) at those times instead of generate()'s sampling.
    Returns dict of device tensors: s_values / s_dot / s_ddot / time [nq, sample_cap], n_samples,
    points [nq, point_cap, 12] (time, position, velocity, acceleration, yaw, yaw rate; NaN = None),
    n_points, total_time, status (include/pmp.h).  Queries whose points overflow the first cap are
    re-run with their exact count when retry_overflow."""
    torch = _lib.device_check()
    L = _lib.load_library()
    ctx = _lib.context()
    arrs = _xyz_arrays(paths)
    # n_samples = max(int(L / res), 100) with L summed in the kernel's (the reference's) order
    res = float(params.path_resolution)
    ns = [max(int(np.cumsum(np.sqrt(np.sum(np.diff(a, axis=0) ** 2, axis=1)))[-1] / res), 100) if len(a) > 1 else 1
          for a in arrs]
    sample_cap = max(ns, default=1) + 1
    profiles = ("s_values", "s_dot", "s_ddot", "time")

    def call(o, a, src, nmax, ev, pp):
        m, pc = o["points"].shape[:2]
        for k in profiles:
            o[k] = torch.empty((m, sample_cap), dtype=torch.float64, device="cuda")
        o["n_samples"] = torch.empty(m, dtype=torch.int32, device="cuda")
        if m:
            rc = L.pmp_totp3d_batch(ctx, _lib.stream_ptr(), ctypes.byref(params), m, *src[:2], nmax, sample_cap,
                                    o["s_values"].data_ptr(), o["s_dot"].data_ptr(), o["s_ddot"].data_ptr(),
                                    o["time"].data_ptr(), o["n_samples"].data_ptr(), pc, o["points"].data_ptr(),
                                    o["n_points"].data_ptr(), o["total_time"].data_ptr(), o["status"].data_ptr(), *ev)
            _lib.check(ctx, rc, "pmp_totp3d_batch")

    return _traj3d_batch(torch, arrs, None, 12, 2, None, None, eval_t, point_cap, lambda arrs, wp: 2048, call,
                         retry_overflow, merge=profiles + ("n_samples",))[0]


def polytraj_segment_times(path, params):
    """numpy restatement of _compute_segment_times (trajectory/polynomial_trajectory.py:89-111) for one
    [n, 3] path: sizes point_cap (the kernel computes its own)."""
    d = np.sqrt(np.sum(np.diff(np.asarray(path, np.float64).reshape(-1, 3), axis=0) ** 2, axis=1))
    vavg = min(params.max_velocity) * 0.7
    est = d / vavg if vavg > 0 else np.ones_like(d)
    return np.maximum(np.maximum(est, 2.0 * np.sqrt(d / min(params.max_acceleration))), 0.5)


def polytraj3d_batch(paths, params, bc=None, point_cap: int | None = None, eval_t=None, sample_dt: float | None = None,
                     retry_overflow: bool = True, cells=None, max_waypoints: int | None = None):
    """Batched PolynomialTrajectory3D(path, constraints, boundary_conditions).generate()
    (trajectory/polynomial_trajectory.py:189-251) on pmp_polytraj3d_batch.  paths: list of [n, 3]
    waypoint arrays (reference order), or None with cells=(path, path_len, (X, Y, Z)): the device
    tensors a 3D grid planner returned (batch.astar3d_batch's "path", "path_len" and grid size), decoded
    on the device.  params: _lib.PolyTrajParams.  bc [nq, 4, 3]: initial / final velocity, initial / final
    acceleration per path (None = zeros).  With eval_t (1-D times), evaluate(t) (:253-286) at those times
    instead of generate()'s sampling; with sample_dt, resample(sample_dt) (trajectory_base.py:193-216).
    Returns dict of device tensors: points [nq, point_cap, 15] (time, position, velocity, acceleration,
    jerk, yaw, yaw rate; NaN = None), n_points, total_time, status, segment_times (flat, path q's n - 1
    values from seg_off[q]; [nq, path_cap] in the cells form) (include/pmp.h).  Paths whose points
    overflow the first cap are re-run with their exact count when retry_overflow."""
    torch = _lib.device_check()
    L = _lib.load_library()
    ctx = _lib.context()
    wp_limit = int(L.pmp_polytraj3d_max_waypoints())
    dt = float(params.min_time_step) if sample_dt is None else float(sample_dt)
    if sample_dt is not None and not dt > 0:
        raise ValueError("sample_dt must be > 0")

    def estimate(arrs, wp):
        # an upper bound of the batch's total_time over the step
        if not (np.isfinite(dt) and dt > 0 and min(params.max_acceleration) > 0):
            return 2048
        if arrs is None:  # neighbouring cells are at most sqrt(3) apart (any-angle paths may overflow: retried)
            tmax = (wp - 1) * float(polytraj_segment_times([[0, 0, 0], [1, 1, 1]], params)[0])
        else:
            with np.errstate(all="ignore"):
                tmax = max((float(np.sum(polytraj_segment_times(a, params))) for a in arrs if len(a) > 1), default=0.0)
        return int(min(tmax / dt, float(1 << 24))) + 3 if np.isfinite(tmax) else 2048

    def call(o, a, src, nmax, ev, pp):
        m, pc = o["points"].shape[:2]
        # segment_times is not merged after a retry: it depends on the waypoints alone
        o["segment_times"] = torch.zeros(int(a.shape[0]) if cells is None else tuple(a.shape), dtype=torch.float64,
                                         device="cuda")
        rc = L.pmp_polytraj3d_batch(ctx, _lib.stream_ptr(), ctypes.byref(params), m, *src, _lib.ptr(pp["bc"]), nmax, pc,
                                    o["points"].data_ptr(), o["n_points"].data_ptr(), o["total_time"].data_ptr(),
                                    o["segment_times"].data_ptr(), o["status"].data_ptr(), *ev,
                                    0.0 if sample_dt is None else dt)
        _lib.check(ctx, rc, "pmp_polytraj3d_batch")

    out, off = _traj3d_batch(torch, _xyz_arrays(paths) if cells is None else None, cells, 15, 2, wp_limit,
                             max_waypoints, eval_t, point_cap, estimate, call, retry_overflow,
                             per_path=dict(bc=(bc, (4, 3))))
    if cells is None:
        out["seg_off"] = off
    return out


def splinetraj3d_batch(paths, params, point_cap: int | None = None, eval_t=None, sample_dt: float | None = None,
                       constant_speed: bool = False, retry_overflow: bool = True, cells=None,
                       max_waypoints: int | None = None):
    """Batched SplineTrajectory3D(path, constraints, spline_degree).generate()
    (trajectory/spline_trajectory.py:205-271, smoothing_factor = 0) on pmp_splinetraj3d_batch.  paths: list
    of [n, 3] waypoint arrays (reference order), or None with cells=(path, path_len, (X, Y, Z)): the device
    tensors a 3D grid planner returned (batch.astar3d_batch's "path", "path_len" and grid size), decoded
    on the device.  params: _lib.SplineTrajParams.  With eval_t (1-D times), evaluate(t) (:273-302) at
    those times instead of generate()'s rows; with sample_dt, resample(sample_dt)
    (trajectory_base.py:193-216); with constant_speed, the rows reparameterize_constant_speed() (:325-392)
    leaves.  The three exclude each other.
    Returns dict of device tensors: points [nq, point_cap, 12] (time, position, velocity, acceleration,
    yaw, yaw rate; NaN = None), n_points, total_time, status (include/pmp.h).  Paths whose points
    overflow the first cap are re-run with their exact count when retry_overflow."""
    torch = _lib.device_check()
    L = _lib.load_library()
    ctx = _lib.context()
    wp_limit = int(L.pmp_splinetraj3d_max_waypoints())
    dt = float(params.min_time_step) if sample_dt is None else float(sample_dt)
    if sample_dt is not None and not dt > 0:
        raise ValueError("sample_dt must be > 0")
    if (eval_t is not None) + (sample_dt is not None) + bool(constant_speed) > 1:
        raise ValueError("eval_t, sample_dt and constant_speed exclude each other")

    def estimate(arrs, wp):
        if arrs is None:  # neighbouring cells are at most sqrt(3) apart (any-angle paths may overflow: retried)
            lmax = (wp - 1) * 3.0 ** 0.5
        else:
            with np.errstate(all="ignore"):
                lmax = max((float(np.sum(np.sqrt(np.sum(np.diff(a, axis=0) ** 2, axis=1)))) for a in arrs if len(a) > 1),
                           default=0.0)
        # total_time is about the curve's length over min|max_velocity| (one unit of u for a short curve);
        # the scaling of _enforce_constraints can stretch it: such paths are retried
        vclip = min(abs(v) for v in params.max_velocity)
        est = max(1.5 * lmax / vclip, 2.0) / dt if vclip > 0 and dt > 0 and np.isfinite(lmax) else 2048.0
        return int(min(est, float(1 << 24))) + 3 if np.isfinite(est) else 2048

    def call(o, a, src, nmax, ev, pp):
        m, pc = o["points"].shape[:2]
        rc = L.pmp_splinetraj3d_batch(ctx, _lib.stream_ptr(), ctypes.byref(params), m, *src, nmax, pc,
                                      o["points"].data_ptr(), o["n_points"].data_ptr(), o["total_time"].data_ptr(),
                                      o["status"].data_ptr(), *ev, 0.0 if sample_dt is None else dt,
                                      1 if constant_speed else 0)
        _lib.check(ctx, rc, "pmp_splinetraj3d_batch")

    return _traj3d_batch(torch, _xyz_arrays(paths) if cells is None else None, cells, 12, 3, wp_limit,
                         max_waypoints, eval_t, point_cap, estimate, call, retry_overflow)[0]


def _dubins_point_cap(torch, s, g, step, max_curv):
    """An upper bound of a launch's point counts: (hypot max_curv + 4 pi) / step + 6 over its pairs (pairs
    beyond it are retried; pairs of non-finite poses or of more than 2^24 steps have no points); 2048 where
    the parameters give none."""
    if not int(s.shape[0]):
        return 1
    if not (step > 0 and max_curv > 0 and math.isfinite(step) and math.isfinite(max_curv)):
        return 2048  # the entry refuses these
    est = (torch.hypot(g[:, 0] - s[:, 0], g[:, 1] - s[:, 1]) * max_curv + 4.0 * math.pi) / step + 6.0
    return int(torch.where(est < float(1 << 24), est, torch.ones_like(est)).max().item())


def dubins_batch(starts, goals, step: float, max_curv: float, cost_only: bool = False, point_cap: int | None = None,
                 retry_overflow: bool = True):
    """Batched Dubins(step, max_curv).generation(start, goal) (curve_generation/dubins_curve.py:238-313) on
    pmp_dubins_batch.  starts, goals: [n, 3] poses (x, y, yaw in radians), host arrays or device tensors.
    Returns dict of device tensors: word [n] u8 (_lib.DUBINS_WORDS; 255 = none), tpq [n, 3], cost [n] (in
    curvature-normalised units, as the reference returns it), n_points [n], points [n, point_cap, 3] (x, y,
    yaw; None with cost_only), status (include/pmp.h).  Pairs whose points overflow the first cap are
    re-run with their exact count when retry_overflow."""
    torch, L, ctx = _open()
    s, g, n = _endpoints(torch, starts, goals, 3, torch.float64)
    if int(g.shape[0]) != n:
        raise ValueError("starts and goals must have the same length")
    prm = _lib.DubinsParams(float(step), float(max_curv))
    if point_cap is None:
        point_cap = _dubins_point_cap(torch, s, g, prm.step, prm.max_curv)
    point_cap = max(int(point_cap), 1)

    def launch(s, g, pc):
        m = int(s.shape[0])
        f64 = dict(dtype=torch.float64, device="cuda")
        o = dict(word=torch.empty(m, dtype=torch.uint8, device="cuda"), tpq=torch.empty((m, 3), **f64),
                 cost=torch.empty(m, **f64), n_points=torch.empty(m, dtype=torch.int32, device="cuda"),
                 points=None if cost_only else torch.empty((m, pc, 3), **f64),
                 status=torch.empty(m, dtype=torch.int32, device="cuda"))
        rc = L.pmp_dubins_batch(ctx, _lib.stream_ptr(), ctypes.byref(prm), m, s.data_ptr(), g.data_ptr(),
                                o["word"].data_ptr(), o["tpq"].data_ptr(), o["cost"].data_ptr(), o["n_points"].data_ptr(),
                                pc, _lib.ptr(o["points"]), o["status"].data_ptr())
        _lib.check(ctx, rc, "pmp_dubins_batch")
        return o

    out = launch(s, g, point_cap)
    if retry_overflow and n and not cost_only:
        _retry_overflowed(torch, out, n, point_cap, 3, lambda redo, idx, pc: launch(s[idx].contiguous(), g[idx].contiguous(), pc))
    return out


def dubins_cost_matrix(starts, goals, step: float, max_curv: float):
    """The Dubins steering metric between every start and every goal on pmp_dubins_cost_matrix: starts
    [A, 3], goals [B, 3] poses (x, y, yaw in radians) -> dict of device tensors cost [A, B] f64 and word
    [A, B] u8 of Dubins(step, max_curv).generation(starts[a], goals[b]) (curve_generation/dubins_curve.py:
    253-273), without sampling; the A B pairs are decoded in the kernel."""
    torch, L, ctx = _open()
    s = _dev(torch, starts, torch.float64).reshape(-1, 3)
    g = _dev(torch, goals, torch.float64).reshape(-1, 3)
    A, B = int(s.shape[0]), int(g.shape[0])
    prm = _lib.DubinsParams(float(step), float(max_curv))
    out = dict(cost=torch.empty((A, B), dtype=torch.float64, device="cuda"),
               word=torch.empty((A, B), dtype=torch.uint8, device="cuda"))
    rc = L.pmp_dubins_cost_matrix(ctx, _lib.stream_ptr(), ctypes.byref(prm), A, s.data_ptr(), B, g.data_ptr(),
                                  out["cost"].data_ptr(), out["word"].data_ptr())
    _lib.check(ctx, rc, "pmp_dubins_cost_matrix")
    return out


def _reeds_shepp_point_cap(torch, s, g, step, max_curv):
    """An upper bound of a launch's point counts.  Every candidate but SLS is at most hypot max_curv + 2 of
    straight piece (the circle centres are within 2 of the chord) and three arcs of at most pi each
    (M()'s range; the pi / 2 arcs and CCCC's acos arcs are shorter), so the shortest is within hypot
    max_curv + 4 pi wherever one of them is feasible; over the step, plus the reference's own 5 + 3 list
    slots.  Pairs beyond it (only SLS feasible) are retried; pairs of non-finite poses or of more than
    2^24 steps have no points; 2048 where the parameters give no bound."""
    if not int(s.shape[0]):
        return 1
    if not (step > 0 and max_curv > 0 and math.isfinite(step) and math.isfinite(max_curv)):
        return 2048  # the entry refuses these
    est = (torch.hypot(g[:, 0] - s[:, 0], g[:, 1] - s[:, 1]) * max_curv + 4.0 * math.pi) / step + 8.0
    return int(torch.where(est < float(1 << 24), est, torch.ones_like(est)).max().item())


def reeds_shepp_batch(starts, goals, step: float, max_curv: float, cost_only: bool = False, point_cap: int | None = None,
                      retry_overflow: bool = True, slot_costs: bool = False):
    """Batched ReedsShepp(step, max_curv).generation(start, goal) (curve_generation/reeds_shepp.py:606-674)
    on pmp_reeds_shepp_batch.  starts, goals: [n, 3] poses (x, y, yaw in radians), host arrays or device
    tensors.  Returns dict of device tensors: slot [n] u8 (_lib.RS_WORDS; 255 = none), lengths [n, 5] (signed,
    curvature-normalised, NaN beyond the word's pieces), cost [n] (best_cost / max_curv, as the reference
    returns it), n_points [n], points [n, point_cap, 3] (x, y, yaw; None with cost_only), status
    (include/pmp.h), and with slot_costs=True slot_costs [n, 46]: every candidate's path_length, NaN =
    infeasible.  Pairs whose points overflow the first cap are re-run with their exact count when
    retry_overflow."""
    torch, L, ctx = _open()
    s, g, n = _endpoints(torch, starts, goals, 3, torch.float64)
    if int(g.shape[0]) != n:
        raise ValueError("starts and goals must have the same length")
    prm = _lib.ReedsSheppParams(float(step), float(max_curv))
    if point_cap is None:
        point_cap = _reeds_shepp_point_cap(torch, s, g, prm.step, prm.max_curv)
    point_cap = max(int(point_cap), 1)

    def launch(s, g, pc, with_costs=slot_costs):
        m = int(s.shape[0])
        f64 = dict(dtype=torch.float64, device="cuda")
        o = dict(slot=torch.empty(m, dtype=torch.uint8, device="cuda"), lengths=torch.empty((m, 5), **f64),
                 cost=torch.empty(m, **f64), n_points=torch.empty(m, dtype=torch.int32, device="cuda"),
                 points=None if cost_only else torch.empty((m, pc, 3), **f64),
                 status=torch.empty(m, dtype=torch.int32, device="cuda"))
        if with_costs:
            o["slot_costs"] = torch.empty((m, len(_lib.RS_WORDS)), **f64)
        rc = L.pmp_reeds_shepp_batch(ctx, _lib.stream_ptr(), ctypes.byref(prm), m, s.data_ptr(), g.data_ptr(),
                                     o["slot"].data_ptr(), o["lengths"].data_ptr(), o["cost"].data_ptr(),
                                     _lib.ptr(o.get("slot_costs")), o["n_points"].data_ptr(), pc, _lib.ptr(o["points"]),
                                     o["status"].data_ptr())
        _lib.check(ctx, rc, "pmp_reeds_shepp_batch")
        return o

    out = launch(s, g, point_cap)
    if retry_overflow and n and not cost_only:
        _retry_overflowed(torch, out, n, point_cap, 3,
                          lambda redo, idx, pc: launch(s[idx].contiguous(), g[idx].contiguous(), pc, False))
    return out


def reeds_shepp_cost_matrix(starts, goals, step: float, max_curv: float):
    """The Reeds-Shepp steering metric between every start and every goal on pmp_reeds_shepp_cost_matrix:
    starts [A, 3], goals [B, 3] poses (x, y, yaw in radians) -> dict of device tensors cost [A, B] f64
    (best_cost / max_curv) and slot [A, B] u8 of ReedsShepp(step, max_curv).generation(starts[a], goals[b])
    (curve_generation/reeds_shepp.py:621-637), without sampling; the A B pairs are decoded in the kernel."""
    torch, L, ctx = _open()
    s = _dev(torch, starts, torch.float64).reshape(-1, 3)
    g = _dev(torch, goals, torch.float64).reshape(-1, 3)
    A, B = int(s.shape[0]), int(g.shape[0])
    prm = _lib.ReedsSheppParams(float(step), float(max_curv))
    out = dict(cost=torch.empty((A, B), dtype=torch.float64, device="cuda"),
               slot=torch.empty((A, B), dtype=torch.uint8, device="cuda"))
    rc = L.pmp_reeds_shepp_cost_matrix(ctx, _lib.stream_ptr(), ctypes.byref(prm), A, s.data_ptr(), B, g.data_ptr(),
                                       out["cost"].data_ptr(), out["slot"].data_ptr())
    _lib.check(ctx, rc, "pmp_reeds_shepp_cost_matrix")
    return out


def _polycurve_params(step, max_acc, max_jerk, dt, t_min, t_max):
    return _lib.PolyCurveParams(float(step), float(max_acc), float(max_jerk), float(dt), float(t_min), float(t_max))


def _polycurve_point_cap(prm):
    """The exact largest row count of a launch, ceil((t_max + dt) / dt): every candidate's time is below
    t_max; 1 where the parameters give none (the entry refuses them)."""
    if not (prm.dt > 0 and math.isfinite(prm.dt) and math.isfinite(prm.t_max)):
        return 1
    cap = math.ceil((prm.t_max + prm.dt) / prm.dt)
    return int(cap) if 1 <= cap <= (1 << 24) else 1


def polynomial_batch(starts, goals, step: float, max_acc: float, max_jerk: float, dt: float = 0.1, t_min: float = 1,
                     t_max: float = 30, cost_only: bool = False, point_cap: int | None = None,
                     retry_overflow: bool = True):
    """Batched Polynomial(step, max_acc, max_jerk).generation(start, goal) (curve_generation/
    polynomial_curve.py:104-164) on pmp_polycurve_batch.  starts, goals: [n, 5] states (x, y, yaw in radians,
    v, a), host arrays or device tensors; dt, t_min, t_max are the reference's instance attributes.  Returns
    dict of device tensors: t_index [n] i32 (-1 = no feasible T), T [n] (inf there), n_points [n], points
    [n, point_cap, 7] (time, x, y, yaw, v, a, jerk; None with cost_only), status (include/pmp.h: 1 = no
    feasible T).  Pairs whose rows overflow a caller's point_cap are re-run with their exact count when
    retry_overflow; the default cap holds every candidate."""
    torch, L, ctx = _open()
    s, g, n = _endpoints(torch, starts, goals, 5, torch.float64)
    if int(g.shape[0]) != n:
        raise ValueError("starts and goals must have the same length")
    prm = _polycurve_params(step, max_acc, max_jerk, dt, t_min, t_max)
    if point_cap is None:
        point_cap = _polycurve_point_cap(prm)
    point_cap = max(int(point_cap), 1)

    def launch(s, g, pc):
        m = int(s.shape[0])
        i32 = dict(dtype=torch.int32, device="cuda")
        o = dict(t_index=torch.empty(m, **i32), T=torch.empty(m, dtype=torch.float64, device="cuda"),
                 n_points=torch.empty(m, **i32),
                 points=None if cost_only else torch.empty((m, pc, 7), dtype=torch.float64, device="cuda"),
                 status=torch.empty(m, **i32))
        rc = L.pmp_polycurve_batch(ctx, _lib.stream_ptr(), ctypes.byref(prm), m, s.data_ptr(), g.data_ptr(),
                                   o["t_index"].data_ptr(), o["T"].data_ptr(), o["n_points"].data_ptr(), pc,
                                   _lib.ptr(o["points"]), o["status"].data_ptr())
        _lib.check(ctx, rc, "pmp_polycurve_batch")
        return o

    out = launch(s, g, point_cap)
    if retry_overflow and n and not cost_only:
        _retry_overflowed(torch, out, n, point_cap, 7, lambda redo, idx, pc: launch(s[idx].contiguous(), g[idx].contiguous(), pc))
    return out


def polynomial_time_matrix(starts, goals, step: float, max_acc: float, max_jerk: float, dt: float = 0.1,
                           t_min: float = 1, t_max: float = 30):
    """The minimum-time metric between every start and every goal state on pmp_polycurve_time_matrix: starts
    [A, 5], goals [B, 5] states (x, y, yaw in radians, v, a) -> dict of device tensors T [A, B] f64 (inf where
    no candidate is feasible) and t_index [A, B] i32 (-1 there) of Polynomial(step, max_acc,
    max_jerk).generation(starts[a], goals[b]) (curve_generation/polynomial_curve.py:130-160), without
    sampling; the A B pairs are decoded in the kernel."""
    torch, L, ctx = _open()
    s = _dev(torch, starts, torch.float64).reshape(-1, 5)
    g = _dev(torch, goals, torch.float64).reshape(-1, 5)
    A, B = int(s.shape[0]), int(g.shape[0])
    prm = _polycurve_params(step, max_acc, max_jerk, dt, t_min, t_max)
    out = dict(T=torch.empty((A, B), dtype=torch.float64, device="cuda"),
               t_index=torch.empty((A, B), dtype=torch.int32, device="cuda"))
    rc = L.pmp_polycurve_time_matrix(ctx, _lib.stream_ptr(), ctypes.byref(prm), A, s.data_ptr(), B, g.data_ptr(),
                                     out["T"].data_ptr(), out["t_index"].data_ptr())
    _lib.check(ctx, rc, "pmp_polycurve_time_matrix")
    return out


def _bezier_point_cap(torch, s, g, step):
    """The largest int(hypot / step) of a launch (a pair whose count the device rounds one higher is
    retried; pairs of non-finite poses or of more than 2^24 points have no points); 1 where the step gives
    none (the entry refuses it)."""
    if not int(s.shape[0]) or not (step > 0 and math.isfinite(step)):
        return 1
    est = torch.hypot(s[:, 0] - g[:, 0], s[:, 1] - g[:, 1]) / step
    return max(int(torch.where(est < float(1 << 24), est, torch.ones_like(est)).max().item()), 1)


def bezier_batch(starts, goals, step: float, offset: float, cost_only: bool = False, point_cap: int | None = None,
                 retry_overflow: bool = True):
    """Batched Bezier(step, offset).generation(start, goal) (curve_generation/bezier_curve.py:34-89) on
    pmp_bezier_batch.  starts, goals: [n, 3] poses (x, y, yaw in radians), host arrays or device tensors.
    Returns dict of device tensors: control [n, 4, 2], n_points [n], points [n, point_cap, 2] (x, y; None with
    cost_only), status (include/pmp.h: 4 = a non-finite pose, where the reference raises).  Pairs whose
    points overflow the first cap are re-run with their exact count when retry_overflow."""
    torch, L, ctx = _open()
    s, g, n = _endpoints(torch, starts, goals, 3, torch.float64)
    if int(g.shape[0]) != n:
        raise ValueError("starts and goals must have the same length")
    prm = _lib.BezierParams(float(step), float(offset))
    if point_cap is None:
        point_cap = _bezier_point_cap(torch, s, g, prm.step)
    point_cap = max(int(point_cap), 1)

    def launch(s, g, pc):
        m = int(s.shape[0])
        f64 = dict(dtype=torch.float64, device="cuda")
        o = dict(control=torch.empty((m, 4, 2), **f64), n_points=torch.empty(m, dtype=torch.int32, device="cuda"),
                 points=None if cost_only else torch.empty((m, pc, 2), **f64),
                 status=torch.empty(m, dtype=torch.int32, device="cuda"))
        rc = L.pmp_bezier_batch(ctx, _lib.stream_ptr(), ctypes.byref(prm), m, s.data_ptr(), g.data_ptr(),
                                o["control"].data_ptr(), o["n_points"].data_ptr(), pc, _lib.ptr(o["points"]),
                                o["status"].data_ptr())
        _lib.check(ctx, rc, "pmp_bezier_batch")
        return o

    out = launch(s, g, point_cap)
    if retry_overflow and n and not cost_only:
        _retry_overflowed(torch, out, n, point_cap, 2, lambda redo, idx, pc: launch(s[idx].contiguous(), g[idx].contiguous(), pc))
    return out


def _pack_waypoints(torch, curves, entry, dims=(2, 3)):
    """The waypoint lists of a launch as (flat [sum n, dim] f64, off [m + 1] i32 device tensors, host off, dim):
    `curves` is a list of [n, dim] arrays (one dim for all) or (flat, off) already packed that way."""
    if isinstance(curves, tuple) and len(curves) == 2 and hasattr(curves[1], "dtype") and getattr(curves[1], "ndim", 0) == 1:
        flat = _dev(torch, curves[0], torch.float64)
        flat = flat.reshape(-1, flat.shape[-1]) if flat.dim() >= 2 else flat.reshape(0, 2)
        off = _dev(torch, curves[1], torch.int32).reshape(-1)
        host = off.cpu().numpy()
    else:
        arrs = [np.asarray(c, np.float64) for c in curves]
        arrs = [a.reshape(-1, a.shape[-1] if a.ndim >= 2 else 2) for a in arrs]
        if len({a.shape[1] for a in arrs}) > 1:
            raise ValueError(f"{entry}: every curve of a launch must have the same dimension")
        host = np.zeros(len(arrs) + 1, np.int32)
        host[1:] = np.cumsum([len(a) for a in arrs])
        flat = torch.as_tensor(np.concatenate(arrs) if arrs else np.zeros((0, 2)), device="cuda")
        off = torch.as_tensor(host, device="cuda")
    if len(host) < 1 or host[0] != 0 or np.any(np.diff(host) < 0) or int(host[-1]) != int(flat.shape[0]):
        raise ValueError(f"{entry}: off must rise from 0 to the number of packed waypoints")
    return flat, off, host, int(flat.shape[1])


def bspline_samples(step: float, three_d: bool = False) -> int:
    """len(t) of BSpline.run (bspline_curve.py:232: int(1 / step)) or BSpline3D.run (at least 2)."""
    n = int(1 / step)
    return max(2, n) if three_d else n


def bspline_batch(curves, step: float, k: int, param_mode: str = "centripetal", spline_mode: str = "interpolation",
                  cost_only: bool = False, three_d: bool = False, params=None, knot=None):
    """Batched BSpline(step, k, param_mode, spline_mode).run(points) (curve_generation/bspline_curve.py:219-271),
    or BSpline3D's with three_d (bspline_curve3d.py:164-220), on pmp_bspline_batch: one wave per curve.
    curves: list of [n, 2 | 3] waypoint arrays, or (flat [sum n, dim], off [m + 1] i32) device tensors.
    params [m, n_max] / knot [m, n_max + k + 1] (optional): use these instead of paramSelection / knotGeneration.
    Returns dict of device tensors: params [m, n_max], knot [m, n_max + k + 1], control [m, n_max, dim],
    n_control [m], points [m, T, dim] (None with cost_only), length [m], status [m] (include/pmp.h: 4 where the
    reference raises LinAlgError), and n_samples = T, the same for every curve."""
    torch, L, ctx = _open()
    entry = "pmp_bspline_batch"
    if param_mode not in _lib.BSPLINE_PARAM_MODES or spline_mode not in _lib.BSPLINE_SPLINE_MODES:
        raise ValueError("unknown param_mode / spline_mode")
    flat, off, host, dim = _pack_waypoints(torch, curves, entry)
    m = len(host) - 1
    counts = np.diff(host)
    lo, hi = (int(counts.min()), int(counts.max())) if m else (2, 2)
    step = float(step)
    T = bspline_samples(step, three_d) if step > 0 and math.isfinite(step) and 1 / step <= 1 << 24 else 0
    prm = _lib.BSplineParams(step, int(k), _lib.BSPLINE_PARAM_MODES.index(param_mode),
                             _lib.BSPLINE_SPLINE_MODES.index(spline_mode), 1 if three_d else 0)
    nm = max(hi, 2)
    nk = nm + max(int(k), 0) + 1
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    pin = None if params is None else _dev(torch, params, torch.float64).reshape(m, nm)
    kin = None if knot is None else _dev(torch, knot, torch.float64).reshape(m, nk)
    out = dict(params=torch.empty((m, nm), **f64), knot=torch.empty((m, nk), **f64),
               control=torch.empty((m, nm, dim), **f64), n_control=torch.empty(m, **i32),
               points=None if cost_only else torch.empty((m, max(T, 0), dim), **f64), length=torch.empty(m, **f64),
               status=torch.empty(m, **i32), n_samples=T)
    rc = L.pmp_bspline_batch(ctx, _lib.stream_ptr(), ctypes.byref(prm), m, flat.data_ptr(), off.data_ptr(), dim, lo, hi,
                             _lib.ptr(pin), _lib.ptr(kin), out["params"].data_ptr(), out["knot"].data_ptr(),
                             out["control"].data_ptr(), out["n_control"].data_ptr(), T, _lib.ptr(out["points"]),
                             out["length"].data_ptr(), out["status"].data_ptr())
    _lib.check(ctx, rc, entry)
    return out


def cubic_spline_batch(curves, step: float, cost_only: bool = False, point_cap: int | None = None,
                       retry_overflow: bool = True, with_derivative: bool = False):
    """Batched CubicSpline(step).run(points) (curve_generation/cubic_spline.py:84-111) on
    pmp_cubic_spline_batch: one wave per waypoint list.  curves: list of [n, 2 | 3] arrays (x, y first), or
    (flat, off) device tensors.  Returns dict of device tensors: arc_length [m] (s[-1]), n_points [m], points
    [m, point_cap, 3] (x, y, yaw; 5 columns with with_derivative: dx, dy too; None with cost_only), status
    (include/pmp.h: 4 where np.arange raises).  Lists whose points overflow the first cap are re-run with
    their exact count when retry_overflow."""
    torch, L, ctx = _open()
    entry = "pmp_cubic_spline_batch"
    flat, off, host, dim = _pack_waypoints(torch, curves, entry)
    m = len(host) - 1
    step = float(step)
    prm = _lib.CubicSplineParams(step, 1 if with_derivative else 0, 0)
    row = 5 if with_derivative else 3
    if point_cap is None:  # the polyline's length / step, from the device's own rounding of it, plus slack
        point_cap = 1
        if m and int(flat.shape[0]) >= 2 and step > 0 and math.isfinite(step):
            d = flat[1:, :2] - flat[:-1, :2]
            seg = torch.hypot(d[:, 0], d[:, 1])
            seg[torch.as_tensor(host[1:-1].astype(np.int64) - 1, device="cuda")] = 0  # the joints between lists
            cs = torch.cat([torch.zeros(1, **dict(dtype=torch.float64, device="cuda")), torch.cumsum(seg, 0)])
            o = torch.as_tensor(host.astype(np.int64), device="cuda")
            tot = cs[torch.clamp(o[1:] - 1, min=0)] - cs[torch.clamp(o[:-1], max=int(flat.shape[0]) - 1)]
            est = torch.ceil(tot / step) + 1
            est = torch.where(torch.isfinite(est) & (est < float(1 << 24)), est, torch.ones_like(est))
            point_cap = max(int(est.max().item()), 1)
    point_cap = max(int(point_cap), 1)

    def launch(flat, off, host, pc):
        n = len(host) - 1
        counts = np.diff(host)
        lo, hi = (int(counts.min()), int(counts.max())) if n else (2, 2)
        f64 = dict(dtype=torch.float64, device="cuda")
        i32 = dict(dtype=torch.int32, device="cuda")
        o = dict(arc_length=torch.empty(n, **f64), n_points=torch.empty(n, **i32),
                 points=None if cost_only else torch.empty((n, pc, row), **f64), status=torch.empty(n, **i32))
        rc = L.pmp_cubic_spline_batch(ctx, _lib.stream_ptr(), ctypes.byref(prm), n, flat.data_ptr(), off.data_ptr(), dim,
                                      lo, hi, o["arc_length"].data_ptr(), o["n_points"].data_ptr(), pc,
                                      _lib.ptr(o["points"]), o["status"].data_ptr())
        _lib.check(ctx, rc, entry)
        return o

    def rerun(redo, idx, pc):
        cnt = np.diff(host)[redo]
        rows = torch.as_tensor(np.concatenate([np.arange(host[i], host[i + 1], dtype=np.int64) for i in redo]), device="cuda")
        h2 = np.zeros(len(redo) + 1, np.int32)
        h2[1:] = np.cumsum(cnt)
        return launch(flat[rows].contiguous(), torch.as_tensor(h2, device="cuda"), h2, pc)

    out = launch(flat, off, host, point_cap)
    if retry_overflow and m and not cost_only:
        _retry_overflowed(torch, out, m, point_cap, row, rerun)
    return out


def pso_default_waves() -> int:
    """The wave64s per workgroup pmp_pso_batch launches unless told otherwise (csrc/pso.hip kDefaultWaves)."""
    return int(_lib.load_library().pmp_pso_default_waves())


def pso_draws(n_particles: int, point_num: int, max_iter: int) -> int:
    """The random.random() draws of PSO.plan()'s iterations: two per point, particle and iteration."""
    return 2 * int(point_num) * int(n_particles) * int(max_iter)


def pso_batch(env_or_occ, starts, goals, init_positions, rnd, n_particles: int, point_num: int, max_iter: int,
              w_inertial: float = 1.0, w_cognitive: float = 1.0, w_social: float = 1.0, max_speed: float = 6,
              trace: bool = False, waves: int | None = None):
    """Batched PSO.plan() after initializePositions() (global_planner/evolutionary_search/pso.py:77-123) on
    pmp_pso_batch: one workgroup per plan, all plans on one grid.
    env_or_occ: a Grid or a uint8 [W, H] occupancy; starts, goals [nq, 2] int; init_positions
    [nq, n_particles, point_num, 2] int (initializePositions() of each plan); rnd [nq, stride] f64, each plan's
    random.random() stream of at least pso_draws() values; waves: wave64s per workgroup (None: the default; the
    results do not depend on it).
    Returns dict of device tensors: status [nq] (4 where the best fitness is inf), best_position [nq, point_num, 2]
    i32, best_fitness [nq], fitness_history [nq, max_iter], positions [nq, n_particles, point_num, 2] i32,
    velocities (same shape, f64), fitness and particle_best_fitness [nq, n_particles], points [nq, 100, 2] and
    length [nq] (the best particle's curve), repeats [nq] i64 (evaluations thrown away because an earlier particle
    replaced the global best), and with trace: trace_positions [nq, max_iter, n_particles, point_num, 2] i32 and
    trace_fitness [nq, max_iter, n_particles] (else None)."""
    torch, L, ctx = _open()
    entry = "pmp_pso_batch"
    occ_bits, W, H = _occ2d(torch, env_or_occ)
    s, g, nq = _endpoints(torch, starts, goals, 2, torch.int32)
    n, pn, iters = int(n_particles), int(point_num), int(max_iter)
    an, apn, ait = max(n, 0), max(pn, 0), max(iters, 0)  # what the outputs are sized by; the entry refuses the rest
    if isinstance(init_positions, torch.Tensor):
        init = _dev(torch, init_positions, torch.int32).reshape(-1, 2)
        lo, hi = (init.amin(0).tolist(), init.amax(0).tolist()) if init.shape[0] else ([0, 0], [0, 0])
    else:
        host = np.ascontiguousarray(init_positions, dtype=np.int32).reshape(-1, 2)
        lo, hi = (host.min(0).tolist(), host.max(0).tolist()) if len(host) else ([0, 0], [0, 0])
        init = torch.as_tensor(host, device="cuda")
    if n >= 1 and pn >= 1 and int(init.shape[0]) != nq * n * pn:
        raise ValueError(f"{entry}: init_positions must be [nq, n_particles, point_num, 2]")
    bounds = (ctypes.c_int32 * 4)(int(lo[0]), int(lo[1]), int(hi[0]), int(hi[1]))
    rnd = _dev(torch, rnd, torch.float64).reshape(nq, -1) if nq else _dev(torch, rnd, torch.float64).reshape(0, 0)
    prm = _lib.PSOParams(W, H, n, pn, iters, int(waves or 0), float(w_inertial), float(w_cognitive), float(w_social),
                         float(max_speed))
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    out = dict(status=torch.empty(nq, **i32), best_position=torch.empty((nq, apn, 2), **i32),
               best_fitness=torch.empty(nq, **f64), fitness_history=torch.empty((nq, ait), **f64),
               positions=torch.empty((nq, an, apn, 2), **i32), velocities=torch.empty((nq, an, apn, 2), **f64),
               fitness=torch.empty((nq, an), **f64), particle_best_fitness=torch.empty((nq, an), **f64),
               points=torch.empty((nq, 100, 2), **f64), length=torch.empty(nq, **f64),
               repeats=torch.empty(nq, dtype=torch.int64, device="cuda"),
               trace_positions=torch.empty((nq, ait, an, apn, 2), **i32) if trace else None,
               trace_fitness=torch.empty((nq, ait, an), **f64) if trace else None)
    rc = L.pmp_pso_batch(ctx, _lib.stream_ptr(), ctypes.byref(prm), occ_bits.data_ptr(), nq, s.data_ptr(), g.data_ptr(),
                         init.data_ptr(), bounds, rnd.data_ptr(), int(rnd.shape[1]), out["status"].data_ptr(),
                         out["best_position"].data_ptr(), out["best_fitness"].data_ptr(),
                         out["fitness_history"].data_ptr(), out["positions"].data_ptr(), out["velocities"].data_ptr(),
                         out["fitness"].data_ptr(), out["particle_best_fitness"].data_ptr(), out["points"].data_ptr(),
                         out["length"].data_ptr(), out["repeats"].data_ptr(), _lib.ptr(out["trace_positions"]),
                         _lib.ptr(out["trace_fitness"]))
    _lib.check(ctx, rc, entry)
    return out


def aco_default_waves() -> int:
    """The wave64s (plans) per workgroup pmp_aco_batch launches unless told otherwise (csrc/aco.hip kDefaultWaves)."""
    return int(_lib.load_library().pmp_aco_default_waves())


def aco_max_waves() -> int:
    """The most waves per workgroup pmp_aco_batch takes."""
    return int(_lib.load_library().pmp_aco_max_waves())


def aco_path_cap(x_range: int, y_range: int) -> int:
    """Entries of an ant's path: ceil(x_range * y_range / 2 + max(x_range, y_range)) choices (aco.py:86, :95) and
    the goal.  No library call: the same rule as pmp_aco_path_cap."""
    return math.ceil(x_range * y_range / 2 + max(x_range, y_range)) + 1


def _mt_words(torch, states):
    """[n, 625] uint32 state words (as int32 bits) on the device, from arrays or random.getstate() tuples"""
    rows = [np.asarray(s[1] if isinstance(s, tuple) and len(s) == 3 and isinstance(s[1], tuple) else s, np.uint32)
            for s in states]
    a = np.ascontiguousarray(np.stack(rows)) if rows else np.zeros((0, 625), np.uint32)
    if a.ndim != 2 or a.shape[1] != 625:
        raise ValueError("an MT19937 state is 624 words and the index")
    return torch.as_tensor(a.view(np.int32), device="cuda")


def mt19937_doubles(state, n: int):
    """The next n values of random.random() from `state` (a random.getstate() tuple or its 625 words) by the
    kernels' generator (csrc/mt19937_dev.h, pmp_mt19937_doubles).  Returns (device f64 [n], numpy uint32 [625]
    state after them)."""
    torch, L, ctx = _open()
    words = _mt_words(torch, [state])
    out = torch.empty(max(int(n), 0), dtype=torch.float64, device="cuda")
    after = torch.empty(625, dtype=torch.int32, device="cuda")
    rc = L.pmp_mt19937_doubles(ctx, _lib.stream_ptr(), words.data_ptr(), int(n), out.data_ptr(), after.data_ptr())
    _lib.check(ctx, rc, "pmp_mt19937_doubles")
    return out, after.cpu().numpy().view(np.uint32)


def aco_batch(env_or_occ, starts, goals, heur, heur_of, mt_states, n_ants: int = 50, max_iter: int = 100,
              alpha: float = 1.0, one_minus_rho: float = 0.9, Q: float = 1.0, trace: bool = False,
              waves: int | None = None):
    """Batched ACO.plan() (global_planner/evolutionary_search/aco.py:65-166) on pmp_aco_batch: one wave64 per
    plan, all plans on one grid, the random.random() draws made in the kernel.
    env_or_occ: a Grid or a uint8 [W, H] occupancy; starts, goals [nq, 2] int; heur [n_tables, W * H] f64, the
    host's (1.0 / h(cell, goal)) ** beta per cell x * H + y (finite for every free cell); heur_of [nq] int, each
    plan's table; mt_states: per plan a random.getstate() tuple or its 625 words; one_minus_rho: the host's
    1 - rho; waves: plans per workgroup (None: the default; the results do not depend on it).
    Scratch per plan, allocated here: the pheromone, W * H * 64 bytes; the iteration's paths, n_ants *
    aco_path_cap(W, H) * 2 bytes (a default plan on the 51 x 31 map: 50 ants x 843 entries, 84 KB, beside 101 KB
    of pheromone); 4 * n_ants bytes of lengths.
    Returns dict of device tensors: status [nq] (0 a path, 1 no ant found the goal, 5 the reference raises
    IndexError), best_len [nq], best_path [nq, cap] i32 cell ids (start first; past best_len zeros or what an
    earlier, longer best path left), n_cost [nq], cost_list
    [nq, max_iter] i32, draws [nq] i64, mt_state_out [nq, 625] (uint32 bits in int32), and with trace ant_found,
    ant_len [nq, max_iter, n_ants] i32 and pheromone [nq, W * H, 8] f64 (else None)."""
    torch, L, ctx = _open()
    entry = "pmp_aco_batch"
    occ_bits, W, H = _occ2d(torch, env_or_occ)
    s, g, nq = _endpoints(torch, starts, goals, 2, torch.int32)
    na, it = int(n_ants), int(max_iter)
    ana, ait = max(na, 0), max(it, 0)  # what the outputs are sized by; the entry refuses the rest
    cells = W * H
    cap = int(L.pmp_aco_path_cap(W, H))
    heur = _dev(torch, heur, torch.float64).reshape(-1, max(cells, 1))
    heur_of = _dev(torch, heur_of, torch.int32).reshape(-1)
    states = mt_states if isinstance(mt_states, torch.Tensor) else _mt_words(torch, mt_states)
    states = states.to(device="cuda", dtype=torch.int32).contiguous().reshape(-1, 625)
    if int(heur_of.shape[0]) != nq or int(states.shape[0]) != nq:
        raise ValueError(f"{entry}: heur_of and mt_states must have one entry per plan")
    prm = _lib.ACOParams(W, H, na, it, int(waves or 0), 0, float(alpha), float(one_minus_rho), float(Q))
    i32 = dict(dtype=torch.int32, device="cuda")
    out = dict(status=torch.empty(nq, **i32), best_len=torch.empty(nq, **i32), best_path=torch.zeros((nq, max(cap, 1)), **i32),
               n_cost=torch.empty(nq, **i32), cost_list=torch.zeros((nq, ait), **i32),
               draws=torch.empty(nq, dtype=torch.int64, device="cuda"), mt_state_out=torch.empty((nq, 625), **i32),
               ant_found=torch.zeros((nq, ait, ana), **i32) if trace else None,
               ant_len=torch.zeros((nq, ait, ana), **i32) if trace else None)
    big = cap > 0  # a grid the entry refuses gets no scratch
    pher = torch.empty((nq, cells if big else 1, 8), dtype=torch.float64, device="cuda")
    paths = torch.empty((nq, ana, cap if big else 1), dtype=torch.int16, device="cuda")
    lens = torch.empty((nq, max(ana, 1)), **i32)
    rc = L.pmp_aco_batch(ctx, _lib.stream_ptr(), ctypes.byref(prm), occ_bits.data_ptr(), nq, s.data_ptr(), g.data_ptr(),
                         heur.data_ptr(), int(heur.shape[0]), heur_of.data_ptr(), states.data_ptr(),
                         out["status"].data_ptr(), out["best_len"].data_ptr(), out["best_path"].data_ptr(),
                         out["n_cost"].data_ptr(), out["cost_list"].data_ptr(), out["draws"].data_ptr(),
                         out["mt_state_out"].data_ptr(), _lib.ptr(out["ant_found"]), _lib.ptr(out["ant_len"]),
                         pher.data_ptr(), paths.data_ptr(), lens.data_ptr())
    _lib.check(ctx, rc, entry)
    out["pheromone"] = pher if trace else None
    out["W"], out["H"] = W, H
    return out
