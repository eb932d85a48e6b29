/*
 * pmp.h -- C-ABI of libpmp_hip.so, the MI355X (gfx950) batched motion-planning core.
 *
 * The reference (Slenderman00/python_motion_planning, pure Python) has no FFI of its own; the
 * boundary it exposes for the hot path is the Planner plug-in API:
 *     Planner.plan() (utils/planner/planner.py:28-33), SearchFactory (search_factory.py:13-51),
 *     ControlFactory (control_factory.py:13-27) and one iteration of LocalPlanner.plan loops.
 * Each entry point below replaces the inner loop of one reference call; the Python host package
 * python_motion_planning_amd binds them with ctypes.
 *
 * Conventions
 *  - Every array pointer is a DEVICE pointer owned by the caller (e.g. torch tensor.data_ptr()),
 *    contiguous, with the dtype written in the signature.  The library never frees caller memory
 *    and allocates only grow-only scratch inside its pmp_ctx.
 *  - Calls are asynchronous on `stream` (a hipStream_t; NULL = default stream).
 *  - Return value: 0 = OK, PMP_EINVAL / PMP_ENOMEM / PMP_EHIP < 0; text via pmp_last_error().
 *  - Per-query status: 0 found, 1 no path, 2 path_cap overflow, 3 heap/expand/capacity overflow,
 *    4 "the reference raises" (D* unreachable -> AttributeError at d_star.py:234).
 *  - Grid cells: occupancy bit-packed x-major, cell id c = x*H + y, bit c at word c>>5, bit c&31
 *    (utils/environment/env.py:41-80 stores obstacles as (x, y) tuples).
 *  - A pmp_ctx must not be used by two host threads at once.
 */
#ifndef PMP_H
#define PMP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMP_OK 0
#define PMP_EINVAL (-1)
#define PMP_ENOMEM (-2)
#define PMP_EHIP (-3)

#define PMP_FOUND 0
#define PMP_NO_PATH 1
#define PMP_PATH_OVERFLOW 2
#define PMP_CAP_OVERFLOW 3
#define PMP_REF_RAISES 4
#define PMP_REF_INDEX_ERROR 5 /* pmp_aco_batch: the reference's roulette indexes past its list (IndexError) */

typedef struct pmp_ctx pmp_ctx;

/* Create a context bound to HIP device `device`; NULL on failure. */
pmp_ctx* pmp_create(int device);
void pmp_destroy(pmp_ctx* ctx);
const char* pmp_last_error(pmp_ctx* ctx);
/* Library version string (static). */
const char* pmp_version(void);

/*
 * Batched 2D A*.  Replaces AStar.plan (global_planner/graph_search/a_star.py:39-83) with its
 * getNeighbor (:85-96), GraphSearcher.h / isCollision (graph_search.py:30-87), CPython heapq
 * ordered by Node.__lt__ (utils/environment/node.py:51-54) and extractPath (:98-117).
 *   occ_bits   [ceil(W*H/32)] u32   shared occupancy of the Grid
 *   heuristic  0 euclidean, 1 manhattan
 *   start_xy, goal_xy  [nq][2] i32
 *   cost       [nq] f64             path cost (sum of hypot, goal->start order)
 *   path_len   [nq] i32             number of cells on the path (goal->start, reference order)
 *   path       [nq][path_cap] u32   cell ids, goal first
 *   n_expanded [nq] i32             len(CLOSED) == len(expand) of the reference
 *   expand     [nq][expand_cap] u32 nullable; CLOSED in insertion order, cell | parent_dir<<28
 *              (parent_dir = motion index of env.py:52-55 that reached the cell, 8 = start)
 *   counters   [nq][4] i64          nullable; pushes, pops, expansions, max heap size
 *   status     [nq] i32
 * W, H <= 8192.  Cells outside [0,W)x[0,H) are blocked (the reference relies on boundary walls).
 */
int pmp_astar2d_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int W, int H, int heuristic,
                      const int32_t* start_xy, const int32_t* goal_xy, int nq, double* cost,
                      int32_t* path_len, uint32_t* path, int path_cap, int32_t* n_expanded,
                      uint32_t* expand, int expand_cap, int64_t* counters, int32_t* status);

/* Planners that share the AStar loop (2D: a_star.py:39-83; 3D: a_star3d.py:33-78). */
enum { PMP_ALGO_ASTAR = 0, PMP_ALGO_DIJKSTRA = 1, PMP_ALGO_GBFS = 2, PMP_ALGO_THETA = 3, PMP_ALGO_LAZY_THETA = 4 };

/*
 * Batched 2D AStar / Dijkstra / GBFS.  algo = PMP_ALGO_ASTAR is pmp_astar2d_batch;
 * PMP_ALGO_DIJKSTRA replaces Dijkstra.plan (global_planner/graph_search/dijkstra.py:36-85: node_n.h
 * = 0, so `heuristic` is unused); PMP_ALGO_GBFS replaces GBFS.plan (gbfs.py:36-86: node_n.g = 0,
 * ordered by h).  PMP_ALGO_THETA replaces ThetaStar.plan (theta_star.py:44-171: updateVertex with
 * the Bresenham lineOfSight) and PMP_ALGO_LAZY_THETA LazyThetaStar.plan (lazy_theta_star.py:38-114:
 * the line of sight at the pop); both need H <= 4096, and their expand records are
 * cell | code << 26 (code 0-7 path 1 via motion d, 8 start, 16+d path 2, 24+d Lazy Theta*'s
 * re-parenting to the CLOSED neighbour in motion d, +32 g = inf).  Same loop, CPython heap ties,
 * goal -> start path and arguments as pmp_astar2d_batch; cost is extractPath's (a_star.py:98-117).
 */
int pmp_graph2d_batch(pmp_ctx* ctx, void* stream, int algo, const uint32_t* occ_bits, int W, int H, int heuristic,
                      const int32_t* start_xy, const int32_t* goal_xy, int nq, double* cost,
                      int32_t* path_len, uint32_t* path, int path_cap, int32_t* n_expanded,
                      uint32_t* expand, int expand_cap, int64_t* counters, int32_t* status);

/*
 * Batched 3D A*.  Replaces AStar3D.plan (global_planner/graph_search/a_star3d.py:33-106) with
 * GraphSearcher3D.h / isCollision (graph_search_3d.py:30-107) over Grid3D's 26 motions
 * (utils/environment/env3d.py:56-70) and the (f, h, counter) tuple heap.
 *   occ_bits  per_query ? [nq][ceil(X*Y*Z/32)] : [ceil(X*Y*Z/32)] u32, cell (x*Y + y)*Z + z
 *   start_xyz, goal_xyz [nq][3] i32;  X, Y, Z <= 256
 *   cost      [nq] f64   inf when unreachable (a_star3d.py:77-78)
 *   path      [nq][path_cap] u32 cells start -> goal;  n_expanded = len(CLOSED) (distinct cells)
 *   expand    nullable [nq][expand_cap] u32 cells in first-insertion order of CLOSED
 *   counters  nullable [nq][4] i64 pushes, pops, expansions (incl. re-expansions), max heap size
 * An endpoint outside the grid is not searched: status 1, cost inf, path_len 0; a start inside the grid
 * is the one CLOSED cell (n_expanded 1, expand[0] = the start; 0 with the start outside) and the
 * counters are 1, 1, n_expanded, 1.  (With the goal alone outside, the reference closes the start's
 * whole component before it returns the same inf and [].)
 */
int pmp_astar3d_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int per_query, int X, int Y, int Z,
                      int heuristic, const int32_t* start_xyz, const int32_t* goal_xyz, int nq, double* cost,
                      int32_t* path_len, uint32_t* path, int path_cap, int32_t* n_expanded, uint32_t* expand,
                      int expand_cap, int64_t* counters, int32_t* status);

/*
 * Batched 3D AStar3D / Dijkstra3D / GBFS3D.  algo = PMP_ALGO_ASTAR is pmp_astar3d_batch;
 * PMP_ALGO_DIJKSTRA replaces Dijkstra3D.plan (global_planner/graph_search/dijkstra3d.py:39-87: key
 * (g, 0.0, counter), `heuristic` unused; its getNeighbor (:89-126) equals isCollision plus an
 * in-bounds test, and cells outside the grid are blocked here); PMP_ALGO_GBFS replaces
 * GBFS3D.plan (gbfs3d.py:34-82: key (h, counter), CLOSED membership tests); PMP_ALGO_THETA
 * replaces ThetaStar3D.plan (theta_star3d.py:38-110: at each push, the expanding node's CLOSED
 * parent becomes the neighbour's parent when lineOfSight(neighbour, parent) (Bresenham, :139-213)
 * holds and it is cheaper); PMP_ALGO_LAZY_THETA replaces LazyThetaStar3D.plan
 * (lazy_theta_star3d.py:41-128: that update without the test, the test deferred to the pop, where
 * a failed line of sight re-parents the node to its best CLOSED neighbour).  Same arguments as
 * pmp_astar3d_batch; cost is extractPath's (Planner3D.dist along the path) for all five; any-voxel
 * parents make paths shorter than their cell counts suggest.
 */
int pmp_graph3d_batch(pmp_ctx* ctx, void* stream, int algo, const uint32_t* occ_bits, int per_query, int X, int Y,
                      int Z, int heuristic, const int32_t* start_xyz, const int32_t* goal_xyz, int nq, double* cost,
                      int32_t* path_len, uint32_t* path, int path_cap, int32_t* n_expanded, uint32_t* expand,
                      int expand_cap, int64_t* counters, int32_t* status);

/*
 * Batched 3D Jump Point Search.  Replaces JPS3D.plan (global_planner/graph_search/jps3d.py:42-88):
 * AStar3D's loop and (f, h, counter) heap with the 26 jump() results (:96-155, forced neighbours
 * :164-244, isCollision graph_search_3d.py:66-107 with Python-int coordinates) as the neighbour set,
 * g(jump point) = g(node) + math.sqrt of the integer square distance (_mk_qnode, :158-160), cost
 * and path by extractPath over CLOSED parents (:248-261); the path lists jump points only.  jump()
 * is evaluated in its collapsed form (csrc/jps3d.hip): a plane-diagonal jump returns the adjacent
 * cell whenever a goal / forced / axis-jump step lies on its ray, a space-diagonal jump the first
 * such step or the first from which a plane-diagonal jump succeeds.
 * Arguments and statuses as pmp_graph3d_batch (inf cost, status 1, path_len 0 when OPEN empties or
 * an endpoint lies outside the grid), and:
 *   expand         nullable [nq][expand_cap] u32 CLOSED cells in first-insertion order
 *   expand_parent  nullable [nq][expand_cap] u32 the final CLOSED parent cell of each of those cells
 *                  (after any re-expansion; the start's parent is the start); needs expand
 *   expand_g       nullable [nq][expand_cap] f64 their final CLOSED g; needs expand
 *   counters       nullable [nq][4] i64 the reference's pushes, pops, expansions (incl. re-expansions),
 *                  max heap size
 * PMP_CAP_OVERFLOW when the heap or the push counter (64 per cell) overflows.
 */
int pmp_jps3d_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int per_query, int X, int Y, int Z,
                    int heuristic, const int32_t* start_xyz, const int32_t* goal_xyz, int nq, double* cost,
                    int32_t* path_len, uint32_t* path, int path_cap, int32_t* n_expanded, uint32_t* expand,
                    uint32_t* expand_parent, double* expand_g, int expand_cap, int64_t* counters, int32_t* status);

/*
 * Batched 2D Jump Point Search.  Replaces JPS.plan (global_planner/graph_search/jps.py:38-83):
 * heappop under Node.__lt__ with CPython heapq's tie behaviour (the heap array equals CPython's after
 * every push and pop), a pop skipped when its cell is in CLOSED (:56-57, no g comparison), the goal
 * test (:60-63), the 8 jump() results (:85-121, forced neighbours :123-164) in the motion order of
 * env.py:52-55, each kept when its cell is not in CLOSED (:69) and pushed in that order until the
 * goal has been pushed (:74-80), then CLOSED[node.current] = node (:82).  g(jump point) adds the
 * motion's cost (1 or math.sqrt(2)) once per step of the jump (Node.__add__ at :97), h is
 * GraphSearcher.h; cost and path by AStar.extractPath over the CLOSED parents (a_star.py:98-117):
 * math.hypot per leg, accumulated goal -> start; the path lists jump points only.  jump() is
 * evaluated in its collapsed form (csrc/jps2d.hip): an axis ray returns the first goal or forced
 * cell before an obstacle, a diagonal ray the first cell before an obstacle that is the goal, forced,
 * or the origin of an axis ray (along either component) that returns something; no corner test.
 * Not reproduced: the reference's RecursionError on rays that nest deeper than Python's recursion
 * limit (an empty 1100-wide room; such queries complete here), and its walk off a grid without
 * border walls -- cells outside the grid count as obstacles, so results equal the reference's on
 * grids whose border cells are obstacles (what Grid builds).
 * occ_bits, heuristic, start_xy, goal_xy, cost, path (cell ids, goal first), path_len, n_expanded
 * (len(CLOSED)) as pmp_astar2d_batch; W, H <= 8192.
 *   expand         nullable [nq][expand_cap] u32 CLOSED cells in insertion order
 *   expand_parent  nullable [nq][expand_cap] u32 each node's parent cell (the start's is the start);
 *                  needs expand
 *   expand_g       nullable [nq][expand_cap] f64 each node's g; needs expand
 *   push_cap       pushes (= heap entries, each with its g, cell and parent) kept per query;
 *                  0 = min(8 W H + 8, 2^20) (a cell closes once and pushes at most 8)
 *   counters       nullable [nq][4] i64 the reference's pushes, pops, expansions (pops not skipped),
 *                  max heap size
 * status: 0 found; 1 OPEN emptied or an endpoint outside the grid (cost 0, path_len 0: the reference
 * returns []; with an endpoint outside, n_expanded and the counters are 0 too); 2 path_cap overflow; 3 push_cap overflow (that query alone stops, nothing of it is
 * valid but n_expanded and the CLOSED records written so far).
 * Scheduling as the A* engines (pmp_astar2d_set_schedule, pmp_astar2d_set_priority), workers per CU
 * by pmp_set_workers_per_cu (default 8), LDS heap share by pmp_set_resident_per_cu.
 */
int pmp_jps2d_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int W, int H, int heuristic,
                    const int32_t* start_xy, const int32_t* goal_xy, int nq, double* cost,
                    int32_t* path_len, uint32_t* path, int path_cap, int32_t* n_expanded,
                    uint32_t* expand, uint32_t* expand_parent, double* expand_g, int expand_cap,
                    int push_cap, int64_t* counters, int32_t* status);

/* LocalPlanner.params (local_planner/local_planner.py:39-55), same names and units. */
typedef struct {
    double dt;             /* TIME_STEP */
    double lookahead_time; /* LOOKAHEAD_TIME */
    double max_lookahead;  /* MAX_LOOKAHEAD_DIST */
    double min_lookahead;  /* MIN_LOOKAHEAD_DIST */
    double max_v_inc, min_v_inc, max_v, min_v;
    double max_w_inc, min_w_inc, max_w, min_w;
    double goal_dist_tol, rotate_tol;
} pmp_lp_params;

/* DWA constructor parameters (local_planner/dwa.py:45-56). nv, nw > 0 fix the number of (v, w)
 * samples instead of int((v1 - v0) / v_resolution) (used for the 64 x 64 = 4096-sample bench). */
typedef struct {
    double heading_weight, obstacle_weight, velocity_weight;
    double predict_time;   /* horizon H = int(predict_time / dt) */
    double inflation;      /* obstacle_inflation_radius */
    double v_resolution, w_resolution;
    int32_t nv, nw;
} pmp_dwa_params;

/*
 * Batched DWA control steps.  Replaces `iters` iterations of DWA.plan (local_planner/dwa.py:72-93):
 * reachGoal, getLookaheadPoint (local_planner.py:103-170), calDynamicWin (dwa.py:111-135),
 * evaluation (dwa.py:137-190: H-step Robot.lookforward rollout of every (v, w) sample, heading /
 * obstacle (cdist, capped at the inflation radius) / velocity, numpy pairwise-sum normalisation,
 * eval_win @ factor, first-index argmax) and Robot.kinematic (utils/agent/agent.py:68-116).
 * One workgroup per agent, or -- with fewer agents than CUs and a fixed window (nv, nw > 0) -- k
 * workgroups per agent, each on a leaf-aligned part of numpy's pairwise-sum tree over the samples,
 * the last to finish combining the leaf sums in the tree's order and taking the argmax (the same bits
 * as one workgroup; pmp_dwa_set_split).  Agents never interact.
 *   occ_bits [ceil(W*H/32)] u32  obstacle cells, cell (ox + i, oy + j) at bit i*H + j
 *   state    [na][5] f64  in/out  x, y, theta, v, w
 *   goal     [na][3] f64          goal pose
 *   path_xy  [*][2] f64, path_off [na+1] i32   global path of each agent (start -> goal)
 *   u        [na][2] f64          last applied (v, w)
 *   best     [na] i32             argmax sample index of the last step
 *   status   [na] i32             0 stepped (not at goal), 1 goal reached, 4 the reference raises
 *   n_steps  [na] i32             steps taken in this call
 *   hist_pose [na][iters][3] f64  nullable; robot pose before each step (Robot.history_pose)
 *   eval     [na][4096][3] f64    nullable; eval_win @ factor of the last step, row c = sample c
 *                                  (c < N = nv*nw <= 4096; v outer, w inner as itertools.product)
 *   best_traj [na][iters][H][5] f64 nullable; traj_win[argmax] of every step (history_traj)
 */
int pmp_dwa_step_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int ox, int oy, int W, int H,
                       const pmp_lp_params* lp, const pmp_dwa_params* dp, int na, double* state,
                       const double* goal, const double* path_xy, const int32_t* path_off, int iters,
                       double* u, int32_t* best, int32_t* status, int32_t* n_steps, double* hist_pose,
                       double* eval, double* best_traj);

/*
 * Batched D* static plans.  Replaces DStar.plan (global_planner/graph_search/d_star.py:75-291):
 * __init__ (every cell NEW, insert(goal, 0)), processState until start is CLOSED, extractPath.
 * OPEN keeps the reference's list semantics exactly (append-always insert, first-minimal-k
 * min_state, first-occurrence remove).  One wave64 per query; queries never interact.
 *   occ_bits as pmp_astar2d_batch; start_xy, goal_xy [nq][2] i32
 *   cost [nq] f64        extractPath cost (sum of GraphSearcher.cost along the path)
 *   path [nq][path_cap]  cells x*H + y, start -> goal; path_len [nq]
 *   n_process [nq] i64   processState calls (len(DStar.EXPAND))
 *   status [nq]          0 found, 2 path_cap overflow, 3 capacity / max_process exceeded,
 *                        4 the reference raises (OPEN empties: AttributeError at d_star.py:234;
 *                        path_len -2: processState reached a node on the grid's border, whose
 *                        getNeighbor looks up an out-of-grid key -- KeyError, d_star.py:276-291 --
 *                        and path[0] is that node's cell)
 *   max_process          0 = unbounded, else stop with status 3 after that many processState calls
 * Grids built by Grid.init have obstacle borders, so the border KeyError never happens for them.
 */
int pmp_dstar2d_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int W, int H, const int32_t* start_xy,
                      const int32_t* goal_xy, int nq, double* cost, int32_t* path_len, int32_t* path, int path_cap,
                      int64_t* n_process, int32_t* status, int64_t max_process);

/*
 * Batched D* with OnPress replanning.  Replaces DStar.plan followed by npress DStar.OnPress(event)
 * calls (d_star.py:102-134) without the figure: an in-grid press on a free cell adds the obstacle,
 * walks from the start along the parents (the walk's path excludes the goal, as there) and runs
 * modify() (:262-274) -- processState on the kept OPEN / cell states -- where an edge collides.
 *   presses [nq][npress][2]       the pressed cells (x, y)
 *   cost, path_len, n_process, status [nq][npress + 1]; path [nq][npress + 1][path_cap]
 *       round 0 = plan() as pmp_dstar2d_batch; round r: the walk's cost / cells / len(EXPAND);
 *       status 0 walked to the goal, 1 the press changed nothing (off the grid or already an
 *       obstacle: len(EXPAND) is kept), 2 path_cap overflow, 3 a cap or a loop the reference never
 *       leaves (4*W*H+4 steps, or modify() on an empty OPEN), 4 the reference raises (a parentless
 *       node: KeyError, reported with path_len -1; a border node processed: KeyError, path_len -2
 *       and path[r][0] = its cell; OPEN emptied: AttributeError), -1 not run (an earlier call
 *       raised or capped)
 * pmp_dstar2d_batch is this call with npress = 0.
 */
int pmp_dstar2d_onpress_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int W, int H,
                              const int32_t* start_xy, const int32_t* goal_xy, int nq, const int32_t* presses, int npress,
                              double* cost, int32_t* path_len, int32_t* path, int path_cap, int64_t* n_process,
                              int32_t* status, int64_t max_process);

/*
 * Batched 3D D* with dynamic obstacles.  Replaces DStar3D (global_planner/graph_search/d_star3d.py:60-281):
 * plan() (:100-109: processState until OPEN empties or the start is CLOSED, then extractPath
 * :153-166) followed by nrounds apply_dynamic_obstacles(newly_blocked) calls (:115-149: block the
 * voxels, walk from the start along the parents, modify() + processState where an edge collides).
 * OPEN keeps the reference's list semantics (append when absent, first-minimal k), so every round's
 * len(EXPAND), cost and path are bit-exact, including the inf costs of the asymmetric isCollision.
 *   occ_bits, per_query, X, Y, Z, start_xyz, goal_xyz as pmp_graph3d_batch (X, Y, Z <= 256)
 *   blocks [nq][nrounds][nblk][3]  voxels newly blocked per round (outside the grid: ignored); may be
 *                                  NULL when nrounds == 0 or nblk == 0
 *   cost, path_len, n_process, status [nq][nrounds + 1]  per round, 0 = plan(): cost (may be inf),
 *                                  len(EXPAND) of that call, status 0 reached the goal, 1 the walk met
 *                                  a parentless voxel (plan: unreachable; the reference returns the
 *                                  partial path), 2 path_cap overflow, 3 cap (max_process, heap, or the
 *                                  4*X*Y*Z+4 walk bound the reference lacks), 4 endpoints off the grid
 *   path [nq][nrounds + 1][path_cap]  voxel ids (x*Y + y)*Z + z, start -> goal (round 0: extractPath's
 *                                  path; rounds: apply_dynamic_obstacles' path, the goal appended when
 *                                  reached)
 *   expand [nq][expand_cap]        nullable: plan()'s EXPAND as voxel ids, in order (duplicates kept)
 *   max_process                    0 = unbounded, else a processState cap per round
 */
int pmp_dstar3d_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int per_query, int X, int Y, int Z,
                      const int32_t* start_xyz, const int32_t* goal_xyz, int nq, const int32_t* blocks, int nrounds,
                      int nblk, double* cost, int32_t* path_len, int32_t* path, int path_cap, int64_t* n_process,
                      int32_t* status, int32_t* expand, int expand_cap, int64_t max_process);

/*
 * Batched 3D LPA* with apply_change rounds.  Replaces LPAStar3D (global_planner/graph_search/
 * lpa_star3d.py:40-225): plan() (:78-82: computeShortestPath :127-145, extractPath :185-225, the
 * greedy min-g walk from the goal that gives (cost, []) when stuck or after 100000 steps) followed by
 * nr apply_change(coord, blocked) calls (:93-124), each re-planning on the kept g / rhs / U.  U keeps
 * the reference's list semantics, so every call's len(EXPAND), cost and path are bit-exact.
 *   occ_bits, per_query, X, Y, Z, heuristic, start_xyz, goal_xyz as pmp_graph3d_batch
 *   changes [nq][nr][4]      (x, y, z, mode): mode 0 = blocked None (toggle), 1 = True, 2 = False
 *   cost, path_len, n_expanded, status [nq][nr + 1]; path [nq][nr + 1][path_cap] (voxels, start -> goal)
 *       status 0 path, 1 the reference's empty path (cost kept), 2 path_cap overflow, 3 max_expansions
 *       (0 = unbounded) hit, 4 endpoints off the grid, -1 not run (an earlier call hit a cap)
 *   counters [nq][4] nullable: U pushes, expansions (all calls), 0, max |U|
 */
int pmp_lpastar3d_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int per_query, int X, int Y, int Z,
                        int heuristic, const int32_t* start_xyz, const int32_t* goal_xyz, int nq, const int32_t* changes,
                        int nr, double* cost, int32_t* path_len, int32_t* path, int path_cap, int64_t* n_expanded,
                        int32_t* status, int64_t* counters, int64_t max_expansions);

/*
 * Batched LPA*.  Replaces LPAStar.plan (global_planner/graph_search/lpa_star.py:78-87): the initial
 * computeShortestPath (:139-160) with updateVertex (:162-179), and extractPath (:209-230).  U keeps
 * the reference's Python-list semantics (first-minimal `min(U, key)`, shifting `U.remove`,
 * `heapq.heappush` on the list), so the expansion order, len(EXPAND) and costs are bit-exact.
 *   occ_bits, heuristic, start_xy, goal_xy as pmp_astar2d_batch
 *   cost [nq] f64        extractPath cost; also kept when extractPath gives up after 1000 steps
 *   path [nq][path_cap]  cells x*H + y, start -> goal (path_cap >= 1001 covers every result)
 *   n_expanded [nq]      len(EXPAND) of computeShortestPath
 *   counters nullable [nq][4] i64: pushes, expansions, extractPath steps, max |U|
 *   status [nq]          0 found, 1 extractPath gave up (1000 steps: the reference returns
 *                        (cost, [], None)), 2 path_cap overflow, 4 the reference raises (U empties:
 *                        ValueError from min(); a neighbour off the grid: KeyError; start == goal
 *                        ends that way too, the goal node being detached from the map)
 */
int pmp_lpastar2d_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int W, int H, int heuristic,
                        const int32_t* start_xy, const int32_t* goal_xy, int nq, double* cost, int32_t* path_len,
                        uint32_t* path, int path_cap, int32_t* n_expanded, int64_t* counters, int32_t* status);

/*
 * Batched D* Lite.  Replaces DStarLite.plan (global_planner/graph_search/d_star_lite.py:14-187; plan()
 * is LPAStar's): the same list-semantics U, searched from the goal (rhs = 0) toward the start with
 * keys min(g, rhs) + h(node, start) + km (km = 0), outdated keys re-keyed at the pop (:104-106), and
 * extractPath from the start to the goal (:156-187).  Arguments, outputs and statuses as
 * pmp_lpastar2d_batch; start == goal raises in the reference (status 4 after one expansion).
 */
int pmp_dstarlite2d_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int W, int H, int heuristic,
                          const int32_t* start_xy, const int32_t* goal_xy, int nq, double* cost, int32_t* path_len,
                          uint32_t* path, int path_cap, int32_t* n_expanded, int64_t* counters, int32_t* status);

/*
 * Batched LPA* incremental replanning: LPAStar.plan() followed by nt LPAStar.OnPress edits
 * (global_planner/graph_search/lpa_star.py:101-137) without the figure.  Edit p toggles the
 * obstacle at toggles[q][p] (in-grid cells): a freed cell gets updateVertex, then its free
 * neighbours do, and plan() runs again on the kept g / rhs / U (len(EXPAND) restarts per plan).
 * Each worker edits its own copy of the grid; the shared occ_bits are not written.
 *   toggles   [nq][nt][2] i32 (nt >= 1)
 *   cost, n_expanded, status  [nq][nt + 1]: every plan's result, status as pmp_lpastar2d_batch,
 *             -1 = not run (an earlier plan raised, which ends OnPress in the reference)
 *   path_len [nq], path [nq][path_cap]: the last plan's path (start -> goal)
 *   counters  nullable [nq][4] i64, cumulative over the plans (pushes, last plan's expansions and
 *             extractPath steps, max |U|)
 */
int pmp_lpastar2d_replan_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int W, int H, int heuristic,
                               const int32_t* start_xy, const int32_t* goal_xy, int nq, const int32_t* toggles, int nt,
                               double* cost, int32_t* n_expanded, int32_t* status, int32_t* path_len, uint32_t* path,
                               int path_cap, int64_t* counters);

/*
 * Batched D* Lite incremental replanning: DStarLite.plan() followed by nt DStarLite.OnPress calls
 * (global_planner/graph_search/d_star_lite.py:61-97) without the figure: walk from the start along
 * min-g neighbours; after the first step set km = h(step, start), apply the edit as
 * pmp_lpastar2d_replan_batch does, computeShortestPath on the kept state, and walk on to the goal.
 * cost[q][p] is the walk's cost and path the last walk (start -> goal); the walk has no step limit
 * in the reference (it can loop forever), so here it stops with status 3 after 4 W H + 4 steps.
 * Arguments and outputs otherwise as pmp_lpastar2d_replan_batch.
 */
int pmp_dstarlite2d_replan_batch(pmp_ctx* ctx, void* stream, const uint32_t* occ_bits, int W, int H, int heuristic,
                                 const int32_t* start_xy, const int32_t* goal_xy, int nq, const int32_t* toggles,
                                 int nt, double* cost, int32_t* n_expanded, int32_t* status, int32_t* path_len,
                                 uint32_t* path, int path_cap, int64_t* counters);

/* LQR settings (local_planner/lqr.py:35-38): diag Q, diag R, Riccati iteration cap and the
 * signed exit threshold of lqr.py:134.  Reference defaults: q = 1,1,1  r = 1,1  iters 100  eps 0.1. */
typedef struct {
    double q[3], r[2];
    int32_t iters;
    double eps;
} pmp_lqr_params;

/* MPC settings: horizons and weights of mpc.py:37-40 (p = prediction horizon, m = control horizon
 * <= 8, Q = diag q, R = diag r), then the ADMM settings of the QP solve that replaces OSQP
 * (mpc.py:196-203): rho, sigma, relaxation alpha, eps_abs / eps_rel on the inf-norm residuals,
 * max_iter, termination checked every check_every iterations, rho adapted every adaptive_every
 * iterations (0 = never) when the residual-ratio estimate leaves [rho/adaptive_tol, rho*adaptive_tol]. */
typedef struct {
    int32_t p, m;
    double q[3], r[2];
    double rho, sigma, alpha, eps_abs, eps_rel, adaptive_tol;
    int32_t max_iter, check_every, adaptive_every, reserved;
} pmp_mpc_params;

/*
 * Batched LQR.lqrControl (local_planner/lqr.py:103-145), one thread per call:
 *   s, s_d [n][3]   current and desired (x, y, theta)      u_r [n][2]  reference (v, w)
 *   robot_vw [n][2] the robot's current (v, w) for linear/angularRegularization (local_planner.py:172-206)
 *   u [n][2]        regularised control
 */
/* Workgroups per agent of pmp_dwa_step_batch: 0 (default) = auto (the device's CUs over the agents,
 * at most 16, only for fixed windows nv, nw > 0), 1 = one workgroup per agent, k = k parts (reduced
 * to the sample tree's leaf count; a part holds at most 1024 samples).  Results are identical for
 * every setting. */
int pmp_dwa_set_split(pmp_ctx* ctx, int parts);

int pmp_lqr_control_batch(pmp_ctx* ctx, void* stream, const pmp_lp_params* lp, const pmp_lqr_params* lq, int n,
                          const double* s, const double* s_d, const double* u_r, const double* robot_vw, double* u);

/*
 * Batched MPC.mpcControl (local_planner/mpc.py:111-214), four calls per wave64 (one per 16-lane
 * row): QP assembly (S_u'QS_u on the f64 MFMA 16x16x4, one pass per row's agent), ADMM solve on the
 * row (DPP broadcasts and scans), u = du0 + u_p + u_r, regularisation.
 *   u_p [n][2] in/out  carried control error (returned as u - u_r, before regularisation)
 *   qp_H [n][2m][2m], qp_g [n][2m], qp_lu [n][2][4m], du [n][2m]   nullable: the assembled QP and its solution
 *   admm_iters, admm_status [n] i32  nullable: iterations, 0 converged / 1 iteration limit
 */
int pmp_mpc_control_batch(pmp_ctx* ctx, void* stream, const pmp_lp_params* lp, const pmp_mpc_params* mp, int n,
                          const double* s, const double* s_d, const double* u_r, double* u_p, const double* robot_vw,
                          double* u, double* qp_H, double* qp_g, double* qp_lu, double* du, int32_t* admm_iters,
                          int32_t* admm_status);

#define PMP_TRACK_LQR 0
#define PMP_TRACK_MPC 1
/*
 * Batched tracking-controller plan iterations: `iters` iterations of LQR.plan (lqr.py:58-86,
 * kind PMP_TRACK_LQR) or MPC.plan (mpc.py:66-94, kind PMP_TRACK_MPC) per agent, four agents per
 * wave64 (one per 16-lane row): reachGoal, getLookaheadPoint, the rotate/move branch, lqrControl / mpcControl,
 * Robot.kinematic.  Arrays as pmp_dwa_step_batch, plus
 *   u_p [na][2] f64 in/out   MPC's carried u_p (start a plan with zeros); unused for LQR
 *   admm_iters [na] i32      nullable; ADMM iterations summed over this call's steps
 */
int pmp_track_step_batch(pmp_ctx* ctx, void* stream, int kind, const pmp_lp_params* lp, const pmp_lqr_params* lq,
                         const pmp_mpc_params* mp, int na, double* state, double* u_p, const double* goal,
                         const double* path_xy, const int32_t* path_off, int iters, double* u, int32_t* status,
                         int32_t* n_steps, double* hist_pose, int32_t* admm_iters);

#define PMP_FOLLOW_PID 0
#define PMP_FOLLOW_APF 1
#define PMP_FOLLOW_RPP 2
/* Settings of the path-following planners: PID's gains (local_planner/pid.py:35-44), APF's force
 * weights and influence distance (apf.py:37-39), RPP's regulation settings (rpp.py:38-40).  Each
 * kind reads its own group. */
typedef struct {
    double k_v_p, k_v_i, k_v_d, k_w_p, k_w_i, k_w_d, k_theta;
    double zeta, eta, d_0;
    double regulated_radius_min, scaling_dist, scaling_gain;
} pmp_follow_params;

/*
 * Batched path-following plan iterations: `iters` iterations of PID.plan (pid.py:55-99, kind
 * PMP_FOLLOW_PID), APF.plan (apf.py:50-95, PMP_FOLLOW_APF) or RPP.plan (rpp.py:51-99,
 * PMP_FOLLOW_RPP) per agent, four agents per wave64 (one per 16-lane row): reachGoal,
 * getLookaheadPoint, the rotate/move branch, the controller, Robot.kinematic.  The distance to the
 * obstacle cells (APF.getRepulsiveForce, RPP.applyObstacleConstraint: a cdist over every obstacle in
 * the reference) is a scan of the cells within d_0 / scaling_dist of the robot; cells outside the
 * grid's box are free.  APF sums its repulsive terms in the scan's order, not list(set)'s.
 * Arrays as pmp_dwa_step_batch (occ_bits may be NULL for PID; W, H <= 8192), plus
 *   pid_state [na][4] f64 in/out   PID's e_v, i_v, e_w, i_w (start a planner with zeros); unused otherwise
 *   hist_lookahead [na][iters][2] f64  nullable; the lookahead point of each step (RPP's lookahead_pts)
 *   status   0 stepped, 1 goal reached, 4 the reference raises (getLookaheadPoint, or RPP's
 *            1.0 / curvature with a curvature of +-0: that step is not taken or recorded)
 */
int pmp_follow_step_batch(pmp_ctx* ctx, void* stream, int kind, const uint32_t* occ_bits, int ox, int oy, int W, int H,
                          const pmp_lp_params* lp, const pmp_follow_params* fp, int na, double* state,
                          double* pid_state, const double* goal, const double* path_xy, const int32_t* path_off,
                          int iters, double* u, int32_t* status, int32_t* n_steps, double* hist_pose,
                          double* hist_lookahead);

/* RRT / RRT* settings: Map size (utils/environment/env.py:92), inflation delta (sample_search.py:22),
 * max_dist, sample_num, goal_sample_rate (rrt.py:36-44), radius r (rrt_star.py:34-38). */
typedef struct {
    double x_range, y_range, delta;
    double max_dist, radius, goal_sample_rate;
    int32_t sample_num;
    int32_t star;          /* 1 = RRTStar.getNearest (choose parent + rewire), 0 = RRT */
} pmp_rrt_params;

/*
 * Batched RRT / RRT*.  Replaces RRT.plan (global_planner/sample_search/rrt.py:49-151) with
 * SampleSearcher.isCollision (sample_search.py:27-135) and RRTStar.getNearest (rrt_star.py:43-76).
 * One workgroup per query; queries never interact.  All arrays are device pointers.
 *   rect [nr][4] (x, y, w, h), circ [nc][3] (x, y, r), bnd [nb][4]   the Map's obs_rect, obs_circ, boundary
 *   start_xy, goal_xy [nq][2]
 *   rnd [nq][rnd_stride]  each query's np.random double stream, in RandomState.random_sample order
 *                         (generateRandomNode draws one double, then two uniforms if it exceeds
 *                         goal_sample_rate); 3*sample_num+1 doubles always suffice
 *   tree_xy [nq][tree_cap][2], tree_g [nq][tree_cap], tree_parent [nq][tree_cap]   out: sample_list in
 *                         insertion order (the start is node 0 and its own parent; the goal is last when found)
 *   n_nodes [nq]          out: len(sample_list)
 *   cost [nq]             out: goal.g, 0 when not found
 *   path_len [nq], path_xy [nq][path_cap][2]   out: extractPath goal -> start
 *   draws [nq] i64        out: doubles consumed from rnd (advance the caller's RNG by this many)
 *   status [nq]           0 found, 1 not found (returns (0, None, nodes)), 2 path_cap overflow,
 *                         3 tree_cap / stream / candidate-list overflow, 4 parent cycle (reference hangs)
 *   counters [nq][4] i64  nullable: iterations, nodes scanned (nearest + radius passes), in-radius
 *                         candidates, segment collision tests
 * A new RRT* node that lands exactly on an existing one replaces it (dict semantics); plain RRT does
 * not check for that (a measure-zero event).
 */
int pmp_rrt_batch(pmp_ctx* ctx, void* stream, const pmp_rrt_params* p, const double* rect, int nr,
                  const double* circ, int nc, const double* bnd, int nb, const double* start_xy,
                  const double* goal_xy, int nq, const double* rnd, int64_t rnd_stride, int tree_cap,
                  double* tree_xy, double* tree_g, int32_t* tree_parent, int32_t* n_nodes, double* cost,
                  int32_t* path_len, double* path_xy, int path_cap, int64_t* draws, int32_t* status,
                  int64_t* counters);

/*
 * Batched Informed RRT*.  Replaces InformedRRT.plan and generateRandomNode
 * (global_planner/sample_search/informed_rrt.py:74-152) on the RRT* iteration of pmp_rrt_batch: the loop
 * runs all sample_num iterations, the goal stays in the tree as an ordinary node once connected (every
 * later connection overwrites its parent and g), the best connection's cost and path are kept, and once
 * a path exists samples come from Ellipse.transform(c_best / 2) applied to points of the unit disk.
 * One workgroup per query.  All arrays are device pointers; those not listed are pmp_rrt_batch's.
 *   p                     pmp_rrt_params; star is ignored (always RRT*)
 *   ellipse [nq][5]       per query: the ellipse's centre x, y, cos(theta), sin(theta) of
 *                         theta = -np.arctan2(gy - sy, gx - sx), and c = hypot(start, goal) / 2 -- computed
 *                         by the caller with the reference's own numpy expressions (np.arctan2 is not
 *                         libm's atan2 to the last bit, so the kernel takes theta's cos / sin as given)
 *   rnd [nq][rnd_stride]  the np.random double stream: 1 or 3 doubles per iteration until the first
 *                         connection, then 2 per try of the rejection sampler -- unbounded, so a query
 *                         that reaches the end of its stream reports status 3 (re-run with a longer one)
 *   tree_*, n_nodes       out: sample_list in insertion order; the goal sits at goal_slot with its final
 *                         parent and g (not necessarily the best path's)
 *   best_cost [nq]        out: the lowest goal.g at any connection, +inf when never connected
 *   n_finds [nq]          out: completed connections (extractPath calls that returned)
 *   goal_slot [nq]        out: the goal's index in the tree, -1 when never connected
 *   path_len [nq], path_xy [nq][path_cap][2]   out: extractPath goal -> start of the best connection
 *   draws [nq] i64        out: doubles consumed, rejected tries included
 *   status [nq]           0 connected at least once, 1 never (returns (inf, None, nodes)), 2 path_cap
 *                         overflow, 3 tree_cap / stream / candidate-list overflow, 4 a connection closed a
 *                         parent cycle (the reference's extractPath never returns; the tree is left as
 *                         at that moment, best_cost / path hold the best connection before it)
 */
int pmp_informed_rrt_batch(pmp_ctx* ctx, void* stream, const pmp_rrt_params* p, const double* rect, int nr,
                           const double* circ, int nc, const double* bnd, int nb, const double* start_xy,
                           const double* goal_xy, const double* ellipse, int nq, const double* rnd,
                           int64_t rnd_stride, int tree_cap, double* tree_xy, double* tree_g,
                           int32_t* tree_parent, int32_t* n_nodes, double* best_cost, int32_t* n_finds,
                           int32_t* goal_slot, int32_t* path_len, double* path_xy, int path_cap, int64_t* draws,
                           int32_t* status, int64_t* counters);

/*
 * Batched RRT-Connect.  Replaces RRTConnect.plan, extractPath and getExpand
 * (global_planner/sample_search/rrt_connect.py:42-147) with RRT.generateRandomNode / getNearest
 * (rrt.py:92-130) and SampleSearcher.isCollision (sample_search.py:27-135): two trees, one rooted at the
 * start and one at the goal; each iteration extends the forward tree towards a sample, the backward tree
 * towards the new node and then greedily on towards it, and the smaller tree becomes the forward one.
 * One 64-lane wave per query, four queries per workgroup; queries never interact.  All arrays are device
 * pointers; those not listed are pmp_rrt_batch's.
 *   p                     pmp_rrt_params; radius and star are ignored
 *   rnd [nq][rnd_stride]  the np.random double stream: 1 or 3 doubles per iteration, so 3*sample_num
 *                         always suffice (there is no `in sample_list` skip: every iteration draws)
 *   tree_xy [nq][2][tree_cap][2], tree_g [nq][2][tree_cap], tree_parent [nq][2][tree_cap]
 *                         out: both sample lists in dict order.  Tree 0 is rooted at the start, tree 1 at
 *                         the goal; parents are indices into their own tree, a root's parent is 0.  A sample
 *                         at distance 0 from its nearest node (the goal, sampled while tree 1 is forward)
 *                         replaces that node in place, as the dict does: its parent becomes itself
 *   n_nodes [nq][2]       out: len() of each tree
 *   forward [nq]          out: which tree was sample_list_f when the plan ended (getExpand interleaves it first)
 *   boundary [nq][2]      out: the meeting node's index in each tree, -1 when the trees never met
 *   cost [nq]             out: the meeting node's g in tree 0 + its g in tree 1, 0 when not found
 *   path_len [nq], path_xy [nq][path_cap][2]   out: extractPath, start -> meeting node -> goal (the meeting
 *                         node once)
 *   iters [nq]            out: iterations run, the one that returned included
 *   draws [nq] i64        out: doubles consumed from rnd (advance the caller's RNG by this many)
 *   status [nq]           0 found, 1 not found (returns (0, None, None)), 2 path_cap overflow (cost, path_len
 *                         and the trees are complete), 3 tree_cap overflow in either tree (or the stream
 *                         ended), 4 a parent walk did not reach its root (the reference never returns)
 *   counters [nq][4] i64  nullable: iterations, nodes scanned by the nearest passes, isCollision calls,
 *                         greedy steps
 * A steered node that lands exactly on a different existing node is appended, not merged (the reference's
 * dict would replace that entry; the chance is about 2^-50 per insert).
 */
int pmp_rrt_connect_batch(pmp_ctx* ctx, void* stream, const pmp_rrt_params* p, const double* rect, int nr,
                          const double* circ, int nc, const double* bnd, int nb, const double* start_xy,
                          const double* goal_xy, int nq, const double* rnd, int64_t rnd_stride, int tree_cap,
                          double* tree_xy, double* tree_g, int32_t* tree_parent, int32_t* n_nodes, int32_t* forward,
                          int32_t* boundary, double* cost, int32_t* path_len, double* path_xy, int path_cap,
                          int32_t* iters, int64_t* draws, int32_t* status, int64_t* counters);
/* Nodes of each tree pmp_rrt_connect_batch keeps in LDS; larger trees continue in the HBM arrays. */
int pmp_rrt_connect_lds_nodes(void);

/* TrajectoryConstraints (trajectory/trajectory_base.py:30-45) and TimeOptimalTrajectory3D's
 * path_resolution (trajectory/time_optimal_trajectory.py:17-29) */
typedef struct {
    double max_velocity[3];
    double max_acceleration[3];
    double min_time_step;
    double path_resolution;
} pmp_totp_params;

/*
 * Batched time-optimal trajectories (config 5's step after 3D planning, examples/3d_example.py:93-128).
 * Replaces TimeOptimalTrajectory3D(path, constraints, path_resolution).generate()
 * (trajectory/time_optimal_trajectory.py:260-302): arc-length parameterisation with scipy's
 * not-a-knot CubicSpline per axis (:41-74), forward / backward velocity integration (:162-226, the
 * reference's sign handling for q' < 0 included), s_ddot and time profiles (:228-258), sampling at
 * t = 0, dt, ... (+ total_time) through interp1d (:304-335), yaw / yaw rate
 * (trajectory_base.py:245-261).  Values match the reference to rounding.
 *   path_xyz [sum n][3] f64, path_off [nq + 1] i32   waypoints per path (reference order)
 *   max_waypoints  >= every path's n (sizes LDS; <= 602)
 *   s_values, s_dot, s_ddot, time_profile [nq][sample_cap]; n_samples [nq] = max(int(L / res), 100)
 *   points [nq][point_cap][12]: time, position[3], velocity[3], acceleration[3], yaw, yaw rate
 *       (NaN where the reference leaves None); n_points [nq]; total_time [nq]
 *   status [nq]  0 ok, 2 sample_cap or point_cap too small (the counts are still reported),
 *                3 path longer than max_waypoints, 4 the reference raises (< 2 waypoints, or
 *                repeated consecutive waypoints: scipy needs strictly increasing knots)
 *   eval_t [n_eval] nullable: instead of generate()'s sampling, evaluate(t) (:304-335) at these times
 *       (yaw / yaw rate NaN, as evaluate leaves them)
 */
int pmp_totp3d_batch(pmp_ctx* ctx, void* stream, const pmp_totp_params* prm, int nq, const double* path_xyz,
                     const int32_t* path_off, int max_waypoints, int sample_cap, double* s_values, double* s_dot,
                     double* s_ddot, double* time_profile, int32_t* n_samples, int point_cap, double* points,
                     int32_t* n_points, double* total_time, int32_t* status, const double* eval_t, int n_eval);

/* TrajectoryConstraints (trajectory/trajectory_base.py:30-45) as PolynomialTrajectory3D reads them */
typedef struct {
    double max_velocity[3];
    double max_acceleration[3];
    double min_time_step;
} pmp_polytraj_params;

/*
 * Batched quintic trajectories (the `polynomial` choice after 3D planning, examples/3d_example.py:100-133).
 * Replaces PolynomialTrajectory3D(path, constraints, boundary_conditions).generate() / evaluate(t) /
 * resample(dt) (trajectory/polynomial_trajectory.py:52-286, trajectory_base.py:193-216): segment times
 * T_i = max(d_i / (min(vmax) 0.7), 2 sqrt(d_i / min(amax)), 0.5) (:89-111), their left-to-right running
 * sum (segment starts and total_time), centred-difference waypoint velocities clipped to +-vmax
 * (:162-187), zero interior accelerations, quintic coefficients per axis and segment (:142-158,
 * recomputed per point, never stored), sampling at t = 0, dt, ... by repeated addition (+ total_time when
 * the last step is short of it, :238-246), evaluate(t) (:253-286: t clipped to [0, total_time], the first
 * segment with t <= start + duration), yaw / yaw rate (trajectory_base.py:245-261).  Times, counts and
 * segment_times of integer waypoints are bit-equal to the reference's; rows match it to rounding.
 *   paths, one of two forms (the other's pointers NULL):
 *     path_xyz [sum n][3] f64, path_off [nq + 1] i32   waypoints per path (reference order)
 *     cells [nq][path_cap] i32, path_len [nq] i32, X, Y, Z   cell ids (x Y Z + y Z + z) as
 *       pmp_graph3d_batch leaves them on the device, decoded in the order given
 *   bc [nq][4][3] f64 nullable: initial velocity, final velocity, initial acceleration, final
 *       acceleration per path; NULL = zeros
 *   max_waypoints  >= every path's n (sizes LDS; 2 .. pmp_polytraj3d_max_waypoints() = 880)
 *   points [nq][point_cap][15]: time, position[3], velocity[3], acceleration[3], jerk[3], yaw, yaw rate
 *       (NaN where the reference leaves None); n_points [nq]; total_time [nq]
 *   segment_times: path q's n - 1 durations start at path_off[q] (buffer of sum n doubles), in the
 *       cells form at q * path_cap (buffer [nq][path_cap])
 *   status [nq]  0 ok, 2 point_cap too small (the count is still reported; a path of more than 2^24
 *                steps reports count 0), 3 more waypoints than max_waypoints (or path_cap), 4 the
 *                reference raises (< 2 waypoints) or never ends (total_time not finite)
 *   eval_t [n_eval] nullable: instead of generate()'s sampling, evaluate(t) at these times (yaw / yaw
 *       rate NaN, as evaluate leaves them)
 *   sample_dt  > 0: resample(sample_dt): the same repeated sum with this step, yaw / yaw rate NaN;
 *       0: generate() with min_time_step
 * Refused with PMP_EINVAL (the reference divides by zero or never leaves its sampling loop):
 * min(max_acceleration) <= 0, non-finite constraints, min_time_step <= 0.  Repeated consecutive
 * waypoints are legal (T = 0.5).
 */
int pmp_polytraj3d_batch(pmp_ctx* ctx, void* stream, const pmp_polytraj_params* prm, int nq, const double* path_xyz,
                         const int32_t* path_off, const int32_t* cells, const int32_t* path_len, int path_cap, int X,
                         int Y, int Z, const double* bc, int max_waypoints, int point_cap, double* points,
                         int32_t* n_points, double* total_time, double* segment_times, int32_t* status,
                         const double* eval_t, int n_eval, double sample_dt);
/* The largest max_waypoints pmp_polytraj3d_batch accepts (its LDS block beside the row stage). */
int pmp_polytraj3d_max_waypoints(void);

/* TrajectoryConstraints (trajectory/trajectory_base.py:30-45) as SplineTrajectory3D reads them, and its
 * spline_degree (trajectory/spline_trajectory.py:16-32; the kernel clamps it to n - 1 per path) */
typedef struct {
    double max_velocity[3];
    double max_acceleration[3];
    double min_time_step;
    int32_t spline_degree;
    int32_t reserved;
} pmp_splinetraj_params;

/*
 * Batched B-spline trajectories (the `spline` choice after 3D planning, examples/3d_example.py:100-133).
 * Replaces SplineTrajectory3D(path, constraints, spline_degree, smoothing_factor=0).generate() /
 * evaluate(t) / resample(dt) / reparameterize_constant_speed() (trajectory/spline_trajectory.py:16-392,
 * trajectory_base.py:193-216): the centripetal parameter u (:60-77), k = min(spline_degree, n - 1), the
 * interpolating spline UnivariateSpline(u, coords, k, s=0) returns (:79-120) -- FITPACK's knots for s = 0
 * are k + 1 copies of u[0], u[(k+1)/2 : n-(k+1)/2] (odd k) or the midpoints (u[j] + u[j+1]) / 2,
 * j = k/2 .. n-k/2-2 (even k), k + 1 copies of u[n-1]; the coefficients solve the banded collocation
 * system, eliminated without pivoting -- its first and second derivative splines, the 500-sample time
 * parameterisation (:154-203), sampling at t = 0, dt, ... by repeated addition through interp1d with the
 * final point at rest (:216-263), _enforce_constraints' time scaling (:304-323), yaw / yaw rate on the
 * scaled rows (trajectory_base.py:245-261).  Counts follow the reference's; values match it to rounding.
 *   paths, one of two forms (the other's pointers NULL):
 *     path_xyz [sum n][3] f64, path_off [nq + 1] i32   waypoints per path (reference order)
 *     cells [nq][path_cap] i32, path_len [nq] i32, X, Y, Z   cell ids (x Y Z + y Z + z) as
 *       pmp_graph3d_batch leaves them on the device, decoded in the order given
 *   max_waypoints  >= every path's n (sizes LDS; 3 .. pmp_splinetraj3d_max_waypoints() = 500)
 *   points [nq][point_cap][12]: time, position[3], velocity[3], acceleration[3], yaw, yaw rate
 *       (NaN where the reference leaves None); n_points [nq]; total_time [nq] (after the scaling)
 *   status [nq]  0 ok, 2 point_cap too small (the count is still reported; a path of more than 2^24
 *                steps reports count 0), 3 more waypoints than max_waypoints (or path_cap), 4 the
 *                reference raises (< 3 waypoints or an effective degree of 1: derivative(2) of a linear
 *                spline; repeated consecutive waypoints: x must be strictly increasing if s = 0) or
 *                never ends (total_time not finite)
 *   eval_t [n_eval] nullable: instead of generate()'s rows, evaluate(t) (:273-302) at these times on the
 *       scaled total_time (u = t / total_time; yaw / yaw rate NaN, as evaluate leaves them)
 *   sample_dt  > 0: resample(sample_dt): evaluate at the repeated sum with this step; 0: generate()
 *   constant_speed != 0: the rows reparameterize_constant_speed() (:325-392) leaves after generate(): the
 *       1000-sample arc-length table, speed min(path_length / total_time, min(max_velocity)), the new
 *       total_time, zero accelerations, no yaw
 *   eval_t, sample_dt and constant_speed exclude each other.
 * Refused with PMP_EINVAL (scipy raises, or the reference divides by zero or never leaves its loop):
 * spline_degree outside 1..5, non-finite constraints, min|max_velocity| <= 0, min(max_acceleration) <= 0,
 * min_time_step <= 0.  smoothing_factor > 0 (FITPACK's knot search) is not offered.
 */
int pmp_splinetraj3d_batch(pmp_ctx* ctx, void* stream, const pmp_splinetraj_params* prm, int nq,
                           const double* path_xyz, const int32_t* path_off, const int32_t* cells,
                           const int32_t* path_len, int path_cap, int X, int Y, int Z, int max_waypoints,
                           int point_cap, double* points, int32_t* n_points, double* total_time, int32_t* status,
                           const double* eval_t, int n_eval, double sample_dt, int constant_speed);
/* The largest max_waypoints pmp_splinetraj3d_batch accepts (its LDS block within 64 KiB). */
int pmp_splinetraj3d_max_waypoints(void);

/* Dubins(step, max_curv) (curve_generation/dubins_curve.py:31-33) */
typedef struct {
    double step;
    double max_curv;
} pmp_dubins_params;

/*
 * Batched Dubins curves (curve_generation/dubins_curve.py, the `dubins` name of CurveFactory; the steering
 * function of the nonholonomic sampling planners).  Replaces Dubins(step, max_curv).generation(start, goal)
 * (:238-313) for n pose pairs: the frame theta / dist / alpha / beta (:253-261, mod2pi as curve.py:51-55,
 * CPython's hypot), the six words LSL, RSR, LSR, RSL, RLR, LRL in the reference's expressions and order
 * (:38-205; a word is infeasible when p^2 < 0, for RLR / LRL when |p| > 1), cost |t| + |p| + |q| in
 * curvature-normalised units (not divided by max_curv, as best_cost is returned), the first strictly
 * cheapest word (:267-273), the interpolation loop (:283-294: per piece the repeated sum length += step,
 * not k step; then the piece's exact end), the strip of trailing points whose local x is exactly 0.0
 * (:301-304: real points too, so equal poses return cost 0 and no point), rotation by theta, translation,
 * pi2pi on the yaw (:306-311).  Words and counts follow the reference's except where two words tie to
 * the last bit; values match it to rounding.
 *   start_xyyaw, goal_xyyaw [n][3] f64: x, y, yaw in radians
 *   word [n] u8      0..5 = LSL, RSR, LSR, RSL, RLR, LRL; 255 = none
 *   tpq [n][3]       the word's piece lengths (NaN with word 255); cost [n] (inf with word 255)
 *   n_points [n]     the reference's len(x_list)
 *   points [n][point_cap][3] nullable: x, y, yaw of the first min(n_points, point_cap) points; NULL =
 *       costs and counts only (point_cap then only sizes the table of step sums)
 *   status [n]  0 ok, 2 point_cap too small (the count is still reported and the first point_cap rows
 *               are valid; a pair of more than 2^24 steps reports count 0), 4 the reference raises (a
 *               non-finite pose: no word is chosen and int(nan) raises ValueError) or never ends (a
 *               coordinate or yaw from about 1e17 on, where mod2pi leaves no angle for pi2pi's loop)
 * Refused with PMP_EINVAL (the reference never leaves its loop, or divides by zero): step <= 0 or
 * non-finite, max_curv <= 0 or non-finite.
 */
int pmp_dubins_batch(pmp_ctx* ctx, void* stream, const pmp_dubins_params* prm, int n, const double* start_xyyaw,
                     const double* goal_xyyaw, uint8_t* word, double* tpq, double* cost, int32_t* n_points,
                     int point_cap, double* points, int32_t* status);
/*
 * The Dubins steering metric between every start and every goal: cost [A][B] and word [A][B] of
 * generation(starts[a], goals[b]) (:253-273) as pmp_dubins_batch computes them, without sampling.  The pair
 * index is decoded in the kernel; the A B pose pairs are never stored.  cost inf / word 255 where the
 * reference raises.  Refused with PMP_EINVAL as pmp_dubins_batch (step is checked although unused).
 */
int pmp_dubins_cost_matrix(pmp_ctx* ctx, void* stream, const pmp_dubins_params* prm, int A, const double* start_xyyaw,
                           int B, const double* goal_xyyaw, double* cost, uint8_t* word);

/* ReedsShepp(step, max_curv) (curve_generation/reeds_shepp.py:30-32) */
typedef struct {
    double step;
    double max_curv;
} pmp_reeds_shepp_params;

/*
 * Batched Reeds-Shepp curves (curve_generation/reeds_shepp.py: the car that can reverse; the steering
 * function of the nonholonomic sampling planners for parking-style manoeuvres).  Replaces
 * ReedsShepp(step, max_curv).generation(start, goal) (:606-674) for n pose pairs: the frame x, y, phi
 * (:621-627; phi = gyaw - syaw unwrapped), the 46 candidates of SCS, CCC, CSC, CCCC, CCSC, CCSCC (:235-573)
 * in the reference's order, called slots 0..45 (0-1 SCS, 2-9 CCC, 10-17 CSC, 18-25 CCCC, 26-41 CCSC, 42-45
 * CCSCC), each from the reference's primitive with its feasibility tests, its lengths as Path(lengths=...)
 * writes them, path_length = sum(|l|) as Python's sum adds it, the first strictly shortest slot (:633-637),
 * the interpolation loop (:646-657: per piece the repeated sum length += d_length with d_length of the
 * length's sign, not k step; then the piece's exact end) from the local pose (0, 0, 0), the strip of trailing
 * points whose local x is exactly 0.0 (:664-667: real points too, so equal poses return cost 0 and no
 * point), the transformation back and pi2pi on the yaw (:670-672).  Slots and counts follow the
 * reference's except where two slots tie to rounding (the mirrored CCC words have the same length
 * mathematically, so ties are common); values match it to rounding.
 *   start_xyyaw, goal_xyyaw [n][3] f64: x, y, yaw in radians
 *   slot [n] u8      0..45; 255 = none
 *   lengths [n][5]   the slot's signed piece lengths, curvature-normalised; NaN beyond the word's 3-5 pieces
 *                    (all NaN with slot 255)
 *   cost [n]         best_cost / max_curv, as generation() returns it (:674): in the units of x and y, where
 *                    pmp_dubins_batch's cost is curvature-normalised as Dubins.generation() returns it; inf
 *                    with slot 255
 *   slot_costs [n][46] nullable: every candidate's path_length (curvature-normalised), NaN = infeasible: the
 *                    k best manoeuvres without a second launch; NULL = not written
 *   n_points [n]     the reference's len(x_list)
 *   points [n][point_cap][3] nullable: x, y, yaw of the first min(n_points, point_cap) points; NULL =
 *       costs and counts only (point_cap then only sizes the table of step sums)
 *   status [n]  0 ok, 2 point_cap too small (the count is still reported and the first point_cap rows
 *               are valid; a pair of more than 2^24 steps reports count 0), 4 the reference raises (a
 *               non-finite pose leaves no candidate below inf and int(inf / step) is an OverflowError, or
 *               the points overrun its int(cost / step) + pieces + 3 list slots: IndexError) or, a
 *               documented limit, |syaw| > 64 or |gyaw - syaw| > 64 radians: the reference's M() spends
 *               |phi| / 2 pi loop rounds there and never ends from about 1e16 on
 * Refused with PMP_EINVAL (the reference never leaves its loop, or divides by zero): step <= 0 or
 * non-finite, max_curv <= 0 or non-finite; null pointers; n < 0; point_cap < 1.
 */
int pmp_reeds_shepp_batch(pmp_ctx* ctx, void* stream, const pmp_reeds_shepp_params* prm, int n,
                          const double* start_xyyaw, const double* goal_xyyaw, uint8_t* slot, double* lengths,
                          double* cost, double* slot_costs, int32_t* n_points, int point_cap, double* points,
                          int32_t* status);
/*
 * The Reeds-Shepp steering metric between every start and every goal: cost [A][B] (best_cost / max_curv)
 * and slot [A][B] of generation(starts[a], goals[b]) (:621-637) as pmp_reeds_shepp_batch computes them,
 * without sampling.  The pair index is decoded in the kernel; the A B pose pairs are never stored.  cost
 * inf / slot 255 where the reference raises or the 64-radian limit refuses.  Refused with PMP_EINVAL as
 * pmp_reeds_shepp_batch (step is checked although unused); A < 0 or B < 0.
 */
int pmp_reeds_shepp_cost_matrix(pmp_ctx* ctx, void* stream, const pmp_reeds_shepp_params* prm, int A,
                                const double* start_xyyaw, int B, const double* goal_xyyaw, double* cost,
                                uint8_t* slot);

/* Polynomial(step, max_acc, max_jerk) and its instance attributes dt, t_min, t_max
 * (curve_generation/polynomial_curve.py:28-34; the reference's defaults are 0.1, 1, 30) */
typedef struct {
    double step;
    double max_acc;
    double max_jerk;
    double dt;
    double t_min;
    double t_max;
} pmp_polycurve_params;

/*
 * Batched quintic polynomial curves (curve_generation/polynomial_curve.py): the minimum-time connection of
 * two states (x, y, yaw, v, a) under peak-acceleration and peak-jerk limits, the steering function and time
 * metric of a kinodynamic sampling planner.  Replaces Polynomial(step, max_acc, max_jerk).generation(start,
 * goal) (:104-164) for n state pairs: the velocities and accelerations split by cos / sin of the yaws
 * (:118-126), the candidate times T_i = np.arange(t_min, t_max, step)[i] = t_min + i ((t_min + step) - t_min),
 * ceil((t_max - t_min) / step) of them (:130), per candidate and axis the 3 x 3 solve of Poly.__init__
 * (:43-61; Gaussian elimination with partial pivoting, where the reference calls LAPACK), the sample times
 * k dt, k < ceil((T + dt) / dt) (:134), and the first candidate with max hypot(ax, ay) <= max_acc and
 * max hypot(jx, jy) <= max_jerk (:158-160; a NaN peak is infeasible).  The rows of that candidate are the
 * reference's (:135-156): yaw = atan2(vy, vx), v = hypot(vx, vy), a = hypot(ax, ay) negated where
 * v[k] - v[k-1] < 0, jerk = hypot(jx, jy) negated where the signed a[k] - a[k-1] < 0 (row 0 has neither rule).
 * t_index and the counts follow the reference's unless a peak lies within rounding of its limit; values
 * match it to rounding (the signs of a and jerk where the difference they turn on is not itself rounding).
 *   start, goal [n][5] f64: x, y, yaw in radians, v, a
 *   t_index [n] i32  the chosen candidate's index i; -1 = no candidate is feasible
 *   T [n]            its time T_i; inf with t_index -1
 *   n_points [n]     the reference's traj.size: ceil((T + dt) / dt); 0 with t_index -1
 *   points [n][point_cap][7] nullable: time, x, y, yaw, v, a, jerk of the first min(n_points, point_cap) rows;
 *       NULL = t_index, T and counts only (point_cap is then unused but must be >= 1)
 *   status [n]  0 ok, 1 no feasible T (the reference returns an empty trajectory: also for a NaN or infinite
 *               pose and for a goal too far to reach within t_max), 2 point_cap too small (the count is still
 *               reported and the first point_cap rows are valid)
 * Refused with PMP_EINVAL (the reference never ends, raises, or answers with garbage): step <= 0 or
 * non-finite; dt <= 0 or non-finite; t_min <= 0 (the system is singular at T = 0) or non-finite; t_max
 * non-finite; max_acc or max_jerk non-finite; more than 2^24 candidate times or sample times; null pointers;
 * n < 0; point_cap < 1.  t_max <= t_min is no error: there is no candidate, status 1.
 */
int pmp_polycurve_batch(pmp_ctx* ctx, void* stream, const pmp_polycurve_params* prm, int n, const double* start,
                        const double* goal, int32_t* t_index, double* T, int32_t* n_points, int point_cap,
                        double* points, int32_t* status);
/*
 * The minimum-time metric between every start and every goal state: T [A][B] (inf where no candidate is
 * feasible) and t_index [A][B] (-1 there) of generation(starts[a], goals[b]) as pmp_polycurve_batch finds
 * them, without sampling.  The pair index is decoded in the kernel; the A B state pairs are never stored.
 * start [A][5], goal [B][5].  Refused with PMP_EINVAL as pmp_polycurve_batch; A < 0 or B < 0.
 */
int pmp_polycurve_time_matrix(pmp_ctx* ctx, void* stream, const pmp_polycurve_params* prm, int A, const double* start,
                              int B, const double* goal, double* T, int32_t* t_index);

/* Bezier(step, offset) (curve_generation/bezier_curve.py:27-29) */
typedef struct {
    double step;
    double offset;
} pmp_bezier_params;

/*
 * Batched cubic Bezier curves (curve_generation/bezier_curve.py).  Replaces Bezier(step, offset).generation(
 * start, goal) (:34-53) for n pose pairs: n_points = int(hypot(sx - gx, sy - gy) / step) (:49), the control
 * points P0 = start, P1 = start + d (cos syaw, sin syaw), P2 = goal - d (cos gyaw, sin gyaw), P3 = goal with
 * d = hypot / offset (:82-89), and the point at each t of np.linspace(0, 1, n_points) (t_i = i (1 / (n - 1)),
 * the last exactly 1; a single point has t = 0) as the left-to-right sum over i = 0..3 of
 * ((C(3, i) t^i) (1 - t)^(3 - i)) P_i (:66-69).  Counts follow the reference's unless hypot / step lies within
 * rounding of an integer; values match it to rounding.
 *   start_xyyaw, goal_xyyaw [n][3] f64: x, y, yaw in radians
 *   control [n][4][2]  the control points
 *   n_points [n]       the reference's len(path); poses closer than step have no point
 *   points [n][point_cap][2] nullable: x, y of the first min(n_points, point_cap) points; NULL = counts and
 *       control points only
 *   status [n]  0 ok, 2 point_cap too small (the count is still reported and the first point_cap rows are
 *               valid; a pair of more than 2^24 points reports count 0), 4 the reference raises (a non-finite
 *               pose: int(nan) is a ValueError, int(inf) an OverflowError)
 * Refused with PMP_EINVAL (the reference divides by zero or answers with NaN): step <= 0 or non-finite,
 * offset == 0 or non-finite; null pointers; n < 0; point_cap < 1.
 */
int pmp_bezier_batch(pmp_ctx* ctx, void* stream, const pmp_bezier_params* prm, int n, const double* start_xyyaw,
                     const double* goal_xyyaw, double* control, int32_t* n_points, int point_cap, double* points,
                     int32_t* status);

/* BSpline / BSpline3D(step, k, param_mode, spline_mode) (curve_generation/bspline_curve.py:26-37,
 * bspline_curve3d.py:29-40) */
enum { PMP_BSPLINE_CENTRIPETAL = 0, PMP_BSPLINE_CHORD_LENGTH = 1, PMP_BSPLINE_UNIFORM = 2 };
enum { PMP_BSPLINE_INTERPOLATION = 0, PMP_BSPLINE_APPROXIMATION = 1 };
enum { PMP_BSPLINE_2D = 0, PMP_BSPLINE_3D = 1 };
typedef struct {
    double step;
    int32_t k;           /* degree, 1..5 */
    int32_t param_mode;  /* PMP_BSPLINE_CENTRIPETAL .. */
    int32_t spline_mode; /* PMP_BSPLINE_INTERPOLATION / _APPROXIMATION */
    int32_t variant;     /* PMP_BSPLINE_2D: BSpline's rules, PMP_BSPLINE_3D: BSpline3D's */
} pmp_bspline_params;

/*
 * Batched B-spline curves through (or near) waypoint lists.  Replaces BSpline(...).run(points) and
 * BSpline3D(...).run(points) for n_curves lists in one launch, one wave per curve: paramSelection,
 * knotGeneration, interpolation or approximation (then parameters and knots again from the control polygon, as
 * run() does), generation at np.linspace(0, 1, n_samples) with the last row's N[-1][-1] = 1, and the rows'
 * polyline length (hypot of x and y; the 3D variant on 3D points: the Euclidean norm).
 * The two variants differ in: the segment length (2D: math.hypot of x and y; 3D: the Euclidean norm over dim
 * coordinates), the guard `s[-1] > 0` (3D only: coinciding points give parameters 0 and a singular system; 2D
 * divides 0 / 0 and every control point and row is NaN, status 0), n_samples (2D: int(1 / step), 3D: at least 2)
 * and the length.  The basis values are the reference's bits (its expressions in its order over the k + 1
 * functions that can be non-zero); the linear systems are solved by banded elimination without pivoting,
 * the reference inverts with LAPACK: control points and rows agree to rounding times the system's condition.
 *   pts [sum n][dim] f64 packed waypoints, off [n_curves + 1] i32 their offsets; dim 2 or 3
 *   min_waypoints / max_waypoints: the shortest and longest curve of the launch, by the caller's own
 *       count (the offsets are on the device); max_waypoints sizes the LDS and the outputs' rows.  A curve found
 *       outside them is not run: status 4, n_control 0
 *   params_in [n_curves][max_waypoints], knot_in [n_curves][max_waypoints + k + 1] nullable: use these
 *       parameters / knots for the solve instead of computing them (interpolation(points, param, knot))
 *   params [n_curves][max_waypoints], knot [n_curves][max_waypoints + k + 1], control [n_curves][max_waypoints][dim],
 *   n_control [n_curves]: what generation() was given (approximation: n - 1 control points and the second
 *       parameters and knots); entries past a curve's own count are 0
 *   n_samples: int(1 / step) (3D: max(2, .)), computed by the caller too, since it sizes points
 *   points [n_curves][n_samples][dim] nullable: NULL = control points, length and status only
 *   length [n_curves], status [n_curves]: 0 ok, 4 the reference raises numpy.linalg.LinAlgError (a pivot that
 *       is exactly zero: a repeated consecutive waypoint, n <= k, coinciding points in 3D); control, rows
 *       and length are then NaN
 * Refused with PMP_EINVAL: k outside 1..5; step <= 0 or non-finite; more than 2^24 samples; no sample (2D,
 * step > 1: the reference raises IndexError); n_samples not int(1 / step); dim not 2 or 3; fewer than 2 or more
 * than 64 waypoints; approximation with fewer than k + 2 (the reference's precondition N > H > k); unknown
 * modes; null pointers; n_curves < 0.
 */
int pmp_bspline_batch(pmp_ctx* ctx, void* stream, const pmp_bspline_params* prm, int n_curves, const double* pts,
                      const int32_t* off, int dim, int min_waypoints, int max_waypoints, const double* params_in,
                      const double* knot_in, double* params, double* knot, double* control, int32_t* n_control,
                      int n_samples, double* points, double* length, int32_t* status);

/* CubicSpline(step) (curve_generation/cubic_spline.py:26-27) */
typedef struct {
    double step;
    int32_t with_derivative; /* rows of 5 (x, y, yaw, dx, dy) instead of 3 */
    int32_t pad_;
} pmp_cubic_spline_params;

/*
 * Batched natural cubic splines over arc length.  Replaces CubicSpline(step).run(points) (:84-111) for n_lists
 * waypoint lists, one wave per list: s = [0] + cumsum(hypot) bit for bit (CPython's hypot, left to right),
 * n_points = len(np.arange(0, s[-1], step)) = ceil(s[-1] / step), the spline coefficients of x(s) and y(s)
 * (:46-67; the tridiagonal system by the Thomas algorithm, the reference by a dense LAPACK solve: rounding
 * apart), and one row per t_i = i step: the interval bisect(s, t) - 1, x, y, yaw = atan2(dy, dx).
 *   pts [sum n][dim] f64 packed waypoints (x, y first), off [n_lists + 1] i32; dim 2 or 3
 *   arc_length [n_lists]  s[-1]
 *   n_points [n_lists], points [n_lists][point_cap][3 or 5] nullable (NULL = counts and arc length only)
 *   status [n_lists]  0 ok (a repeated consecutive waypoint divides by zero: the full count of NaN rows, as the
 *       reference), 2 point_cap too small (the count is reported, the first point_cap rows are valid), 4 the
 *       reference raises (np.arange of a non-finite s[-1]) or the list has more than 2^24 points
 * Refused with PMP_EINVAL: step <= 0 or non-finite; dim not 2 or 3; fewer than 2 or more than 512 waypoints;
 * null pointers; n_lists < 0; point_cap < 1.
 */
int pmp_cubic_spline_batch(pmp_ctx* ctx, void* stream, const pmp_cubic_spline_params* prm, int n_lists, const double* pts,
                           const int32_t* off, int dim, int min_waypoints, int max_waypoints, double* arc_length,
                           int32_t* n_points, int point_cap, double* points, int32_t* status);

/* PSO(start, goal, env, n_particles, point_num, w_inertial, w_cognitive, w_social, max_speed, max_iter)
 * (global_planner/evolutionary_search/pso.py:44-61) and the grid's ranges */
typedef struct {
    int32_t x_range, y_range;
    int32_t n_particles;
    int32_t point_num; /* 1..62: with start and goal at most 64 waypoints */
    int32_t max_iter;
    int32_t waves;     /* wave64s per workgroup, 1..16; 0 = pmp_pso_default_waves(), or fewer: no more than there are
                          particles or than the LDS holds beside the swarm.  Results do not depend on it */
    double w_inertial, w_cognitive, w_social;
    double max_speed;
} pmp_pso_params;

/*
 * Batched particle-swarm plans on one grid.  Replaces PSO.plan() (pso.py:77-123) after initializePositions()
 * for n_plans independent plans in one launch, one workgroup per plan: the initial fitness of every particle,
 * max_iter iterations of optimizeParticle over the particles in index order (a particle that beats the global
 * best replaces it at once, for the particles after it too), and the best particle's curve.  The curve is
 * BSpline(step=0.01, k=4)'s (centripetal interpolation, 100 rows) through [start] + position + [goal] with
 * repeated points dropped; the fitness is 100000 / (length + 50000 obs_cost), obs_cost the number of the 99
 * consecutive pairs of round()ed rows for which PSO.isCollision holds, and inf where the curve raises (fewer
 * than 5 points left, or a singular collocation matrix).  best_pos is position in the reference (the same
 * list), so the cognitive term is w_cognitive * rand1 * 0.  Positions, velocities and every decision are the
 * reference's exactly as long as no two compared fitness values lie within the curve's rounding of each other
 * and no row coordinate within it of a half-integer; fitness values, rows and length agree to that rounding.
 * An iteration evaluates the particles not yet committed in parallel against the global best as it stands and
 * repeats those after the first one that replaces it; the result is the sequential one for any `waves`.
 *   occ_bits: the grid's bit-packed x-major occupancy (cell x * y_range + y), as for pmp_astar2d_batch
 *   start, goal [n_plans][2] i32; init_positions [n_plans][n_particles][point_num][2] i32 (initializePositions())
 *   init_bounds: HOST int32[4] = min x, min y, max x, max y over init_positions, by the caller's own count (the
 *       positions are on the device).  A plan found with a position outside the grid is not run: status 4,
 *       best_fitness and length NaN, nothing else written
 *   rnd [n_plans][rnd_stride] f64: each plan's random.random() stream; particle p's point i at iteration t
 *       reads rand1, rand2 at 2 ((t n_particles + p) point_num + i); 2 point_num n_particles max_iter draws
 *   status [n_plans]: 0, or 4 where the best fitness is inf (plan() raises the curve's LinAlgError at its last line)
 *   best_position [n_plans][point_num][2] i32, best_fitness [n_plans], fitness_history [n_plans][max_iter]
 *   positions [n_plans][n_particles][point_num][2] i32, velocities (same shape) f64, fitness and
 *   particle_best_fitness [n_plans][n_particles]: the final swarm
 *   points [n_plans][100][2], length [n_plans]: the best particle's curve (NaN with status 4)
 *   repeats [n_plans] i64: evaluations thrown away because an earlier particle replaced the global best
 *   trace_positions [n_plans][max_iter][n_particles][point_num][2] i32 and trace_fitness
 *       [n_plans][max_iter][n_particles], both nullable (together): the swarm after every iteration
 * Refused with PMP_EINVAL: x_range or y_range < 1; n_particles < 1; point_num outside 1..62; max_iter < 0; a
 * non-finite weight; max_speed < 0 or NaN; waves outside 0..16; init_bounds outside the grid; rnd_stride below
 * the draw count; a swarm whose LDS (two copies of its state beside `waves` B-spline states) exceeds 160 KiB;
 * null pointers; n_plans < 0.
 */
int pmp_pso_batch(pmp_ctx* ctx, void* stream, const pmp_pso_params* prm, const uint32_t* occ_bits, int n_plans,
                  const int32_t* start, const int32_t* goal, const int32_t* init_positions, const int32_t* init_bounds,
                  const double* rnd, int64_t rnd_stride, int32_t* status, int32_t* best_position, double* best_fitness,
                  double* fitness_history, int32_t* positions, double* velocities, double* fitness,
                  double* particle_best_fitness, double* points, double* length, int64_t* repeats,
                  int32_t* trace_positions, double* trace_fitness);
/* The most waves per workgroup pmp_pso_batch launches where pmp_pso_params.waves is 0.  No device call. */
int pmp_pso_default_waves(void);

/* ACO(start, goal, env, n_ants, alpha, beta, rho, Q, max_iter) (global_planner/evolutionary_search/aco.py:40-49)
 * and the grid's ranges.  beta is in the caller's heuristic table, rho is passed as the host's own 1 - rho */
typedef struct {
    int32_t x_range, y_range;
    int32_t n_ants;
    int32_t max_iter;
    int32_t waves;    /* wave64s (plans) per workgroup, 1..8; 0 = pmp_aco_default_waves().  Results do not depend on it */
    int32_t reserved;
    double alpha;     /* 1.0 (pheromone ** 1.0 is the pheromone) or 0.0 (it is 1.0) */
    double one_minus_rho;
    double Q;
} pmp_aco_params;

/*
 * Batched ant-colony plans on one grid.  Replaces ACO.plan() (aco.py:65-166) for n_plans independent plans in
 * one launch, one wave64 per plan: max_iter iterations of n_ants ants, each walking from the start over open,
 * unvisited neighbours by roulette (one random.random() per step, drawn by MT19937 in the kernel from the
 * plan's state) until it stands next to the goal, has no candidate with a non-zero weight, or has made
 * ceil(x_range y_range / 2 + max(x_range, y_range)) choices; then the evaporation, the successful ants'
 * deposits in ant order and the reference's bookkeeping of the best path.  Every operation on doubles is the
 * reference's, in its order, so the walk, the pheromone and the generator's state are the reference's bit for
 * bit.  An edge is (cell, motion index m), env.motions order (-1,0) (-1,1) (0,1) (1,1) (1,0) (1,-1) (0,-1) (-1,-1).
 *   occ_bits: the grid's bit-packed x-major occupancy (cell x * y_range + y), as for pmp_astar2d_batch
 *   starts, goals [n_plans][2] i32
 *   heur [n_tables][x_range y_range] f64: (1.0 / h(cell, goal)) ** beta by the host's own pow, any finite value
 *       for the goal and the obstacles (never read into a sum); heur_of [n_plans] i32: each plan's table
 *   mt_state_in [n_plans][625] u32: random.getstate()[1], the 624 words and the index
 *   status [n_plans]: 0 a path, 1 no ant ever found the goal, 5 the roulette's draw exceeded its last cumulative
 *       quotient (the reference raises IndexError): the plan stops there, the generator just after that draw
 *   best_len [n_plans], best_path [n_plans][cap] i32 cell ids, start first, cap = pmp_aco_path_cap()
 *       (entries from best_len on are not written: what an earlier, longer best path left, or the caller's fill)
 *   n_cost [n_plans], cost_list [n_plans][max_iter] i32: an entry per iteration from the first successful one
 *   draws [n_plans] i64; mt_state_out [n_plans][625]
 *   ant_found, ant_len [n_plans][max_iter][n_ants] i32, nullable together: every ant's found_goal and len(path)
 *   pheromone [n_plans][x_range y_range][8] f64: the plan's pheromone, final on return (1.0 evaporated and
 *       deposited on for an open edge, 0.0 for the others)
 *   paths [n_plans][n_ants][cap] u16 and ant_scratch [n_plans][n_ants] i32: scratch
 * The entry checks the device-resident inputs with a small kernel and waits for its verdict: one
 * synchronisation of the stream per call, so it cannot be captured into a graph.
 * Refused with PMP_EINVAL: alpha other than 0.0 or 1.0; n_ants < 1; max_iter < 0; a non-finite one_minus_rho, Q
 * or heur entry of a free cell; a start or goal outside the grid or in an obstacle; heur_of outside the tables;
 * more than 65,536 cells; waves outside 0..8; an MT index above 624; a free cell on the grid's border (the
 * reference's ant steps outside the grid there and dies with KeyError one step later); null pointers;
 * n_plans < 0.
 */
int pmp_aco_batch(pmp_ctx* ctx, void* stream, const pmp_aco_params* prm, const uint32_t* occ_bits, int n_plans,
                  const int32_t* starts, const int32_t* goals, const double* heur, int n_tables, const int32_t* heur_of,
                  const uint32_t* mt_state_in, int32_t* status, int32_t* best_len, int32_t* best_path, int32_t* n_cost,
                  int32_t* cost_list, int64_t* draws, uint32_t* mt_state_out, int32_t* ant_found, int32_t* ant_len,
                  double* pheromone, uint16_t* paths, int32_t* ant_scratch);
/* Waves per workgroup where pmp_aco_params.waves is 0, and the most it takes.  No device call. */
int pmp_aco_default_waves(void);
int pmp_aco_max_waves(void);
/* Entries of a path: ceil(x_range y_range / 2 + max(x_range, y_range)) + 1; 0 for a grid the entry refuses */
int pmp_aco_path_cap(int x_range, int y_range);
/* The next n values of random.random() from state_in [625] (random.getstate()[1]; an index above 624 is read
 * as 624) into out [n], and the state after them into state_out [625]: mt19937_dev.h's generator on its own.
 * All device pointers; one wave.  Refused with PMP_EINVAL: n < 0; null pointers. */
int pmp_mt19937_doubles(pmp_ctx* ctx, void* stream, const uint32_t* state_in, int64_t n, double* out, uint32_t* state_out);

/* Launch-span recording for profiling: while set, every A* 2D launch of this context folds its
 * workers' first start and last end wall-clock ticks into span[0] (atomic min) and span[1] (atomic
 * max); the caller initialises span to {UINT64_MAX, 0}.  NULL switches it off. */
int pmp_set_timing(pmp_ctx* ctx, uint64_t* span);
/* Work counters for profiling: while set, every MPC pmp_track_step_batch launch of this context adds
 * the number of QP solves it ran (agent-iterations whose MPC.plan branch called mpcControl,
 * mpc.py:85-91) into stats[0] (atomic add; the caller zeroes it).  The matrix-core work of a launch
 * is that count x ceil(3p / 16) x 10 v_mfma_f64_16x16x4 instructions.  NULL switches it off. */
int pmp_set_stats(pmp_ctx* ctx, int64_t* stats);
/* Rate of the wall-clock ticks above, in kHz. */
int pmp_wall_clock_khz(pmp_ctx* ctx, int* khz);
/* A* 2D query scheduling across the persistent workers: 1 (default) = longest start-goal distance
 * first (the expansion count grows with it, so long queries stop forming a tail), 0 = input order.
 * Results are identical either way; only which worker runs which query changes. */
int pmp_astar2d_set_schedule(pmp_ctx* ctx, int longest_first);
/* With the longest-first schedule, the first n_high queries (the longest) run at raised wave
 * priority, so they finish sooner and the short queries fill the issue slots they leave idle.
 * Default 64; 0 switches it off.  Results are identical for any value. */
int pmp_astar2d_set_priority(pmp_ctx* ctx, int n_high);
/* A* 2D queries resident per CU across all the launches that run at once, in [0, 128] (default 0 =
 * this context's own launch alone: ceil(max_slots / 256) of pmp_astar2d_reserve).  The LDS share of
 * each query's heap is 160 KiB / per_cu, so several batches in flight with fewer queries each (e.g.
 * 6 contexts x 2048 queries on the multi-query engine) set 48 here to stay resident together: every
 * batch's longest queries then start at once instead of behind the earlier batches.  A share too
 * small for the engine's fixed LDS needs is refused (PMP_EINVAL).  Re-sizes the reserved scratch
 * (call after pmp_astar2d_reserve).  Results are identical for any accepted value. */
int pmp_astar2d_set_residency(pmp_ctx* ctx, int per_cu);

/* A* 2D engine of the context (replaces nothing in the reference: a scheduling knob of
 * AStar.plan / Dijkstra.plan / GBFS.plan, a_star.py:39-83).  engine 2: four queries per wave, one
 * per 16-lane row, for A* / Dijkstra / GBFS whose heaps stay within 32,767 entries (a query that
 * outgrows it reports PMP_CAP_OVERFLOW; re-reserving with a larger heap_cap selects engine 0);
 * t2_lds = keep its level-10..14 heap direction bits in LDS (1) or HBM (0).  engine 0: one query per
 * wave (also Theta* / Lazy Theta*, and heaps of any size); on grids whose occupancy, cell state and
 * g fit in a wave's LDS share beside its heap (the README grid: 14 KB) all of them live in LDS.
 * engine 3: one query per workgroup with the CU's whole LDS as its heap (pmp_astar2d_sq_cap entries:
 * 13,632 beside no grid; a query that outgrows it reports PMP_CAP_OVERFLOW) and the heap's choice bits in
 * registers -- a single query's latency (the drop-in AStar.plan).  engine 1 (default): engine 3 for
 * batches of <= 256 queries whose heap capacity it holds, engine 2 for batches of >= 1024 queries on
 * grids too large for engine 0's LDS grid block, engine 0 otherwise.  Results are identical.
 * Applies to the next launch (re-reserves the scratch geometry when one is set). */
int pmp_astar2d_set_engine(pmp_ctx* ctx, int engine, int t2_lds);
/* Heap entries engine 3 holds for a W x H grid (its LDS beside the grid block it keeps in LDS on
 * small grids); 0 = the grid leaves too little for the engine.  No device call. */
int pmp_astar2d_sq_cap(int W, int H);

/* Persistent workers (one wave each) per CU of the one-wave-per-query planners: pmp_graph3d_batch,
 * pmp_dstar2d_batch / pmp_dstar2d_onpress_batch, pmp_dstar3d_batch and pmp_lpastar3d_batch (default 16
 * each), and the LPA* / D* Lite 2D entry points (default 24); 0 = the default.
 * Each launch caps it at ceil(nq / 256), so a small batch gets fewer workers with a larger LDS share
 * each.  Fewer workers leave each a larger LDS share of its heap (fewer spilled positions), more
 * workers hide more latency.  The longest-first schedule and its raised priority
 * (pmp_astar2d_set_schedule, pmp_astar2d_set_priority) apply to these planners as well.  Results are
 * identical for any value. */
int pmp_set_workers_per_cu(pmp_ctx* ctx, int per_cu);
/* pmp_dstar2d_batch / pmp_dstar2d_onpress_batch run in two passes: the first with a heap and entry
 * capacity of `entries` per query (0 = the default, W*H + 64: a smaller per-worker scratch, so more
 * workers fit the scratch budget), the second, on the same stream, re-runs every query whose heap or
 * entry list outgrew it with the bound (4 W*H + 64) on a few workers.  Results are identical for any
 * value. */
int pmp_dstar_set_first_cap(pmp_ctx* ctx, int entries);
/* Workers resident per CU over all the launches that run at once, for pmp_graph3d_batch,
 * pmp_dstar2d_batch / pmp_dstar2d_onpress_batch and pmp_dstar3d_batch: each worker's LDS heap share
 * is sized for max(this, the launch's own workers per CU), so several batches in flight with few
 * workers each stay resident together (as pmp_astar2d_set_residency for A* 2D); 0 = the launch's own
 * count.  pmp_rrt_batch sizes each query's LDS copy of its tree for this many workgroups per CU, at
 * least 2 (its 256-thread workgroups run two per CU) and at most 4.  Results are identical for any
 * value. */
int pmp_set_resident_per_cu(pmp_ctx* ctx, int per_cu);

/* Pre-size the A* scratch (heap of heap_cap entries per concurrent query, up to max_slots
 * concurrent queries) so that later batch calls allocate nothing (hipGraph-capturable). */
int pmp_astar2d_reserve(pmp_ctx* ctx, int W, int H, int max_slots, int heap_cap);
/* The A* 2D scratch geometry in force: out[0..5] = {W, H, max_slots, heap_cap in force, flags,
 * sized by the launches (1) or by pmp_astar2d_reserve (0)}; all 0 before any.  flags: bit 0 the
 * multi-query engine is reserved, bit 1 heap_cap was the caller's own (pmp_astar2d_reserve's
 * heap_cap > 0) -- without it the geometry is restored with heap_cap = 0 (the default, which the
 * engine may cut to its limit). */
int pmp_astar2d_geometry(pmp_ctx* ctx, int32_t* out6);
/* Forget the host's pmp_astar2d_reserve geometry: the next launch sizes the scratch for its own
 * batch and later larger batches grow it, as on a fresh context (allocated scratch is kept). */
int pmp_astar2d_reserve_auto(pmp_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* PMP_H */
