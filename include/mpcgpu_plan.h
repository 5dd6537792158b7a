/*
 * mpcgpu_plan.h -- C-ABI of the batched visibility-graph shortest-path planner in libmpcgpu.so.
 *
 * Replaces what the reference asks of extremitypathfinder on every reset (src/pkg_dqn/environment/environment.py:122-146):
 * given the inflated boundary, the inflated obstacle outlines and two points, the shortest start-to-goal path that stays
 * in free space.  One launch plans B independent maps, one workgroup per map.  Inflation is the caller's business.
 *
 * Record of one map (doubles, mpcgpu_plan_record_doubles(params) long, rows of `rings`):
 *     [0] number of rings R (1 .. n_ring_max)      [1] number of ring vertices V (sum of the ring sizes, <= n_vert_max)
 *     [2 .. 2 + n_ring_max)  vertices of ring k (>= 3; 0 beyond R)
 *     [2 + n_ring_max ..)    x, y of every vertex, ring after ring (2 * n_vert_max doubles)
 * Ring 0 is the boundary, COUNTER-CLOCKWISE; rings 1 .. R - 1 are obstacles, CLOCKWISE (the host normalises that).  The
 * obstacles may overlap each other and may stick out of the boundary.  Free space is the closed set inside ring 0 minus
 * the open interiors of the obstacles.
 *
 * Graph nodes are start (0), goal (1), then every ring vertex, in table order, that is reflex as seen from free space, not
 * strictly inside another obstacle and not strictly outside ring 0.  Two nodes see each other iff the open segment
 * between them meets no point strictly inside an obstacle or strictly outside the boundary (running along an edge and
 * touching a vertex are allowed).  The path is Dijkstra's from start over sqrt(dx*dx + dy*dy): the next node is the
 * smallest (distance, node index), dist[v] is replaced only when dist[u] + w < dist[v] strictly, and the search ends when
 * goal is settled.
 *
 * Output per map:
 *     status [B] int32: 0 ok, 1 no path, 2 start or goal not in free space, 3 more than n_node_max path nodes,
 *                       4 malformed record (ring count / sizes outside the limits of `params`)
 *     n_nodes [B] int32: path nodes incl. start and goal (status 0; the count found for status 3; else 0)
 *     nodes [B][MPCGPU_PLAN_MAX_NODES][2] doubles: copies of the input coordinates, 0 beyond n_nodes
 *     length [B] doubles: sum of the segment lengths in path order (0 unless status 0)
 *
 * All pointers are DEVICE pointers.  The call enqueues one kernel on `stream` and returns: it does not synchronise,
 * allocate or copy, so it can be captured into a graph.  0 = ok, < 0 = error (text via mpcgpu_plan_last_error,
 * thread-local); limits are checked before anything is enqueued.  There is no CPU fallback.
 */
#ifndef MPCGPU_PLAN_H
#define MPCGPU_PLAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCGPU_PLAN_MAX_VERTICES 256   /* ring vertices of one map */
#define MPCGPU_PLAN_MAX_RINGS 32       /* rings of one map, the boundary included */
#define MPCGPU_PLAN_MAX_NODES 64       /* nodes of a returned path (n_path_max limit of the environment record) */

typedef struct mpcgpu_plan_params {
    int32_t n_vert_max;   /* 3 .. MPCGPU_PLAN_MAX_VERTICES: vertex capacity of a record */
    int32_t n_ring_max;   /* 1 .. MPCGPU_PLAN_MAX_RINGS: ring capacity of a record */
    int32_t n_node_max;   /* 2 .. MPCGPU_PLAN_MAX_NODES: longer paths give status 3 */
    int32_t reserved;     /* 0 */
} mpcgpu_plan_params;

/* doubles of one map record (no device needed); < 0 if params is outside the limits */
int32_t mpcgpu_plan_record_doubles(const mpcgpu_plan_params* params);

/* rings [B][record_doubles], start_goal [B][4] doubles (start x, y, goal x, y); outputs as described above */
int32_t mpcgpu_plan_paths_dev(int32_t device, const mpcgpu_plan_params* params, int32_t B, const double* rings,
                              const double* start_goal, int32_t* status, int32_t* n_nodes, double* nodes, double* length,
                              void* stream);

const char* mpcgpu_plan_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
