/*
 * mpcgpu_fleet.h -- C-ABI of the fleet coupling of the device tracker in libmpcgpu.so ("Fleet tick on the device").
 *
 * A fleet is B robots in groups ("worlds"): the robots of a group see each other's predicted positions through the
 * other-robot block of the problem (mpc_generator.py:179-188, block c), robots of different groups do not.  The reference
 * fills that block per robot from a dictionary (get_other_robot_states, src/scenario_simulator.py:154-163) and solves the
 * robots of a world one after the other, each seeing the FRESH prediction of those before it (:226-233).  The two calls
 * below are what a tick of that kind needs on top of include/mpcgpu.h's device tracker, with nothing read back:
 *
 *   Jacobi tick         share once, then mpcgpu_tracker_step_dev: every robot sees the previous tick's predictions.
 *   Gauss-Seidel tick   mpcgpu_tracker_window_dev once; then for colour c = 0, 1, ...: share, and the tick of the robots
 *                       at position c of every group (mpcgpu_tracker_step_rows_dev).  Robots of one colour belong to
 *                       different groups, so they are independent; the share in front of colour c hands it the
 *                       predictions colours < c have just written.  That is the reference's sequential loop.
 *
 * Group table (device memory, int32, written once by the caller):
 *     members [B]       the groups concatenated, each in its own order; a permutation of 0 .. B-1
 *     group_start [B]   robot b -> index in `members` where b's group begins
 *     group_len [B]     robot b -> number of robots of b's group (>= 1)
 *     pos [B]           robot b -> position of b inside its group: members[group_start[b] + pos[b]] == b
 * The library cannot check a table that lives on the device; a table that is not a partition gives a meaningless block
 * (indices are pinned into the arrays, nothing outside them is touched).
 *
 * All pointers are DEVICE pointers (float64 / int32 / uint8), `handle` is a handle of mpcgpu_create, `stream` follows the
 * convention of mpcgpu_solve_batch_dev.  0 = ok, < 0 = error (text via mpcgpu_last_error(handle)); arguments are checked
 * before anything is enqueued.  There is no CPU fallback.
 */
#ifndef MPCGPU_FLEET_H
#define MPCGPU_FLEET_H

#include <stdint.h>

#include "mpcgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* other [B][Nother][N][3] from pred_states [B][N][3]: slot s of robot b = the prediction of the s-th member of b's group
 * with b itself skipped, in group order; the first min(group_len[b] - 1, Nother) slots are filled, every other double of
 * the block is set to 0.0.  Copies only: bit for bit.  N must be the handle's N_hor, Nother is the handle's.  One kernel. */
int32_t mpcgpu_fleet_share_dev(void* handle, int32_t B, int32_t N, const int32_t* members, const int32_t* group_start,
                               const int32_t* group_len, const int32_t* pos, const double* pred_states, double* other,
                               void* stream);

/* mpcgpu_tracker_step_dev for the robots rows[0 .. n): problem j of the launch is robot rows[j].
 *   t, refs [B][N][3]         robot-indexed, t->B robots; only the rows of the call are read and updated
 *   rows [n] int32            DISTINCT robots in 0 .. B-1 (not checked here: the list is on the device; a row outside the
 *                             range is pinned into it for the assembly and skipped by the update); NULL = every robot in
 *                             order, and then n must be t->B
 *   u0 [n][2N] or NULL, u [n][2N], cost, status, inner_it, outer_it [n], actions_out [n][2]
 *                             compact, in the order of `rows` (inner_it, outer_it, actions_out may be NULL)
 *   arrived [B] uint8 or NULL robot-indexed: the termination test's verdict (1 / 0), written for the rows of the call
 *   stop_when_done            != 0: a robot whose test fires is frozen (active = 0, action 0), what InterfaceMpc.get_action
 *                             does; 0: the multi-robot simulator's rule -- the test only reports through `arrived`,
 *                             `active` is left as it is and the robot is solved and moved like every other
 * With rows == NULL, arrived == NULL and stop_when_done != 0 this is mpcgpu_tracker_step_dev, kernel for kernel.
 * Only enqueues, under the conditions of mpcgpu_tracker_step_dev (mpcgpu_reserve_shape; throughput / latency kernel rule for
 * n problems).  Everything ends on `stream`: the next call may read pred_states. */
int32_t mpcgpu_tracker_step_rows_dev(void* handle, const mpcgpu_tracker* t, const int32_t* rows, int32_t n,
                                     int32_t stop_when_done, uint8_t* arrived, const double* refs, const double* u0,
                                     double* u, double* cost, int32_t* status, int32_t* inner_it, int32_t* outer_it,
                                     double* actions_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
