/*
 * mpcgpu_dqn_per.h -- C-ABI of the prioritized K-step launch of the fused DQN update in libmpcgpu.so.
 *
 * K gradient steps of the ray Q-network on a PRIORITIZED replay buffer as ONE launch of ONE workgroup: every step draws its
 * minibatch from the sum tree of mpcgpu_per.h, makes the weighted step of mpcgpu_dqn.h and writes the new priorities back,
 * tree repaired, before the next step samples.  The state block is the one of mpcgpu_dqn.h, the tree the one of mpcgpu_per.h
 * (2 * capacity - 1 doubles, heap order); the tree's state block (max_p, rows since it was read) is not touched, as
 * mpcgpu_per_update_dev does not touch it.
 *
 * ONE STEP, step s of a launch (0 <= s < K), rows i = 0 .. n - 1 (1 <= n <= MPCGPU_DQN_MAX_ROWS), C = per->capacity:
 *   1 draw            bits_i = mix64(mix64(seed + G * (serial0 + s)) + G * (i + 1))   (mix64, G: the stream of mpcgpu_map.h; the
 *                     stream of mpcgpu_dqn_train_dev);  u_i = (double)(bits_i >> 11) * 2^-53, in [0, 1)
 *   2 sample          as mpcgpu_per_sample_dev on u:  total = tree[0];  segment = total / (double)n;  a = segment * i;
 *                     b = segment * (i + 1);  s_i = a + (b - a) * u_i;  from the root: left if s <= tree[left], else right with
 *                     s - tree[left]; a child whose sum is 0 is never entered (its sibling is taken instead);  idx_i = the leaf
 *                     reached;  pos_i = idx_i - (C - 1);  w_i = pow((double)n_entries * tree[idx_i] / total, -beta) (pow as the
 *                     C library rounds it, per_pow.hpp);  wmax = the maximum over the rows;  weight_i = (float)(w_i / wmax)
 *   3 step            the ONE STEP of mpcgpu_dqn.h on buffer rows pos_i with weights weight_i: weighted loss row and weighted
 *                     coefficient, then apply with scale 1;  losses[s] = that step's loss;  d_i = that step's delta
 *   4 re-prioritise   as mpcgpu_per_update_dev on (idx, d):  leaf idx_i := pow(|d_i| + epsilon, alpha) in float64 from the
 *                     float32 d_i; on a repeated index the highest row i wins;  then every ancestor of a written leaf is
 *                     recomputed as tree[left] + tree[right], depth by depth, deepest first
 * Step s + 1 samples from the tree that step s left.  So one launch of K steps equals, bit for bit in the state block, all
 * 2 C - 1 doubles of the tree and the K losses, K rounds of mpcgpu_per_sample_dev(u), a gather of the rows,
 * mpcgpu_dqn_step_dev with those weights and mpcgpu_per_update_dev(indices, delta); and a launch of K steps equals launches
 * of K1 and K - K1 steps from serial0 and serial0 + K1.
 *
 * The descent always ends on a leaf, so 0 <= pos_i < C whatever the tree holds: the five buffer arrays must hold C rows
 * (rows that were never written are read when the tree gives them a priority).  Actions are clamped into 0 .. 8.  On a tree
 * whose root is 0 the results are unspecified; nothing is indexed out of bounds.
 *
 * All pointers are DEVICE pointers.  The call enqueues ONE kernel on `stream` and returns: it does not synchronise, allocate
 * or copy to the host, so it can be captured into a graph.  0 = ok, < 0 = error (text via mpcgpu_dqn_per_last_error,
 * thread-local); a refused call enqueues nothing: invalid dqn or per parameters (the rules of the two headers), n outside
 * 1 .. 256, K outside 1 .. MPCGPU_DQN_MAX_STEPS, n_entries outside 1 .. capacity, a null required pointer.  There is no CPU
 * fallback.
 */
#ifndef MPCGPU_DQN_PER_H
#define MPCGPU_DQN_PER_H

#include <stdint.h>

#include "mpcgpu_dqn.h"
#include "mpcgpu_per.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * state: the block of mpcgpu_dqn.h;  tree [2 * capacity - 1] doubles;  buf_*: the replay buffer's five arrays, capacity rows
 * each;  n_entries = transitions stored;  losses [K];  indices [K][n] int64 (the tree indices every step drew) or NULL;
 * td [K][n] float (every step's delta) or NULL.
 */
int32_t mpcgpu_dqn_train_per_dev(int32_t device, const mpcgpu_dqn_params* dqn, const mpcgpu_per_params* per,
                                 float* state, double* tree,
                                 const float* buf_obs, const float* buf_next_obs, const int64_t* buf_actions,
                                 const float* buf_rewards, const float* buf_dones,
                                 int64_t n_entries, int32_t n, int32_t K, uint64_t seed, uint64_t serial0,
                                 float* losses /* [K] */, int64_t* indices /* [K][n] or NULL */,
                                 float* td /* [K][n] or NULL */, void* stream);

const char* mpcgpu_dqn_per_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MPCGPU_DQN_PER_H */
