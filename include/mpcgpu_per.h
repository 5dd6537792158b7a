/*
 * mpcgpu_per.h -- C-ABI of the device-resident sum tree of prioritized experience replay in libmpcgpu.so.
 *
 * Replaces PerReplayBuffer of the reference (src/pkg_dqn/utils/per_dqn.py:25-187): the priorities of the stored
 * transitions as the leaves of a binary sum tree, `add` (new rows take the running maximum), `update_priority` and the
 * stratified `sample` with its importance weights.  The transitions themselves are the caller's business.
 *
 * The tree is ONE device array of 2 * capacity - 1 doubles owned by the caller, in heap order: the children of node i
 * are 2 i + 1 and 2 i + 2, the leaf of ring position pos is node pos + capacity - 1.  capacity is any positive integer,
 * so the leaves sit on two depths.  An inner node is always tree[left] + tree[right], recomputed bottom-up, depth by
 * depth, after a leaf below it changed (never `+= change`): the sums do not drift.
 *
 * State block (doubles, device, owned by the caller, written by the kernels only), mpcgpu_per_state_doubles() long:
 *     [0] max_p: the priority new rows take   [1] rows added since max_p was last read (a whole number)
 *     [2..3] reserved (0)   [4..] scratch of the maximum reduction (contents unspecified)
 *
 * All pointers are DEVICE pointers.  Every call enqueues its kernels on `stream` and returns: none synchronises,
 * allocates or copies to the host, so all of them can be captured into a graph (sizes, positions and n_entries are baked
 * into a captured call like any other kernel argument).  Plain pointers and sizes, no ownership taken, no exceptions:
 * 0 = ok, < 0 = error (text via mpcgpu_per_last_error, thread-local).  Every call checks the parameters first and refuses,
 * before it touches the device, what the comments of mpcgpu_per_params exclude (a NaN is excluded everywhere).  There is no CPU
 * fallback.
 */
#ifndef MPCGPU_PER_H
#define MPCGPU_PER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCGPU_PER_MAX_ROWS 4096       /* rows of one update / sample call */

typedef struct mpcgpu_per_params {
    int64_t capacity;          /* 1 .. 2^30 */
    int64_t update_max_freq;   /* >= 1: max_p is re-read at the start of an add call once this many rows were added since */
    double alpha;              /* >= 0: priority = (|td| + epsilon)^alpha, 0.3 */
    double beta;               /* >= 0 and finite (0: every weight is 1): weight = (n_entries * p / total)^-beta, 0.4 */
    double epsilon;            /* >= 0, 1e-3 */
    double initial_priority;   /* max_p of an empty buffer, 1 */
} mpcgpu_per_params;

/* doubles of the state block (no device needed) */
int32_t mpcgpu_per_state_doubles(void);

/* tree := 0, state := (initial_priority, update_max_freq, 0, 0): the next add reads max_p */
int32_t mpcgpu_per_reset_dev(int32_t device, const mpcgpu_per_params* params, double* tree, double* state, void* stream);

/*
 * Rows pos .. pos + n - 1 (mod capacity) take max_p; n_entries = transitions stored BEFORE this call (0: the buffer is
 * empty and max_p is initial_priority).  If update_max_freq or more rows were added since the last reading, max_p is
 * first re-read as the maximum over all leaves.  n >= 1; n > capacity writes every leaf.
 */
int32_t mpcgpu_per_add_dev(int32_t device, const mpcgpu_per_params* params, double* tree, double* state, int64_t pos,
                           int64_t n, int64_t n_entries, void* stream);

/*
 * indices [n] int64 (tree indices as returned by sample), td_error [n] float: leaf := (|td| + epsilon)^alpha in float64.
 * On a repeated index the highest row wins.  A row whose index is not a leaf is ignored.  1 <= n <= MPCGPU_PER_MAX_ROWS.
 */
int32_t mpcgpu_per_update_dev(int32_t device, const mpcgpu_per_params* params, double* tree, const int64_t* indices,
                              const float* td_error, int32_t n, void* stream);

/*
 * u [n] doubles in [0, 1).  Row i descends with s = a + (b - a) u_i, a = segment i, b = segment (i + 1), segment =
 * tree[0] / n: left if s <= tree[left], else right with s - tree[left]; a child whose sum is 0 is never entered (its
 * sibling is taken instead).  indices [n] int64 tree indices, positions [n] int64 ring positions, weights [n] float:
 * (n_entries * tree[index] / tree[0])^-beta divided by their maximum.  1 <= n <= MPCGPU_PER_MAX_ROWS, n_entries >= 1.
 */
int32_t mpcgpu_per_sample_dev(int32_t device, const mpcgpu_per_params* params, const double* tree, const double* u,
                              int32_t n, int64_t n_entries, int64_t* indices, int64_t* positions, float* weights,
                              void* stream);

/* diagnostics: out[0] = tree[0] (sum of all priorities), out[1] = max_p; out is a device pointer to 2 doubles */
int32_t mpcgpu_per_stats_dev(int32_t device, const mpcgpu_per_params* params, const double* tree, const double* state,
                             double* out, void* stream);

const char* mpcgpu_per_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
