/*
 * mpcgpu_eval.h -- C-ABI of evaluation episodes inside one launch in libmpcgpu.so.
 *
 * Every row of a ray environment plays E episodes to their end with the policy of mpcgpu_collect.h -- greedy with eps = 0, the
 * model.predict(deterministic=True) of an evaluation callback -- as launches of the step kernel of mpcgpu_env.h: grid B, one
 * wavefront per environment, up to S steps per row and launch.  A row that has its E episodes is PARKED: its wavefront returns
 * at once, and nothing of the row changes any more.
 *
 * PROGRESS of row b, four vectors the caller keeps between the launches of one evaluation (all zero at its start):
 *   episodes_done[b]   episodes the row has finished, 0 .. E
 *   steps_done[b]      steps the row has made in this evaluation
 *   ep_return[b]       the running return of the episode the row is in, a double
 *   ep_length[b]       the steps of that episode so far
 *
 * ONE LAUNCH.  The wavefront of row b:
 *   if episodes_done[b] >= E it returns before it reads or writes anything else (parked; so does a row whose count is negative,
 *   which no launch leaves behind);
 *   otherwise, while it has made fewer than S trips in this launch, a trip
 *   1. reads the observation the environment holds (obs_external[b], obs_internal[b]);
 *   2. acts by the rule of mpcgpu_collect.h with eps and serial serial0 + steps_done[b];
 *   3. runs the step of mpcgpu_env_step_autoreset_dev with that action;
 *   4. ep_return[b] = ep_return[b] + reward, one double addition; ep_length[b] and steps_done[b] grow by 1;
 *   5. when the episode ended (terminated or truncated), with e = episodes_done[b]:
 *        returns[b][e] = ep_return[b];  lengths[b][e] = ep_length[b];
 *        outcome[b][e] = (the step's flag word, state[26]) & 7, plus 8 when the step was a time-limit truncation
 *                        (bit 0 obstacle collision, bit 1 boundary collision, bit 2 goal reached, bit 3 time limit);
 *        then ep_return[b] = 0, ep_length[b] = 0, episodes_done[b] = e + 1;
 *   6. when episodes_done[b] is now E, the wavefront stops.  The auto-reset of that last step has happened: the row stands at
 *      the first observation of a new episode.
 *   Slots e >= episodes_done[b] of the three [B][E] outputs are never written.
 *
 * For every row the state, the environment's outputs, the progress vectors and the three [B][E] outputs are bit for bit what
 * driving that row alone from the host gives: mpcgpu_collect_act_dev, mpcgpu_env_step_autoreset_dev and the bookkeeping of 4
 * and 5, until its E-th episode ends.  A launch of S steps equals launches of S1 and S - S1 steps on the same progress vectors:
 * the serial comes from steps_done, nothing else is adjusted.  ceil(E * max_episode_steps / S) launches always finish every row.
 *
 * All pointers are DEVICE pointers except the two params structs.  The call enqueues ONE kernel on `stream` and returns: it
 * does not synchronise, allocate or copy, so it can be captured into a graph.  0 = ok, < 0 = error (text via
 * mpcgpu_eval_last_error, thread-local); a refused call touches no device and no array.  There is no CPU fallback.
 */
#ifndef MPCGPU_EVAL_H
#define MPCGPU_EVAL_H

#include <stdint.h>

#include "mpcgpu_collect.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPCGPU_EVAL_MAX_EPISODES      256    /* episodes per row of one evaluation */
#define MPCGPU_EVAL_MAX_LAUNCH_STEPS  4096   /* steps a row makes in one launch */

typedef struct mpcgpu_eval_params {
    double eps;                 /* 0 <= eps <= 1; 0 is model.predict(deterministic=True) */
    uint64_t seed, serial0;     /* the trip of row b draws from (seed, serial0 + steps_done[b]) */
    int32_t episodes;           /* E, 1 .. MPCGPU_EVAL_MAX_EPISODES */
    int32_t max_steps;          /* S, 1 .. MPCGPU_EVAL_MAX_LAUNCH_STEPS: steps of this launch, per row */
} mpcgpu_eval_params;

/*
 * params .. max_episode_steps: the arguments of mpcgpu_env_step_autoreset_dev without `action`, none of them NULL.
 * theta [1177] float (mpcgpu_dqn.h).  Progress, in and out: episodes_done [B] int32, steps_done [B] int64, ep_return [B] double,
 * ep_length [B] int32.  Outputs: returns [B][E] double, lengths [B][E] int32, outcome [B][E] uint8.
 * Refused: a NULL pointer, B < 0, E outside 1 .. 256, S outside 1 .. 4096, eps outside [0, 1] or NaN, max_episode_steps <= 0,
 * and the env params mpcgpu_env_step_autoreset_dev refuses, in its words.  B == 0 returns 0.
 */
int32_t mpcgpu_eval_rays_dev(int32_t device, const mpcgpu_env_params* params, int32_t B, const double* records, double* state,
                             float* obs_internal, float* obs_external, double* reward, uint8_t* terminated, uint8_t* truncated,
                             float* terminal_obs_internal, float* terminal_obs_external, int32_t max_episode_steps,
                             const float* theta, const mpcgpu_eval_params* eval, int32_t* episodes_done, int64_t* steps_done,
                             double* ep_return, int32_t* ep_length, double* returns, int32_t* lengths, uint8_t* outcome,
                             void* stream);

const char* mpcgpu_eval_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MPCGPU_EVAL_H */
