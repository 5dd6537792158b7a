/*
 * mpcgpu_collect_fresh.h -- C-ABI of collection inside one launch on the two-record table in libmpcgpu.so.
 *
 * T environment steps -- act, auto-reset step with map turnover, replay-buffer row, episode return -- as ONE launch of the step
 * kernel of mpcgpu_env.h on the [2][B][R] record table of mpcgpu_map.h: grid B, one wavefront per environment.  The action rule,
 * the ring row, the return bookkeeping and mpcgpu_collect_params are those of mpcgpu_collect.h; the step is the one of
 * mpcgpu_env_step_fresh_dev with max_episode_steps > 0.
 *
 * T STEPS.  The wavefront of row b, for t = 0 .. T - 1, does steps 1 .. 5 of mpcgpu_collect.h with the step of
 * mpcgpu_env_step_fresh_dev as step 3: an episode that ends in step t while spare_ready[b] is set starts its next episode on
 * the other table (which[b] flips, spare_ready[b] = 0, loaded[b] += 1), and otherwise resets on the record the row is on
 * (stale[b] += 1).  which[b] and spare_ready[b] are read again at every ending, so an ending sees what an earlier ending of the
 * same launch left.  There is one spare per row and nothing refills it inside the launch: the first ending of a row in a launch
 * may take the spare, every later ending in that launch finds spare_ready[b] = 0 and counts stale[b].
 *
 * A launch of T steps equals T rounds of mpcgpu_collect_act_dev, mpcgpu_env_step_fresh_dev (auto-reset, no refill between the
 * rounds) and the stores of step 4 and 5 of mpcgpu_collect.h, bit for bit: in the state, the observations, the reward (double),
 * the flags and the terminal observations, the five ring arrays, ep_return, the [T][B] outputs and which, spare_ready, loaded and
 * stale; records2 is not written.  It equals launches of T1 and T - T1 steps from (serial0, pos0) and
 * (serial0 + T1, (pos0 + T1 * B) mod capacity).  It is NOT equal to T such rounds with a refill of the spares between them: a
 * refill can only stand behind the launch.
 *
 * All pointers are DEVICE pointers except the two params structs.  The call enqueues ONE kernel on `stream` and returns: it does
 * not synchronise, allocate or copy to the host, so it can be captured into a graph.  0 = ok, < 0 = error (text via
 * mpcgpu_collect_fresh_last_error, thread-local, a slot of its own: a refusal here leaves mpcgpu_collect_last_error and
 * mpcgpu_env_last_error as they were); a refused call touches no device and no array.  There is no CPU fallback.
 */
#ifndef MPCGPU_COLLECT_FRESH_H
#define MPCGPU_COLLECT_FRESH_H

#include <stdint.h>

#include "mpcgpu_collect.h"
#include "mpcgpu_map.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The arguments of mpcgpu_collect_rays_dev with `records` replaced by records2 [2][B][R], which, spare_ready, loaded, stale [B]
 * int32, in the order of mpcgpu_env_step_fresh_dev.  Refused: a NULL which / spare_ready / loaded / stale, in the words of
 * mpcgpu_env_step_fresh_dev, first; then everything mpcgpu_collect_rays_dev refuses, in its order and its words
 * (max_episode_steps <= 0 included: this entry never only observes).
 */
int32_t mpcgpu_collect_rays_fresh_dev(int32_t device, const mpcgpu_env_params* params, int32_t B, const double* records2,
                                      int32_t* which, int32_t* spare_ready, int32_t* loaded, int32_t* stale, double* state,
                                      float* obs_internal, float* obs_external, double* reward, uint8_t* terminated,
                                      uint8_t* truncated, float* terminal_obs_internal, float* terminal_obs_external,
                                      int32_t max_episode_steps, const float* theta, const mpcgpu_collect_params* collect,
                                      float* buf_obs, float* buf_next_obs, int64_t* buf_actions, float* buf_rewards,
                                      float* buf_dones, double* ep_return, int32_t* actions, uint8_t* done, uint8_t* success,
                                      double* episode_return, void* stream);

const char* mpcgpu_collect_fresh_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MPCGPU_COLLECT_FRESH_H */
