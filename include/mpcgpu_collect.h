/*
 * mpcgpu_collect.h -- C-ABI of collection inside one launch in libmpcgpu.so.
 *
 * The epsilon-greedy policy of the ray Q-network (dqn.QNetwork, 46 -> 16 -> 16 -> 9, parameter layout of mpcgpu_dqn.h) as one
 * launch, and T environment steps -- act, auto-reset step, replay-buffer row, episode return -- as one launch of the step
 * kernel of mpcgpu_env.h: grid B, one wavefront per environment.
 *
 * THE ACTION of step s (a running serial) on row b, with the parameter vector theta (MPCGPU_DQN_PARAMS floats) and
 * x = the row's flat observation, 32 external values then 14 internal ones (dqn_train.flatten_observation):
 *   q[0..8]   the online network on x by the dense-layer rule of mpcgpu_dqn.h: out[j] = acc, acc = b[j];
 *             acc = acc + W[j][k] * x[k] for k ascending; hidden layers: acc > 0 ? acc : 0.  Every product and every sum
 *             is a rounded float32 operation; x * y + z is two operations.
 *   greedy    greedy = 0; for a = 1 .. 8: if q[a] > q[greedy] then greedy = a   (a strict > keeps the lowest index at a tie)
 *   key       key = mix64(seed + G * s)                                         (mix64, G: the stream of mpcgpu_map.h,
 *   bits_e    bits_e = mix64(key + G * (2 b + 1))                                all sums and products modulo 2^64)
 *   bits_a    bits_a = mix64(key + G * (2 b + 2))
 *   u         u = (bits_e >> 11) * 2^-53, a double in [0, 1);   explore = u < eps, compared in double
 *   random    random = (bits_a * 9) >> 64, the high half of the 128-bit product
 *   action    action = explore ? random : greedy
 * Nothing above depends on how the kernel spreads the work over its lanes.
 *
 * T STEPS.  The wavefront of row b, for t = 0 .. T - 1:
 *   1. reads the observation the environment holds (obs_external[b], obs_internal[b]);
 *   2. acts by the rule above with serial serial0 + t and eps[t];
 *   3. runs the step of mpcgpu_env_step_autoreset_dev with that action;
 *   4. writes ring row (pos0 + t * B + b) mod capacity: obs = the observation acted on; next_obs = the terminal observation
 *      when the episode ended in this step, else the new observation; the action; (float) reward; dones = 1 when the step
 *      terminated (collision or goal), 0 otherwise -- a time-limit truncation is not terminal;
 *   5. ep_return[b] = ep_return[b] + reward, one double addition; when the episode ended (terminated or truncated) the sum is
 *      reported in episode_return[t][b] and ep_return[b] becomes 0.
 * A launch of T steps equals T rounds of mpcgpu_collect_act_dev, mpcgpu_env_step_autoreset_dev and the stores of step 4 and 5
 * bit for bit, and equals launches of T1 and T - T1 steps from (serial0, pos0) and (serial0 + T1, (pos0 + T1 * B) mod capacity).
 *
 * All pointers are DEVICE pointers except the two params structs.  Every call enqueues ONE kernel on `stream` and returns:
 * none synchronises, allocates or copies to the host, so both can be captured into a graph.  0 = ok, < 0 = error (text via
 * mpcgpu_collect_last_error, thread-local); a refused call touches no device and no array.  There is no CPU fallback.
 */
#ifndef MPCGPU_COLLECT_H
#define MPCGPU_COLLECT_H

#include <stdint.h>

#include "mpcgpu_dqn.h"
#include "mpcgpu_env.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPCGPU_COLLECT_MAX_STEPS 64     /* steps of one launch */

typedef struct mpcgpu_collect_params {
    double eps[MPCGPU_COLLECT_MAX_STEPS];   /* eps[t] of step t, 0 <= eps <= 1; entries from T on are not read */
    uint64_t seed, serial0;                 /* step t draws from (seed, serial0 + t) */
    int64_t capacity;                       /* rows of the ring, >= T * B */
    int64_t pos0;                           /* 0 <= pos0 < capacity: ring row of (t = 0, b = 0) */
    int32_t T;                              /* 1 .. MPCGPU_COLLECT_MAX_STEPS */
    int32_t reserved;                       /* 0 */
} mpcgpu_collect_params;

/*
 * The action rule on B rows: obs_external [B][32], obs_internal [B][14] float, theta [1177] float.
 * Writes actions [B] int32 and, when q is not NULL, q [B][9] float.  0 <= eps <= 1.
 */
int32_t mpcgpu_collect_act_dev(int32_t device, const float* theta, const float* obs_external, const float* obs_internal,
                               int32_t B, double eps, uint64_t seed, uint64_t serial, int32_t* actions, float* q, void* stream);

/*
 * T steps in one launch.  params .. max_episode_steps: the arguments of mpcgpu_env_step_autoreset_dev without `action`, none of
 * them NULL; on return they hold what T auto-reset steps leave in them.  The ring: buf_obs, buf_next_obs [capacity][46] float,
 * buf_actions [capacity] int64, buf_rewards, buf_dones [capacity] float; rows outside the T * B written ones are not touched.
 * ep_return [B] double, in and out.  Optional [T][B] outputs, NULL allowed: actions int32, done uint8 (terminated or
 * truncated), success uint8 (the goal was reached in this step), episode_return double (written only where done).
 * Refused: a NULL pointer, T outside 1 .. 64, T * B > capacity, pos0 outside the ring, max_episode_steps <= 0, an eps[t]
 * (t < T) outside [0, 1] or NaN, and the env params mpcgpu_env_step_autoreset_dev refuses, in its words.
 */
int32_t mpcgpu_collect_rays_dev(int32_t device, const mpcgpu_env_params* params, int32_t B, const double* records, double* state,
                                float* obs_internal, float* obs_external, double* reward, uint8_t* terminated,
                                uint8_t* truncated, float* terminal_obs_internal, float* terminal_obs_external,
                                int32_t max_episode_steps, const float* theta, const mpcgpu_collect_params* collect,
                                float* buf_obs, float* buf_next_obs, int64_t* buf_actions, float* buf_rewards, float* buf_dones,
                                double* ep_return, int32_t* actions, uint8_t* done, uint8_t* success, double* episode_return,
                                void* stream);

const char* mpcgpu_collect_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MPCGPU_COLLECT_H */
