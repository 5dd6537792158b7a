/*
 * mpcgpu_dqn.h -- C-ABI of the fused DQN update of the ray Q-network in libmpcgpu.so.
 *
 * One gradient step of dqn_train.DqnTrainer -- forward and backward of the 46 -> 16 -> 16 -> 9 ReLU network, Huber loss,
 * gradient clip and Adam -- as ONE launch of ONE workgroup, and K such steps on a uniform replay buffer as one launch.
 * The network is fixed to dqn.QNetwork's shape; arithmetic is float32 without fused multiply-add.
 *
 * Parameter vector: MPCGPU_DQN_PARAMS = 1 177 floats in the order of QNetwork.parameters(), row-major:
 *     W0 [16][46] at 0, b0 [16] at 736, W1 [16][16] at 752, b1 [16] at 1008, W2 [9][16] at 1024, b2 [9] at 1168
 * Gradients have the same layout (the all-reduce bucket of DqnTrainer).
 *
 * State block (floats, device, owned by the caller), mpcgpu_dqn_state_floats() = MPCGPU_DQN_STATE_FLOATS long, 8-byte aligned:
 *     [0, 1177) theta   [1177, 2354) target theta   [2354, 3531) m   [3531, 4708) v
 *     [4708, 4710) the step count t as ONE int64 (little endian, the two float slots hold its bits)   [4710, 4712) reserved
 * The target parameters are only read: a hard target sync is the caller's copy of [0, 1177) onto [1177, 2354).
 *
 * ONE STEP on rows i = 0 .. n - 1 (1 <= n <= MPCGPU_DQN_MAX_ROWS).  Every operation is a rounded float32 operation, in the
 * order written; x * y + z is two operations.
 *   dense layer       out[j] = acc,  acc = b[j];  acc = acc + W[j][k] * x[k]  for k ascending;  hidden layers: max(acc, 0)
 *   next_v            the target network on next_obs gives qt[0..8].  Without double_q: v = qt[0]; for a = 1 .. 8:
 *                     if qt[a] > v then v = qt[a].  With double_q the same scan over the ONLINE network's values on next_obs
 *                     finds the index (a strict > keeps the lowest index at a tie) and v = qt[index].
 *   target            y = r + ((1 - done) * gamma) * v
 *   delta             d = y - q[a],  a = action clamped into 0 .. 8,  q = the online network on obs
 *   loss row          e = |d|;  l = e < 1 ? (0.5 * e) * e : e - 0.5;  weighted: l = w * l
 *   loss              the rows' l in slots 0 .. 255 (0 from slot n on), folded in halves: slot[s] = slot[s] + slot[s + h] for
 *                     h = 128, 64, .., 1; loss = slot[0] / n
 *   row coefficient   c = (e < 1 ? -d : (d > 0 ? -1 : 1));  weighted: c = w * c;  g = c / n   (d loss / d q[a])
 *   backward          dz2[j] = j == a ? g : 0;   dz1[k] = h2[k] > 0 ? W2[a][k] * g : 0;   dh1[k] = acc, acc = 0,
 *                     acc = acc + W1[j][k] * dz1[j] for j ascending;   dz0[k] = h1[k] > 0 ? dh1[k] : 0
 *                     (h1, h2: the hidden activations on obs)
 *   gradient          every entry: acc = 0; acc = acc + (row i's term) for i ascending.  Terms: W0[j][k]: dz0[j] * x[k];
 *                     b0[j]: dz0[j];  W1[j][k]: dz1[j] * h1[k];  b1[j]: dz1[j];  W2[j][k]: dz2[j] * h2[k];  b2[j]: dz2[j].
 *                     This is the UNCLIPPED mean gradient.
 *   apply             g := g * scale.  Sum of squares: lane L = 0 .. 255 adds g[p]^2 for p = L, L + 256, .. ascending
 *                     (from 0), the 256 lane sums are folded in halves as the loss is; norm = sqrt(sum);
 *                     coef = min(1, max_grad_norm / (norm + 1e-6));  g := g * coef.
 *                     t := t + 1;  in float64: bc1 = 1 - beta1^t, bc2 = 1 - beta2^t (pow as the C library rounds it,
 *                     per_pow.hpp), step = lr / bc1, root = sqrt(bc2); both rounded to float32.  Then
 *                     m = beta1 * m + (1 - beta1) * g;   v = beta2 * v + (1 - beta2) * (g * g);
 *                     theta = theta - step * (m / (sqrt(v) / root + eps))
 *                     with beta1, beta2, eps rounded to float32 and 1 - beta formed in float64, then rounded.
 * Nothing above depends on how the kernel spreads the work over its threads.
 *
 * All pointers are DEVICE pointers.  Every call enqueues ONE kernel on `stream` and returns: none synchronises, allocates
 * or copies to the host, so all of them can be captured into a graph.  0 = ok, < 0 = error (text via
 * mpcgpu_dqn_last_error, thread-local); a refused call enqueues nothing.  There is no CPU fallback.
 */
#ifndef MPCGPU_DQN_H
#define MPCGPU_DQN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCGPU_DQN_OBS 46
#define MPCGPU_DQN_HIDDEN 16
#define MPCGPU_DQN_ACTIONS 9
#define MPCGPU_DQN_PARAMS 1177
#define MPCGPU_DQN_MAX_ROWS 256          /* rows of one minibatch */
#define MPCGPU_DQN_MAX_STEPS 65536       /* steps of one train call */
#define MPCGPU_DQN_STATE_T 4708          /* float offset of the int64 step count */
#define MPCGPU_DQN_STATE_FLOATS 4712

typedef struct mpcgpu_dqn_params {
    double lr;              /* > 0 */
    double gamma;
    double max_grad_norm;   /* > 0 */
    double beta1, beta2;    /* 0 <= beta < 1 */
    double eps;             /* > 0 */
    int32_t double_q;       /* 0 / 1 */
    int32_t reserved;       /* 0 */
} mpcgpu_dqn_params;

/* floats of the state block (no device needed) */
int32_t mpcgpu_dqn_state_floats(void);

/*
 * obs, next_obs [n][46] float, actions [n] int64, rewards, dones [n] float, weights [n] float or NULL (all 1).
 * Writes grad [1177] (unclipped mean gradient), loss [1] and, when td is not NULL, td [n] = delta.  The state is only read.
 */
int32_t mpcgpu_dqn_grad_dev(int32_t device, const mpcgpu_dqn_params* params, const float* state, const float* obs,
                            const float* next_obs, const int64_t* actions, const float* rewards, const float* dones,
                            const float* weights, int32_t n, float* grad, float* loss, float* td, void* stream);

/* grad [1177] times scale (1 / world after an all-reduce): clip, Adam step, t += 1.  grad is only read. */
int32_t mpcgpu_dqn_apply_dev(int32_t device, const mpcgpu_dqn_params* params, float* state, const float* grad, float scale,
                             void* stream);

/* grad_dev and apply_dev (scale 1) in one launch, bit for bit; inputs and outputs as grad_dev */
int32_t mpcgpu_dqn_step_dev(int32_t device, const mpcgpu_dqn_params* params, float* state, const float* obs,
                            const float* next_obs, const int64_t* actions, const float* rewards, const float* dones,
                            const float* weights, int32_t n, float* grad, float* loss, float* td, void* stream);

/*
 * K steps (1 <= K <= MPCGPU_DQN_MAX_STEPS) without weights on a uniform replay buffer of `size` rows (1 <= size < 2^31), given
 * as its five arrays.  Row i of step s (0 <= s < K) is buffer row (bits * size) >> 64 with
 *     bits = mix64(mix64(seed + G * (serial0 + s)) + G * (i + 1))      (mix64, G: the stream of mpcgpu_map.h)
 * so a run of K steps equals runs of K1 and K - K1 steps from serial0 and serial0 + K1.  losses [K].
 */
int32_t mpcgpu_dqn_train_dev(int32_t device, const mpcgpu_dqn_params* params, float* state, const float* buf_obs,
                             const float* buf_next_obs, const int64_t* buf_actions, const float* buf_rewards,
                             const float* buf_dones, int64_t size, int32_t n, int32_t K, uint64_t seed, uint64_t serial0,
                             float* losses, void* stream);

const char* mpcgpu_dqn_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MPCGPU_DQN_H */
