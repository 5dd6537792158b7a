// envgpu_internal.hpp -- what the image-observation entries (envimg.hip) and the map stream (mapgpu.hip) share with the
// environment step (envgpu.hip): the record layout, the error slot of mpcgpu_env_last_error and the shared argument checks.
// Not part of the C-ABI: the public declarations are in include/mpcgpu_env.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mpcgpu_env.h"
#include "abi_host.hpp"

namespace envgpu {

struct EnvK {
    mpcgpu_env_params p;
    int rec, o_cum, o_len, o_xy, o_anim, an, o_edge;
};

struct EnvOut {
    float* obs_int; float* obs_ext; double* reward; uint8_t* terminated;
    // in-kernel auto-reset (max_steps > 0): time-limit flag, and where the observation an episode ENDED in is kept
    uint8_t* truncated; float* term_int; float* term_ext; int max_steps;
    // image variant only (NULL otherwise): per-environment image state (IMG_STATE doubles) that receives, at IMG_PRE..+4,
    // the pose and clock the step observed BEFORE an in-kernel reset and whether that reset happened; the fresh-map step
    // adds, at IMG_PRE + 5, the record table the row was on when the step began
    double* pre_reset;
};

// the fresh-map step (include/mpcgpu_map.h): per-row table selector, spare flag and the two counters; unused (null) otherwise
struct EnvFresh {
    int32_t* which; int32_t* spare_ready; int32_t* loaded; int32_t* stale;
};

// per-environment image state (mpcgpu_env_img_state_doubles): [0] observations since the last reset, [1..6] obstacle
// clock of each of the last 6 observations (ring, slot (k - 1) % 6 holds observation k), [7] reserved,
// [8..11] x, y, theta, clock of the last step before an in-kernel reset, [12] 1 when that reset happened,
// [13] fresh-map step only (include/mpcgpu_map.h): 0 / 1, the record table the row was on at the entry of that step -- the
// record an episode that ended in it ENDED on, while which[b] already names the one the next episode starts on,
// [14..15] reserved.  [8..13] are hand-over scratch between the two launches of one step, rewritten by every step.
constexpr int IMG_STATE = 16;
constexpr int IMG_HIST = 6;
constexpr int IMG_PRE = 8;

// what every entry that takes mpcgpu_env_params says when layout() refuses them
constexpr const char* BAD_PARAMS = "invalid mpcgpu_env_params (P 2..64, M 0..31, K 1..4, E >= 1)";

bool layout(const mpcgpu_env_params& p, EnvK& k);
extern thread_local abi::ErrorSlot g_err;   // mpcgpu_env_last_error: the ray, image and fresh-map entries share it
inline int fail(const char* what) { return g_err.fail(what); }
// the argument checks of the auto-reset step, rays and images (the refusal names the variant's entry that only observes)
int autoreset_args(const int32_t* action, int32_t max_episode_steps, bool images);
// the argument checks of the fresh-map step, rays and images (include/mpcgpu_map.h).  `also_bad` is a refusal of the caller's own
// that ranks second, or NULL.  `out` comes in filled as for an auto-reset step; with max_episode_steps = 0 the step only
// observes and the fields of the in-kernel reset are cleared
int fresh_args(const EnvFresh& fresh, const char* also_bad, const int32_t* action, EnvOut& out);
// validates params and pointers (obs_ext may be NULL when need_ext is false) and enqueues env_step_kernel<false>, or
// env_step_kernel<true> on a [2][B][rec] table when `fresh` is given
int launch_step(int32_t device, const mpcgpu_env_params* params, int32_t B, const double* records, double* state,
                const int32_t* action, EnvOut out, bool need_ext, void* stream, const EnvFresh* fresh = nullptr);

}  // namespace envgpu
