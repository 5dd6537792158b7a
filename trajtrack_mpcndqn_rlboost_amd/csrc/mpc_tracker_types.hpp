// mpc_tracker_types.hpp -- what mpcgpu.hip (host entry points, assembly kernel) and trackgpu.hip (the small per-robot kernels)
// share: the device view of the tracker state and the launchers of trackgpu.hip's kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mpcgpu {

// device view of the tracker state of B robots (all pointers are device memory owned by the caller)
struct TrackerView {
    int B, ref_cap, action_steps;
    double* states;              // [B][3]  in/out
    const double* goals;         // [B][3]
    double* last_actions;        // [B][2]  in/out
    const double* ref;           // [B][ref_cap][3] global reference trajectories, padded
    const int32_t* ref_len;      // [B]
    int32_t* idx_ref;            // [B]     in/out
    const double* stc;           // [B][Nstcobs * nstcobs]
    const double* dyn;           // [B][Ndynobs * 6 * N]
    const double* other;         // [B][3 * N * Nother] or NULL (zeros)
    double* pred_states;         // [B][N][3]  out
    uint8_t* active;             // [B]  in/out
    double tuning[10];           // tuning_params of the work mode
    double base_speed, low_speed, stc_weight, dyn_weight;
    // fleet form of a tick (include/mpcgpu_fleet.h): problem j of a launch is robot rows[j].  Appended, so that the fields above
    // keep their kernel-argument offsets; the kernels of the plain tick are instantiated without them (fleet_form == false).
    const int32_t* rows;         // [n] distinct robots in 0..B-1, or NULL (problem j is robot j)
    uint8_t* arrived;            // [B] or NULL: the termination test's verdict for the rows of the call
    int n;                       // problems of the launch (B without a row list)
    int stop_when_done;          // 1: a robot whose termination test fires is frozen (active = 0); 0: only `arrived` is written
};
// the plain tick: every robot, in order, frozen on arrival -- the form whose kernels never look at the four fields above
inline bool fleet_form(const TrackerView& t) { return t.rows != nullptr || t.arrived != nullptr || t.stop_when_done == 0; }

// launchers of the kernels that live in trackgpu.hip (their own translation unit: the ILP scheduler this file is compiled with
// crashes LLVM's register allocator on the rollout loops)
struct RlLimits { double acc_max, acc_min, angacc_max, angacc_min, speed_min, speed_max, angvel_min, angvel_max; };
hipError_t launch_tracker_window(const TrackerView& t, int N, double* refs_out, hipStream_t s);
hipError_t launch_tracker_apply(const TrackerView& t, int N, double ts, const double* u, double* actions_out, hipStream_t s);
// other [B][Nother][N][3] from pred_states [B][N][3] and the group table (fleet_share_kernel)
hipError_t launch_fleet_share(int B, int N, int Nother, const int32_t* members, const int32_t* group_start, const int32_t* group_len,
                              const int32_t* pos, const double* pred_states, double* other, hipStream_t s);
hipError_t launch_rl_reference(int B, const double* agent, int agent_stride, const int64_t* action, double ts, int steps,
                               double ref_speed, const RlLimits& lim, double* rl_ref, hipStream_t s);
hipError_t launch_hint_switch(int B, int N, int O, int V, const double* polygons, const uint8_t* valid, const double* states,
                              const double* original, const double* rl_ref, int rl_steps, const uint8_t* live,
                              double switch_distance, double detach_distance, double detach_steps, uint8_t* switch_on,
                              int32_t* detach_cnt, double* chosen, hipStream_t s);

}  // namespace mpcgpu
