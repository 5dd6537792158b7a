// mpc_tracker.hpp -- the batched tracker harness on the device and the reference generator of the
// hybrid DQN -> MPC loop (row f2).  One control tick of B robots without the padded 21 KB parameter vector and without a host
// round trip:
//   tracker_window_kernel    get_local_ref_traj (src/mpc_traj_tracker/trajectory_generator.py:206-232): nearest sample of the
//                            global reference inside the window [idx - a, idx + 5a), then N rows from there, tail padded;
//   tracker_assemble_kernel  check_termination_condition (:156-162) + run_step's parameter assembly (:251-275) written DIRECTLY as
//                            the compact workspace record of the solve kernel: prep_problem (mpc_kernels.hpp) reads the same
//                            parameter indices through a source that maps them onto the tracker's own arrays -- the record is
//                            bitwise what prep_kernel makes of the assembled vector;
//   tracker_apply_kernel     the post-solve part of run_step (:325-339): the taken state (one step under input action_steps - 1,
//                            as the reference's loop leaves it), the prediction rolled out from it;
//   fleet_share_kernel       get_other_robot_states (src/scenario_simulator.py:154-163) for every robot of a fleet of worlds; with the
//                            row-list forms of the assembly and apply kernels the Gauss-Seidel tick (include/mpcgpu_fleet.h);
//   rl_reference_kernel      the DQN's proposal: decoded acceleration pair + 20-step rollout with decaying turn rate
//                            (src/pkg_dqn/environment/agent.py:86-145, src/main.py:193-202);
//   hint_switch_kernel       HintSwitcher.switch (src/main_pre.py:27-52) for every robot + the reference it tracks this tick
//                            (ref_traj_filter with decay 1 = the proposal with the original heading column, src/main.py:34-41).
#pragma once
#include "mpc_kernels.hpp"
#include "mpc_tracker_types.hpp"

namespace mpcgpu {

// ---- parameter source of prep_problem: index of the reference's parameter vector (mpc_generator.py:179-188) -> tracker arrays
struct TrackerParams {
    const double* state; const double* last_u; const double* refs;   // this robot's rows
    const double* stc; const double* dyn; const double* other;
    const double* tuning;
    double vref, stc_w, dyn_w;
    int N, r0, c0, os0, od0, qs0, qd0;
    __device__ __forceinline__ double operator[](int i) const {
        if (i >= od0) {
            if (i < qs0) return dyn[i - od0];
            return i < qd0 ? stc_w : dyn_w;
        }
        if (i >= os0) return stc[i - os0];
        if (i >= c0) return other ? other[i - c0] : 0.0;
        if (i >= r0 + 3 * N) return vref;
        if (i >= r0) return refs[i - r0];
        if (i >= 8) return tuning[i - 8];
        if (i >= 6) return last_u[i - 6];
        if (i >= 3) return refs[3 * (N - 1) + i - 3];      // finish state = last row of the reference that is tracked
        return state[i];
    }
};

// one wavefront per problem: termination test, speed rule, compact record.  refs [B][N][3]: the reference every robot tracks.
// ROWS = false is the plain tick (problem b is robot b, a robot that has arrived is frozen); ROWS = true the fleet form of
// mpc_tracker_types.hpp: record j is built from robot rows[j], `arrived` is written and `active` only with stop_when_done.
template <bool ROWS>
__global__ __launch_bounds__(WAVE) void tracker_assemble_kernel(KParams kp, TrackerView t, const double* __restrict__ refs,
                                                                double* __restrict__ ws, int* counts) {
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= (ROWS ? t.n : t.B)) return;
    int b = j;
    if constexpr (ROWS) {
        if (t.rows) {      // rows are the caller's promise (distinct, in range); a bad one is pinned into the arrays, never followed out of them
            b = t.rows[j];
            b = b < 0 ? 0 : (b >= t.B ? t.B - 1 : b);
        }
    }
    const int N = kp.N;
    const double* st = t.states + 3 * b;
    const double* gl = t.goals + 3 * b;
    // check_termination_condition: within 5 cm of the goal in x and y with a last speed below 0.05
    if (lane == 0) {
        const bool near = fabs(st[0] - gl[0]) <= 0.05 && fabs(st[1] - gl[1]) <= 0.05;
        const bool done = near && fabs(t.last_actions[2 * b]) < 0.05;
        if constexpr (ROWS) {
            if (t.arrived) t.arrived[b] = done ? 1 : 0;
            if (done && t.stop_when_done) t.active[b] = 0;
        } else {
            if (done) t.active[b] = 0;
        }
    }
    TrackerParams p;
    p.state = st; p.last_u = t.last_actions + 2 * b; p.refs = refs + (size_t)b * N * 3;
    p.stc = t.stc + (size_t)b * kp.Nstcobs * kp.stcw; p.dyn = t.dyn + (size_t)b * kp.Ndynobs * 6 * N;
    p.other = t.other ? t.other + (size_t)b * 3 * N * kp.Nother : nullptr;
    p.tuning = t.tuning;
    // speed reference: constant, scaled down near the FINAL goal, floored by low_speed (trajectory_generator.py:257-264)
    const double dist = hypot(st[0] - gl[0], st[1] - gl[1]);
    p.vref = dist >= t.base_speed * N * kp.ts ? t.base_speed : fmax(dist / N / kp.ts, t.low_speed);
    p.stc_w = t.stc_weight; p.dyn_w = t.dyn_weight;
    p.N = N; p.r0 = kp.r0; p.c0 = kp.c0; p.os0 = kp.os0; p.od0 = kp.od0; p.qs0 = kp.qs0; p.qd0 = kp.qd0;
    prep_problem(kp, p, ws + (size_t)j * kp.ws_stride, counts, lane);
}

}  // namespace mpcgpu
