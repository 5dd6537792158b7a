// envgpu.hip -- batched DRL environment step for gfx950 (MI355X): C-ABI of include/mpcgpu_env.h.
//
// One wavefront = one environment, grid = B.  The 64 lanes split the padded obstacle / boundary edges (sector and
// ray distances, inside tests), the obstacles (key-frame poses) and the reference-path segments (projection); the
// cross-lane results are DPP minima and ballots, and one lane finishes the scalar bookkeeping (flags, reward,
// observation vectors).  The map record is read once per step, coalesced (lanes stride over consecutive edges).
// Reference semantics: see the file:line list in include/mpcgpu_env.h; CPU restatement: oracle/rl_env_numpy.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "../../include/mpcgpu_collect_fresh.h"
#include "../../include/mpcgpu_eval.h"
#include "dqn_act.hpp"
#include "envgpu_internal.hpp"

namespace envgpu {

constexpr int WAVE = 64;
constexpr int NSEG = 8;      // sectors / rays (rays_reward1.py:20)
constexpr int NCORNER = 3;   // corner samples (rays_reward1.py:18)
constexpr int HDR = 16;
constexpr int SDIM = MPCGPU_ENV_STATE_DOUBLES;
constexpr int MAX_OBST = 31;
constexpr double L_SECTOR = 1000.0;  // ext_obsv_sector_and_ray.py:32

__host__ __device__ inline int anim_doubles(int K) { return 4 + (K + 1) + 3 * K; }

bool layout(const mpcgpu_env_params& p, EnvK& k) {
    if (p.n_path_max < 2 || p.n_path_max > WAVE || p.n_obst_max < 0 || p.n_obst_max > MAX_OBST || p.n_kf_max < 1 ||
        p.n_kf_max > 4 || p.n_edge_max < 1)
        return false;
    k.p = p;
    k.o_cum = HDR;
    k.o_len = k.o_cum + p.n_path_max;
    k.o_xy = k.o_len + p.n_path_max;
    k.o_anim = k.o_xy + 2 * p.n_path_max;
    k.an = anim_doubles(p.n_kf_max);
    k.o_edge = k.o_anim + p.n_obst_max * k.an;
    k.rec = k.o_edge + 5 * p.n_edge_max;
    k.rec += k.rec & 1;
    return true;
}

// ---- wave primitives (DPP: cross-lane operands inside VALU instructions) ------------------------------------------
template <int CTRL>
__device__ __forceinline__ double dpp_fill(double x, double fill) {  // lanes without a source receive `fill`
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(__double2loint(fill), lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(__double2hiint(fill), hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_value(double x, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_min(double x) {  // uniform result
    const double inf = INFINITY;
    x = fmin(x, dpp_fill<0x111>(x, inf));  // row_shr:1
    x = fmin(x, dpp_fill<0x112>(x, inf));
    x = fmin(x, dpp_fill<0x114>(x, inf));
    x = fmin(x, dpp_fill<0x118>(x, inf));
    return fmin(fmin(lane_value(x, 15), lane_value(x, 31)), fmin(lane_value(x, 47), lane_value(x, 63)));
}
__device__ __forceinline__ unsigned wave_xor(unsigned m) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m ^= (unsigned)__shfl_xor((int)m, off, WAVE);
    return m;
}
// fmin / fmax as the single instruction they are: the library forms canonicalise every operand the compiler did not compute itself
// (v_max_f64 x, x, x in front of each), three instructions for one in the clip chains of the edge loop.  v_min_f64 / v_max_f64 return
// the other operand for a quiet NaN exactly as fmin / fmax do (IEEE mode): the same values.
__device__ __forceinline__ double min_raw(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double max_raw(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// 1 / x: hardware estimate + one Newton step (~1e-15 relative; the observations are rounded to float32 afterwards)
__device__ __forceinline__ double fast_rcp(double x) {
    const double r = __builtin_amdgcn_rcp(x);
    return r * (2.0 - x * r);
}
__device__ __forceinline__ double normalize_distance(double d) {  // components/utils.py:10-15
    return 2.0 * fast_rcp(1.0 + exp(-0.2 * d)) - 1.0;   // (the observations are rounded to float32)
}

// cos / sin of j * pi / 8, j = 0..15
__constant__ double DIRC[16] = {1.0, 0.92387953251128673848, 0.70710678118654757274, 0.38268343236508978178,
                                0.0, -0.38268343236508978178, -0.70710678118654757274, -0.92387953251128673848,
                                -1.0, -0.92387953251128673848, -0.70710678118654757274, -0.38268343236508978178,
                                0.0, 0.38268343236508978178, 0.70710678118654757274, 0.92387953251128673848};
__constant__ double DIRS[16] = {0.0, 0.38268343236508978178, 0.70710678118654757274, 0.92387953251128673848,
                                1.0, 0.92387953251128673848, 0.70710678118654757274, 0.38268343236508978178,
                                0.0, -0.38268343236508978178, -0.70710678118654757274, -0.92387953251128673848,
                                -1.0, -0.92387953251128673848, -0.70710678118654757274, -0.38268343236508978178};

// COLLECT (include/mpcgpu_collect.h): what the step kernel gets on top of its own arguments, and nothing without it
struct CollectK {
    const float* theta;
    float* buf_obs; float* buf_next_obs; int64_t* buf_actions; float* buf_rewards; float* buf_dones;
    double* ep_return;
    int32_t* actions; uint8_t* done; uint8_t* success; double* episode_return;   // [T][B], each may be NULL
    mpcgpu_collect_params p;
};
struct NoCollect {};
// EVAL (include/mpcgpu_eval.h): the policy, the progress vectors and the [B][E] outputs
struct EvalK {
    const float* theta;
    int32_t* episodes_done; int64_t* steps_done; double* ep_return; int32_t* ep_length;
    double* returns; int32_t* lengths; uint8_t* outcome;
    mpcgpu_eval_params p;
};
__device__ __forceinline__ int collect_steps(const CollectK& co) { return co.p.T; }
__device__ __forceinline__ int collect_steps(const EvalK& co) { return co.p.max_steps; }
__device__ __forceinline__ int collect_steps(const NoCollect&) { return 1; }
__device__ __forceinline__ int eval_episodes(const EvalK& co) { return co.p.episodes; }
template <class K> __device__ __forceinline__ int eval_episodes(const K&) { return 0; }
__device__ __forceinline__ dqnact::ActLds& collect_lds() {   // LDS of the instantiations that call it only
    __shared__ dqnact::ActLds lds;
    return lds;
}

// FRESH (include/mpcgpu_map.h): rec_all is a [2][B][rec] table, row b steps on table which[b], and an episode that ends while
// spare_ready[b] is set starts its next episode on the other table.  Everything FRESH adds sits under `if constexpr`.
// COLLECT (include/mpcgpu_collect.h): the body below runs co.p.T times; before each step the wavefront chooses its action from
// the observation the previous step left in global memory, after it the transition goes into the ring.  Every trip reads the
// state and writes it back exactly as a launch of its own does, so T trips are T launches; everything COLLECT adds sits under
// `if constexpr`, and without it the loop is `do { } while (false)`.
// EVAL (include/mpcgpu_eval.h): the same trips with one eps, the serial taken from steps_done[b], and the episode bookkeeping in
// place of the ring; a parked row returns before it reads anything else, and the loop ends with the row's E-th episode or after
// co.p.max_steps trips, whichever comes first -- both bounds are arguments, no trip waits for anything.  ACTS = COLLECT or EVAL.
// FRESH and COLLECT (include/mpcgpu_collect_fresh.h): rec, n_path, n_obst, n_edge, gx and gy are carried from trip to trip and change
// in the turnover block alone, which reads which[b] and spare_ready[b] from global memory in every trip -- lane 0 may have rewritten
// them in an earlier trip of this launch; the workgroup fence and the barrier in front of the ring stores stand between that store and
// these reads.  One spare per row: the first ending of a row in a launch takes it, every later one resets on the map the row is on
// and counts stale[b], as T launches without a refill between them do.
template <bool FRESH, bool COLLECT = false, bool EVAL = false>
__global__ __launch_bounds__(WAVE, 4) void env_step_kernel(EnvK k, const double* __restrict__ rec_all, double* state_all,
                                                        const int32_t* __restrict__ action, EnvOut out, int B, EnvFresh fr,
                                                        std::conditional_t<EVAL, EvalK, std::conditional_t<COLLECT, CollectK, NoCollect>> co) {
    static_assert(!(EVAL && (COLLECT || FRESH)), "the evaluation mode is built for one record table and has no ring");
    constexpr bool ACTS = COLLECT || EVAL;
    float* const obs_int = out.obs_int;
    float* const obs_ext = out.obs_ext;
    double* const reward = out.reward;
    uint8_t* const terminated = out.terminated;
    __shared__ double pose[MAX_OBST + 1][4];
    __shared__ __attribute__((aligned(16))) double dirs[16][2];
    const int b = blockIdx.x;
    if (b >= B) return;
    int ep_done = 0, ep_len = 0;
    if constexpr (EVAL) {
        ep_done = co.episodes_done[b];
        // parked: the only word of the row this wavefront touches (a negative count, which no launch leaves, parks the row too:
        // it would index in front of the row's slots)
        if ((unsigned)ep_done >= (unsigned)co.p.episodes) return;
    }
    const int lane = threadIdx.x;
    const double* rec = rec_all + (size_t)b * k.rec;
    if constexpr (FRESH) rec = rec_all + ((size_t)fr.which[b] * B + b) * k.rec;
    double* st = state_all + (size_t)b * SDIM;
    const mpcgpu_env_params& P = k.p;
    int n_path = (int)rec[0], n_obst = (int)rec[1], n_edge = (int)rec[2];   // (not const: FRESH re-reads them with the record)
    double gx = rec[3], gy = rec[4];
    int t = 0, chosen = 0;
    double ep_ret = 0.0;
    uint64_t steps_made = 0;
    if constexpr (ACTS) {
        dqnact::stage_theta(collect_lds(), co.theta, lane, WAVE);
        ep_ret = co.ep_return[b];
    }
    if constexpr (EVAL) {
        ep_len = co.ep_length[b];
        steps_made = (uint64_t)co.steps_done[b];
    }
    do {
    if constexpr (ACTS) {
        // ---- the action (include/mpcgpu_collect.h): the flat observation, external then internal, into LDS.  From the second trip
        //      on it is what this workgroup wrote: the fence and the barrier in front of the ring stores below cover these reads too
        dqnact::ActLds& L = collect_lds();
        __syncthreads();   // the ring stores of the previous trip have read L.x
        if (lane < MPCGPU_ENV_EXTERNAL_OBS) L.x[lane] = obs_ext[(size_t)b * MPCGPU_ENV_EXTERNAL_OBS + lane];
        else if (lane < dqnact::OBS) L.x[lane] = obs_int[(size_t)b * MPCGPU_ENV_INTERNAL_OBS + lane - MPCGPU_ENV_EXTERNAL_OBS];
        __syncthreads();
        if constexpr (EVAL) chosen = dqnact::act(L, lane, co.p.eps, co.p.seed, co.p.serial0 + steps_made, (uint64_t)b);
        else chosen = dqnact::act(L, lane, co.p.eps[t], co.p.seed, co.p.serial0 + (uint64_t)t, (uint64_t)b);
    }
    double x = st[0], y = st[1], th = st[2], v = st[3], w = st[4], clock = st[5];
    double last_prog = st[6], steps = st[25];
    int flags = (int)st[7];
    bool act = action != nullptr;
    double ts = P.time_step;
    if constexpr (ACTS) {
        act = true;
        // The time step must not be a loop invariant: the compiler would hoist products such as ts * P.angacc_max out of the loop over
        // t, and a product formed up there is no longer fused into the addition it feeds (-ffp-contract=fast fuses within a block),
        // so a trip would round differently from a launch of its own.  Behind the empty barrier every trip computes them anew.
        asm volatile("" : "+s"(ts));
    }

    // ---- obstacles' clock and the robot (environment.py:199-203, agent.py:97-139); every lane keeps the same copy
    if (act) {
        int a;
        if constexpr (ACTS) a = chosen;
        else a = action[b];
        clock += ts;
        const int row = a / 3, col = a % 3;
        if (row == 0) v += ts * P.acc_max;
        if (row == 2) v += ts * P.acc_min;
        if (col == 0) w += ts * P.angacc_max;
        if (col == 2) w += ts * P.angacc_min;
        if (v > P.speed_max) v = P.speed_max;
        if (v < P.speed_min) v = P.speed_min;
        if (w > P.angvel_max) w = P.angvel_max;
        if (w < P.angvel_min) w = P.angvel_min;
        th += ts * w;
    }
    // cos / sin of the heading once: the kinematic step and the observation pass use the same angle
    double cth0, sth0;
    sincos(th, &sth0, &cth0);
    if (act) {
        x += ts * v * cth0;
        y += ts * v * sth0;
    }
    // Pass 0 is the step itself.  With in-kernel auto-reset (out.max_steps > 0) an environment whose episode ended is
    // put back to its start state and observed again in pass 1 -- no host round trip, no second launch.
    auto run_pass = [&](const int pass, const double cth, const double sth) -> bool {   // returns true when the episode ended and pass 1 is wanted

    // ---- key-frame pose of obstacle `lane` (obstacle.py:71-88): (x, y, cos rot, sin rot) -> LDS
    if (lane < n_obst) {
        const double* an = rec + k.o_anim + lane * k.an;
        const int kind = (int)an[0], nk = (int)an[2];
        const double* tsv = an + 4;
        const double* kf = an + 4 + (P.n_kf_max + 1);
        const double tm = fmod(clock + an[1], an[3]);
        double px = kf[3 * (nk - 1)], py = kf[3 * (nk - 1) + 1], rot = kf[3 * (nk - 1) + 2];
        double t = 0.0;
        bool found = false;
        for (int i = 0; i < nk; ++i) {
            t += tsv[i];
            if (!found && t <= tm && tm < t + tsv[i + 1]) {
                const double xx = (tm - t) * fast_rcp(tsv[i + 1]);
                const double alpha = kind == 1 ? (1.0 - cos(xx * M_PI)) / 2.0 : xx;
                const double* k0 = kf + 3 * i;
                const double* k1 = kf + 3 * ((i + 1) % nk);
                px = k0[0] * (1.0 - alpha) + k1[0] * alpha;
                py = k0[1] * (1.0 - alpha) + k1[1] * alpha;
                rot = k0[2] * (1.0 - alpha) + k1[2] * alpha;
                found = true;
            }
        }
        double crot, srot;
        sincos(rot, &srot, &crot);
        pose[lane][0] = px; pose[lane][1] = py; pose[lane][2] = crot; pose[lane][3] = srot;
    }
    __syncthreads();

    // ---- the 16 directions theta + j pi/8 (even j = ray / sector centre, odd j = sector borders) live in LDS: every
    //      lane reads the same entry (a broadcast), which keeps 64 VGPRs free for a fourth resident wavefront per SIMD
    if (lane < 16) {
        dirs[lane][0] = cth * DIRC[lane] - sth * DIRS[lane];
        dirs[lane][1] = sth * DIRC[lane] + cth * DIRS[lane];
    }
    __syncthreads();

    // ---- edges: closest point of (edge within sector i), first hit of ray i, crossing parity per outline
    double sec[NSEG], ray[NSEG];
#pragma unroll
    for (int i = 0; i < NSEG; ++i) { sec[i] = INFINITY; ray[i] = INFINITY; }
    unsigned mask = 0u;  // bit 0: padded boundary, bit j+1: obstacle j -- set when the robot is inside that outline
    for (int e = lane; e < n_edge; e += WAVE) {
        const double* ed = rec + k.o_edge + 5 * e;
        double x0 = ed[0], y0 = ed[1], x1 = ed[2], y1 = ed[3];
        const int owner = (int)ed[4];
        if (owner < -1) continue;
        if (owner >= 0) {  // obstacle.py:174-188: position + R * nodes
            const double ox = pose[owner][0], oy = pose[owner][1], c = pose[owner][2], s = pose[owner][3];
            const double a0 = ox + c * x0 - s * y0, b0 = oy + s * x0 + c * y0;
            const double a1 = ox + c * x1 - s * y1, b1 = oy + s * x1 + c * y1;
            x0 = a0; y0 = b0; x1 = a1; y1 = b1;
        }
        const double Px = x0 - x, Py = y0 - y, Qx = x1 - x, Qy = y1 - y;
        const double Ex = Qx - Px, Ey = Qy - Py;
        if ((Py > 0.0) != (Qy > 0.0)) {  // even-odd rule along +x from the robot
            const double xi = Ex * (-Py) * fast_rcp(Ey) + Px;
            if (xi > 0.0) mask ^= 1u << (owner + 1);
        }
        const double ee = Ex * Ex + Ey * Ey, pe = Px * Ex + Py * Ey;
        const double t_free = ee > 0.0 ? -pe * fast_rcp(ee) : 0.0;
        // Line j through the robot with direction d_j meets the edge's carrier at parameter tc; g0 / g1 are the signed
        // distances (x |d| = 1) of P and of the edge direction from that line.  Odd lines are sector borders (each
        // shared by two neighbouring sectors), even lines carry the rays.  The lines
        // are walked in order and only the previous border is kept (registers: residency, see __launch_bounds__).
        struct Line { double g0, g1, tc, dx, dy; };
        asm volatile("" ::: "memory");  // keep the direction reads inside the loop (hoisted, they pin 64 VGPRs again)
        auto line = [&](int j) {
            Line l;
            l.dx = dirs[j][0]; l.dy = dirs[j][1];
            l.g0 = l.dx * Py - l.dy * Px;
            l.g1 = l.dx * Ey - l.dy * Ex;
            l.tc = -l.g0 * fast_rcp(l.g1);   // inf / nan when the edge is parallel to the line: handled below
            return l;
        };
        // Line j + 8 is line j walked the other way: g0 and g1 change sign, tc stays.  Sector i and the sector opposite to it (i + 4)
        // share their two border carriers, ray i and ray i + 4 their carrier: nine line evaluations per edge instead of sixteen.
        auto sector = [&](int i, const Line& lo, const Line& up, double sgn) {
            // wedge = {cross(d_lower, X) >= 0} and {cross(d_upper, X) <= 0}: clip the edge's parameter range [0, 1]
            const double lg1 = sgn * lo.g1, lg0 = sgn * lo.g0, ug1 = sgn * up.g1, ug0 = sgn * up.g0;
            double t0 = 0.0, t1 = 1.0;
            bool empty = false;
            if (lg1 > 0.0) t0 = max_raw(t0, lo.tc);
            else if (lg1 < 0.0) t1 = min_raw(t1, lo.tc);
            else if (lg0 < 0.0) empty = true;
            if (ug1 < 0.0) t0 = max_raw(t0, up.tc);
            else if (ug1 > 0.0) t1 = min_raw(t1, up.tc);
            else if (ug0 > 0.0) empty = true;
            if (!empty && t0 <= t1) {
                const double tt = min_raw(max_raw(t_free, t0), t1);
                const double cx = Px + tt * Ex, cy = Py + tt * Ey;
                sec[i] = min_raw(sec[i], cx * cx + cy * cy);  // squared; the root is taken once, after the reduction
            }
        };
        auto rayhit = [&](int i, const Line& ce, double sgn) {
            // ray i: P + t E = s d with t = tc of the centre line; s follows from the projection on d (|d| = 1)
            if (ce.g1 != 0.0) {
                const double t = ce.tc;
                const double sd = sgn * ((Px + t * Ex) * ce.dx + (Py + t * Ey) * ce.dy);
                if (sd >= 0.0 && t >= 0.0 && t <= 1.0 && sd <= L_SECTOR) ray[i] = min_raw(ray[i], sd);
            }
        };
        Line lower = line(7);   // line 15 = line 7 reversed: the lower border of sector 0
#pragma unroll
        for (int i = 0; i < NSEG / 2; ++i) {
            const Line centre = line(2 * i);
            const Line upper = line(2 * i + 1);
            // sector i lies between lines 2i - 1 and 2i + 1; for i = 0 the lower border is line 15 = -line 7
            {   // sector i
                Line lo = lower;
                if (i == 0) { lo.g0 = -lo.g0; lo.g1 = -lo.g1; }
                sector(i, lo, upper, 1.0);
                // the opposite sector i + 4: borders 2i + 7 = -(2i - 1) ... and 2i + 9 = -(2i + 1)
                sector(i + NSEG / 2, lo, upper, -1.0);
            }
            rayhit(i, centre, 1.0);
            rayhit(i + NSEG / 2, centre, -1.0);
            lower = upper;
        }
    }
    mask = wave_xor(mask);
    const bool in_obstacle = (mask & ~1u) != 0u;
    // 16 minima over 64 lanes as ONE butterfly: every exchange halves the number of values a lane still carries
    // (8 + 4 + 2 + 1 + 1 + 1 = 17 exchanges instead of 16 x 6).  Afterwards lane l holds value number
    // 8 b5 + 4 b4 + 2 b3 + b2 (b_k = bit k of l); values 0..7 = squared sector distances, 8..15 = ray distances.
    double red;
    {
        double v8[8], v4[4], v2[2];
        const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8, h2 = lane & 4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double keep = h5 ? ray[i] : sec[i], send = h5 ? sec[i] : ray[i];
            v8[i] = min_raw(keep, __shfl_xor(send, 32, WAVE));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double keep = h4 ? v8[4 + i] : v8[i], send = h4 ? v8[i] : v8[4 + i];
            v4[i] = min_raw(keep, __shfl_xor(send, 16, WAVE));
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const double keep = h3 ? v4[2 + i] : v4[i], send = h3 ? v4[i] : v4[2 + i];
            v2[i] = min_raw(keep, __shfl_xor(send, 8, WAVE));
        }
        const double keep = h2 ? v2[1] : v2[0], send = h2 ? v2[0] : v2[1];
        red = min_raw(keep, __shfl_xor(send, 4, WAVE));
        red = min_raw(red, __shfl_xor(red, 2, WAVE));
        red = min_raw(red, __shfl_xor(red, 1, WAVE));
    }
    // ---- external observation with one-step memory (ext_obsv_sector_and_ray.py:66-74): 16 lanes, one entry each
    if ((lane & 3) == 0) {
        const int idx = ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
        // inside a padded obstacle the robot itself belongs to sector ∩ obstacle: every distance is 0
        const double d = in_obstacle ? 0.0 : (idx < NSEG ? sqrt(red) : red);
        const float o = (float)normalize_distance(d);
        if (obs_ext) {   // NULL for the image variant, which keeps only the memory in the state
            float* oe = obs_ext + (size_t)b * MPCGPU_ENV_EXTERNAL_OBS;
            oe[idx] = o;
            oe[2 * NSEG + idx] = (float)st[8 + idx];
        }
        st[8 + idx] = (double)o;
    }

    // ---- path progress = LineString.project: first closest segment (environment.py:118)
    const double* cum = rec + k.o_cum;
    const double* len = rec + k.o_len;
    const double* pxy = rec + k.o_xy;
    double dist = INFINITY, tproj = 0.0, cpx = 0.0, cpy = 0.0;
    if (lane < n_path - 1) {
        const double ax = pxy[2 * lane], ay = pxy[2 * lane + 1];
        const double ex = pxy[2 * lane + 2] - ax, ey = pxy[2 * lane + 3] - ay;
        const double den = ex * ex + ey * ey;
        double t = den == 0.0 ? 0.0 : ((x - ax) * ex + (y - ay) * ey) * fast_rcp(den);
        t = fmin(1.0, fmax(0.0, t));
        cpx = ax + t * ex; cpy = ay + t * ey;
        tproj = t;
        dist = sqrt((x - cpx) * (x - cpx) + (y - cpy) * (y - cpy));
    }
    const double cte = wave_min(dist);
    const int iseg = __ffsll((long long)__ballot(dist == cte)) - 1;
    const double progress = cum[iseg] + lane_value(tproj, iseg) * len[iseg];
    cpx = lane_value(cpx, iseg); cpy = lane_value(cpy, iseg);
    // sample point at progress + offset (LineString.interpolate, clamped to the line)
    double spx = cpx, spy = cpy;
    if (P.sample_offset != 0.0) {
        const double s = progress + P.sample_offset;
        const double total = cum[n_path - 1];
        if (s <= 0.0) { spx = pxy[0]; spy = pxy[1]; }
        else if (s >= total) { spx = pxy[2 * (n_path - 1)]; spy = pxy[2 * (n_path - 1) + 1]; }
        else {
            const unsigned long long bal = __ballot(lane < n_path - 1 && s < cum[lane < n_path - 1 ? lane + 1 : 0]);
            const int i = bal ? __ffsll((long long)bal) - 1 : n_path - 2;
            const double t = (s - cum[i]) * fast_rcp(len[i]);
            spx = pxy[2 * i] + t * (pxy[2 * i + 2] - pxy[2 * i]);
            spy = pxy[2 * i + 1] + t * (pxy[2 * i + 3] - pxy[2 * i + 1]);
        }
    }
    // first node whose cumulative length reaches the progress (int_obsv_reference_path_corner.py:29-33)
    const unsigned long long reach = __ballot(lane < n_path && cum[lane < n_path ? lane : 0] >= progress);
    int icorner = reach ? __ffsll((long long)reach) - 1 : n_path - 1;

    // ---- path observations (components/int_obsv_reference_path_{sample,corner}.py): lanes 0..3, one point each
    float* oi = obs_int + (size_t)b * MPCGPU_ENV_INTERNAL_OBS;
    if (lane < 1 + NCORNER) {
        double qx = spx, qy = spy;
        if (lane > 0) {
            int ic = icorner + lane - 1;
            if (ic > n_path - 1) ic = n_path - 1;
            qx = pxy[2 * ic]; qy = pxy[2 * ic + 1];
        }
        // cos / sin of (bearing - theta) and the normalised distance; atan2(0, 0) = 0 for a coincident point
        const double ddx = qx - x, ddy = qy - y;
        const double d = sqrt(ddx * ddx + ddy * ddy);
        double cr = cth, sr = -sth;
        if (d > 0.0) { const double id = fast_rcp(d); cr = (ddx * cth + ddy * sth) * id; sr = (ddy * cth - ddx * sth) * id; }
        float* o = oi + 2 + 3 * lane;
        o[0] = (float)cr; o[1] = (float)sr; o[2] = (float)normalize_distance(d);
    }
    // ---- status flags, sticky (environment.py:113-116); uniform, every lane keeps a copy
    if (in_obstacle) flags |= 1;
    if (!(mask & 1u)) flags |= 2;
    if (sqrt((gx - x) * (gx - x) + (gy - y) * (gy - y)) < P.radius) flags |= 4;
    const bool collided = (flags & 3) != 0, reached = (flags & 4) != 0;
    if (act) { steps += 1.0; }
    const bool timeout = out.max_steps > 0 && steps >= (double)out.max_steps && !(collided || reached);

    if (lane == 0) {
        // ---- speed and angular velocity (components/int_obsv_speed.py, int_obsv_angular_velocity.py)
        oi[0] = (float)(2.0 * (v - P.speed_min) * fast_rcp(P.speed_max - P.speed_min) - 1.0);
        // the reference normalises the angular velocity with the angular ACCELERATION limits (int_obsv_angular_velocity.py:13-19)
        oi[1] = (float)(2.0 * (w - P.angacc_min) * fast_rcp(P.angacc_max - P.angacc_min) - 1.0);
        if (pass == 0) {
            // ---- reward R1 (rays_reward1.py:26-39; summed in component order)
            if (act) {
                double r = collided ? -P.collision_factor : 0.0;
                r += -ts * P.cross_track_factor * cte * cte;
                r += reached ? P.reach_goal_factor : 0.0;
                const double err = copysign(1.0, P.reference_speed) * (v - P.reference_speed);
                r += -ts * P.excessive_speed_factor * fmax(0.0, err);
                r += P.path_progress_factor * (progress - last_prog);
                if (reward) reward[b] = r;
            } else if (reward) {
                reward[b] = 0.0;
            }
            if (terminated) terminated[b] = (collided || reached) ? 1 : 0;
            if (out.truncated) out.truncated[b] = timeout ? 1 : 0;
            st[26] = (double)flags;   // flags of this step, still readable after an in-kernel reset
            if (out.pre_reset) {      // image variant: what the terminal image is drawn from
                double* pr = out.pre_reset + (size_t)b * IMG_STATE + IMG_PRE;
                pr[0] = x; pr[1] = y; pr[2] = th; pr[3] = clock;
                pr[4] = (out.max_steps > 0 && act && (collided || reached || timeout)) ? 1.0 : 0.0;
                // the table the row was on at entry (which[b] is flipped further down, after this pass): the record the
                // image kernel draws the terminal image from
                if constexpr (FRESH) pr[5] = (double)fr.which[b];
            }
        }
        st[0] = x; st[1] = y; st[2] = th; st[3] = v; st[4] = w; st[5] = clock;
        st[6] = (act || pass == 1) ? (pass == 1 ? 0.0 : progress) : last_prog;
        st[7] = (double)flags;
        st[24] = progress;
        st[25] = steps;
    }
    return pass == 0 && out.max_steps > 0 && act && (collided || reached || timeout);
    };  // run_pass

    if (run_pass(0, cth0, sth0)) {
    // ---- the episode ended: keep its last observation, go back to the start state (environment.py:166-186) and
    //      observe once more.  The observation memory (st[8..23]) is not cleared -- the reference's component keeps it.
    __threadfence();
    __syncthreads();
    if (out.term_int && lane < MPCGPU_ENV_INTERNAL_OBS)
        out.term_int[(size_t)b * MPCGPU_ENV_INTERNAL_OBS + lane] = obs_int[(size_t)b * MPCGPU_ENV_INTERNAL_OBS + lane];
    if (out.term_ext && lane < MPCGPU_ENV_EXTERNAL_OBS)
        out.term_ext[(size_t)b * MPCGPU_ENV_EXTERNAL_OBS + lane] = obs_ext[(size_t)b * MPCGPU_ENV_EXTERNAL_OBS + lane];
    __syncthreads();
    if constexpr (FRESH) {
        // every lane reads the row's two words before lane 0 rewrites them; the workgroup owns the row, so no atomics
        const int cur = fr.which[b], ready = fr.spare_ready[b];
        __syncthreads();
        if (ready) {
            rec = rec_all + ((size_t)(cur ^ 1) * B + b) * k.rec;
            n_path = (int)rec[0]; n_obst = (int)rec[1]; n_edge = (int)rec[2];
            gx = rec[3]; gy = rec[4];
            if (lane == 0) { fr.which[b] = cur ^ 1; fr.spare_ready[b] = 0; fr.loaded[b] += 1; }
        } else if (lane == 0) {
            fr.stale[b] += 1;
        }
    }
    x = rec[5]; y = rec[6]; th = rec[7]; v = rec[8]; w = rec[9];
    clock = 0.0; flags = 0; steps = 0.0; last_prog = 0.0; act = false;
    sincos(th, &sth0, &cth0);
    run_pass(1, cth0, sth0);
    }
    if constexpr (COLLECT) {
        // ---- the transition (dqn_train.ReplayBuffer.add as DqnLearner.learn calls it) and the episode return, read back from
        //      what the step wrote: the same words the host-driven round reads.  Writers and readers are lanes of this one
        //      workgroup, so a workgroup-scope fence orders them; an agent-scope __threadfence() here, once per step in every
        //      wavefront, writes back and invalidates L2 lines across the whole device and cost most of the launch
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __syncthreads();
        const dqnact::ActLds& L = collect_lds();
        const bool term = terminated[b] != 0, ended = term || out.truncated[b] != 0;
        const double r = reward[b];
        const size_t slot = (size_t)t * B + b;
        const size_t row = (size_t)(((uint64_t)co.p.pos0 + slot) % (uint64_t)co.p.capacity);
        if (lane < dqnact::OBS) {
            const bool ext = lane < MPCGPU_ENV_EXTERNAL_OBS;
            const float* src = ext ? (ended ? out.term_ext : obs_ext) + (size_t)b * MPCGPU_ENV_EXTERNAL_OBS + lane
                                   : (ended ? out.term_int : obs_int) + (size_t)b * MPCGPU_ENV_INTERNAL_OBS + lane - MPCGPU_ENV_EXTERNAL_OBS;
            co.buf_obs[row * dqnact::OBS + lane] = L.x[lane];
            co.buf_next_obs[row * dqnact::OBS + lane] = *src;
        }
        ep_ret = ep_ret + r;
        if (lane == 0) {
            co.buf_actions[row] = chosen;
            co.buf_rewards[row] = (float)r;
            co.buf_dones[row] = term ? 1.0f : 0.0f;
            if (co.actions) co.actions[slot] = chosen;
            if (co.done) co.done[slot] = ended ? 1 : 0;
            if (co.success) co.success[slot] = ((int)st[26] & 4) ? 1 : 0;
            if (ended && co.episode_return) co.episode_return[slot] = ep_ret;
        }
        if (ended) ep_ret = 0.0;
    }
    if constexpr (EVAL) {
        // ---- the episode bookkeeping (include/mpcgpu_eval.h), read back from what the step wrote behind the same workgroup-scope
        //      fence and barrier as the ring stores above: lane 0 wrote these words, every lane reads them and keeps the same copy
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __syncthreads();
        const bool trunc = out.truncated[b] != 0, ended = terminated[b] != 0 || trunc;
        ep_ret = ep_ret + reward[b];
        ep_len += 1;
        steps_made += 1;
        if (ended) {
            if (lane == 0) {
                const size_t slot = (size_t)b * co.p.episodes + ep_done;
                co.returns[slot] = ep_ret;
                co.lengths[slot] = ep_len;
                co.outcome[slot] = (uint8_t)(((int)st[26] & 7) | (trunc ? 8 : 0));
            }
            ep_ret = 0.0; ep_len = 0; ep_done += 1;
        }
    }
    } while (ACTS && ++t < collect_steps(co) && !(EVAL && ep_done >= eval_episodes(co)));
    if constexpr (ACTS) {
        if (lane == 0) co.ep_return[b] = ep_ret;
    }
    if constexpr (EVAL) {
        if (lane == 0) { co.episodes_done[b] = ep_done; co.steps_done[b] = (int64_t)steps_made; co.ep_length[b] = ep_len; }
    }
}

// the action rule alone (mpcgpu_collect_act_dev): one wavefront per workgroup, the rows dealt out over the grid
__global__ __launch_bounds__(WAVE) void collect_act_kernel(const float* __restrict__ theta, const float* __restrict__ obs_ext,
                                                          const float* __restrict__ obs_int, int B, double eps, uint64_t seed,
                                                          uint64_t serial, int32_t* actions, float* q) {
    __shared__ dqnact::ActLds L;
    const int lane = threadIdx.x;
    dqnact::stage_theta(L, theta, lane, WAVE);
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        __syncthreads();
        if (lane < MPCGPU_ENV_EXTERNAL_OBS) L.x[lane] = obs_ext[(size_t)b * MPCGPU_ENV_EXTERNAL_OBS + lane];
        else if (lane < dqnact::OBS) L.x[lane] = obs_int[(size_t)b * MPCGPU_ENV_INTERNAL_OBS + lane - MPCGPU_ENV_EXTERNAL_OBS];
        __syncthreads();
        const int a = dqnact::act(L, lane, eps, seed, serial, (uint64_t)b);
        if (lane == 0) actions[b] = a;
        if (q && lane < dqnact::ACT) q[(size_t)b * dqnact::ACT + lane] = L.q[lane];
    }
}

thread_local abi::ErrorSlot g_err;

// what launch_step refuses in the params, or NULL; fills k
const char* params_error(const mpcgpu_env_params* params, EnvK& k) {
    if (!params || !layout(*params, k)) return BAD_PARAMS;
    if (params->num_segments != NSEG || params->corner_samples != NCORNER)
        return "only num_segments = 8 and corner_samples = 3 are built (rays_reward1.py:18-20)";
    return nullptr;
}

int autoreset_args(const int32_t* action, int32_t max_episode_steps, bool images) {
    if (!action)
        return fail(images ? "auto-reset needs actions (use mpcgpu_env_step_imgs_dev to observe)"
                           : "auto-reset needs actions (use mpcgpu_env_step_dev to observe)");
    if (max_episode_steps <= 0) return fail("max_episode_steps must be positive");
    return 0;
}

int fresh_args(const EnvFresh& fr, const char* also_bad, const int32_t* action, EnvOut& out) {
    if (!fr.which || !fr.spare_ready || !fr.loaded || !fr.stale) return fail("null pointer (which / spare_ready / loaded / stale)");
    if (also_bad) return fail(also_bad);
    if (out.max_steps < 0) return fail("max_episode_steps must not be negative");
    if (out.max_steps > 0 && !action) return fail("auto-reset needs actions (max_episode_steps = 0 observes)");
    if (out.max_steps > 0 && !out.truncated) return fail("null pointer (truncated)");
    if (out.max_steps == 0) {
        out.truncated = nullptr; out.term_int = out.term_ext = nullptr; out.pre_reset = nullptr;
    }
    return 0;
}

int launch_step(int32_t device, const mpcgpu_env_params* params, int32_t B, const double* records, double* state,
                const int32_t* action, EnvOut out, bool need_ext, void* stream, const EnvFresh* fresh) {
    EnvK k;
    if (const char* bad = params_error(params, k)) return fail(bad);
    if (B < 0 || !records || !state || !out.obs_int || (need_ext && !out.obs_ext)) return fail("null pointer / negative batch");
    if (B == 0) return 0;
    if (abi::on_device(g_err, device)) return -1;
    if (fresh)
        hipLaunchKernelGGL(env_step_kernel<true>, dim3(B), dim3(WAVE), 0, (hipStream_t)stream, k, records, state, action, out,
                           (int)B, *fresh, NoCollect{});
    else
        hipLaunchKernelGGL(env_step_kernel<false>, dim3(B), dim3(WAVE), 0, (hipStream_t)stream, k, records, state, action, out,
                           (int)B, EnvFresh{}, NoCollect{});
    return abi::launched(g_err, "env_step_kernel launch");
}

thread_local abi::ErrorSlot g_collect_err;   // mpcgpu_collect_last_error
int collect_fail(const char* what) { return g_collect_err.fail(what); }
bool eps_ok(double eps) { return eps >= 0.0 && eps <= 1.0; }   // false for NaN

// the argument checks and the launch of the two T-step entries: mpcgpu_collect_rays_dev (fresh = NULL, records [B][rec]) and
// mpcgpu_collect_rays_fresh_dev (records [2][B][rec]), each with the error slot of its own.  `co` comes in without its params
int launch_collect(abi::ErrorSlot& err, int32_t device, const mpcgpu_env_params* params, int32_t B, const double* records,
                   double* state, const EnvOut& out, CollectK co, const mpcgpu_collect_params* collect, void* stream,
                   const EnvFresh* fresh) {
    if (fresh && (!fresh->which || !fresh->spare_ready || !fresh->loaded || !fresh->stale))
        return err.fail("null pointer (which / spare_ready / loaded / stale)");
    EnvK k;
    if (const char* bad = params_error(params, k)) return err.fail(bad);
    if (!records || !state || !out.obs_int || !out.obs_ext || !out.reward || !out.terminated || !out.truncated || !out.term_int ||
        !out.term_ext)
        return err.fail("null pointer (an environment tensor)");
    if (!co.theta || !collect || !co.buf_obs || !co.buf_next_obs || !co.buf_actions || !co.buf_rewards || !co.buf_dones ||
        !co.ep_return)
        return err.fail("null pointer (theta / collect / ring / ep_return)");
    if (B < 0) return err.fail("negative batch");
    if (out.max_steps <= 0) return err.fail("max_episode_steps must be positive");
    if (collect->T < 1 || collect->T > MPCGPU_COLLECT_MAX_STEPS) return err.fail("1 <= T <= 64 (MPCGPU_COLLECT_MAX_STEPS)");
    if (collect->capacity < 1 || collect->pos0 < 0 || collect->pos0 >= collect->capacity)
        return err.fail("capacity >= 1 and 0 <= pos0 < capacity");
    if ((int64_t)collect->T * B > collect->capacity)
        return err.fail("T * B must not exceed capacity: the rows of one launch would overwrite each other");
    for (int t = 0; t < collect->T; ++t)
        if (!eps_ok(collect->eps[t])) return err.fail("every eps[t], t < T, must lie in [0, 1]");
    if (B == 0) return 0;
    if (abi::on_device(err, device)) return -1;
    co.p = *collect;
    if (fresh)
        hipLaunchKernelGGL((env_step_kernel<true, true>), dim3(B), dim3(WAVE), 0, (hipStream_t)stream, k, records, state,
                           (const int32_t*)nullptr, out, (int)B, *fresh, co);
    else
        hipLaunchKernelGGL((env_step_kernel<false, true>), dim3(B), dim3(WAVE), 0, (hipStream_t)stream, k, records, state,
                           (const int32_t*)nullptr, out, (int)B, EnvFresh{}, co);
    return abi::launched(err, "env_step_kernel launch");
}
thread_local abi::ErrorSlot g_collect_fresh_err;   // mpcgpu_collect_fresh_last_error
thread_local abi::ErrorSlot g_eval_err;            // mpcgpu_eval_last_error

}  // namespace envgpu

extern "C" {

int32_t mpcgpu_env_record_doubles(const mpcgpu_env_params* params) {
    envgpu::EnvK k;
    if (!params || !envgpu::layout(*params, k)) return envgpu::fail(envgpu::BAD_PARAMS);
    return k.rec;
}

int32_t mpcgpu_env_step_dev(int32_t device, const mpcgpu_env_params* params, int32_t B, const double* records,
                            double* state, const int32_t* action, float* obs_internal, float* obs_external,
                            double* reward, uint8_t* terminated, void* stream) {
    envgpu::EnvOut out{obs_internal, obs_external, reward, terminated, nullptr, nullptr, nullptr, 0, nullptr};
    return envgpu::launch_step(device, params, B, records, state, action, out, true, stream);
}

int32_t mpcgpu_env_step_autoreset_dev(int32_t device, const mpcgpu_env_params* params, int32_t B, const double* records,
                                      double* state, const int32_t* action, float* obs_internal, float* obs_external,
                                      double* reward, uint8_t* terminated, uint8_t* truncated, float* terminal_obs_internal,
                                      float* terminal_obs_external, int32_t max_episode_steps, void* stream) {
    if (envgpu::autoreset_args(action, max_episode_steps, false)) return -1;
    envgpu::EnvOut out{obs_internal, obs_external, reward, terminated, truncated, terminal_obs_internal,
                       terminal_obs_external, max_episode_steps, nullptr};
    return envgpu::launch_step(device, params, B, records, state, action, out, true, stream);
}

const char* mpcgpu_env_last_error(void) { return envgpu::g_err.text.c_str(); }

// include/mpcgpu_map.h
int32_t mpcgpu_env_step_fresh_dev(int32_t device, const mpcgpu_env_params* params, int32_t B, const double* records2,
                                  int32_t* which, int32_t* spare_ready, int32_t* loaded, int32_t* stale, double* state,
                                  const int32_t* action, float* obs_internal, float* obs_external, double* reward,
                                  uint8_t* terminated, uint8_t* truncated, float* terminal_obs_internal,
                                  float* terminal_obs_external, int32_t max_episode_steps, void* stream) {
    envgpu::EnvOut out{obs_internal, obs_external, reward, terminated, truncated, terminal_obs_internal,
                       terminal_obs_external, max_episode_steps, nullptr};
    const envgpu::EnvFresh fresh{which, spare_ready, loaded, stale};
    if (envgpu::fresh_args(fresh, nullptr, action, out)) return -1;
    return envgpu::launch_step(device, params, B, records2, state, action, out, true, stream, &fresh);
}

}  // extern "C"

// include/mpcgpu_collect.h
extern "C" {

int32_t mpcgpu_collect_act_dev(int32_t device, const float* theta, const float* obs_external, const float* obs_internal,
                               int32_t B, double eps, uint64_t seed, uint64_t serial, int32_t* actions, float* q, void* stream) {
    using namespace envgpu;
    if (!theta || !obs_external || !obs_internal || !actions) return collect_fail("null pointer (theta / obs_external / obs_internal / actions)");
    if (B < 0) return collect_fail("negative batch");
    if (!eps_ok(eps)) return collect_fail("eps must lie in [0, 1]");
    if (B == 0) return 0;
    if (abi::on_device(g_collect_err, device)) return -1;
    hipLaunchKernelGGL(collect_act_kernel, dim3(B < 1024 ? B : 1024), dim3(WAVE), 0, (hipStream_t)stream, theta, obs_external,
                       obs_internal, (int)B, eps, seed, serial, actions, q);
    return abi::launched(g_collect_err, "collect_act_kernel launch");
}

int32_t mpcgpu_collect_rays_dev(int32_t device, const mpcgpu_env_params* params, int32_t B, const double* records, double* state,
                                float* obs_internal, float* obs_external, double* reward, uint8_t* terminated,
                                uint8_t* truncated, float* terminal_obs_internal, float* terminal_obs_external,
                                int32_t max_episode_steps, const float* theta, const mpcgpu_collect_params* collect,
                                float* buf_obs, float* buf_next_obs, int64_t* buf_actions, float* buf_rewards, float* buf_dones,
                                double* ep_return, int32_t* actions, uint8_t* done, uint8_t* success, double* episode_return,
                                void* stream) {
    using namespace envgpu;
    const EnvOut out{obs_internal, obs_external, reward, terminated, truncated, terminal_obs_internal, terminal_obs_external,
                     max_episode_steps, nullptr};
    const CollectK co{theta, buf_obs, buf_next_obs, buf_actions, buf_rewards, buf_dones, ep_return, actions, done, success,
                      episode_return, {}};
    return launch_collect(g_collect_err, device, params, B, records, state, out, co, collect, stream, nullptr);
}

const char* mpcgpu_collect_last_error(void) { return envgpu::g_collect_err.text.c_str(); }

}  // extern "C"

// include/mpcgpu_collect_fresh.h
extern "C" {

int32_t mpcgpu_collect_rays_fresh_dev(int32_t device, const mpcgpu_env_params* params, int32_t B, const double* records2,
                                      int32_t* which, int32_t* spare_ready, int32_t* loaded, int32_t* stale, double* state,
                                      float* obs_internal, float* obs_external, double* reward, uint8_t* terminated,
                                      uint8_t* truncated, float* terminal_obs_internal, float* terminal_obs_external,
                                      int32_t max_episode_steps, const float* theta, const mpcgpu_collect_params* collect,
                                      float* buf_obs, float* buf_next_obs, int64_t* buf_actions, float* buf_rewards,
                                      float* buf_dones, double* ep_return, int32_t* actions, uint8_t* done, uint8_t* success,
                                      double* episode_return, void* stream) {
    using namespace envgpu;
    const EnvOut out{obs_internal, obs_external, reward, terminated, truncated, terminal_obs_internal, terminal_obs_external,
                     max_episode_steps, nullptr};
    const CollectK co{theta, buf_obs, buf_next_obs, buf_actions, buf_rewards, buf_dones, ep_return, actions, done, success,
                      episode_return, {}};
    const EnvFresh fresh{which, spare_ready, loaded, stale};
    return launch_collect(g_collect_fresh_err, device, params, B, records2, state, out, co, collect, stream, &fresh);
}

const char* mpcgpu_collect_fresh_last_error(void) { return envgpu::g_collect_fresh_err.text.c_str(); }

}  // extern "C"

// include/mpcgpu_eval.h
extern "C" {

int32_t mpcgpu_eval_rays_dev(int32_t device, const mpcgpu_env_params* params, int32_t B, const double* records, double* state,
                             float* obs_internal, float* obs_external, double* reward, uint8_t* terminated, uint8_t* truncated,
                             float* terminal_obs_internal, float* terminal_obs_external, int32_t max_episode_steps,
                             const float* theta, const mpcgpu_eval_params* eval, int32_t* episodes_done, int64_t* steps_done,
                             double* ep_return, int32_t* ep_length, double* returns, int32_t* lengths, uint8_t* outcome,
                             void* stream) {
    using namespace envgpu;
    abi::ErrorSlot& err = g_eval_err;
    const EnvOut out{obs_internal, obs_external, reward, terminated, truncated, terminal_obs_internal, terminal_obs_external,
                     max_episode_steps, nullptr};
    EnvK k;
    if (const char* bad = params_error(params, k)) return err.fail(bad);
    if (!records || !state || !obs_internal || !obs_external || !reward || !terminated || !truncated || !terminal_obs_internal ||
        !terminal_obs_external)
        return err.fail("null pointer (an environment tensor)");
    if (!theta || !eval) return err.fail("null pointer (theta / eval)");
    if (!episodes_done || !steps_done || !ep_return || !ep_length)
        return err.fail("null pointer (episodes_done / steps_done / ep_return / ep_length)");
    if (!returns || !lengths || !outcome) return err.fail("null pointer (returns / lengths / outcome)");
    if (B < 0) return err.fail("negative batch");
    if (max_episode_steps <= 0) return err.fail("max_episode_steps must be positive");
    if (eval->episodes < 1 || eval->episodes > MPCGPU_EVAL_MAX_EPISODES)
        return err.fail("1 <= episodes <= 256 (MPCGPU_EVAL_MAX_EPISODES)");
    if (eval->max_steps < 1 || eval->max_steps > MPCGPU_EVAL_MAX_LAUNCH_STEPS)
        return err.fail("1 <= max_steps <= 4096 (MPCGPU_EVAL_MAX_LAUNCH_STEPS)");
    if (!eps_ok(eval->eps)) return err.fail("eps must lie in [0, 1]");
    if (B == 0) return 0;
    if (abi::on_device(err, device)) return -1;
    const EvalK co{theta, episodes_done, steps_done, ep_return, ep_length, returns, lengths, outcome, *eval};
    hipLaunchKernelGGL((env_step_kernel<false, false, true>), dim3(B), dim3(WAVE), 0, (hipStream_t)stream, k, records, state,
                       (const int32_t*)nullptr, out, (int)B, EnvFresh{}, co);
    return abi::launched(err, "env_step_kernel launch");
}

const char* mpcgpu_eval_last_error(void) { return envgpu::g_eval_err.text.c_str(); }

}  // extern "C"
