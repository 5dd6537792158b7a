// dqn_act.hpp -- the action rule of include/mpcgpu_collect.h for one wavefront: forward pass of the ray Q-network out of LDS,
// the arg-max scan and the two draws of the counter stream.  Used by both kernels of that header (envgpu.hip).
//
// The forward pass is float32 WITHOUT fused multiply-add under any -ffp-contract setting: inside a translation unit built with
// -ffp-contract=fast neither `#pragma clang fp contract(off)` nor __fmul_rn / __fadd_rn keep the compiler from v_fmac_f32, so the
// product passes through an empty register barrier before it is added (v_mul_f32 + v_add_f32).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "counter_stream.hpp"
#include "dqn_layout.hpp"

namespace dqnact {

using namespace dqn_layout;      // OBS, HID, ACT and the offsets OFF_W0 .. OFF_B2 into theta
static_assert(OFF_B2 + ACT == MPCGPU_DQN_PARAMS, "parameter layout of mpcgpu_dqn.h");

// theta with its rows padded to an odd stride (lane j reads row j: 16 lanes, 16 banks), the observation, the activations
struct ActLds {
    float w0[HID][OBS + 1], b0[HID], w1[HID][HID + 1], b1[HID], w2[ACT][HID + 1], b2[ACT];
    float x[OBS], h1[HID], h2[HID], q[ACT];
};

__device__ __forceinline__ float mul_then_add(float acc, float w, float x) {   // two rounded operations, never one
    float p = w * x;
    asm volatile("" : "+v"(p));
    return acc + p;
}

// every thread of the workgroup calls it; the caller synchronises before the first act()
__device__ inline void stage_theta(ActLds& L, const float* __restrict__ theta, int lane, int threads) {
    for (int i = lane; i < HID * OBS; i += threads) L.w0[i / OBS][i % OBS] = theta[OFF_W0 + i];
    for (int i = lane; i < HID * HID; i += threads) L.w1[i / HID][i % HID] = theta[OFF_W1 + i];
    for (int i = lane; i < ACT * HID; i += threads) L.w2[i / HID][i % HID] = theta[OFF_W2 + i];
    if (lane < HID) { L.b0[lane] = theta[OFF_B0 + lane]; L.b1[lane] = theta[OFF_B1 + lane]; }
    if (lane < ACT) L.b2[lane] = theta[OFF_B2 + lane];
}

// One wavefront (= the workgroup), L.x written and synchronised by the caller.  Leaves q in L.q and returns the action, the same
// value in every lane.  Ends behind a barrier: the caller may read L.q and must synchronise before it rewrites L.x.
__device__ inline int act(ActLds& L, int lane, double eps, uint64_t seed, uint64_t serial, uint64_t b) {
    if (lane < HID) {
        float acc = L.b0[lane];
        for (int k = 0; k < OBS; ++k) acc = mul_then_add(acc, L.w0[lane][k], L.x[k]);
        L.h1[lane] = acc > 0.0f ? acc : 0.0f;
    }
    __syncthreads();
    if (lane < HID) {
        float acc = L.b1[lane];
        for (int k = 0; k < HID; ++k) acc = mul_then_add(acc, L.w1[lane][k], L.h1[k]);
        L.h2[lane] = acc > 0.0f ? acc : 0.0f;
    }
    __syncthreads();
    if (lane < ACT) {
        float acc = L.b2[lane];
        for (int k = 0; k < HID; ++k) acc = mul_then_add(acc, L.w2[lane][k], L.h2[k]);
        L.q[lane] = acc;
    }
    __syncthreads();
    int greedy = 0;
    float best = L.q[0];
    for (int a = 1; a < ACT; ++a) {
        const float qa = L.q[a];
        if (qa > best) { best = qa; greedy = a; }
    }
    const uint64_t key = counter_stream::key_of(seed, serial);      // row b owns draws 2 b (explore?) and 2 b + 1 (which action)
    const uint64_t bits_e = COUNTER_STREAM_DRAW(key, 2 * b + 1), bits_a = COUNTER_STREAM_DRAW(key, 2 * b + 2);
    return counter_stream::unit(bits_e) < eps ? (int)__umul64hi(bits_a, 9ull) : greedy;
}

}  // namespace dqnact
