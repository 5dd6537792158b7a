// counter_stream.hpp -- the counter-based random stream of include/mpcgpu_map.h, the ONLY definition on the device: the map
// stream (mapgpu.hip), the minibatch rows and tree uniforms of the fused DQN launches (dqngpu.hip) and the exploration draws of
// the collection kernel (dqn_act.hpp) all come from here.  Host twins: map_stream.CounterUniform and tests/support/*_numpy.py.
//
//   key  = mix64(seed + G * serial)          one key per (seed, serial): a map, a gradient step, an environment step
//   bits = mix64(key + G * (k + 1))          draw k = 0, 1, .. of that key: its counter is k + 1
//   u    = (bits >> 11) * 2^-53              the unit double of 64 bits, in [0, 1)
//
// Everything here is 64-bit integer arithmetic but the last line, an exact conversion of a 53-bit integer and an exact
// multiplication by a power of two: there is nothing to contract or reassociate, so the header means the same under every flag
// set of the Makefile.  What a file does WITH u (mapgpu.hip's lo + (hi - lo) * u) is contraction-sensitive and stays in that file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace counter_stream {

constexpr uint64_t G = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {   // SplitMix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t key_of(uint64_t seed, uint64_t serial) { return mix64(seed + G * serial); }

__device__ __forceinline__ double unit(uint64_t bits) { return (double)(bits >> 11) * 0x1p-53; }

}  // namespace counter_stream

// The 64 bits of draw k = 0, 1, .. of a key.  Its counter is k + 1 (counter 0 is never drawn) and the call site forms it.
// A macro and not a function: the optimiser simplifies a helper's body and the expression at its call site separately before it
// inlines, and behind a function dqn_act.hpp's key + G * (2 b + 1) came out reassociated, with two more SGPRs in
// collect_act_kernel.  Spliced into the expression, every site compiles to the instructions it had when it spelled this out.
#define COUNTER_STREAM_DRAW(key, counter) (counter_stream::mix64((key) + counter_stream::G * (counter)))
