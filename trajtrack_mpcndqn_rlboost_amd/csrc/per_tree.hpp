// per_tree.hpp -- the device-side rules of the sum tree (include/mpcgpu_per.h), written ONCE for the two
// translation units that walk it: pergpu.hip (the tree's own kernels) and dqngpu.hip (the prioritized K-step launch,
// DESIGN.md 8.7).  Both call the functions below, so a sample or an update inside the fused launch is the sample or update
// kernel's arithmetic by construction.  Layout and the rule "an inner node is recomputed only after both children are final"
// are stated at the head of pergpu.hip.  Both files are built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/mpcgpu_per.h"
#include "per_pow.hpp"

namespace pergpu {

// x^y as the C library rounds it (per_pow.hpp); outside the range a priority or a weight can have, the device library's
__device__ inline double pow_as_libm(double x, double y) {
    double v;
    return libm_pow(x, y, &v) ? v : pow(x, y);
}

__host__ __device__ inline int depth_of(int64_t i) { return 63 - __builtin_clzll((unsigned long long)(i + 1)); }

// what every entry that takes mpcgpu_per_params says when valid() refuses them
constexpr const char* BAD_PARAMS =
    "invalid mpcgpu_per_params (capacity 1..2^30, update_max_freq >= 1, alpha, epsilon >= 0, 0 <= beta < inf, initial_priority > 0)";
inline bool valid(const mpcgpu_per_params* p) {
    return p && p->capacity >= 1 && p->capacity <= ((int64_t)1 << 30) && p->update_max_freq >= 1 && p->alpha >= 0.0 &&
           p->beta >= 0.0 && p->beta <= DBL_MAX && p->epsilon >= 0.0 && p->initial_priority > 0.0;      // a NaN fails every comparison
}

// the point row i of n descends with: u in [0, 1) of the way through stratum i of [0, total)
__device__ inline double stratum_point(double total, int n, int i, double u) {
    const double segment = total / (double)n;
    const double a = segment * (double)i, b = segment * (double)(i + 1);
    return a + (b - a) * u;
}

// from the root to a leaf of a tree of len = 2 C - 1 nodes: always ends on a leaf, C - 1 <= index <= 2 C - 2, whatever the
// tree holds
__device__ inline int64_t descend(const double* tree, int64_t len, double s) {
    int64_t idx = 0;
    for (int64_t left = 1; left < len; left = 2 * idx + 1) {
        const double tl = tree[left], tr = tree[left + 1];
        bool go_left = s <= tl;
        if (go_left && tl == 0.0) go_left = false;          // never into an empty subtree: the sibling instead
        else if (!go_left && tr == 0.0) go_left = true;
        if (go_left) idx = left;
        else { s = s - tl; idx = left + 1; }
    }
    return idx;
}

// importance weight of a leaf before the division by the rows' maximum
__device__ inline double raw_weight(int64_t n_entries, double leaf, double total, double beta) {
    return pow_as_libm((double)n_entries * leaf / total, -beta);
}

// the priority a TD error gives its leaf
__device__ inline double priority(float td, double epsilon, double alpha) { return pow_as_libm(fabs((double)td) + epsilon, alpha); }

// leaf idx's ancestor at depth d := the sum of its children (nothing when the leaf is not below depth d).  The caller puts a
// barrier between two depths, deepest first.
__device__ inline void recompute_ancestor(double* tree, int64_t idx, int d) {
    const int dl = depth_of(idx);
    if (dl <= d) return;
    const int64_t node = ((idx + 1) >> (dl - d)) - 1;
    tree[node] = tree[2 * node + 1] + tree[2 * node + 2];
}

}  // namespace pergpu
