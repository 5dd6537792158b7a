// pergpu.hip -- the sum tree of prioritized experience replay on the device (include/mpcgpu_per.h).
//
// The tree is 2 C - 1 doubles in heap order; leaf of ring position p = node p + C - 1.  C is any positive integer, so the
// leaves sit on the two deepest depths D - 1 and D, D = depth(2 C - 2), depth(i) = floor(log2(i + 1)); the nodes of one
// depth are the contiguous index range [2^d - 1, 2^(d+1) - 2].
//
// ONE rule carries the correctness of every kernel below: an inner node is recomputed as tree[left] + tree[right] only
// after BOTH children are final.  So ancestors are recomputed DEPTH BY DEPTH, deepest first -- never "every row climbs one
// parent per round", which mixes the two leaf depths and reads stale sums.  Rows that share an ancestor may both recompute
// it: they write the same value.  Between two depths stands a workgroup barrier (the small calls: one workgroup) or a
// kernel boundary (the wide levels of `add`).
//
// Built with -ffp-contract=off: sums, the descent and the powers (per_pow.hpp) follow tests/support/per_numpy.py operation by
// operation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/mpcgpu_per.h"
#include "abi_host.hpp"
#include "per_tree.hpp"

namespace pergpu {

constexpr int STATE_HEAD = 4;          // max_p, rows since the last reading, 2 reserved
constexpr int MAX_BLOCKS = 256;        // partial maxima of the leaf reduction
constexpr int STATE_DOUBLES = STATE_HEAD + MAX_BLOCKS;
constexpr int SMALL = 1024;            // threads of the one-workgroup kernels
// a bit pattern no priority has (a negative quiet NaN), greater as an unsigned integer than every non-negative double:
// marks the leaves of an update while the rows settle which of them wins
constexpr unsigned long long TAG = 0xFFF8000000000000ull;

// pow_as_libm, depth_of, the descent, the weight, the priority and the recomputation of one ancestor: per_tree.hpp (shared with
// the prioritized K-step launch of dqngpu.hip)

// up to four contiguous leaf ranges (ring wrap x two leaf depths), each on ONE depth
struct Ranges {
    int64_t lo[4], hi[4];
    int32_t depth[4];
    int32_t count;
};

__host__ __device__ inline int64_t ancestors_at(const Ranges& rg, int k, int d, int64_t* first) {
    if (rg.depth[k] <= d) return 0;
    const int sh = rg.depth[k] - d;
    const int64_t a = ((rg.lo[k] + 1) >> sh) - 1, b = ((rg.hi[k] + 1) >> sh) - 1;
    *first = a;
    return b - a + 1;
}

__global__ void per_reset_kernel(double* tree, int64_t len, double* state, double initial_priority, double freq) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += stride) tree[i] = 0.0;
    if (blockIdx.x == 0 && threadIdx.x < STATE_DOUBLES)
        state[threadIdx.x] = threadIdx.x == 0 ? initial_priority : threadIdx.x == 1 ? freq : 0.0;
}

// ---- add ---------------------------------------------------------------------------------------------------------------
// (1) partial maxima over the leaves, only when a reading is due (every block reads the same state[1]; nothing writes it
// in this kernel)
__global__ void per_max_partial_kernel(const double* leaves, int64_t C, double* state, double freq, int64_t n_entries) {
    if (state[1] < freq || n_entries == 0) return;
    __shared__ double red[256];
    double m = -INFINITY;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < C; i += stride) {
        const double v = leaves[i];
        m = v > m ? v : m;
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x + s] > red[threadIdx.x] ? red[threadIdx.x + s] : red[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) state[STATE_HEAD + blockIdx.x] = red[0];
}

// (2) one workgroup of MAX_BLOCKS threads: max_p and the counter
__global__ void per_max_final_kernel(double* state, int blocks, double freq, double initial_priority, int64_t n_entries, double n) {
    __shared__ double red[MAX_BLOCKS];
    const bool due = state[1] >= freq;
    red[threadIdx.x] = (due && n_entries > 0 && (int)threadIdx.x < blocks) ? state[STATE_HEAD + threadIdx.x] : -INFINITY;
    __syncthreads();
    for (int s = MAX_BLOCKS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x + s] > red[threadIdx.x] ? red[threadIdx.x + s] : red[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double since = state[1];
        if (due) {
            state[0] = n_entries > 0 ? red[0] : initial_priority;
            since = 0.0;
        }
        state[1] = since + n;
    }
}

// (3) the new rows' leaves
__global__ void per_add_leaves_kernel(double* tree, const double* state, int64_t C, int64_t pos, int64_t rows) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    tree[C - 1 + (pos + r) % C] = state[0];
}

// (4) ancestors of the ranges at depths d_from .. d_to (descending).  Several depths in one launch only with ONE
// workgroup (the barrier orders them); the host launches the wide levels one depth at a time.
__global__ void per_climb_ranges_kernel(double* tree, Ranges rg, int d_from, int d_to) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int d = d_from; d >= d_to; --d) {
        int64_t first[4] = {0, 0, 0, 0}, cnt[4] = {0, 0, 0, 0}, total = 0;
        for (int k = 0; k < rg.count; ++k) {
            cnt[k] = ancestors_at(rg, k, d, &first[k]);
            total += cnt[k];
        }
        for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
            int64_t off = t;
            int k = 0;
            while (off >= cnt[k]) off -= cnt[k++];
            const int64_t node = first[k] + off;
            tree[node] = tree[2 * node + 1] + tree[2 * node + 2];
        }
        if (d > d_to) __syncthreads();
    }
}

// ---- update: one workgroup -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SMALL) per_update_kernel(double* tree, int64_t C, const int64_t* indices, const float* td,
                                                           int n, double alpha, double epsilon) {
    unsigned long long* bits = reinterpret_cast<unsigned long long*>(tree);
    // the highest row of every leaf wins: all rows raise the leaf to TAG | row, the barrier, then the row that finds its
    // own tag stores the priority.  Deterministic, and needs no scratch.
    for (int r = threadIdx.x; r < n; r += SMALL) {
        const int64_t idx = indices[r];
        if (idx >= C - 1 && idx <= 2 * C - 2) atomicMax(&bits[idx], TAG | (unsigned long long)r);
    }
    __syncthreads();
    for (int r = threadIdx.x; r < n; r += SMALL) {
        const int64_t idx = indices[r];
        if (idx >= C - 1 && idx <= 2 * C - 2 &&
            __hip_atomic_load(&bits[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (TAG | (unsigned long long)r))
            tree[idx] = priority(td[r], epsilon, alpha);
    }
    __syncthreads();
    const int D = depth_of(2 * C - 2);
    for (int d = D - 1; d >= 0; --d) {
        for (int r = threadIdx.x; r < n; r += SMALL) {
            const int64_t idx = indices[r];
            if (idx < C - 1 || idx > 2 * C - 2) continue;
            recompute_ancestor(tree, idx, d);
        }
        __syncthreads();
    }
}

// ---- sample: one workgroup ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SMALL) per_sample_kernel(const double* tree, int64_t C, const double* u, int n, int64_t n_entries,
                                                           double beta, int64_t* indices, int64_t* positions, float* weights) {
    __shared__ double red[SMALL];
    constexpr int PER_THREAD = MPCGPU_PER_MAX_ROWS / SMALL;
    const int64_t len = 2 * C - 1;
    const double total = tree[0];
    double w[PER_THREAD];
    double wmax = -INFINITY;
    for (int j = 0; j < PER_THREAD; ++j) {
        const int i = threadIdx.x + j * SMALL;
        w[j] = 0.0;
        if (i >= n) continue;
        const int64_t idx = descend(tree, len, stratum_point(total, n, i, u[i]));
        indices[i] = idx;
        positions[i] = idx - (C - 1);
        w[j] = raw_weight(n_entries, tree[idx], total, beta);
        wmax = w[j] > wmax ? w[j] : wmax;
    }
    red[threadIdx.x] = wmax;
    __syncthreads();
    for (int s = SMALL / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x + s] > red[threadIdx.x] ? red[threadIdx.x + s] : red[threadIdx.x];
        __syncthreads();
    }
    wmax = red[0];
    for (int j = 0; j < PER_THREAD; ++j) {
        const int i = threadIdx.x + j * SMALL;
        if (i < n) weights[i] = (float)(w[j] / wmax);
    }
}

__global__ void per_stats_kernel(const double* tree, const double* state, double* out) {
    out[0] = tree[0];
    out[1] = state[0];
}

// ---- host ------------------------------------------------------------------------------------------------------------------
thread_local abi::ErrorSlot g_err;
int fail(const char* what) { return g_err.fail(what); }
int launched(const char* what) { return abi::launched(g_err, what); }

// the device is set BEFORE the entries check their pointers: a caller without a device hears of that first
int begin(int32_t device, const mpcgpu_per_params* p) {
    if (!valid(p)) return fail(BAD_PARAMS);
    return abi::on_device(g_err, device);
}

// the leaves of ring rows pos .. pos + rows - 1 (mod C) as ranges of tree indices, each on one depth
Ranges leaf_ranges(int64_t C, int64_t pos, int64_t rows) {
    Ranges rg{};
    const int D = depth_of(2 * C - 2);
    const int64_t split = ((int64_t)1 << D) - 1;   // first node of depth D
    int64_t piece[2][2];
    int pieces = 0;
    if (rows >= C) { piece[0][0] = 0; piece[0][1] = C - 1; pieces = 1; }
    else {
        piece[0][0] = pos; piece[0][1] = (pos + rows < C ? pos + rows : C) - 1; pieces = 1;
        if (pos + rows > C) { piece[1][0] = 0; piece[1][1] = pos + rows - C - 1; pieces = 2; }
    }
    for (int k = 0; k < pieces; ++k) {
        const int64_t lo = piece[k][0] + C - 1, hi = piece[k][1] + C - 1;
        if (lo < split) { rg.lo[rg.count] = lo; rg.hi[rg.count] = hi < split ? hi : split - 1; rg.depth[rg.count++] = D - 1; }
        if (hi >= split) { rg.lo[rg.count] = lo > split ? lo : split; rg.hi[rg.count] = hi; rg.depth[rg.count++] = D; }
    }
    return rg;
}

}  // namespace pergpu

extern "C" {

int32_t mpcgpu_per_state_doubles(void) { return pergpu::STATE_DOUBLES; }

int32_t mpcgpu_per_reset_dev(int32_t device, const mpcgpu_per_params* params, double* tree, double* state, void* stream) {
    using namespace pergpu;
    if (begin(device, params)) return -1;
    if (!tree || !state) return fail("null pointer");
    const int64_t len = 2 * params->capacity - 1;
    const int blocks = (int)((len + 255) / 256 < 1024 ? (len + 255) / 256 : 1024);
    hipLaunchKernelGGL(per_reset_kernel, dim3(blocks), dim3(STATE_DOUBLES > 256 ? 512 : 256), 0, (hipStream_t)stream, tree, len, state,
                       params->initial_priority, (double)params->update_max_freq);
    return launched("per_reset_kernel launch");
}

int32_t mpcgpu_per_add_dev(int32_t device, const mpcgpu_per_params* params, double* tree, double* state, int64_t pos,
                           int64_t n, int64_t n_entries, void* stream) {
    using namespace pergpu;
    if (begin(device, params)) return -1;
    const int64_t C = params->capacity;
    if (!tree || !state) return fail("null pointer");
    if (n < 1 || pos < 0 || pos >= C || n_entries < 0 || n_entries > C) return fail("add: n >= 1, 0 <= pos < capacity, 0 <= n_entries <= capacity");
    hipStream_t st = (hipStream_t)stream;
    const double freq = (double)params->update_max_freq;
    const int blocks = (int)((C + 255) / 256 < MAX_BLOCKS ? (C + 255) / 256 : MAX_BLOCKS);
    hipLaunchKernelGGL(per_max_partial_kernel, dim3(blocks), dim3(256), 0, st, tree + (C - 1), C, state, freq, n_entries);
    hipLaunchKernelGGL(per_max_final_kernel, dim3(1), dim3(MAX_BLOCKS), 0, st, state, blocks, freq, params->initial_priority, n_entries, (double)n);
    const int64_t rows = n < C ? n : C;
    hipLaunchKernelGGL(per_add_leaves_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, tree, state, C, pos, rows);
    const Ranges rg = leaf_ranges(C, pos, rows);
    for (int d = depth_of(2 * C - 2) - 1; d >= 0; --d) {
        int64_t width = 0, first;
        for (int k = 0; k < rg.count; ++k) width += ancestors_at(rg, k, d, &first);
        if (width > SMALL) {     // a wide level: one launch, the kernel boundary orders it before the next
            hipLaunchKernelGGL(per_climb_ranges_kernel, dim3((unsigned)((width + 255) / 256)), dim3(256), 0, st, tree, rg, d, d);
        } else {                 // the rest of the way up in one workgroup
            hipLaunchKernelGGL(per_climb_ranges_kernel, dim3(1), dim3(SMALL), 0, st, tree, rg, d, 0);
            break;
        }
    }
    return launched("per add launch");
}

int32_t mpcgpu_per_update_dev(int32_t device, const mpcgpu_per_params* params, double* tree, const int64_t* indices,
                              const float* td_error, int32_t n, void* stream) {
    using namespace pergpu;
    if (begin(device, params)) return -1;
    if (!tree || !indices || !td_error) return fail("null pointer");
    if (n < 1 || n > MPCGPU_PER_MAX_ROWS) return fail("update: 1 <= n <= 4096");
    hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(SMALL), 0, (hipStream_t)stream, tree, params->capacity, indices, td_error,
                       (int)n, params->alpha, params->epsilon);
    return launched("per_update_kernel launch");
}

int32_t mpcgpu_per_sample_dev(int32_t device, const mpcgpu_per_params* params, const double* tree, const double* u,
                              int32_t n, int64_t n_entries, int64_t* indices, int64_t* positions, float* weights,
                              void* stream) {
    using namespace pergpu;
    if (begin(device, params)) return -1;
    if (!tree || !u || !indices || !positions || !weights) return fail("null pointer");
    if (n < 1 || n > MPCGPU_PER_MAX_ROWS) return fail("sample: 1 <= n <= 4096");
    if (n_entries < 1 || n_entries > params->capacity) return fail("sample: 1 <= n_entries <= capacity");
    hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(SMALL), 0, (hipStream_t)stream, tree, params->capacity, u, (int)n, n_entries,
                       params->beta, indices, positions, weights);
    return launched("per_sample_kernel launch");
}

int32_t mpcgpu_per_stats_dev(int32_t device, const mpcgpu_per_params* params, const double* tree, const double* state,
                             double* out, void* stream) {
    using namespace pergpu;
    if (begin(device, params)) return -1;
    if (!tree || !state || !out) return fail("null pointer");
    hipLaunchKernelGGL(per_stats_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, tree, state, out);
    return launched("per_stats_kernel launch");
}

const char* mpcgpu_per_last_error(void) { return pergpu::g_err.text.c_str(); }

}  // extern "C"
