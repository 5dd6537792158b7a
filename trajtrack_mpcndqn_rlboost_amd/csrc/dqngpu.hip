// dqngpu.hip -- the DQN update of the ray Q-network as one workgroup (include/mpcgpu_dqn.h).
//
// ONE kernel body serves the four entries (gradient, apply, step, K steps): what differs between them is which phases run, so
// step == gradient + apply and K steps == K single steps hold by construction.  256 threads, one workgroup:
//   phase A  thread i = row i: target network on next_obs, (double_q: online network on next_obs,) online network on obs, delta,
//            the row's loss term and coefficient, the backward pass down to dz0.  Both parameter vectors are read from LDS, where
//            every row of a weight matrix starts on a 16-byte boundary (W0's rows are padded from 46 to 48 words), four weights
//            per read, every lane the same words: a broadcast.  The row leaves everything the gradient sums need -- x, h1, h2,
//            dz0, dz1, dz2 and a constant 1 -- in an LDS record of RS = 121 words (odd: the lanes' records fall on different banks).
//   phase B  thread L owns the parameters L, L + 256, .. (five slots at most).  Every gradient entry is the sum over the rows,
//            in ascending order, of record[cofs] * record[iofs] for two offsets that depend on the entry alone (a bias takes the
//            constant 1 as its input: c * 1 is c), so the five slots run through ONE loop over the rows, LDS reads only.
//   phase C  clip and Adam on the owned slots; the new parameters go back to LDS (the next step reads them) and to the state.
// In the K-step loop m, v and theta of the owned slots stay in registers and the state block is written once, at the end.
// LDS: 256 records of 484 bytes + two padded parameter vectors + the fold's slots = 134 KB of the CU's 160 KB.
//
// The kernel is a template over PER.  <false> is the kernel of the four entries as it always was (same registers, scratch and
// LDS: `make resources`).  <true> (include/mpcgpu_dqn_per.h) adds two phases around A/B/C in every step:
//   phase S  thread i = row i: u from the counter stream, the descent of the sum tree, the weight; the maximum weight over the rows
//            and "the highest row of a repeated leaf wins" are settled in 4 KB of LDS (256 doubles, 256 indices);
//   phase U  the winners store their leaves' new priorities, then every row recomputes its ancestors depth by depth.
// Descent, weight, priority and the recomputation of an ancestor are per_tree.hpp's, the functions pergpu.hip's kernels call.  The
// tree stays in global memory and only this workgroup touches it during the launch: a barrier stands between the leaf stores,
// each depth of the climb and the next step's descent.
//
// SUMMATION ORDERS (restated from the header; tests/support/dqn_numpy.py follows them operation by operation): dot products
// bias first, then k ascending; dh1 from 0, j ascending; gradients from 0, rows ascending; loss and sum of squares over 256
// slots folded in halves 128, 64, .., 1 (the sum of squares after each lane added its slots in ascending order from 0).
//
// Built with -ffp-contract=off: a * b + c is two rounded operations, as in the numpy twin.  Division and square root are the
// correctly rounded ones (hipcc's default).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "../../include/mpcgpu_dqn.h"
#include "../../include/mpcgpu_dqn_per.h"
#include "abi_host.hpp"
#include "counter_stream.hpp"
#include "dqn_layout.hpp"
#include "per_tree.hpp"

namespace dqngpu {

constexpr int NT = MPCGPU_DQN_MAX_ROWS;     // threads = rows at most
using namespace dqn_layout;                 // OBS, HID, ACT, NP and the offsets OFF_W0 .. OFF_B2 into a parameter vector
static_assert(OFF_B2 + ACT == NP, "parameter layout");
// the same vector in LDS: W0's rows padded to 48 words, so that every matrix row is 16-byte aligned
constexpr int OBS_PAD = 48, PAD = HID * (OBS_PAD - OBS);
constexpr int L_W0 = 0, L_B0 = OFF_B0 + PAD, L_W1 = OFF_W1 + PAD, L_B1 = OFF_B1 + PAD, L_W2 = OFF_W2 + PAD, L_B2 = OFF_B2 + PAD,
              L_WORDS = ((NP + PAD + 3) / 4) * 4;
constexpr int SLOTS = (NP + NT - 1) / NT;   // 5
// words of a row record
constexpr int R_X = 0, R_H1 = R_X + OBS, R_H2 = R_H1 + HID, R_DZ0 = R_H2 + HID, R_DZ1 = R_DZ0 + HID, R_DZ2 = R_DZ1 + HID,
              R_ONE = R_DZ2 + ACT, RS = R_ONE + 2;      // 120 words and one of padding
static_assert(RS == 121, "an odd record stride");
constexpr int ST_THETA = 0, ST_TARGET = NP, ST_M = 2 * NP, ST_V = 3 * NP;
static_assert(4 * NP == MPCGPU_DQN_STATE_T, "state layout");

enum : int { DO_GRAD = 1, DO_APPLY = 2, DO_SAMPLE = 4 };

struct Args {
    float* state;                // apply: written; gradient only: read
    const float* obs;            // minibatch arrays, or the buffer's with DO_SAMPLE
    const float* next_obs;
    const int64_t* actions;
    const float* rewards;
    const float* dones;
    const float* weights;        // may be null
    const float* grad_in;        // apply without gradient: the gradient to apply
    float* grad_out;             // may be null (K steps)
    float* loss;                 // [steps]
    float* td;                   // may be null
    int64_t size;
    uint64_t seed, serial0;
    double lr, beta1, beta2;
    float gamma, max_norm, b1, b2, omb1, omb2, eps, scale;
    int n, steps, mode, double_q;
};

__host__ __device__ constexpr int lds_pos(int p) { return p < OFF_B0 ? (p / OBS) * OBS_PAD + p % OBS : p + PAD; }

using pergpu::pow_as_libm;

// out[j] = b[j] + sum over k ascending of W[j][k] * x[k]; W's rows are STRIDE words apart and 16-byte aligned
template <int IN, int STRIDE, int OUT, bool RELU>
__device__ __forceinline__ void dense(const float* W, const float* b, const float (&x)[IN], float (&out)[OUT]) {
#pragma unroll
    for (int j = 0; j < OUT; ++j) {
        float acc = b[j];
        const float4* row = reinterpret_cast<const float4*>(W + j * STRIDE);
#pragma unroll
        for (int q = 0; q < (IN + 3) / 4; ++q) {
            const float4 w = row[q];
            if (4 * q < IN) acc = acc + w.x * x[4 * q];
            if (4 * q + 1 < IN) acc = acc + w.y * x[(4 * q + 1) % IN];
            if (4 * q + 2 < IN) acc = acc + w.z * x[(4 * q + 2) % IN];
            if (4 * q + 3 < IN) acc = acc + w.w * x[(4 * q + 3) % IN];
        }
        out[j] = RELU ? (acc > 0.0f ? acc : 0.0f) : acc;
    }
}

__device__ __forceinline__ void network(const float* th, const float (&x)[OBS], float (&h1)[HID], float (&h2)[HID], float (&q)[ACT]) {
    dense<OBS, OBS_PAD, HID, true>(th + L_W0, th + L_B0, x, h1);
    dense<HID, HID, HID, true>(th + L_W1, th + L_B1, h1, h2);
    dense<HID, HID, ACT, false>(th + L_W2, th + L_B2, h2, q);
}

__device__ __forceinline__ void load_row(const float* base, int64_t row, float (&x)[OBS]) {
    const float2* src = reinterpret_cast<const float2*>(base + row * OBS);   // a row is 184 bytes: 8-byte aligned
#pragma unroll
    for (int k = 0; k < OBS / 2; ++k) {
        const float2 v = src[k];
        x[2 * k] = v.x;
        x[2 * k + 1] = v.y;
    }
}

// slots [0, 256) folded in halves; every thread gets slot 0
__device__ __forceinline__ float fold(float* red, float mine) {
    const int t = threadIdx.x;
    red[t] = mine;
    __syncthreads();
#pragma unroll
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (t < h) red[t] = red[t] + red[t + h];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// gradient entry p = sum over the rows of record[cofs] * record[iofs]
__device__ __forceinline__ void entry_offsets(int p, int* cofs, int* iofs) {
    *cofs = *iofs = R_ONE;                                                    // past the last parameter: 1 * 1, never used
    if (p < OFF_B0) { *cofs = R_DZ0 + p / OBS; *iofs = R_X + p % OBS; }
    else if (p < OFF_W1) *cofs = R_DZ0 + (p - OFF_B0);
    else if (p < OFF_B1) { *cofs = R_DZ1 + (p - OFF_W1) / HID; *iofs = R_H1 + (p - OFF_W1) % HID; }
    else if (p < OFF_W2) *cofs = R_DZ1 + (p - OFF_B1);
    else if (p < OFF_B2) { *cofs = R_DZ2 + (p - OFF_W2) / HID; *iofs = R_H2 + (p - OFF_W2) % HID; }
    else if (p < NP) *cofs = R_DZ2 + (p - OFF_B2);
}

// the sum tree of a prioritized launch; unused by the four entries of mpcgpu_dqn.h
struct PerArgs {
    double* tree;                // [2 C - 1]
    int64_t* indices;            // [steps][n], may be null
    int64_t C, n_entries;
    double alpha, beta, epsilon;
};
struct NoTree {};

// The body of every entry.  PER = false: the four entries of mpcgpu_dqn.h, no tree.  PER = true: gradient and apply in every
// step, the step's rows drawn from the sum tree in front of phase A (phase S) and their leaves re-prioritised behind phase C
// (phase U), by the functions of per_tree.hpp that the tree's own kernels call.  All tree traffic is this workgroup's; a barrier
// stands between the leaf stores, each depth of the climb and the next step's descent.
template <bool PER>
__global__ void __launch_bounds__(NT) dqn_kernel(const Args a, const std::conditional_t<PER, PerArgs, NoTree> tr) {
    __shared__ __align__(16) float th[L_WORDS], tt[L_WORDS];      // online and target parameters, padded layout
    __shared__ float rec[NT * RS];
    __shared__ float red[NT];
    const int t = threadIdx.x, n = a.n;
    const bool do_grad = PER || (a.mode & DO_GRAD), do_apply = PER || (a.mode & DO_APPLY), sample = !PER && (a.mode & DO_SAMPLE);
    const float nf = (float)n;

    float theta[SLOTS], m[SLOTS], v[SLOTS], g[SLOTS];
    int cofs[SLOTS], iofs[SLOTS];
#pragma unroll
    for (int c = 0; c < SLOTS; ++c) {
        const int p = t + c * NT;
        theta[c] = m[c] = v[c] = g[c] = 0.0f;
        entry_offsets(p, &cofs[c], &iofs[c]);
        if (p < NP) {
            theta[c] = a.state[ST_THETA + p];
            if (do_grad) {
                th[lds_pos(p)] = theta[c];
                tt[lds_pos(p)] = a.state[ST_TARGET + p];
            }
            if (do_apply) {
                m[c] = a.state[ST_M + p];
                v[c] = a.state[ST_V + p];
            }
        }
    }
    if (do_grad && t < PAD) {                    // the padding words are read (and not used): keep them defined
        th[(t / 2) * OBS_PAD + OBS + t % 2] = 0.0f;
        tt[(t / 2) * OBS_PAD + OBS + t % 2] = 0.0f;
    }
    int64_t count = do_apply ? *reinterpret_cast<const int64_t*>(a.state + MPCGPU_DQN_STATE_T) : 0;
    __syncthreads();

    for (int s = 0; s < a.steps; ++s) {
        // the step's key of the counter stream: row t takes draw t, its uniform in phase S or its buffer row in phase A
        const uint64_t key = counter_stream::key_of(a.seed, a.serial0 + (uint64_t)s);
        int64_t leaf = 0;            // PER: this row's tree index, its weight, its delta and whether it is the highest row of its leaf
        float drawn_w = 1.0f, delta = 0.0f;
        bool wins = false;
        if constexpr (PER) {
            // ---- phase S: the stratified sample of per_sample_kernel, u from the counter stream
            __shared__ double wred[NT];
            __shared__ int64_t drawn[NT];
            const double total = tr.tree[0];
            double w = -INFINITY;
            if (t < n) {
                const double u = counter_stream::unit(COUNTER_STREAM_DRAW(key, (uint64_t)(t + 1)));
                leaf = pergpu::descend(tr.tree, 2 * tr.C - 1, pergpu::stratum_point(total, n, t, u));
                w = pergpu::raw_weight(tr.n_entries, tr.tree[leaf], total, tr.beta);
                if (tr.indices) tr.indices[(int64_t)s * n + t] = leaf;
            }
            wred[t] = w;
            drawn[t] = leaf;
            __syncthreads();
#pragma unroll
            for (int h = NT / 2; h > 0; h >>= 1) {
                if (t < h) wred[t] = wred[t + h] > wred[t] ? wred[t + h] : wred[t];
                __syncthreads();
            }
            drawn_w = (float)(w / wred[0]);
            // on a repeated index the highest row wins.  Every lane reads every row (a broadcast, and no exit that depends on
            // what was read, so the reads run back to back): a scan from the row's own index that stops at the first repeat was
            // a chain of up to 255 LDS latencies and cost 9 us of the 79 us step at 256 rows
            bool repeated = false;
#pragma unroll 8
            for (int j = 0; j < n; ++j) repeated |= (j > t) & (drawn[j] == leaf);
            wins = t < n && !repeated;
        }
        if (do_grad) {
            // ---- phase A: one row per thread
            float mine = 0.0f;
            if (t < n) {
                int64_t row = t;
                if constexpr (PER) row = leaf - (tr.C - 1);
                if (sample) row = (int64_t)__umul64hi(COUNTER_STREAM_DRAW(key, (uint64_t)(t + 1)), (uint64_t)a.size);
                float x[OBS], h1[HID], h2[HID], q[ACT], scan[ACT];
                load_row(a.next_obs, row, x);
                network(tt, x, h1, h2, q);
                if (a.double_q) network(th, x, h1, h2, scan);
                else {
#pragma unroll
                    for (int k = 0; k < ACT; ++k) scan[k] = q[k];
                }
                float top = scan[0], next_v = q[0];
#pragma unroll
                for (int k = 1; k < ACT; ++k)
                    if (scan[k] > top) {
                        top = scan[k];
                        next_v = q[k];
                    }
                load_row(a.obs, row, x);
                network(th, x, h1, h2, q);
                int64_t act64 = a.actions[row];
                const int act = act64 < 0 ? 0 : act64 > ACT - 1 ? ACT - 1 : (int)act64;
                float qa = q[0];
#pragma unroll
                for (int k = 1; k < ACT; ++k) qa = act == k ? q[k] : qa;
                const float y = a.rewards[row] + ((1.0f - a.dones[row]) * a.gamma) * next_v;
                const float d = y - qa, e = fabsf(d);
                float l = e < 1.0f ? (0.5f * e) * e : e - 0.5f;
                float c = e < 1.0f ? -d : (d > 0.0f ? -1.0f : 1.0f);
                if (PER || a.weights) {
                    const float w = PER ? drawn_w : a.weights[row];
                    l = w * l;
                    c = w * c;
                }
                const float gq = c / nf;
                float* r = rec + t * RS;
                float dz1[HID], dh1[HID];
                const float4* w2 = reinterpret_cast<const float4*>(th + L_W2 + act * HID);
#pragma unroll
                for (int k4 = 0; k4 < HID / 4; ++k4) {
                    const float4 w = w2[k4];
                    dz1[4 * k4] = h2[4 * k4] > 0.0f ? w.x * gq : 0.0f;
                    dz1[4 * k4 + 1] = h2[4 * k4 + 1] > 0.0f ? w.y * gq : 0.0f;
                    dz1[4 * k4 + 2] = h2[4 * k4 + 2] > 0.0f ? w.z * gq : 0.0f;
                    dz1[4 * k4 + 3] = h2[4 * k4 + 3] > 0.0f ? w.w * gq : 0.0f;
                }
#pragma unroll
                for (int k = 0; k < HID; ++k) dh1[k] = 0.0f;
#pragma unroll
                for (int j = 0; j < HID; ++j) {              // j ascending for every k
                    const float4* w1 = reinterpret_cast<const float4*>(th + L_W1 + j * HID);
#pragma unroll
                    for (int k4 = 0; k4 < HID / 4; ++k4) {
                        const float4 w = w1[k4];
                        dh1[4 * k4] = dh1[4 * k4] + w.x * dz1[j];
                        dh1[4 * k4 + 1] = dh1[4 * k4 + 1] + w.y * dz1[j];
                        dh1[4 * k4 + 2] = dh1[4 * k4 + 2] + w.z * dz1[j];
                        dh1[4 * k4 + 3] = dh1[4 * k4 + 3] + w.w * dz1[j];
                    }
                }
#pragma unroll
                for (int k = 0; k < OBS; ++k) r[R_X + k] = x[k];
#pragma unroll
                for (int k = 0; k < HID; ++k) {
                    r[R_H1 + k] = h1[k];
                    r[R_H2 + k] = h2[k];
                    r[R_DZ0 + k] = h1[k] > 0.0f ? dh1[k] : 0.0f;
                    r[R_DZ1 + k] = dz1[k];
                }
#pragma unroll
                for (int k = 0; k < ACT; ++k) r[R_DZ2 + k] = act == k ? gq : 0.0f;
                r[R_ONE] = 1.0f;
                if (a.td) a.td[PER ? (int64_t)s * n + t : t] = d;
                if constexpr (PER) delta = d;
                mine = l;
            }
            const float total = fold(red, mine);      // its first barrier also publishes the records
            if (t == 0) a.loss[s] = total / nf;
            // ---- phase B: the owned gradient entries, all slots in one loop over the rows
#pragma unroll
            for (int c = 0; c < SLOTS; ++c) g[c] = 0.0f;
#pragma unroll 4
            for (int i = 0; i < n; ++i) {
                const float* r = rec + i * RS;
#pragma unroll
                for (int c = 0; c < SLOTS; ++c) g[c] = g[c] + r[cofs[c]] * r[iofs[c]];
            }
            if (a.grad_out) {
#pragma unroll
                for (int c = 0; c < SLOTS; ++c)
                    if (t + c * NT < NP) a.grad_out[t + c * NT] = g[c];
            }
        } else {
#pragma unroll
            for (int c = 0; c < SLOTS; ++c) {
                const int p = t + c * NT;
                if (p < NP) g[c] = a.grad_in[p];
            }
        }
        if (do_apply) {
            // ---- phase C: clip and Adam
            float ss = 0.0f;
#pragma unroll
            for (int c = 0; c < SLOTS; ++c) {
                g[c] = g[c] * a.scale;
                if (t + c * NT < NP) ss = ss + g[c] * g[c];
            }
            const float norm = sqrtf(fold(red, ss));   // every thread is past phase B behind its barriers
            const float ratio = a.max_norm / (norm + 1e-6f);
            const float coef = ratio < 1.0f ? ratio : 1.0f;
            count += 1;
            const double bc1 = 1.0 - pow_as_libm(a.beta1, (double)count), bc2 = 1.0 - pow_as_libm(a.beta2, (double)count);
            const float step = (float)(a.lr / bc1), root = (float)sqrt(bc2);
#pragma unroll
            for (int c = 0; c < SLOTS; ++c) {
                const int p = t + c * NT;
                if (p < NP) {
                    const float gc = g[c] * coef;
                    m[c] = a.b1 * m[c] + a.omb1 * gc;
                    v[c] = a.b2 * v[c] + a.omb2 * (gc * gc);
                    theta[c] = theta[c] - step * (m[c] / (sqrtf(v[c]) / root + a.eps));
                    if (do_grad) th[lds_pos(p)] = theta[c];
                }
            }
        }
        if constexpr (PER) {
            // ---- phase U: per_update_kernel's leaves and climb
            if (wins) tr.tree[leaf] = pergpu::priority(delta, tr.epsilon, tr.alpha);
            __syncthreads();  // the leaves are final; the next step reads the new parameters, and may overwrite the records
            for (int d = pergpu::depth_of(2 * tr.C - 2) - 1; d >= 0; --d) {
                if (t < n) pergpu::recompute_ancestor(tr.tree, leaf, d);
                __syncthreads();
            }
        } else {
            __syncthreads();  // the next step reads the new parameters, and may overwrite the records
        }
    }
    if (do_apply) {
#pragma unroll
        for (int c = 0; c < SLOTS; ++c) {
            const int p = t + c * NT;
            if (p < NP) {
                a.state[ST_THETA + p] = theta[c];
                a.state[ST_M + p] = m[c];
                a.state[ST_V + p] = v[c];
            }
        }
        if (t == 0) *reinterpret_cast<int64_t*>(a.state + MPCGPU_DQN_STATE_T) = count;
    }
}


// ---- host ------------------------------------------------------------------------------------------------------------------
thread_local abi::ErrorSlot g_err;          // mpcgpu_dqn_last_error
thread_local abi::ErrorSlot g_err_per;      // mpcgpu_dqn_per_last_error: a slot of its own, a refusal there leaves g_err alone
int fail(const char* what) { return g_err.fail(what); }

// what every entry that takes mpcgpu_dqn_params says when valid() refuses them
constexpr const char* BAD_PARAMS = "invalid mpcgpu_dqn_params (lr, max_grad_norm, eps > 0, 0 <= beta < 1, double_q 0 / 1)";
bool valid(const mpcgpu_dqn_params* p) {
    return p && p->lr > 0.0 && p->max_grad_norm > 0.0 && p->beta1 >= 0.0 && p->beta1 < 1.0 && p->beta2 >= 0.0 && p->beta2 < 1.0 &&
           p->eps > 0.0 && (p->double_q == 0 || p->double_q == 1);
}

Args base(const mpcgpu_dqn_params* p) {
    Args a{};
    a.lr = p->lr; a.beta1 = p->beta1; a.beta2 = p->beta2;
    a.gamma = (float)p->gamma; a.max_norm = (float)p->max_grad_norm;
    a.b1 = (float)p->beta1; a.b2 = (float)p->beta2;
    a.omb1 = (float)(1.0 - p->beta1); a.omb2 = (float)(1.0 - p->beta2);
    a.eps = (float)p->eps; a.scale = 1.0f;
    a.double_q = p->double_q; a.steps = 1; a.n = 1;
    return a;
}

// the one place that launches dqn_kernel: Tree = NoTree for the entries of mpcgpu_dqn.h, PerArgs for the prioritized launch
template <typename Tree>
int launch(abi::ErrorSlot& slot, int32_t device, const Args& a, const Tree& tr, void* stream) {
    constexpr bool PER = std::is_same_v<Tree, PerArgs>;
    if (abi::on_device(slot, device)) return -1;
    hipLaunchKernelGGL(dqn_kernel<PER>, dim3(1), dim3(NT), 0, (hipStream_t)stream, a, tr);
    return abi::launched(slot, PER ? "dqn_kernel<PER> launch" : "dqn_kernel launch");
}

int minibatch(int32_t device, const mpcgpu_dqn_params* params, float* state, const float* obs, const float* next_obs,
              const int64_t* actions, const float* rewards, const float* dones, const float* weights, int32_t n, float* grad,
              float* loss, float* td, int mode, void* stream) {
    if (!valid(params)) return fail(BAD_PARAMS);
    if (n < 1 || n > MPCGPU_DQN_MAX_ROWS) return fail("1 <= n <= 256");
    if (!state || !obs || !next_obs || !actions || !rewards || !dones || !grad || !loss) return fail("null pointer");
    Args a = base(params);
    a.state = state; a.obs = obs; a.next_obs = next_obs; a.actions = actions; a.rewards = rewards; a.dones = dones;
    a.weights = weights; a.grad_out = grad; a.loss = loss; a.td = td; a.n = n; a.mode = mode;
    return launch(g_err, device, a, NoTree{}, stream);
}

}  // namespace dqngpu

extern "C" {

int32_t mpcgpu_dqn_state_floats(void) { return MPCGPU_DQN_STATE_FLOATS; }

int32_t mpcgpu_dqn_grad_dev(int32_t device, const mpcgpu_dqn_params* params, const float* state, const float* obs,
                            const float* next_obs, const int64_t* actions, const float* rewards, const float* dones,
                            const float* weights, int32_t n, float* grad, float* loss, float* td, void* stream) {
    return dqngpu::minibatch(device, params, const_cast<float*>(state), obs, next_obs, actions, rewards, dones, weights, n, grad,
                             loss, td, dqngpu::DO_GRAD, stream);
}

int32_t mpcgpu_dqn_step_dev(int32_t device, const mpcgpu_dqn_params* params, float* state, const float* obs,
                            const float* next_obs, const int64_t* actions, const float* rewards, const float* dones,
                            const float* weights, int32_t n, float* grad, float* loss, float* td, void* stream) {
    return dqngpu::minibatch(device, params, state, obs, next_obs, actions, rewards, dones, weights, n, grad, loss, td,
                             dqngpu::DO_GRAD | dqngpu::DO_APPLY, stream);
}

int32_t mpcgpu_dqn_apply_dev(int32_t device, const mpcgpu_dqn_params* params, float* state, const float* grad, float scale,
                             void* stream) {
    using namespace dqngpu;
    if (!valid(params)) return fail(BAD_PARAMS);
    if (!state || !grad) return fail("null pointer");
    Args a = base(params);
    a.state = state; a.grad_in = grad; a.scale = scale; a.mode = DO_APPLY;
    return launch(g_err, device, a, NoTree{}, stream);
}

int32_t mpcgpu_dqn_train_dev(int32_t device, const mpcgpu_dqn_params* params, float* state, const float* buf_obs,
                             const float* buf_next_obs, const int64_t* buf_actions, const float* buf_rewards,
                             const float* buf_dones, int64_t size, int32_t n, int32_t K, uint64_t seed, uint64_t serial0,
                             float* losses, void* stream) {
    using namespace dqngpu;
    if (!valid(params)) return fail(BAD_PARAMS);
    if (n < 1 || n > MPCGPU_DQN_MAX_ROWS) return fail("1 <= n <= 256");
    if (K < 1 || K > MPCGPU_DQN_MAX_STEPS) return fail("1 <= K <= 65536");
    if (size < 1 || size >= ((int64_t)1 << 31)) return fail("1 <= size < 2^31");
    if (!state || !buf_obs || !buf_next_obs || !buf_actions || !buf_rewards || !buf_dones || !losses) return fail("null pointer");
    Args a = base(params);
    a.state = state; a.obs = buf_obs; a.next_obs = buf_next_obs; a.actions = buf_actions; a.rewards = buf_rewards;
    a.dones = buf_dones; a.size = size; a.n = n; a.steps = K; a.seed = seed; a.serial0 = serial0; a.loss = losses;
    a.mode = DO_GRAD | DO_APPLY | DO_SAMPLE;
    return launch(g_err, device, a, NoTree{}, stream);
}

const char* mpcgpu_dqn_last_error(void) { return dqngpu::g_err.text.c_str(); }

// ---- include/mpcgpu_dqn_per.h -------------------------------------------------------------------------------------------------
int32_t mpcgpu_dqn_train_per_dev(int32_t device, const mpcgpu_dqn_params* dqn, const mpcgpu_per_params* per, float* state,
                                 double* tree, const float* buf_obs, const float* buf_next_obs, const int64_t* buf_actions,
                                 const float* buf_rewards, const float* buf_dones, int64_t n_entries, int32_t n, int32_t K,
                                 uint64_t seed, uint64_t serial0, float* losses, int64_t* indices, float* td, void* stream) {
    using namespace dqngpu;
    abi::ErrorSlot& slot = g_err_per;
    if (!valid(dqn)) return slot.fail(BAD_PARAMS);
    if (!pergpu::valid(per)) return slot.fail(pergpu::BAD_PARAMS);
    if (n < 1 || n > MPCGPU_DQN_MAX_ROWS) return slot.fail("1 <= n <= 256");
    if (K < 1 || K > MPCGPU_DQN_MAX_STEPS) return slot.fail("1 <= K <= 65536");
    if (n_entries < 1 || n_entries > per->capacity) return slot.fail("1 <= n_entries <= capacity");
    if (!state || !tree || !buf_obs || !buf_next_obs || !buf_actions || !buf_rewards || !buf_dones || !losses) return slot.fail("null pointer");
    Args a = base(dqn);
    a.state = state; a.obs = buf_obs; a.next_obs = buf_next_obs; a.actions = buf_actions; a.rewards = buf_rewards;
    a.dones = buf_dones; a.n = n; a.steps = K; a.seed = seed; a.serial0 = serial0; a.loss = losses; a.td = td;
    a.mode = DO_GRAD | DO_APPLY;
    PerArgs tr{};
    tr.tree = tree; tr.indices = indices; tr.C = per->capacity; tr.n_entries = n_entries;
    tr.alpha = per->alpha; tr.beta = per->beta; tr.epsilon = per->epsilon;
    return launch(slot, device, a, tr, stream);
}

const char* mpcgpu_dqn_per_last_error(void) { return dqngpu::g_err_per.text.c_str(); }

}  // extern "C"
