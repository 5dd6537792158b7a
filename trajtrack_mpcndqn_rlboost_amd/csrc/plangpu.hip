// plangpu.hip -- batched visibility-graph shortest paths (include/mpcgpu_plan.h).
//
// One workgroup of 256 threads plans one map; everything it needs lives in LDS (about 23 KB): the ring table, the node
// list, the adjacency bit matrix (258 x 288 bits) and Dijkstra's arrays.  Phases, separated by workgroup barriers:
//   1. load the ring table; 2. one thread per vertex: is it a graph node?  threads 0 / 1: are start / goal free?
//   3. compact the nodes in table order; 4. all node pairs i < j, strided over the threads, each against every ring
//   vertex and edge; 5. Dijkstra in wavefront 0 (a node belongs to lane `index & 63`; the next node is a cross-lane
//   minimum over (distance, index)); 6. lanes 0..63 write the path.
//
// Built with -ffp-contract=off: orientation signs and distance ties follow tests/support/plan_numpy.py operation by
// operation.  The contact rule (what a collinear or touching contact means) is written down there and in DESIGN.md 8.3.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/mpcgpu_plan.h"
#include "abi_host.hpp"

namespace plangpu {

constexpr int THREADS = 256;
constexpr int VMAX = MPCGPU_PLAN_MAX_VERTICES;
constexpr int RMAX = MPCGPU_PLAN_MAX_RINGS;
constexpr int NMAX = VMAX + 2;                 // graph nodes: start, goal, ring vertices
constexpr int ADJ_WORDS = (NMAX + 31) / 32;    // 9
constexpr int PMAX = MPCGPU_PLAN_MAX_NODES;

enum : int { OK = 0, NO_PATH = 1, NOT_FREE = 2, TOO_MANY_NODES = 3, MALFORMED = 4 };

struct Rings {
    double x[VMAX], y[VMAX];
    unsigned short prev[VMAX], next[VMAX];
    unsigned char ring[VMAX], node[VMAX];
    int lo[RMAX + 1];
    int n_rings, n_vert;
};

__device__ inline double orient2d(double ax, double ay, double bx, double by, double cx, double cy) {
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

// 0 strictly outside, 1 on the outline, 2 strictly inside (even-odd) of ring vertices lo .. hi - 1
__device__ int locate(double px, double py, const Rings& R, int lo, int hi) {
    bool inside = false;
    for (int i = lo; i < hi; ++i) {
        const int j = i + 1 < hi ? i + 1 : lo;
        const double ax = R.x[i], ay = R.y[i], bx = R.x[j], by = R.y[j];
        const double o = orient2d(ax, ay, bx, by, px, py);
        if (o == 0.0 && (ax < bx ? ax : bx) <= px && px <= (ax < bx ? bx : ax) && (ay < by ? ay : by) <= py &&
            py <= (ay < by ? by : ay))
            return 1;
        if ((ay > py) != (by > py) && (o > 0.0) == (by > ay)) inside = !inside;
    }
    return inside ? 2 : 0;
}

// does direction d leave vertex v (neighbours a, b) into the forbidden open set (right of the directed outline)?
__device__ inline bool into_forbidden(double ax, double ay, double vx, double vy, double bx, double by, double dx, double dy) {
    const double e0x = vx - ax, e0y = vy - ay, e1x = bx - vx, e1y = by - vy;
    const double t = e0x * e1y - e0y * e1x;
    const double c0 = e0x * dy - e0y * dx;
    const double c1 = e1x * dy - e1y * dx;
    if (t > 0.0) return c0 < 0.0 || c1 < 0.0;
    return c0 < 0.0 && c1 < 0.0;
}

__device__ bool visible(double px, double py, double qx, double qy, const Rings& R) {
    const double dx = qx - px, dy = qy - py;
    const double len2 = dx * dx + dy * dy;
    const int nv = R.n_vert;
    for (int i = 0; i < nv; ++i) {
        const double vx = R.x[i], vy = R.y[i];
        const int a = R.prev[i], b = R.next[i];
        const double ax = R.x[a], ay = R.y[a], bx = R.x[b], by = R.y[b];
        const double si = orient2d(px, py, qx, qy, vx, vy);
        if (vx == px && vy == py) {
            if (into_forbidden(ax, ay, vx, vy, bx, by, dx, dy)) return false;
        } else if (vx == qx && vy == qy) {
            if (into_forbidden(ax, ay, vx, vy, bx, by, -dx, -dy)) return false;
        } else if (si == 0.0) {
            const double t = (vx - px) * dx + (vy - py) * dy;
            if (0.0 < t && t < len2 &&
                (into_forbidden(ax, ay, vx, vy, bx, by, dx, dy) || into_forbidden(ax, ay, vx, vy, bx, by, -dx, -dy)))
                return false;
        }
        // the edge v -> b
        const double sj = orient2d(px, py, qx, qy, bx, by);
        const double op = orient2d(vx, vy, bx, by, px, py);
        const double oq = orient2d(vx, vy, bx, by, qx, qy);
        if (((si > 0.0 && sj < 0.0) || (si < 0.0 && sj > 0.0)) && ((op > 0.0 && oq < 0.0) || (op < 0.0 && oq > 0.0)))
            return false;
        const double ex = bx - vx, ey = by - vy;
        const double e2 = ex * ex + ey * ey;
        if (op == 0.0 && oq < 0.0) {
            const double u = (px - vx) * ex + (py - vy) * ey;
            if (0.0 < u && u < e2) return false;
        }
        if (oq == 0.0 && op < 0.0) {
            const double u = (qx - vx) * ex + (qy - vy) * ey;
            if (0.0 < u && u < e2) return false;
        }
    }
    return true;
}

__device__ bool in_free_space(double px, double py, const Rings& R) {
    if (locate(px, py, R, R.lo[0], R.lo[1]) == 0) return false;
    for (int k = 1; k < R.n_rings; ++k)
        if (locate(px, py, R, R.lo[k], R.lo[k + 1]) == 2) return false;
    return true;
}

__global__ void __launch_bounds__(THREADS) plan_paths_kernel(mpcgpu_plan_params prm, int record_doubles, const double* __restrict__ rings,
                                                             const double* __restrict__ start_goal, int32_t* __restrict__ status,
                                                             int32_t* __restrict__ n_nodes, double* __restrict__ nodes,
                                                             double* __restrict__ length) {
    __shared__ Rings R;
    __shared__ double nx[NMAX], ny[NMAX], dist[NMAX];
    __shared__ unsigned int adj[NMAX * ADJ_WORDS];
    __shared__ short parent[NMAX];
    __shared__ unsigned char done[NMAX];
    __shared__ short order[PMAX];
    __shared__ int s_free[2], s_status, s_count;
    __shared__ double s_length;

    const int tid = threadIdx.x;
    const int64_t map = blockIdx.x;
    const double* rec = rings + map * record_doubles;
    int32_t* out_status = status + map;
    int32_t* out_n = n_nodes + map;
    double* out_nodes = nodes + map * (2 * PMAX);
    double* out_len = length + map;

    // ---- 1. the ring table --------------------------------------------------------------------------------------------
    if (tid == 0) {
        const double fr = rec[0], fv = rec[1];
        int bad = !(fr >= 1.0 && fr <= (double)prm.n_ring_max && fv >= 3.0 && fv <= (double)prm.n_vert_max);
        int nr = bad ? 0 : (int)fr, total = 0;
        R.lo[0] = 0;
        for (int k = 0; k < nr; ++k) {
            const double fn = rec[2 + k];
            if (!(fn >= 3.0 && fn <= (double)prm.n_vert_max) || total + (int)fn > prm.n_vert_max) { bad = 1; break; }
            total += (int)fn;
            R.lo[k + 1] = total;
        }
        if (!bad && total != (int)fv) bad = 1;
        R.n_rings = nr;
        R.n_vert = bad ? 0 : total;
        s_status = bad ? MALFORMED : OK;
        s_count = 0;
        s_length = 0.0;
    }
    __syncthreads();
    if (s_status == MALFORMED) {
        if (tid == 0) { *out_status = MALFORMED; *out_n = 0; *out_len = 0.0; }
        if (tid < 2 * PMAX) out_nodes[tid] = 0.0;
        return;
    }
    const int nv = R.n_vert, nr = R.n_rings;
    const double* xy = rec + 2 + prm.n_ring_max;
    if (tid < nv) {
        int k = 0;
        while (tid >= R.lo[k + 1]) ++k;
        const int lo = R.lo[k], hi = R.lo[k + 1];
        R.x[tid] = xy[2 * tid];
        R.y[tid] = xy[2 * tid + 1];
        R.ring[tid] = (unsigned char)k;
        R.prev[tid] = (unsigned short)(tid > lo ? tid - 1 : hi - 1);
        R.next[tid] = (unsigned short)(tid + 1 < hi ? tid + 1 : lo);
    }
    __syncthreads();

    // ---- 2. which vertices are nodes; are start and goal free ---------------------------------------------------------
    const double sx = start_goal[4 * map], sy = start_goal[4 * map + 1], gx = start_goal[4 * map + 2], gy = start_goal[4 * map + 3];
    if (tid < nv) {
        const int a = R.prev[tid], b = R.next[tid], k = R.ring[tid];
        const double vx = R.x[tid], vy = R.y[tid];
        const double turn = (vx - R.x[a]) * (R.y[b] - vy) - (vy - R.y[a]) * (R.x[b] - vx);
        bool is_node = turn < 0.0;
        if (is_node && k != 0 && locate(vx, vy, R, R.lo[0], R.lo[1]) == 0) is_node = false;
        for (int m = 1; is_node && m < nr; ++m)
            if (m != k && locate(vx, vy, R, R.lo[m], R.lo[m + 1]) == 2) is_node = false;
        R.node[tid] = is_node ? 1 : 0;
    }
    if (tid >= THREADS - 2) {          // the last two threads: they rarely own a vertex
        const int w = tid - (THREADS - 2);
        s_free[w] = in_free_space(w == 0 ? sx : gx, w == 0 ? sy : gy, R) ? 1 : 0;
    }
    __syncthreads();
    if (!(s_free[0] && s_free[1])) {
        if (tid == 0) { *out_status = NOT_FREE; *out_n = 0; *out_len = 0.0; }
        if (tid < 2 * PMAX) out_nodes[tid] = 0.0;
        return;
    }

    // ---- 3. the node list: start, goal, then the node vertices in table order -------------------------------------------
    int N = 2;
    for (int i = 0; i < nv; ++i) N += R.node[i];
    if (tid < nv && R.node[tid]) {
        int rank = 2;
        for (int i = 0; i < tid; ++i) rank += R.node[i];
        nx[rank] = R.x[tid];
        ny[rank] = R.y[tid];
    }
    if (tid == 0) { nx[0] = sx; ny[0] = sy; nx[1] = gx; ny[1] = gy; }
    for (int i = tid; i < N * ADJ_WORDS; i += THREADS) adj[i] = 0u;
    __syncthreads();

    // ---- 4. visibility of every pair i < j ------------------------------------------------------------------------------
    for (int t = tid; t < N * N; t += THREADS) {
        const int i = t / N, j = t - i * N;
        if (i >= j) continue;
        if (visible(nx[i], ny[i], nx[j], ny[j], R)) {
            atomicOr(&adj[i * ADJ_WORDS + (j >> 5)], 1u << (j & 31));
            atomicOr(&adj[j * ADJ_WORDS + (i >> 5)], 1u << (i & 31));
        }
    }
    __syncthreads();

    // ---- 5. Dijkstra in wavefront 0 ---------------------------------------------------------------------------------------
    if (tid < 64) {
        const int lane = tid;
        for (int k = lane; k < N; k += 64) {
            dist[k] = k == 0 ? 0.0 : INFINITY;
            parent[k] = -1;
            done[k] = 0;
        }
        int result = NO_PATH;
        for (int round = 0; round < N; ++round) {
            double best = INFINITY;
            int u = INT_MAX;
            for (int k = lane; k < N; k += 64)
                if (!done[k] && dist[k] < best) { best = dist[k]; u = k; }
            for (int off = 32; off > 0; off >>= 1) {
                const double ob = __shfl_xor(best, off, 64);
                const int ou = __shfl_xor(u, off, 64);
                if (ob < best || (ob == best && ou < u)) { best = ob; u = ou; }
            }
            if (u == INT_MAX) break;                      // nothing reachable is left
            if (u == 1) { result = OK; break; }
            if ((u & 63) == lane) done[u] = 1;
            const double ux = nx[u], uy = ny[u];
            const unsigned int* row = &adj[u * ADJ_WORDS];
            for (int k = lane; k < N; k += 64) {
                if (done[k] || k == u || !((row[k >> 5] >> (k & 31)) & 1u)) continue;
                const double ddx = nx[k] - ux, ddy = ny[k] - uy;
                const double nd = best + sqrt(ddx * ddx + ddy * ddy);
                if (nd < dist[k]) { dist[k] = nd; parent[k] = (short)u; }
            }
        }
        // the owners' parent[] writes must be visible to lane 0 (one wavefront: an LDS fence is enough)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane == 0) {
            int count = 0;
            if (result == OK) {
                count = 1;
                for (int k = 1; k != 0 && count <= N; k = parent[k]) ++count;
                if (count > prm.n_node_max) result = TOO_MANY_NODES;
            }
            double len = 0.0;
            if (result == OK) {
                int k = 1;
                for (int pos = count - 1; pos >= 0; --pos) { order[pos] = (short)k; k = parent[k]; }
                for (int pos = 0; pos + 1 < count; ++pos) {
                    const double ddx = nx[order[pos + 1]] - nx[order[pos]], ddy = ny[order[pos + 1]] - ny[order[pos]];
                    len = len + sqrt(ddx * ddx + ddy * ddy);
                }
            }
            s_status = result;
            s_count = result == NO_PATH ? 0 : count;
            s_length = len;
        }
    }
    __syncthreads();

    // ---- 6. output ---------------------------------------------------------------------------------------------------------
    if (tid < PMAX) {
        const bool have = s_status == OK && tid < s_count;
        out_nodes[2 * tid] = have ? nx[order[tid]] : 0.0;
        out_nodes[2 * tid + 1] = have ? ny[order[tid]] : 0.0;
    }
    if (tid == 0) { *out_status = s_status; *out_n = s_count; *out_len = s_length; }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
thread_local abi::ErrorSlot g_err;
int fail(const char* what) { return g_err.fail(what); }

int check(const mpcgpu_plan_params* p) {
    if (!p) return fail("null mpcgpu_plan_params");
    if (p->n_vert_max < 3 || p->n_vert_max > MPCGPU_PLAN_MAX_VERTICES) return fail("plan: at most 256 ring vertices per map (3 <= n_vert_max <= 256)");
    if (p->n_ring_max < 1 || p->n_ring_max > MPCGPU_PLAN_MAX_RINGS) return fail("plan: at most 32 rings per map (1 <= n_ring_max <= 32)");
    if (p->n_node_max < 2 || p->n_node_max > MPCGPU_PLAN_MAX_NODES) return fail("plan: at most 64 path nodes (2 <= n_node_max <= 64)");
    return 0;
}

int record_doubles(const mpcgpu_plan_params* p) {
    const int r = 2 + p->n_ring_max + 2 * p->n_vert_max;
    return r + (r & 1);
}

}  // namespace plangpu

extern "C" {

int32_t mpcgpu_plan_record_doubles(const mpcgpu_plan_params* params) {
    if (plangpu::check(params)) return -1;
    return plangpu::record_doubles(params);
}

int32_t mpcgpu_plan_paths_dev(int32_t device, const mpcgpu_plan_params* params, int32_t B, const double* rings,
                              const double* start_goal, int32_t* status, int32_t* n_nodes, double* nodes, double* length,
                              void* stream) {
    using namespace plangpu;
    if (check(params)) return -1;
    if (B < 1) return fail("plan: B >= 1");
    if (!rings || !start_goal || !status || !n_nodes || !nodes || !length) return fail("null pointer");
    if (abi::on_device(g_err, device)) return -1;
    hipLaunchKernelGGL(plan_paths_kernel, dim3((unsigned)B), dim3(THREADS), 0, (hipStream_t)stream, *params, record_doubles(params), rings,
                       start_goal, status, n_nodes, nodes, length);
    return abi::launched(g_err, "plan_paths_kernel launch");
}

const char* mpcgpu_plan_last_error(void) { return plangpu::g_err.text.c_str(); }

}  // extern "C"
