// mapgpu.hip -- device side of the per-episode map stream for gfx950 (MI355X): C-ABI of include/mpcgpu_map.h.
//
// One wavefront = one map, grid = B, three kernels that a refill runs around the planner (csrc/plangpu.hip):
//   map_draw_kernel    the 71 counter-based draws of generate_map_dynamic (utils/map.py:158-189 as restated by
//                      rl_env.random_dynamic_spec) -> spec record; host twin map_stream.spec_of + pack_specs
//   map_rings_kernel   spec -> the planner's ring record and start / goal; host twin path_plan.inflate_spec + oriented_rings +
//                      pack_rings (lanes over the vertices of one ring, rings in turn)
//   map_record_kernel  spec + planned path -> environment record in the row's spare slot; host twin rl_env.make_map +
//                      pack_records (lanes over vertices, obstacles and edges; the drop of near-duplicate points on one lane)
// The first two agree with their twins bit for bit and the third in everything but outline coordinates behind cos / sin / atan2 /
// acos / hypot: every operation below is the one Python performs, in its order, and the file is compiled without contraction
// (MAP_FLAGS).  Specs, records and outline nodes are staged in LDS; no kernel uses scratch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mpcgpu_map.h"
#include "counter_stream.hpp"
#include "envgpu_internal.hpp"

namespace mapgpu {

constexpr int WAVE = 64;
constexpr int SPEC = MPCGPU_MAP_SPEC_DOUBLES;
constexpr int O_BOUNDARY = 16;
constexpr int O_STATIC = O_BOUNDARY + 2 * MPCGPU_MAP_MAX_BOUNDARY;
constexpr int STATIC_STRIDE = 2 + 2 * MPCGPU_MAP_MAX_STATIC_VERTS;
constexpr int O_PERIODIC = O_STATIC + MPCGPU_MAP_MAX_STATIC * STATIC_STRIDE;
constexpr int PERIODIC_STRIDE = 8;
static_assert(SPEC == O_PERIODIC + MPCGPU_MAP_MAX_PERIODIC * PERIODIC_STRIDE, "spec layout");

constexpr int N_STATIC = 3, N_PERIODIC = 7;   // generate_map_dynamic: ten obstacles, the first three are boxes

// draw k of the map with key `key`: lo + (hi - lo) * u_k, as CounterUniform.uniform (two rounded operations: MAP_FLAGS)
__device__ __forceinline__ double uniform(uint64_t key, int k, double lo, double hi) {
    const double u = counter_stream::unit(COUNTER_STREAM_DRAW(key, (uint64_t)(k + 1)));
    return lo + (hi - lo) * u;
}

__global__ __launch_bounds__(WAVE) void map_draw_kernel(uint64_t seed, double* __restrict__ spec_all,
                                                        const int32_t* __restrict__ spare_ready, int32_t* attempt, int B) {
    __shared__ double spec[SPEC];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B || spare_ready[b] != 0) return;          // uniform: the whole workgroup leaves
    const int n = attempt[b];
    const uint64_t serial = (uint64_t)b + (uint64_t)B * (uint64_t)n;
    const uint64_t key = counter_stream::key_of(seed, serial);
    for (int i = lane; i < SPEC; i += WAVE) spec[i] = 0.0;
    __syncthreads();
    const double two_pi = 2.0 * 3.141592653589793;
    // draws 0, 1: start; 2 .. 13: four per box; 14 .. 69: eight per periodic obstacle; 70: goal
    if (lane < N_STATIC) {
        const int k = 2 + 4 * lane;
        const double x = uniform(key, k, 10.0, 30.0), y = uniform(key, k + 1, 0.0, 20.0);
        const double w = fmax(4.0, uniform(key, k + 2, 0.0, 0.5 * fmin(x - 10.0, 30.0 - x)));
        const double h = fmax(4.0, uniform(key, k + 3, 0.0, fmin(y, 20.0 - y)));
        const double x0 = x - w / 2.0, y0 = y - h / 2.0;
        double* s = spec + O_STATIC + lane * STATIC_STRIDE;
        s[0] = 4.0;
        s[2] = x0;     s[3] = y0;
        s[4] = x0 + w; s[5] = y0;
        s[6] = x0 + w; s[7] = y0 + h;
        s[8] = x0;     s[9] = y0 + h;
    } else if (lane < N_STATIC + N_PERIODIC) {
        const int k = 2 + 4 * N_STATIC + 8 * (lane - N_STATIC);
        const double x = uniform(key, k, 10.0, 30.0), y = uniform(key, k + 1, 0.0, 20.0);
        double* d = spec + O_PERIODIC + (lane - N_STATIC) * PERIODIC_STRIDE;
        d[0] = x; d[1] = y;
        d[2] = x + uniform(key, k + 2, -5.0, 5.0);
        d[3] = y + uniform(key, k + 3, -5.0, 5.0);
        d[5] = uniform(key, k + 4, 0.2, 1.2);   // rx
        d[6] = uniform(key, k + 5, 0.2, 1.2);   // ry
        d[4] = uniform(key, k + 6, 0.3, 0.7);   // freq
        d[7] = uniform(key, k + 7, 0.0, two_pi);
    } else if (lane == N_STATIC + N_PERIODIC) {
        spec[0] = 5.0;
        spec[1] = uniform(key, 0, 5.0, 15.0);
        spec[2] = uniform(key, 1, 0.0, two_pi);
        spec[5] = 35.0;
        spec[6] = uniform(key, 2 + 4 * N_STATIC + 8 * N_PERIODIC, 5.0, 15.0);
        spec[7] = 4.0; spec[8] = (double)N_STATIC; spec[9] = (double)N_PERIODIC;
        double* bd = spec + O_BOUNDARY;           // the 40 x 20 m hall
        bd[2] = 40.0; bd[4] = 40.0; bd[5] = 20.0; bd[7] = 20.0;
        attempt[b] = n + 1;
    }
    __syncthreads();
    double* out = spec_all + (size_t)b * SPEC;
    for (int i = lane; i < SPEC; i += WAVE) out[i] = spec[i];
}

// ---- rings: what path_plan.inflate_spec + oriented_rings + pack_rings make of a spec -----------------------------------------
constexpr int RING_USED = 2 + MPCGPU_MAP_RING_MAX + 2 * MPCGPU_MAP_VERT_MAX;
constexpr int RING_REC = RING_USED + (RING_USED & 1);   // mpcgpu_plan_record_doubles: padded to an even number of doubles
constexpr int MAXV = MPCGPU_MAP_MAX_BOUNDARY;   // vertices of the largest input ring
static_assert(MPCGPU_MAP_MAX_STATIC_VERTS <= MAXV && MAXV <= WAVE, "one lane per ring vertex");

// rl_geometry.signed_area > 0, summed in vertex order (uniform: every lane walks the ring in LDS).  numpy sums long rings pairwise;
// the sign can differ only for an area within rounding of zero, which no polygon with an interior has.
__device__ __forceinline__ bool area_positive(const double (*p)[2], int n) {
    double a = 0.0;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 < n ? i + 1 : 0;
        a += p[i][0] * p[j][1] - p[j][0] * p[i][1];
    }
    return 0.5 * a > 0.0;
}

// rl_geometry.mitre_polygon(ring, distance, mitre_limit = 2, check = False) for vertex `lane` of the counter-clockwise ring p[0..n):
// the one or two offset points of that vertex; returns their number.  Operation for operation the host's float64 arithmetic.
struct Mitre { double x0, y0, x1, y1; int cnt; };
__device__ __forceinline__ Mitre mitre_vertex(const double (*p)[2], int n, int i, double distance) {
    Mitre o{0.0, 0.0, 0.0, 0.0, 1};
    const double r = fabs(distance), sgn = distance > 0.0 ? 1.0 : -1.0, limit = 2.0 * r;
    const int ip = i > 0 ? i - 1 : n - 1, in = i + 1 < n ? i + 1 : 0;
    const double vx = p[i][0], vy = p[i][1];
    double d0x = vx - p[ip][0], d0y = vy - p[ip][1], d1x = p[in][0] - vx, d1y = p[in][1] - vy;
    const double l0 = sqrt(d0x * d0x + d0y * d0y), l1 = sqrt(d1x * d1x + d1y * d1y);
    d0x = d0x / l0; d0y = d0y / l0; d1x = d1x / l1; d1y = d1y / l1;
    const double n0x = sgn * d0y, n0y = sgn * -d0x, n1x = sgn * d1y, n1y = sgn * -d1x;
    const double turn = d0x * d1y - d0y * d1x;
    const double c = n0x * n1x + n0y * n1y;
    if (fabs(turn) < 1e-14 && c > 0.0) {                     // collinear: one offset point
        o.x0 = vx + r * n0x; o.y0 = vy + r * n0y;
        return o;
    }
    if (turn * sgn > 0.0 && r * sqrt(2.0 / (1.0 + c)) > limit) {   // the mitre would reach past the limit: bevel
        double mx = n0x + n1x, my = n0y + n1y;
        const double lm = sqrt(mx * mx + my * my);
        mx = mx / lm; my = my / lm;
        const double tx = -my, ty = mx;
        const double s0 = (r - limit * (mx * n0x + my * n0y)) / (tx * n0x + ty * n0y);
        const double s1 = (r - limit * (mx * n1x + my * n1y)) / (tx * n1x + ty * n1y);
        o.x0 = vx + limit * mx + s0 * tx; o.y0 = vy + limit * my + s0 * ty;
        o.x1 = vx + limit * mx + s1 * tx; o.y1 = vy + limit * my + s1 * ty;
        o.cnt = 2;
        return o;
    }
    o.x0 = vx + r * (n0x + n1x) / (1.0 + c); o.y0 = vy + r * (n0y + n1y) / (1.0 + c);
    return o;
}

__global__ __launch_bounds__(WAVE) void map_rings_kernel(const double* __restrict__ spec_all, const int32_t* __restrict__ spare_ready,
                                                         double* __restrict__ rings_all, double* __restrict__ start_goal, int B) {
    __shared__ double spec[SPEC];
    __shared__ double rec[RING_REC];
    __shared__ double raw[MAXV][2], poly[MAXV][2];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    double* out = rings_all + (size_t)b * RING_REC;
    if (spare_ready[b] != 0) {                               // skipped row: no rings, the planner answers status 4
        if (lane == 0) out[0] = 0.0;
        return;
    }
    for (int i = lane; i < SPEC; i += WAVE) spec[i] = spec_all[(size_t)b * SPEC + i];
    for (int i = lane; i < RING_REC; i += WAVE) rec[i] = 0.0;
    __syncthreads();
    const int n_static = min(max((int)spec[8], 0), MPCGPU_MAP_MAX_STATIC);   // (counts are clamped to the table: no index leaves it)
    int total = 0;                                           // ring vertices written so far (uniform)
    for (int ring = 0; ring <= n_static; ++ring) {
        const double* src = ring == 0 ? spec + O_BOUNDARY : spec + O_STATIC + (ring - 1) * STATIC_STRIDE + 2;
        const int n = min(max(ring == 0 ? (int)spec[7] : (int)spec[O_STATIC + (ring - 1) * STATIC_STRIDE], 0),
                          ring == 0 ? MPCGPU_MAP_MAX_BOUNDARY : MPCGPU_MAP_MAX_STATIC_VERTS);
        const double distance = ring == 0 ? -0.5 : 0.8;      // environment.py:130-140: boundary shrunk, obstacles grown
        if (lane < n) { raw[lane][0] = src[2 * lane]; raw[lane][1] = src[2 * lane + 1]; }
        __syncthreads();
        // rl_geometry.orient (counter-clockwise), the float32 pass, and mitre_polygon's own orient of the rounded ring
        const bool keep = area_positive(raw, n);
        if (lane < n) {
            const int j = keep ? lane : n - 1 - lane;
            poly[lane][0] = (double)(float)raw[j][0]; poly[lane][1] = (double)(float)raw[j][1];
        }
        __syncthreads();
        if (!area_positive(poly, n)) {
            double qx = 0.0, qy = 0.0;
            if (lane < n) { qx = poly[n - 1 - lane][0]; qy = poly[n - 1 - lane][1]; }
            __syncthreads();
            if (lane < n) { poly[lane][0] = qx; poly[lane][1] = qy; }
            __syncthreads();
        }
        Mitre pt{0.0, 0.0, 0.0, 0.0, 0};
        if (lane < n) pt = mitre_vertex(poly, n, lane, distance);
        const int cnt = pt.cnt;
        const unsigned long long two = __ballot(cnt == 2);
        const int m = n + __popcll(two);                     // vertices of the offset ring
        if (lane < n) {
            const int at = lane + __popcll(two & ((1ull << lane) - 1ull));
            // the offset ring is counter-clockwise: the boundary stays, an obstacle is stored clockwise (oriented_rings)
            double* xy = rec + 2 + MPCGPU_MAP_RING_MAX + 2 * total;
            const int i0 = ring == 0 ? at : m - 1 - at;
            xy[2 * i0] = pt.x0; xy[2 * i0 + 1] = pt.y0;
            if (cnt == 2) {
                const int i1 = ring == 0 ? at + 1 : m - 2 - at;
                xy[2 * i1] = pt.x1; xy[2 * i1 + 1] = pt.y1;
            }
        }
        if (lane == 0) rec[2 + ring] = (double)m;
        total += m;
        __syncthreads();
    }
    if (lane == 0) { rec[0] = (double)(n_static + 1); rec[1] = (double)total; }
    __syncthreads();
    for (int i = lane; i < RING_REC; i += WAVE) out[i] = rec[i];
    if (lane < 2) start_goal[(size_t)b * 4 + lane] = spec[lane];                              // start x, y
    else if (lane < 4) start_goal[(size_t)b * 4 + lane] = (double)(float)spec[5 + lane - 2];  // goal through float32
}

// ---- records: what rl_env.pack_records([make_map(path = planned nodes, **spec)], limits = the table's) writes --------------------
constexpr int MAX_OUTLINES = 1 + MPCGPU_MAP_MAX_STATIC + MPCGPU_MAP_MAX_PERIODIC;
constexpr int NODE_CAP = MPCGPU_MAP_MAX_EDGES;   // outline nodes (= edges) of one map that are staged in LDS
constexpr int PER_VERTEX = 9;                    // offset points of one vertex: both edge ends and the fillet's inner points, nseg <= 8
constexpr int TMP = MAXV * PER_VERTEX;
constexpr int HEAD_CAP = 16 + 4 * 64 + 31 * (4 + 5 + 12);   // everything in front of the edge table at P = 64, M = 31, K = 4
constexpr int CORNERS = 12;                      // obstacle.py:193-199

__global__ __launch_bounds__(WAVE) void map_record_kernel(envgpu::EnvK k, const double* __restrict__ spec_all,
                                                          const int32_t* __restrict__ plan_status, const int32_t* __restrict__ plan_n,
                                                          const double* __restrict__ plan_nodes, double* records2,
                                                          const int32_t* __restrict__ which, int32_t* spare_ready, int32_t* status,
                                                          int B) {
    __shared__ double spec[SPEC];
    __shared__ double head[HEAD_CAP];
    __shared__ double nodes[NODE_CAP][2];
    __shared__ double tmp[TMP][2];
    __shared__ double raw[MAXV][2], poly[MAXV][2];
    __shared__ int cntv[MAXV];
    __shared__ int ostart[MAX_OUTLINES + 1];
    __shared__ int overflow;
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    if (spare_ready[b] != 0) {                               // skipped row
        if (lane == 0) status[b] = -1;
        return;
    }
    const int ps = plan_status[b];
    if (ps != 0) {                                           // no path: the row draws again at the next refill
        if (lane == 0) status[b] = ps;
        return;
    }
    const mpcgpu_env_params& P = k.p;
    for (int i = lane; i < SPEC; i += WAVE) spec[i] = spec_all[(size_t)b * SPEC + i];
    for (int i = lane; i < k.o_edge; i += WAVE) head[i] = 0.0;
    if (lane == 0) { overflow = 0; ostart[0] = 0; }
    __syncthreads();
    const int nb = min(max((int)spec[7], 0), MPCGPU_MAP_MAX_BOUNDARY);
    const int ns = min(max((int)spec[8], 0), MPCGPU_MAP_MAX_STATIC);
    const int nd = min(max((int)spec[9], 0), MPCGPU_MAP_MAX_PERIODIC);
    const int n_path = plan_n[b];
    const double r = P.radius;
    const double quantum = 3.141592653589793 / 2.0 / 4.0;    // buffer_polygon: quad_segs = 4
    const double two_pi = 2.0 * 3.141592653589793;
    int total = 0;
    for (int o = 0; o < 1 + ns + nd; ++o) {
        const bool periodic = o > ns;
        const double sgn = o == 0 ? -1.0 : 1.0;              // the boundary shrinks, obstacles grow
        int n;
        if (periodic) {                                      // rl_geometry.ellipse_nodes(rx, ry, 12)
            const double* d = spec + O_PERIODIC + (o - 1 - ns) * PERIODIC_STRIDE;
            n = CORNERS;
            if (lane < n) {
                const double a = two_pi * (double)lane / (double)CORNERS;
                raw[lane][0] = d[5] * cos(a); raw[lane][1] = -d[6] * sin(a);
            }
        } else {
            const double* src = o == 0 ? spec + O_BOUNDARY : spec + O_STATIC + (o - 1) * STATIC_STRIDE + 2;
            n = o == 0 ? nb : min(max((int)spec[O_STATIC + (o - 1) * STATIC_STRIDE], 0), MPCGPU_MAP_MAX_STATIC_VERTS);
            if (lane < n) { raw[lane][0] = src[2 * lane]; raw[lane][1] = src[2 * lane + 1]; }
        }
        __syncthreads();
        // orient (not for the ellipse: obstacle.py rounds its nodes as they come), float32, and buffer_polygon's own orient
        const bool keep = periodic ? true : area_positive(raw, n);
        if (lane < n) {
            const int j = keep ? lane : n - 1 - lane;
            poly[lane][0] = (double)(float)raw[j][0]; poly[lane][1] = (double)(float)raw[j][1];
        }
        __syncthreads();
        if (!area_positive(poly, n)) {
            double qx = 0.0, qy = 0.0;
            if (lane < n) { qx = poly[n - 1 - lane][0]; qy = poly[n - 1 - lane][1]; }
            __syncthreads();
            if (lane < n) { poly[lane][0] = qx; poly[lane][1] = qy; }
            __syncthreads();
        }
        // rl_geometry.buffer_polygon(poly, sgn * r, quad_segs = 4, check = False), vertex `lane`
        int cnt = 0, nseg = 0;
        double vx = 0.0, vy = 0.0, n0x = 0.0, n0y = 0.0, n1x = 0.0, n1y = 0.0, a0 = 0.0, inc = 0.0, dot = 0.0;
        bool fillet = false, collinear = false;
        if (lane < n) {
            const int ip = lane > 0 ? lane - 1 : n - 1, in = lane + 1 < n ? lane + 1 : 0;
            vx = poly[lane][0]; vy = poly[lane][1];
            double d0x = vx - poly[ip][0], d0y = vy - poly[ip][1], d1x = poly[in][0] - vx, d1y = poly[in][1] - vy;
            const double l0 = hypot(d0x, d0y), l1 = hypot(d1x, d1y);
            d0x = d0x / l0; d0y = d0y / l0; d1x = d1x / l1; d1y = d1y / l1;
            n0x = sgn * d0y; n0y = sgn * -d0x; n1x = sgn * d1y; n1y = sgn * -d1x;
            const double turn = d0x * d1y - d0y * d1x;
            dot = n0x * n1x + n0y * n1y;
            cnt = 1;
            if (fabs(turn) < 1e-14) {
                collinear = true;
            } else if (turn * sgn > 0.0) {                   // the corner opens on the offset side: fillet around the vertex
                fillet = true;
                a0 = atan2(n0y, n0x);
                const double tot = acos(fmax(-1.0, fmin(1.0, dot)));
                nseg = (int)(tot / quantum + 0.5);
                if (nseg >= 1) inc = tot / (double)nseg * (turn > 0.0 ? 1.0 : -1.0);
                cnt = nseg >= 1 ? nseg + 1 : 2;
                if (cnt > PER_VERTEX) cnt = PER_VERTEX;      // (tot <= pi gives nseg <= 8)
            }
            cntv[lane] = cnt;
        }
        __syncthreads();
        int at = 0, m_all = 0;
        for (int i = 0; i < n; ++i) { if (i < lane) at += cntv[i]; m_all += cntv[i]; }
        if (lane < n) {
            if (fillet) {
                tmp[at][0] = vx + r * n0x; tmp[at][1] = vy + r * n0y;
                for (int q = 1; q < cnt - 1; ++q) {
                    const double a = a0 + (double)q * inc;
                    tmp[at + q][0] = vx + r * cos(a); tmp[at + q][1] = vy + r * sin(a);
                }
                tmp[at + cnt - 1][0] = vx + r * n1x; tmp[at + cnt - 1][1] = vy + r * n1y;
            } else if (collinear) {
                tmp[at][0] = vx + r * n0x; tmp[at][1] = vy + r * n0y;
            } else {                                         // the offset edges meet: their intersection
                tmp[at][0] = vx + r * (n0x + n1x) / (1.0 + dot); tmp[at][1] = vy + r * (n0y + n1y) / (1.0 + dot);
            }
        }
        __syncthreads();
        // the sequential drop of (near-)duplicate points, then the float32 pass of obstacle outlines (the boundary stays float64)
        if (lane == 0) {
            const double thr = 1e-6 * r;
            int kept = 0;
            double fx = 0.0, fy = 0.0, lx = 0.0, ly = 0.0;
            for (int i = 0; i < m_all; ++i) {
                const double px = tmp[i][0], py = tmp[i][1];
                if (i == 0 || hypot(px - lx, py - ly) > thr) {
                    if (i == 0) { fx = px; fy = py; }
                    lx = px; ly = py;
                    if (total + kept < NODE_CAP) {
                        nodes[total + kept][0] = o == 0 ? px : (double)(float)px;
                        nodes[total + kept][1] = o == 0 ? py : (double)(float)py;
                    } else {
                        overflow = 1;
                    }
                    ++kept;
                }
            }
            if (kept > 1 && hypot(lx - fx, ly - fy) <= thr) --kept;
            ostart[o + 1] = total + kept;
        }
        __syncthreads();
        total = ostart[o + 1];
    }
    const int n_obst = ns + nd;
    const bool fits = n_path >= 2 && n_path <= P.n_path_max && n_obst <= P.n_obst_max && (nd > 0 ? 2 : 1) <= P.n_kf_max &&
                      total <= P.n_edge_max && overflow == 0;
    if (!fits) {
        if (lane == 0) status[b] = 5;
        return;
    }
    // ---- header, path, animation blocks: staged in LDS, every double of the record is then written exactly once
    const double* pn = plan_nodes + (size_t)b * MPCGPU_PLAN_MAX_NODES * 2;
    if (lane < n_path) { head[k.o_xy + 2 * lane] = pn[2 * lane]; head[k.o_xy + 2 * lane + 1] = pn[2 * lane + 1]; }
    if (lane == 0) {
        head[0] = (double)n_path; head[1] = (double)n_obst; head[2] = (double)total;
        head[3] = (double)(float)spec[5]; head[4] = (double)(float)spec[6];
        for (int i = 0; i < 5; ++i) head[5 + i] = spec[i];
        double cum = 0.0;                                    // rl_env.path_lengths: summed in path order
        for (int i = 0; i + 1 < n_path; ++i) {
            const double dx = pn[2 * i + 2] - pn[2 * i], dy = pn[2 * i + 3] - pn[2 * i + 1];
            const double seg = sqrt(dx * dx + dy * dy);
            head[k.o_len + i] = seg;
            cum = cum + seg;
            head[k.o_cum + i + 1] = cum;
        }
    }
    if (lane < n_obst) {
        double* a = head + k.o_anim + lane * k.an;
        double* kf = a + 4 + (P.n_kf_max + 1);
        if (lane < ns) {                                     // rl_env.static_obstacle: one key frame at the origin, linear
            a[2] = 1.0; a[3] = 1.0; a[5] = 1.0;
        } else {                                             // rl_env.periodic_obstacle
            const double* d = spec + O_PERIODIC + (lane - ns) * PERIODIC_STRIDE;
            const double step = d[4] != 0.0 ? 3.141592653589793 / d[4] : 1.0;
            // the reference builds the key frames with the LAST node angle, not the caller's (obstacle.py:196-198): kept
            const double rot = two_pi * (double)(CORNERS - 1) / (double)CORNERS;
            a[0] = 1.0; a[2] = 2.0; a[3] = step + step; a[5] = step; a[6] = step;
            kf[0] = (double)(float)d[0]; kf[1] = (double)(float)d[1]; kf[2] = rot;
            kf[3] = (double)(float)d[2]; kf[4] = (double)(float)d[3]; kf[5] = rot;
        }
    }
    __syncthreads();
    double* rec = records2 + ((size_t)(1 - which[b]) * B + b) * k.rec;
    for (int i = lane; i < k.o_edge; i += WAVE) rec[i] = head[i];
    for (int e = lane; e < P.n_edge_max; e += WAVE) {
        double* ed = rec + k.o_edge + 5 * e;
        if (e < total) {
            int o = 0;
            while (e >= ostart[o + 1]) ++o;
            const int nx = e + 1 < ostart[o + 1] ? e + 1 : ostart[o];
            ed[0] = nodes[e][0]; ed[1] = nodes[e][1]; ed[2] = nodes[nx][0]; ed[3] = nodes[nx][1]; ed[4] = (double)(o - 1);
        } else {
            ed[0] = 0.0; ed[1] = 0.0; ed[2] = 0.0; ed[3] = 0.0; ed[4] = -2.0;
        }
    }
    if (lane == 0) {
        if (k.o_edge + 5 * P.n_edge_max < k.rec) rec[k.rec - 1] = 0.0;   // the record's padding to an even length
        status[b] = 0;
        spare_ready[b] = 1;
    }
}

thread_local abi::ErrorSlot g_err;
int fail(const char* what) { return g_err.fail(what); }

}  // namespace mapgpu

extern "C" {

int32_t mpcgpu_map_spec_doubles(void) { return mapgpu::SPEC; }

int32_t mpcgpu_map_draw_dev(int32_t device, int32_t B, uint64_t seed, double* spec_table, const int32_t* spare_ready,
                            int32_t* attempt, void* stream) {
    if (B < 0 || !spec_table || !spare_ready || !attempt) return mapgpu::fail("null pointer / negative batch");
    if (B == 0) return 0;
    if (abi::on_device(mapgpu::g_err, device)) return -1;
    hipLaunchKernelGGL(mapgpu::map_draw_kernel, dim3(B), dim3(mapgpu::WAVE), 0, (hipStream_t)stream, seed, spec_table,
                       spare_ready, attempt, (int)B);
    return abi::launched(mapgpu::g_err, "map_draw_kernel launch");
}

int32_t mpcgpu_map_rings_dev(int32_t device, int32_t B, const double* spec_table, const int32_t* spare_ready, double* rings,
                             double* start_goal, void* stream) {
    if (B < 0 || !spec_table || !spare_ready || !rings || !start_goal) return mapgpu::fail("null pointer / negative batch");
    if (B == 0) return 0;
    if (abi::on_device(mapgpu::g_err, device)) return -1;
    hipLaunchKernelGGL(mapgpu::map_rings_kernel, dim3(B), dim3(mapgpu::WAVE), 0, (hipStream_t)stream, spec_table, spare_ready,
                       rings, start_goal, (int)B);
    return abi::launched(mapgpu::g_err, "map_rings_kernel launch");
}

int32_t mpcgpu_map_record_dev(int32_t device, const mpcgpu_env_params* params, int32_t B, const double* spec_table,
                              const int32_t* plan_status, const int32_t* plan_n_nodes, const double* plan_nodes, double* records2,
                              const int32_t* which, int32_t* spare_ready, int32_t* status, void* stream) {
    envgpu::EnvK k;
    if (!params || !envgpu::layout(*params, k)) return mapgpu::fail(envgpu::BAD_PARAMS);
    if (B < 0 || !spec_table || !plan_status || !plan_n_nodes || !plan_nodes || !records2 || !which || !spare_ready || !status)
        return mapgpu::fail("null pointer / negative batch");
    if (k.o_edge > mapgpu::HEAD_CAP) return mapgpu::fail("record header larger than the kernel stages");
    if (B == 0) return 0;
    if (abi::on_device(mapgpu::g_err, device)) return -1;
    hipLaunchKernelGGL(mapgpu::map_record_kernel, dim3(B), dim3(mapgpu::WAVE), 0, (hipStream_t)stream, k, spec_table, plan_status,
                       plan_n_nodes, plan_nodes, records2, which, spare_ready, status, (int)B);
    return abi::launched(mapgpu::g_err, "map_record_kernel launch");
}

const char* mpcgpu_map_last_error(void) { return mapgpu::g_err.text.c_str(); }

}  // extern "C"
