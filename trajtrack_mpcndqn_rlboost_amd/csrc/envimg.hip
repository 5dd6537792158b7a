// envimg.hip -- image observation of the batched DRL environment (TrajectoryPlannerEnvironmentImgsReward1) for gfx950:
// the mpcgpu_env_*imgs* entries of include/mpcgpu_env.h and the fresh-map image step of include/mpcgpu_map.h.
//
// A step is two kernels on one stream: env_step_kernel (envgpu.hip) moves the robot and the obstacles and writes the
// internal observation, reward and flags exactly as for the ray variant; env_img_kernel then draws the two images.
// One workgroup (256 threads) per environment.  The 2W x 2H rasters are never stored as bytes: each is a bit plane in
// LDS (64-bit words, 3 per row at most), one for the padded boundary and one per obstacle clock, and the pixel value is
// 255 where the boundary bit is set and the obstacle bit is not (the boundary is filled with 255 first, every
// obstacle with 0 afterwards, so order among obstacles does not matter).  Phases, separated by barriers:
//   0  obstacle key-frame poses at both clocks -> LDS
//   1  every outline vertex -> integer pixel (truncation toward zero), the edge's 16.16 slope -> LDS
//   2  outline lines (clipped, Bresenham, 8-connected; one thread per edge) and the scanline fill (one thread per row
//      and polygon: the row's crossings become a toggle mask and a hit mask, the even-odd pairing is their prefix xor)
//   3  the half-size resize ((a + b + c + d + 2) >> 2 of each 2 x 2 block) and the distance field, written as words
// The rule restated here is the one of tests/support/image_obs_numpy.py (which also keeps the sort-and-pair form of the
// fill and the step-by-step form of the lines); DESIGN.md states it and marks it unpinned against OpenCV.
//
// Built with -ffp-contract=off (Makefile, IMG_FLAGS): the vertex arithmetic ends in a truncation to an integer pixel, and
// a fused multiply-add in front of it would move vertices that lie close to a pixel boundary.  The operations are
// written in the order the numpy restatement uses.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/mpcgpu_map.h"
#include "envgpu_internal.hpp"

namespace envimg {

using envgpu::EnvK;
using envgpu::IMG_HIST;
using envgpu::IMG_PRE;
using envgpu::IMG_STATE;

constexpr int THREADS = 256;
constexpr int MIN_SIDE = 8, MAX_SIDE = 96;
constexpr int MAX_ROWS = 2 * MAX_SIDE;    // rows of a raster
constexpr int NW = 3;                     // 64-bit words per raster row (2 W <= 192)
constexpr int MAX_OBST = 31;
constexpr int MAX_POLY = 1 + 2 * MAX_OBST;  // the boundary, and every obstacle at both clocks
constexpr double PIX_CLAMP = 1048576.0;   // vertices are clamped to +-2^20 px (keeps the 16.16 arithmetic in 64 bits)
constexpr int LDS_LIMIT = 65536;
typedef unsigned long long u64;

struct EdgePix {      // one outline edge in pixels, in the order of the record (v[k] -> v[k + 1])
    int x0, y0, x1, y1;
    long long dx;     // ((x1 - x0) << 16) / (y1 - y0), truncated; 0 for a horizontal edge
};

struct ImgK {
    int rec, o_anim, an, o_edge, n_kf_max, n_edge_max;
    int W, H;
    double osx, osy, scx, scy, cx, cy, angle;
};

constexpr int STATIC_LDS = 3 * MAX_ROWS * NW * 8 + 2 * (MAX_OBST + 1) * 4 * 8 + 2 * (MAX_OBST + 2) * 4 + 2 * MAX_POLY * 4 +
                           (IMG_HIST + 3) * 8;

__device__ __forceinline__ int to_pixel(double v) {   // np.int32: truncation toward zero
    v = fmin(fmax(v, -PIX_CLAMP), PIX_CLAMP);
    return (int)v;
}

// obstacle.py:71-88 / oracle.rl_env_numpy.keyframe_pose, with exact division (the step kernel uses a reciprocal)
__device__ void keyframe_pose(const double* an, int K, double clock, double* out) {
    const int kind = (int)an[0], nk = (int)an[2];
    const double* tsv = an + 4;
    const double* kf = an + 4 + (K + 1);
    const double tm = fmod(clock + an[1], an[3]);
    double px = kf[3 * (nk - 1)], py = kf[3 * (nk - 1) + 1], rot = kf[3 * (nk - 1) + 2];
    double t = 0.0;
    for (int i = 0; i < nk; ++i) {
        t += tsv[i];
        if (t <= tm && tm < t + tsv[i + 1]) {
            const double xx = (tm - t) / tsv[i + 1];
            const double alpha = kind == 1 ? (1.0 - cos(xx * M_PI)) / 2.0 : xx;
            const double* k0 = kf + 3 * i;
            const double* k1 = kf + 3 * ((i + 1) % nk);
            px = k0[0] * (1.0 - alpha) + k1[0] * alpha;
            py = k0[1] * (1.0 - alpha) + k1[1] * alpha;
            rot = k0[2] * (1.0 - alpha) + k1[2] * alpha;
            break;
        }
    }
    double c, s;
    sincos(rot, &s, &c);
    out[0] = px; out[1] = py; out[2] = c; out[3] = s;
}

__device__ __forceinline__ void set_pixel(u64* plane, long long x, long long y, int W2, int H2) {
    if (x >= 0 && x < W2 && y >= 0 && y < H2) atomicOr(&plane[y * NW + (x >> 6)], 1ull << (x & 63));
}

// cv2.clipLine (Cohen-Sutherland on the integer rectangle, intersections in double, truncated); x1 is updated before
// the second end point is clipped, as OpenCV does
__device__ bool clip_line(long long W2, long long H2, long long& x1, long long& y1, long long& x2, long long& y2) {
    const long long right = W2 - 1, bottom = H2 - 1;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        long long a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (long long)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (long long)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (long long)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (long long)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

// cv2.line with LINE_8 through LineIterator(leftToRight = true): clip, walk left to right along the major axis, step the
// minor axis while the error term is negative
__device__ void draw_line(u64* plane, const EdgePix& q, int W2, int H2) {
    long long x0 = q.x0, y0 = q.y0, x1 = q.x1, y1 = q.y1;
    if (!clip_line(W2, H2, x0, y0, x1, y1)) return;
    long long dx = x1 - x0, dy = y1 - y0;
    if (dx < 0) { x0 = x1; y0 = y1; dx = -dx; dy = -dy; }
    const long long sy = dy < 0 ? -1 : 1, ady = dy < 0 ? -dy : dy;
    const bool ymajor = ady > dx;
    const long long major = ymajor ? ady : dx, minor = ymajor ? dx : ady;
    long long err = major - 2 * minor;
    long long x = x0, y = y0;
    for (long long i = 0; i <= major; ++i) {
        set_pixel(plane, x, y, W2, H2);
        const bool mv = err < 0;
        err += -2 * minor + (mv ? 2 * major : 0);
        if (ymajor) { y += sy; x += mv ? 1 : 0; }
        else { x += 1; y += mv ? sy : 0; }
    }
}

__device__ __forceinline__ u64 prefix_xor(u64 v) {   // bit i = xor of bits 0..i
    v ^= v << 1; v ^= v << 2; v ^= v << 4; v ^= v << 8; v ^= v << 16; v ^= v << 32;
    return v;
}

struct Shared {
    u64 plane[3][MAX_ROWS * NW];        // boundary, obstacles at clock 0, obstacles at clock 1
    double pose[2][MAX_OBST + 1][4];    // x, y, cos, sin of every obstacle at both clocks
    int first[MAX_OBST + 2], end[MAX_OBST + 2];   // edge range of outline owner + 1
    int ymin[MAX_POLY], ymax[MAX_POLY];
    double hist[IMG_HIST + 1];          // observation count, clock ring
    double clk[2];
};

// Draws the image pair of robot pose (rx, ry, th) with the obstacles at clocks sh.clk[0] / sh.clk[1] into out
// ([3][H][W] bytes of one environment).  Every thread of the workgroup calls it.
__device__ void render(const ImgK& k, Shared& sh, EdgePix* epix, const double* rec, const uint8_t* dfield, double rx,
                       double ry, double th, uint8_t* out) {
    const int t = threadIdx.x;
    const int W2 = 2 * k.W, H2 = 2 * k.H;
    const int n_obst = (int)rec[1], n_edge = (int)rec[2];
    const int E = k.n_edge_max;
    const double* ed = rec + k.o_edge;

    // ---- phase 0: clear the planes and tables, obstacle poses at both clocks
    for (int i = t; i < 3 * MAX_ROWS * NW; i += THREADS) (&sh.plane[0][0])[i] = 0ull;
    if (t < MAX_OBST + 2) { sh.first[t] = 0; sh.end[t] = 0; }
    if (t < MAX_POLY) { sh.ymin[t] = INT_MAX; sh.ymax[t] = INT_MIN; }
    if (t < 2 * (MAX_OBST + 1)) {
        const int j = t & MAX_OBST, s = t >> 5;
        if (j < n_obst) keyframe_pose(rec + k.o_anim + j * k.an, k.n_kf_max, sh.clk[s], sh.pose[s][j]);
    }
    __syncthreads();

    // ---- phase 1: outline vertices -> pixels (ext_obsv_image.py:57-60):
    //      pixel = original_size * (scale * (R (v - p)) + center), R = [[s, -c], [c, s]], angle theta - image angle
    double c, s;
    sincos(th - k.angle, &s, &c);
    for (int task = t; task < 2 * n_edge; task += THREADS) {
        const int set = task >= n_edge, e = task - set * n_edge;
        const double* q = ed + 5 * e;
        const int owner = (int)q[4];
        if (owner < -1 || (owner == -1 && set == 1)) continue;
        double v[4] = {q[0], q[1], q[2], q[3]};
        if (owner >= 0) {   // obstacle.py:195-201: position + R(rotation) * padded node
            const double* po = sh.pose[set][owner];
            for (int i = 0; i < 2; ++i) {
                const double nx = v[2 * i], ny = v[2 * i + 1];
                v[2 * i] = po[0] + (po[2] * nx - po[3] * ny);
                v[2 * i + 1] = po[1] + (po[3] * nx + po[2] * ny);
            }
        }
        int p[4];
        for (int i = 0; i < 2; ++i) {
            const double dx = v[2 * i] - rx, dy = v[2 * i + 1] - ry;
            p[2 * i] = to_pixel(k.osx * (k.scx * (s * dx - c * dy) + k.cx));
            p[2 * i + 1] = to_pixel(k.osy * (k.scy * (c * dx + s * dy) + k.cy));
        }
        EdgePix ep;
        ep.x0 = p[0]; ep.y0 = p[1]; ep.x1 = p[2]; ep.y1 = p[3];
        ep.dx = p[1] == p[3] ? 0 : ((long long)(p[2] - p[0]) * 65536) / (long long)(p[3] - p[1]);
        epix[set * E + e] = ep;
        if (set == 0) {   // outlines are contiguous runs of the edge table (rl_env.pack_records)
            if (e == 0 || (int)ed[5 * (e - 1) + 4] != owner) sh.first[owner + 1] = e;
            if (e == n_edge - 1 || (int)ed[5 * (e + 1) + 4] != owner) sh.end[owner + 1] = e + 1;
        }
        const int poly = owner < 0 ? 0 : 1 + 2 * owner + set;
        atomicMin(&sh.ymin[poly], min(p[1], p[3]));
        atomicMax(&sh.ymax[poly], max(p[1], p[3]));
    }
    __syncthreads();

    // ---- phase 2: outlines (CollectPolyEdges draws every edge, horizontal ones included) and the scanline fill
    const int n_poly = 1 + 2 * n_obst;
    const int n_line = 2 * n_edge;
    for (int task = t; task < n_line + n_poly * H2; task += THREADS) {
        if (task < n_line) {
            const int set = task >= n_edge, e = task - set * n_edge;
            const int owner = (int)ed[5 * e + 4];
            if (owner < -1 || (owner == -1 && set == 1)) continue;
            draw_line(sh.plane[owner < 0 ? 0 : 1 + set], epix[set * E + e], W2, H2);
            continue;
        }
        const int poly = (task - n_line) / H2, row = (task - n_line) - poly * H2;
        if (row < sh.ymin[poly] || row >= sh.ymax[poly]) continue;
        const int set = poly == 0 ? 0 : (poly - 1) & 1, oi = poly == 0 ? 0 : 1 + ((poly - 1) >> 1);
        // edge active on rows y_upper <= row < y_lower, x carried in 16.16 from its upper vertex; the crossings, sorted
        // and paired even-odd, fill [xl >> 16, xr >> 16].  Pixel x is inside a pair iff an odd number of crossings lie
        // left of it (prefix xor of the toggles at xi + 1) or a crossing lies on it (hit).
        u64 tg[NW] = {0ull, 0ull, 0ull}, ht[NW] = {0ull, 0ull, 0ull};
        for (int e = sh.first[oi]; e < sh.end[oi]; ++e) {
            const EdgePix q = epix[set * E + e];
            if (q.y0 == q.y1) continue;
            const bool down = q.y0 < q.y1;
            const int xu = down ? q.x0 : q.x1, yu = down ? q.y0 : q.y1, yl = down ? q.y1 : q.y0;
            if (row < yu || row >= yl) continue;
            const long long X = (long long)xu * 65536 + (long long)(row - yu) * q.dx;
            const long long xi = X >> 16;
            if (xi + 1 < W2) {
                const int pos = xi + 1 < 0 ? 0 : (int)(xi + 1);
#pragma unroll
                for (int w = 0; w < NW; ++w) tg[w] ^= (pos >> 6) == w ? 1ull << (pos & 63) : 0ull;
            }
            if (xi >= 0 && xi < W2) {
#pragma unroll
                for (int w = 0; w < NW; ++w) ht[w] |= (int)(xi >> 6) == w ? 1ull << (xi & 63) : 0ull;
            }
        }
        u64* dst = sh.plane[poly == 0 ? 0 : 1 + set] + row * NW;
        u64 carry = 0ull;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const u64 par = prefix_xor(tg[w]) ^ carry;
            carry = (par >> 63) ? ~0ull : 0ull;
            const int valid = W2 - 64 * w;
            const u64 keep = valid >= 64 ? ~0ull : valid <= 0 ? 0ull : (1ull << valid) - 1ull;
            const u64 f = (par | ht[w]) & keep;
            if (f) atomicOr(&dst[w], f);
        }
    }
    __syncthreads();

    // ---- phase 3: half-size resize of both images + distance field -> out [3][H][W]
    const int HW = k.H * k.W;
    auto value = [&](int q) -> unsigned {
        const int ch = q / HW, rem = q - ch * HW;
        if (ch == 2) return dfield[rem];
        const int r = rem / k.W, cc = rem - r * k.W;
        const u64* B = sh.plane[0];
        const u64* O = sh.plane[1 + ch];
        unsigned n = 0;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = 2 * r + dy, x = 2 * cc, w = y * NW + (x >> 6);
            const u64 bits = (B[w] & ~O[w]) >> (x & 63);   // x even: both pixels of the pair are in one word
            n += (unsigned)(bits & 1ull) + (unsigned)((bits >> 1) & 1ull);
        }
        return (255u * n + 2u) >> 2;
    };
    const int nbytes = 3 * HW;
    if ((HW & 3) == 0 && (((uintptr_t)out) & 3) == 0) {
        uint32_t* o32 = (uint32_t*)out;
        for (int wq = t; wq < nbytes / 4; wq += THREADS) {
            const int q = 4 * wq;
            o32[wq] = value(q) | (value(q + 1) << 8) | (value(q + 2) << 16) | (value(q + 3) << 24);
        }
    } else {
        for (int q = t; q < nbytes; q += THREADS) out[q] = (uint8_t)value(q);
    }
    __syncthreads();
}

//
// FRESH (include/mpcgpu_map.h, mpcgpu_env_step_imgs_fresh_dev): rec_all is the [2][B][rec] table of the fresh-map step and
// which[b] -- already flipped by env_step_kernel<true> when the row turned over in this step -- names the record the row
// is on NOW.  The image of the row's current state is drawn from that record; the terminal image of an episode that
// ended in this step is drawn from the record it ENDED on, whose table index the step left at IMG_PRE + 5.  render()
// keeps nothing of a record between two calls: it reads the counts from the record it is given and clears the planes, the
// outline ranges, the row extents and the poses it uses at its start, so the two records of a row may differ in
// everything.  Stream order is the only synchronisation: this kernel runs behind the step on the caller's stream, and
// a refill enqueued behind it may overwrite the record a row has just left (its new spare slot) -- by then the terminal
// image has been drawn.  Everything FRESH adds sits under `if constexpr`.
template <bool FRESH>
__global__ __launch_bounds__(THREADS) void env_img_kernel(ImgK k, const double* __restrict__ rec_all,
                                                         const double* __restrict__ state_all, double* img_all,
                                                         const uint8_t* __restrict__ dfield, uint8_t* out_img,
                                                         uint8_t* term_img, int autoreset, int B,
                                                         const int32_t* __restrict__ which) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    __shared__ Shared sh;
    const int b = blockIdx.x;
    if (b >= B) return;
    const int t = threadIdx.x;
    EdgePix* epix = (EdgePix*)dyn;
    const double* rec = rec_all + (size_t)b * k.rec;
    if constexpr (FRESH) rec = rec_all + ((size_t)(which[b] & 1) * B + b) * k.rec;
    const double* st = state_all + (size_t)b * MPCGPU_ENV_STATE_DOUBLES;
    double* ist = img_all + (size_t)b * IMG_STATE;
    const size_t img_bytes = (size_t)3 * k.H * k.W;

    // history (ext_obsv_image.py:66-71): every observation prepends the current outlines and keeps 6; channel 1 shows
    // the oldest kept.  Only the clocks are kept: observation n (n = 1, 2, ... since the reset) sits in slot (n - 1) % 6.
    auto push = [&](double clock) {   // thread 0
        sh.hist[0] += 1.0;
        const int n = (int)sh.hist[0];
        sh.hist[1 + (n - 1) % IMG_HIST] = clock;
        const int oldest = n - (IMG_HIST - 1) > 1 ? n - (IMG_HIST - 1) : 1;
        sh.clk[0] = clock;
        sh.clk[1] = sh.hist[1 + (oldest - 1) % IMG_HIST];
    };
    if (t == 0)
        for (int i = 0; i <= IMG_HIST; ++i) sh.hist[i] = ist[i];
    if (autoreset && ist[IMG_PRE + 4] != 0.0) {
        // the episode ended in this step: its image from the pose and clock before the in-kernel reset, with the history
        // up to it; then reset() clears the history (environment.py:161-180)
        if (t == 0) push(ist[IMG_PRE + 3]);
        __syncthreads();
        const double* ended_on = rec;
        if constexpr (FRESH) ended_on = rec_all + ((size_t)((int)ist[IMG_PRE + 5] & 1) * B + b) * k.rec;
        if (term_img) render(k, sh, epix, ended_on, dfield, ist[IMG_PRE], ist[IMG_PRE + 1], ist[IMG_PRE + 2], term_img + b * img_bytes);
        if (t == 0) sh.hist[0] = 0.0;
        // the ring slots past the count are never read; the fresh step clears them all the same, so that the image state
        // after a turnover is bit for bit the one reset() leaves (step, replace_maps, reset: the form it is tested against)
        if constexpr (FRESH)
            if (t == 0)
                for (int i = 1; i <= IMG_HIST; ++i) sh.hist[i] = 0.0;
    }
    if (t == 0) push(st[5]);
    __syncthreads();
    render(k, sh, epix, rec, dfield, st[0], st[1], st[2], out_img + b * img_bytes);
    if (t <= IMG_HIST) ist[t] = sh.hist[t];
}

static int check_img(const mpcgpu_env_img_params* img) {
    if (!img) return envgpu::fail("null mpcgpu_env_img_params");
    if (img->down_sample != 2) return envgpu::fail("invalid mpcgpu_env_img_params: only down_sample = 2 is built");
    if (img->width < MIN_SIDE || img->width > MAX_SIDE || img->height < MIN_SIDE || img->height > MAX_SIDE)
        return envgpu::fail("invalid mpcgpu_env_img_params: width and height must be 8..96");
    if (!std::isfinite(img->scale_x) || !std::isfinite(img->scale_y) || !std::isfinite(img->center_x) ||
        !std::isfinite(img->center_y) || !std::isfinite(img->angle))
        return envgpu::fail("invalid mpcgpu_env_img_params: scale, center and angle must be finite");
    return 0;
}

static int32_t launch(int32_t device, const mpcgpu_env_params* params, const mpcgpu_env_img_params* img, int32_t B,
                      const double* records, double* state, double* img_state, const uint8_t* dfield,
                      const int32_t* action, envgpu::EnvOut out, uint8_t* obs_image, uint8_t* term_image, void* stream,
                      const envgpu::EnvFresh* fresh = nullptr) {
    if (check_img(img) != 0) return -1;
    EnvK ek;
    if (!params || !envgpu::layout(*params, ek)) return envgpu::fail(envgpu::BAD_PARAMS);
    const size_t dyn = (size_t)2 * params->n_edge_max * sizeof(EdgePix);
    if (dyn + sizeof(Shared) > (size_t)LDS_LIMIT)
        return envgpu::fail("too many outline edges for the image kernel (n_edge_max * 48 bytes + 17 KB must fit 64 KB of LDS)");
    if (B < 0 || !img_state || !dfield || !obs_image) return envgpu::fail("null pointer / negative batch");
    // the step: internal observation, reward, flags; the ray external observation is not written
    const int rc = envgpu::launch_step(device, params, B, records, state, action, out, false, stream, fresh);
    if (rc != 0 || B == 0) return rc;
    ImgK k;
    k.rec = ek.rec; k.o_anim = ek.o_anim; k.an = ek.an; k.o_edge = ek.o_edge;
    k.n_kf_max = params->n_kf_max; k.n_edge_max = params->n_edge_max;
    k.W = img->width; k.H = img->height;
    k.osx = 2.0 * img->width; k.osy = 2.0 * img->height;
    k.scx = img->scale_x; k.scy = img->scale_y; k.cx = img->center_x; k.cy = img->center_y; k.angle = img->angle;
    // both launches on the caller's stream, the step first: the image kernel reads the state, the pre-reset block and (fresh)
    // which[] the step has just written
    if (fresh)
        hipLaunchKernelGGL(env_img_kernel<true>, dim3(B), dim3(THREADS), dyn, (hipStream_t)stream, k, records, state, img_state,
                           dfield, obs_image, term_image, out.pre_reset ? 1 : 0, (int)B, (const int32_t*)fresh->which);
    else
        hipLaunchKernelGGL(env_img_kernel<false>, dim3(B), dim3(THREADS), dyn, (hipStream_t)stream, k, records, state, img_state,
                           dfield, obs_image, term_image, out.pre_reset ? 1 : 0, (int)B, (const int32_t*)nullptr);
    return abi::launched(envgpu::g_err, "env_img_kernel launch");
}

}  // namespace envimg

extern "C" {

int32_t mpcgpu_env_img_state_doubles(const mpcgpu_env_img_params* img) {
    if (envimg::check_img(img) != 0) return -1;
    return envgpu::IMG_STATE;
}

int32_t mpcgpu_env_step_imgs_dev(int32_t device, const mpcgpu_env_params* params, const mpcgpu_env_img_params* img,
                                 int32_t B, const double* records, double* state, double* img_state,
                                 const uint8_t* distance_field, const int32_t* action, float* obs_internal,
                                 uint8_t* obs_image, double* reward, uint8_t* terminated, void* stream) {
    envgpu::EnvOut out{obs_internal, nullptr, reward, terminated, nullptr, nullptr, nullptr, 0, nullptr};
    return envimg::launch(device, params, img, B, records, state, img_state, distance_field, action, out, obs_image,
                          nullptr, stream);
}

int32_t mpcgpu_env_step_imgs_autoreset_dev(int32_t device, const mpcgpu_env_params* params,
                                           const mpcgpu_env_img_params* img, int32_t B, const double* records,
                                           double* state, double* img_state, const uint8_t* distance_field,
                                           const int32_t* action, float* obs_internal, uint8_t* obs_image,
                                           double* reward, uint8_t* terminated, uint8_t* truncated,
                                           float* terminal_obs_internal, uint8_t* terminal_obs_image,
                                           int32_t max_episode_steps, void* stream) {
    if (envgpu::autoreset_args(action, max_episode_steps, true)) return -1;
    if (!img_state) return envgpu::fail("null pointer / negative batch");
    envgpu::EnvOut out{obs_internal, nullptr, reward, terminated, truncated, terminal_obs_internal, nullptr,
                       max_episode_steps, img_state};
    return envimg::launch(device, params, img, B, records, state, img_state, distance_field, action, out, obs_image,
                          terminal_obs_image, stream);
}

// include/mpcgpu_map.h
int32_t mpcgpu_env_step_imgs_fresh_dev(int32_t device, const mpcgpu_env_params* params, const mpcgpu_env_img_params* img,
                                       int32_t B, const double* records2, int32_t* which, int32_t* spare_ready,
                                       int32_t* loaded, int32_t* stale, double* state, double* img_state,
                                       const uint8_t* distance_field, const int32_t* action, float* obs_internal,
                                       uint8_t* obs_image, double* reward, uint8_t* terminated, uint8_t* truncated,
                                       float* terminal_obs_internal, uint8_t* terminal_obs_image,
                                       int32_t max_episode_steps, void* stream) {
    envgpu::EnvOut out{obs_internal, nullptr, reward, terminated, truncated, terminal_obs_internal, nullptr, max_episode_steps,
                       img_state};
    const envgpu::EnvFresh fresh{which, spare_ready, loaded, stale};
    const bool mine = img_state && distance_field && obs_image;
    if (envgpu::fresh_args(fresh, mine ? nullptr : "null pointer (img_state / distance_field / obs_image)", action, out)) return -1;
    return envimg::launch(device, params, img, B, records2, state, img_state, distance_field, action, out, obs_image,
                          max_episode_steps > 0 ? terminal_obs_image : nullptr, stream, &fresh);
}

}  // extern "C"
