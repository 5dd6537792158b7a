/*
 * mpcgpu_map.h -- C-ABI of per-episode map turnover for the batched DRL environment in libmpcgpu.so.
 *
 * The reference's training environment gets a new map on every reset() (src/pkg_dqn/environment/environment.py:161-169).
 * Here every environment row owns TWO records of the layout of mpcgpu_env.h: the one it steps on and a spare.  The step
 * below is mpcgpu_env_step_autoreset_dev with one addition: a row whose episode ends while its spare is ready starts the
 * next episode on the spare, inside the same launch.  Who fills the spares is the caller's business (rl_env.py:
 * BatchedRaysEnv.load_spares packs host-built maps into them).
 *
 * Tables, all DEVICE pointers, int32 unless said otherwise:
 *     records2     [2][B][R] doubles, R = mpcgpu_env_record_doubles(params); row b steps on records2[which[b]][b]
 *     which        [B] 0 / 1: the table row b is on
 *     spare_ready  [B] 1 when records2[1 - which[b]][b] holds a complete record that has not been used yet
 *     loaded       [B] episodes of row b that started on a new record (counted by the kernel)
 *     stale        [B] in-kernel resets of row b that found no spare and started again on the same record
 *
 * When the episode of row b ends, the workgroup of that row -- before the reset observation -- reads spare_ready[b]; if
 * it is set it flips which[b], clears spare_ready[b], reads path, obstacle and edge counts, goal and start state from the
 * other record and adds 1 to loaded[b]; otherwise it resets on the record it has and adds 1 to stale[b].  A workgroup
 * touches the words of its own row only, so there are no atomics; whatever writes spares and sets spare_ready must be
 * enqueued on the SAME stream as the step (or be ordered against it by the caller): the step reads spare_ready and the
 * spare record without any other synchronisation.
 *
 * Maps can be DRAWN on the device.  The spec table holds one record of MPCGPU_MAP_SPEC_DOUBLES doubles per map, the
 * keyword form of rl_env.make_map without a path (map_stream.pack_specs writes the same record on the host):
 *     [0..4] start state x, y, theta, v, w   [5..6] goal x, y
 *     [7] boundary vertices (3..16)   [8] static polygons (0..8)   [9] periodic obstacles (0..8)   [10..15] reserved, 0
 *     [16 .. 48)      boundary x, y per vertex, in the caller's order and orientation
 *     [48 .. 224)     static polygon s at 48 + 22 s: vertex count (3..10), reserved, then x, y per vertex
 *     [224 .. 288)    periodic obstacle d at 224 + 8 d: p1 x, y, p2 x, y, freq, rx, ry, angle (12 corners, obstacle.py:193-201)
 * Unused entries are 0.
 *
 * mpcgpu_map_draw_dev draws generate_map_dynamic maps (utils/map.py:158-189: a 40 x 20 m hall, three boxes, seven periodic
 * obstacles) from a counter-based stream, so that a map can be regenerated from (seed, serial) alone:
 *     draw k of map `serial` = lo + (hi - lo) * u_k,   u_k = (bits >> 11) * 2^-53,
 *     bits = mix64(mix64(seed + G * serial) + G * (k + 1)) modulo 2^64,   G = 0x9E3779B97F4A7C15,
 *     mix64(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 * (the SplitMix64 finaliser).  A map takes 71 draws in the order of rl_env.random_dynamic_spec, whose result on
 * map_stream.CounterUniform(seed, serial) is the host twin of the kernel, bit for bit.
 */
#ifndef MPCGPU_MAP_H
#define MPCGPU_MAP_H

#include <stdint.h>

#include "mpcgpu_env.h"
#include "mpcgpu_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPCGPU_MAP_MAX_BOUNDARY 16      /* boundary vertices of a spec */
#define MPCGPU_MAP_MAX_STATIC 8         /* static polygons of a spec */
#define MPCGPU_MAP_MAX_STATIC_VERTS 10  /* vertices of one static polygon */
#define MPCGPU_MAP_MAX_PERIODIC 8       /* periodic obstacles of a spec */
#define MPCGPU_MAP_SPEC_DOUBLES 288
/* capacities of the planner records mpcgpu_map_rings_dev writes (mpcgpu_plan_params n_ring_max, n_vert_max): the boundary
 * and every static polygon, each vertex bevelled into two */
#define MPCGPU_MAP_RING_MAX 9
#define MPCGPU_MAP_VERT_MAX 192
#define MPCGPU_MAP_MAX_EDGES 1024       /* outline edges of one map mpcgpu_map_record_dev can build (more: status 5) */

/*
 * One step on the rows' current records.  max_episode_steps > 0: with in-kernel auto-reset and map turnover as described
 * above; every other argument as in mpcgpu_env_step_autoreset_dev.  max_episode_steps = 0: no reset and no turnover, as
 * mpcgpu_env_step_dev (action may then be NULL = observe only; truncated and terminal_obs_* are not written).
 */
int32_t mpcgpu_env_step_fresh_dev(int32_t device, const mpcgpu_env_params* params, int32_t B, const double* records2,
                                  int32_t* which, int32_t* spare_ready, int32_t* loaded, int32_t* stale, double* state,
                                  const int32_t* action, float* obs_internal, float* obs_external, double* reward,
                                  uint8_t* terminated, uint8_t* truncated, float* terminal_obs_internal,
                                  float* terminal_obs_external, int32_t max_episode_steps, void* stream);

/*
 * The same step for the image observation (mpcgpu_env_step_imgs_autoreset_dev with map turnover): img, img_state,
 * distance_field and the images as in mpcgpu_env.h, the tables as above.  Two launches on `stream`, the step and then the
 * image kernel.  Which record an image is drawn from, for a row whose episode ended in this step:
 *     terminal_obs_image[b]  the record the episode ENDED on -- its outlines and key frames at the clock of the last step,
 *                            with the image history up to it -- also when the row has moved to its spare in this call
 *     obs_image[b]           the record the row is on NOW, records2[which[b]][b] as the step left which[b]: the first
 *                            image of the next episode, on the new map when the row turned over
 * and for every other row obs_image[b] from records2[which[b]][b].  The step leaves the table index a row was on at its
 * entry in img_state[b][13] for the image kernel; img_state[b][8..13] are scratch between the two launches.
 * max_episode_steps = 0: no reset and no turnover, as mpcgpu_env_step_imgs_dev on records2[which[b]][b] (action may be
 * NULL; truncated and terminal_obs_* are not written).
 * Ordering: stream order only.  Whatever refills spares is enqueued BEHIND this call on the same stream; it may then
 * overwrite the record a row has just left (that slot is the row's new spare), because the image kernel that drew the
 * terminal image from it has finished by then.  A writer on another stream must be ordered behind the image kernel.
 * Refused before anything is enqueued (< 0, text via mpcgpu_env_last_error): a null which / spare_ready / loaded / stale /
 * img_state / distance_field / obs_image, a negative max_episode_steps, auto-reset without action or truncated, invalid
 * image params, and an n_edge_max whose edge staging does not fit the image kernel's LDS.
 */
int32_t mpcgpu_env_step_imgs_fresh_dev(int32_t device, const mpcgpu_env_params* params, const mpcgpu_env_img_params* img,
                                       int32_t B, const double* records2, int32_t* which, int32_t* spare_ready,
                                       int32_t* loaded, int32_t* stale, double* state, double* img_state,
                                       const uint8_t* distance_field, const int32_t* action, float* obs_internal,
                                       uint8_t* obs_image, double* reward, uint8_t* terminated, uint8_t* truncated,
                                       float* terminal_obs_internal, uint8_t* terminal_obs_image,
                                       int32_t max_episode_steps, void* stream);

/* doubles of one spec record (MPCGPU_MAP_SPEC_DOUBLES; no device needed) */
int32_t mpcgpu_map_spec_doubles(void);

/*
 * For every row b with spare_ready[b] == 0: spec_table[b] = map number b + B * attempt[b] of stream `seed`, and
 * attempt[b] += 1.  Rows with spare_ready[b] != 0 are left alone.  spec_table [B][MPCGPU_MAP_SPEC_DOUBLES] doubles,
 * spare_ready and attempt [B] int32.  One kernel on `stream`, no synchronisation.  0 = ok, < 0 = error (text via
 * mpcgpu_map_last_error, thread-local).
 */
int32_t mpcgpu_map_draw_dev(int32_t device, int32_t B, uint64_t seed, double* spec_table, const int32_t* spare_ready,
                            int32_t* attempt, void* stream);

/*
 * Spec table -> what the planner takes (mpcgpu_plan.h): rings [B][mpcgpu_plan_record_doubles] doubles for
 * mpcgpu_plan_params{MPCGPU_MAP_VERT_MAX, MPCGPU_MAP_RING_MAX, ..} (396 doubles), and start_goal [B][4].  Bit for bit what the host
 * makes of the same spec (path_plan.inflate_spec, oriented_rings, pack_rings; environment.py:130-140): every ring made counter-
 * clockwise (rl_geometry.orient, open rings) and rounded through float32; the boundary moved inwards by 0.5 and the static
 * polygons outwards by 0.8 with mitred joins of limit 2 (rl_geometry.mitre_polygon, its collinear and bevel branches included);
 * the boundary stored counter-clockwise, the obstacles clockwise; start as it is, goal through float32.  The periodic obstacles
 * are not visible to the planner.  The host's validity tests (check=True: the offset ring is simple, a shrunk ring stays inside)
 * are NOT repeated: the caller answers for polygons whose local offset construction applies.  generate_map_dynamic draws never
 * need them -- its boxes are at least 4 m wide and high, so an offset by 0.8 m cannot make an edge vanish, and its hall is a
 * rectangle of 40 x 20 m.  A row with spare_ready[b] != 0 is skipped: its ring count becomes 0 and the planner leaves it with
 * status 4.  Then call mpcgpu_plan_paths_dev on the same stream.
 */
int32_t mpcgpu_map_rings_dev(int32_t device, int32_t B, const double* spec_table, const int32_t* spare_ready, double* rings,
                             double* start_goal, void* stream);

/*
 * Spec table + planner output -> environment records in the rows' SPARE slots, records2[1 - which[b]][b], as rl_env.pack_records
 * ([make_map(path = planned nodes, **spec)], limits = params) writes them: static_obstacle and periodic_obstacle (the kept
 * rotation quirk and step = pi / freq included), ellipse_nodes, the round-join rl_geometry.buffer_polygon by params->radius with
 * its fillet count rule and its sequential drop of near-duplicate points, the float32 pass of padded nodes, key frames and goal,
 * the boundary shrunk by the radius in float64, path lengths summed in path order, the edge table with its owner column and
 * the -2 padding.  Counts, path, animation blocks, owners and padding are exactly the host's; outline coordinates come after
 * cos, sin, atan2, acos and hypot of the device library, which may differ from the host's by an ulp of the float64 value.
 * The validity tests of the host (check=True) are NOT repeated, see mpcgpu_map_rings_dev.
 *   plan_status, plan_n_nodes [B], plan_nodes [B][MPCGPU_PLAN_MAX_NODES][2]: from mpcgpu_plan_paths_dev on the same stream
 *   status [B]: -1 row skipped (spare_ready[b] != 0); the planner's 1..4; 5 the map does not fit n_path_max, n_obst_max,
 *               n_kf_max or n_edge_max of params (or has more than MPCGPU_MAP_MAX_EDGES outline edges); 0 record written and
 *               spare_ready[b] set.  Nothing of a row is written unless its status is 0.
 * Upper bound of edges of a generate_map_dynamic map: the shrunk rectangle 4; a box 4 corners x (4 fillet segments + 1) = 20,
 * three of them 60; a 12-corner ellipse is convex, its turning angles t_i sum to 2 pi and vertex i gives
 * max(int(t_i / (pi / 8) + 0.5) + 1, 2) <= t_i / (pi / 8) + 2 points, so at most 16 + 24 = 40, seven of them 280: 344 in all.
 * A path bends at box corners only (the rectangle has no reflex corner): at most 2 + 12 = 14 nodes.
 */
int32_t mpcgpu_map_record_dev(int32_t device, const mpcgpu_env_params* params, int32_t B, const double* spec_table,
                              const int32_t* plan_status, const int32_t* plan_n_nodes, const double* plan_nodes, double* records2,
                              const int32_t* which, int32_t* spare_ready, int32_t* status, void* stream);

const char* mpcgpu_map_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MPCGPU_MAP_H */
