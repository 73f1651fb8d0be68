/*
 * pct_corridor.h -- C ABI of libpct_corridor.so: the safe-region RRT* corridor finder
 * (include/pct_corridor_finder.hpp) for callers that cannot include C++ (tests, bench, cgo/ctypes).
 *
 * Replaces, call for call, the planner node's use of safeRegionRrtStar
 * (Planner/src/sim_planning_demo.cpp:143, 167, 346-347, 350, 354, 367, 399, 412-413, 416, 487, 761;
 * class surface Planner/include/pointcloudTraj/corridor_finder.h:81-149).  SafeRegionExpansion / Refine / Evaluate exist in both
 * forms: `_timed` takes the reference's wall-clock limit in seconds (corridor_finder.h:97-99, read before every iteration as at
 * corridor_finder.cpp:721-722, 774-775, 900-901, 950-951); the plain ones take iteration counts (deterministic runs).  A timed run
 * reports the iterations it consumed; the plain run of that many iterations gives the identical tree.
 */
#ifndef PCT_CORRIDOR_H
#define PCT_CORRIDOR_H
#include <stdint.h>

#include "pct_engine.h"     /* pct_depth_view */
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pct_corridor pct_corridor;

int pct_corridor_create(int64_t cloud_capacity, int device, pct_corridor **out);   /* 0 = ok */
void pct_corridor_destroy(pct_corridor *c);
const char *pct_corridor_last_error(void);

int pct_corridor_set_param(pct_corridor *c, double safety_margin, double search_margin, double max_radius, double sample_range);
int pct_corridor_reset(pct_corridor *c);
/* samples evaluated per GPU round trip in Expansion/Refine: 1 = one by one (the reference's loop); K > 1 = speculative batches
 * that are replayed in order and give the identical corridor */
int pct_corridor_set_speculation(pct_corridor *c, int k);
int pct_corridor_set_input(pct_corridor *c, const void *points, int64_t n, int64_t stride_bytes, int build_index);
/* Rolling map (config C5): the obstacle cloud becomes a sliding window of cloud_capacity points over the rolling-map index
 * (pct_cloud_ring_index: cell_size <= 0 = chosen from the first data; extent may be NULL).  Call once before the first frame; a
 * sensor tick is then pct_corridor_append_input (the newest frame overwrites the oldest points, the index is updated in place) ->
 * evaluate -> refine, where the reference's is set_input of the whole cloud.  pct_corridor_set_input still replaces the window.
 * stride_bytes = 16 for pcl::PointXYZ records, 12 for packed xyz. */
int pct_corridor_enable_rolling(pct_corridor *c, float cell_size, const float extent[3]);
int pct_corridor_append_input(pct_corridor *c, const void *points, int64_t n, int64_t stride_bytes);
/* after pct_corridor_enable_rolling: res > 0 makes pct_corridor_append_input keep only the points whose voxel of that size is new
 * to the window (pct_cloud_ring_dedup: a window of unique voxels); res = 0 turns it off. */
int pct_corridor_set_rolling_dedup(pct_corridor *c, double res);
/* after pct_corridor_enable_rolling: take points out of the window (pct_engine.h, paragraph "Removing points"); *removed (may be
 * NULL) = the number of points removed.  forget_outside removes everything farther than r from centre: the lidar-mode tick is
 * append_input -> forget_outside(drone, sensing range) -> evaluate -> refine, and with set_rolling_dedup on the window then holds
 * exactly the frame's points, the cloud the reference's lidar mode replaces its map with every frame.  clear_ball / clear_box
 * withdraw a stale obstacle.  A window left without a point is the empty cloud.  Radii that may now grow are re-checked by evaluate. */
int pct_corridor_forget_outside(pct_corridor *c, const double centre[3], double r, int64_t *removed);
int pct_corridor_clear_ball(pct_corridor *c, const double centre[3], double r, int64_t *removed);
int pct_corridor_clear_box(pct_corridor *c, const double lo[3], const double hi[3], int64_t *removed);
/* after pct_corridor_enable_rolling: give the slots of removed points back to the window (pct_engine.h, paragraph "Compacting the
 * window").  compact_window compacts now, *reclaimed (may be NULL) = the slots reclaimed; set_rolling_compact(f), 0 < f <= 1, lets
 * every removal above and clear_seen_through compact by itself once f of the capacity is dead (0 = off, the default).  Obstacle
 * indices change; the finder keeps none across calls. */
int pct_corridor_compact_window(pct_corridor *c, int64_t *reclaimed);
int pct_corridor_set_rolling_compact(pct_corridor *c, double dead_fraction);
/* after pct_corridor_enable_rolling: depth images as the map's input (pct_engine.h, paragraph "Depth images").  The rgbd tick is
 * clear_seen_through -> append_depth -> evaluate -> refine with the same image: the carve removes what the image sees through
 * (*removed, may be NULL), the append un-projects the valid pixels on the device and files them as append_input files a point
 * frame (*kept, may be NULL = the points the window took). */
int pct_corridor_clear_seen_through(pct_corridor *c, const pct_depth_view *view, const float *image, double margin, int64_t *removed);
int pct_corridor_append_depth(pct_corridor *c, const pct_depth_view *view, const float *image, double max_depth, int64_t *kept);
/* the same two calls for a lidar's range image (pct_engine.h, paragraph "Range images").  The lidar tick is
 * clear_seen_through_range -> append_range -> evaluate -> refine with the same scan. */
int pct_corridor_clear_seen_through_range(pct_corridor *c, const pct_range_view *view, const float *image, double margin, int64_t *removed);
int pct_corridor_append_range(pct_corridor *c, const pct_range_view *view, const float *image, double max_range, int64_t *kept);
/* after pct_corridor_enable_rolling: radius outlier removal on the window itself (pct_engine.h, paragraph "Removing outliers"): of the
 * `newest` most recent points (<= 0: every point), those with fewer than min_neighbours other points of the window within r are
 * removed (*removed, may be NULL).  With a noisy sensor the tick is clear_seen_through -> append_depth -> remove_outliers ->
 * evaluate -> refine with newest = *kept of the append. */
int pct_corridor_remove_outliers(pct_corridor *c, double r, int32_t min_neighbours, int64_t newest, int64_t *removed);
/* after pct_corridor_enable_rolling: statistical outlier removal (pct_engine.h, paragraph "Statistical outliers").  remove_statistical:
 * of the `newest` most recent points (<= 0: every point), those whose mean distance to their k nearest other points is greater than
 * mean + stddev_mult * stddev over the judged points are removed (*removed and *stats may be NULL; stats->threshold is the threshold
 * it used).  remove_isolated: the same removal under a fixed threshold.  With a noisy sensor: every so often remove_statistical over
 * the whole window, every frame clear_seen_through -> append_depth -> remove_isolated(k, that threshold, newest = *kept) -> evaluate
 * -> refine. */
int pct_corridor_remove_statistical(pct_corridor *c, int32_t k, double stddev_mult, int64_t newest, int64_t *removed, pct_knn_stats *stats);
int pct_corridor_remove_isolated(pct_corridor *c, int32_t k, double max_mean_distance, int64_t newest, int64_t *removed);
/* the engine's handle of the finder's obstacle cloud (SafeRegionRrtStar::obstacleMap().handle()), for the read-only calls of
 * pct_engine.h -- pct_radius_crop reads the window back; owned by the finder, replaced by a set_input that has to grow the map */
int pct_corridor_cloud(pct_corridor *c, pct_cloud **cloud);
int pct_corridor_set_pt(pct_corridor *c, const double start[3], const double end[3], double xl, double xh, double yl, double yh,
                        double zl, double zh, double local_range, int max_iter, double sample_portion, double goal_portion);
int pct_corridor_set_start_pt(pct_corridor *c, const double start[3], const double end[3]);
int pct_corridor_reset_root(pct_corridor *c, const double target[3]);
int pct_corridor_expansion(pct_corridor *c, int64_t iterations);
int pct_corridor_refine(pct_corridor *c, int64_t iterations);
int pct_corridor_evaluate(pct_corridor *c);
/* SafeRegionExpansion / Refine / Evaluate (double time_limit), corridor_finder.h:97-99; iterations_done may be NULL */
int pct_corridor_expansion_timed(pct_corridor *c, double time_limit, int64_t *iterations_done);
int pct_corridor_refine_timed(pct_corridor *c, double time_limit, int64_t *iterations_done);
int pct_corridor_evaluate_timed(pct_corridor *c, double time_limit);
int pct_corridor_check_traj_pt_col(pct_corridor *c, const double p[3], int *collides);
/* Path (k x 3, root first) and Radius (k); k through *n_out (may exceed cap; only cap rows written).
 * No path: the reference's placeholder, a 3x3 identity and three zero radii. */
int pct_corridor_get_path(pct_corridor *c, double *path, double *radius, int64_t cap, int64_t *n_out);
int pct_corridor_status(pct_corridor *c, int *path_exists, int *global_navi, int64_t *n_nodes, uint64_t *inflation_queries);
int pct_corridor_speculation_stats(pct_corridor *c, uint64_t *replayed_from_batch, uint64_t *fell_back);
/* on (default): one fused launch per speculative batch (nearest node -> steer -> inflation -> neighbourhood), over the cell index
 * of a static cloud or the rolling-map index; off: the same three stages as three batched launches.  The corridor does not depend on it. */
int pct_corridor_set_fused_expansion(pct_corridor *c, int on);
int pct_corridor_expansion_launches(pct_corridor *c, uint64_t *launches);
/* GPU round trips treeRepair (corridor_finder.cpp:938-1021) has made: two per pass -- one launch for every failed node's neighbourhood,
 * one for the sphere inflation of every node that may be re-checked -- where the reference's loop asks two per neighbour */
int pct_corridor_repair_batches(pct_corridor *c, uint64_t *batches);

/* Test hooks.
 * get_tree: the whole search tree (SafeRegionRrtStar::getTree()), the live spheres in insertion order -- the reference's NodeList,
 * which kd rebuilds follow.  Row i: centre (3 doubles), radius, g (cost from the root), f (distance to the goal), parent = the
 * parent's row (-1 = none), flags bit0 = valid, bit1 = on the best route.  *n = the number of spheres (may exceed cap; only cap rows
 * are written; any array may be NULL).
 * debug_counters: which branches have run since the finder was created (reset does not clear them): out[0] = neighbourhood lists
 * that came back truncated and were asked again through kd_nearest_rangef, out[1] = fused launches refused (the finder switched to
 * the staged form), out[2] = one-by-one iterations (three single queries each), out[3] = the largest node count the kd tree had. */
int pct_corridor_get_tree(pct_corridor *c, double *centre, float *radius, float *g, float *f, int32_t *parent, uint8_t *flags,
                          int64_t cap, int64_t *n);
int pct_corridor_debug_counters(pct_corridor *c, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
