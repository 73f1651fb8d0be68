// pct_obstacle_map.hpp -- C++ host-side mirror of the planner's obstacle-cloud seam, header only,
// over the C ABI of pct_engine.h.  Method names, argument meaning and return conventions follow
// the reference so that the call sites listed below change by one line each.
//
//   reference (paths relative to /root/reference/Planner)                      this class
//   ---------------------------------------------------------------------     -----------------------------
//   safeRegionRrtStar::setInput(pcl::PointCloud<PointXYZ>)  src/corridor_finder.cpp:93-99    setInput(points, n, stride)
//   safeRegionRrtStar::setParam(safety, search, max_r, range) :17-23; setPt :52-91           setParam(...), setStartPt(...)
//   safeRegionRrtStar::radiusSearch(Vector3d&)              :113-133                          radiusSearch(p)
//   safeRegionRrtStar::checkRadius(Vector3d&)               :656-659                          checkRadius(p)
//   safeRegionRrtStar::checkTrajPtCol(Vector3d&)            :412-416                          checkTrajPtCol(p)
//   loops over checkRadius in SafeRegionEvaluate :829-835 and treeRepair :958-974             checkRadiusBatch(pts, n, out)
//   checkSafeTrajectory(double) + getPosFromBezier          src/sim_planning_demo.cpp:715-781 checkSafeTrajectory(...)
//
// No Eigen/PCL types appear: points are plain double[3] / float records, exactly the bytes
// Eigen::Vector3d and pcl::PointXYZ hold (INTEGRATION.md shows the adapter lines).
// Errors: engine failures throw std::runtime_error carrying pct_last_error(); there is no CPU path.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "pct_engine.h"
#include "pct_trajgen.h"

namespace pct {

// Trajectory generation (pct_trajgen.h, paragraph "Trajectory generation"): what trajGeneration does between the corridor finder and
// the checks (sim_planning_demo.cpp:262-263, timeAllocation + BezierConicOptimizer), for one corridor under K time scales at once.
// GeneratedTrajectories owns the packed candidates: candidate k = the corridor with every segment time multiplied by scales[k];
// polycoef holds the rows in the layout the checks read and batch() is the pct_bezier_batch over them (valid while this object
// lives and is not changed).
struct GeneratedTrajectories {
    std::vector<double> centres, radius, seg_time, start_state, end_state, polycoef;
    std::vector<int32_t> orders, seg_offsets;
    std::vector<double> planes;             // generateTrajectoriesInPolyhedra: the candidates' planes; centres then holds the anchors
    std::vector<int32_t> plane_offsets;
    std::vector<pct_trajgen_result> results;
    int64_t row_stride = 0;
    pct_bezier_batch batch() const
    {
        return pct_bezier_batch{ polycoef.data(), row_stride, seg_time.data(), orders.data(), seg_offsets.data(), nullptr, (int64_t)results.size() };
    }
    const double *rows(int64_t k) const { return polycoef.data() + (int64_t)seg_offsets[(size_t)k] * row_stride; }
};

// A free function: it needs no map.  path = m sphere centres (m x 3), radius and times m each (times e.g. from pct_time_allocation),
// orders m each (5..12), start / end = p, v, a (9 doubles).  params: pct_trajgen_params (limits, margin, eps, iteration budget).
// out.results[k].status says what became of candidate k (PCT_GEN_OK, PCT_GEN_NOT_CONVERGED, PCT_GEN_INVALID).  Returns the number of
// candidates that are PCT_GEN_OK.
inline int64_t generateTrajectories(const double *path, const double *radius, const double *times, const int32_t *orders, int32_t m,
                                    const double *scales, int64_t K, const double start[9], const double end[9],
                                    const pct_trajgen_params &params, GeneratedTrajectories &out)
{
    if (m < 1 || K < 0 || !path || !radius || !times || !orders || (K > 0 && !scales) || !start || !end)
        throw std::runtime_error("generateTrajectories: bad arguments");
    const size_t total = (size_t)K * (size_t)m;
    out.centres.resize(3 * total); out.radius.resize(total); out.seg_time.resize(total); out.orders.resize(total);
    out.seg_offsets.resize((size_t)K + 1); out.start_state.resize(9 * (size_t)K); out.end_state.resize(9 * (size_t)K);
    out.results.assign((size_t)K, pct_trajgen_result{});
    int32_t max_order = 0;
    for (int32_t s = 0; s < m; s++) max_order = orders[s] > max_order ? orders[s] : max_order;
    out.row_stride = 3 * (int64_t)((max_order > 12 ? 12 : max_order < 5 ? 5 : max_order) + 1);
    out.polycoef.assign(total * (size_t)out.row_stride, 0.0);
    out.seg_offsets[0] = 0;
    for (int64_t k = 0; k < K; k++) {
        for (int32_t s = 0; s < m; s++) {
            const size_t g = (size_t)k * (size_t)m + (size_t)s;
            for (int d = 0; d < 3; d++) out.centres[3 * g + d] = path[3 * s + d];
            out.radius[g] = radius[s];
            out.seg_time[g] = times[s] * scales[k];
            out.orders[g] = orders[s];
        }
        out.seg_offsets[(size_t)k + 1] = (int32_t)((k + 1) * m);
        for (int i = 0; i < 9; i++) { out.start_state[9 * (size_t)k + i] = start[i]; out.end_state[9 * (size_t)k + i] = end[i]; }
    }
    const pct_trajgen_batch b{ out.centres.data(), out.radius.data(), out.seg_time.data(), out.orders.data(), out.seg_offsets.data(),
                               out.start_state.data(), out.end_state.data(), K };
    if (pct_bezier_generate_batch(&b, &params, out.polycoef.data(), out.row_stride, out.results.data()) != PCT_OK)
        throw std::runtime_error(std::string("pct_bezier_generate_batch: ") + pct_last_error());
    int64_t ok = 0;
    for (const pct_trajgen_result &r : out.results) ok += r.status == PCT_GEN_OK ? 1 : 0;
    return ok;
}

// The same in a polyhedral corridor (pct_trajgen.h, paragraph "Trajectory generation in polyhedra"): waypoints = m + 1 route points
// ((m + 1) x 3), segment s runs along the edge waypoints[s] -> waypoints[s + 1] inside the polytope planes[plane_offsets[s] ..
// plane_offsets[s + 1]) (4 doubles each: n0 n1 n2 off, n . y <= off; plane_offsets has m + 1 entries, as ObstacleMap::segmentPolyhedra
// fills them; at most pct_trajgen_max_planes() planes per edge).  The start iterate of a segment is its edge's midpoint.  times and
// orders are m each; the caller supplies the times.  Returns the number of candidates that are PCT_GEN_OK; results[k].sphere_slack is
// the corridor slack.
inline int64_t generateTrajectoriesInPolyhedra(const double *waypoints, const double *planes, const int64_t *plane_offsets, const double *times,
                                               const int32_t *orders, int32_t m, const double *scales, int64_t K, const double start[9],
                                               const double end[9], const pct_trajgen_params &params, GeneratedTrajectories &out)
{
    if (m < 1 || K < 0 || !waypoints || !plane_offsets || !times || !orders || (K > 0 && !scales) || !start || !end || plane_offsets[0] != 0)
        throw std::runtime_error("generateTrajectoriesInPolyhedra: bad arguments");
    for (int32_t s = 0; s < m; s++)
        if (plane_offsets[s + 1] < plane_offsets[s]) throw std::runtime_error("generateTrajectoriesInPolyhedra: plane_offsets descend");
    const int64_t np = plane_offsets[m];
    if (np > 0 && !planes) throw std::runtime_error("generateTrajectoriesInPolyhedra: bad arguments");
    const size_t total = (size_t)K * (size_t)m;
    out.centres.resize(3 * total); out.radius.clear(); out.seg_time.resize(total); out.orders.resize(total);
    out.seg_offsets.resize((size_t)K + 1); out.start_state.resize(9 * (size_t)K); out.end_state.resize(9 * (size_t)K);
    out.planes.resize(4 * (size_t)K * (size_t)np + 4); out.plane_offsets.resize(total + 1);
    out.results.assign((size_t)K, pct_trajgen_result{});
    int32_t max_order = 0;
    for (int32_t s = 0; s < m; s++) max_order = orders[s] > max_order ? orders[s] : max_order;
    out.row_stride = 3 * (int64_t)((max_order > 12 ? 12 : max_order < 5 ? 5 : max_order) + 1);
    out.polycoef.assign(total * (size_t)out.row_stride, 0.0);
    out.seg_offsets[0] = 0;
    out.plane_offsets[0] = 0;
    for (int64_t k = 0; k < K; k++) {
        for (int32_t s = 0; s < m; s++) {
            const size_t g = (size_t)k * (size_t)m + (size_t)s;
            for (int d = 0; d < 3; d++) out.centres[3 * g + d] = 0.5 * (waypoints[3 * s + d] + waypoints[3 * (s + 1) + d]);
            out.seg_time[g] = times[s] * scales[k];
            out.orders[g] = orders[s];
            out.plane_offsets[g + 1] = (int32_t)(k * np + plane_offsets[s + 1]);
        }
        for (int64_t j = 0; j < 4 * np; j++) out.planes[(size_t)(4 * k * np + j)] = planes[j];
        out.seg_offsets[(size_t)k + 1] = (int32_t)((k + 1) * m);
        for (int i = 0; i < 9; i++) { out.start_state[9 * (size_t)k + i] = start[i]; out.end_state[9 * (size_t)k + i] = end[i]; }
    }
    const pct_trajgen_poly_batch b{ out.centres.data(), out.planes.data(), out.plane_offsets.data(), out.seg_time.data(), out.orders.data(),
                                    out.seg_offsets.data(), out.start_state.data(), out.end_state.data(), K };
    if (pct_bezier_generate_poly_batch(&b, &params, out.polycoef.data(), out.row_stride, out.results.data()) != PCT_OK)
        throw std::runtime_error(std::string("pct_bezier_generate_poly_batch: ") + pct_last_error());
    int64_t ok = 0;
    for (const pct_trajgen_result &r : out.results) ok += r.status == PCT_GEN_OK ? 1 : 0;
    return ok;
}

class ObstacleMap {
public:
    explicit ObstacleMap(int64_t capacity = 1 << 20, int device = 0) : capacity_(capacity)
    {
        check(pct_init(device), "pct_init");
        check(pct_cloud_create(capacity, &cloud_), "pct_cloud_create");
    }
    ~ObstacleMap() { if (cloud_) pct_cloud_destroy(cloud_); }
    ObstacleMap(const ObstacleMap &) = delete;
    ObstacleMap &operator=(const ObstacleMap &) = delete;

    // corridor_finder.cpp:17-23
    void setParam(double safety_margin, double search_margin, double max_radius, double sample_range)
    {
        safety_margin_ = safety_margin;
        prm_.search_margin = search_margin;
        prm_.max_radius = max_radius;
        prm_.sample_range = sample_range;
    }
    // corridor_finder.cpp:43-50 (start_pt) and :87 (setPt overwrites sample_range with local_range)
    void setStartPt(const double start[3]) { for (int i = 0; i < 3; i++) prm_.start[i] = start[i]; }
    void setSampleRange(double local_range) { prm_.sample_range = local_range; }

    // corridor_finder.cpp:93-99.  stride_bytes = 16 for pcl::PointXYZ (cloud.points.data()), 12 for packed xyz.
    // build_index: also build the cell index used by the batched queries (worth it for static clouds).
    void setInput(const void *points, int64_t n, int64_t stride_bytes = 16, bool build_index = true)
    {
        if (n > capacity_) {   // grow: the reference accepts any cloud size.  The larger cloud is created FIRST: if that fails
            pct_cloud *bigger = nullptr;   // (check throws) the map keeps its old, valid cloud
            const int64_t cap = n + n / 2;
            check(pct_cloud_create(cap, &bigger), "pct_cloud_create");
            if (rolling_ && pct_cloud_ring_index(bigger, 0.0f, nullptr) != PCT_OK) {
                pct_cloud_destroy(bigger);
                check(PCT_ERR_HIP, "pct_cloud_ring_index");
            }
            if (rolling_ && dedup_res_ > 0 && pct_cloud_ring_dedup(bigger, dedup_res_) != PCT_OK) {     // the larger cloud keeps the mode
                pct_cloud_destroy(bigger);
                check(PCT_ERR_HIP, "pct_cloud_ring_dedup");
            }
            if (rolling_ && compact_fraction_ > 0 && pct_cloud_ring_autocompact(bigger, compact_fraction_) != PCT_OK) {
                pct_cloud_destroy(bigger);
                check(PCT_ERR_HIP, "pct_cloud_ring_autocompact");
            }
            pct_cloud_destroy(cloud_);
            cloud_ = bigger;
            capacity_ = cap;
        }
        check(pct_cloud_upload_aos(cloud_, points, n, stride_bytes), "pct_cloud_upload_aos");
        cloud_empty_ = (n == 0);
        if (build_index && n > 0 && !rolling_) check(pct_cloud_build_grid(cloud_, 0.0f), "pct_cloud_build_grid");
    }
    // rolling map with the in-place index (config C5): call once before the first appendInput; appends then update the index
    // instead of dropping it, and every query below searches it
    void enableRollingIndex(float cell_size = 0.0f, const float *extent = nullptr)
    {
        check(pct_cloud_ring_index(cloud_, cell_size, extent), "pct_cloud_ring_index");
        rolling_ = true;
    }
    // rolling map as a window of UNIQUE voxels (pct_cloud_ring_dedup): after enableRollingIndex; res > 0: appendInput keeps only the
    // points whose voxel (pct_voxel.h's round(p / res)) is new to the window -- a sensor that re-emits the same surface lattice frame
    // after frame (the reference's rgbd mode) then fills the window with geometry instead of copies; res = 0: off.  Every keyed
    // point of a frame has its voxel in the window after that frame's append.  setInput (replace) is not filtered.
    void setRollingDedup(double res)
    {
        check(pct_cloud_ring_dedup(cloud_, res), "pct_cloud_ring_dedup");
        dedup_res_ = res;
    }
    // rolling map (config C5): append the newest sensor frame, evicting the oldest points
    void appendInput(const void *points, int64_t n, int64_t stride_bytes = 16)
    {
        check(pct_cloud_append_aos(cloud_, points, n, stride_bytes), "pct_cloud_append_aos");
        cloud_empty_ = pct_cloud_size(cloud_) == 0;
    }

    // Removing points from the rolling map (pct_engine.h, paragraph "Removing points"): a removed point becomes a NaN row -- never a
    // neighbour on any path -- and every other point keeps its index; a window left without a point becomes the empty cloud.  Each
    // call returns the number of points it removed and needs enableRollingIndex.
    //   forgetOutside   the window follows the drone: what the reference's lidar mode gets by replacing the planner's cloud with
    //                   crop(global map, drone, max_dist) every frame (camera_sensor.cpp:133-145, sim_planning_demo.cpp:159-167)
    //   clearBall / clearBox   withdraw a stale obstacle: a region the sensor now sees as free
    //   removePoints    the indices a search reported (radiusSearchBatch, radiusIndices, nearest); a point named twice counts once
    int64_t forgetOutside(const double centre[3], double r) { return removeBall(centre, r, 1); }
    int64_t clearBall(const double centre[3], double r) { return removeBall(centre, r, 0); }
    int64_t clearBox(const double lo[3], const double hi[3])
    {
        needRolling("clearBox");
        int64_t removed = 0;
        check(pct_cloud_ring_remove_box(cloud_, lo, hi, 0, &removed), "pct_cloud_ring_remove_box");
        cloud_empty_ = pct_cloud_size(cloud_) == 0;
        return removed;
    }
    int64_t removePoints(const uint32_t *indices, int64_t n)
    {
        needRolling("removePoints");
        int64_t removed = 0;
        check(pct_cloud_ring_remove_indices(cloud_, indices, n, &removed), "pct_cloud_ring_remove_indices");
        cloud_empty_ = pct_cloud_size(cloud_) == 0;
        return removed;
    }
    // points of the window that are still there (rows without a NaN coordinate); size() counts the removed slots too
    int64_t liveSize()
    {
        needRolling("liveSize");
        int64_t live = 0, gone = 0;
        check(pct_cloud_ring_live(cloud_, &live, &gone), "pct_cloud_ring_live");
        return live;
    }

    // Compacting the window (pct_engine.h, paragraph "Compacting the window"; needs enableRollingIndex): removed slots stay below size()
    // and the ring cursor overwrites live and dead slots alike, so a full window that was thinned evicts live points while dead slots
    // sit unused.  A compaction moves the live points to slots 0 .. L-1, oldest first, files the table again and lets the next
    // appends fill the reclaimed slots.  Indices change: remap (may be null; remap_cap >= size()) receives the new index of every
    // old slot, or PCT_NO_INDEX.
    //   compactWindow      compact now; returns the number of slots reclaimed
    //   setRollingCompact  dead_fraction > 0: every removal above (and clearSeenThrough) that leaves that share of the capacity dead
    //                      compacts before it returns; 0 = off (default)
    //   compactions        compactions that moved points so far: indices held across a call are stale when it has changed
    int64_t compactWindow(uint32_t *remap = nullptr, int64_t remap_cap = 0)
    {
        needRolling("compactWindow");
        int64_t live = 0, reclaimed = 0;
        check(pct_cloud_ring_compact(cloud_, &live, &reclaimed, remap, remap_cap), "pct_cloud_ring_compact");
        cloud_empty_ = pct_cloud_size(cloud_) == 0;
        return reclaimed;
    }
    void setRollingCompact(double dead_fraction)
    {
        check(pct_cloud_ring_autocompact(cloud_, dead_fraction), "pct_cloud_ring_autocompact");
        compact_fraction_ = dead_fraction;
    }
    uint64_t compactions()
    {
        uint64_t n = 0;
        check(pct_cloud_ring_compact_count(cloud_, &n), "pct_cloud_ring_compact_count");
        return n;
    }

    // Removing outliers (pct_engine.h, paragraph "Removing outliers"; needs enableRollingIndex): a flying pixel at a depth edge or a
    // speckle in free space is one obstacle point that closes a corridor; the radius rule withdraws it before the planner sees it.
    //   removeOutliers    of the `newest` most recent points (0: every point), those with fewer than min_neighbours other points of
    //                     the window within r are removed -- one judgement on the window as it is, then one removal; returns the
    //                     number removed.  newest = what the append just made kept is the per-frame filter.
    //   neighbourCounts   the same judgement without the removal: per slot min(neighbours, count_cap), PCT_NO_INDEX for a slot that
    //                     holds no point or is out of scope
    int64_t removeOutliers(double r, int min_neighbours, int64_t newest = 0)
    {
        needRolling("removeOutliers");
        int64_t removed = 0;
        check(pct_cloud_ring_remove_outliers(cloud_, r, min_neighbours, newest, &removed), "pct_cloud_ring_remove_outliers");
        cloud_empty_ = pct_cloud_size(cloud_) == 0;
        return removed;
    }
    std::vector<uint32_t> neighbourCounts(double r, int count_cap, int64_t newest = 0)
    {
        needRolling("neighbourCounts");
        std::vector<uint32_t> counts((size_t)pct_cloud_size(cloud_));
        check(pct_cloud_ring_neighbour_counts(cloud_, r, count_cap, newest, counts.data(), (int64_t)counts.size()), "pct_cloud_ring_neighbour_counts");
        return counts;
    }

    // Statistical outliers (pct_engine.h, paragraph "Statistical outliers"; needs enableRollingIndex): the rule for a sensor whose
    // density falls with range, where no single r of the radius rule fits -- a point is judged by the mean distance to its k nearest
    // other points of the window.
    //   removeStatisticalOutliers   of the `newest` most recent points (0: every point), those whose mean distance is greater than
    //                               mean + stddev_mult * stddev over the judged points are removed; returns the number removed and,
    //                               through `stats` (may be null), the statistics with the threshold it used
    //   removeIsolated              the same removal under a fixed threshold -- the per-frame call, with the threshold an occasional
    //                               whole-window removeStatisticalOutliers delivered and newest = what the append just made kept
    //   knnMeanDistances            the judgement without the removal: per slot the mean distance, +inf with fewer than k other
    //                               points, NaN for a slot that holds no point or is out of scope
    //   knnDistanceStats            the statistics without the removal
    int64_t removeStatisticalOutliers(int k, double stddev_mult, int64_t newest = 0, pct_knn_stats *stats = nullptr)
    {
        needRolling("removeStatisticalOutliers");
        int64_t removed = 0;
        check(pct_cloud_ring_remove_statistical(cloud_, k, stddev_mult, newest, &removed, stats), "pct_cloud_ring_remove_statistical");
        cloud_empty_ = pct_cloud_size(cloud_) == 0;
        return removed;
    }
    int64_t removeIsolated(int k, double max_mean_distance, int64_t newest = 0)
    {
        needRolling("removeIsolated");
        int64_t removed = 0;
        check(pct_cloud_ring_remove_isolated(cloud_, k, max_mean_distance, newest, &removed), "pct_cloud_ring_remove_isolated");
        cloud_empty_ = pct_cloud_size(cloud_) == 0;
        return removed;
    }
    std::vector<double> knnMeanDistances(int k, int64_t newest = 0)
    {
        needRolling("knnMeanDistances");
        const size_t n = (size_t)pct_cloud_size(cloud_);
        std::vector<double> mean(n ? n : 1);
        check(pct_cloud_ring_knn_mean_distances(cloud_, k, newest, mean.data(), (int64_t)mean.size()), "pct_cloud_ring_knn_mean_distances");
        mean.resize(n);
        return mean;
    }
    pct_knn_stats knnDistanceStats(int k, double stddev_mult, int64_t newest = 0)
    {
        needRolling("knnDistanceStats");
        pct_knn_stats stats{};
        check(pct_cloud_ring_knn_distance_stats(cloud_, k, stddev_mult, newest, &stats), "pct_cloud_ring_knn_distance_stats");
        return stats;
    }

    // Depth images on the rolling map (pct_engine.h, paragraph "Depth images"; both need enableRollingIndex).  The rgbd tick is
    // clearSeenThrough(image) then appendDepthImage(the same image): carve first, then append, with a small positive margin so that
    // the next frame's carve leaves the points this frame appended alone.
    //   clearSeenThrough   free-space clearing: removes every point the image sees through -- a point in the image whose pixel is
    //                      finite and shows a surface strictly farther than the point plus margin
    //                      (safety_controller::check_image_for_point, safety_controller.cpp:102-130); returns the number removed
    //   appendDepthImage   un-projects the valid pixels (finite, near_z <= depth <= max_depth) on the device
    //                      (img_pcl_map_observer::save_point, map_observer.cpp:92-100) and appends them as appendInput appends the
    //                      same points; returns the number of points the window took
    int64_t clearSeenThrough(const pct_depth_view &view, const float *image, double margin)
    {
        needRolling("clearSeenThrough");
        int64_t removed = 0;
        check(pct_cloud_ring_carve_depth(cloud_, &view, image, margin, &removed), "pct_cloud_ring_carve_depth");
        cloud_empty_ = pct_cloud_size(cloud_) == 0;
        return removed;
    }
    int64_t appendDepthImage(const pct_depth_view &view, const float *image, double max_depth)
    {
        needRolling("appendDepthImage");
        int64_t offered = 0, kept = 0;
        check(pct_cloud_append_depth(cloud_, &view, image, max_depth, &offered, &kept), "pct_cloud_append_depth");
        cloud_empty_ = pct_cloud_size(cloud_) == 0;
        return kept;
    }

    // Range images on the rolling map (pct_engine.h, paragraph "Range images"; both need enableRollingIndex): the organised scan of a
    // lidar, rings by columns, with the caller's edge and direction tables in the view.  The lidar tick is clearSeenThroughRange(scan)
    // then appendRangeImage(the same scan): carve first, then append, with a small positive margin.
    //   clearSeenThroughRange   removes every point the scan sees through -- a point in the image whose pixel is finite and shows a
    //                           return strictly farther than the point plus margin; returns the number removed
    //   appendRangeImage        un-projects the valid pixels (finite, near_range <= range <= max_range) on the device and appends
    //                           them as appendInput appends the same points; returns the number of points the window took
    int64_t clearSeenThroughRange(const pct_range_view &view, const float *image, double margin)
    {
        needRolling("clearSeenThroughRange");
        int64_t removed = 0;
        check(pct_cloud_ring_carve_range(cloud_, &view, image, margin, &removed), "pct_cloud_ring_carve_range");
        cloud_empty_ = pct_cloud_size(cloud_) == 0;
        return removed;
    }
    int64_t appendRangeImage(const pct_range_view &view, const float *image, double max_range)
    {
        needRolling("appendRangeImage");
        int64_t offered = 0, kept = 0;
        check(pct_cloud_append_range(cloud_, &view, image, max_range, &offered, &kept), "pct_cloud_append_range");
        cloud_empty_ = pct_cloud_size(cloud_) == 0;
        return kept;
    }

    // corridor_finder.cpp:113-133
    double radiusSearch(const double p[3])
    {
        double r = 0;
        check(pct_inflate_batch(cloud_, &prm_, p, 1, &r, nullptr, nullptr), "pct_inflate_batch");
        return r;
    }
    double checkRadius(const double p[3]) { return radiusSearch(p); }               // :656-659
    bool checkTrajPtCol(const double p[3]) { return radiusSearch(p) < 0.0; }        // :412-416

    // the independent re-checks of SafeRegionEvaluate (:829-835) / treeRepair (:958-974) as ONE launch
    void checkRadiusBatch(const double *pts, int64_t n, double *radius, uint32_t *nn_index = nullptr, double *nn_d2 = nullptr)
    {
        check(pct_inflate_batch(cloud_, &prm_, pts, n, radius, nn_index, nn_d2), "pct_inflate_batch");
    }
    // Segment queries (pct_engine.h, paragraph "Segment queries"): what lies between two points, without sampling the line.
    // segments: n x 6 doubles, a then b.
    //   segmentSearch    the nearest obstacle point within `reach` of each segment: index (PCT_NO_INDEX: none that near), d2 and the
    //                    parameter s of the closest point on the segment (0 at a, 1 at b); d2 / s may be null.  On an empty map every
    //                    segment reports "none".
    //   checkSegments    capsule inflation with the map's own parameters: radius = min(distance to the nearest obstacle point -
    //                    search_margin, max_radius), radius < 0 <=> the segment collides with the margin, as checkTrajPtCol judges a
    //                    point; no start-distance early-out.  nn_index / s name the nearest point where radius < max_radius.
    //   segmentCollides  one segment: is the straight line from a to b blocked?
    void segmentSearch(const double *segments, int64_t n, double reach, uint32_t *index, double *d2, double *s)
    {
        const std::vector<double> reaches((size_t)(n > 0 ? n : 0), reach);
        check(pct_segment_nn_batch(cloud_, PCT_ALGO_AUTO, segments, reaches.data(), n, index, d2, s), "pct_segment_nn_batch");
    }
    void checkSegments(const double *segments, int64_t n, double *radius, uint32_t *nn_index = nullptr, double *s = nullptr)
    {
        check(pct_segment_inflate_batch(cloud_, &prm_, segments, n, radius, nn_index, s), "pct_segment_inflate_batch");
    }
    bool segmentCollides(const double a[3], const double b[3])
    {
        const double seg[6] = { a[0], a[1], a[2], b[0], b[1], b[2] };
        double r = 0;
        checkSegments(seg, 1, &r);
        return r < 0.0;
    }
    // Segment sweeps (pct_engine.h, paragraph "Segment sweeps"): how far a sphere gets along a straight line, and what stops it.
    //   sweepSegments  for each segment a -> b the point a sphere of `radius` touches first (PCT_NO_INDEX: none) and the parameter t
    //                  its centre reaches: 0 = in contact at a, 1 = the whole segment is free; t may be null.  On an empty map every
    //                  segment is free.
    //   freeFraction   one sweep with the map's own search_margin as the radius: the fraction of a -> b that can be flown.
    // Contact is INCLUSIVE here -- a point at exactly the radius stops the sphere -- whereas checkTrajPtCol collides on a strict `<`
    // (radius < 0): a line that passes an obstacle point at exactly search_margin has freeFraction < 1 and segmentCollides false.
    void sweepSegments(const double *segments, int64_t n, double radius, uint32_t *index, double *t)
    {
        const std::vector<double> radii((size_t)(n > 0 ? n : 0), radius);
        check(pct_segment_sweep_batch(cloud_, PCT_ALGO_AUTO, segments, radii.data(), n, index, t), "pct_segment_sweep_batch");
    }
    double freeFraction(const double a[3], const double b[3])
    {
        const double seg[6] = { a[0], a[1], a[2], b[0], b[1], b[2] };
        uint32_t index = 0;
        double t = 0;
        sweepSegments(seg, 1, prm_.search_margin, &index, &t);
        return t;
    }
    // Capsule search (pct_engine.h, paragraph "Capsule search"): the obstacle points within `reach` of each segment, as lists -- the
    // input of a free-space decomposition around an edge, the constraints of a local optimiser, a crop before a finer check.
    // segments: n x 6 doubles, a then b.
    //   segmentNeighbours  row i of the result = indices / sqr_distances (/ params) entries [offsets[i], offsets[i + 1]), offsets has
    //                      n + 1 entries; params (optional) receives the parameter of the closest point on the segment (0 at a, 1 at b).
    //                      sorted: nearest first, ties in ascending index; otherwise ascending index.
    //   segmentCounts      just the row lengths.
    // A point at exactly `reach` is listed (inclusive).  The walk follows the map's index: the rolling-map bucket table, the cell index,
    // or neither.  On an empty map every row is empty.
    void segmentNeighbours(const std::vector<double> &segments, double reach, std::vector<int64_t> &offsets, std::vector<uint32_t> &indices,
                           std::vector<double> &sqr_distances, std::vector<double> *params = nullptr, bool sorted = true)
    {
        const int64_t n = (int64_t)(segments.size() / 6);
        const std::vector<double> reaches((size_t)n, reach);
        offsets.assign((size_t)n + 1, 0);
        int64_t total = 0;
        check(pct_segment_search_batch(cloud_, PCT_ALGO_AUTO, segments.data(), reaches.data(), n, sorted ? PCT_ORDER_DISTANCE : PCT_ORDER_INDEX,
                                       offsets.data(), &total), "pct_segment_search_batch");
        indices.resize((size_t)total);
        sqr_distances.resize((size_t)total);
        if (params) params->resize((size_t)total);
        check(pct_segment_search_read(cloud_, 0, total, indices.data(), sqr_distances.data(), params ? params->data() : nullptr),
              "pct_segment_search_read");
    }
    void segmentCounts(const std::vector<double> &segments, double reach, std::vector<uint32_t> &counts)
    {
        const int64_t n = (int64_t)(segments.size() / 6);
        const std::vector<double> reaches((size_t)n, reach);
        counts.assign((size_t)n, 0u);
        check(pct_segment_count_batch(cloud_, PCT_ALGO_AUTO, segments.data(), reaches.data(), n, counts.data()), "pct_segment_count_batch");
    }
    // Free-space polyhedra (pct_engine.h, paragraph "Free-space polyhedra"): a bounded convex region around each segment that holds
    // the segment and no obstacle point closer than `margin` to its faces' inside -- what a QP / SOCP corridor constraint takes.
    // segments: n x 6 doubles, a then b.  Row i of the result = planes entries [offsets[i], offsets[i + 1]), 4 doubles each
    // (nh0 nh1 nh2 off: the half-space nh . y <= off), offsets has n + 1 entries:
    //   * first the support planes of the segment's capsule row, each with its off reduced by `margin` (the robot's size: the region
    //     is margin-clear of every obstacle point within `reach` of the segment);
    //   * then six planes of a box that lies INSIDE the capsule (segment, reach), which turns "nothing is claimed outside the
    //     capsule" into "the polytope is free": half-width reach / sqrt(3) across the segment, from -reach / sqrt(3) to
    //     |b - a| + reach / sqrt(3) along it, so that its farthest corners are at distance reach from the segment.  Its frame: t =
    //     e / |e|, u perpendicular to t built from the coordinate axis of smallest |t_k| (the lowest k on ties), v = t x u; the
    //     coordinate axes for a == b.  The box is plain host arithmetic on the fp32-narrowed ends, not bit-pinned.
    // A segment that collides -- its nearest support lies at d2 <= margin^2, a point on the segment included -- is reported by an
    // EMPTY row: no polytope around it contains it.  So is a segment with a non-finite end or a reach that is not a finite number
    // >= 0.  Every non-empty row therefore has at least six planes and contains its segment.  indices (optional): per plane the
    // obstacle point that supports it, PCT_NO_INDEX for the six box planes.
    void segmentPolyhedra(const std::vector<double> &segments, double reach, double margin, std::vector<int64_t> &offsets,
                          std::vector<double> &planes, std::vector<uint32_t> *indices = nullptr)
    {
        const int64_t n = (int64_t)(segments.size() / 6);
        const std::vector<double> reaches((size_t)n, reach);
        std::vector<int64_t> sup((size_t)n + 1, 0);
        int64_t total = 0;
        const int st = pct_segment_polyhedron_batch(cloud_, PCT_ALGO_AUTO, segments.data(), reaches.data(), n, sup.data(), &total);
        if (st != PCT_ERR_EMPTY) check(st, "pct_segment_polyhedron_batch");      // an empty map: no supports, the boxes alone
        std::vector<uint32_t> idx((size_t)total);
        std::vector<double> d2((size_t)total), pl(4 * (size_t)total);
        check(pct_segment_polyhedron_read(cloud_, 0, total, idx.data(), d2.data(), nullptr, pl.data()), "pct_segment_polyhedron_read");
        offsets.assign((size_t)n + 1, 0);
        planes.clear();
        if (indices) indices->clear();
        const auto put = [&](double n0, double n1, double n2, double off, uint32_t id) {
            planes.push_back(n0); planes.push_back(n1); planes.push_back(n2); planes.push_back(off);
            if (indices) indices->push_back(id);
        };
        for (int64_t i = 0; i < n; i++) {
            const double *sg = &segments[6 * (size_t)i];
            double a[3], e[3], t[3] = { 1.0, 0.0, 0.0 }, u[3] = { 0.0, 1.0, 0.0 }, v[3] = { 0.0, 0.0, 1.0 };
            bool valid = std::isfinite(reach) && reach >= 0.0;
            for (int k = 0; k < 3; k++) {
                const float fa = (float)sg[k], fb = (float)sg[3 + k];
                a[k] = (double)fa;
                e[k] = (double)fb - (double)fa;
                valid = valid && std::isfinite(fa) && std::isfinite(fb);
            }
            const bool collides = sup[i + 1] > sup[i] && d2[(size_t)sup[i]] <= margin * margin;      // the first support is the nearest
            if (valid && !collides) {
                for (int64_t j = sup[i]; j < sup[i + 1]; j++) put(pl[4 * j], pl[4 * j + 1], pl[4 * j + 2], pl[4 * j + 3] - margin, idx[(size_t)j]);
                const double len = std::sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
                if (len > 0.0) {
                    for (int k = 0; k < 3; k++) t[k] = e[k] / len;
                    int m = 0;
                    for (int k = 1; k < 3; k++) if (std::fabs(t[k]) < std::fabs(t[m])) m = k;
                    double ul = 0.0;
                    for (int k = 0; k < 3; k++) { u[k] = (k == m ? 1.0 : 0.0) - t[m] * t[k]; ul += u[k] * u[k]; }
                    ul = std::sqrt(ul);                                           // >= sqrt(2 / 3): |t_m| <= 1 / sqrt(3)
                    for (int k = 0; k < 3; k++) u[k] /= ul;
                    v[0] = t[1] * u[2] - t[2] * u[1]; v[1] = t[2] * u[0] - t[0] * u[2]; v[2] = t[0] * u[1] - t[1] * u[0];
                }
                const double hw = reach / std::sqrt(3.0);
                const double ta = (t[0] * a[0] + t[1] * a[1]) + t[2] * a[2], ua = (u[0] * a[0] + u[1] * a[1]) + u[2] * a[2],
                             va = (v[0] * a[0] + v[1] * a[1]) + v[2] * a[2];
                put(t[0], t[1], t[2], ta + len + hw, PCT_NO_INDEX);
                put(-t[0], -t[1], -t[2], hw - ta, PCT_NO_INDEX);
                put(u[0], u[1], u[2], ua + hw, PCT_NO_INDEX);
                put(-u[0], -u[1], -u[2], hw - ua, PCT_NO_INDEX);
                put(v[0], v[1], v[2], va + hw, PCT_NO_INDEX);
                put(-v[0], -v[1], -v[2], hw - va, PCT_NO_INDEX);
            }
            offsets[(size_t)i + 1] = (int64_t)(planes.size() / 4);
        }
    }
    // corridor_finder.cpp:661-669
    int checkNodeUpdate(double new_radius, double old_radius) const
    {
        if (new_radius < safety_margin_) return -1;
        if (new_radius < old_radius) return 0;
        return 1;
    }

    // sim_planning_demo.cpp:729-781.  poly_coeff: segments x row_stride row-major (the MatrixXd the optimiser
    // returns, traj_optimizer.cpp:739-751, is column-major: pass PolyCoeff.transpose().eval().data() or a
    // RowMajor copy); seg_time = _Time; orders = _poly_orderList; t_now = max(0, odom stamp - start time).
    // Returns true on collision like the reference; *first_hit_sample (optional) is the index of that sample.
    bool checkSafeTrajectory(const double *poly_coeff, int64_t row_stride, const double *seg_time, const int32_t *orders,
                             int32_t segment_num, double t_now, double stop_time, int64_t *first_hit_sample = nullptr,
                             int64_t *samples = nullptr)
    {
        pct_bezier_traj tr{ poly_coeff, row_stride, seg_time, orders, segment_num };
        int64_t fh = -1, ns = 0;
        check(pct_bezier_check(cloud_, &tr, &prm_, t_now, stop_time, 0.02, &fh, &ns, 4096, nullptr, nullptr, nullptr, nullptr),
              "pct_bezier_check");
        if (first_hit_sample) *first_hit_sample = fh;
        if (samples) *samples = ns;
        return fh >= 0;
    }

    // The same check for a set of candidates over this map in ONE call (pct_engine.h, paragraph "Batched Bezier check"): the same
    // corridor under several time allocations, evasive variants, a fan of primitives.  Same dt = 0.02 and cap = 4096 as
    // checkSafeTrajectory; candidates.t_start = each candidate's t_now (NULL: 0).  verdicts[b]: the unclipped sample count, the first
    // colliding sample (-1: none) and -- what ranks the free candidates -- the smallest radius with the lowest sample that attains it.
    // Returns the number of colliding candidates.
    int64_t checkSafeTrajectories(const pct_bezier_batch &candidates, double stop_time, std::vector<pct_traj_verdict> &verdicts)
    {
        verdicts.resize((size_t)(candidates.B > 0 ? candidates.B : 0));
        check(pct_bezier_check_batch(cloud_, &candidates, &prm_, stop_time, 0.02, 4096, verdicts.data(), nullptr, 0, nullptr, nullptr, nullptr,
                                     nullptr),
              "pct_bezier_check_batch");
        int64_t colliding = 0;
        for (const pct_traj_verdict &v : verdicts) colliding += v.first_hit >= 0 ? 1 : 0;
        return colliding;
    }

    // The certified check (pct_engine.h, paragraph "Certified Bezier check"): whole candidates proven free of the map by
    // search_margin (setParam) or shown to collide, by subdivision -- no dt, no sampling gap, and the work follows how close a curve
    // comes to the obstacles.  candidates.t_start is not read: a horizon is the segments that cover it.  certificates[b].status is
    // PCT_CERT_FREE (a proof), PCT_CERT_HIT (hit_seg / hit_u / hit_idx say where and against which point), PCT_CERT_UNDECIDED (closer
    // than max_depth halvings could tell: treat as not free) or PCT_CERT_INVALID.  piece_cap 0: 64 pieces per segment, at least 4096.
    // stats (optional): {rounds, pieces examined, capped}.  Returns the number of candidates that are NOT certified free.
    int64_t certifyTrajectories(const pct_bezier_batch &candidates, std::vector<pct_traj_certificate> &certificates, int max_depth = 12,
                                int64_t piece_cap = 0, int64_t *stats = nullptr)
    {
        const int64_t B = candidates.B > 0 ? candidates.B : 0;
        certificates.resize((size_t)B);
        if (piece_cap <= 0) {
            const int64_t nseg = B > 0 && candidates.seg_offsets ? candidates.seg_offsets[B] : 0;
            piece_cap = 64 * nseg > 4096 ? 64 * nseg : 4096;
        }
        check(pct_bezier_certify_batch(cloud_, PCT_ALGO_AUTO, &candidates, prm_.search_margin, max_depth, piece_cap, certificates.data(), stats),
              "pct_bezier_certify_batch");
        int64_t not_free = 0;
        for (const pct_traj_certificate &v : certificates) not_free += v.status != PCT_CERT_FREE ? 1 : 0;
        return not_free;
    }
    // One trajectory, the arguments of checkSafeTrajectory without its times: true unless the whole trajectory is certified free
    // (the reference's sense: true = do not fly it).  certificate (optional) receives the details.
    bool certifySafeTrajectory(const double *poly_coeff, int64_t row_stride, const double *seg_time, const int32_t *orders,
                               int32_t segment_num, pct_traj_certificate *certificate = nullptr, int max_depth = 12)
    {
        const int32_t seg_offsets[2] = { 0, segment_num };
        const pct_bezier_batch one{ poly_coeff, row_stride, seg_time, orders, seg_offsets, nullptr, 1 };
        std::vector<pct_traj_certificate> cert;
        const int64_t not_free = certifyTrajectories(one, cert, max_depth);
        if (certificate) *certificate = cert[0];
        return not_free != 0;
    }

    // The clearance (pct_engine.h, paragraph "Trajectory clearance"): how close each whole candidate comes to the map, as a bracket
    // clearances[b].lo <= clearance <= clearances[b].hi no wider than tol metres (status PCT_CLR_DONE) -- the number to rank candidates
    // by once all of them pass.  cap: clearance beyond it is of no interest (a piece that far away retires at once).  PCT_CLR_OPEN:
    // max_depth halvings or piece_cap did not close the bracket; lo still holds.  at_seg / at_u / at_idx say where hi is attained and
    // against which point.  candidates.t_start is not read.  piece_cap 0: 64 pieces per segment, at least 4096.  stats (optional):
    // {rounds, pieces examined, capped}.  Returns the number of candidates whose bracket is NOT closed (status != PCT_CLR_DONE).
    int64_t trajectoryClearances(const pct_bezier_batch &candidates, std::vector<pct_traj_clearance> &clearances, double tol,
                                 double cap = std::numeric_limits<double>::infinity(), int max_depth = 16, int64_t piece_cap = 0,
                                 int64_t *stats = nullptr)
    {
        const int64_t B = candidates.B > 0 ? candidates.B : 0;
        clearances.resize((size_t)B);
        if (piece_cap <= 0) {
            const int64_t nseg = B > 0 && candidates.seg_offsets ? candidates.seg_offsets[B] : 0;
            piece_cap = 64 * nseg > 4096 ? 64 * nseg : 4096;
        }
        check(pct_bezier_clearance_batch(cloud_, PCT_ALGO_AUTO, &candidates, tol, cap, max_depth, piece_cap, clearances.data(), stats),
              "pct_bezier_clearance_batch");
        int64_t not_done = 0;
        for (const pct_traj_clearance &v : clearances) not_done += v.status != PCT_CLR_DONE ? 1 : 0;
        return not_done;
    }
    // One trajectory, the arguments of certifySafeTrajectory: its record
    pct_traj_clearance trajectoryClearance(const double *poly_coeff, int64_t row_stride, const double *seg_time, const int32_t *orders,
                                           int32_t segment_num, double tol, double cap = std::numeric_limits<double>::infinity(),
                                           int max_depth = 16)
    {
        const int32_t seg_offsets[2] = { 0, segment_num };
        const pct_bezier_batch one{ poly_coeff, row_stride, seg_time, orders, seg_offsets, nullptr, 1 };
        std::vector<pct_traj_clearance> rec;
        trajectoryClearances(one, rec, tol, cap, max_depth);
        return rec[0];
    }

    // The two checks above for a time window of each candidate (pct_engine.h, paragraph "Windows of a trajectory"): candidate b is
    // examined for t in [t_start[b], t_start[b] + horizons[b]] -- candidates.t_start IS read here (NULL: 0 for all), horizons holds B
    // values or is NULL (+inf for all).  A part already flown or beyond the horizon neither collides nor enters the bracket; hit_u /
    // at_u are in the segment's own parameter; a window at or past the end of a candidate is FREE / DONE with no piece examined.
    // Everything else, the return values included, as certifyTrajectories and trajectoryClearances.
    int64_t certifyTrajectoryWindows(const pct_bezier_batch &candidates, const double *horizons, std::vector<pct_traj_certificate> &certificates,
                                     int max_depth = 12, int64_t piece_cap = 0, int64_t *stats = nullptr)
    {
        const int64_t B = candidates.B > 0 ? candidates.B : 0;
        certificates.resize((size_t)B);
        if (piece_cap <= 0) {
            const int64_t nseg = B > 0 && candidates.seg_offsets ? candidates.seg_offsets[B] : 0;
            piece_cap = 64 * nseg > 4096 ? 64 * nseg : 4096;
        }
        check(pct_bezier_certify_window_batch(cloud_, PCT_ALGO_AUTO, &candidates, horizons, prm_.search_margin, max_depth, piece_cap,
                                              certificates.data(), stats),
              "pct_bezier_certify_window_batch");
        int64_t not_free = 0;
        for (const pct_traj_certificate &v : certificates) not_free += v.status != PCT_CERT_FREE ? 1 : 0;
        return not_free;
    }
    int64_t trajectoryClearanceWindows(const pct_bezier_batch &candidates, const double *horizons, std::vector<pct_traj_clearance> &clearances,
                                       double tol, double cap = std::numeric_limits<double>::infinity(), int max_depth = 16,
                                       int64_t piece_cap = 0, int64_t *stats = nullptr)
    {
        const int64_t B = candidates.B > 0 ? candidates.B : 0;
        clearances.resize((size_t)B);
        if (piece_cap <= 0) {
            const int64_t nseg = B > 0 && candidates.seg_offsets ? candidates.seg_offsets[B] : 0;
            piece_cap = 64 * nseg > 4096 ? 64 * nseg : 4096;
        }
        check(pct_bezier_clearance_window_batch(cloud_, PCT_ALGO_AUTO, &candidates, horizons, tol, cap, max_depth, piece_cap, clearances.data(),
                                                stats),
              "pct_bezier_clearance_window_batch");
        int64_t not_done = 0;
        for (const pct_traj_clearance &v : clearances) not_done += v.status != PCT_CLR_DONE ? 1 : 0;
        return not_done;
    }
    // The tick's question, the arguments of checkSafeTrajectory: is the committed trajectory safe from t_now for the next check_time
    // seconds?  True unless that window is certified free (the reference's sense: true = do not fly it); an obstacle beside the part
    // already flown, or beyond the horizon, does not force a replan.  certificate (optional) receives the details.
    bool certifySafeTrajectoryFrom(const double *poly_coeff, int64_t row_stride, const double *seg_time, const int32_t *orders,
                                   int32_t segment_num, double t_now, double check_time, pct_traj_certificate *certificate = nullptr,
                                   int max_depth = 12)
    {
        const int32_t seg_offsets[2] = { 0, segment_num };
        const pct_bezier_batch one{ poly_coeff, row_stride, seg_time, orders, seg_offsets, &t_now, 1 };
        std::vector<pct_traj_certificate> cert;
        const int64_t not_free = certifyTrajectoryWindows(one, &check_time, cert, max_depth);
        if (certificate) *certificate = cert[0];
        return not_free != 0;
    }
    // The same window's clearance record
    pct_traj_clearance trajectoryClearanceFrom(const double *poly_coeff, int64_t row_stride, const double *seg_time, const int32_t *orders,
                                               int32_t segment_num, double t_now, double check_time, double tol,
                                               double cap = std::numeric_limits<double>::infinity(), int max_depth = 16)
    {
        const int32_t seg_offsets[2] = { 0, segment_num };
        const pct_bezier_batch one{ poly_coeff, row_stride, seg_time, orders, seg_offsets, &t_now, 1 };
        std::vector<pct_traj_clearance> rec;
        trajectoryClearanceWindows(one, &check_time, rec, tol, cap, max_depth);
        return rec[0];
    }

    // Corridor -> trajectory -> proof in one call: generate one candidate per time scale (generateTrajectories above; limits carries
    // max_vel / max_acc and the iteration budget, its margin is replaced by `margin`, what is taken off every sphere radius), certify all
    // of them against this map (certifyTrajectories: search_margin of setParam) and return the index of the shortest-duration candidate
    // that is both PCT_GEN_OK and PCT_CERT_FREE, or -1 when there is none.  out.results and certificates hold both records of every
    // candidate; out.rows(k) / out.batch() are what flies.
    int64_t generateSafeTrajectory(const double *path, const double *radius, const double *times, const int32_t *orders, int32_t m,
                                   const double *scales, int64_t K, const double start[9], const double end[9], const pct_trajgen_params &limits,
                                   double margin, GeneratedTrajectories &out, std::vector<pct_traj_certificate> &certificates, int max_depth = 12)
    {
        pct_trajgen_params prm = limits;
        prm.margin = margin;
        generateTrajectories(path, radius, times, orders, m, scales, K, start, end, prm, out);
        certificates.clear();
        if (K == 0) return -1;
        certifyTrajectories(out.batch(), certificates, max_depth);
        int64_t best = -1;
        for (int64_t k = 0; k < K; k++) {
            if (out.results[(size_t)k].status != PCT_GEN_OK || certificates[(size_t)k].status != PCT_CERT_FREE) continue;
            if (best < 0 || out.results[(size_t)k].duration < out.results[(size_t)best].duration) best = k;
        }
        return best;
    }

    // Route -> polytopes -> trajectory -> proof: the m edges of waypoints ((m + 1) x 3) get their free-space polyhedra
    // (segmentPolyhedra with `reach` and `margin`), one candidate per time scale is generated inside them (the edge midpoints as
    // start iterates) and all are certified against this map.  The polytopes' planes already carry `margin`, so the generator runs
    // with params.margin = 0: it is not taken off twice.  Returns -1 before anything is solved when an edge collides (an empty row of
    // segmentPolyhedra: no polytope contains that edge) or a row holds more than pct_trajgen_max_planes() planes; otherwise the index
    // of the shortest-duration candidate that is PCT_GEN_OK and PCT_CERT_FREE, or -1 when there is none.
    int64_t generateSafeTrajectoryInPolyhedra(const double *waypoints, int32_t m, double reach, const double *times, const int32_t *orders,
                                              const double *scales, int64_t K, const double start[9], const double end[9],
                                              const pct_trajgen_params &limits, double margin, GeneratedTrajectories &out,
                                              std::vector<pct_traj_certificate> &certificates, int max_depth = 12)
    {
        if (m < 1 || !waypoints) throw std::runtime_error("generateSafeTrajectoryInPolyhedra: bad arguments");
        std::vector<double> segments(6 * (size_t)m), planes;
        for (int32_t s = 0; s < m; s++)
            for (int d = 0; d < 6; d++) segments[6 * (size_t)s + d] = waypoints[3 * s + d];
        std::vector<int64_t> offsets;
        segmentPolyhedra(segments, reach, margin, offsets, planes);
        certificates.clear();
        out.results.clear();
        for (int32_t s = 0; s < m; s++) {
            const int64_t cnt = offsets[(size_t)s + 1] - offsets[(size_t)s];
            if (cnt == 0 || cnt > pct_trajgen_max_planes()) return -1;
        }
        pct_trajgen_params prm = limits;
        prm.margin = 0.0;
        generateTrajectoriesInPolyhedra(waypoints, planes.data(), offsets.data(), times, orders, m, scales, K, start, end, prm, out);
        if (K == 0) return -1;
        certifyTrajectories(out.batch(), certificates, max_depth);
        int64_t best = -1;
        for (int64_t k = 0; k < K; k++) {
            if (out.results[(size_t)k].status != PCT_GEN_OK || certificates[(size_t)k].status != PCT_CERT_FREE) continue;
            if (best < 0 || out.results[(size_t)k].duration < out.results[(size_t)best].duration) best = k;
        }
        return best;
    }

    // SURVEY 3.3 (config C5's build extension): the same threshold test on the raw control points of the committed trajectory
    // (control point j of segment i = poly_coeff[i][d*(n+1)+j] * T_i, the point traj_optimizer.cpp:624-648 keeps inside sphere i)
    bool checkControlPoints(const double *poly_coeff, int64_t row_stride, const double *seg_time, const int32_t *orders,
                            int32_t segment_num, double t_now, int64_t *first_hit_point = nullptr, int64_t *points = nullptr)
    {
        pct_bezier_traj tr{ poly_coeff, row_stride, seg_time, orders, segment_num };
        int64_t fh = -1, nc = 0;
        check(pct_ctrl_points_check(cloud_, &tr, &prm_, t_now, &fh, &nc, 0, nullptr, nullptr, nullptr, nullptr), "pct_ctrl_points_check");
        if (first_hit_point) *first_hit_point = fh;
        if (points) *points = nc;
        return fh >= 0;
    }

    // raw batched NN for other consumers (status_inspector.cpp:33-46 collision test, camera_sensor.cpp:133-145 crop)
    void nearest(const float *queries, int64_t n, uint32_t *index, double *d2)
    {
        check(pct_nn_batch(cloud_, queries, n, index, d2), "pct_nn_batch");
    }
    // the k > 1 form of the same call (kdtreeForMap.nearestKSearch(p, k, ..), corridor_finder.cpp:130): index / d2 are n x k row-major,
    // each row nearest first, ties in ascending index, padded with PCT_NO_INDEX / +inf beyond the cloud's size; 1 <= k <= PCT_KNN_MAX_K.
    // Index-accelerated on every indexed map: the cell index, or -- after enableRollingIndex -- the rolling-map bucket table
    void nearestKSearch(const float *queries, int64_t n, int k, uint32_t *index, double *d2)
    {
        check(pct_knn_batch(cloud_, queries, n, (int32_t)k, index, d2), "pct_knn_batch");
    }
    // PCL's radiusSearch(p, r, indices, sqr_distances) for n queries at once (cone_keeper.cpp:120-126 asks it once per marked point):
    // row i of the result = index / d2 entries [offsets[i], offsets[i + 1]), offsets has n + 1 entries.  sorted: nearest first, ties in
    // ascending index (what PCL returns with sorted results); otherwise ascending index.  Not to be confused with radiusSearch(const
    // double[3]) above, the planner's sphere inflation, which keeps its name.  On a rolling map (enableRollingIndex) the rows come
    // from the buckets of each ball's bounding box, not from a scan of the window.
    void radiusSearchBatch(const float *queries, const float *radii, int64_t n, std::vector<int64_t> &offsets, std::vector<uint32_t> &index,
                           std::vector<double> &d2, bool sorted = true)
    {
        offsets.assign((size_t)n + 1, 0);
        int64_t total = 0;
        check(pct_radius_search_batch(cloud_, PCT_ALGO_AUTO, queries, radii, n, sorted ? PCT_ORDER_DISTANCE : PCT_ORDER_INDEX, offsets.data(), &total),
              "pct_radius_search_batch");
        index.resize((size_t)total);
        d2.resize((size_t)total);
        check(pct_radius_search_read(cloud_, 0, total, index.data(), d2.data()), "pct_radius_search_read");
    }
    std::vector<uint32_t> radiusIndices(const float center[3], float radius)
    {
        std::vector<uint32_t> out((size_t)std::max<int64_t>(pct_cloud_size(cloud_), 1));
        int64_t n = 0;
        check(pct_radius_indices(cloud_, center, radius, out.data(), (int64_t)out.size(), &n), "pct_radius_indices");
        out.resize((size_t)n);
        return out;
    }

    // lidar sensor (camera_sensor.cpp:133-145): the points within max_dist of the sensor become this frame's observed map
    void cropTo(const double center[3], double radius, ObstacleMap &observed)
    {
        check(pct_cloud_crop_to(cloud_, center, radius, observed.cloud_), "pct_cloud_crop_to");
        observed.cloud_empty_ = pct_cloud_size(observed.cloud_) == 0;
        if (!observed.cloud_empty_) check(pct_cloud_build_grid(observed.cloud_, 0.0f), "pct_cloud_build_grid");
    }
    // supervisor (status_inspector.cpp:33-46): nearestKSearch(point, 1) and sqrt(d2) < col_rad
    bool collides(const double p[3], double col_rad)
    {
        if (cloud_empty_) return false;
        const float q[3] = { (float)p[0], (float)p[1], (float)p[2] };       // pcl::PointXYZ(cmd.position.x, ...)
        uint32_t idx;
        double d2;
        check(pct_nn_batch(cloud_, q, 1, &idx, &d2), "pct_nn_batch");
        return std::sqrt(d2) < col_rad;
    }

    int64_t size() const { return pct_cloud_size(cloud_); }
    bool empty() const { return cloud_empty_; }
    pct_cloud *handle() { return cloud_; }
    const pct_inflate_params &params() const { return prm_; }

private:
    static void check(int status, const char *what)
    {
        if (status != PCT_OK && status != PCT_ERR_EMPTY)
            throw std::runtime_error(std::string(what) + ": " + pct_last_error());
    }
    void needRolling(const char *what) const
    {
        if (!rolling_) throw std::runtime_error(std::string(what) + ": the map has no rolling index (enableRollingIndex)");
    }
    int64_t removeBall(const double centre[3], double r, int outside)
    {
        needRolling(outside ? "forgetOutside" : "clearBall");
        int64_t removed = 0;
        check(pct_cloud_ring_remove_ball(cloud_, centre, r, outside, &removed), "pct_cloud_ring_remove_ball");
        cloud_empty_ = pct_cloud_size(cloud_) == 0;
        return removed;
    }
    pct_cloud *cloud_ = nullptr;
    int64_t capacity_ = 0;
    bool cloud_empty_ = true;
    bool rolling_ = false;
    double dedup_res_ = 0.0;
    double compact_fraction_ = 0.0;
    double safety_margin_ = 0.0;
    pct_inflate_params prm_{ { 0, 0, 0 }, 0.0, 0.0, 0.0 };
};

}  // namespace pct
