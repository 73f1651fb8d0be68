/*
 * pct_engine.h -- C ABI of the MI355X obstacle-cloud engine (libpct_engine.so).
 *
 * This is the batched extension SURVEY.md section 8(b) specifies next to the kd_* functions
 * (include/kdtree/kdtree.h): an opaque cloud handle in HBM plus batch queries that replace
 * the per-point PCL/FLANN calls on the planner's hot path.  Plain pointers and sizes only;
 * int status codes; no exceptions cross the boundary; host buffers are caller-owned.
 *
 * Reference interface each entry point replaces (paths relative to /root/reference/):
 *   pct_cloud_upload_*      safeRegionRrtStar::setInput           Planner/src/corridor_finder.cpp:93-99
 *                           (rcvPointCloudCallBack                Planner/src/sim_planning_demo.cpp:159-167)
 *   pct_nn_batch            kdtreeForMap.nearestKSearch(p,1,..)   Planner/src/corridor_finder.cpp:130
 *                           with kd_nearestf arithmetic           Utils/kdtree/src/kdtree.c:345-491
 *   pct_knn_batch           the same nearestKSearch(p, k, ..) for k > 1 (PCL's k-NN interface, called with k = 1 at :130)
 *   pct_radius_count_batch  kd_nearest_rangef + kd_res_size       Utils/kdtree/src/kdtree.c:262-293,561-593,620-623
 *   pct_radius_search_batch kdtree.radiusSearch(p, r, idx, dist) per marked point  Planner/src/cone_keeper.cpp:92-153
 *   pct_inflate_batch       safeRegionRrtStar::radiusSearch       Planner/src/corridor_finder.cpp:113-133
 *                           (+ checkRadius :656-659, checkTrajPtCol :412-416), batched over the loops at
 *                           :829-835 (SafeRegionEvaluate) and :958-974 (treeRepair)
 *   pct_bezier_check        checkSafeTrajectory/getPosFromBezier  Planner/src/sim_planning_demo.cpp:715-781
 *   pct_bezier_check_batch  the same check for a set of candidate trajectories over one map in one call (the loop a caller of
 *                           checkSafeTrajectory would write around its candidates; variants as in Planner/src/traj_postprocessing.cpp)
 *   pct_bezier_certify_batch  the same question answered for every point of the curves, not for samples of them (no reference
 *                           counterpart: checkSafeTrajectory only samples)
 *   pct_bezier_clearance_batch  how close each whole curve comes to the cloud, as a bracket (no reference counterpart)
 *   pct_cloud_ring_index +  the per-frame rebuild of the search tree: rcvPointCloudCallBack -> setInput
 *   pct_cloud_append_aos    Planner/src/sim_planning_demo.cpp:159-167 -> Planner/src/corridor_finder.cpp:93-99 (rolling map, config C5)
 *   pct_ctrl_points_check   the containment the optimizer enforces on the control points, Planner/src/traj_optimizer.cpp:624-648,
 *                           as the threshold test of checkTrajPtCol (corridor_finder.cpp:412-416) on control point * T_i
 *   pct_plan_create_replan  one replan tick's query side in one captured graph: SafeRegionEvaluate's re-check loop
 *   pct_plan_replan_run     corridor_finder.cpp:829-835 + checkSafeTrajectory sim_planning_demo.cpp:729-781 + the control points
 *   pct_*_dev               the same batches on device buffers and the caller's stream (multi-GPU: include/pct_shard.h)
 *
 * Arithmetic contract (what "parity" means): coordinates are fp32 in HBM; every distance is
 * computed in fp64 from the float-widened operands as ((dx*dx + dy*dy) + dz*dz) with one
 * rounding per operation and no fused multiply-add -- bit-identical to kdtree.c:379-382.
 * Nearest neighbour: the minimum of that value; among fp64-equal minima the LOWEST index
 * wins (the reference's winner on exact ties depends on tree shape).  Radius count:
 * d2 <= (double)r * (double)r, inclusive (kdtree.c:273).
 *
 * Domain: ANY finite fp32 cloud and query, on every path.  The fp64 value above is finite for every pair of finite floats (at most
 * ~1.4e78), so magnitudes decide nothing but speed: where the fp32 screening of a kernel overflows (separations beyond
 * sqrt(FLT_MAX) = 1.8447e19) or underflows, the pairs concerned are decided in fp64 (parity section).
 *
 * Non-finite input (tests/test_numeric_edges.py, tests/test_gpu_numeric_edges.py) follows from the same comparisons, a NaN or
 * infinite d2 being neither < +inf nor <= a finite r*r:
 *   - a query with a NaN or infinite coordinate: status PCT_OK, idx = PCT_NO_INDEX, d2 = +inf, count 0 (under r*r = +inf: the
 *     number of points whose d2 is +inf rather than NaN -- every finite point when the query holds no NaN); the other queries of
 *     the batch are answered as without it.
 *     Planner points (fp64) are narrowed to fp32 first, so |p| > FLT_MAX is such a query; pct_inflate_batch applies the
 *     reference's early-out to it before any search (|p - start| = +inf > sample_range + max_radius: radius = max_radius -
 *     search_margin; a NaN compares false there and yields radius = max_radius).
 *   - a radius: r enters only as r*r -- a negative r counts as |r|, r = +/-inf counts every point at a finite d2, NaN counts none.
 *   - a cloud row with a NaN or infinite coordinate is never a nearest neighbour and is counted only under r*r = +inf (and no NaN):
 *     the brute-force paths (PCT_ALGO_STREAM, PCT_ALGO_STREAM_EXACT) and a rolling-map index created with an extent accept such
 *     rows; pct_cloud_build_grid, and pct_cloud_ring_index without an extent on a cloud that already holds such a row, need the
 *     data's bounding box and return PCT_ERR_INVALID ("cloud holds non-finite coordinates"), leaving the cloud as it was, without
 *     an index.
 *
 * k nearest neighbours (pct_knn_batch*, 1 <= k <= PCT_KNN_MAX_K): row i of idx / d2 (row-major Q x k) holds the k smallest points of
 * query i in the total order of the nearest-neighbour contract -- smaller fp64 d2 first, among equal d2 the lower index first -- and
 * lists them in that order.  Every d2 is the arithmetic above, bit-identical to what pct_nn_batch reports for the same pair; idx is
 * index_base + local index (the ring slot on a rolling map); k = 1 equals pct_nn_batch on every path.  Slots beyond the number of
 * points at a finite d2 hold PCT_NO_INDEX / +inf: the tail of a row when k exceeds the cloud's size; the whole row of a query with a
 * NaN or infinite coordinate (the other rows of the batch are as without it); and the place of cloud rows with a NaN or infinite
 * coordinate on the paths that accept them (above), which are never listed.  k < 1 or k > PCT_KNN_MAX_K: PCT_ERR_INVALID.  Q = 0:
 * PCT_OK.  Empty cloud: every slot padded; the host forms return PCT_ERR_EMPTY, pct_knn_batch_dev PCT_OK, as for pct_nn_batch*.
 * On a rolling map PCT_ALGO_RING (and PCT_ALGO_AUTO, which takes it there) walks the rolling-map index: the expanding cube of buckets
 * around the query until the list holds k entries and no unseen bucket can hold a closer point -- same rows, bit for bit, as the
 * exhaustive PCT_ALGO_STREAM over the window.
 *
 * Radius search with lists (pct_radius_search_batch*): PCL's radiusSearch(p, r, indices, sqr_distances) for a batch, the sibling of
 * pct_knn_batch.  The result is a CSR: row i = entries [offsets[i], offsets[i + 1]), offsets has Q + 1 entries, offsets[0] = 0 and
 * offsets[Q] is the total.  Row i lists exactly the points pct_radius_count_batch counts for (q_i, r_i) -- the same fp64 test
 * ((dx*dx + dy*dy) + dz*dz) <= (double)r * (double)r, inclusive, and the same non-finite rules: a negative r counts as |r|, a NaN r
 * gives an empty row, r = +/-inf lists every point whose d2 is not NaN, a query with a NaN coordinate gives an empty row, and the
 * other rows of the batch are unaffected -- so offsets[i + 1] - offsets[i] equals that count on every path.  idx is index_base +
 * local index (the ring slot on a rolling map); d2 is bit-identical to what pct_nn_batch / pct_knn_batch report for the same pair.
 * Order: PCT_ORDER_INDEX lists each row in ascending index (the order of pct_radius_indices, and of the reference's kd_nearest_range
 * result once sorted); PCT_ORDER_DISTANCE lists nearest first, among equal d2 the lower index first (the engine's total order: that
 * of pct_knn_batch and of pct_radius_crop(sort_by_distance)).  Both are deterministic: two runs give identical bytes.
 * Algorithms: PCT_ALGO_GRID uses the cell index and returns PCT_ERR_INVALID without one; PCT_ALGO_RING uses the rolling-map index
 * (the buckets of the ball's bounding box, each read once, and the overflow queue) and returns PCT_ERR_INVALID on a cloud without
 * pct_cloud_ring_index; PCT_ALGO_STREAM is exhaustive, for any cloud (PCT_ALGO_STREAM_EXACT is accepted as STREAM); PCT_ALGO_AUTO
 * takes the rolling-map index on a rolling map, the grid when one is built and the streaming form otherwise -- under
 * PCT_ALGO_STREAM, and on a small host-mapped cloud under any algo, the answer is therefore exact but NOT index-accelerated: every
 * query examines every point of the window.  pct_radius_count_batch* dispatches the same way.  An unknown algo, or an order other
 * than 0 / 1: PCT_ERR_INVALID.  Host form: the lists stay in a cloud-owned device buffer of 12 B per entry, grown on demand; offsets and total
 * are copied out and pct_radius_search_read then copies any range of the lists, so a caller sizes its buffers from total without a
 * second search.  A result lasts until the next radius search (either form), upload, append, grid build or drop, or destroy on that
 * cloud: a read after any of those, a read before any search, or a range outside [0, total] returns PCT_ERR_INVALID; n = 0 is
 * PCT_OK.  Q = 0: PCT_OK, offsets[0] = 0, total = 0.  Empty cloud: PCT_OK with every row empty (as the count and
 * pct_radius_indices).  More than 2^32 - 1 entries: PCT_ERR_CAPACITY.  If the list buffer cannot be allocated: PCT_ERR_ALLOC with
 * offsets / total still valid.  Device form: d_offsets[Q + 1] is always written; the lists are written only when
 * d_offsets[Q] <= cap -- the kernels test this on the device and leave d_idx / d_d2 untouched otherwise, the caller reads
 * d_offsets[Q] to find out.  There is no max_nn: a bounded list is pct_knn_batch cut at r*r.
 *
 * Batched Bezier check (pct_bezier_check_batch*): pct_bezier_check for B candidate trajectories against one cloud -- the same corridor
 * under several time allocations, evasive variants, a fan of motion primitives, the committed trajectories of several vehicles.  Both
 * forms share one contract, identical on a plain, cell-indexed, rolling-map or small host-mapped cloud.  The batch is packed (struct
 * pct_bezier_batch): the segments of all trajectories one after another, trajectory b = segments [seg_offsets[b], seg_offsets[b+1]).
 * Trajectory b is evaluated exactly as pct_bezier_check(c, traj_b, p, t_start[b], stop_time, dt, .., cap, ..) evaluates it: the same
 * segment search with its strict `>`, the same sequential fp64 additions t += dt and t_accu += dt, the same Bernstein arithmetic, the
 * same inflation.  Its verdict (struct pct_traj_verdict): nsamples is the UNCLIPPED count, the number of samples the reference's loops
 * would evaluate; the evaluated samples are the first m_b = min(nsamples_b, cap, 4096), and first_hit, min_radius and min_sample cover
 * exactly those: first_hit is the first of them with radius < 0 (-1 = none), min_radius the smallest radius among them (folded with <
 * in ascending sample order; +inf when nothing was evaluated) and min_sample the LOWEST sample index that attains it (-1 when nothing
 * was evaluated) -- what ranks the collision-free candidates by clearance.  A radius is never NaN for finite parameters.  Sample lists,
 * a CSR like the radius search's: offsets[b] = sum of m_a over a < b, offsets has B + 1 entries and offsets[B] is the total; row b of
 * pos / radius / d2 / idx is entries [offsets[b], offsets[b+1]), each bit-identical to what pct_bezier_check writes for that sample --
 * PCT_NO_INDEX / +inf / max_radius - search_margin included where the early-out fired or the cloud is empty.  The lists are written
 * only when offsets[B] <= list_cap; otherwise nothing is written into them, and nothing behind offsets[B] is ever touched: the caller
 * compares offsets[B] with list_cap.  Host form: the verdicts are always complete; the library sizes its own workspaces and waits
 * once on the host for the total; offsets == NULL means no lists are wanted; an empty cloud gives PCT_OK with the early-out radius
 * everywhere (first_hit = -1, min_sample = 0); on a rolling map an append in flight is finished first and the overflow-queue overrun
 * paragraph below applies as to the other host forms.  Device form: asynchronous on `stream`, no host synchronisation and no allocation
 * inside, ordered after the cloud's mutations like the other *_dev forms; the struct is read on the host, its pointers are device
 * memory; the caller reserves first (pct_cloud_reserve_queries(c, list_cap); list_cap must not exceed the reserved size) and the
 * lists may all be NULL; d_offsets[B + 1] and every nsamples are always written, and when d_offsets[B] > list_cap the other verdict
 * fields are set to -2, -2, NaN ("not evaluated").  PCT_ERR_INVALID, before any launch and with nothing written: a NULL required
 * pointer, B < 0, cap <= 0, dt not > 0, and in the host form seg_offsets not starting at 0 or not strictly ascending, an order outside
 * 0..12, a row_stride below 3 * (order + 1).  B == 0: PCT_OK, and the only thing written is offsets[0] = 0 when offsets were given.
 * The enumeration always ends on the device: the host form returns PCT_ERR_INVALID for a trajectory whose
 * min(stop_time, sum of its seg_time) / dt is not <= 2^20 (a batch is for candidate sets, not for logs); the device form, which
 * cannot see the data, bounds each trajectory's loop at 2^20 samples (plus one per segment), and a trajectory that reaches the bound,
 * has an order outside 0..12 or a row too short for it, or whose segment range is empty, descending or outside [0, seg_offsets[B]]
 * reports nsamples = -1, contributes no sample and has none of its rows read.
 *
 * Rolling-map index and the overflow-queue overrun: the append kernels flag a queue that would overrun (ring.hpp: cannot happen by the
 * queue's sizing; a point is then missing from the table although it is in the window).  The host forms of the calls that search the
 * table look at the flag after their wait, file the window again and ask once more; the device forms (*_dev) return before their
 * kernels have run and cannot repair -- the next host-form call or append on the cloud does.
 *
 * De-duplicating appends (pct_cloud_ring_dedup): a rolling map that holds a window of UNIQUE voxels.  key(p) is pct_voxel.h's voxel
 * coordinate per axis, (int) round((double) p / res), fp64 division, half away from zero; a point is keyless if a coordinate is
 * non-finite or a voxel coordinate falls outside [-2^20, 2^20) -- a keyless point is always kept and matches nothing, so one NaN
 * never rejects a frame.  An append of the frame F[0..n) onto a window with cap, count, next (n <= cap, judged on the offered n):
 * the doomed slots are (next + j) mod cap for j < n, those below count -- what a plain append of all n points would overwrite; the
 * holders are the keys of the keyed points in the other slots below count; F[i] is kept iff it is keyless, or its key is no holder
 * and no earlier point of the frame has it (first occurrence wins, as in voxel_map).  The n' kept points, in frame order and with
 * their coordinates unchanged, are appended exactly as pct_cloud_append_aos appends a frame made of them; n' = 0 changes nothing.
 * Invariant: after an append, the key of every keyed point of that frame is present in the window (only doomed slots are evicted,
 * and a point is dropped only for an earlier point of the frame or a holder outside the doomed slots -- asking the whole window
 * would drop a re-sensed obstacle for a holder the same append evicts).  Copies: a key gains a second copy only when all its
 * holders lie among the n oldest slots; no bound is promised (frames of half the window: up to 3 seen).  Host wait: such an append
 * waits once on the host for the survivor count n' (a host-mapped word, polled) before it can queue the unchanged eviction and
 * insert launches; those stay asynchronous as for any copied frame, their source being a device buffer the library owns.
 * Uploads (pct_cloud_upload_*) are not filtered.  Captured plans are unaffected by such appends.
 *
 * Removing points (pct_cloud_ring_remove_ball / _box / _indices): on a rolling-map cloud -- one with a live pct_cloud_ring_index -- a
 * removal turns chosen slots below pct_cloud_size into REMOVED slots: the slot's three coordinates read back as NaN and its record
 * is retired from the bucket table or the overflow queue.  From then on the cloud is observably the cloud that an upload of the same
 * rows, with NaN in those rows, would have produced (the NaN-row equivalence), on every path and every algorithm: nearest neighbour,
 * k-NN, radius counts (r = +/-inf included), radius lists, crop, inflation, the Bezier check, the control-point check,
 * pct_rrt_expand_batch, the replan plan and the de-dup holders (a removed row is keyless and holds no voxel: the next append that
 * offers its voxel keeps the point).  Nothing else changes: every other point keeps its index (ring slot + index_base);
 * pct_cloud_size, the capacity and the ring cursor are unchanged; a later append overwrites a removed slot like any other (evicting
 * it touches nothing); appends do not prefer removed slots.  A row that already holds a NaN coordinate -- removed, or the caller's
 * own -- is left alone and not counted: *removed counts the rows this call changed.  Ball: inside <=> ((dx*dx + dy*dy) + dz*dz) <=
 * r*r with dx = (double)x - centre[0] and so on, fp64 without contraction -- exactly the rows pct_radius_indices_q64(centre, r)
 * lists; a negative r counts as |r|, a NaN r puts nothing inside.  Box: inside <=> lo[k] <= (double)p[k] <= hi[k] on all three
 * axes.  A row with an infinite coordinate and no NaN is outside every finite region.  outside == 0 removes the rows inside the
 * region, outside != 0 those outside it ("forget").  The empty-window rule: a removal that changes a row and leaves no row without
 * a NaN coordinate makes the cloud empty -- size 0, cursor at slot 0, tables cleared, the index still configured, the de-dup mode
 * kept -- so the reference's empty-cloud rule applies again (radius = max_radius - search_margin, corridor_finder.cpp:115-116).
 * All forms are host forms ordered on the library's stream: an append still in flight is finished first and the removal sees its
 * frame; each waits once on the host for {removed, live after} (a host-mapped word, polled).  Captured plans stay valid across
 * removals, the reset included.  Records now die out of arrival order: dead records behind a live bucket head take bucket room
 * until the head passes them (a bucket that looks full spills newcomers to the overflow queue: correct, slower); nothing is
 * compacted by a removal itself (see the next paragraph).  A table sized automatically ignores removed rows when it is sized again.
 *
 * Compacting the window (pct_cloud_ring_compact, pct_cloud_ring_autocompact, pct_cloud_ring_compact_count): removed slots stay below
 * pct_cloud_size and the cursor overwrites live and dead slots alike, so every removal lowers the effective capacity of a window that
 * has filled; a compaction gives the room back.  Live: a row is live iff it is below size and has no NaN coordinate -- exactly what
 * pct_cloud_ring_live counts; a caller's own NaN rows are dropped like removed ones, rows with +/-inf and no NaN are live and stay.
 * Order: the L live rows move to slots 0 .. L-1 in arrival order, oldest first; arrival order is slot order starting at `start`,
 * start = the ring cursor when size == capacity (the ring has wrapped) and 0 otherwise; the compaction is stable in that order.
 * After the call size = L and the cursor stands at L mod capacity: the next append fills the free slots L .. without evicting
 * anything, and once the window is full again the ring evicts in the same oldest-first order as before; the bucket table is filed
 * again from the compacted rows, no dead record remains, the overflow queue holds only genuine spills, and the removed-rows mark of
 * the window is cleared.  Equivalence: after the call the cloud is observably the rolling-map cloud that an append of those L rows,
 * in that order, into an empty window of the same configuration (cell size, table shape, bucket records, de-dup mode and res, index
 * base) would have produced.  Every search and check gives the same distances as before the call; indices are the new ones
 * (index_base + new slot), ties go to the lowest NEW index.  *live = L and *reclaimed = old size - L; either may be NULL.  remap may
 * be NULL; otherwise it is host memory with remap_cap >= old size, and for an old slot i remap[i] = index_base + new slot, or
 * PCT_NO_INDEX for a row that was dropped.  PCT_ERR_INVALID, with nothing changed: a NULL cloud, a cloud without a rolling-map
 * index, a remap shorter than the window.  L == old size: nothing moves, not even a wrapped ring's rotation; remap is the identity
 * and *reclaimed = 0.  An empty cloud: PCT_OK, zeros.  L == 0 (possible only with a caller's own NaN rows) follows the empty-window
 * rule of the paragraph above.  An append still in flight is finished first, as every removal does.  Captured plans stay valid: no
 * pointer, table shape or workspace changes (the rows are scattered into a scratch buffer and copied back, the coordinate arrays
 * keep their addresses) and the generation is not bumped.  The call waits once on the host for L (a host-mapped word, polled) and
 * once more only when remap is asked for.  pct_cloud_ring_autocompact(f): f == 0 turns the mode off (the default: nothing anywhere
 * behaves differently); 0 < f <= 1 turns it on: a removal entry point (pct_cloud_ring_remove_ball / _box / _indices,
 * pct_cloud_ring_carve_depth) whose own wait reports size − live >= f × capacity and live > 0 compacts before it returns, on the exact counts that wait delivered (no host-side guess, no further wait); *removed
 * of that call is unchanged.  With the mode on, "every other point keeps its index" holds only between compactions:
 * pct_cloud_ring_compact_count is the number of compactions that moved rows (0 < L < old size) since the cloud was created, and a
 * caller who holds indices compares it before and after a call.  f < 0, f > 1 or non-finite, or f > 0 on a cloud without
 * pct_cloud_ring_index: PCT_ERR_INVALID; pct_cloud_ring_drop turns the mode off, as it does de-dup.
 *
 * Removing outliers (pct_cloud_ring_remove_outliers, pct_cloud_ring_neighbour_counts): the radius rule on the window itself -- a
 * judged row stays iff at least min_neighbours OTHER rows of the window lie within r of it -- judged in place, no row crosses the bus.
 * Neighbour: row j is a neighbour of row i iff j != i as ring slots, both rows are below pct_cloud_size and hold no NaN, and
 * ((dx*dx + dy*dy) + dz*dz) <= r*r in fp64 on the float-widened rows, one rounding per operation, no contraction: the inclusive test
 * of the radius count (a row exactly r away is a neighbour).  Exclusion is by slot, not by distance: a coincident copy in another
 * slot is a neighbour.  A row with +/-inf and no NaN is live; for the finite r this call takes it has no neighbour and is nobody's
 * neighbour, because every d2 that involves it is inf or NaN (an r*r that overflows is held at DBL_MAX).  Judged rows: the `newest` most recent rows in arrival order -- with
 * n = size and start = (n == capacity ? cursor : 0), arrival position p lives in slot (start + p) mod capacity, the order of the
 * paragraph above; positions p >= n - newest are judged, newest <= 0 or newest >= n judges every row; neighbours are always sought in
 * the whole window; rows that hold a NaN are not judged.  newest = the kept count of the append just made
 * (pct_cloud_ring_dedup_last, pct_cloud_append_depth) is the per-frame filter.  One judgement, then one removal: every judged row is
 * counted on the window as it is when the call begins, then every judged row with fewer than min_neighbours neighbours is removed --
 * the result does not depend on thread order, and it is not the fixed point of repeated removal (three points 0.4 apart on a line,
 * r = 0.5, min_neighbours = 2: the two ends go and the middle stays; a second call removes the middle).  The call is a removal in
 * every sense of the paragraph "Removing points": it needs a live rolling-map index, finishes an append in flight first, satisfies
 * the NaN-row equivalence on every path, *removed counts the rows this call changed (may be NULL), the empty-window rule and the
 * auto-compaction rule (pct_cloud_ring_autocompact, on the counts this call's wait delivered) apply, captured plans stay valid, the
 * de-dup holders forget the removed voxels, and there is one host wait, the removal's own.  r must be finite and >= 0 and
 * min_neighbours >= 0, else PCT_ERR_INVALID with nothing changed; min_neighbours == 0 removes nothing and launches nothing; an empty
 * cloud returns PCT_OK with zero.  pct_cloud_ring_neighbour_counts is the same judgement without the removal: counts[slot], for
 * slot < size, is min(neighbours, count_cap) for a judged row and PCT_NO_INDEX for a row that holds a NaN or is out of scope; n
 * (the entries of counts, host memory) must be >= size and count_cap >= 1, else PCT_ERR_INVALID; it changes nothing in the cloud.
 * Cost: a row reads the buckets of the (2 ceil(r / cell) + 3)^3 cells its ball can touch until min_neighbours (count_cap) neighbours
 * are found -- its own bucket first -- so the cost grows with (r / cell)^3 and, for the rows that are removed, is always the whole
 * box: an r of many cells is not what this call is for.
 *
 * Statistical outliers (pct_cloud_ring_remove_statistical, pct_cloud_ring_remove_isolated, pct_cloud_ring_knn_mean_distances,
 * pct_cloud_ring_knn_distance_stats): PCL's StatisticalOutlierRemoval on the window itself -- a judged row is measured by the mean
 * distance to its k nearest OTHER rows of the window and removed when that mean is greater than a threshold -- in place, no row crosses
 * the bus.  All arithmetic is fp64 on the float-widened rows, one rounding per operation, no contraction; sqrt and / are correctly
 * rounded.  Window, judged rows and scope are those of the paragraph above: `newest` selects the most recent rows in arrival order,
 * position p lives in slot (start + p) mod capacity, newest <= 0 or newest >= size judges every row, rows that hold a NaN are not
 * judged, and neighbours are always sought in the whole window, on the window as it is when the call begins.  Candidates of row i:
 * every row j != i (as ring slots) below the size that holds no NaN and has a finite d2 = ((dx*dx + dy*dy) + dz*dz); exclusion is by
 * slot, so a coincident copy in another slot is a neighbour at distance 0.  The k nearest are the k best candidates in the engine's
 * total order (d2, then slot), the order of pct_knn_batch; 1 <= k <= PCT_KNN_MAX_K.  Mean distance: s = 0; for e = 0 .. k-1 in that
 * order (nearest first): s = s + sqrt(d2[e]); mean = s / (double)k.  A judged row is MEASURED iff it has at least k candidates; a row
 * with an infinite coordinate never has k candidates, because every d2 that involves it is inf or NaN; an unmeasured judged row has
 * mean = +inf; an unjudged slot reports NaN.  Statistics over the measured judged rows: v[slot] is the mean of a measured judged row
 * and +0.0 for every other slot below the size.  tree_sum(v), the tree order: pad with +0.0 to a multiple of 256, view as rows of 256
 * consecutive slots, fold each row by halves -- for h = 128, 64, ..., 1: a[i] = a[i] + a[i + h] for i < h -- the row's value is a[0];
 * repeat the same procedure on the array of row values until one value is left.  sum = tree_sum(v); sum_sq = tree_sum(v * v), the
 * product rounded once; N = the number of measured judged rows.  N >= 1: mean = sum / N; var = (sum_sq - (sum * sum) / N) / (N - 1)
 * for N >= 2, a var that is not greater than 0 counts as 0, and var = 0 for N = 1; stddev = sqrt(var); threshold = mean + stddev_mult *
 * stddev.  N = 0: mean = stddev = NaN and threshold = +inf.  This is PCL's rule -- sample variance, strict compare -- except that the
 * means stay fp64 and the sums have a stated order, so the result is a function of the window alone.  One removal rule for both
 * calls: a judged row is removed iff mean > threshold, a strict compare; an unmeasured row (+inf) is therefore removed under every
 * finite threshold and never under +inf.  pct_cloud_ring_remove_statistical derives the threshold from its own scope;
 * pct_cloud_ring_remove_isolated takes it as max_mean_distance -- the per-frame call: with de-dup on, the rows a later frame keeps are
 * almost only its outliers, whose own statistics would condemn nothing, so the threshold comes from an occasional whole-window
 * statistical call.  One judgement, then one removal: the result does not depend on thread order, and it is not the fixed point of
 * repeated calls.  Both are removals in every sense of the paragraph "Removing points": they need a live rolling-map index, finish an
 * append in flight first, removed rows become NaN rows, *removed may be NULL, the empty-window rule and the auto-compaction rule
 * apply, captured plans stay valid, the de-dup holders forget the removed voxels, and there is one host wait, the removal's own: the
 * threshold stays on the device between the reduction and the removal, and the statistics (*stats, may be NULL) come back with that
 * wait.  k outside 1 .. PCT_KNN_MAX_K, a stddev_mult that is not finite, a max_mean_distance that is NaN or < 0 (+inf is allowed and
 * removes nothing): PCT_ERR_INVALID with nothing changed.  pct_cloud_ring_knn_mean_distances (mean[slot] for slot < size, host
 * memory of n >= size entries) and pct_cloud_ring_knn_distance_stats are the judgement and the statistics without the removal: they
 * change nothing in the cloud; n < size or a NULL output: PCT_ERR_INVALID.  An empty cloud returns PCT_OK with zeros and the N = 0
 * statistics.  Cost: a whole-window judgement is a whole-window k-NN; a row walks the expanding cube of cells until its list is full
 * and the cube's faces are farther than entry k - 1.
 *
 * Depth images (pct_cloud_ring_carve_depth, pct_cloud_append_depth, pct_depth_classify): the consumer side of the reference's rgbd and
 * camera modes -- img_pcl_map_observer::save_point back-projects a rendered depth image to the observed cloud (map_observer.cpp:92-100),
 * safety_controller::check_image_for_point decides whether a point lies in observed free space (safety_controller.cpp:102-130).  One
 * projection serves all three calls (struct pct_depth_view below); all arithmetic is fp64 from float-widened operands, one rounding
 * per operation, no contraction, in the order written here.  Projection of a point p (an fp32 row): d = (double)p - t;
 * c_k = (d0*R[0][k] + d1*R[1][k]) + d2*R[2][k] for the camera axes k = x, y, z (R[i][k] = R[3*i + k]).  The point is IN THE IMAGE iff
 * c_z >= near_z (a NaN fails) and, with scale = focal / c_z * width (the same scale on both axes, as in the reference),
 * u = c_x*scale + width/2.0, v = c_y*scale + height/2.0, ru = round(u), rv = round(v), half away from zero,
 * 0 <= ru <= width - 1 and 0 <= rv <= height - 1 -- compared in fp64 before any conversion to int.  Its pixel value is
 * val = (double)image[rv*width + ru].  The point is SEEN THROUGH by the image iff it is in the image, val is finite (a +inf pixel proves
 * nothing: nothing was rendered there, as in the reference; NaN and -inf likewise) and, with w = val - margin: c_z < w (PCT_DEPTH_Z), or
 * w > 0 && ((d0*d0 + d1*d1) + d2*d2) < w*w (PCT_DEPTH_RANGE: no square root, so the test stays exact).  The comparison is strict: a
 * point at exactly val - margin stays.  Un-projection of pixel (x, y) holding dep, PCT_DEPTH_Z only: the pixel is valid iff dep is
 * finite, dep >= near_z and dep <= max_depth; a = ((double)x/width - 0.5)/focal, b = ((double)y - 0.5*height)/width/focal,
 * p_k = t[k] + dep*((a*R[k][0] + b*R[k][1]) + R[k][2]), narrowed to fp32 with round-to-nearest; valid pixels are emitted in row-major
 * order.  (Un-projecting a range image would need a normalisation whose rounding this contract would have to pin: PCT_ERR_INVALID.)
 * pct_cloud_ring_carve_depth removes every point the image sees through and is a removal in every sense of the paragraph above: it
 * needs a live rolling-map index, finishes an append in flight first, makes one pass over the slots below pct_cloud_size and waits
 * once on the host for {removed, live after}; rows that hold a NaN are left alone and not counted; removed rows become NaN rows
 * whose records are retired, so the NaN-row equivalence holds on every path, the empty-window rule applies and captured plans stay
 * valid.  pct_cloud_append_depth un-projects the image on the device, compacts the valid pixels in row-major order into a device
 * buffer the library owns and appends that frame exactly as pct_cloud_append_aos appends the same points (through the de-dup filter
 * when de-dup is on; pct_cloud_ring_dedup_last reports it like any other append): no point list crosses the bus; the call waits
 * once on the host for the number of valid pixels and, with de-dup on, once more for the survivor count.  pct_depth_classify needs no
 * cloud: each planner point (fp64) is narrowed to fp32 first, as every planner point is; seen_by[i] is the lowest view whose image
 * sees point i through, or -1; pixel[2i], pixel[2i + 1] are (ru, rv) of the point in the LAST view, or -1, -1 when it is not in that
 * image (the reference's `good` flag).  Order of operations and the margin: carve first, then append the same image.  The points an
 * image appends project back onto their own pixel at a z-depth within fp32 narrowing of the pixel value (numpy restatement, 40 random
 * poses with |t| <= 100 m, fov 40 to 120 degrees, 8 x 6 and 64 x 48 images, depths in [0.1, 30]: every point on its own pixel,
 * |c_z - val| <= 6.1e-6), so with margin = 0 the next carve by the same image could remove some of them; with a small positive margin
 * (1e-3 on that domain) it cannot.  Sensor simulation -- rendering a world into an image -- is not part of the library.
 *
 * Range images (pct_cloud_ring_carve_range, pct_cloud_append_range, pct_range_classify): the organised scan of a spinning or
 * solid-state lidar -- rings by columns, a range per beam (the reference's camera/sensor_type = lidar) -- as the map's input, beside
 * the depth images above and with the same three calls.  One projection serves all three (struct pct_range_view below); all
 * arithmetic is fp64 from float-widened operands, one rounding per operation, no contraction, in the order written here; / and sqrt
 * are correctly rounded.  The library calls no sin, cos or atan2: angles reach it only as tables the caller made.  Pseudo-angle:
 * pa(x, y) is a monotone stand-in for atan2(y, x) on [0, 2 pi), exported as pct_range_pseudo_angle (a host function with no HIP call
 * in it) so that callers build col_edge from their calibration with the arithmetic the device uses: den = |x| + |y|; if den is 0 or
 * not finite the result is NaN; p = y / den; if x < 0, pa = 2.0 - p; otherwise, if y < 0, pa = 4.0 + p; otherwise pa = p.  The range
 * is [0, 4): 0 = +x, 1 = +y, 2 = -x, 3 = -y.  Projection of a cloud row p (fp32): d = (double)p - t; r2 = (d0*d0 + d1*d1) + d2*d2;
 * s_k = (d0*R[0][k] + d1*R[1][k]) + d2*R[2][k] for the sensor axes k = 0, 1, 2 (R[i][k] = R[3*i + k]); h = sqrt(s0*s0 + s1*s1),
 * a = pa(s0, s1), q = s2 / h.  The point is IN THE IMAGE iff r2 >= near_range*near_range and r2 < +inf; h > 0;
 * col_edge[0] <= a < col_edge[width]; row_edge[0] <= q < row_edge[height] -- a NaN fails every one of them.  Its pixel is (r, c):
 * c = (number of col_edge entries <= a) - 1, r = (number of row_edge entries <= q) - 1; a value equal to an edge belongs to the cell
 * above it.  The search is a plain binary search; its result is defined by these counts, not by the search.  The point is SEEN THROUGH
 * iff it is in the image, val = (double)image[r*width + c] is finite (a +inf pixel proves nothing: no return; -inf and NaN likewise,
 * as for depth images) and, with w = val - margin: w > 0 && r2 < w*w -- strict, no square root, the PCT_DEPTH_RANGE test: a point at
 * exactly val - margin stays.  Un-projection of pixel (r, c) holding rho: the pixel is valid iff rho is finite, rho >= near_range and
 * rho <= max_range; e0 = row_dir[r][0]*col_dir[c][0], e1 = row_dir[r][0]*col_dir[c][1], e2 = row_dir[r][1];
 * p_k = t[k] + rho*((e0*R[k][0] + e1*R[k][1]) + e2*R[k][2]), narrowed to fp32 with round-to-nearest; valid pixels are emitted in
 * row-major order.  Conventions: a scan that does not cover the whole circle chooses its sensor frame so that azimuth 0 (the +x axis)
 * is not inside its span, for example x along the first column's lower edge; R and both direction tables are the caller's, in one
 * frame.  A full-circle scan has col_edge[0] = 0 and col_edge[width] = 4.  Columns ascend in azimuth: a sensor that spins the other
 * way hands over a mirrored R, or reorders its columns.  Per-pixel azimuth offsets (staggered beams) are out of scope: such a driver
 * appends points, and may still carve with the nominal tables and a larger margin.  The three calls mean, word for word, what the
 * depth calls they stand beside mean: pct_cloud_ring_carve_range is a removal in every sense of the paragraph "Removing points" (a
 * live rolling-map index, an append in flight finished first, one pass over the slots below pct_cloud_size, one host wait for
 * {removed, live after}; NaN rows left alone and not counted; removed rows become NaN rows whose records are retired, so the NaN-row
 * equivalence holds on every path, the empty-window rule applies and captured plans stay valid); pct_cloud_append_range is
 * pct_cloud_append_aos of the un-projected frame, through the de-dup filter when it is on, with the same host waits and
 * PCT_ERR_CAPACITY; pct_range_classify narrows planner points to fp32, reports the lowest view that sees the point through and the
 * pixel in the LAST view as pixel[2i] = c, pixel[2i + 1] = r (-1, -1 when the point is not in that image).  The tables are host memory,
 * copied per call, the caller's again when the call returns.  Order of operations and the margin: carve first, then append the same
 * image.  The points a scan appends project back onto their own pixel at a range within fp32 narrowing of the pixel value (numpy
 * restatement, 40 random poses with |t| <= 100 m, ranges in [0.3, 60], widths 8 to 2048, heights 1 to 128, full-circle and partial
 * spans, uniform and non-uniform rings, every cell at least 1e-3 rad wide: every point on its own pixel, |range - val| <= 5.7e-6),
 * so with margin = 0 the next carve by the same scan could remove some of them; with a small positive margin (1e-3 on that domain) it
 * cannot.  A cell much narrower than 1e-3 rad can lose its own point to a neighbour at short range: fp32 narrowing moves a point at
 * 0.3 m from a sensor 100 m from the origin by up to 2.2e-5 rad.  Rendering a world into a scan is not part of the library.
 *
 * Segment queries (pct_segment_nn_batch*, pct_segment_inflate_batch): the nearest obstacle point to a LINE SEGMENT, for the questions a
 * planner asks between two points -- is the straight line to the goal free with the margin, how wide is the free tube around this
 * edge, can the sphere chain be shortcut -- without sampling the line.  A segment is two planner points a, b (fp64 xyz), each
 * narrowed to fp32 first, as every planner point is, then widened again; a row p is an fp32 cloud row, widened.  All arithmetic is
 * fp64, one rounding per operation, no contraction, in exactly this order:  e_k = b_k - a_k;  L2 = (e0*e0 + e1*e1) + e2*e2;
 * w_k = p_k - a_k;  dot = (w0*e0 + w1*e1) + w2*e2;  s = (L2 == 0) ? 0 : dot / L2;  if (!(s > 0)) s = 0; else if (s > 1) s = 1 (a NaN
 * becomes 0);  c_k = w_k - s*e_k (one product, one difference);  d2 = (c0*c0 + c1*c1) + c2*c2.  `/` and sqrt are correctly rounded, as
 * for the statistical outliers above.  A segment with a == b therefore gives exactly the d2 of the nearest-neighbour searches.
 * Candidates: a row is a candidate iff it is below the size, its d2 is finite and d2 <= reach*reach -- inclusive; an r*r that
 * overflows is held at DBL_MAX; reach = +inf means every finite d2.  The winner is the best candidate in the engine's order: d2, then
 * index, the lowest index on ties.  Rows that hold a NaN never win (removed rows and the caller's own NaN rows), nor do rows with an
 * infinite coordinate, whose d2 is not finite.  Outputs per segment: idx = index_base + slot of the winner, or PCT_NO_INDEX when there
 * is no candidate; d2 = the winner's d2, or +inf; s = the winner's parameter on the segment (0 at a, 1 at b), or NaN.  "No candidate"
 * is also the answer for a segment with a non-finite endpoint (judged after the narrowing), a NaN reach and a negative reach.
 * An empty cloud fills the "no candidate" outputs and the host form returns PCT_ERR_EMPTY (the device form PCT_OK), as for
 * pct_nn_batch*; Q == 0: PCT_OK; a NULL required pointer or Q < 0: PCT_ERR_INVALID with nothing written.  d2 and s may be NULL in
 * every form, idx in the inflate form.  algo: PCT_ALGO_STREAM works on any cloud, brute force over the window with every pair in
 * fp64; PCT_ALGO_RING walks the rolling-map index (the overflow queue, then the buckets of the cells the capsule (segment, reach) can
 * touch) and needs a live one, PCT_ERR_INVALID otherwise; PCT_ALGO_AUTO takes the ring form on a cloud with a live index and the
 * streaming form otherwise; PCT_ALGO_GRID and PCT_ALGO_STREAM_EXACT are PCT_ERR_INVALID for this call (there is no grid form and only
 * one streaming form), as is an unknown algo.  Both forms give the same answers, bit for bit.  Host forms: an append in flight is
 * finished first, they wait once on the host, and the overflow-queue overrun paragraph above applies as to the other host forms.
 * Device form: asynchronous on `stream`, no host wait and no allocation inside, ordered after the cloud's mutations like the other
 * *_dev forms; reserve the batch size first (pct_cloud_reserve_queries).  Capsule inflation (pct_segment_inflate_batch): with d2* the
 * smallest finite d2 over all rows of the window, or +inf when there is none, radius = min(sqrt(d2*) - search_margin, max_radius),
 * "min" as pct_inflate_batch writes it (rr < max_radius ? rr : max_radius); radius < 0 means the segment collides, exactly as for
 * checkTrajPtCol.  idx and s are the winner's when sqrt(d2*) - search_margin < max_radius, PCT_NO_INDEX and NaN otherwise.  An empty
 * cloud (size 0) follows the engine's empty-cloud rule: radius = max_radius - search_margin, PCT_OK.  The start-distance early-out of
 * pct_inflate_batch is NOT applied -- a segment has no single distance to the start -- so start and sample_range are not read.  The
 * walk is bounded by a reach derived from max_radius + search_margin that provably never changes this result (the rounding argument
 * stands beside the code); the contract is the unbounded formula.
 *
 * Segment sweeps (pct_segment_sweep_batch*): the first contact of a sphere of radius r that moves along a line segment from a to b --
 * how far can the planner go before it touches something, and which point stops it.  The point that stops the sphere is in general
 * not the point nearest to the segment.  A sweep is a segment a -> b (fp64 xyz, narrowed to fp32 and widened again exactly as for
 * "Segment queries") and a radius r.  All arithmetic is fp64 on float-widened operands, one rounding per operation, no contraction, `/`
 * and sqrt correctly rounded.  e, L2, w, dot, s and d2 are those of "Segment queries".  r2 = min(r*r, DBL_MAX).  A row is a BLOCKER iff
 * d2 <= r2 -- inclusive; this is the candidate test of pct_segment_nn_batch under reach = r, so "blocked" here is exactly "has a
 * candidate" there.  The entry parameter t of a blocker, in exactly this order:  ww = (w0*w0 + w1*w1) + w2*w2;  if (ww <= r2) t = 0
 * (the sphere is in contact at the start; this covers a == b);  otherwise  g = ww - r2;  disc = dot*dot - L2*g;
 * if (!(disc > 0)) disc = 0;  t = (dot - sqrt(disc)) / L2;  if (!(t > 0)) t = 0; else if (t > s) t = s (s: the blocker's own clamped
 * closest-approach parameter; geometrically the entry never lies behind the closest approach, the clamp is what rounding can ask for).
 * The winner is the blocker with the smallest t, the lowest index on ties.  Outputs per sweep: idx = index_base + slot of the winner
 * and its t.  With no blocker: idx = PCT_NO_INDEX and t = 1 -- the whole segment can be flown.  An invalid sweep -- a non-finite endpoint
 * (judged after the narrowing), a NaN or a negative radius -- gives idx = PCT_NO_INDEX and t = NaN, never "free".  Rows that hold a NaN
 * and rows with an infinite coordinate never block.  t may be NULL.  An empty cloud fills the free / invalid outputs and the host form
 * returns PCT_ERR_EMPTY (the device form PCT_OK); Q == 0: PCT_OK; a NULL required pointer or Q < 0: PCT_ERR_INVALID with nothing
 * written.  algo is PCT_ALGO_AUTO, PCT_ALGO_STREAM or PCT_ALGO_RING, chosen as for "Segment queries"; PCT_ALGO_GRID,
 * PCT_ALGO_STREAM_EXACT and an unknown algo are PCT_ERR_INVALID, as is PCT_ALGO_RING without a live index.  Both forms give the same
 * answers, bit for bit: the streaming form measures every row; the rolling-map form reads the overflow queue, then the capsule's cells
 * in layers along the segment from a's side, and stops once no unseen row can beat the contact it holds (the argument stands beside
 * the code).  The host form finishes an append in flight first and waits once; the device form is asynchronous on `stream`, allocates
 * nothing and waits for nothing (reserve the batch size first, pct_cloud_reserve_queries).
 *
 * Capsule search (pct_segment_count_batch*, pct_segment_search_batch*, pct_segment_search_read): how many rows of the window lie within
 * reach of a line segment, and which -- what pct_radius_count_batch / pct_radius_search_batch answer for a point, for an edge: the
 * points around a corridor edge or a straight-line shortcut, without sampling the segment into balls.  Row i of the answer holds
 * every row of the window that is a CANDIDATE of segment i under reach[i] in the sense of "Segment queries": the ends are narrowed to
 * fp32 and widened, d2 is that paragraph's arithmetic, and a row is listed iff d2 <= min(reach*reach, DBL_MAX), inclusive.  A
 * non-finite end (judged after the narrowing), a NaN reach or a negative reach gives an empty row; rows that hold a NaN (removed rows
 * of a rolling map among them) and rows with an infinite coordinate are never listed.  A segment with a == b gives exactly the row of
 * pct_radius_search_batch for the fp32 point a, d2 bit for bit, whenever reach*reach taken in fp64 equals the square of the fp32
 * radius.  The result is the radius search's CSR: offsets has Q + 1 entries, offsets[0] = 0, offsets[Q] is the total, and the counts
 * of pct_segment_count_batch are offsets[i + 1] - offsets[i] on every path.  Each entry carries idx = index_base + local index (the
 * ring slot on a rolling map), the fp64 d2, and optionally s, the parameter of the closest point on the segment (0 at a, 1 at b) --
 * never NaN for an entry; s is recomputed after the sort from the segment and the row the index names, of which it is a function.
 * Order: PCT_ORDER_INDEX or PCT_ORDER_DISTANCE (d2, then index) as for the radius search; both are deterministic.  algo:
 * PCT_ALGO_STREAM measures every row of the window, on any cloud; PCT_ALGO_GRID walks the cell index -- the cells of the capsule's
 * bounding box, without those whose centre is farther than reach + h from the segment (the argument stands beside the code) -- and
 * answers PCT_ERR_INVALID "without a grid" on a cloud that has none, a rolling map included; PCT_ALGO_RING walks the rolling-map index
 * as pct_segment_nn_batch does and needs a live one, PCT_ERR_INVALID otherwise; PCT_ALGO_AUTO takes the rolling-map index when it is
 * live, else the grid when one is built, else the streaming form; PCT_ALGO_STREAM_EXACT and an unknown algo are PCT_ERR_INVALID, as
 * is an order other than 0 / 1.  All forms give the same bytes.  Host forms: an append in flight is finished first; the lists stay in
 * cloud-owned device buffers of their own (20 B per entry, grown on demand -- not those of the radius search, whose last result stays
 * readable), pct_segment_search_read copies any range of them (idx, d2 or s may be NULL), and a result lasts until the next host-form
 * capsule search, a device-form one that borrows the buffer for its sort keys, an upload, append, grid build or drop, or destroy: a
 * read after any of those, before any search, or of a range outside [0, total] is PCT_ERR_INVALID; n = 0 is PCT_OK.  Q == 0: PCT_OK,
 * offsets[0] = 0, total = 0.  An empty cloud gives all-zero counts and offsets; the host forms then return PCT_ERR_EMPTY, the device
 * forms PCT_OK.  A NULL required pointer, Q < 0 or cap < 0: PCT_ERR_INVALID with nothing written.  More than 2^32 - 1 entries:
 * PCT_ERR_CAPACITY.  Device forms: asynchronous on `stream`, no host wait; the workspaces are those of pct_cloud_reserve_queries
 * (reserve the batch size first; the scan's share of them is set up by the first search after a reserve).  d_offsets[Q + 1] is always
 * written; the lists are written only when d_offsets[Q] <= cap -- tested on the device, d_idx / d_d2 / d_s stay untouched otherwise.
 * d_d2 and d_s may be NULL; with PCT_ORDER_DISTANCE and d_d2 == NULL the sort keys live in the cloud's own capsule-search list buffer,
 * grown to cap entries by the call.  pct_last_work reports the records read and the cells / buckets opened by the count and the
 * fill together (the streaming form: Q x size, known on the host).
 *
 * Free-space polyhedra (pct_segment_polyhedron_batch, pct_segment_polyhedron_read, pct_segment_supports_dev): a convex free region
 * around each segment, as half-spaces -- the step from "these points lie near this edge" to "this polyhedron around the edge is
 * free", for a corridor handed to a QP or SOCP solver.  For segment i with reach[i], take row i of "Capsule search" in
 * PCT_ORDER_DISTANCE: its entries ordered by d2, then index; every term is that paragraph's.  Walk the row in that order: an entry is
 * a SUPPORT iff no earlier support of the same row cuts it.  The cut test is fp64 on float-widened operands, one rounding per
 * operation, no contraction, in exactly this order.  For a support with row p, s and d2 are those of "Segment queries" and
 * n_k = w_k - s*e_k, that paragraph's c_k.  For a later entry with row x:  u_k = x_k - p_k;  h = (n0*u0 + n1*u1) + n2*u2.  The
 * support cuts the entry iff h >= 0 -- inclusive.  Nothing can overflow (products of differences of finite floats) and nothing can
 * be NaN.  Hence: the first entry of a non-empty row is always a support; a second copy of a support's point is cut (u = 0, h = 0);
 * a row with d2 == 0 -- a point ON the segment -- has n = 0 and cuts everything behind it: its plane is the empty half-space and the
 * caller reads "the segment collides" from d2.  The plane of a support:  d = sqrt(d2);  nh_k = n_k / d;  off = (nh0*p0 + nh1*p1) +
 * nh2*p2;  the half-space is {y : nh.y <= off};  for d2 == 0 the plane is (0, 0, 0, -1).  `/` and sqrt are correctly rounded, as
 * elsewhere in this header.  Guarantees, in real arithmetic (rounding moves a plane by a few ulp of the coordinates, no more):
 * (1) the segment lies in every half-space, strictly when d2 > 0 -- n = p - c with c the closest point of a convex set, so
 * n.(y - c) <= 0 for every y on the segment; (2) no row of the window within reach of the segment lies in the interior of the
 * intersection -- every candidate is a support, and lies on its own plane, or is cut by one; (3) nothing is claimed outside the
 * capsule (segment, reach): a caller who wants a bounded polytope intersects with a region inside that capsule, as
 * ObstacleMap::segmentPolyhedra does.  The robot's size is not part of the call: shrinking by a margin m is off - m per plane, the
 * caller's step; the cut test uses the unshifted planes, which is what makes the shrunk region m-clear of every cut point.  Each
 * entry of the result carries idx = index_base + local index (the ring slot on a rolling map), d2, s and the plane nh0 nh1 nh2 off;
 * the result is a CSR like the capsule search's, offsets[Q + 1] with offsets[0] = 0 and offsets[Q] the total, supports in row order
 * (nearest first).  Invalid segments give empty rows exactly as in the capsule search (a non-finite end, a NaN or negative reach);
 * rows that hold a NaN, removed rows and rows with an infinite coordinate never appear.  Host form: the capsule search's count,
 * scan, fill and distance sort on the path `algo` selects exactly as there (PCT_ALGO_AUTO, _STREAM, _GRID, _RING; anything the
 * capsule search refuses is PCT_ERR_INVALID), then the filter, a count of supports per row, a scan and a compaction -- all forms
 * give the same bytes.  An append in flight is finished first, an overflow-queue overrun is asked twice, and the host is read
 * twice: the candidate total, which sizes the lists, and the support offsets.  The candidate rows live in cloud-owned buffers of
 * their own (12 B per entry): the call does NOT borrow the capsule search's list buffer, and pct_segment_search_read still reads
 * the last capsule search after it.  The supports stay in cloud-owned buffers too (52 B per support);
 * pct_segment_polyhedron_read copies any range of them (idx, d2, s or plane may be NULL); a result lasts until the next
 * pct_segment_polyhedron_batch, an upload, append, grid build or drop, or destroy: a read after any of those, before any call, or
 * of a range outside [0, total] is PCT_ERR_INVALID; n = 0 is PCT_OK.  An empty cloud gives all-zero offsets; the host form then
 * returns PCT_ERR_EMPTY, the device form PCT_OK.  Q == 0: PCT_OK with offsets[0] = 0.  A NULL required pointer, Q < 0, cap < 0 or
 * row_cap < 0: PCT_ERR_INVALID with nothing written.  Device form (pct_segment_supports_dev): the filter alone, over rows the
 * caller made with pct_segment_search_batch_dev(..., PCT_ORDER_DISTANCE, ...) -- d_row_offsets[Q + 1], d_row_idx, and row_cap the
 * cap of that call; asynchronous on `stream`, no host wait.  d_offsets[Q + 1] is always written.  If d_row_offsets[Q] > row_cap the
 * rows were never written: every entry of d_offsets is then -1 and nothing else is touched.  Otherwise the lists are written only
 * when d_offsets[Q] <= cap -- tested on the device; d_d2, d_s and d_plane may be NULL.  A row index outside the cloud is never a
 * support and is never dereferenced.  The filter trusts the given order and does not re-sort.  d2, s and the plane are recomputed
 * from the segment and the row the index names, of which they are functions.  The positions of the supports inside their rows live
 * in a cloud-owned buffer of 4 B per row entry, grown to row_cap by the call (refused during graph capture, like
 * pct_cloud_reserve_queries; reserve the batch size first).  pct_polyhedron_lds_rows() is the longest row the filter keeps in LDS
 * in one piece; longer rows are served in windows of that length, with the same bytes.
 *
 * Certified Bezier check (pct_bezier_certify_batch*): whole trajectories proven free, or shown to collide, by subdivision instead of
 * sampling -- the verdict does not depend on a dt or on the speed, and the work grows with how close a curve comes to the obstacles,
 * not with its length.  A Bezier piece lies in the convex hull of its control points, hence in a capsule around its chord: if that
 * capsule holds no row of the window the whole piece is free; if an end of the piece is within the margin the curve collides there;
 * otherwise the piece is cut in half by de Casteljau and both halves are asked again.  Input: a pct_bezier_batch as the batched check
 * takes it -- t_start is NOT read: whole trajectories are certified, and a caller who wants a horizon passes the segments that cover
 * it through seg_offsets -- with margin (finite, >= 0), max_depth (0..20), piece_cap and algo.  All arithmetic is fp64, one rounding
 * per operation, no contraction, in the order given here.  (1) World control points of a segment of order n:
 * P[j][k] = polycoef[row][k*(n+1) + j] * seg_time[row], the point pct_ctrl_points_check names.  A trajectory is INVALID, with nothing
 * else examined, if any of its seg_time is not finite or not > 0, or if any |P[j][k]| is not <= FLT_MAX; an INVALID trajectory is
 * never FREE (its depth and pieces are 0, its hit fields and min_d2 those of "no hit").  (2) A piece is a control polygon P[0..n], a
 * segment number, a depth d and a position k; it stands for u in [k/2^d, (k+1)/2^d]; the first pieces are the segments themselves
 * (d = 0).  (3) Halving: level by level q[i] = (p[i] + p[i+1]) * 0.5; the left child (position 2k) takes the first point of every
 * level, the right child (2k + 1) the last point of every level, reversed.  (4) Geometry of a piece: a = (double)(float)P[0] and
 * b = (double)(float)P[n]; rho2 = the maximum over j = 0..n of the d2 of "Segment queries" for segment (a, b) with the row replaced
 * by the fp64 point P[j]; rho = sqrt(rho2); cmax = max |P[j][k]|; reach = ((margin + rho) * (1 + 2^-20)) + cmax * 2^-40.  The piece
 * is BLOCKED iff segment (a, b) has a candidate under reach in the sense of "Segment queries" -- its capsule count is non-zero.  An
 * end x of {a, b} is a HIT iff sqrt(d2) - margin < 0 with d2 the nearest-neighbour d2 of the fp32 point x: the collision test of
 * pct_bezier_check for a sample at that point, without the start-distance early-out.  (5) Rounds: in round r every live piece (all
 * of depth r) is examined.  A trajectory with a hit in this round becomes HIT and is retired; it reports the hit with the lowest
 * (segment, u), u = k/2^d for a and (k+1)/2^d for b, with the nearest point's index and d2.  Of the remaining pieces an unblocked one
 * is done; a blocked one at d == max_depth makes its trajectory UNDECIDED; the other blocked pieces split -- unless twice their number
 * exceeds piece_cap: then nothing splits in this round, every trajectory that owns one of them becomes UNDECIDED and the call's
 * "capped" flag is set.  A trajectory with no live piece left and no other verdict is FREE.  Output per trajectory: struct
 * pct_traj_certificate (48 bytes, below); without a hit the hit fields are -1, PCT_NO_INDEX, NaN and +inf; min_d2 is the smallest end
 * d2 examined (+inf when none), an upper bound on the squared clearance; depth is the deepest level examined, pieces the pieces
 * examined (a HIT trajectory counts every piece of its last round).  Output per call: optional stats[3] = {rounds that examined a
 * piece, pieces examined, capped flag}.  What FREE means: no row of the window lies within margin of ANY point of the trajectory.
 * The argument (it stands, with its roundings, beside the kernels in csrc/bezier_certify.hpp): the distance to a segment is a convex
 * function, so every point of a piece is within rho of its chord; a row within margin of the curve is therefore a candidate under
 * margin + rho; the two slack terms of reach cover the roundings of rho, of reach * reach and of d2 unconditionally, and the inherited
 * roundings of the halvings -- at most 2^-45 of the largest |world control coordinate| M0 of the segment -- whenever
 * margin + rho >= 2^-25 * M0 (30 micrometres per kilometre of coordinate) or the piece's own cmax >= M0 / 16; a margin below that on
 * a piece far nearer the origin than its curve reaches is the one case the slack does not provably cover.  The check is conservative
 * by that slack: a point one fp32 ulp outside the margin of a straight line is UNDECIDED, not FREE.  HIT means what it means for the
 * sampled check: a point of the curve (an end of a piece) whose nearest row is nearer than margin.  Paths: algo follows the capsule
 * count's rules (PCT_ALGO_AUTO, _STREAM, _GRID, _RING; anything else, GRID without a grid and RING without a live index are
 * PCT_ERR_INVALID) for the chord test; the end test goes through the nearest-neighbour path of the same index (the table, the grid,
 * the streaming kernels); all forms give the same bytes.  Empty cloud: every valid trajectory is FREE at depth 0 (pieces = its
 * segments, min_d2 = +inf), PCT_OK in both forms, as for the batched check.  PCT_ERR_INVALID with nothing written: a NULL required
 * pointer, B < 0, a margin that is not finite or < 0, max_depth outside 0..20, piece_cap below the number of segments (host form) or
 * below 1 or above 2^24, and in the host form the batched check's own refusals (seg_offsets not starting at 0 or not strictly
 * ascending, an order outside 0..12, a row_stride below 3 * (order + 1)).  B == 0: PCT_OK (stats, when given, are zeros).  Rolling
 * map: the host form finishes an append in flight first, and the overflow-queue overrun paragraph applies to it.  Host form: it reads
 * the live count once per round, sizes its launches and its piece buffers by it and stops at zero.  Device form: asynchronous on
 * `stream`, waits for nothing and can be captured on a cloud with a cell index or a live rolling-map index (under capture the
 * streaming path and an empty cloud are PCT_ERR_INVALID, like the streaming k-NN kernel: its counts rely on a memset that a replayed
 * graph was seen not to honour); the struct is read on the host, its pointers are device memory; it runs
 * max_depth + 1 rounds over piece_cap slots with device-side counts, dead slots posing queries the searches answer without a walk;
 * the caller reserves 2 * piece_cap queries first (pct_cloud_reserve_queries); the piece buffers (328 B per piece, two sets) and the
 * per-trajectory state are cloud-owned and grown by the call, which is refused during graph capture (call once with the same sizes
 * before capturing).  It cannot see the data: a trajectory whose segment range is empty, descending or outside [0, seg_offsets[B]],
 * that has an order outside 0..12 or a row too short for it is INVALID and none of its rows is read; when seg_offsets[B] exceeds
 * piece_cap nothing is examined, every sound trajectory is UNDECIDED and the capped flag is set.
 *
 * Trajectory clearance (pct_bezier_clearance_batch*): how close each curve comes to the cloud, as a bracket lo <= clearance <= hi,
 * by the subdivision of the certified check and the nearest-neighbour answers at the ends of its pieces -- no capsule search, so it
 * runs on every index that answers a nearest-neighbour batch.  Input: a pct_bezier_batch exactly as "Certified Bezier check" reads
 * it -- the world control points of its step (1), the same INVALID rule, t_start NOT read -- with tol (finite, >= 0, metres), cap
 * (> 0 or +inf: clearance beyond it is of no interest, the role max_radius plays for inflation), max_depth (0..20), piece_cap
 * (1..2^24, in the host form not below the number of segments) and algo.  All arithmetic is fp64, one rounding per operation, no
 * contraction, in the order given here.  Pieces, halving and the order of the piece buffer (trajectory, segment, k) are those of
 * steps (2) and (3) there; all live pieces of a round have the round's depth.  Geometry of a piece: a, b, rho and cmax exactly as in
 * step (4) there, and ell = sqrt((e0*e0 + e1*e1) + e2*e2) with e = b - a.  Queries: the nearest-neighbour d2 of the fp32 points a
 * and b give da = sqrt(d2_a), db = sqrt(d2_b).  The bound of a piece:
 *   L = max(0, (((da + db) - ell) * 0.5 - rho) - (((da + db) + ell + rho) * 2^-20 + cmax * 2^-40)),
 * sums left to right, max(0, t) being t where t > 0 and +0 elsewhere; L = +inf when either d2 is +inf.  A round r: (i) every live
 * piece counts into pieces and depth of its trajectory; (ii) both end d2 are folded into the trajectory's U2, the minimum over every
 * end examined so far, this round included, and the end that attains it is kept: smaller d2 wins, on equal d2 the earlier round,
 * within a round the lowest (segment, u), i.e. the lowest 2 * slot + end; (iii) after the fold is complete a piece RETIRES iff
 * L >= min(sqrt(U2), cap) - tol, and a retired piece folds its L into the trajectory's lo (a minimum).  Three other kinds of piece
 * also fold their L into lo and make the trajectory OPEN: one that does not retire at d == max_depth; one with ell == 0 and
 * rho == 0 (a single point as the searches see it: halving cannot improve it, so it never splits); and every would-be splitter of a
 * round in which twice their number exceeds piece_cap, which sets the call's capped flag as in the certified check; (iv) every other
 * piece splits.  Output per trajectory: struct pct_traj_clearance (48 bytes, below): hi = sqrt(U2); lo = min(folded L, hi); at_seg,
 * at_u (k/2^d for a, (k+1)/2^d for b) and at_idx (index_base applied) name the end that attains hi; with no end at finite distance
 * hi = lo = +inf, at_seg = -1, at_idx = PCT_NO_INDEX, at_u = NaN; INVALID: lo = hi = NaN with the same "nowhere" fields and
 * depth = pieces = 0.  Output per call: optional stats[3] = {rounds that examined a piece, pieces examined, capped flag}.  What the
 * record guarantees in every status but INVALID: no point of the curve is nearer than lo to any row of the window.  The argument
 * (it stands, with its roundings, beside the kernels in csrc/bezier_clearance.hpp): a point x of the piece is within rho of a chord
 * point a + s*e, so |x - a| <= rho + s*ell and |x - b| <= rho + (1 - s)*ell; the distance to the cloud is 1-Lipschitz, hence
 * d(x) >= max(da - s*ell, db - (1 - s)*ell) - rho >= (da + db - ell)/2 - rho; the two slack terms cover the roundings local to the
 * piece unconditionally and the inherited roundings of the halvings -- at most 2^-45 of the largest |world control coordinate| M0 of
 * the segment -- whenever da + db + ell + rho >= 2^-24 * M0 (60 micrometres per kilometre of coordinate) or the piece's own
 * cmax >= M0 / 16; below that no claim is made.  hi is the distance the sampled check would measure at that piece end: a point of
 * the curve rounded to fp32, not the clearance of the exact curve.  DONE adds lo >= min(hi, cap) - tol: hi only falls, so a piece
 * retired against an earlier, larger hi still satisfies it.  A tol below the slack, about 2 * d * 1e-6 at distance d, cannot be met
 * and ends OPEN.  Paths: algo is resolved for the nearest-neighbour batch on the cloud's index (PCT_ALGO_AUTO, _STREAM, _GRID,
 * _RING) and the refusals are the certified check's; all forms give the same bytes, and a trajectory's bytes do not depend on the
 * rest of the batch.  Empty cloud: every valid trajectory is DONE at depth 0 with lo = hi = +inf.  B == 0: PCT_OK (stats, when
 * given, are zeros).  PCT_ERR_INVALID with nothing written: the certified check's list with tol and cap in margin's place (tol not
 * finite or < 0, cap not > 0).  Rolling map: the host form finishes an append in flight first.  Host form: it reads the live count
 * once per round, sizes its launches and piece rooms by it and stops at zero.  Device form: max_depth + 1 rounds over piece_cap
 * slots with device-side counts, no host wait, capturable under the certified check's conditions; reserve 2 * piece_cap queries
 * first; the piece buffers are the certified check's (the two calls must not run concurrently on one cloud), the piece scalars
 * (32 B per piece) and the per-trajectory state are cloud-owned and grown by the call; what it cannot see is treated as there
 * (an unsound trajectory is INVALID; seg_offsets[B] above piece_cap: nothing examined, every sound trajectory OPEN, capped set).
 *
 * Windows of a trajectory (pct_bezier_certify_window_batch*, pct_bezier_clearance_window_batch*): the two calls above for the part of
 * each trajectory with time in [t0, t1] -- "is it safe from now for the next check_time seconds?" -- instead of whole curves.  The
 * whole-curve forms are unchanged and still do not read t_start.  Input: as there, plus horizon (B doubles, NULL = +inf for all);
 * batch->t_start IS read here (NULL = 0 for every trajectory).  All arithmetic is fp64, one rounding per operation, no contraction,
 * in the order given here.  (1) Window: t0 = t_start[b]; t1 = t0 + horizon[b], one addition (a horizon of +inf gives +inf).  A
 * trajectory is INVALID, with nothing examined, if t0 is not finite or < 0, or if horizon is NaN or not > 0; otherwise it is subject
 * to the INVALID rule of "Certified Bezier check" over ALL its segments, inside the window or not.  (2) Per segment: c = 0 at the
 * trajectory's first segment, cn = c + T_i, then c = cn (sequential sums).  Segment i is in the window iff t0 < cn && t1 > c; then
 * u0 = (t0 <= c) ? 0 : (t0 - c) / T_i and u1 = (t1 >= cn) ? 1 : (t1 - c) / T_i, and the segment drops out if !(u0 < u1).  The
 * comparisons come before the divisions, so a covered end is exactly 0 or 1.  (3) Restriction of the world polygon P of step (1)
 * there: if u1 < 1, cut at t = u1 and keep the left part; then, if u0 > 0, cut at t = u0 / u1 (one division) and keep the right
 * part.  A cut is level by level q[i] = w * p[i] + t * p[i+1] with w = 1 - t computed once (two products, one sum); the left part is
 * the first point of every level, the right part the last point of every level, reversed.  A segment with u0 == 0 && u1 == 1 is not
 * cut at all: its first piece is byte for byte the whole-curve form's.  (4) First pieces: slot = segment, as there; a segment outside
 * the window, or dropped in (2), is a dead slot.  Rounds, halving, geometry, hit rule, piece_cap rule, fold order, retirement and
 * statuses are exactly those of the two contracts above.  (5) Reporting: hit_seg / at_seg stay indices into the packed batch;
 * hit_u / at_u are in the segment's own parameter: with v = (k + end) / 2^d, u = (1 - v) * u0 + v * u1 -- v itself for an uncut
 * segment, u0 at v = 0, u1 at v = 1; pieces, depth, min_d2 and stats count what was examined.  (6) Empty window: t0 at or past the
 * trajectory's end has no piece: FREE (DONE for the clearance), depth = pieces = 0, min_d2 = hi = lo = +inf and the "nowhere" hit
 * fields -- the answer of the sampled check's "no sample at all".  (7) What FREE and lo prove: the statements above for the points of
 * the curve with u in [u0, u1] of every segment the window touches, u0 and u1 as computed in (2).  The restriction adds roundings to
 * the inherited error: a cut rounds three times per value and w + t misses 1 by up to 2^-54, 84 * 2^-53 * M0 over two cuts of up to
 * 12 levels, and the rounding of u0 / u1 moves the first piece by at most 24 * 2^-53 * M0 -- 108 * 2^-53 * M0 for the restriction,
 * and with the halvings' 240 * 2^-53 * M0 at most 348 * 2^-53 * M0 < 0.68 * 2^-44 * M0, no longer under 2^-45 * M0.  The slack terms
 * stay as they are (reach and L are unchanged) and cover it when the piece's own cmax >= M0 / 16, and otherwise when
 * margin + rho >= 2^-24 * M0 (60 micrometres per kilometre of coordinate; the whole-curve form asks 2^-25) -- for the clearance when
 * da + db + ell + rho >= 2^-24 * M0, the whole-curve condition.  Below that no claim is made.  The argument stands beside
 * bc_seed_window_kernel in csrc/bezier_certify.hpp.  Refusals, the empty cloud, B == 0, the capture rules, the overrun paragraph and
 * piece_cap versus seg_offsets[B] follow the whole-curve forms (piece_cap counts all segments of the batch, inside a window or not);
 * a non-NULL horizon or t_start is not read by a refused call, and nothing is written.  Host form: t_start and horizon are host
 * arrays.  Device form: device arrays; win[segment] = {u0, u1} (16 B per slot, piece_cap slots) is cloud-owned and grown by the call,
 * which is refused during graph capture (call once with the same sizes first).
 *
 * All entry points need a HIP device; there is no host fallback.
 */
#ifndef PCT_ENGINE_H
#define PCT_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pct_cloud pct_cloud;     /* opaque: an obstacle cloud resident in HBM */
typedef struct pct_plan pct_plan;       /* opaque: a hipGraph-captured fixed-shape query batch */

enum pct_status {
    PCT_OK = 0,
    PCT_ERR_NO_DEVICE = 1,   /* no HIP device / runtime failure at init */
    PCT_ERR_INVALID = 2,     /* bad argument */
    PCT_ERR_ALLOC = 3,       /* host or device allocation failed */
    PCT_ERR_HIP = 4,         /* a HIP call failed; see pct_last_error() */
    PCT_ERR_EMPTY = 5,       /* query against an empty cloud (outputs are still filled: idx=PCT_NO_INDEX, d2=+inf) */
    PCT_ERR_CAPACITY = 6,    /* more points than the cloud's capacity */
    PCT_ERR_INTERNAL = 7     /* a self-check of the library failed (e.g. a built index whose records are not a permutation of the cloud) */
};

#define PCT_NO_INDEX 0xFFFFFFFFu

enum pct_algo {
    PCT_ALGO_AUTO = 0,       /* rolling-map index when the cloud has one, grid kernel when a grid is built, streaming kernel otherwise */
    PCT_ALGO_STREAM = 1,     /* brute-force SoA streaming kernels: fp32 filter + exact fp64 recheck (no index needed) */
    PCT_ALGO_GRID = 2,       /* cell-pruned kernel (needs pct_cloud_build_grid) */
    PCT_ALGO_STREAM_EXACT = 3, /* brute force with every pair in fp64 (the filter's reference; same results) */
    PCT_ALGO_RING = 4        /* the rolling-map index (needs pct_cloud_ring_index; PCT_ERR_INVALID without a live one) */
};

enum pct_order {
    PCT_ORDER_INDEX = 0,     /* each row in ascending index */
    PCT_ORDER_DISTANCE = 1   /* each row nearest first, equal d2 in ascending index */
};

/* ---- process / device ---------------------------------------------------------------- */
int pct_init(int device);                       /* select the HIP device for this process */
const char *pct_last_error(void);               /* thread-local text of the last failure */
int pct_device_count(void);
int pct_sync(void);                             /* wait for everything queued by this library */

/* ---- cloud lifecycle ----------------------------------------------------------------- */
int pct_cloud_create(int64_t capacity, pct_cloud **out);
/* a cloud whose coordinates live in host-mapped memory: appends are plain host stores (no launch, no copy),
 * kernels read over the bus.  For small, frequently growing point sets (the RRT* node tree behind kd_*). */
int pct_cloud_create_small(int64_t capacity, pct_cloud **out);
int pct_cloud_destroy(pct_cloud *c);
int64_t pct_cloud_size(const pct_cloud *c);
int64_t pct_cloud_capacity(const pct_cloud *c);
/* index reported for local point i is base + i (multi-GPU shards; default 0) */
int pct_cloud_set_index_base(pct_cloud *c, int64_t base);

/* Replace the cloud.  `pts` is array-of-structures: x,y,z fp32 at byte offsets 0,4,8 of
 * each `stride_bytes` record (12 = packed, 16 = pcl::PointXYZ).  De-interleaved to SoA on
 * the device.  Drops any grid. */
int pct_cloud_upload_aos(pct_cloud *c, const void *pts, int64_t n, int64_t stride_bytes);
/* Same for a sensor_msgs/PointCloud2 payload: n records of point_step bytes, FLOAT32 fields at the given byte
 * offsets (msg.fields[i].offset), any order, any padding (sim_planning_demo.cpp:159-167). */
int pct_cloud_upload_fields(pct_cloud *c, const void *data, int64_t n, int64_t point_step, int64_t off_x, int64_t off_y, int64_t off_z);
/* Same, from three device arrays (already SoA, e.g. produced on the GPU). */
int pct_cloud_upload_soa_dev(pct_cloud *c, const float *d_x, const float *d_y, const float *d_z, int64_t n);
/* Rolling map: append n points, overwriting the oldest once capacity is reached (ring).
 * Index of a point = its slot in the ring.  Drops any cell-sorted grid; updates the rolling-map index in place.
 * `pts` is the caller's again when the call returns.  On a rolling-map cloud a frame of up to 4 MB is copied to a staging buffer
 * and the call returns once the launches are queued (every later call on the cloud is ordered behind them on the library's
 * stream); an error of those launches is reported by the next call on the cloud. */
int pct_cloud_append_aos(pct_cloud *c, const void *pts, int64_t n, int64_t stride_bytes);

/* Rolling-map index (config C5: the obstacle map is a sliding window fed one sensor frame at a time, where the reference
 * rebuilds its search tree per frame -- safeRegionRrtStar::setInput, Planner/src/corridor_finder.cpp:93-99 called from
 * rcvPointCloudCallBack, Planner/src/sim_planning_demo.cpp:159-167).  After this call pct_cloud_append_aos no longer drops an
 * index: it retires the points it overwrites from a world-anchored bucket table and files the new frame, in place, and
 * pct_nn_batch / pct_inflate_batch / pct_bezier_check / pct_ctrl_points_check / pct_rrt_expand_batch / the replan plan search that table (ALGO_AUTO,
 * ALGO_RING and, for these nearest-point calls, ALGO_GRID), and so do pct_knn_batch*, pct_radius_count_batch* and
 * pct_radius_search_batch* (ALGO_AUTO and ALGO_RING; ALGO_GRID is PCT_ERR_INVALID there, as on any cloud without a grid).
 * ALGO_STREAM still scans the whole window.  Results are the same as on any other cloud: exact fp64
 * distances, lowest ring slot on ties.  cell_size <= 0: chosen from the first data (about 6 points per cell at capacity);
 * extent (may be NULL): the window's size per axis, when the caller knows it (e.g. the sensing range) -- the table is then
 * allocated at once.  Memory: 512 B per bucket (32 records of 16 B), buckets = the extent / cell_size per axis plus a quarter,
 * rounded up to powers of two; a cell holding more records than a bucket has room for spills to a queue every query scans
 * exhaustively (pct_cloud_ring_info reports its length), and when that queue holds more than about 1 % of the window the buckets
 * are doubled -- 64, 128, at most 256 records, 4 KiB per bucket, the table never beyond 32 GiB -- and the window is filed again
 * (pct_cloud_ring_bucket_records).  Not available for small (host-mapped) clouds; excludes pct_cloud_build_grid. */
int pct_cloud_ring_index(pct_cloud *c, float cell_size, const float extent[3]);
int pct_cloud_ring_drop(pct_cloud *c);
int pct_cloud_has_ring_index(const pct_cloud *c);
int pct_cloud_ring_info(pct_cloud *c, int32_t dims[3], double *cell_size, int64_t *overflow_entries);
/* records per bucket of the rolling-map index: 32 to begin with; doubled (up to 256, the window filed again) when more than ~1 % of the window
 * sits in the overflow queue although the cells were sized from the window -- surfaces on a lattice finer than the cell, the same points sensed
 * frame after frame (the reference's rgbd mode, camera_sensor.cpp:160-166).  0 = no rolling-map index. */
int pct_cloud_ring_bucket_records(const pct_cloud *c);
/* res > 0: appends (pct_cloud_append_aos / pct_cloud_append_frame) on this rolling-map cloud keep only points whose voxel is new
 * to the window (the rule in the paragraph "De-duplicating appends" above); res == 0: off (default; appends exactly as before).
 * PCT_ERR_INVALID unless pct_cloud_ring_index was asked for on the cloud, or for res < 0 / non-finite.  A cell size chosen
 * automatically is at least res; an explicit cell_size < res / 2 is PCT_ERR_INVALID from whichever of pct_cloud_ring_index /
 * pct_cloud_ring_dedup comes second (a table already sized automatically with smaller cells is sized again here).
 * pct_cloud_ring_drop turns the mode off.  On a cloud whose table does not exist yet the first append applies the in-frame rule alone
 * (the window is empty) and the compacted frame sizes the table.  Each filtered append waits once on the host, see above. */
int pct_cloud_ring_dedup(pct_cloud *c, double res);
/* the last append: points offered, points kept; flags[min(offered, cap)] = 1 kept / 0 dropped (may be NULL); totals since enabled.
 * PCT_ERR_INVALID while the mode is off. */
int pct_cloud_ring_dedup_last(pct_cloud *c, int64_t *offered, int64_t *kept, uint8_t *flags, int64_t cap,
                              uint64_t *total_offered, uint64_t *total_kept);
/* Removing points from a rolling-map cloud (the paragraph "Removing points" above).  PCT_ERR_INVALID: no rolling-map index, a NULL
 * argument, a NaN in centre / lo / hi, or an index outside [index_base, index_base + size) -- the list is judged on the host first and
 * nothing is removed then.  n = 0 or an empty cloud: PCT_OK with *removed = 0.  `removed` may be NULL.
 * outside == 0: remove the points INSIDE the region; != 0: remove those OUTSIDE it ("forget") */
int pct_cloud_ring_remove_ball(pct_cloud *c, const double centre[3], double r, int outside, int64_t *removed);
int pct_cloud_ring_remove_box(pct_cloud *c, const double lo[3], const double hi[3], int outside, int64_t *removed);
/* idx: n indices as the searches report them (index_base + slot), host memory; a slot named twice counts once */
int pct_cloud_ring_remove_indices(pct_cloud *c, const uint32_t *idx, int64_t n, int64_t *removed);
/* rows below size without a NaN coordinate, and size - that (one launch, one wait) */
int pct_cloud_ring_live(pct_cloud *c, int64_t *live, int64_t *not_live);
/* Compacting the window (the paragraph "Compacting the window" above) */
int pct_cloud_ring_compact(pct_cloud *c, int64_t *live, int64_t *reclaimed, uint32_t *remap, int64_t remap_cap);
int pct_cloud_ring_autocompact(pct_cloud *c, double dead_fraction);
int pct_cloud_ring_compact_count(const pct_cloud *c, uint64_t *compactions);
/* Removing outliers (the paragraph "Removing outliers" above) */
int pct_cloud_ring_remove_outliers(pct_cloud *c, double r, int32_t min_neighbours, int64_t newest, int64_t *removed);
int pct_cloud_ring_neighbour_counts(pct_cloud *c, double r, int32_t count_cap, int64_t newest, uint32_t *counts, int64_t n);
/* Statistical outliers (the paragraph "Statistical outliers" above).  sum, sum_sq: the tree sums of the means and of their squares */
typedef struct pct_knn_stats { int64_t measured; double sum, sum_sq, mean, stddev, threshold; } pct_knn_stats;
int pct_cloud_ring_knn_mean_distances(pct_cloud *c, int32_t k, int64_t newest, double *mean, int64_t n);
int pct_cloud_ring_knn_distance_stats(pct_cloud *c, int32_t k, double stddev_mult, int64_t newest, pct_knn_stats *stats);
int pct_cloud_ring_remove_statistical(pct_cloud *c, int32_t k, double stddev_mult, int64_t newest, int64_t *removed, pct_knn_stats *stats);
int pct_cloud_ring_remove_isolated(pct_cloud *c, int32_t k, double max_mean_distance, int64_t newest, int64_t *removed);
/* Depth images (the paragraph "Depth images" above).  One pinned projection for the three calls below. */
enum pct_depth_metric { PCT_DEPTH_Z = 0, PCT_DEPTH_RANGE = 1 };
typedef struct pct_depth_view {
    double t[3];      /* camera position, world */
    double R[9];      /* row-major; column k = camera axis k in world: x image right, y image down, z optical
                         (Eigen Affine3f::rotation().col(k)); not checked for orthonormality */
    double focal;     /* focal distance in image widths, 0.5 / tan(fov_hor / 2) (map_observer::get_focal_distance) */
    double near_z;    /* a point with z-depth < near_z is not in the image (reference: 0.01) */
    int32_t width, height;
    int32_t metric;   /* what a pixel holds: depth along the optical axis (save_point) or range along the ray (check_image_for_point) */
    int32_t reserved; /* 0 */
} pct_depth_view;
/* `image`: host memory, width*height floats, row-major, the caller's again when the call returns (it is copied through a staging
 * buffer the library owns).  PCT_ERR_INVALID, with the cloud left as it was: a NULL argument; width or height < 1 or
 * width*height > 2^24; focal or near_z not finite and > 0; a NaN or infinity in t or R; a NaN margin; a NaN max_depth (+inf is
 * allowed); metric outside {0, 1}; reserved != 0; a cloud without pct_cloud_ring_index.
 * carve: removes every point the image sees through (strict; margin in the pixel's unit); *removed = rows this call changed; an
 * empty cloud: PCT_OK, *removed = 0.
 * append: metric PCT_DEPTH_Z only (PCT_DEPTH_RANGE: PCT_ERR_INVALID).  *offered = valid pixels, *kept = what the window took (equal
 * without de-dup).  More valid pixels than the capacity: PCT_ERR_CAPACITY, nothing changed. */
int pct_cloud_ring_carve_depth(pct_cloud *c, const pct_depth_view *v, const float *image, double margin, int64_t *removed);
int pct_cloud_append_depth(pct_cloud *c, const pct_depth_view *v, const float *image, double max_depth, int64_t *offered, int64_t *kept);
/* views[k] and images[k], 1 <= n_views <= 16, each view with its own size; pts: n planner points (fp64 xyz); seen_by[n];
 * pixel[2n] may be NULL.  n = 0: PCT_OK. */
int pct_depth_classify(const pct_depth_view *views, const float *const *images, int32_t n_views, const double *pts, int64_t n,
                       double margin, int32_t *seen_by, int32_t *pixel);
/* Range images (the paragraph "Range images" above).  One pinned projection for the three calls below. */
typedef struct pct_range_view {
    double t[3];            /* sensor position, world */
    double R[9];            /* row-major; column k = sensor axis k in world: x azimuth 0, y azimuth +90 deg, z up (elevation +); not checked for orthonormality */
    double near_range;      /* finite, > 0: a point or pixel nearer than this is not in the image */
    int32_t width, height;  /* columns (azimuth) x rows (rings); 1..4096 x 1..1024, width*height <= 2^24 */
    int32_t reserved[2];    /* 0 */
    const double *col_edge; /* width + 1, strictly ascending pseudo-angles in [0, 4]: column c covers [col_edge[c], col_edge[c+1]) */
    const double *row_edge; /* height + 1, strictly ascending finite values of q = z / hypot(x, y): row r covers [row_edge[r], row_edge[r+1]) */
    const double *col_dir;  /* width x 2: (cos, sin) of each column's beam azimuth; append only, may be NULL otherwise */
    const double *row_dir;  /* height x 2: (cos, sin) of each row's beam elevation; append only, may be NULL otherwise */
} pct_range_view;
/* `image`: host memory, width*height floats, row-major (row = ring), the caller's again when the call returns, as are the four tables
 * (all are copied through staging buffers the library owns).  PCT_ERR_INVALID, with the cloud left as it was: a NULL required
 * pointer; sizes outside the limits above; near_range not finite or not > 0; a non-finite t or R; reserved != 0; a NaN margin or
 * max_range (+inf is allowed); an edge table that is not finite and strictly ascending, or a col_edge entry outside [0, 4]; col_dir /
 * row_dir NULL or non-finite in pct_cloud_append_range; a cloud without pct_cloud_ring_index.
 * carve: removes every point the scan sees through (strict; margin in metres); *removed = rows this call changed; an empty cloud:
 * PCT_OK, *removed = 0.  append: *offered = valid pixels, *kept = what the window took (equal without de-dup); more valid pixels than
 * the capacity: PCT_ERR_CAPACITY, nothing changed.  classify: views[k] and images[k], 1 <= n_views <= 16, each view with its own size
 * and tables; pts: n planner points (fp64 xyz); seen_by[n]; pixel[2n] may be NULL.  n = 0: PCT_OK. */
int pct_cloud_ring_carve_range(pct_cloud *c, const pct_range_view *v, const float *image, double margin, int64_t *removed);
int pct_cloud_append_range(pct_cloud *c, const pct_range_view *v, const float *image, double max_range, int64_t *offered, int64_t *kept);
int pct_range_classify(const pct_range_view *views, const float *const *images, int32_t n_views, const double *pts, int64_t n,
                       double margin, int32_t *seen_by, int32_t *pixel);
double pct_range_pseudo_angle(double x, double y);
/* Zero-copy ingest.  pct_cloud_frame_buffer hands out a host-mapped staging buffer of at least `bytes` bytes (valid until the next
 * call that asks for a larger one, or pct_cloud_destroy); the producer -- a sensor driver, the deserialiser of a
 * sensor_msgs/PointCloud2 -- writes the frame's records there (x, y, z floats at the start of each stride-byte record) and
 * pct_cloud_append_frame appends the first n of them exactly as pct_cloud_append_aos would (rcvPointCloudCallBack,
 * sim_planning_demo.cpp:159-178), minus the host-side copy: on a rolling-map cloud the insert kernel reads the buffer over the bus. */
int pct_cloud_frame_buffer(pct_cloud *c, int64_t bytes, void **host_ptr);
int pct_cloud_append_frame(pct_cloud *c, int64_t n, int64_t stride_bytes);

/* diagnostics (tests): where ring slot `slot`'s record is filed: out = {where word, bucket of the slot's coordinates, head, tail of
 * that bucket (or of the overflow queue, bit 31 of the where word), id word stored at the filed position, overflow queue length}.
 * A removed slot's where word is 0xFFFFFFFF (no record; the other words then mean nothing). */
int pct_debug_ring_slot(pct_cloud *c, int64_t slot, uint32_t out[6]);
/* diagnostics (tests; needs no GPU): 1 when the dense PCT_ALGO_GRID NN batch kernel would address `records` cell-sorted records (the
 * cloud's points + its 16 spare ones), `cell_entries` run bounds and a batch of `queries` with 32-bit byte offsets, 0 when it keeps
 * 64-bit addresses, negative for a negative argument. */
int pct_debug_narrow_offsets(int64_t records, int64_t cell_entries, int64_t queries);
/* diagnostics (tests; needs no GPU): bins[i] = the bin the batch sort files query i (q: Q x 3 fp32) under, for a grid of dims[3] cells
 * at `origin` with cells of 1 / inv_h, bin shift `shift` (clamped to 0..4) and strips of `strip` bin rows (clamped to 1..by), computed
 * on the host by the function the sort kernels run.  *nbins = the number of bins (every bins[i] is below it), *fast = 1 when the index
 * build would choose the multiply-free form for such a grid, 0 for the generic one (both give the same bins). */
int pct_debug_query_bins(const int32_t dims[3], const float origin[3], float inv_h, int shift, int strip, const float *q, int64_t Q,
                         uint32_t *bins, uint32_t *nbins, int *fast);

/* Build / drop the uniform-cell index used by PCT_ALGO_GRID.  cell_size <= 0 picks one from
 * the bounding box and point count (about `pct` points per cell).
 * The cell has a floor: a cell_size (given or chosen) below max_ext / 1023, max_ext the longest side of the bounding box, is
 * raised to that value without notice -- in double, before the cell is rounded to float -- so the grid has at most 1024
 * cells per axis (1023 or 1024 on the longest one, as the rounding falls) and at most 2^30 cells in all.
 * pct_cloud_grid_info reports the cell actually used, not the one asked for. */
int pct_cloud_build_grid(pct_cloud *c, float cell_size);
int pct_cloud_drop_grid(pct_cloud *c);
int pct_cloud_has_grid(const pct_cloud *c);
/* grid facts for tests/bench: dims[3], cell size, origin[3], number of cells */
int pct_cloud_grid_info(const pct_cloud *c, int32_t dims[3], float *cell_size, float origin[3], int64_t *ncells);

/* ---- batch queries, host buffers, synchronous ------------------------------------------ */
/* q: Q x 3 fp32.  idx[Q] (index_base + local index), d2[Q] fp64. */
int pct_nn_batch(pct_cloud *c, const float *q, int64_t Q, uint32_t *idx, double *d2);
int pct_nn_batch_algo(pct_cloud *c, int algo, const float *q, int64_t Q, uint32_t *idx, double *d2);
/* The k nearest points of every query (contract: top of this file).  idx / d2: Q x k, row-major, each row nearest first.
 * PCT_ALGO_GRID: the cell-pruned k-NN kernel (needs pct_cloud_build_grid, PCT_ERR_INVALID otherwise); PCT_ALGO_STREAM and
 * PCT_ALGO_STREAM_EXACT: the streaming k-NN kernel, all fp64, which reads the cloud once per tile of 8 queries whatever k is;
 * PCT_ALGO_RING: the rolling-map index (needs pct_cloud_ring_index, PCT_ERR_INVALID otherwise), a block per query;
 * PCT_ALGO_AUTO: the rolling-map index on a rolling map, the cell-pruned kernel when a grid is built, otherwise the streaming
 * one -- that covers a small host-mapped cloud, where (as under PCT_ALGO_STREAM on any cloud) the answer is exact but NOT
 * index-accelerated: every query examines every point of the window. */
#define PCT_KNN_MAX_K 64
int pct_knn_batch(pct_cloud *c, const float *q, int64_t Q, int32_t k, uint32_t *idx, double *d2);
int pct_knn_batch_algo(pct_cloud *c, int algo, const float *q, int64_t Q, int32_t k, uint32_t *idx, double *d2);
/* same with fp64 query coordinates (kd_nearest's double positions); streaming kernel */
int pct_nn_batch_q64(pct_cloud *c, const double *q, int64_t Q, uint32_t *idx, double *d2);
/* the same, also reporting how many points attain the minimum: ties[i] >= 1 where counted (single queries against clouds of up
 * to 16384 points -- the RRT* node sets of the kd_* drop-in), 0 = not counted on the path taken.  ties may be NULL. */
int pct_nn_batch_q64_ties(pct_cloud *c, const double *q, int64_t Q, uint32_t *idx, double *d2, uint32_t *ties);
/* count[Q] = #points with d2 <= r*r.  algo as for pct_radius_search_batch: the rolling-map index (PCT_ALGO_RING, and PCT_ALGO_AUTO
 * on a rolling map), the grid, or the exhaustive streaming kernels */
int pct_radius_count_batch(pct_cloud *c, const float *q, const float *r, int64_t Q, uint32_t *count);
int pct_radius_count_batch_algo(pct_cloud *c, int algo, const float *q, const float *r, int64_t Q, uint32_t *count);
/* Which points lie within r, for many queries at once (contract: top of this file).
 * rows of a CSR: row i = entries [offsets[i], offsets[i+1]) ; offsets has Q + 1 entries, offsets[0] = 0, *total = offsets[Q] */
int pct_radius_search_batch(pct_cloud *c, int algo, const float *q, const float *r, int64_t Q, int order, int64_t *offsets, int64_t *total);
/* entries [first, first + n) of the lists of the LAST pct_radius_search_batch on this cloud; idx or d2 may be NULL */
int pct_radius_search_read(pct_cloud *c, int64_t first, int64_t n, uint32_t *idx, double *d2);
/* lidar-style crop (camera_sensor.cpp:133-145): indices of all points within r of ONE centre,
 * ascending index order; returns the count through *n_out.  *n_out may exceed cap: the list is then truncated to the cap LOWEST
 * indices among the hits, ascending (idx_out[0 .. cap) is a prefix of the full list), at every cloud size; cap = 0 only counts. */
int pct_radius_indices(pct_cloud *c, const float q[3], float r, uint32_t *idx_out, int64_t cap, int64_t *n_out);
int pct_radius_indices_q64(pct_cloud *c, const double q[3], double r, uint32_t *idx_out, int64_t cap, int64_t *n_out);
/* the same with the SQUARED radius given exactly (d2 <= r2): with r2 = the d2 a nearest-neighbour query returned it lists every
 * point tied at the minimum */
int pct_radius_indices_r2_q64(pct_cloud *c, const double q[3], double r2, uint32_t *idx_out, int64_t cap, int64_t *n_out);
/* The same crop with everything its consumer builds from it: idx_out[cap], d2_out[cap] (fp64, kdtree.c arithmetic) and
 * xyz_out[cap*3] (the cropped cloud = pcl::PointCloud(cloud, indices)); any of the three may be NULL.  Order: ascending
 * index, or -- sort_by_distance != 0 -- nearest first with ties in ascending index, the order pcl's radiusSearch returns
 * (PCL's own fp32 distances are parity-unpinned; cap must then hold every hit).  *n_out = number of hits. */
int pct_radius_crop(pct_cloud *c, const double q[3], double r, int sort_by_distance, int64_t cap, uint32_t *idx_out, double *d2_out,
                    float *xyz_out, int64_t *n_out);
/* dst := the points of src within r of q, in src's order, device to device (camera_sensor.cpp:398-401 known_map_pcl;
 * a lidar frame cropped out of a resident world map).  dst's cell index is dropped; rebuild it with pct_cloud_build_grid. */
int pct_cloud_crop_to(pct_cloud *src, const double q[3], double r, pct_cloud *dst);
/* K range queries against a SMALL cloud (<= 65536 points) in one launch.  ids_out[k*cap_per_query + j] in arrival order;
 * counts_out[k] >= 0: number of hits, all stored; < 0: -(number of hits), list truncated -- ask that query alone. */
int pct_radius_indices_batch_q64(pct_cloud *c, const double *q, const double *r, int64_t K, uint32_t *ids_out, int64_t cap_per_query,
                                 int64_t *counts_out);

/* ---- node sets of any dimension with fp64 coordinates (the general form of the kd_* API: kd_create(k), double positions --
 * Utils/kdtree/src/kdtree.c:112-131, 167-209).  Rows of `dim` doubles in HBM, insertion order = node number; every distance is
 * the reference's sum  s = 0; for i < dim: s += (row[i] - q[i])^2  in that order, in fp64, without contraction
 * (kdtree.c:267-272, 379-382, 420-423).  Exhaustive kernels: these sets are search trees of a planner (10^3 .. 10^6 nodes), not
 * obstacle clouds -- 3-D fp32 clouds belong in a pct_cloud. */
typedef struct pct_nodeset pct_nodeset;
int pct_nodeset_create(int dim, int64_t capacity, pct_nodeset **out);      /* 1 <= dim <= 1024; capacity grows on append */
int pct_nodeset_destroy(pct_nodeset *s);
int pct_nodeset_clear(pct_nodeset *s);
int64_t pct_nodeset_size(const pct_nodeset *s);
int pct_nodeset_dim(const pct_nodeset *s);
int pct_nodeset_append(pct_nodeset *s, const double *rows, int64_t n);     /* n rows of dim doubles, host memory */
/* nearest node of ONE query (dim doubles): idx = the LOWEST node number at the minimum distance, d2 = that distance, ties = how
 * many nodes attain it.  Empty set: idx = PCT_NO_INDEX, d2 = +inf, ties = 0. */
int pct_nodeset_nearest(pct_nodeset *s, const double *q, uint32_t *idx, double *d2, uint32_t *ties);
/* node numbers with d2 <= r2, ascending; *n_out = number of hits (may exceed cap; only cap written) */
int pct_nodeset_radius_indices_r2(pct_nodeset *s, const double *q, double r2, uint32_t *idx_out, int64_t cap, int64_t *n_out);

typedef struct pct_inflate_params {
    double start[3];        /* start_pt */
    double sample_range;    /* early-out: |p - start| > sample_range + max_radius */
    double search_margin;
    double max_radius;
} pct_inflate_params;

/* pts: Q x 3 fp64 (the planner's Vector3d).  radius[Q] as radiusSearch returns it;
 * idx/d2 (optional, may be NULL) = NN, or PCT_NO_INDEX / +inf where the early-out fired. */
int pct_inflate_batch(pct_cloud *c, const pct_inflate_params *p, const double *pts, int64_t Q,
                      double *radius, uint32_t *idx, double *d2);

/* Segment queries (contract: top of this file, "Segment queries").  seg: Q x 6 fp64, a then b; reach[Q]; idx[Q], d2[Q], s[Q] -- d2 and
 * s may be NULL.  algo: PCT_ALGO_AUTO, PCT_ALGO_STREAM or PCT_ALGO_RING; PCT_ALGO_GRID and PCT_ALGO_STREAM_EXACT: PCT_ERR_INVALID.
 * The device form (device pointers, asynchronous on `stream`) takes its workspace from pct_cloud_reserve_queries. */
int pct_segment_nn_batch(pct_cloud *c, int algo, const double *seg /* Q x 6: a then b */, const double *reach /* Q */, int64_t Q,
                         uint32_t *idx, double *d2, double *s);
int pct_segment_nn_batch_dev(pct_cloud *c, int algo, const double *d_seg, const double *d_reach, int64_t Q,
                             uint32_t *d_idx, double *d_d2, double *d_s, void *stream);
/* capsule inflation: radius[Q] = min(sqrt(d2*) - search_margin, max_radius) over the whole window, no start-distance early-out;
 * idx / s (may be NULL): the winner's where the radius is below max_radius, PCT_NO_INDEX / NaN elsewhere */
int pct_segment_inflate_batch(pct_cloud *c, const pct_inflate_params *p, const double *seg, int64_t Q,
                              double *radius, uint32_t *idx, double *s);

/* Segment sweeps (contract: top of this file, "Segment sweeps").  seg: Q x 6 fp64, a then b; radius[Q]; idx[Q] = the point that stops
 * the sphere, PCT_NO_INDEX when nothing does; t[Q] (may be NULL) = how far along a -> b its centre gets: 0 in contact at the start,
 * 1 free, NaN for an invalid sweep.  algo as for pct_segment_nn_batch. */
int pct_segment_sweep_batch(pct_cloud *c, int algo, const double *seg, const double *radius, int64_t Q, uint32_t *idx, double *t);
int pct_segment_sweep_batch_dev(pct_cloud *c, int algo, const double *d_seg, const double *d_radius, int64_t Q,
                                uint32_t *d_idx, double *d_t, void *stream);

/* Capsule search (contract: top of this file, "Capsule search").  seg: Q x 6 fp64, a then b; reach[Q].  count[Q] = the rows within
 * reach of each segment; the search returns them as a CSR (offsets[Q + 1], total) whose lists pct_segment_search_read copies out.
 * algo: PCT_ALGO_AUTO, PCT_ALGO_STREAM, PCT_ALGO_GRID or PCT_ALGO_RING.  order: PCT_ORDER_INDEX or PCT_ORDER_DISTANCE. */
int pct_segment_count_batch(pct_cloud *c, int algo, const double *seg, const double *reach, int64_t Q, uint32_t *count);
int pct_segment_count_batch_dev(pct_cloud *c, int algo, const double *d_seg, const double *d_reach, int64_t Q, uint32_t *d_count, void *stream);
int pct_segment_search_batch(pct_cloud *c, int algo, const double *seg, const double *reach, int64_t Q, int order, int64_t *offsets, int64_t *total);
/* entries [first, first + n) of the lists of the LAST pct_segment_search_batch on this cloud; idx, d2 or s may be NULL */
int pct_segment_search_read(pct_cloud *c, int64_t first, int64_t n, uint32_t *idx, double *d2, double *s);
/* device buffers, asynchronous on `stream`; d_offsets[Q + 1] always written, the lists (d_d2 / d_s may be NULL) only when
 * d_offsets[Q] <= cap.  Reserve the batch size first (pct_cloud_reserve_queries). */
int pct_segment_search_batch_dev(pct_cloud *c, int algo, const double *d_seg, const double *d_reach, int64_t Q, int order, int64_t *d_offsets,
                                 int64_t cap, uint32_t *d_idx, double *d_d2, double *d_s, void *stream);

/* Free-space polyhedra (contract: top of this file, "Free-space polyhedra").  seg: Q x 6 fp64, a then b; reach[Q].  The supports of
 * every segment's capsule row as a CSR (offsets[Q + 1], total) whose lists pct_segment_polyhedron_read copies out; algo as for
 * pct_segment_search_batch.  The capsule search's last result stays readable. */
int pct_segment_polyhedron_batch(pct_cloud *c, int algo, const double *seg, const double *reach, int64_t Q, int64_t *offsets, int64_t *total);
/* entries [first, first + n) of the LAST pct_segment_polyhedron_batch on this cloud; plane: n x 4 doubles, nh0 nh1 nh2 off; any of
 * idx, d2, s and plane may be NULL */
int pct_segment_polyhedron_read(pct_cloud *c, int64_t first, int64_t n, uint32_t *idx, double *d2, double *s, double *plane);
/* the filter alone over device rows made by pct_segment_search_batch_dev(..., PCT_ORDER_DISTANCE, ..., cap = row_cap, ...);
 * asynchronous on `stream`.  d_offsets[Q + 1] always written (all -1 when d_row_offsets[Q] > row_cap), the lists (d_d2 / d_s /
 * d_plane may be NULL) only when d_offsets[Q] <= cap.  Reserve the batch size first (pct_cloud_reserve_queries). */
int pct_segment_supports_dev(pct_cloud *c, const double *d_seg, int64_t Q, const int64_t *d_row_offsets, int64_t row_cap,
                             const uint32_t *d_row_idx, int64_t *d_offsets, int64_t cap, uint32_t *d_idx, double *d_d2, double *d_s,
                             double *d_plane, void *stream);
/* diagnostics, needs no GPU: the longest row the filter kernel keeps in LDS in one piece */
int pct_polyhedron_lds_rows(void);

/* ---- one RRT* iteration's three dependent queries in ONE launch (corridor_finder.cpp:385-410 genNewNode, :428-437
 * findNearstVertex, :464 treeRewire's neighbourhood), for K samples at once: nearest tree node of the fp32-narrowed
 * sample -> steer -> sphere inflation of the steered centre against `obstacles` -> tree nodes within 2*float(radius) of the
 * centre.  `nodes` is the small (host-mapped) cloud of node coordinates; pct_cloud_small_aux() hands out its per-node
 * planner data, 4 doubles per node {x, y, z, radius} (the node's fp64 centre and float radius, as the steer step reads
 * them), which the caller keeps current with plain stores.  ids[k*cap_per_query ...] = candidate node numbers (unordered);
 * out[k].count < 0 means -(count) hits of which only part were stored.  near_idx = -1 for an empty node set (centre = sample).
 * `obstacles` needs an index, either kind: the cell index (pct_cloud_build_grid) or the rolling-map index (pct_cloud_ring_index),
 * whose bucket table the inflation then searches -- same arithmetic, same radii.  A non-empty cloud with neither is
 * PCT_ERR_INVALID (the staged queries pct_nn_batch / pct_inflate_batch / pct_radius_* still answer on it).  An empty cloud -- a
 * rolling window nothing has been appended to, with or without its table, included -- gives every centre
 * the radius max_radius - search_margin (corridor_finder.cpp:115-116).  An append still in flight on `obstacles` is finished first and
 * the answer sees its frame; this is a host form in the sense of the overflow-queue overrun paragraph at the top of this file.
 * At most 1024 samples per call. */
typedef struct pct_expand_result { double center[3]; double radius; int32_t near_idx; int32_t count; } pct_expand_result;
int pct_cloud_small_aux(pct_cloud *nodes, double **host_aux);
int pct_rrt_expand_batch(pct_cloud *nodes, pct_cloud *obstacles, const pct_inflate_params *p, const double *samples, int64_t K,
                         int64_t cap_per_query, pct_expand_result *out, uint32_t *ids);

typedef struct pct_bezier_traj {
    const double *polycoef;   /* nseg rows of row_stride doubles: [x_0..x_n, y_0..y_n, z_0..z_n], n = orders[seg] */
    int64_t row_stride;       /* 3 * (max_order + 1) */
    const double *seg_time;   /* nseg */
    const int32_t *orders;    /* nseg, each <= 12 */
    int32_t nseg;
} pct_bezier_traj;

/* Sample the trajectory every dt from t_start over stop_time (reference loop semantics),
 * inflate every sample, report the first one with negative radius (NN distance <
 * search_margin).  first_hit = -1 when none.  Optional per-sample outputs (capacity cap):
 * pos (cap x 3 fp64), radius, d2, idx.
 * Contract, the same on every kind of cloud and whatever was called before: *nsamples is the UNCLIPPED count, the number of samples
 * the reference's loops would evaluate; *first_hit and the arrays cover the first min(nsamples, cap, 4096) samples and nothing
 * else -- a collision further on is not reported, entries behind them are not written.  No sample at all (t_start at or past the
 * end, stop_time < dt): PCT_OK, nsamples = 0, first_hit = -1.  cap <= 0, dt not > 0, nseg <= 0, an order outside 0..12 or a
 * row_stride below 3 * (order + 1): PCT_ERR_INVALID. */
int pct_bezier_check(pct_cloud *c, const pct_bezier_traj *traj, const pct_inflate_params *p,
                     double t_start, double stop_time, double dt,
                     int64_t *first_hit, int64_t *nsamples,
                     int64_t cap, double *pos, double *radius, double *d2, uint32_t *idx);

/* The same check for B trajectories in one call (contract: top of this file, "Batched Bezier check").  Host pointers in the host
 * form, device pointers in the device form. */
typedef struct pct_bezier_batch {
    const double  *polycoef;     /* total_seg rows of row_stride doubles, the trajectories one after another; row layout as pct_bezier_traj */
    int64_t        row_stride;   /* >= 3 * (largest order + 1) */
    const double  *seg_time;     /* total_seg */
    const int32_t *orders;       /* total_seg, each 0..12 */
    const int32_t *seg_offsets;  /* B + 1, seg_offsets[0] = 0, strictly ascending: trajectory b = segments [seg_offsets[b], seg_offsets[b+1]) */
    const double  *t_start;      /* B, or NULL = 0.0 for every trajectory */
    int64_t        B;
} pct_bezier_batch;

typedef struct pct_traj_verdict {   /* 32 bytes */
    int64_t nsamples;     /* the UNCLIPPED count, as pct_bezier_check reports it */
    int64_t first_hit;    /* first evaluated sample with radius < 0, -1 = none */
    int64_t min_sample;   /* LOWEST evaluated sample index that attains min_radius, -1 when nothing was evaluated */
    double  min_radius;   /* smallest radius over the evaluated samples, +inf when nothing was evaluated */
} pct_traj_verdict;

int pct_bezier_check_batch(pct_cloud *c, const pct_bezier_batch *batch, const pct_inflate_params *p, double stop_time, double dt,
                           int64_t cap, pct_traj_verdict *verdict /* B */,
                           int64_t *offsets /* B + 1, may be NULL */, int64_t list_cap,
                           double *pos, double *radius, double *d2, uint32_t *idx /* list_cap entries each (pos x3), any may be NULL */);

/* Certified Bezier check (contract: top of this file, "Certified Bezier check"): B trajectories proven free or shown to collide by
 * subdivision.  Host pointers in the host form, device pointers (the struct itself on the host) in the device form. */
enum pct_cert_status {
    PCT_CERT_FREE = 0,        /* no row of the window within margin of any point of the trajectory */
    PCT_CERT_HIT = 1,         /* an end of a piece is nearer than margin to its nearest row */
    PCT_CERT_UNDECIDED = 2,   /* a blocked piece at max_depth, or splits refused by piece_cap */
    PCT_CERT_INVALID = 3      /* a seg_time not finite or not > 0, a world control point beyond FLT_MAX (device form: an unsound range, order or row) */
};

typedef struct pct_traj_certificate {   /* 48 bytes */
    int32_t  status;      /* enum pct_cert_status */
    int32_t  depth;       /* deepest level examined */
    int32_t  hit_seg;     /* segment of the reported hit (an index into the packed batch), -1 = none */
    uint32_t hit_idx;     /* nearest point's index at the reported hit, PCT_NO_INDEX = none */
    double   hit_u;       /* parameter u of the reported hit inside hit_seg, NaN = none */
    double   hit_d2;      /* d2 of the reported hit, +inf = none */
    double   min_d2;      /* smallest end d2 examined, +inf when none: an upper bound on the squared clearance */
    int64_t  pieces;      /* pieces examined */
} pct_traj_certificate;

int pct_bezier_certify_batch(pct_cloud *c, int algo, const pct_bezier_batch *batch, double margin, int32_t max_depth, int64_t piece_cap,
                             pct_traj_certificate *cert /* B */, int64_t stats[3] /* {rounds, pieces, capped}; may be NULL */);

/* Trajectory clearance (contract: top of this file, "Trajectory clearance"): each of B trajectories gets a bracket lo <= clearance <= hi
 * of its distance to the cloud.  Host pointers in the host form, device pointers (the struct itself on the host) in the device form. */
enum pct_clearance_status {
    PCT_CLR_DONE = 0,         /* lo >= min(hi, cap) - tol */
    PCT_CLR_OPEN = 1,         /* a piece not retired at max_depth, a piece that is a single point, or splits refused by piece_cap: lo still holds */
    PCT_CLR_INVALID = 2       /* as PCT_CERT_INVALID; lo = hi = NaN */
};

typedef struct pct_traj_clearance {   /* 48 bytes */
    int32_t  status;      /* enum pct_clearance_status */
    int32_t  depth;       /* deepest level examined */
    int32_t  at_seg;      /* segment of the piece end that attains hi (an index into the packed batch), -1 = none */
    uint32_t at_idx;      /* nearest row of that end (index_base applied), PCT_NO_INDEX = none */
    double   at_u;        /* parameter u of that end inside at_seg, NaN = none */
    double   lo;          /* no point of the curve is nearer than lo to any row of the window */
    double   hi;          /* distance from that end -- a curve point rounded to fp32 -- to its nearest row; +inf = no end at finite distance */
    int64_t  pieces;      /* pieces examined */
} pct_traj_clearance;

int pct_bezier_clearance_batch(pct_cloud *c, int algo, const pct_bezier_batch *batch, double tol, double cap, int32_t max_depth, int64_t piece_cap,
                               pct_traj_clearance *out /* B */, int64_t stats[3] /* {rounds, pieces, capped}; may be NULL */);

/* The two calls above for the window [t_start[b], t_start[b] + horizon[b]] of each trajectory (contract: top of this file, "Windows of
 * a trajectory"): batch->t_start IS read (NULL = 0 for all); horizon: B doubles, NULL = +inf for all.  hit_u / at_u are in the
 * segment's own parameter. */
int pct_bezier_certify_window_batch(pct_cloud *c, int algo, const pct_bezier_batch *batch, const double *horizon /* B, or NULL */, double margin,
                                    int32_t max_depth, int64_t piece_cap, pct_traj_certificate *cert /* B */, int64_t stats[3] /* may be NULL */);
int pct_bezier_clearance_window_batch(pct_cloud *c, int algo, const pct_bezier_batch *batch, const double *horizon /* B, or NULL */, double tol,
                                      double cap, int32_t max_depth, int64_t piece_cap, pct_traj_clearance *out /* B */,
                                      int64_t stats[3] /* may be NULL */);

/* Control-point check (SURVEY.md 3.3, config C5's build extension): the threshold test of checkTrajPtCol
 * (Planner/src/corridor_finder.cpp:412-416) applied to the raw control points of the committed trajectory in world units --
 * control point j of segment i is polycoef[i][d*(n+1)+j] * seg_time[i] (layout Planner/src/traj_optimizer.cpp:739-751), the
 * point the optimizer's cone constraint keeps inside corridor sphere i (Planner/src/traj_optimizer.cpp:624-648).  Segments
 * from the one holding t_start on (the segment search of checkSafeTrajectory, sim_planning_demo.cpp:735-741), j ascending.
 * first_hit = index into that list of the first control point with radiusSearch(point) < 0, -1 when none; nctrl = its length;
 * optional per-point outputs (capacity cap): pos (cap x 3), radius, d2, idx. */
int pct_ctrl_points_check(pct_cloud *c, const pct_bezier_traj *traj, const pct_inflate_params *p, double t_start,
                          int64_t *first_hit, int64_t *nctrl, int64_t cap, double *pos, double *radius, double *d2, uint32_t *idx);

/* ---- batch queries, DEVICE buffers, asynchronous on `stream` (a hipStream_t; NULL = HIP's null
 * stream, as in any HIP call -- that is also PyTorch's default stream).  Every kernel of the batch is
 * ordered on that stream and nothing else, so work the caller queues behind it (a collective, a copy)
 * sees the results.  One batch at a time per cloud: the cloud's scratch buffers are shared, so do not
 * issue batches on the same cloud from two streams concurrently.  A rolling-map append that is still running on the library's
 * own stream (pct_cloud_append_aos returns once its launches are queued) is waited for through an event, so a batch issued right
 * after it on `stream` sees the appended frame.  algo as for the host forms, PCT_ALGO_RING included; on a rolling map the device
 * forms search the table as it is and cannot repair an overflow-queue overrun (top of this file).  For torch.distributed sharding and
 * graph capture.  An empty shard yields idx=PCT_NO_INDEX, d2=+inf and PCT_OK. ---------------------- */
int pct_nn_batch_dev(pct_cloud *c, int algo, const float *d_q, int64_t Q, uint32_t *d_idx, double *d_d2, void *stream);
int pct_radius_count_batch_dev(pct_cloud *c, int algo, const float *d_q, const float *d_r, int64_t Q, uint32_t *d_count, void *stream);
/* pct_knn_batch_algo on device buffers (d_idx / d_d2: Q x k); reserve the batch size first (pct_cloud_reserve_queries).  The streaming
 * kernel's scratch (96 MiB) is allocated by the first call that needs it. */
int pct_knn_batch_dev(pct_cloud *c, int algo, const float *d_q, int64_t Q, int32_t k, uint32_t *d_idx, double *d_d2, void *stream);
/* pct_radius_search_batch on device buffers, asynchronous on `stream`, no host synchronisation inside; d_d2 may be NULL (with
 * PCT_ORDER_DISTANCE the sort keys then live in the cloud's own list buffer, grown to cap entries by the call).  Reserve the batch
 * size first (pct_cloud_reserve_queries). */
int pct_radius_search_batch_dev(pct_cloud *c, int algo, const float *d_q, const float *d_r, int64_t Q, int order, int64_t *d_offsets,
                                int64_t cap, uint32_t *d_idx, double *d_d2, void *stream);
/* Stream variants of the planner arithmetic (same results as pct_inflate_batch / pct_bezier_check, nothing crosses the bus but the
 * trajectory's coefficients): d_pts = Q x 3 fp64 planner points on the device; d_radius[Q] required, d_idx / d_d2 optional.
 * Reserve the batch size first (pct_cloud_reserve_queries). */
int pct_inflate_batch_dev(pct_cloud *c, const pct_inflate_params *p, const double *d_pts, int64_t Q, double *d_radius, uint32_t *d_idx,
                          double *d_d2, void *stream);
/* traj's arrays are host memory (copied on the stream: keep them alive until the stream has passed the call); outputs on the device:
 * d_radius[cap] required, d_pos[3*cap] / d_d2[cap] / d_idx[cap] optional, *d_first_hit (int64, -1 = none), *d_nsamples (int32: the
 * number of samples the reference would evaluate; the first min(nsamples, cap) slots are valid).  cap <= 4096 and <= the reserved
 * batch size. */
int pct_bezier_check_dev(pct_cloud *c, const pct_bezier_traj *traj, const pct_inflate_params *p, double t_start, double stop_time, double dt,
                         int64_t cap, double *d_pos, double *d_radius, double *d_d2, uint32_t *d_idx, long long *d_first_hit, int32_t *d_nsamples,
                         void *stream);
/* pct_bezier_check_batch on device buffers ("Batched Bezier check" at the top of this file): d_batch_fields is a struct on the host
 * whose pointers are device memory; d_verdict[B] and d_offsets[B + 1] are required, the lists (list_cap entries each, d_pos x3) may
 * be NULL.  Reserve list_cap first (pct_cloud_reserve_queries). */
int pct_bezier_check_batch_dev(pct_cloud *c, const pct_bezier_batch *d_batch_fields /* struct on the host, its pointers on the device */,
                               const pct_inflate_params *p, double stop_time, double dt, int64_t cap, pct_traj_verdict *d_verdict,
                               int64_t *d_offsets /* B + 1, required */, int64_t list_cap,
                               double *d_pos, double *d_radius, double *d_d2, uint32_t *d_idx, void *stream);
/* pct_bezier_certify_batch on device buffers: d_cert[B] required, d_stats[3] may be NULL.  Reserve 2 * piece_cap queries first
 * (pct_cloud_reserve_queries).  Asynchronous on `stream`; can be captured once the piece buffers have their size. */
int pct_bezier_certify_batch_dev(pct_cloud *c, int algo, const pct_bezier_batch *d_batch_fields /* struct on the host, its pointers on the device */,
                                 double margin, int32_t max_depth, int64_t piece_cap, pct_traj_certificate *d_cert, int64_t *d_stats,
                                 void *stream);
/* pct_bezier_clearance_batch on device buffers: d_out[B] required, d_stats[3] may be NULL.  Reserve 2 * piece_cap queries first
 * (pct_cloud_reserve_queries).  Asynchronous on `stream`, no host wait; can be captured once the piece buffers have their size. */
int pct_bezier_clearance_batch_dev(pct_cloud *c, int algo, const pct_bezier_batch *d_batch_fields /* struct on the host, its pointers on the device */,
                                   double tol, double cap, int32_t max_depth, int64_t piece_cap, pct_traj_clearance *d_out, int64_t *d_stats,
                                   void *stream);
/* The window forms on device buffers ("Windows of a trajectory"): d_batch_fields->t_start and d_horizon are device arrays of B doubles
 * or NULL.  Reservation, stream and capture as for the two calls above. */
int pct_bezier_certify_window_batch_dev(pct_cloud *c, int algo, const pct_bezier_batch *d_batch_fields, const double *d_horizon, double margin,
                                        int32_t max_depth, int64_t piece_cap, pct_traj_certificate *d_cert, int64_t *d_stats, void *stream);
int pct_bezier_clearance_window_batch_dev(pct_cloud *c, int algo, const pct_bezier_batch *d_batch_fields, const double *d_horizon, double tol,
                                          double cap, int32_t max_depth, int64_t piece_cap, pct_traj_clearance *d_out, int64_t *d_stats,
                                          void *stream);
/* Exchange step of a sharded cloud (one process per GPU): between all_reduce(min) on the squared distances and all_reduce(min) on
 * the indices, a rank offers its global index only where its own d2 equals the reduced minimum (and is finite), INT32_MAX
 * elsewhere -- so the second reduction returns the lowest global index among the ranks that tie.  Device pointers, async on
 * `stream`; global indices must be < 2^31 - 1. */
int pct_merge_mask_dev(const double *d_d2_local, const double *d_d2_best, const uint32_t *d_idx_local, int32_t *d_cand, int64_t Q, void *stream);
/* behind the second reduction: merged int32 candidates -> u32 indices (INT32_MAX -> PCT_NO_INDEX).  include/pct_shard.h wraps the
 * whole exchange step (these two kernels + the RCCL calls) for C / C++ callers. */
int pct_merge_finish_dev(const int32_t *d_cand, uint32_t *d_idx, int64_t Q, void *stream);
/* ---- device helpers of the spatially routed multi-GPU form (include/pct_shard.h; the host logic lives in libpct_shard.so).
 * cuts: world + 1 ascending slab boundaries along `axis` (cuts[0] = -inf, cuts[world] = +inf); an answer record is
 * {uint32 query, uint32 global index, double d2} = 16 bytes, d2 < 0 = "not certified by its owner". ---- */
int pct_cloud_upload_aos_dev(pct_cloud *c, const void *d_pts, int64_t n, int64_t stride_bytes);      /* setInput from device memory */
int pct_route_owner_dev(const double *cuts, int world, int axis, int rank, const float *d_q, int64_t Q, uint32_t *d_counts /* [world] */,
                        uint32_t *d_mine_ids, float *d_mine_q, void *stream);
/* partitioned batches (every rank brings its own queries): owner + counts per owner, then the queries grouped by owner with their slots */
int pct_route_owner_all_dev(const double *cuts, int world, int axis, const float *d_q, int64_t Q, uint32_t *d_counts /* [world] */, unsigned char *d_owner, void *stream);
int pct_route_partition_dev(const uint32_t *offsets /* host, [world] */, int world, const unsigned char *d_owner, const float *d_q, int64_t Q,
                            uint32_t *d_cursors /* [world] */, float *d_out_xyz, uint32_t *d_out_slot, void *stream);
int pct_route_certify_dev(int axis, double lo_edge, double hi_edge, const float *d_mine_q, const uint32_t *d_mine_ids, int64_t m,
                          const uint32_t *d_lidx, const double *d_ld2, const uint32_t *d_gid, void *d_answers, void *stream);
int pct_route_scatter_dev(const void *d_answers, int64_t n, uint32_t *d_idx, double *d_d2, uint32_t *d_flag_count, uint32_t *d_flag_ids, void *stream);
int pct_route_gather_queries_dev(const float *d_q, const uint32_t *d_ids, int64_t n, float *d_out, void *stream);
int pct_route_to_global_dev(uint32_t *d_lidx, int64_t n, const uint32_t *d_gid, void *stream);
int pct_route_put_back_dev(const uint32_t *d_ids, int64_t n, const uint32_t *d_idx, const double *d_d2, uint32_t *d_out_idx, double *d_out_d2, void *stream);
/* make sure workspaces for batches up to Q exist (call before capturing a graph) */
int pct_cloud_reserve_queries(pct_cloud *c, int64_t Q);

/* ---- hipGraph-captured fixed-shape batches (config C5: 20 Hz replan) ----------------------- */
/* Captures H2D(queries) -> NN kernels -> D2H(idx,d2) once; pct_plan_run replays it.
 * A plan belongs to its cloud and must be destroyed before it.  The captured kernels hold the cloud's point count, index and
 * workspace pointers; whenever one of them changes (upload / append on a cloud without the ring index, pct_cloud_build_grid /
 * drop_grid, pct_cloud_ring_index, a larger batch that grows the workspaces) the next run captures the graph again by itself
 * (one capture costs a few hundred microseconds).  Appends on a ring-indexed cloud change none of them. */
int pct_plan_create_nn(pct_cloud *c, int algo, int64_t Q, pct_plan **out);
int pct_plan_run(pct_plan *p, const float *q, uint32_t *idx, double *d2);
int pct_plan_destroy(pct_plan *p);

/* The whole query side of one replan tick as ONE captured graph (config C5; the reference's chain is
 * rcvPointCloudCallBack -> checkSafeTrajectory, Planner/src/sim_planning_demo.cpp:159-178, 729-781, next to
 * SafeRegionEvaluate's re-check of the corridor nodes, Planner/src/corridor_finder.cpp:829-835):
 *   arguments in (corridor node centres, trajectory, sample times) -> ONE kernel with a block per planner point: sphere
 *   inflation of every corridor node, getPosFromBezier + inflation of every sample of the committed trajectory, inflation of
 *   every control point (pct_ctrl_points_check) -> first colliding sample / control point -> results out.
 * The cloud needs an index: the rolling-map one (pct_cloud_ring_index; appends then never invalidate the plan) or the
 * cell-sorted one (pct_cloud_build_grid; re-captured after a rebuild).  Capacities are fixed at creation: at most max_nodes
 * corridor nodes, max_samples trajectory samples (further ones are counted in nsamples but not evaluated), max_segments
 * segments (13 control points each).  want_nn != 0: exact nearest neighbour for every point (idx / d2 outputs meaningful);
 * 0: the search may stop once everything unseen is beyond max_radius + search_margin (radii identical, idx / d2 then only
 * say "some point at least this near"). */
typedef struct pct_replan_out {
    double *node_radius; uint32_t *node_idx; double *node_d2;                      /* n_nodes each; any may be NULL */
    double *sample_pos, *sample_radius, *sample_d2; uint32_t *sample_idx;          /* up to max_samples (pos: x3); any may be NULL */
    double *ctrl_pos, *ctrl_radius, *ctrl_d2; uint32_t *ctrl_idx;                  /* nctrl (pos: x3); any may be NULL */
    int64_t nsamples, first_hit_sample;                                            /* filled: as pct_bezier_check */
    int64_t nctrl, first_hit_ctrl;                                                 /* filled: as pct_ctrl_points_check */
} pct_replan_out;
int pct_plan_create_replan(pct_cloud *c, int32_t max_nodes, int32_t max_samples, int32_t max_segments, pct_plan **out);
/* traj may be NULL (corridor nodes only) */
int pct_plan_replan_run(pct_plan *p, const pct_inflate_params *prm, const double *nodes, int64_t n_nodes, const pct_bezier_traj *traj,
                        double t_start, double stop_time, double dt, int want_nn, pct_replan_out *out);
/* host wall time of the last pct_plan_replan_run in microseconds: {argument fill, hipGraphLaunch, wait for results, read-out} */
int pct_plan_last_run_us(pct_plan *p, double us[4]);

/* ---- measurement hooks (bench.py): HIP events recorded on the stream the kernels ran on.
 * pct_last_kernel_ms: the last batch's DOMINANT kernel alone (nn_grid_coop_kernel, the brute-force filter
 * or the nn_stream_kernel passes) -- the same quantity rocprofv3 --kernel-trace averages;
 * pct_last_batch_ms: every kernel of the batch (binning, bounds, reduction included). ---------- */
int pct_last_kernel_ms(pct_cloud *c, float *ms);
int pct_last_batch_ms(pct_cloud *c, float *ms);
/* which HIP events the batch entry points record: 0 = none, 1 = around the batch's dominant kernel (default; what
 * pct_last_kernel_ms / pct_kernel_ms_history read), 2 = also around the whole batch (pct_last_batch_ms).  An event pair
 * costs 5-9 us per batch. */
int pct_set_timing(pct_cloud *c, int level);
/* dominant-kernel durations of the most recent batches (up to 64 are kept, oldest first): K batches can be queued back to
 * back without a host sync and every launch's duration read afterwards */
int pct_kernel_ms_history(pct_cloud *c, float *ms, int cap, int *n);
/* Sampling: with stride n > 1 the index path (PCT_ALGO_GRID batches) times only every n-th launch, the first one after this call
 * included -- the kernel's own begin / end timestamps (hipExtLaunchKernel), no marker packets on the stream; timing every launch
 * costs ~4 us of a 160 us step.  pct_kernel_ms_samples: how many durations have been recorded so far (host counter, no sync), so
 * that a caller can tell how many of them fall into a region it brackets. */
int pct_set_timing_stride(pct_cloud *c, int stride);
int pct_kernel_ms_samples(pct_cloud *c, uint64_t *count);
/* algorithmic work of the last batch: points examined (sum over queries), cells examined */
int pct_last_work(pct_cloud *c, uint64_t *points_scanned, uint64_t *cells_scanned);
int pct_set_work_counters(pct_cloud *c, int enabled);
/* diagnostics / tests: which form of the brute-force fp32 filter runs -- -1 automatic (expanded |p|^2 - 2 p.q form while its error
 * band is small against the cloud's point spacing, clouds of 200 000 points or more), 0 always the direct (p - q)^2 form,
 * 1 the expanded form whenever a bounding box exists.  Results are identical; only speed differs. */
int pct_debug_set_filter_mode(int mode);
/* diagnostics: the fp32 upper bounds the streaming filter used for the last batch */
int pct_debug_read_bounds(pct_cloud *c, float *out, int64_t Q);
/* test hook: copies of the cell index as built -- cell_start[ncells + 1] and the cell-ordered records (4 floats per point:
 * x, y, z, bit-cast original index); either pointer may be NULL */
int pct_debug_read_grid(pct_cloud *c, uint32_t *cell_start, float *records);
/* the same index checked on the device, through the caches the query kernels read it through:
 * out = {ids out of range, duplicated ids, records outside their cell's run, decreasing cell_start steps, cell_start[0],
 * cell_start[ncells]} -- a sound index gives {0, 0, 0, 0, 0, n} */
int pct_debug_verify_grid(pct_cloud *c, uint64_t out[6]);
/* the buffers the library holds at this moment, over every handle and its process-wide workspaces: blocks allocated and not yet
 * freed, and their bytes (device, pinned and host-mapped memory together).  A handle that is closed gives all of its own back. */
int pct_debug_live_buffers(int64_t *blocks, int64_t *bytes);
/* work counters of the last instrumented batch: {points scanned, cell runs scanned, pyramid node visits (8 boxes of 32 B each)} */
int pct_last_work_ex(pct_cloud *c, uint64_t out[3]);
/* bounding-box pyramid over the cell index (built for sparsely occupied clouds; PCT_PYRAMID=0/1 never / always):
 * levels = 0 when the cloud has none; empty_fraction = empty cells / cells of the index as built */
int pct_cloud_pyramid_info(const pct_cloud *c, int32_t *levels, int64_t *nodes, double *empty_fraction);

#ifdef __cplusplus
}
#endif
#endif /* PCT_ENGINE_H */
