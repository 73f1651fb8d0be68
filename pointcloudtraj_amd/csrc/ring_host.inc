// ring_host.inc -- host side of the rolling-map index (ring.hpp) and of the fused replan batch; included by engine.hip inside
// its extern "C" block's translation unit (it needs struct pct_cloud and the helpers defined there).  Not a stand-alone header.

namespace {

void ring_free(pct_cloud *c)
{
    c->ring_ht.release(); c->ring_slots.release(); c->ring_ovf.release(); c->ring_where.release(); c->ring_st.release();
    c->ring_cells = 0;
    c->ring_ready = false;
}

// bounding box of the points currently in the SoA arrays (device reduction, one read-back); lo > hi: no row was looked at
int cloud_bbox(pct_cloud *c, float lo[3], float hi[3])
{
    const int64_t n = c->count;
    hipStream_t s = g_stream;
    const int bblocks = (int)std::min<int64_t>(1024, (n + 255) / 256);
    DevBuf<float> d_part;
    PCTCHK(d_part.reset((size_t)bblocks * 6));
    // removals since the last upload: the removed rows (three NaNs) are no data to size a table from
    if (c->ring_removed_any) bbox_partial_kernel<true><<<bblocks, 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)n, d_part);
    else bbox_partial_kernel<false><<<bblocks, 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)n, d_part);
    std::vector<float> part((size_t)bblocks * 6);
    hipError_t e = hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(float), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(PCT_ERR_HIP, "bbox reduction failed: %s", hipGetErrorString(e));
    for (int k = 0; k < 3; k++) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    for (int b = 0; b < bblocks; b++)
        for (int k = 0; k < 3; k++) {
            lo[k] = std::min(lo[k], part[(size_t)b * 6 + k]);
            hi[k] = std::max(hi[k], part[(size_t)b * 6 + 3 + k]);
        }
    return PCT_OK;
}

// Choose the cell size and the table dimensions and allocate the tables.  ext = extent of the window per axis (from the caller,
// or the bounding box of the first data), density = capacity points over that box.
int ring_configure(pct_cloud *c, const double ext_in[3])
{
    ring_free(c);
    double ext[3];
    const double diag = std::max({ ext_in[0], ext_in[1], ext_in[2], 1e-6 });
    double vol = 1.0;
    for (int k = 0; k < 3; k++) { ext[k] = std::max(ext_in[k], diag * 1e-3); vol *= ext[k]; }
    double h = c->ring_cell_req;
    if (!(h > 0)) {
        double ppc = 6.0;                                   // as the cell-sorted index (DESIGN.md): ~6 points per cell
        if (const char *e = std::getenv("PCT_RING_PPC")) ppc = std::max(0.05, std::atof(e));
        h = std::cbrt(vol * ppc / (double)std::max<int64_t>(c->cap, 1));
    }
    if (!(h > 0) || !std::isfinite(h)) h = 1.0;
    if (c->dd_res > 0 && !(c->ring_cell_req > 0)) h = std::max(h, c->dd_res);      // de-dup: a voxel's box then touches at most 3 cells per axis
    // table: the window's extent plus a quarter of slack per axis, rounded up to a power of two; at most 2^24 buckets
    // (8 GiB of records at 32 x 16 B each; only the buckets in use are ever touched)
    int g[3], lg[3];
    for (;;) {
        int64_t cells = 1;
        for (int k = 0; k < 3; k++) {
            g[k] = (int)pow2_at_least<int64_t>(1, std::max<int64_t>(4, (int64_t)std::ceil(1.25 * ext[k] / h) + 2), &lg[k]);
            cells *= g[k];
        }
        if (cells <= (1ll << 24)) break;
        h *= 1.26;                                          // 2x fewer cells
    }
    RingDesc R{};
    R.h = h;
    R.inv_h = 1.0 / h;
    R.gx = g[0]; R.gy = g[1]; R.gz = g[2];
    R.lx = lg[0]; R.ly = lg[1];
    R.K = std::max<uint32_t>(kRingK, std::min<uint32_t>(kRingKMax, c->ring_K));
    const uint32_t ovf_cap = (uint32_t)pow2_at_least<int64_t>(1, 2 * std::max<int64_t>(c->cap, 16) + 16);     // see RingDesc::ovf_mask
    R.ovf_mask = ovf_cap - 1u;
    if (!c->ring_status) PCTCHK(c->ring_status.reset(4));
    c->ring_status.host()[0] = c->ring_status.host()[1] = 0;
    R.status = c->ring_status.get();
    const size_t cells = (size_t)g[0] * g[1] * g[2];
    int ast = c->ring_ht.reset(cells);
    if (!ast) ast = c->ring_slots.reset(cells * R.K);
    if (!ast) ast = c->ring_ovf.reset((size_t)ovf_cap);
    if (!ast) ast = c->ring_where.reset((size_t)c->cap4 + 4);
    if (!ast) ast = c->ring_st.reset(1);
    if (ast) { ring_free(c); return ast; }            // no half-allocated index: the cloud answers by brute force until it is configured again
    c->R = R;
    c->ring_cells = cells;
    c->ring_ready = true;
    c->ring_cfg_count = c->count;
    c->ring_appends_since_cfg = 0;
    c->generation++;
    return PCT_OK;
}

// clear the tables and file every point of the SoA arrays
int ring_refile_all(pct_cloud *c)
{
    hipStream_t s = g_stream;
    HIPCHK(hipMemsetAsync(c->ring_ht, 0, sizeof(uint2) * c->ring_cells, s));
    HIPCHK(hipMemsetAsync(c->ring_st, 0, sizeof(RingState), s));
    if (c->count > 0)
        ring_refile_kernel<<<ceil_div(c->count, 256), 256, 0, s>>>(c->R, c->x, c->y, c->z, 0u, (uint32_t)c->count, c->ring_ht, c->ring_slots,
                                                                   c->ring_ovf, c->ring_where, c->ring_st, c->ring_removed_any ? 1 : 0);
    ring_set_count_kernel<<<1, 1, 0, s>>>(c->ring_st, (uint32_t)c->count);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

// first data on a ring-indexed cloud that has no table yet: size it from the data (or the caller's extent) and file everything
int ring_setup_from_cloud(pct_cloud *c)
{
    double ext[3];
    if (c->ring_extent_req[0] > 0 && c->ring_extent_req[1] > 0 && c->ring_extent_req[2] > 0) {
        for (int k = 0; k < 3; k++) ext[k] = c->ring_extent_req[k];
    } else {
        float lo[3], hi[3];
        PCTCHK(cloud_bbox(c, lo, hi));
        for (int k = 0; k < 3; k++) {
            if (c->ring_removed_any && lo[k] > hi[k]) { ext[k] = 0.0; continue; }     // nothing but removed rows
            if (!std::isfinite(lo[k]) || !std::isfinite(hi[k])) return fail(PCT_ERR_INVALID, "cloud holds non-finite coordinates: give pct_cloud_ring_index an extent");
            ext[k] = std::max((double)hi[k] - (double)lo[k], 0.0);
        }
    }
    PCTCHK(ring_configure(c, ext));
    return ring_refile_all(c);
}

// a host-mapped staging buffer of appended frames -- the producer's (c->frame) or the library's own (c->astage): grow-only, a power
// of two from 64 KiB that holds the frame and 64 bytes of slack.  The caller knows that no launch still reads it.
int ensure_frame_staging(MappedBuf<unsigned char> &b, size_t bytes)
{
    return b.reserve(bytes + 64, pow2_at_least((size_t)1 << 16, bytes + 64));
}

// Self-checks on the host-mapped status words an append's launches wrote.  [0]: the overflow queue was about to overrun its table
// (impossible by the bound in RingDesc; if it happens the SoA arrays are still the truth: rebuild).  [1]: its length -- a table
// sized automatically from unrepresentative first data (a tiny first frame) spills most points into the queue, which every query
// then scans exhaustively; re-size it from the window's current contents once the window has at least doubled since the last
// sizing (bulk duplicates spill whatever the cell size: the doubling rule keeps them from re-sizing on every frame).
int ring_after_append(pct_cloud *c)
{
    hipStream_t s = g_stream;
    if (c->ring_status.host()[0]) {
        c->ring_status.host()[0] = 0;
        PCTCHK(ring_refile_all(c));
        HIPCHK(hipStreamSynchronize(s));
    } else if (!(c->ring_cell_req > 0) && !(c->ring_extent_req[0] > 0) && (int64_t)c->ring_status.host()[1] > c->count / 8 + 64 && c->count >= 2 * std::max<int64_t>(c->ring_cfg_count, 1)) {
        PCTCHK(ring_setup_from_cloud(c));
        HIPCHK(hipStreamSynchronize(s));
    } else if ((int64_t)c->ring_status.host()[1] > c->count / 128 + 4096 && c->ring_K < kRingKMax && c->ring_appends_since_cfg >= 4 &&
               (size_t)c->ring_cells * 2 * c->ring_K * sizeof(float4) <= ((size_t)32 << 30)) {
        // A good share of the window in the overflow queue (every query scans it exhaustively: 100 k entries cost a search ~150 us) although
        // the cells were sized from the window itself: the cells that hold points
        // hold more than K of them -- surfaces on a lattice finer than the cell, the same lattice points sensed frame after frame (the
        // reference's rgbd mode accumulates them, camera_sensor.cpp:160-166).  Every query scans that queue exhaustively (5 M-point window
        // of pillar faces: 2.3 M entries, 3.4 ms per replan tick instead of 0.09), so the buckets get twice the room (at most three
        // times: 32 -> 256 records, table <= 32 GiB) and the window is filed again; captured plans re-capture by the generation count.
        c->ring_K *= 2;
        // (extents that make ring_configure choose the table it has: ceil(1.25 ext / h) + 2 = g - 1 -> the same power of two g)
        double ext[3] = { c->R.h * (c->R.gx - 3.5) / 1.25, c->R.h * (c->R.gy - 3.5) / 1.25, c->R.h * (c->R.gz - 3.5) / 1.25 };
        const float keep_cell = c->ring_cell_req;
        c->ring_cell_req = (float)c->R.h;                 // same cells, same table shape: only the buckets grow
        const int st = ring_configure(c, ext);
        c->ring_cell_req = keep_cell;
        PCTCHK(st);
        PCTCHK(ring_refile_all(c));
        HIPCHK(hipStreamSynchronize(s));
    }
    return PCT_OK;
}

// The overflow queue overran (ring.hpp ring_file: "cannot happen"): points are missing from the index although they are in the SoA
// arrays.  Called after every wait of a batch that searched the ring index: refile the whole window and tell the caller to ask again.
int ring_overrun_repair(pct_cloud *c, bool *again)
{
    *again = false;
    if (!c->ring_ready || !c->ring_status.host() || !c->ring_status.host()[0]) return PCT_OK;
    c->ring_status.host()[0] = 0;
    PCTCHK(ring_refile_all(c));
    HIPCHK(hipStreamSynchronize(g_stream));
    *again = true;
    return PCT_OK;
}

// ask: queues a batch that may have searched the rolling-map index and waits for it.  If the index had lost points meanwhile
// (overflow-queue overrun) it has been refiled by now and the batch is asked once more -- once: a second overrun is repaired, not re-asked.
template <typename F>
int ask_twice_after_overrun(pct_cloud *c, F ask)
{
    bool again = false;
    PCTCHK(ask());
    PCTCHK(ring_overrun_repair(c, &again));
    if (!again) return PCT_OK;
    PCTCHK(ask());
    return ring_overrun_repair(c, &again);
}

// an append that returned before its insert kernel had finished (ring_append): wait for it and run its checks
int ring_finish_pending(pct_cloud *c)
{
    if (!c->append_pending) return PCT_OK;
    c->append_pending = false;
    PCTCHK(express_wait(c));
    if (!c->ring_ready) return PCT_OK;          // the index was dropped / rebuilt meanwhile: nothing left to check
    return ring_after_append(c);
}

// append on a cloud whose ring index is live: evict what the overwritten slots held, store and file the new frame.
// d_own != nullptr: the frame is already in a device buffer the library owns (the survivors of the de-dup filter, below) and `pts`
// is not looked at -- same launches, no staging; the call may return before they have run, as for a frame copied to the staging buffer.
int ring_append(pct_cloud *c, const void *pts, int64_t n, int64_t stride, const unsigned char *d_own = nullptr)
{
    hipStream_t s = g_stream;
    const size_t bytes = (size_t)n * (size_t)stride;
    PCTCHK(ring_finish_pending(c));             // the previous frame has left the staging buffer; its status words are in
    // Frames up to 4 MB go through a host-mapped staging buffer: the evictions (which do not need the new data) are launched first
    // and run while the host copies the frame into the buffer, the insert kernel reads it over the bus, and its last block releases
    // the completion word the host polls -- no DMA setup for a pageable source, no stream synchronise.  Measured (50 k points): 67 us
    // either way -- the 600 KB cross the bus in ~35 us whether the copy engine or the kernel moves them; what the path buys is a tighter
    // p99 and the zero-copy entry point (pct_cloud_append_frame), not the median.
    // in_place: the producer wrote the frame straight into the staging buffer (pct_cloud_frame_buffer / pct_cloud_append_frame)
    const bool in_place = !d_own && pts == c->frame.host() && c->frame.host() != nullptr && bytes <= c->frame.capacity();
    const bool mapped = in_place || ((d_own || bytes <= ((size_t)4 << 20)) && mapped_io_on());
    const unsigned char *d_src = nullptr;
    if (d_own) d_src = d_own;
    else if (in_place) d_src = c->frame;
    else if (mapped) {
        // copies go through a staging buffer of their own: the producer of zero-copy frames owns c->frame.host() and may be writing
        // the next frame into it while the previous (asynchronous) copy append is still being read
        PCTCHK(ensure_frame_staging(c->astage, bytes));
        d_src = c->astage;
    } else {
        PCTCHK(ensure_stage(c, bytes + 64));
        HIPCHK(hipMemcpyAsync(c->d_stage, pts, bytes, hipMemcpyHostToDevice, s));
        d_src = c->d_stage;
    }
    const int64_t count_before = c->count;
    const int64_t first = std::min(n, c->cap - c->ring_next);
    const int64_t part_slot0[2] = { c->ring_next, 0 }, part_n[2] = { first, n - first }, part_off[2] = { 0, first };
    const int64_t new_count = std::min(c->cap, count_before + n);
    for (int k = 0; k < 2; k++) {               // the two parts occupy disjoint slots: every eviction may precede every insertion
        const int64_t cnt = part_n[k], s0 = part_slot0[k];
        if (cnt <= 0) continue;
        const int64_t old_valid = std::max<int64_t>(0, std::min<int64_t>(cnt, count_before - s0));
        if (old_valid > 0)
            ring_evict_kernel<<<ceil_div(old_valid, 256), 256, 0, s>>>(c->R, c->x, c->y, c->z, (uint32_t)s0, (uint32_t)old_valid, c->ring_ht, c->ring_slots,
                                                                       c->ring_ovf, c->ring_where, c->ring_st);
    }
    if (mapped && !in_place && !d_own) std::memcpy(c->astage.host(), pts, bytes);
    for (int k = 0; k < 2; k++) {
        const int64_t cnt = part_n[k], s0 = part_slot0[k];
        if (cnt <= 0) continue;
        const bool last = k == 1 || part_n[1] <= 0;
        ring_insert_kernel<<<ceil_div(cnt, 256), 256, 0, s>>>(c->R, c->x, c->y, c->z, d_src + part_off[k] * stride, (uint32_t)stride, (uint32_t)cnt,
                                                              (uint32_t)s0, c->ring_ht, c->ring_slots, c->ring_ovf, c->ring_where, c->ring_st,
                                                              last ? (uint32_t)new_count : 0xFFFFFFFFu, (last && mapped) ? next_signal(c) : ExpressSignal{});
    }
    HIPCHK(hipGetLastError());
    c->ring_next = (c->ring_next + n) % c->cap;
    c->count = new_count;
    c->content_epoch++;
    c->ring_appends_since_cfg++;
    // A frame copied into the staging buffer leaves the caller's buffer free at once, and everything else this library does with the
    // cloud is ordered behind the insert kernel on the same stream: return without waiting.  The completion word and the status
    // words are looked at when the staging buffer is needed again (the next append) -- a replan graph launched right after the
    // append then queues behind the insert instead of starting after a host round trip (C5 tick: 100 -> ~87 us).
    static const bool async_on = [] { const char *e = std::getenv("PCT_ASYNC_APPEND"); return e ? std::atoi(e) != 0 : true; }();
    if (mapped && !in_place && async_on) { c->append_pending = true; return note_mutation(c); }
    if (mapped) PCTCHK(express_wait(c));        // zero-copy frames: the producer may rewrite the staging buffer as soon as we return
    else HIPCHK(hipStreamSynchronize(s));
    return ring_after_append(c);
}

// ---- de-duplicating appends (ring_dedup.hpp) ---------------------------------------------------------------------------------
int after_replace(pct_cloud *c);

// the host wait behind the tile scan's DdPublish (ring_dedup.hpp): the grand total of the scan launched with `seq`, from the host-mapped {sequence, total}
// pair it publishes
int dd_scan_wait(pct_cloud *c, uint32_t seq, int64_t *total)
{
    PCTCHK(c->dd_word.wait(seq, "the frame filter"));
    *total = (int64_t)c->dd_word.w.host()[1];
    return PCT_OK;
}

// entries of the frame filter's key table for a frame of n points: a power of two >= 2 n (load factor <= 0.5), at least 1024
uint32_t dedup_table_size(int64_t n) { return (uint32_t)pow2_at_least<uint64_t>(1024, 2ull * (uint64_t)n); }

// scratch of the frame filter for a frame of n points (grow-only)
int dedup_ensure(pct_cloud *c, int64_t n)
{
    PCTCHK(c->dd_word.ensure(4));
    const uint32_t T = dedup_table_size(n);
    if (T > c->dd_tcap) {
        HIPCHK(hipStreamSynchronize(g_stream));
        PCTCHK(regrow(c->dd_tcap, T, part(c->dd_keys, T), part(c->dd_vals, T)));
    }
    if (n > c->dd.ncap) {
        HIPCHK(hipStreamSynchronize(g_stream));       // the previous append's insert kernel may still be reading the compacted frame
        const int64_t cap = std::min<int64_t>(std::max<int64_t>(c->cap, 1), std::max<int64_t>(n, 2 * c->dd.ncap));
        PCTCHK(c->dd.ensure(cap, part(c->dd_pslot, (size_t)cap)));      // one group with the table slots
    }
    return PCT_OK;
}

// The filter's launches over the frame at d_src (device-visible), then the ONE host wait of a de-dup append: the survivor count,
// polled in host-mapped memory as express_wait polls its word.  probe = false: the window is empty, the in-frame rule alone.
int dedup_filter(pct_cloud *c, const unsigned char *d_src, int64_t n, int64_t stride, bool probe, int64_t *kept)
{
    hipStream_t s = g_stream;
    const uint32_t T = dedup_table_size(n);
    const uint32_t un = (uint32_t)n;
    const int ntiles = ceil_div(n, kDdTile);
    const DdWindow W{ (uint32_t)c->ring_next, (uint32_t)c->cap, un };
    const uint32_t seq = c->dd_word.next();
    pct_vox::vox_table_init_kernel<<<std::min(ceil_div(T, 256), 2048), 256, 0, s>>>(c->dd_keys, c->dd_vals, T);
    dd_key_kernel<<<ceil_div(n, 256), 256, 0, s>>>(d_src, un, (uint32_t)stride, c->dd_res, c->dd_keys, c->dd_vals, T - 1u, c->dd_pslot);
    if (probe)
        dd_probe_kernel<true><<<ceil_div(n, kDdPointsPerBlock), 256, 0, s>>>(ring_view(c), W, c->dd_res, un, c->dd_keys, c->dd_vals, c->dd_pslot, c->dd.flags);
    else
        dd_probe_kernel<false><<<ceil_div(n, kDdPointsPerBlock), 256, 0, s>>>(RingView{}, W, c->dd_res, un, c->dd_keys, c->dd_vals, c->dd_pslot, c->dd.flags);
    dd_rank_kernel<<<ntiles, 256, 0, s>>>(c->dd.flags, un, c->dd.rank, c->dd.tile);
    scan_tile_sums_kernel<uint32_t><<<1, 256, 0, s>>>(c->dd.tile, (uint32_t)ntiles, DdPublish{ c->dd_word.w, seq });
    dd_compact_kernel<<<ceil_div(n, 256), 256, 0, s>>>(d_src, un, (uint32_t)stride, c->dd.flags, c->dd.rank, c->dd.tile, c->dd.out);
    HIPCHK(hipGetLastError());
    PCTCHK(dd_scan_wait(c, seq, kept));
    if (*kept > n) return fail(PCT_ERR_INTERNAL, "the de-dup filter kept %lld of %lld points", (long long)*kept, (long long)n);
    return PCT_OK;
}

// first data on a rolling-map cloud (the window has no table yet) from a packed frame in a device buffer the library owns: the
// rows go into the ring slots as append_unindexed stores a host frame, and the table is sized from them
int append_unindexed_dev(pct_cloud *c, const float *d_pts, int64_t n)
{
    const unsigned char *src = reinterpret_cast<const unsigned char *>(d_pts);
    const int64_t first = std::min(n, c->cap - c->ring_next);
    if (first > 0) deinterleave_kernel<<<ceil_div(first, 256), 256, 0, g_stream>>>(src, 12u, (uint32_t)first, c->x, c->y, c->z, (uint32_t)c->ring_next);
    if (first < n) deinterleave_kernel<<<ceil_div(n - first, 256), 256, 0, g_stream>>>(src + first * 12, 12u, (uint32_t)(n - first), c->x, c->y, c->z, 0u);
    HIPCHK(hipGetLastError());
    c->ring_next = (c->ring_next + n) % c->cap;
    c->count = std::min(c->cap, c->count + n);
    return after_replace(c);
}

// pct_cloud_append_aos on a rolling-map cloud with de-dup on: filter the frame against itself and the window, append the survivors.
// d_own != nullptr: the frame (packed, stride 12) is already in a device buffer the library owns and `pts` is not looked at
int ring_append_dedup(pct_cloud *c, const void *pts, int64_t n, int64_t stride, const unsigned char *d_own = nullptr)
{
    hipStream_t s = g_stream;
    PCTCHK(ring_finish_pending(c));
    c->dd_last_offered = n;
    c->dd_last_kept = 0;
    c->dd_total_offered += (uint64_t)n;
    if (n == 0) return PCT_OK;
    drop_grid(c);
    // a cloud that holds points but lost its table (an allocation failed) gets it back first: the filter searches the table
    if (!c->ring_ready && c->count > 0) { PCTCHK(ring_setup_from_cloud(c)); HIPCHK(hipStreamSynchronize(s)); }
    PCTCHK(dedup_ensure(c, n));
    const size_t bytes = (size_t)n * (size_t)stride;
    const bool in_place = !d_own && pts == c->frame.host() && c->frame.host() != nullptr && bytes <= c->frame.capacity();
    const unsigned char *d_src = d_own ? d_own : c->frame;
    if (!in_place && !d_own) {
        PCTCHK(ensure_stage(c, bytes + 64));
        HIPCHK(hipMemcpyAsync(c->d_stage, pts, bytes, hipMemcpyHostToDevice, s));
        d_src = c->d_stage;
    }
    int64_t kept = 0;
    PCTCHK(dedup_filter(c, d_src, n, stride, c->ring_ready, &kept));
    // (a copied frame has left the caller's buffer by now: the copy precedes the kernel that released the count.  The compaction
    // kernel may still be reading the frame where the filter found it -- the library's staging buffer, or the producer's, below)
    c->dd_last_kept = kept;
    c->dd_total_kept += (uint64_t)kept;
    if (kept == 0) {                            // nothing changes; a producer's buffer is its own again once the compaction has read it
        if (in_place) HIPCHK(hipStreamSynchronize(s));
        return PCT_OK;
    }
    if (c->ring_ready) {
        PCTCHK(ring_append(c, nullptr, kept, 12, reinterpret_cast<const unsigned char *>(c->dd.out.get())));
        // zero-copy frames: the producer may rewrite the staging buffer as soon as we return, and the compaction kernel read it
        if (in_place) PCTCHK(ring_finish_pending(c));
        return PCT_OK;
    }
    // first data (the window is empty and has no table yet): the compacted frame takes the first-data path, which sizes the table from it
    return append_unindexed_dev(c, c->dd.out, kept);
}

// the cloud's contents were replaced (upload) or grew on a cloud whose ring table does not exist yet
int after_replace(pct_cloud *c)
{
    c->content_epoch++;
    if (!c->ring_on) { c->generation++; return PCT_OK; }     // captured NN plans hold the point count
    if (c->ring_ready) PCTCHK(ring_refile_all(c));
    else if (c->count > 0) PCTCHK(ring_setup_from_cloud(c));
    HIPCHK(hipStreamSynchronize(g_stream));
    return PCT_OK;
}

RingView ring_view(const pct_cloud *c)
{
    RingView V{};
    V.R = c->R;
    V.ht = c->ring_ht;
    V.slots = c->ring_slots;
    V.ovf = c->ring_ovf;
    V.st = c->ring_st;
    return V;
}

}  // namespace

// ---- the fused planner batch: argument block, launch, results ------------------------------------------------------------
struct ReplanCtx {
    int max_nodes = 0, max_samples = 0, max_seg = 0, max_ctrl = 0, row_cap = 0;
    bool copies = false;                 // true: arguments / results cross the bus in memcpy nodes; false: host-mapped memory
    size_t args_bytes = 0, f64_off = 0, u32_off = 0;
    // views of the owners below -- mapped: d_* is the device alias of h_*; copies: pinned h_* and device d_*
    unsigned char *h_args = nullptr, *d_args = nullptr;
    ExpressOut *h_res = nullptr, *d_res_host = nullptr;      // results where the caller reads them (d_res_host: device alias / copy source)
    double *h_pos = nullptr, *d_pos = nullptr;               // positions of samples and control points
    ReplanSummary *h_sum = nullptr, *d_sum = nullptr;
    MappedBuf<unsigned char> m_args;
    MappedBuf<ExpressOut> m_res;
    MappedBuf<double> m_pos;
    MappedBuf<ReplanSummary> m_sum;
    PinnedBuf<unsigned char> p_args;
    PinnedBuf<ExpressOut> p_res;
    PinnedBuf<double> p_pos;
    PinnedBuf<ReplanSummary> p_sum;
    DevBuf<unsigned char> c_args;
    DevBuf<ExpressOut> c_res;
    DevBuf<double> c_pos;
    DevBuf<ReplanSummary> c_sum;
    DevBuf<ReplanMeet> d_meet;
    uint32_t seq = 0;                    // ticks filled so far = launches queued; tick k's header lives in slot k & 1 (ring.hpp ReplanMeet)
    ReplanHeader hdr{};                  // the fixed offsets
    ReplanHeader hdr_sent{};             // the header of the tick in flight, as the host wrote it
};

void replan_ctx_free(ReplanCtx *x) { delete x; }

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int replan_ctx_create(int max_nodes, int max_samples, int max_seg, bool copies, ReplanCtx **out)
{
    ReplanCtx *x = new (std::nothrow) ReplanCtx();
    if (!x) return fail(PCT_ERR_ALLOC, "host allocation failed");
    x->max_nodes = max_nodes; x->max_samples = max_samples; x->max_seg = max_seg;
    x->max_ctrl = max_seg * (kMaxBezierOrder + 1);
    x->row_cap = 3 * (kMaxBezierOrder + 1);
    x->copies = copies;
    static_assert(sizeof(ReplanHeader) <= kReplanHdrSlot, "header slot too small");
    x->f64_off = 2 * kReplanHdrSlot;
    const size_t n64 = (size_t)3 * max_nodes + (size_t)max_seg * x->row_cap + max_seg + max_samples;
    x->u32_off = x->f64_off + align_up(n64 * sizeof(double), 256);
    const size_t n32 = (size_t)max_seg + max_samples + 2 * (size_t)x->max_ctrl;
    x->args_bytes = x->u32_off + align_up(n32 * sizeof(uint32_t), 256);
    const size_t nres = (size_t)max_nodes + max_samples + x->max_ctrl;
    const size_t npos = 3 * ((size_t)max_samples + x->max_ctrl);
    int st = PCT_OK;
    if (copies) {
        st = x->p_args.reset(x->args_bytes);
        if (!st) st = x->p_res.reset(nres);
        if (!st) st = x->p_pos.reset(std::max<size_t>(npos, 1));
        if (!st) st = x->p_sum.reset(1);
        if (!st) st = x->c_args.reset(x->args_bytes);
        if (!st) st = x->c_res.reset(nres);
        if (!st) st = x->c_pos.reset(std::max<size_t>(npos, 1));
        if (!st) st = x->c_sum.reset(1);
        x->h_args = x->p_args; x->h_res = x->p_res; x->h_pos = x->p_pos; x->h_sum = x->p_sum;
        x->d_args = x->c_args; x->d_res_host = x->c_res; x->d_pos = x->c_pos; x->d_sum = x->c_sum;
    } else {
        st = x->m_args.reset(x->args_bytes);
        if (!st) st = x->m_res.reset(nres);
        if (!st) st = x->m_pos.reset(std::max<size_t>(npos, 1));
        if (!st) st = x->m_sum.reset(1);
        x->h_args = x->m_args.host(); x->h_res = x->m_res.host(); x->h_pos = x->m_pos.host(); x->h_sum = x->m_sum.host();
        x->d_args = x->m_args; x->d_res_host = x->m_res; x->d_pos = x->m_pos; x->d_sum = x->m_sum;
    }
    if (!st) st = x->d_meet.reset(1);
    if (!st) {
        const ReplanMeet m0{ 0u, 0x7FFFFFFF, 0x7FFFFFFF, 0u, 0u, { 0u, 0u, 0u } };
        if (hipMemcpy(x->d_meet, &m0, sizeof m0, hipMemcpyHostToDevice) != hipSuccess) st = fail(PCT_ERR_HIP, "hipMemcpy failed");
    }
    if (st) { replan_ctx_free(x); return st; }
    std::memset(x->h_sum, 0, sizeof(ReplanSummary));
    // fixed layout of the variable parts
    ReplanHeader &H = x->hdr;
    H.off_nodes = 0;
    H.off_coef = 3u * (uint32_t)max_nodes;
    H.off_segtime = H.off_coef + (uint32_t)(max_seg * x->row_cap);
    H.off_sample_t = H.off_segtime + (uint32_t)max_seg;
    H.off_orders = 0;
    H.off_sample_seg = (uint32_t)max_seg;
    H.off_ctrl_seg = H.off_sample_seg + (uint32_t)max_samples;
    H.off_ctrl_j = H.off_ctrl_seg + (uint32_t)x->max_ctrl;
    *out = x;
    return PCT_OK;
}

// the launches of one fused batch on stream s (plain or under capture); grid = the context's capacity
int replan_enqueue(pct_cloud *c, ReplanCtx *x, hipStream_t s)
{
    const int blocks = x->max_nodes + x->max_samples + x->max_ctrl;
    const ReplanHeader *dh = reinterpret_cast<const ReplanHeader *>(x->d_args);
    const double *f64a = reinterpret_cast<const double *>(x->d_args + x->f64_off);
    const uint32_t *u32a = reinterpret_cast<const uint32_t *>(x->d_args + x->u32_off);
    if (x->copies) HIPCHK(hipMemcpyAsync(x->d_args, x->h_args, x->args_bytes, hipMemcpyHostToDevice, s));
    // ONE kernel: every block writes its result where the caller reads it (d_res_host: host-mapped memory, or the device buffer
    // the copies below take) and the last one to finish adds the summary and the sequence word
    if (c->ring_ready)
        replan_block_kernel<true><<<blocks, 256, 0, s>>>(ring_view(c), GridDesc{}, nullptr, nullptr, 0, dh, f64a, u32a, (uint32_t)c->index_base,
                                                         x->d_res_host, x->d_pos, x->d_meet, x->d_sum);
    else
        replan_block_kernel<false><<<blocks, 256, 0, s>>>(RingView{}, c->G, c->sorted, c->cell_start, (int)std::min<int64_t>(c->count, 1), dh, f64a, u32a,
                                                          (uint32_t)c->index_base, x->d_res_host, x->d_pos, x->d_meet, x->d_sum);
    replan_empty_kernel<<<1, 1, 0, s>>>(dh, x->d_meet, x->d_sum);
    if (x->copies) {
        const size_t nres = (size_t)blocks;
        HIPCHK(hipMemcpyAsync(x->h_res, x->d_res_host, nres * sizeof(ExpressOut), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(x->h_pos, x->d_pos, 3 * ((size_t)x->max_samples + x->max_ctrl) * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(x->h_sum, x->d_sum, sizeof(ReplanSummary), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

// Fill the argument block: header, corridor nodes, trajectory, the sample times (the reference's nested loops,
// sim_planning_demo.cpp:729-771) and the control-point list (segments from the one holding t_start on).
// sample_cap: the caller's sample capacity.  Only the first min(context capacity, sample_cap) samples are handed to the kernel, so
// the first hit it reports covers exactly the samples the caller reads, whatever capacity an earlier call left the context with.
int replan_fill(ReplanCtx *x, const pct_inflate_params *p, const double *nodes, int64_t n_nodes, const pct_bezier_traj *traj, double t_start,
                double stop_time, double dt, int want_nn, int with_ctrl, int64_t sample_cap, int64_t *nsamples_total)
{
    const int64_t room = std::min<int64_t>(x->max_samples, std::max<int64_t>(sample_cap, 0));
    ReplanHeader H = x->hdr;
    H.P = to_dev(p);
    H.n_nodes = (int32_t)n_nodes;
    H.n_samples = 0; H.n_ctrl = 0; H.nseg = 0; H.row_stride = 0; H.first_seg = 0;
    H.want_nn = want_nn;
    double *f64a = reinterpret_cast<double *>(x->h_args + x->f64_off);
    uint32_t *u32a = reinterpret_cast<uint32_t *>(x->h_args + x->u32_off);
    if (n_nodes > x->max_nodes) return fail(PCT_ERR_CAPACITY, "%lld corridor nodes > plan capacity %d", (long long)n_nodes, x->max_nodes);
    if (n_nodes) std::memcpy(f64a + H.off_nodes, nodes, sizeof(double) * 3 * n_nodes);
    *nsamples_total = 0;
    if (traj) {
        if (traj->nseg <= 0 || traj->nseg > x->max_seg) return fail(PCT_ERR_CAPACITY, "%d segments > plan capacity %d", traj->nseg, x->max_seg);
        PCTCHK(bezier_check_orders(traj));
        H.nseg = traj->nseg;
        H.row_stride = x->row_cap;
        for (int i = 0; i < traj->nseg; i++) {
            const int m3 = 3 * (traj->orders[i] + 1);
            std::memcpy(f64a + H.off_coef + (size_t)i * x->row_cap, traj->polycoef + (size_t)i * traj->row_stride, sizeof(double) * m3);
            f64a[H.off_segtime + i] = traj->seg_time[i];
            u32a[H.off_orders + i] = (uint32_t)traj->orders[i];
        }
        double t_s;
        const int first_seg = bezier_first_segment(traj->seg_time, 0, traj->nseg, t_start, t_s);
        H.first_seg = first_seg;
        const int64_t n = bezier_enumerate<false>(traj->seg_time, 0, traj->nseg, t_start, stop_time, dt, room, kBezierNoBound, [&](long long k, double t, int seg) {
            f64a[H.off_sample_t + k] = t;
            u32a[H.off_sample_seg + k] = (uint32_t)seg;
        });
        *nsamples_total = n;
        H.n_samples = (int32_t)std::min<int64_t>(n, room);
        if (with_ctrl) {
            int k = 0;
            for (int i = first_seg; i < traj->nseg; i++)
                for (int j = 0; j <= traj->orders[i]; j++) { u32a[H.off_ctrl_seg + k] = (uint32_t)i; u32a[H.off_ctrl_j + k] = (uint32_t)j; k++; }
            H.n_ctrl = k;
        }
    }
    H.seq = ++x->seq;
    x->hdr_sent = H;
    std::memcpy(x->h_args + (size_t)(H.seq & 1u) * kReplanHdrSlot, &H, sizeof H);     // the slot launch number `seq` reads
    return PCT_OK;
}

// wait for the batch: the finish kernel's sequence word in host-mapped memory (a stream sync costs ~20 us more), or the stream
int replan_wait(ReplanCtx *x, hipStream_t s)
{
    hipError_t e = hipSuccess;       // (never poll in `copies` mode: the word arrives with the last copy)
    const bool seen = pct_host::wait_word(&x->h_sum->seq, x->seq, !x->copies && poll_results() ? 40000000l : 0l, [&] { e = hipStreamSynchronize(s); });
    if (e != hipSuccess) return fail(PCT_ERR_HIP, "hipStreamSynchronize -> %s", hipGetErrorString(e));
    if (!seen) return fail(PCT_ERR_HIP, "replan batch finished without its sequence word (%u != %u)", x->h_sum->seq, x->seq);
    return PCT_OK;
}

// sample_cap: how many sample entries the caller's arrays hold (the captured plan documents "max_samples"; pct_bezier_check hands
// its own `cap` down).  replan_fill was given the same figure, so the evaluated samples are the first min(nsamples, sample_cap) and
// first_hit covers exactly those; nsamples is the unclipped count.
void replan_read(const ReplanCtx *x, int64_t nsamples_total, pct_replan_out *o, int64_t sample_cap)
{
    const ReplanHeader &H = x->hdr_sent;
    const ExpressOut *r = x->h_res;
    const int n_out = (int)std::min<int64_t>(H.n_samples, std::max<int64_t>(sample_cap, 0));
    for (int i = 0; i < H.n_nodes; i++) {
        if (o->node_radius) o->node_radius[i] = r[i].radius;
        if (o->node_idx) o->node_idx[i] = r[i].idx;
        if (o->node_d2) o->node_d2[i] = r[i].d2;
    }
    r += H.n_nodes;
    for (int i = 0; i < n_out; i++) {
        if (o->sample_radius) o->sample_radius[i] = r[i].radius;
        if (o->sample_idx) o->sample_idx[i] = r[i].idx;
        if (o->sample_d2) o->sample_d2[i] = r[i].d2;
    }
    if (o->sample_pos && n_out) std::memcpy(o->sample_pos, x->h_pos, sizeof(double) * 3 * n_out);
    r += H.n_samples;
    for (int i = 0; i < H.n_ctrl; i++) {
        if (o->ctrl_radius) o->ctrl_radius[i] = r[i].radius;
        if (o->ctrl_idx) o->ctrl_idx[i] = r[i].idx;
        if (o->ctrl_d2) o->ctrl_d2[i] = r[i].d2;
    }
    if (o->ctrl_pos && H.n_ctrl) std::memcpy(o->ctrl_pos, x->h_pos + 3 * (size_t)H.n_samples, sizeof(double) * 3 * H.n_ctrl);
    o->nsamples = nsamples_total;
    o->nctrl = H.n_ctrl;
    o->first_hit_sample = x->h_sum->first_hit_sample;
    o->first_hit_ctrl = x->h_sum->first_hit_ctrl;
}

bool cloud_indexed(const pct_cloud *c) { return c->ring_ready || c->has_grid; }

bool replan_copies_default()
{
    static const bool v = [] { const char *e = std::getenv("PCT_REPLAN_COPIES"); return e ? std::atoi(e) != 0 : false; }();
    return v;
}

// un-captured fused batch on the cloud's own context (pct_bezier_check / pct_ctrl_points_check / small inflations on ring clouds)
int replan_direct(pct_cloud *c, const pct_inflate_params *p, const double *nodes, int64_t n_nodes, const pct_bezier_traj *traj, double t_start,
                  double stop_time, double dt, int want_nn, int with_ctrl, int max_samples, pct_replan_out *o)
{
    const int need_seg = traj ? traj->nseg : 1;
    if (!c->rp || c->rp->max_nodes < n_nodes || c->rp->max_seg < need_seg || c->rp->max_samples < max_samples) {
        HIPCHK(hipStreamSynchronize(g_stream));
        replan_ctx_free(c->rp);
        c->rp = nullptr;
        PCTCHK(replan_ctx_create((int)std::max<int64_t>(n_nodes, 64), std::max(max_samples, 128), std::max(need_seg, 4), false, &c->rp));
    }
    int64_t ntot = 0;
    PCTCHK(ask_twice_after_overrun(c, [&] {
        PCTCHK(replan_fill(c->rp, p, nodes, n_nodes, traj, t_start, stop_time, dt, want_nn, with_ctrl, max_samples, &ntot));
        if (const int st = replan_enqueue(c, c->rp, g_stream)) { c->rp->seq--; return st; }     // nothing ran: the slot is filled again
        return replan_wait(c->rp, g_stream);
    }));
    replan_read(c->rp, ntot, o, max_samples);
    return PCT_OK;
}

}  // namespace

extern "C" {

// ---- rolling-map index -----------------------------------------------------------------------------------------------------
int pct_cloud_ring_index(pct_cloud *c, float cell_size, const float extent[3])
{
    if (!c) return fail(PCT_ERR_INVALID, "null cloud");
    if (c->host_mapped) return fail(PCT_ERR_INVALID, "small (host-mapped) clouds take no index");
    if (cell_size < 0 || !std::isfinite(cell_size)) return fail(PCT_ERR_INVALID, "bad cell size");
    if (c->ring_on && c->dd_res > 0 && cell_size > 0 && (double)cell_size < c->dd_res / 2)
        return fail(PCT_ERR_INVALID, "cell size %g is less than half the de-dup voxel %g (pct_cloud_ring_dedup)", (double)cell_size, c->dd_res);
    HIPCHK(hipStreamSynchronize(g_stream));
    drop_grid(c);
    c->ring_on = true;
    c->ring_cell_req = cell_size;
    for (int k = 0; k < 3; k++) c->ring_extent_req[k] = extent ? extent[k] : 0.0f;
    ring_free(c);
    c->generation++;
    const bool have_extent = extent && extent[0] > 0 && extent[1] > 0 && extent[2] > 0;
    if (c->count > 0 || have_extent) {
        PCTCHK(ring_setup_from_cloud(c));
        HIPCHK(hipStreamSynchronize(g_stream));
    }
    return PCT_OK;
}

int pct_cloud_frame_buffer(pct_cloud *c, int64_t bytes, void **host_ptr)
{
    if (!c || bytes <= 0 || !host_ptr) return fail(PCT_ERR_INVALID, "bad frame_buffer arguments");
    if (c->host_mapped) return fail(PCT_ERR_INVALID, "small (host-mapped) clouds are appended with plain stores already");
    HIPCHK(hipStreamSynchronize(g_stream));             // a launch may still be reading the old buffer
    PCTCHK(ring_finish_pending(c));
    PCTCHK(ensure_frame_staging(c->frame, (size_t)bytes));
    *host_ptr = c->frame.host();
    return PCT_OK;
}

int pct_cloud_append_frame(pct_cloud *c, int64_t n, int64_t stride_bytes)
{
    if (!c || !c->frame.host()) return fail(PCT_ERR_INVALID, "no frame buffer (pct_cloud_frame_buffer)");
    if (n < 0 || stride_bytes < 12 || (uint64_t)n * (uint64_t)stride_bytes > c->frame.capacity()) return fail(PCT_ERR_INVALID, "the frame does not fit the buffer handed out");
    return pct_cloud_append_aos(c, c->frame.host(), n, stride_bytes);
}

int pct_cloud_ring_drop(pct_cloud *c)
{
    if (!c) return fail(PCT_ERR_INVALID, "null cloud");
    HIPCHK(hipStreamSynchronize(g_stream));
    ring_free(c);
    c->ring_on = false;
    c->dd_res = 0.0;
    c->rc_fraction = 0.0;
    c->generation++;
    return PCT_OK;
}

int pct_cloud_ring_dedup(pct_cloud *c, double res)
{
    if (!c) return fail(PCT_ERR_INVALID, "null cloud");
    if (!(res >= 0) || !std::isfinite(res)) return fail(PCT_ERR_INVALID, "the de-dup voxel size must be finite and >= 0");
    if (res == 0) { c->dd_res = 0.0; return PCT_OK; }
    if (!c->ring_on) return fail(PCT_ERR_INVALID, "de-duplicating appends need the rolling-map index (pct_cloud_ring_index)");
    if (c->ring_cell_req > 0 && (double)c->ring_cell_req < res / 2)
        return fail(PCT_ERR_INVALID, "the de-dup voxel %g is more than twice the cell size %g asked of pct_cloud_ring_index", res, (double)c->ring_cell_req);
    PCTCHK(ring_finish_pending(c));
    c->dd_res = res;
    c->dd_last_offered = c->dd_last_kept = 0;
    c->dd_total_offered = c->dd_total_kept = 0;
    // a table whose cell size was chosen automatically is sized again if its cells are smaller than the voxel
    if (c->ring_ready && !(c->ring_cell_req > 0) && c->R.h < res) {
        HIPCHK(hipStreamSynchronize(g_stream));
        PCTCHK(ring_setup_from_cloud(c));
        HIPCHK(hipStreamSynchronize(g_stream));
    }
    return PCT_OK;
}

int pct_cloud_ring_dedup_last(pct_cloud *c, int64_t *offered, int64_t *kept, uint8_t *flags, int64_t cap, uint64_t *total_offered,
                              uint64_t *total_kept)
{
    if (!c || (flags && cap < 0)) return fail(PCT_ERR_INVALID, "bad ring_dedup_last arguments");
    if (!(c->dd_res > 0)) return fail(PCT_ERR_INVALID, "de-duplicating appends are off on this cloud (pct_cloud_ring_dedup)");
    if (offered) *offered = c->dd_last_offered;
    if (kept) *kept = c->dd_last_kept;
    if (total_offered) *total_offered = c->dd_total_offered;
    if (total_kept) *total_kept = c->dd_total_kept;
    const int64_t nf = std::min(c->dd_last_offered, cap);
    if (flags && nf > 0) {
        HIPCHK(hipStreamSynchronize(g_stream));
        HIPCHK(hipMemcpy(flags, c->dd.flags, (size_t)nf, hipMemcpyDeviceToHost));
    }
    return PCT_OK;
}

int pct_cloud_has_ring_index(const pct_cloud *c) { return c && c->ring_ready ? 1 : 0; }

int pct_cloud_ring_bucket_records(const pct_cloud *c) { return (c && c->ring_ready) ? (int)c->R.K : 0; }

int pct_cloud_ring_info(pct_cloud *c, int32_t dims[3], double *cell_size, int64_t *overflow_entries)
{
    if (!c || !c->ring_ready) return fail(PCT_ERR_INVALID, "no ring index");
    if (dims) { dims[0] = c->R.gx; dims[1] = c->R.gy; dims[2] = c->R.gz; }
    if (cell_size) *cell_size = c->R.h;
    if (overflow_entries) {
        RingState st{};
        HIPCHK(hipStreamSynchronize(g_stream));
        HIPCHK(hipMemcpy(&st, c->ring_st, sizeof st, hipMemcpyDeviceToHost));
        *overflow_entries = (int64_t)(uint32_t)(st.ovf_tail - st.ovf_head);
    }
    return PCT_OK;
}

/* diagnostics (tests): where the record of ring slot `slot` is filed and what is stored there.
 * out[0] = where word, out[1] = bucket of the slot's current coordinates, out[2] / out[3] = that bucket's head / tail (or the
 * overflow queue's when the where word says so), out[4] = id word of the record at the filed position, out[5] = queue live length */
int pct_debug_ring_slot(pct_cloud *c, int64_t slot, uint32_t out[6])
{
    if (!c || !c->ring_ready || slot < 0 || slot >= c->cap || !out) return fail(PCT_ERR_INVALID, "bad debug_ring_slot arguments");
    HIPCHK(hipDeviceSynchronize());
    uint32_t w = 0;
    float p[3];
    HIPCHK(hipMemcpy(&w, c->ring_where + slot, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&p[0], c->x + slot, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&p[1], c->y + slot, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&p[2], c->z + slot, 4, hipMemcpyDeviceToHost));
    const RingDesc &R = c->R;
    int cc[3];
    for (int k = 0; k < 3; k++) {
        const double v = std::floor((double)p[k] * R.inv_h);
        cc[k] = !(v > -(double)kRingCellClamp && v < (double)kRingCellClamp) ? (v > 0.0 ? kRingCellClamp : -kRingCellClamp) : (int)v;
    }
    const uint32_t b = ((uint32_t)(cc[2] & (R.gz - 1)) << (R.lx + R.ly)) | ((uint32_t)(cc[1] & (R.gy - 1)) << R.lx) | (uint32_t)(cc[0] & (R.gx - 1));
    RingState st{};
    HIPCHK(hipMemcpy(&st, c->ring_st, sizeof st, hipMemcpyDeviceToHost));
    out[0] = w; out[1] = b; out[5] = st.ovf_tail - st.ovf_head;
    float4 rec;
    if (w & kRingInOvf) {
        out[2] = st.ovf_head; out[3] = st.ovf_tail;
        HIPCHK(hipMemcpy(&rec, c->ring_ovf + (w & R.ovf_mask), sizeof rec, hipMemcpyDeviceToHost));
    } else {
        uint2 ht;
        HIPCHK(hipMemcpy(&ht, c->ring_ht + b, sizeof ht, hipMemcpyDeviceToHost));
        out[2] = ht.x; out[3] = ht.y;
        HIPCHK(hipMemcpy(&rec, c->ring_slots + (size_t)b * R.K + (w & (R.K - 1)), sizeof rec, hipMemcpyDeviceToHost));
    }
    std::memcpy(&out[4], &rec.w, 4);
    return PCT_OK;
}

// ---- control-point check (SURVEY 3.3's build extension) -----------------------------------------------------------------------
int pct_ctrl_points_check(pct_cloud *c, const pct_bezier_traj *traj, const pct_inflate_params *p, double t_start, int64_t *first_hit,
                          int64_t *nctrl, int64_t cap, double *pos, double *radius, double *d2, uint32_t *idx)
{
    if (!c || !traj || !p || !first_hit || !nctrl || !traj->polycoef || !traj->seg_time || !traj->orders || traj->nseg <= 0 || cap < 0)
        return fail(PCT_ERR_INVALID, "bad ctrl_points_check arguments");
    PCTCHK(bezier_check_orders(traj));
    // the control points in world units, segments from the one holding t_start on (the segment search of checkSafeTrajectory)
    double t_s;
    const int first_seg = bezier_first_segment(traj->seg_time, 0, traj->nseg, t_start, t_s);
    std::vector<double> pts;
    for (int i = first_seg; i < traj->nseg; i++) {
        const int m = traj->orders[i] + 1;
        const double *row = traj->polycoef + (size_t)i * traj->row_stride, T = traj->seg_time[i];
        for (int j = 0; j < m; j++) { pts.push_back(row[j] * T); pts.push_back(row[m + j] * T); pts.push_back(row[2 * m + j] * T); }
    }
    const int64_t n = (int64_t)pts.size() / 3;
    std::vector<double> r((size_t)n), dd((size_t)n);
    std::vector<uint32_t> ii((size_t)n);
    PCTCHK(pct_inflate_batch(c, p, pts.data(), n, r.data(), (idx || d2) ? ii.data() : nullptr, (idx || d2) ? dd.data() : nullptr));
    int64_t fh = -1;
    for (int64_t k = 0; k < n; k++) {
        if (fh < 0 && r[(size_t)k] < 0.0) fh = k;
        if (k < cap) {
            if (pos) { pos[3 * k] = pts[3 * (size_t)k]; pos[3 * k + 1] = pts[3 * (size_t)k + 1]; pos[3 * k + 2] = pts[3 * (size_t)k + 2]; }
            if (radius) radius[k] = r[(size_t)k];
            if (d2) d2[k] = dd[(size_t)k];
            if (idx) idx[k] = ii[(size_t)k];
        }
    }
    *nctrl = n;
    *first_hit = fh;
    return PCT_OK;
}

// ---- the captured replan batch ---------------------------------------------------------------------------------------------
static int plan_capture_replan(pct_plan *p)
{
    if (!cloud_indexed(p->c)) return fail(PCT_ERR_INVALID, "the replan plan needs an index on the cloud (pct_cloud_ring_index or pct_cloud_build_grid)");
    return plan_capture(p, [&] { return replan_enqueue(p->c, p->rx, g_stream); });
}

int pct_plan_create_replan(pct_cloud *c, int32_t max_nodes, int32_t max_samples, int32_t max_segments, pct_plan **out)
{
    if (!c || !out || max_nodes < 0 || max_samples < 0 || max_segments < 0 || max_nodes + max_samples + max_segments <= 0 ||
        max_nodes > 65536 || max_samples > 65536 || max_segments > 4096)
        return fail(PCT_ERR_INVALID, "bad replan plan shape");
    PCTCHK(require_init());
    pct_plan *p = new (std::nothrow) pct_plan();
    if (!p) return fail(PCT_ERR_ALLOC, "host allocation failed");
    p->kind = 1;
    p->c = c;
    int st = replan_ctx_create(max_nodes, max_samples, std::max(max_segments, 1), replan_copies_default(), &p->rx);
    if (!st) st = plan_capture_replan(p);
    if (st) { pct_plan_destroy(p); return st; }
    *out = p;
    return PCT_OK;
}

int pct_plan_replan_run(pct_plan *p, const pct_inflate_params *prm, const double *nodes, int64_t n_nodes, const pct_bezier_traj *traj,
                        double t_start, double stop_time, double dt, int want_nn, pct_replan_out *out)
{
    if (!p || p->kind != 1 || !prm || !out || n_nodes < 0 || (n_nodes > 0 && !nodes) || (traj && !(dt > 0)))
        return fail(PCT_ERR_INVALID, "bad replan_run arguments");
    if (traj && (!traj->polycoef || !traj->seg_time || !traj->orders)) return fail(PCT_ERR_INVALID, "bad trajectory");
    pct_cloud *c = p->c;
    if (p->generation != c->generation) PCTCHK(plan_capture_replan(p));       // the cloud's index was rebuilt / replaced: capture again
    int64_t ntot = 0;
    return ask_twice_after_overrun(c, [&]() -> int {        // the index lost points (overflow-queue overrun): refiled, asked once more
        const auto t0 = std::chrono::steady_clock::now();
        PCTCHK(replan_fill(p->rx, prm, nodes, n_nodes, traj, t_start, stop_time, dt, want_nn, 1, p->rx->max_samples, &ntot));
        const auto t1 = std::chrono::steady_clock::now();
        if (const hipError_t le = hipGraphLaunch(p->exec, g_stream); le != hipSuccess) {
            p->rx->seq--;                                        // nothing ran: host and device tick counts stay in step
            return fail(PCT_ERR_HIP, "hipGraphLaunch -> %s", hipGetErrorString(le));
        }
        const auto t2 = std::chrono::steady_clock::now();
        PCTCHK(replan_wait(p->rx, g_stream));
        const auto t3 = std::chrono::steady_clock::now();
        replan_read(p->rx, ntot, out, p->rx->max_samples);
        const auto t4 = std::chrono::steady_clock::now();
        const auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        p->run_us[0] = us(t0, t1); p->run_us[1] = us(t1, t2); p->run_us[2] = us(t2, t3); p->run_us[3] = us(t3, t4);
        return PCT_OK;
    });
}

/* host wall time of the last pct_plan_replan_run, microseconds: argument fill, hipGraphLaunch, wait for the results, read-out */
int pct_plan_last_run_us(pct_plan *p, double us[4])
{
    if (!p || !us) return fail(PCT_ERR_INVALID, "bad arguments");
    for (int k = 0; k < 4; k++) us[k] = p->run_us[k];
    return PCT_OK;
}

}  // extern "C"

// ---- removing points from the rolling map (ring_remove.hpp) ----------------------------------------------------------------------
namespace {

int ring_remove_ensure(pct_cloud *c)
{
    PCTCHK(c->rm_word.ensure(4));
    if (!c->d_rm_meet) {
        PCTCHK(c->d_rm_meet.reset(1));
        HIPCHK(hipMemsetAsync(c->d_rm_meet, 0, sizeof(RingRemoveMeet), g_stream));
    }
    return PCT_OK;
}

// the ONE host wait of a removal: {removed, live after}, polled in host-mapped memory as the de-dup filter's survivor count is
int ring_remove_wait(pct_cloud *c, uint32_t seq, int64_t *removed, int64_t *live)
{
    PCTCHK(c->rm_word.wait(seq, "the removal"));
    *removed = (int64_t)c->rm_word.w.host()[1];
    *live = (int64_t)c->rm_word.w.host()[2];
    if (*removed + *live > c->count) return fail(PCT_ERR_INTERNAL, "a removal counted %lld + %lld rows of %lld", (long long)*removed, (long long)*live, (long long)c->count);
    return PCT_OK;
}

// what every removal entry point asks first: a live rolling-map index, the append in flight finished (the removal sees its frame)
int ring_remove_begin(pct_cloud *c, const char *what)
{
    if (!c->ring_on) return fail(PCT_ERR_INVALID, "%s needs the rolling-map index (pct_cloud_ring_index)", what);
    PCTCHK(ring_finish_pending(c));
    if (!c->ring_ready && c->count > 0) return fail(PCT_ERR_INVALID, "%s: the cloud has no live rolling-map index", what);
    return PCT_OK;
}

// The window in age order (rc_slot) and the scope of a judgement over its `newest` most recent rows (<= 0 or >= size: every row):
// age positions [p0, size), `judged` of them.  ring_scope(c, 0): the whole window.
struct RingScope { RcWindow W; uint32_t p0; int64_t judged; };

RingScope ring_scope(const pct_cloud *c, int64_t newest)
{
    const int64_t n = c->count, judged = (newest <= 0 || newest >= n) ? n : newest;
    return RingScope{ RcWindow{ (uint32_t)(n == c->cap ? c->ring_next : 0), (uint32_t)c->cap, (uint32_t)n }, (uint32_t)(n - judged), judged };
}

// a judgement that counts its work (pct_set_work_counters) starts from zeroed device counters; nothing to do when counting is off
int ring_work_begin(pct_cloud *c)
{
    if (!c->count_work) return PCT_OK;
    c->host_work = false;
    HIPCHK(hipMemsetAsync(c->d_work, 0, sizeof(WorkCounters) * kWorkSlots, g_stream));
    return PCT_OK;
}

// the window becomes the empty cloud (the empty-window rule of the removal paragraph): size 0, cursor at slot 0, tables cleared
int ring_reset_empty(pct_cloud *c)
{
    c->count = 0;
    c->ring_next = 0;
    c->ring_removed_any = false;
    PCTCHK(ring_refile_all(c));
    HIPCHK(hipStreamSynchronize(g_stream));
    return PCT_OK;
}

// ---- compacting the window (ring_compact.hpp) ---------------------------------------------------------------------------------------
// scratch of a compaction (grow-only; the capacity never changes, so it is allocated once): three SoA arrays, tile totals, and the
// device remap when a caller asks for it
int ring_compact_ensure(pct_cloud *c, bool want_remap)
{
    PCTCHK(c->dd_word.ensure(4));
    if (c->rc_rows < c->cap) {
        HIPCHK(hipStreamSynchronize(g_stream));
        c->rc_rows = 0;
        PCTCHK(c->rc_xyz.reserve(3 * (size_t)c->cap));
        PCTCHK(c->rc_tile.reserve((size_t)ceil_div(c->cap, kRcTile)));
        c->rc_rows = c->cap;
    }
    if (want_remap && c->rc_remap.capacity() < (size_t)c->cap) {
        HIPCHK(hipStreamSynchronize(g_stream));
        PCTCHK(c->rc_remap.reserve((size_t)c->cap));
    }
    return PCT_OK;
}

// The compaction itself; the caller has finished the append in flight and checked the arguments, and the window holds rows.
// known_live >= 0: the wait of the removal that asks (auto mode) has delivered L already and L < size: no wait of its own.
// remap (host, may be null): filled for the old slots [0, old size).
int ring_compact_run(pct_cloud *c, int64_t known_live, int64_t *live_out, uint32_t *remap)
{
    hipStream_t s = g_stream;
    const int64_t n = c->count;
    PCTCHK(ring_compact_ensure(c, remap != nullptr));
    const RcWindow W = ring_scope(c, 0).W;
    const int ntiles = ceil_div(n, kRcTile);
    const uint32_t seq = c->dd_word.next();
    rc_count_kernel<<<ntiles, 256, 0, s>>>(W, c->x, c->y, c->z, c->rc_tile);
    scan_tile_sums_kernel<uint32_t><<<1, 256, 0, s>>>(c->rc_tile.get(), (uint32_t)ntiles, DdPublish{ c->dd_word.w, seq });
    HIPCHK(hipGetLastError());
    int64_t L = known_live;
    if (L < 0) {
        PCTCHK(dd_scan_wait(c, seq, &L));
        if (L > n) return fail(PCT_ERR_INTERNAL, "a compaction counted %lld live rows of %lld", (long long)L, (long long)n);
    }
    *live_out = L;
    const uint32_t base = (uint32_t)c->index_base;
    if (L == n) {                               // nothing to reclaim: nothing moves, not even a wrapped ring's rotation
        if (remap) for (int64_t i = 0; i < n; i++) remap[i] = base + (uint32_t)i;
        return PCT_OK;
    }
    if (L == 0) {                               // only the caller's own NaN rows were left: the empty-window rule
        if (remap) for (int64_t i = 0; i < n; i++) remap[i] = PCT_NO_INDEX;
        PCTCHK(ring_reset_empty(c));
        c->content_epoch++;
        return note_mutation(c);
    }
    float *ox = c->rc_xyz.get(), *oy = ox + c->rc_rows, *oz = oy + c->rc_rows;
    rc_scatter_kernel<<<ntiles, 256, 0, s>>>(W, c->x, c->y, c->z, c->rc_tile, ox, oy, oz, remap ? c->rc_remap.get() : nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->x, ox, sizeof(float) * (size_t)L, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(c->y, oy, sizeof(float) * (size_t)L, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(c->z, oz, sizeof(float) * (size_t)L, hipMemcpyDeviceToDevice, s));
    c->count = L;
    c->ring_next = L % c->cap;
    c->ring_removed_any = false;                // no NaN row is left below the new size
    PCTCHK(ring_refile_all(c));
    c->content_epoch++;
    c->rc_count++;
    if (remap) {                                // the second wait, only for a caller who asks for the remap
        HIPCHK(hipMemcpyAsync(remap, c->rc_remap, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (base) for (int64_t i = 0; i < n; i++) if (remap[i] != PCT_NO_INDEX) remap[i] += base;
    }
    return note_mutation(c);
}

// bookkeeping behind a removal's wait.  A window left without a single row free of NaN becomes the empty cloud: what an upload of
// zero points does to a rolling-map cloud (size 0, cursor at slot 0, tables cleared; the index stays configured and de-dup stays on,
// captured plans stay valid: no pointer, table shape or workspace changes).
int ring_remove_finish(pct_cloud *c, int64_t removed, int64_t live)
{
    if (removed > 0) {
        c->ring_removed_any = true;
        c->content_epoch++;
        if (live == 0) PCTCHK(ring_reset_empty(c));
    }
    // auto-compaction (pct_cloud_ring_autocompact), on the exact counts this removal's wait delivered
    if (c->rc_fraction > 0 && live > 0 && (double)(c->count - live) >= c->rc_fraction * (double)c->cap) {
        int64_t L = 0;
        return ring_compact_run(c, live, &L, nullptr);
    }
    return note_mutation(c);
}

// what a removal launch edits, as ring_view() is what a search reads; `seq`: the sequence number its last block publishes
RingEdit ring_edit(pct_cloud *c, uint32_t seq)
{
    return RingEdit{ c->R, c->x, c->y, c->z, (uint32_t)c->count, c->ring_ht, c->ring_slots, c->ring_ovf, c->ring_where, c->ring_st, c->d_rm_meet,
                     c->rm_word.w, seq };
}

// the tail of every removal behind its launches: the one host wait, `removed` handed out (removed_out may be null), the bookkeeping
int ring_remove_settle(pct_cloud *c, uint32_t seq, int64_t *removed_out)
{
    int64_t removed = 0, live = 0;
    PCTCHK(ring_remove_wait(c, seq, &removed, &live));
    if (removed_out) *removed_out = removed;
    return ring_remove_finish(c, removed, live);
}

// A one-pass removal of the rows `pred` names (ring_remove_kernel), whole: the caller has passed ring_remove_begin and queued what the
// predicate reads.  An empty window removes nothing and launches nothing.
template <typename Pred>
int ring_remove_run(pct_cloud *c, const Pred &pred, int64_t *removed_out)
{
    if (removed_out) *removed_out = 0;
    if (c->count == 0) return PCT_OK;
    PCTCHK(ring_remove_ensure(c));
    const uint32_t seq = c->rm_word.next();
    ring_remove_kernel<<<ceil_div(c->count, 256), 256, 0, g_stream>>>(ring_edit(c, seq), pred);
    HIPCHK(hipGetLastError());
    return ring_remove_settle(c, seq, removed_out);
}

}  // namespace

extern "C" {

int pct_cloud_ring_remove_ball(pct_cloud *c, const double centre[3], double r, int outside, int64_t *removed)
{
    if (!c || !centre) return fail(PCT_ERR_INVALID, "bad ring_remove_ball arguments");
    if (std::isnan(centre[0]) || std::isnan(centre[1]) || std::isnan(centre[2])) return fail(PCT_ERR_INVALID, "ring_remove_ball: the centre holds a NaN");
    PCTCHK(ring_remove_begin(c, "pct_cloud_ring_remove_ball"));
    RingRegion G{};
    for (int k = 0; k < 3; k++) G.a[k] = centre[k];
    G.r2 = r * r;                               // a negative r counts as |r|; a NaN r puts nothing inside
    G.kind = 0;
    G.outside = outside ? 1 : 0;
    return ring_remove_run(c, G, removed);
}

int pct_cloud_ring_remove_box(pct_cloud *c, const double lo[3], const double hi[3], int outside, int64_t *removed)
{
    if (!c || !lo || !hi) return fail(PCT_ERR_INVALID, "bad ring_remove_box arguments");
    for (int k = 0; k < 3; k++)
        if (std::isnan(lo[k]) || std::isnan(hi[k])) return fail(PCT_ERR_INVALID, "ring_remove_box: a corner holds a NaN");
    PCTCHK(ring_remove_begin(c, "pct_cloud_ring_remove_box"));
    RingRegion G{};
    for (int k = 0; k < 3; k++) { G.a[k] = lo[k]; G.b[k] = hi[k]; }
    G.kind = 1;
    G.outside = outside ? 1 : 0;
    return ring_remove_run(c, G, removed);
}

int pct_cloud_ring_remove_indices(pct_cloud *c, const uint32_t *idx, int64_t n, int64_t *removed_out)
{
    if (!c || n < 0 || (n > 0 && !idx)) return fail(PCT_ERR_INVALID, "bad ring_remove_indices arguments");
    if (removed_out) *removed_out = 0;
    PCTCHK(ring_remove_begin(c, "pct_cloud_ring_remove_indices"));
    if (n == 0) return PCT_OK;
    // the whole list is judged before anything is removed
    for (int64_t i = 0; i < n; i++)
        if ((int64_t)idx[i] < c->index_base || (int64_t)idx[i] >= c->index_base + c->count)
            return fail(PCT_ERR_INVALID, "ring_remove_indices: entry %lld = %u is outside [%lld, %lld)", (long long)i, idx[i], (long long)c->index_base,
                        (long long)(c->index_base + c->count));
    if (n > 0xFFFFFFF0ll) return fail(PCT_ERR_INVALID, "ring_remove_indices: the list is too long");
    PCTCHK(ring_remove_ensure(c));
    if ((size_t)n > c->d_rm_list.capacity()) {
        HIPCHK(hipStreamSynchronize(g_stream));
        PCTCHK(c->d_rm_list.reserve((size_t)n, pow2_at_least<size_t>(1024, (size_t)n)));
    }
    std::vector<uint32_t> slots;
    try { slots.resize((size_t)n); } catch (const std::bad_alloc &) { return fail(PCT_ERR_ALLOC, "host allocation failed"); }
    for (int64_t i = 0; i < n; i++) slots[(size_t)i] = idx[i] - (uint32_t)c->index_base;
    HIPCHK(hipMemcpyAsync(c->d_rm_list, slots.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, g_stream));
    const uint32_t seq = c->rm_word.next();
    ring_remove_list_kernel<<<ceil_div(n, 256), 256, 0, g_stream>>>(ring_edit(c, seq), c->d_rm_list, (uint32_t)n);
    ring_live_count_kernel<<<ceil_div(c->count, 256), 256, 0, g_stream>>>(ring_edit(c, seq));
    HIPCHK(hipGetLastError());
    return ring_remove_settle(c, seq, removed_out);             // (the list has left `slots` by its wait: the copy precedes the kernels)
}

// ---- removing outliers (ring_outlier.hpp) ----------------------------------------------------------------------------------------
}  // extern "C"

namespace {

// queue the judgement of the `newest` most recent rows (<= 0 or >= size: every row) on the window as it is: ro_counts[slot] =
// min(neighbours, target) for a judged row, PCT_NO_INDEX for every other slot below the size.  The window holds rows.  An r*r that
// overflows is held at DBL_MAX: every finite d2 is within it, and a d2 of +inf (a row with an infinite coordinate) never is.
int ring_outlier_judge(pct_cloud *c, double r, uint32_t target, int64_t newest)
{
    hipStream_t s = g_stream;
    if (c->ro_counts.capacity() < (size_t)c->cap) {
        HIPCHK(hipStreamSynchronize(s));
        PCTCHK(c->ro_counts.reserve((size_t)c->cap));
    }
    const RingScope S = ring_scope(c, newest);
    HIPCHK(hipMemsetAsync(c->ro_counts, 0xFF, sizeof(uint32_t) * (size_t)c->count, s));
    const int blocks = ceil_div(S.judged, (int64_t)kRoRows);
    const double r2 = std::min(r * r, std::numeric_limits<double>::max());
    PCTCHK(ring_work_begin(c));
    with_bool(c->count_work, [&](auto w) {
        ring_outlier_judge_kernel<decltype(w)::value><<<blocks, 256, 0, s>>>(ring_view(c), S.W, S.p0, c->x, c->y, c->z, r, r2, target, c->ro_counts,
                                                                             c->count_work ? c->d_work.get() : nullptr);
    });
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

}  // namespace

extern "C" {

int pct_cloud_ring_remove_outliers(pct_cloud *c, double r, int32_t min_neighbours, int64_t newest, int64_t *removed_out)
{
    if (!c) return fail(PCT_ERR_INVALID, "null cloud");
    if (!(std::isfinite(r) && r >= 0)) return fail(PCT_ERR_INVALID, "pct_cloud_ring_remove_outliers: r must be finite and >= 0");
    if (min_neighbours < 0) return fail(PCT_ERR_INVALID, "pct_cloud_ring_remove_outliers: min_neighbours must be >= 0");
    PCTCHK(ring_remove_begin(c, "pct_cloud_ring_remove_outliers"));
    if (removed_out) *removed_out = 0;
    if (min_neighbours == 0 || c->count == 0) return PCT_OK;
    PCTCHK(ring_outlier_judge(c, r, (uint32_t)min_neighbours, newest));
    return ring_remove_run(c, RoBelow{ c->ro_counts, (uint32_t)min_neighbours }, removed_out);
}

int pct_cloud_ring_neighbour_counts(pct_cloud *c, double r, int32_t count_cap, int64_t newest, uint32_t *counts, int64_t n)
{
    if (!c) return fail(PCT_ERR_INVALID, "null cloud");
    if (!(std::isfinite(r) && r >= 0)) return fail(PCT_ERR_INVALID, "pct_cloud_ring_neighbour_counts: r must be finite and >= 0");
    if (count_cap < 1) return fail(PCT_ERR_INVALID, "pct_cloud_ring_neighbour_counts: count_cap must be >= 1");
    PCTCHK(ring_remove_begin(c, "pct_cloud_ring_neighbour_counts"));
    if (n < c->count || (c->count > 0 && !counts))
        return fail(PCT_ERR_INVALID, "pct_cloud_ring_neighbour_counts: %lld counts for a window of %lld", (long long)n, (long long)c->count);
    if (c->count == 0) return PCT_OK;
    PCTCHK(ring_outlier_judge(c, r, (uint32_t)count_cap, newest));
    HIPCHK(hipMemcpyAsync(counts, c->ro_counts, sizeof(uint32_t) * (size_t)c->count, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return PCT_OK;
}

// ---- statistical outliers (ring_statistical.hpp) ---------------------------------------------------------------------------------
}  // extern "C"

namespace {

static_assert(sizeof(KsRecord) == sizeof(pct_knn_stats), "KsRecord is pct_knn_stats, field for field");

// rows of every level of the reduction tree over `n` values, kept one level behind the other
size_t ks_tree_rows(int64_t n)
{
    size_t rows = 0;
    int64_t m = n;
    do {
        m = (m + 255) / 256;
        rows += (size_t)m;
    } while (m > 1);
    return std::max<size_t>(rows, 1);
}

// the statistics of no measured row
pct_knn_stats ks_none()
{
    pct_knn_stats s{};
    s.mean = s.stddev = std::numeric_limits<double>::quiet_NaN();
    s.threshold = std::numeric_limits<double>::infinity();
    return s;
}

int ks_ensure(pct_cloud *c)
{
    if (c->ks_mean.capacity() < (size_t)c->cap || c->ks_part.capacity() < ks_tree_rows(c->cap)) {
        HIPCHK(hipStreamSynchronize(g_stream));
        PCTCHK(c->ks_mean.reserve((size_t)c->cap));
        PCTCHK(c->ks_part.reserve(ks_tree_rows(c->cap)));
    }
    if (!c->ks_rec) {
        PCTCHK(c->ks_rec.reset(1));
        PCTCHK(c->ks_rec_host.reset(1));
    }
    return PCT_OK;
}

// queue the judgement of the `newest` most recent rows (<= 0 or >= size: every row) on the window as it is: ks_mean[slot] = the mean
// distance to the k nearest other rows for a judged row (+inf: fewer than k candidates), NaN for every other slot below the size
// (all bits set is a NaN).  The window holds rows.
int ks_judge(pct_cloud *c, int k, int64_t newest)
{
    hipStream_t s = g_stream;
    const RingScope S = ring_scope(c, newest);
    HIPCHK(hipMemsetAsync(c->ks_mean, 0xFF, sizeof(double) * (size_t)c->count, s));
    const int blocks = ceil_div(S.judged, (int64_t)kKsRows);
    const bool work = c->count_work;
    PCTCHK(ring_work_begin(c));
    with_kcap(k, [&](auto kc) {
        with_bool(work, [&](auto w) {
            ring_knn_mean_kernel<decltype(kc)::value, decltype(w)::value><<<blocks, 256, 0, s>>>(ring_view(c), S.W, S.p0, c->x, c->y, c->z, k, c->ks_mean,
                                                                                                 work ? c->d_work.get() : nullptr);
        });
    });
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

// queue the tree reduction of ks_mean[0, size) and, in its last launch, the record
int ks_reduce(pct_cloud *c, double mult)
{
    hipStream_t s = g_stream;
    KsPart *out = c->ks_part;
    uint32_t m = (uint32_t)ceil_div(c->count, 256);
    ks_reduce_kernel<true><<<m, 256, 0, s>>>(c->ks_mean, nullptr, (uint32_t)c->count, out, mult, c->ks_rec, c->ks_rec_host);
    while (m > 1) {
        const KsPart *in = out;
        out += m;
        const uint32_t blocks = (uint32_t)ceil_div(m, 256);
        ks_reduce_kernel<false><<<blocks, 256, 0, s>>>(nullptr, in, m, out, mult, c->ks_rec, c->ks_rec_host);
        m = blocks;
    }
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

bool ks_bad_k(int32_t k) { return k < 1 || k > PCT_KNN_MAX_K; }

}  // namespace

extern "C" {

int pct_cloud_ring_knn_mean_distances(pct_cloud *c, int32_t k, int64_t newest, double *mean, int64_t n)
{
    if (!c) return fail(PCT_ERR_INVALID, "null cloud");
    if (ks_bad_k(k)) return fail(PCT_ERR_INVALID, "pct_cloud_ring_knn_mean_distances: k must be in 1 .. %d", PCT_KNN_MAX_K);
    if (!mean) return fail(PCT_ERR_INVALID, "pct_cloud_ring_knn_mean_distances: null output");
    PCTCHK(ring_remove_begin(c, "pct_cloud_ring_knn_mean_distances"));
    if (n < c->count)
        return fail(PCT_ERR_INVALID, "pct_cloud_ring_knn_mean_distances: %lld means for a window of %lld", (long long)n, (long long)c->count);
    if (c->count == 0) return PCT_OK;
    PCTCHK(ks_ensure(c));
    PCTCHK(ks_judge(c, k, newest));
    HIPCHK(hipMemcpyAsync(mean, c->ks_mean, sizeof(double) * (size_t)c->count, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return PCT_OK;
}

int pct_cloud_ring_knn_distance_stats(pct_cloud *c, int32_t k, double stddev_mult, int64_t newest, pct_knn_stats *stats)
{
    if (!c) return fail(PCT_ERR_INVALID, "null cloud");
    if (ks_bad_k(k)) return fail(PCT_ERR_INVALID, "pct_cloud_ring_knn_distance_stats: k must be in 1 .. %d", PCT_KNN_MAX_K);
    if (!std::isfinite(stddev_mult)) return fail(PCT_ERR_INVALID, "pct_cloud_ring_knn_distance_stats: stddev_mult must be finite");
    if (!stats) return fail(PCT_ERR_INVALID, "pct_cloud_ring_knn_distance_stats: null output");
    PCTCHK(ring_remove_begin(c, "pct_cloud_ring_knn_distance_stats"));
    *stats = ks_none();
    if (c->count == 0) return PCT_OK;
    PCTCHK(ks_ensure(c));
    PCTCHK(ks_judge(c, k, newest));
    PCTCHK(ks_reduce(c, stddev_mult));
    HIPCHK(hipStreamSynchronize(g_stream));
    std::memcpy(stats, c->ks_rec_host.host(), sizeof *stats);
    return PCT_OK;
}

int pct_cloud_ring_remove_statistical(pct_cloud *c, int32_t k, double stddev_mult, int64_t newest, int64_t *removed_out, pct_knn_stats *stats)
{
    if (!c) return fail(PCT_ERR_INVALID, "null cloud");
    if (ks_bad_k(k)) return fail(PCT_ERR_INVALID, "pct_cloud_ring_remove_statistical: k must be in 1 .. %d", PCT_KNN_MAX_K);
    if (!std::isfinite(stddev_mult)) return fail(PCT_ERR_INVALID, "pct_cloud_ring_remove_statistical: stddev_mult must be finite");
    PCTCHK(ring_remove_begin(c, "pct_cloud_ring_remove_statistical"));
    if (removed_out) *removed_out = 0;
    if (stats) *stats = ks_none();
    if (c->count == 0) return PCT_OK;
    PCTCHK(ks_ensure(c));
    PCTCHK(ks_judge(c, k, newest));
    PCTCHK(ks_reduce(c, stddev_mult));
    // the record's host-mapped copy was written by a launch that finished before the removal's began: it is there behind the wait
    const int st = ring_remove_run(c, KsAbove{ c->ks_mean, c->ks_rec }, removed_out);
    if (stats && st == PCT_OK) std::memcpy(stats, c->ks_rec_host.host(), sizeof *stats);
    return st;
}

int pct_cloud_ring_remove_isolated(pct_cloud *c, int32_t k, double max_mean_distance, int64_t newest, int64_t *removed_out)
{
    if (!c) return fail(PCT_ERR_INVALID, "null cloud");
    if (ks_bad_k(k)) return fail(PCT_ERR_INVALID, "pct_cloud_ring_remove_isolated: k must be in 1 .. %d", PCT_KNN_MAX_K);
    if (!(max_mean_distance >= 0)) return fail(PCT_ERR_INVALID, "pct_cloud_ring_remove_isolated: max_mean_distance must be >= 0 (+inf allowed)");
    PCTCHK(ring_remove_begin(c, "pct_cloud_ring_remove_isolated"));
    if (removed_out) *removed_out = 0;
    if (c->count == 0 || std::isinf(max_mean_distance)) return PCT_OK;          // no mean is greater than +inf: nothing to launch
    PCTCHK(ks_ensure(c));
    PCTCHK(ks_judge(c, k, newest));
    ks_set_threshold_kernel<<<1, 1, 0, g_stream>>>(c->ks_rec, max_mean_distance);
    return ring_remove_run(c, KsAbove{ c->ks_mean, c->ks_rec }, removed_out);
}

int pct_cloud_ring_live(pct_cloud *c, int64_t *live_out, int64_t *not_live)
{
    if (!c || !live_out || !not_live) return fail(PCT_ERR_INVALID, "bad ring_live arguments");
    *live_out = *not_live = 0;
    PCTCHK(ring_remove_begin(c, "pct_cloud_ring_live"));
    if (c->count == 0) return PCT_OK;
    PCTCHK(ring_remove_ensure(c));
    const uint32_t seq = c->rm_word.next();
    ring_live_count_kernel<<<ceil_div(c->count, 256), 256, 0, g_stream>>>(ring_edit(c, seq));
    HIPCHK(hipGetLastError());
    int64_t removed = 0, live = 0;
    PCTCHK(ring_remove_wait(c, seq, &removed, &live));
    *live_out = live;
    *not_live = c->count - live;
    return PCT_OK;
}

int pct_cloud_ring_compact(pct_cloud *c, int64_t *live, int64_t *reclaimed, uint32_t *remap, int64_t remap_cap)
{
    if (!c) return fail(PCT_ERR_INVALID, "null cloud");
    PCTCHK(ring_remove_begin(c, "pct_cloud_ring_compact"));
    if (remap && remap_cap < c->count) return fail(PCT_ERR_INVALID, "pct_cloud_ring_compact: a remap of %lld entries for a window of %lld", (long long)remap_cap, (long long)c->count);
    if (live) *live = 0;
    if (reclaimed) *reclaimed = 0;
    if (c->count == 0) return PCT_OK;
    const int64_t n = c->count;
    int64_t L = 0;
    PCTCHK(ring_compact_run(c, -1, &L, remap));
    if (live) *live = L;
    if (reclaimed) *reclaimed = n - L;
    return PCT_OK;
}

int pct_cloud_ring_autocompact(pct_cloud *c, double dead_fraction)
{
    if (!c) return fail(PCT_ERR_INVALID, "null cloud");
    if (!(dead_fraction >= 0 && dead_fraction <= 1)) return fail(PCT_ERR_INVALID, "the dead fraction of auto-compaction must lie in [0, 1]");
    if (dead_fraction == 0) { c->rc_fraction = 0.0; return PCT_OK; }
    if (!c->ring_on) return fail(PCT_ERR_INVALID, "auto-compaction needs the rolling-map index (pct_cloud_ring_index)");
    c->rc_fraction = dead_fraction;
    return PCT_OK;
}

int pct_cloud_ring_compact_count(const pct_cloud *c, uint64_t *compactions)
{
    if (!c || !compactions) return fail(PCT_ERR_INVALID, "bad ring_compact_count arguments");
    *compactions = c->rc_count;
    return PCT_OK;
}

}  // extern "C"

// ---- depth images on the rolling map (ring_depth.hpp) ----------------------------------------------------------------------------
namespace {

// what the three depth entry points refuse in a view (pct_engine.h)
int depth_view_check(const pct_depth_view *v, const char *what)
{
    if (!v) return fail(PCT_ERR_INVALID, "%s: null view", what);
    if (v->width < 1 || v->height < 1 || (int64_t)v->width * (int64_t)v->height > (1ll << 24))
        return fail(PCT_ERR_INVALID, "%s: bad image size %d x %d (at most 2^24 pixels)", what, v->width, v->height);
    if (!(std::isfinite(v->focal) && v->focal > 0) || !(std::isfinite(v->near_z) && v->near_z > 0))
        return fail(PCT_ERR_INVALID, "%s: focal and near_z must be finite and > 0", what);
    for (int k = 0; k < 3; k++) if (!std::isfinite(v->t[k])) return fail(PCT_ERR_INVALID, "%s: the camera position is not finite", what);
    for (int k = 0; k < 9; k++) if (!std::isfinite(v->R[k])) return fail(PCT_ERR_INVALID, "%s: the camera rotation is not finite", what);
    if (v->metric != PCT_DEPTH_Z && v->metric != PCT_DEPTH_RANGE) return fail(PCT_ERR_INVALID, "%s: unknown depth metric %d", what, v->metric);
    if (v->reserved != 0) return fail(PCT_ERR_INVALID, "%s: the reserved field must be 0", what);
    return PCT_OK;
}

int depth_stage_image(DepthStage *S, const float *image, size_t off, size_t npix)
{
    std::memcpy(S->h + off, image, sizeof(float) * npix);
    HIPCHK(hipMemcpyAsync(S->d + off, S->h + off, sizeof(float) * npix, hipMemcpyHostToDevice, g_stream));
    return PCT_OK;
}

int depth_stage_ensure(DepthStage *S, size_t floats)
{
    if (floats <= S->cap) return PCT_OK;
    HIPCHK(hipStreamSynchronize(g_stream));
    const size_t cap = pow2_at_least((size_t)1 << 14, floats);
    return regrow(S->cap, cap, part(S->h, cap), part(S->d, cap));
}

// scratch of pct_cloud_append_depth for an image of npix pixels (grow-only): validity flags, ranks, tile totals, the packed frame
int depth_scratch_ensure(pct_cloud *c, int64_t npix)
{
    PCTCHK(c->dd_word.ensure(4));
    if (npix <= c->dp.ncap) return PCT_OK;
    HIPCHK(hipStreamSynchronize(g_stream));       // the previous append's insert kernel may still be reading the packed frame
    return c->dp.ensure(pow2_at_least<int64_t>(4096, npix));
}

// pct_depth_classify and pct_range_classify have no cloud to keep their buffers in: one grow-only set for the process, used under a lock
struct DepthClassifyWork {
    std::mutex lock;
    DepthStage images;
    RangeStage tables;                           // pct_range_classify: the edge tables of every view
    DevBuf<double> d_pts;
    DevBuf<int32_t> d_seen, d_pixel;
    int64_t ncap = 0;
};
DepthClassifyWork &g_depth_work = *new DepthClassifyWork();      // never destroyed: the HIP runtime may be gone by then

// the cloud's image staging: copy `image` in and hand back where the kernels read it
int depth_cloud_image(pct_cloud *c, size_t npix, const float *image, const float **d_image)
{
    PCTCHK(depth_stage_ensure(&c->dp_img, npix));
    PCTCHK(depth_stage_image(&c->dp_img, image, 0, npix));
    *d_image = c->dp_img.d;
    return PCT_OK;
}

// The tail of pct_cloud_append_depth / pct_cloud_append_range behind their un-projection kernels: the FIRST host wait (the valid
// count of launch `seq`), the capacity test, then pct_cloud_append_aos of the n un-projected points, their source being the packed
// device frame c->dp.out
int image_frame_append(pct_cloud *c, uint32_t seq, int64_t npix, const char *kind, int64_t *offered, int64_t *kept)
{
    int64_t n = 0;
    PCTCHK(dd_scan_wait(c, seq, &n));
    if (n > npix) return fail(PCT_ERR_INTERNAL, "the %s un-projection counted %lld valid pixels of %lld", kind, (long long)n, (long long)npix);
    if (n > c->cap) return fail(PCT_ERR_CAPACITY, "appending %lld valid pixels to a ring of %lld", (long long)n, (long long)c->cap);
    *offered = n;
    const unsigned char *d_frame = reinterpret_cast<const unsigned char *>(c->dp.out.get());
    if (c->dd_res > 0) {
        PCTCHK(ring_append_dedup(c, nullptr, n, 12, d_frame));          // the SECOND host wait: the survivor count
        *kept = c->dd_last_kept;
        return PCT_OK;
    }
    *kept = n;
    if (n == 0) return PCT_OK;
    drop_grid(c);
    if (c->ring_ready) return ring_append(c, nullptr, n, 12, d_frame);
    return append_unindexed_dev(c, c->dp.out, n);
}

}  // namespace

extern "C" {

int pct_cloud_ring_carve_depth(pct_cloud *c, const pct_depth_view *v, const float *image, double margin, int64_t *removed_out)
{
    if (!c || !image || !removed_out) return fail(PCT_ERR_INVALID, "bad ring_carve_depth arguments");
    PCTCHK(depth_view_check(v, "pct_cloud_ring_carve_depth"));
    if (std::isnan(margin)) return fail(PCT_ERR_INVALID, "pct_cloud_ring_carve_depth: the margin is a NaN");
    PCTCHK(ring_remove_begin(c, "pct_cloud_ring_carve_depth"));
    *removed_out = 0;
    if (c->count == 0) return PCT_OK;
    const float *d_image = nullptr;
    PCTCHK(depth_cloud_image(c, (size_t)v->width * (size_t)v->height, image, &d_image));
    return ring_remove_run(c, DepthSeenThrough{ *v, d_image, margin }, removed_out);
}

int pct_cloud_append_depth(pct_cloud *c, const pct_depth_view *v, const float *image, double max_depth, int64_t *offered, int64_t *kept)
{
    if (!c || !image || !offered || !kept) return fail(PCT_ERR_INVALID, "bad append_depth arguments");
    PCTCHK(depth_view_check(v, "pct_cloud_append_depth"));
    if (std::isnan(max_depth)) return fail(PCT_ERR_INVALID, "pct_cloud_append_depth: max_depth is a NaN");
    if (v->metric != PCT_DEPTH_Z) return fail(PCT_ERR_INVALID, "pct_cloud_append_depth: only z-depth images are un-projected (PCT_DEPTH_Z)");
    if (!c->ring_on) return fail(PCT_ERR_INVALID, "pct_cloud_append_depth needs the rolling-map index (pct_cloud_ring_index)");
    hipStream_t s = g_stream;
    PCTCHK(ring_finish_pending(c));             // the previous frame's insert kernel has read the packed frame below
    *offered = *kept = 0;
    const int64_t npix = (int64_t)v->width * (int64_t)v->height;
    PCTCHK(depth_scratch_ensure(c, npix));
    const float *d_image = nullptr;
    PCTCHK(depth_cloud_image(c, (size_t)npix, image, &d_image));
    // flags of the valid pixels, their ranks in row-major order, and the FIRST host wait: the valid count -- the capacity test, the
    // slots the append takes and the filter's table size all need it before anything is queued that changes the window
    const uint32_t un = (uint32_t)npix, seq = c->dd_word.next();
    const int ntiles = ceil_div(npix, kDdTile);
    depth_valid_kernel<<<ceil_div(npix, 256), 256, 0, s>>>(*v, d_image, un, max_depth, c->dp.flags);
    dd_rank_kernel<<<ntiles, 256, 0, s>>>(c->dp.flags, un, c->dp.rank, c->dp.tile);
    scan_tile_sums_kernel<uint32_t><<<1, 256, 0, s>>>(c->dp.tile, (uint32_t)ntiles, DdPublish{ c->dd_word.w, seq });
    depth_unproject_kernel<<<ceil_div(npix, 256), 256, 0, s>>>(*v, d_image, un, c->dp.flags, c->dp.rank, c->dp.tile, c->dp.out);
    HIPCHK(hipGetLastError());
    return image_frame_append(c, seq, npix, "depth", offered, kept);
}

int pct_depth_classify(const pct_depth_view *views, const float *const *images, int32_t n_views, const double *pts, int64_t n, double margin,
                       int32_t *seen_by, int32_t *pixel)
{
    if (!views || !images || n_views < 1 || n_views > kDepthMaxViews || n < 0 || !pts || !seen_by || n > 0xFFFFFFF0ll)
        return fail(PCT_ERR_INVALID, "bad depth_classify arguments (1 <= n_views <= %d)", kDepthMaxViews);
    if (std::isnan(margin)) return fail(PCT_ERR_INVALID, "pct_depth_classify: the margin is a NaN");
    size_t total = 0;
    for (int k = 0; k < n_views; k++) {
        if (!images[k]) return fail(PCT_ERR_INVALID, "pct_depth_classify: image %d is NULL", k);
        PCTCHK(depth_view_check(&views[k], "pct_depth_classify"));
        total += (size_t)views[k].width * (size_t)views[k].height;
    }
    if (n == 0) return PCT_OK;
    PCTCHK(require_init());
    DepthClassifyWork &W = g_depth_work;
    std::lock_guard<std::mutex> guard(W.lock);
    PCTCHK(depth_stage_ensure(&W.images, total));
    if (n > W.ncap) {
        HIPCHK(hipStreamSynchronize(g_stream));
        const int64_t cap = pow2_at_least<int64_t>(1024, n);
        PCTCHK(regrow(W.ncap, cap, part(W.d_pts, 3 * (size_t)cap), part(W.d_seen, (size_t)cap), part(W.d_pixel, 2 * (size_t)cap)));
    }
    DepthViews S{};
    S.n = n_views;
    size_t off = 0;
    for (int k = 0; k < n_views; k++) {
        const size_t npix = (size_t)views[k].width * (size_t)views[k].height;
        S.v[k] = views[k];
        S.image[k] = W.images.d + off;
        PCTCHK(depth_stage_image(&W.images, images[k], off, npix));
        off += npix;
    }
    HIPCHK(hipMemcpyAsync(W.d_pts, pts, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, g_stream));
    depth_classify_kernel<<<ceil_div(n, 256), 256, 0, g_stream>>>(S, W.d_pts, (uint32_t)n, margin, W.d_seen, pixel ? W.d_pixel : nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(seen_by, W.d_seen, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, g_stream));
    if (pixel) HIPCHK(hipMemcpyAsync(pixel, W.d_pixel, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return PCT_OK;
}

}  // extern "C"

// ---- range images on the rolling map (ring_range.hpp) ----------------------------------------------------------------------------
namespace {

// finite and strictly ascending (a NaN fails both comparisons' sense: it is not finite)
bool range_edges_ok(const double *e, int n)
{
    for (int k = 0; k <= n; k++) {
        if (!std::isfinite(e[k])) return false;
        if (k > 0 && !(e[k - 1] < e[k])) return false;
    }
    return true;
}

// what the three range entry points refuse in a view (pct_engine.h); dirs: the call un-projects and needs both direction tables
int range_view_check(const pct_range_view *v, const char *what, bool dirs)
{
    if (!v) return fail(PCT_ERR_INVALID, "%s: null view", what);
    if (v->width < 1 || v->width > kRangeMaxWidth || v->height < 1 || v->height > kRangeMaxHeight || (int64_t)v->width * (int64_t)v->height > (1ll << 24))
        return fail(PCT_ERR_INVALID, "%s: bad scan size %d x %d (1..%d columns, 1..%d rows)", what, v->width, v->height, kRangeMaxWidth, kRangeMaxHeight);
    if (!(std::isfinite(v->near_range) && v->near_range > 0)) return fail(PCT_ERR_INVALID, "%s: near_range must be finite and > 0", what);
    for (int k = 0; k < 3; k++) if (!std::isfinite(v->t[k])) return fail(PCT_ERR_INVALID, "%s: the sensor position is not finite", what);
    for (int k = 0; k < 9; k++) if (!std::isfinite(v->R[k])) return fail(PCT_ERR_INVALID, "%s: the sensor rotation is not finite", what);
    if (v->reserved[0] != 0 || v->reserved[1] != 0) return fail(PCT_ERR_INVALID, "%s: the reserved fields must be 0", what);
    if (!v->col_edge || !v->row_edge) return fail(PCT_ERR_INVALID, "%s: a null edge table", what);
    if (!range_edges_ok(v->col_edge, v->width) || !(v->col_edge[0] >= 0.0 && v->col_edge[v->width] <= 4.0))
        return fail(PCT_ERR_INVALID, "%s: col_edge must be finite, strictly ascending and inside [0, 4]", what);
    if (!range_edges_ok(v->row_edge, v->height)) return fail(PCT_ERR_INVALID, "%s: row_edge must be finite and strictly ascending", what);
    if (dirs) {
        if (!v->col_dir || !v->row_dir) return fail(PCT_ERR_INVALID, "%s: a null direction table", what);
        for (int k = 0; k < 2 * v->width; k++) if (!std::isfinite(v->col_dir[k])) return fail(PCT_ERR_INVALID, "%s: col_dir is not finite", what);
        for (int k = 0; k < 2 * v->height; k++) if (!std::isfinite(v->row_dir[k])) return fail(PCT_ERR_INVALID, "%s: row_dir is not finite", what);
    }
    return PCT_OK;
}

size_t range_table_doubles(const pct_range_view *v, bool dirs)
{
    return (size_t)(v->width + 1) + (size_t)(v->height + 1) + (dirs ? 2 * (size_t)v->width + 2 * (size_t)v->height : 0);
}

int range_stage_ensure(RangeStage *S, size_t doubles)
{
    if (doubles <= S->cap) return PCT_OK;
    HIPCHK(hipStreamSynchronize(g_stream));
    const size_t cap = pow2_at_least((size_t)1 << 12, doubles);
    return regrow(S->cap, cap, part(S->h, cap), part(S->d, cap));
}

// Copy a checked view's tables into the stage at `off` (room ensured by the caller) and hand back the view as the kernels take it;
// dirs != nullptr: the two direction tables too, dirs[0] = col_dir, dirs[1] = row_dir on the device.  The caller's tables are its
// own again when this returns.
int range_tables_stage(RangeStage *S, const pct_range_view *v, size_t off, RangeViewDev *out, const double **dirs)
{
    const size_t nc = (size_t)v->width + 1, nr = (size_t)v->height + 1;
    double *h = S->h + off;
    std::memcpy(h, v->col_edge, sizeof(double) * nc);
    std::memcpy(h + nc, v->row_edge, sizeof(double) * nr);
    if (dirs) {
        std::memcpy(h + nc + nr, v->col_dir, sizeof(double) * 2 * (size_t)v->width);
        std::memcpy(h + nc + nr + 2 * (size_t)v->width, v->row_dir, sizeof(double) * 2 * (size_t)v->height);
    }
    const size_t total = range_table_doubles(v, dirs != nullptr);
    HIPCHK(hipMemcpyAsync(S->d + off, h, sizeof(double) * total, hipMemcpyHostToDevice, g_stream));
    for (int k = 0; k < 3; k++) out->t[k] = v->t[k];
    for (int k = 0; k < 9; k++) out->R[k] = v->R[k];
    out->near_range = v->near_range;
    out->width = v->width; out->height = v->height;
    const double *d = S->d + off;
    out->col_edge = d; out->row_edge = d + nc;
    if (dirs) { dirs[0] = d + nc + nr; dirs[1] = d + nc + nr + 2 * (size_t)v->width; }
    return PCT_OK;
}

}  // namespace

extern "C" {

double pct_range_pseudo_angle(double x, double y) { return range_pseudo_angle(x, y); }

int pct_cloud_ring_carve_range(pct_cloud *c, const pct_range_view *v, const float *image, double margin, int64_t *removed_out)
{
    if (!c || !image || !removed_out) return fail(PCT_ERR_INVALID, "bad ring_carve_range arguments");
    PCTCHK(range_view_check(v, "pct_cloud_ring_carve_range", false));
    if (std::isnan(margin)) return fail(PCT_ERR_INVALID, "pct_cloud_ring_carve_range: the margin is a NaN");
    PCTCHK(ring_remove_begin(c, "pct_cloud_ring_carve_range"));
    *removed_out = 0;
    if (c->count == 0) return PCT_OK;
    RangeViewDev V;
    PCTCHK(range_stage_ensure(&c->rg_tab, range_table_doubles(v, false)));
    PCTCHK(range_tables_stage(&c->rg_tab, v, 0, &V, nullptr));
    const float *d_image = nullptr;
    PCTCHK(depth_cloud_image(c, (size_t)v->width * (size_t)v->height, image, &d_image));
    return ring_remove_run(c, RangeSeenThrough{ V, d_image, margin }, removed_out);
}

int pct_cloud_append_range(pct_cloud *c, const pct_range_view *v, const float *image, double max_range, int64_t *offered, int64_t *kept)
{
    if (!c || !image || !offered || !kept) return fail(PCT_ERR_INVALID, "bad append_range arguments");
    PCTCHK(range_view_check(v, "pct_cloud_append_range", true));
    if (std::isnan(max_range)) return fail(PCT_ERR_INVALID, "pct_cloud_append_range: max_range is a NaN");
    if (!c->ring_on) return fail(PCT_ERR_INVALID, "pct_cloud_append_range needs the rolling-map index (pct_cloud_ring_index)");
    hipStream_t s = g_stream;
    PCTCHK(ring_finish_pending(c));             // the previous frame's insert kernel has read the packed frame below
    *offered = *kept = 0;
    const int64_t npix = (int64_t)v->width * (int64_t)v->height;
    PCTCHK(depth_scratch_ensure(c, npix));
    RangeViewDev V;
    const double *dirs[2] = { nullptr, nullptr };
    PCTCHK(range_stage_ensure(&c->rg_tab, range_table_doubles(v, true)));
    PCTCHK(range_tables_stage(&c->rg_tab, v, 0, &V, dirs));
    const float *d_image = nullptr;
    PCTCHK(depth_cloud_image(c, (size_t)npix, image, &d_image));
    // as pct_cloud_append_depth: flags of the valid pixels, their ranks in row-major order, the un-projection into the packed frame
    const uint32_t un = (uint32_t)npix, seq = c->dd_word.next();
    const int ntiles = ceil_div(npix, kDdTile);
    range_valid_kernel<<<ceil_div(npix, 256), 256, 0, s>>>(V.near_range, d_image, un, max_range, c->dp.flags);
    dd_rank_kernel<<<ntiles, 256, 0, s>>>(c->dp.flags, un, c->dp.rank, c->dp.tile);
    scan_tile_sums_kernel<uint32_t><<<1, 256, 0, s>>>(c->dp.tile, (uint32_t)ntiles, DdPublish{ c->dd_word.w, seq });
    range_unproject_kernel<<<ceil_div(npix, 256), 256, 0, s>>>(V, dirs[0], dirs[1], d_image, un, c->dp.flags, c->dp.rank, c->dp.tile, c->dp.out);
    HIPCHK(hipGetLastError());
    return image_frame_append(c, seq, npix, "range", offered, kept);
}

int pct_range_classify(const pct_range_view *views, const float *const *images, int32_t n_views, const double *pts, int64_t n, double margin,
                       int32_t *seen_by, int32_t *pixel)
{
    if (!views || !images || n_views < 1 || n_views > kRangeMaxViews || n < 0 || !pts || !seen_by || n > 0xFFFFFFF0ll)
        return fail(PCT_ERR_INVALID, "bad range_classify arguments (1 <= n_views <= %d)", kRangeMaxViews);
    if (std::isnan(margin)) return fail(PCT_ERR_INVALID, "pct_range_classify: the margin is a NaN");
    size_t total = 0, tables = 0;
    for (int k = 0; k < n_views; k++) {
        if (!images[k]) return fail(PCT_ERR_INVALID, "pct_range_classify: image %d is NULL", k);
        PCTCHK(range_view_check(&views[k], "pct_range_classify", false));
        total += (size_t)views[k].width * (size_t)views[k].height;
        tables += range_table_doubles(&views[k], false);
    }
    if (n == 0) return PCT_OK;
    PCTCHK(require_init());
    DepthClassifyWork &W = g_depth_work;
    std::lock_guard<std::mutex> guard(W.lock);
    PCTCHK(depth_stage_ensure(&W.images, total));
    PCTCHK(range_stage_ensure(&W.tables, tables));
    if (n > W.ncap) {
        HIPCHK(hipStreamSynchronize(g_stream));
        const int64_t cap = pow2_at_least<int64_t>(1024, n);
        PCTCHK(regrow(W.ncap, cap, part(W.d_pts, 3 * (size_t)cap), part(W.d_seen, (size_t)cap), part(W.d_pixel, 2 * (size_t)cap)));
    }
    RangeViews S{};
    S.n = n_views;
    size_t off = 0, toff = 0;
    for (int k = 0; k < n_views; k++) {
        const size_t npix = (size_t)views[k].width * (size_t)views[k].height;
        PCTCHK(range_tables_stage(&W.tables, &views[k], toff, &S.v[k], nullptr));
        S.image[k] = W.images.d + off;
        PCTCHK(depth_stage_image(&W.images, images[k], off, npix));
        off += npix;
        toff += range_table_doubles(&views[k], false);
    }
    HIPCHK(hipMemcpyAsync(W.d_pts, pts, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, g_stream));
    range_classify_kernel<<<ceil_div(n, 256), 256, 0, g_stream>>>(S, W.d_pts, (uint32_t)n, margin, W.d_seen, pixel ? W.d_pixel : nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(seen_by, W.d_seen, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, g_stream));
    if (pixel) HIPCHK(hipMemcpyAsync(pixel, W.d_pixel, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return PCT_OK;
}

}  // extern "C"
