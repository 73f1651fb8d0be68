// engine.hip -- host side of libpct_engine.so: the C ABI of include/pct_engine.h over the
// gfx950 kernels in kernels.hpp.  One process drives one GPU (pct_init selects it); all work
// is queued on one library-owned HIP stream unless a caller passes its own (the *_dev entry
// points), so copies and kernels of a batch stay ordered without host synchronisation.
//
// Data layout in HBM per cloud:
//   x[cap4], y[cap4], z[cap4]   fp32 SoA, insertion order (cap4 = capacity rounded up to 4)
//   sorted[n]                   float4 {x, y, z, bitcast(original index)} in cell order   (grid only)
//   cell_start[ncells + 1]      u32 exclusive prefix of per-cell counts                   (grid only)
//   query workspaces sized by pct_cloud_reserve_queries
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/pct_engine.h"
#include "engine_internal.hpp"
#include "kernels.hpp"
#include "gridbuild.hpp"
#include "pyramid.hpp"
#include "ring.hpp"
#include "ring_dedup.hpp"
#include "ring_remove.hpp"
#include "ring_compact.hpp"
#include "ring_depth.hpp"
#include "ring_range.hpp"
#include "ring_outlier.hpp"
#include "ring_statistical.hpp"
#include "brute2.hpp"
#include "knn.hpp"
#include "rsearch.hpp"
#include "ring_search.hpp"
#include "bezier_batch.hpp"
#include "segment.hpp"
#include "segment_search.hpp"
#include "segment_polyhedron.hpp"
#include "bezier_certify.hpp"
#include "bezier_clearance.hpp"

using namespace pct;
using pct_host::dropped;
using pct_host::part;
using pct_host::pow2_at_least;
using pct_host::regrow;
using pct_internal::DevBuf;
using pct_internal::MappedBuf;
using pct_internal::PinnedBuf;

namespace {

thread_local char g_err[512] = "";
hipStream_t g_stream = nullptr;
int g_device = -1;

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return fail(PCT_ERR_HIP, "%s -> %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define PCTCHK(call)                    \
    do {                                \
        int s_ = (call);                \
        if (s_ != PCT_OK) return s_;    \
    } while (0)

constexpr int kMaxParts = 2048;       // streaming kernel: at most 8 blocks of 256 per CU
constexpr int64_t kPartQueries = 16384;   // the partial buffers hold this many queries (400 MB); a 1 M-query reservation used to
                                          // take 26 GB of HBM for them
constexpr int kBezierCapMax = 4096;

inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// ---- run-time value -> template parameter --------------------------------------------------------------------------------------
// f receives the value as a std::integral_constant and names the kernel instance with it: one argument list per call site
template <typename F>
void with_bool(bool b, F f)
{
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// list capacity of the k-NN kernels (knn.hpp): the smallest of 8 / 16 / 32 / 64 that holds k
template <typename F>
void with_kcap(int k, F f)
{
    if (k <= 8) f(std::integral_constant<int, 8>{});
    else if (k <= 16) f(std::integral_constant<int, 16>{});
    else if (k <= 32) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 64>{});
}

// the streaming kernels take a batch in tiles of 8 / 4 / 2 / 1 queries: f(tile size as a constant, first query, queries in the tile)
template <typename F>
void for_each_query_tile(int64_t Q, F f)
{
    for (int64_t q0 = 0; q0 < Q;) {
        const int64_t left = Q - q0;
        if (left >= 8) { f(std::integral_constant<int, 8>{}, (int)q0, 8); q0 += 8; }
        else if (left > 2) { const int n = (int)std::min<int64_t>(4, left); f(std::integral_constant<int, 4>{}, (int)q0, n); q0 += n; }
        else if (left == 2) { f(std::integral_constant<int, 2>{}, (int)q0, 2); q0 += 2; }
        else { f(std::integral_constant<int, 1>{}, (int)q0, 1); q0 += 1; }
    }
}

constexpr int kExpressMaxQ = 1024;        // queries per express (block-per-query) launch
constexpr int64_t kMappedMaxQ = 65536;    // host-buffer batches up to this size travel through host-mapped memory, larger ones by DMA
constexpr int64_t kSmallNNMax = 16384;    // clouds up to this size answer single queries with one-block kernels
constexpr uint32_t kExpressIdsCap = 1u << 16;

bool poll_results()
{
    static const bool v = [] { const char *e = std::getenv("PCT_POLL_RESULTS"); return e ? std::atoi(e) != 0 : true; }();
    return v;
}

int sync_library_stream()
{
    HIPCHK(hipStreamSynchronize(g_stream));
    return PCT_OK;
}

// A {sequence, results...} completion word in host-mapped memory: the last block of a launch stores the launch's number into [0]
// behind its results, and the host polls it (a stream synchronise costs ~20 us of host time more), falling back to the stream after
// ~2 s of spinning or when polling is off.
struct SeqWord {
    MappedBuf<uint32_t> w;
    uint32_t seq = 0;                            // the number of the last launch handed one
    int ensure(size_t words)
    {
        if (w) return PCT_OK;
        PCTCHK(w.reset(words));
        for (size_t k = 0; k < words; k++) w.host()[k] = 0;
        return PCT_OK;
    }
    uint32_t next() { return ++seq; }
    // what: the launch stores its word whether polling is on or off, so a word that still differs behind the stream is an error
    // named after it; nullptr: the launch is handed no word when polling is off, and the stream is the whole wait
    int wait(uint32_t want, const char *what)
    {
        int st = PCT_OK;
        const bool seen = pct_host::wait_word(w.host(), want, poll_results() ? 200000000l : 0l, [&] { st = sync_library_stream(); });
        PCTCHK(st);
        if (!seen && what) return fail(PCT_ERR_HIP, "%s finished without its sequence word (%u != %u)", what, w.host()[0], want);
        return PCT_OK;
    }
};

// Scratch of one order-preserving compaction of a frame (ring_dedup.hpp dd_rank, the tile scan with DdPublish, and a compacting kernel): keep flags,
// ranks, tile totals and the packed xyz rows the insert kernel then reads.  ensure() allocates for exactly `cap` points, and with them
// whatever further parts the caller sizes by ncap (one group); the caller has chosen cap and synchronised.
struct CompactScratch {
    DevBuf<uint8_t> flags;
    DevBuf<uint32_t> rank, tile;
    DevBuf<float> out;
    int64_t ncap = 0;                            // points the scratch holds
    template <typename... More>
    int ensure(int64_t cap, More... more)
    {
        return regrow(ncap, cap, part(flags, (size_t)cap), part(rank, (size_t)cap), part(tile, (size_t)ceil_div(cap, kDdTile)), part(out, 3 * (size_t)cap), more...);
    }
};

// An image on its way to the device: the caller's floats are copied into pinned memory the library owns and from there to a device
// buffer on the library's stream (both grow-only), so the caller's buffer is its own again at once and the kernels gather from HBM
// / L2, not across the bus.  Every user waits for a kernel behind the copy before it returns: the pinned buffer is free by then.
struct DepthStage {
    PinnedBuf<float> h;
    DevBuf<float> d;
    size_t cap = 0;                              // floats
};

// The tables of a range view on the same way (ring_range.hpp): col_edge, row_edge and, for an append, col_dir and row_dir, one
// behind the other.  The same rule frees the pinned copy: every user waits for a kernel behind the copy before it returns.
struct RangeStage {
    PinnedBuf<double> h;
    DevBuf<double> d;
    size_t cap = 0;                              // doubles
};

}  // namespace

struct ReplanCtx;

// The cloud-owned lists of a host-form list search's last result: idx, d2 and (capsule search) s, grow-only, valid until the next
// search that writes them or until the cloud or its index changes.  `what` names the search in the messages.
struct ListStore {
    const char *what;
    DevBuf<uint32_t> idx;
    DevBuf<double> d2, s;
    size_t cap = 0;
    int64_t total = 0;
    bool valid = false;
};

struct pct_cloud {
    int64_t cap = 0, cap4 = 0, count = 0, ring_next = 0;
    int64_t index_base = 0;
    // coordinates: views of xyz_dev, or of xyz_map on "small" clouds, which keep them in host-mapped memory (kernels read them over
    // the bus; the host appends with plain stores through hx / hy / hz and no launch) -- the RRT* node sets of the kd_* drop-in
    float *x = nullptr, *y = nullptr, *z = nullptr;
    bool host_mapped = false;
    float *hx = nullptr, *hy = nullptr, *hz = nullptr;
    DevBuf<float> xyz_dev[3];
    MappedBuf<float> xyz_map[3];
    DevBuf<float4> gb_tmp;                      // index build scratch (gridbuild.hpp): slab-ordered records, kept between builds
    DevBuf<uint32_t> gb_small;                  // per-block slab table + slab totals / cursors / starts
    // express path: host-mapped result / argument / id buffers
    MappedBuf<ExpressOut> xout;
    MappedBuf<double> xin, xr;
    MappedBuf<uint32_t> xids;
    SeqWord xseq;                               // completion word of the express launches (kernels.hpp ExpressSignal)
    DevBuf<uint32_t> d_xcounter;
    // host-buffer batches of up to kMappedMaxQ queries: queries read from, results exported to, host-mapped memory (no DMA copies)
    MappedBuf<float> mq;
    MappedBuf<uint32_t> mi;
    MappedBuf<double> md;
    int64_t mcap = 0;
    MappedBuf<unsigned char> frame;             // host-mapped staging of appended sensor frames (ring_append)
    MappedBuf<unsigned char> astage;            // the library's own staging of copied frames
    hipEvent_t ev_mut = nullptr;                                // recorded on the library's stream behind an asynchronous mutation
    bool mut_pending = false;                                   // ... which a call on another stream has to order itself behind
    bool append_pending = false;                                // ring_append returned before its insert kernel finished (ring_host.inc)
    // fused RRT* expansion (small clouds = node sets): per-node {x, y, z, radius} as the planner holds them, and the results
    MappedBuf<double> aux;
    MappedBuf<ExpandOut> eout;
    MappedBuf<double> bpos;                     // express Bezier check: sample positions
    DevBuf<unsigned char> d_stage;
    DevBuf<float> d_bbox;                       // bounding-box partials of the index build (a buffer of their own, not the upload staging)
    DevBuf<GbCheck> d_gbcheck;                  // the build's self-check (gridbuild.hpp): device words + pinned read-back
    PinnedBuf<GbCheck> h_gbcheck;
    GbCheck last_check{};                       // as read back by the last build
    // bounding-box pyramid over the cell index (pyramid.hpp): built for clouds with sparse occupancy
    bool has_pyr = false;
    int nn_block = 256;            // threads per block of the dense NN batch kernel (build_grid chooses; kernels.hpp kNNBlock)
    PyrDesc P{};
    DevBuf<PyrNode> pyr_nodes;
    DevBuf<unsigned char> pyr_hint;             // start level of the walk per level-0 cell
    size_t pyr_total = 0;
    double empty_frac = 0.0;
    bool was_sparse = false;                    // the previous build found most cells empty: this one uses smaller cells
    // grid
    bool has_grid = false;
    GridDesc G{};
    DevBuf<uint32_t> cell_start;
    DevBuf<float4> sorted;
    DevBuf<uint4> blocks;                    // block table (kernels.hpp block_corner_kernel): 2 x uint4 per lattice corner
    BinDesc B{};
    DevBuf<float4> d_qsorted;                                                   // {x,y,z,id} records of the sorted batch (reserve_queries)
    DevBuf<uint32_t> d_sort1;                                                   // total1 | total1 (second set)
    DevBuf<uint32_t> d_slice;                                                   // per sort block, its offset inside every bucket (reserve_queries)
    int sort_phase = 0;                                                         // which set of totals the next batch adds into
    // query workspaces (one group: pct_cloud_reserve_queries)
    int64_t qcap = 0;
    DevBuf<float> d_q, d_r;
    DevBuf<double> d_q64, d_r2, d_d2, d_radius, d_pts64;
    DevBuf<double> d_seg;                                       // the host forms' staged segments (segment.hpp): 6 doubles each
    DevBuf<uint32_t> d_idx, d_count, d_bound;
    DevBuf<uint32_t> d_todo;                                    // {count, ticket, slots...}: queries the fp32 pyramid walk leaves to the exact one
    DevBuf<unsigned char> d_skip;
    DevBuf<double> d_part_d2;         // per-(query, block) partial minima of the streaming kernels: part_q x kMaxParts entries;
    DevBuf<uint32_t> d_part_idx;      // larger batches go through them in slices of part_q queries
    int64_t part_q = 0;
    DevBuf<uint32_t> d_ovf;                                    // [0] = number of overflowed candidate lists, [1..] = their queries
    DevBuf<uint32_t> d_cand_count, d_cand_idx;                 // candidate lists of the brute-force filter: part_q x kCandCap
    DevBuf<double> d_cand_d2;
    // k-NN batches (knn.hpp): the host entry points' Q x k result rows and the streaming kernel's per-block partial lists (grow-only)
    DevBuf<uint32_t> d_knn_idx, d_knn_pidx;
    DevBuf<double> d_knn_d2, d_knn_pd2;
    size_t knn_out_cap = 0, knn_part_cap = 0;
    // radius-search batches (rsearch.hpp): scan / cursor / queue workspaces sized with the query workspaces, the host form's offsets
    // and the lists of its last result (12 B per entry: no s)
    DevBuf<long long> rs_off;
    DevBuf<uint64_t> rs_tiles;
    DevBuf<uint32_t> rs_cursor, rs_queue;
    int64_t rs_qcap = 0;
    ListStore rs{ "radius-search" };
    // capsule search (segment_search.hpp): the lists of the host form's last result in buffers of their own (20 B per entry)
    // -- pct_radius_search_read promises the last RADIUS search
    ListStore ss{ "capsule-search" };
    // free-space polyhedra (segment_polyhedron.hpp): the host form's candidate rows in buffers of their own (idx + d2, 12 B per entry
    // -- the capsule search's last result stays readable), the supports of its last result (idx, d2, s + 4 doubles of plane), the
    // support offsets on the device, and the per-entry support positions of either form (grown to the rows' capacity by the call)
    ListStore pc{ "polyhedron-candidate" };
    ListStore pl{ "free-space-polyhedron" };
    DevBuf<double> pl_plane;
    DevBuf<long long> pl_off;
    DevBuf<uint32_t> pl_sup;
    // order-preserving crop (lidar): tile counts and the compacted {index, d2, x, y, z} of the last crop
    DevBuf<uint32_t> crop_tile, crop_idx;
    DevBuf<double> crop_d2;
    DevBuf<float> crop_x, crop_y, crop_z;
    size_t crop_cap = 0;
    // bezier
    DevBuf<double> d_coef, d_segtime;
    DevBuf<int> d_orders, d_nsamples;
    DevBuf<long long> d_first_hit;
    size_t seg_cap = 0;
    // batched Bezier check, host form (bezier_batch.hpp): device copies of seg_offsets / t_start, the offsets and the verdicts, at
    // least bb_cap >= B + 1 entries each (one group; the certified check grows bb_segoff alone where it needs more)
    DevBuf<int32_t> bb_segoff;
    DevBuf<double> bb_tstart;
    DevBuf<long long> bb_off;
    DevBuf<pct_traj_verdict> bb_verdict;
    size_t bb_cap = 0;
    // certified Bezier check (bezier_certify.hpp): two sets of pieces (polygon + meta, 328 B per piece) that the rounds write in turn,
    // the split flags and tile sums of a round, the per-trajectory state, the control words, and the host form's certificates and
    // stats (all grow-only)
    DevBuf<double> bc_poly[2];
    DevBuf<BcMeta> bc_meta[2];
    DevBuf<uint32_t> bc_flag, bc_tile;
    DevBuf<BcTraj> bc_traj;
    DevBuf<BcCtl> bc_ctl;
    DevBuf<pct_traj_certificate> bc_cert;
    DevBuf<long long> bc_stats;
    // trajectory clearance (bezier_clearance.hpp): it shares the piece sets, flags, tile sums, state and control words above (the two
    // calls never run concurrently on one cloud) and adds the piece scalars (32 B per piece), its own per-trajectory minima and the
    // host form's records
    DevBuf<double> cl_geom;
    DevBuf<ClTraj> cl_traj;
    DevBuf<pct_traj_clearance> cl_out;
    // windows of a trajectory (both calls' window forms): u0, u1 per segment, and the host forms' copies of t_start and horizon
    DevBuf<double> bc_win, bc_tstart, bc_horizon;
    // measurement
    hipEvent_t ev0 = nullptr, ev1 = nullptr;    // around the whole batch (all kernels of one query call)
    hipEvent_t ev2 = nullptr, ev3 = nullptr;    // around the batch's dominant kernel only (aliases of the ring's current pair)
    // the last kDomRing batches' dominant-kernel event pairs, so a caller can time K back-to-back batches without a host
    // sync in between and read every launch's duration afterwards (bench.py's roofline figure)
    static constexpr int kDomRing = 64;
    hipEvent_t dom_ring[2 * kDomRing] = {};
    uint64_t dom_seq = 0;                       // completed (begin + end) pairs
    uint64_t dom_launch = 0;                    // launches of the sampled (index) path since pct_set_timing_stride
    int dom_stride = 1;                         // the index path records every dom_stride-th launch (pct_set_timing_stride)
    hipEvent_t last2 = nullptr, last3 = nullptr;    // the most recent COMPLETE pair (pct_last_kernel_ms)
    bool ev_valid = false, dom_valid = false;
    int timing_level = 1;                       // 0 = no events, 1 = dominant kernel only (default), 2 = + the whole batch
    DevBuf<WorkCounters> d_work;
    bool count_work = false;
    bool host_work = false;        // last batch's work is known on the host (streaming kernel)
    uint64_t host_points = 0;
    bool capturing = false;
    // bumped whenever something a captured plan baked in goes away or changes meaning: workspace reallocation, a new point
    // count on a cloud without the ring index, grid build / drop, ring-index (re)configuration
    uint64_t generation = 1;
    // contents version (bumped by every upload / append) and the bounding box last computed for it (brute2.hpp's centred filter)
    uint64_t content_epoch = 1, bbox_epoch = 0;
    float bbox_lo[3] = { 0, 0, 0 }, bbox_hi[3] = { 0, 0, 0 };
    // rolling-map index (ring.hpp): bucket table that appends update in place
    bool ring_on = false, ring_ready = false;
    float ring_cell_req = 0.0f;
    uint32_t ring_K = 32;                    // records per bucket of the rolling-map index (ring.hpp kRingK .. kRingKMax; grows when the overflow queue fills)
    float ring_extent_req[3] = { 0.0f, 0.0f, 0.0f };
    RingDesc R{};
    size_t ring_cells = 0;
    DevBuf<uint2> ring_ht;
    DevBuf<float4> ring_slots, ring_ovf;
    DevBuf<uint32_t> ring_where;
    DevBuf<RingState> ring_st;
    MappedBuf<uint32_t> ring_status;                                  // host-mapped {overrun flag, overflow-queue length}
    int64_t ring_cfg_count = 0;                                       // points in the window when the table was last sized
    int ring_appends_since_cfg = 0;
    // removing points (ring_remove.hpp, pct_cloud_ring_remove_*): removals since the last upload (the sizing box and a refile then
    // leave the removed rows out), the device words a removal's blocks meet on, the host-mapped {sequence, removed, live} the host
    // polls, and the staging of an index list
    bool ring_removed_any = false;
    DevBuf<RingRemoveMeet> d_rm_meet;
    SeqWord rm_word;
    DevBuf<uint32_t> d_rm_list;
    // compacting the window (ring_compact.hpp, pct_cloud_ring_compact): the dead share of the capacity at which a removal compacts
    // before it returns (0 = off), compactions that moved rows so far, and the grow-only scratch -- three SoA arrays of rc_rows rows
    // each in one block, tile totals, the device remap
    double rc_fraction = 0.0;
    uint64_t rc_count = 0;
    DevBuf<float> rc_xyz;
    DevBuf<uint32_t> rc_tile, rc_remap;
    int64_t rc_rows = 0;
    // removing outliers (ring_outlier.hpp, pct_cloud_ring_remove_outliers): one clamped neighbour count per slot, sized by the capacity
    // on first use (grow-only)
    DevBuf<uint32_t> ro_counts;
    // statistical outliers (ring_statistical.hpp, pct_cloud_ring_remove_statistical): one k-NN mean distance per slot and the rows of
    // the reduction tree, sized by the capacity on first use (grow-only); the {sums, mean, deviation, threshold} record on the device
    // and its host-mapped copy
    DevBuf<double> ks_mean;
    DevBuf<KsPart> ks_part;
    DevBuf<KsRecord> ks_rec;
    MappedBuf<KsRecord> ks_rec_host;
    // de-duplicating appends (ring_dedup.hpp, pct_cloud_ring_dedup): voxel size (0 = off), the frame filter's scratch -- key table,
    // per-point table slot, the compaction scratch (sized with it) -- and the host-mapped {sequence, survivors} pair
    double dd_res = 0.0;
    DevBuf<unsigned long long> dd_keys;
    DevBuf<uint32_t> dd_vals, dd_pslot;
    uint32_t dd_tcap = 0;                    // entries of the key table
    CompactScratch dd;
    SeqWord dd_word;
    int64_t dd_last_offered = 0, dd_last_kept = 0;
    uint64_t dd_total_offered = 0, dd_total_kept = 0;
    // depth images (ring_depth.hpp, pct_cloud_ring_carve_depth / pct_cloud_append_depth): the image's staging and the un-projection's
    // compaction scratch.  Two instances: a depth append with de-dup on reads dp.out while the filter writes dd.out.
    DepthStage dp_img;
    CompactScratch dp;
    RangeStage rg_tab;                           // range images (ring_range.hpp) share dp_img and dp; their tables are staged here
    ReplanCtx *rp = nullptr;                     // lazily created context of the un-captured fused planner batch
};

void replan_ctx_free(ReplanCtx *x);              // ring_host.inc

struct pct_plan {
    int kind = 0;                                // 0 = NN batch, 1 = fused replan batch
    uint64_t generation = 0;                     // the cloud's generation the graph was captured at
    int algo = 0;
    ReplanCtx *rx = nullptr;
    double run_us[4] = { 0, 0, 0, 0 };
    pct_cloud *c = nullptr;
    int64_t Q = 0;
    PinnedBuf<float> h_q;
    PinnedBuf<uint32_t> h_idx;
    PinnedBuf<double> h_d2;
    DevBuf<float> d_q;
    DevBuf<uint32_t> d_idx;
    DevBuf<double> d_d2;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

namespace {

// What a cloud-owned buffer calls before it grows.  Growth is refused while the cloud captures a graph or, where the site names one,
// while *capture_stream is being captured; then whatever may still read the old block is waited for.  Each site says what it has
// always tested and waited for: this decides nothing for it.
enum class Wait { Nothing, LibraryStream, Device };
int may_grow(pct_cloud *c, Wait wait, const hipStream_t *capture_stream, const char *what)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (c->capturing || (capture_stream && hipStreamIsCapturing(*capture_stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone))
        return fail(PCT_ERR_INVALID, "cannot grow %s during graph capture (call once with these sizes before capturing)", what);
    if (wait == Wait::LibraryStream) HIPCHK(hipStreamSynchronize(g_stream));
    if (wait == Wait::Device) HIPCHK(hipDeviceSynchronize());
    return PCT_OK;
}

// the device forms work in the query workspaces: n entries must fit what pct_cloud_reserve_queries reserved
inline int require_reserved(const pct_cloud *c, int64_t n, const char *what)
{
    if (n > c->qcap) return fail(PCT_ERR_INVALID, "%s of %lld exceeds reserved %lld (call pct_cloud_reserve_queries)", what, (long long)n, (long long)c->qcap);
    return PCT_OK;
}

// completion word for the next express launch on this cloud (seq = nullptr when polling is off: express_wait then synchronises)
ExpressSignal next_signal(pct_cloud *c)
{
    const uint32_t seq = c->xseq.next();
    return ExpressSignal{ c->d_xcounter, poll_results() ? c->xseq.w.get() : nullptr, seq };
}

// wait for the express launch that carried next_signal()
int express_wait(pct_cloud *c) { return c->xseq.wait(c->xseq.seq, nullptr); }

// host-mapped query / result buffers of the mid-size host-buffer batches (grow-only, power of two)
int ensure_mapped_io(pct_cloud *c, int64_t Q)
{
    if (Q <= c->mcap) return PCT_OK;
    const int64_t cap = pow2_at_least<int64_t>(4096, Q);
    return regrow(c->mcap, cap, part(c->mq, (size_t)(4 * cap)),      // 3 floats per query + a radius
                  part(c->mi, (size_t)cap), part(c->md, (size_t)cap));
}

bool mapped_io_on()
{
    static const bool on = [] { const char *e = std::getenv("PCT_MAPPED_IO"); return e ? std::atoi(e) != 0 : true; }();
    return on && poll_results();
}

// Rolling-map appends and index builds return once their launches are queued on the library's stream.  Calls on that stream are
// ordered behind them by construction; a *_dev call on the caller's own stream waits on this event (until it has been seen complete).
int note_mutation(pct_cloud *c)
{
    if (!c->ev_mut) HIPCHK(hipEventCreateWithFlags(&c->ev_mut, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->ev_mut, g_stream));
    c->mut_pending = true;
    return PCT_OK;
}

int order_after_mutations(pct_cloud *c, hipStream_t s)
{
    if (!c->mut_pending || s == g_stream) return PCT_OK;
    const hipError_t q = hipEventQuery(c->ev_mut);
    if (q == hipSuccess) { c->mut_pending = false; return PCT_OK; }
    if (q != hipErrorNotReady) return fail(PCT_ERR_HIP, "hipEventQuery -> %s", hipGetErrorString(q));
    HIPCHK(hipStreamWaitEvent(s, c->ev_mut, 0));
    return PCT_OK;
}

int require_init()
{
    if (g_device < 0) return pct_init(0);
    return PCT_OK;
}

int ensure_stage(pct_cloud *c, size_t bytes) { return c->d_stage.reserve(bytes); }

// Close a build: read the self-check back behind the last launch, synchronise, compare.  The ids of the records must sum and xor
// to those of 0..n-1 and no record may sit outside its slab / cell; anything else is a wrong index and is reported, not served.
int finish_build(pct_cloud *c, const GridDesc &G, hipError_t e, hipStream_t s)
{
    if (e == hipSuccess) e = hipMemcpyAsync(c->h_gbcheck, c->d_gbcheck, sizeof(GbCheck) * kGbCheckSlots, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(PCT_ERR_HIP, "grid build failed: %s", hipGetErrorString(e));
    GbCheck k{};
    for (int i = 0; i < kGbCheckSlots; i++) {
        k.sum_ids += c->h_gbcheck[i].sum_ids; k.xor_ids ^= c->h_gbcheck[i].xor_ids;
        k.misplaced += c->h_gbcheck[i].misplaced; k.empty_cells += c->h_gbcheck[i].empty_cells;
    }
    c->last_check = k;
    const uint64_t n = (uint64_t)c->count;
    const uint64_t want_sum = n * (n - 1) / 2;
    uint32_t want_xor = 0;                       // xor of 0 .. n-1
    switch ((n - 1) & 3u) { case 0: want_xor = (uint32_t)(n - 1); break; case 1: want_xor = 1u; break; case 2: want_xor = (uint32_t)n; break; default: want_xor = 0u; }
    if (k.sum_ids != want_sum || k.xor_ids != want_xor || k.misplaced != 0 || k.empty_cells > G.ncells)
        return fail(PCT_ERR_INTERNAL, "index build self-check failed: ids sum %llu (want %llu) xor %08x (want %08x), %u misplaced records, %u of %u cells empty",
                    (unsigned long long)k.sum_ids, (unsigned long long)want_sum, k.xor_ids, want_xor, k.misplaced, k.empty_cells, G.ncells);
    return PCT_OK;
}

// counting sort of the cloud into the cells of G: c->cell_start (ncells+1 prefix) and c->sorted, the float4 {x,y,z,index} copy in cell order
int sort_into_cells(pct_cloud *c, const GridDesc &G)
{
    hipStream_t s = g_stream;
    const int64_t n = c->count;
    const uint64_t ncells = G.ncells;
    PCTCHK(c->cell_start.reserve(ncells + 1));
    if (n > 0) PCTCHK(c->sorted.reserve((size_t)n + kGridPad));      // + spare records behind the last one (gridbuild.hpp)
    // ---- two-level counting sort on LDS histograms (gridbuild.hpp): no device-scope atomic per point ----
    // slabs of 2^s1 consecutive cells, sized for ~2-6 k points each (level 2 then holds a whole slab in LDS), at most kGbMaxSlabs;
    // more, smaller slabs make level 1 slower (more open write streams, more LDS per block) faster than they help level 2
    const uint64_t want_slabs = std::min<uint64_t>((uint64_t)kGbMaxSlabs, std::max<uint64_t>(64, (uint64_t)n / 2048));
    int s1 = 0;
    while (((ncells + (1ull << s1) - 1) >> s1) > want_slabs) s1++;
    if (n >= 4096 && (1u << s1) <= (uint32_t)kGbMaxSlabCells && (uint64_t)n < 0xFFFFFFF0ull) {
        GbDesc D{};
        D.s1 = s1;
        D.nslabs = (uint32_t)((ncells + (1ull << s1) - 1) >> s1);
        const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>(kGbMaxBlocks, (n + 16383) / 16384));
        D.chunk = (uint32_t)((((n + nblk - 1) / nblk) + 3) & ~3ll);
        const int blocks = (int)((n + D.chunk - 1) / D.chunk);
        // level-2 block size by the mean slab: a block holds up to 8 records per thread in LDS (larger slabs stream through twice)
        const double mean_slab = (double)n / D.nslabs;
        const int cthreads = mean_slab <= 1400 ? 256 : mean_slab <= 3000 ? 512 : 1024;
        const size_t lds1 = sizeof(uint32_t) * ((size_t)D.nslabs + 1);
        const size_t lds_cnt = sizeof(uint32_t) * ((((size_t)1 << s1) + 1 + 3) & ~(size_t)3);
        const uint32_t stage_cap = (uint32_t)std::min<size_t>((size_t)kGbStagePerThread * cthreads, (150 * 1024 - lds_cnt) / sizeof(float4));
        const size_t lds2 = lds_cnt + sizeof(float4) * stage_cap;
        static bool attr = false;
        if (!attr) {      // more than the default 64 KiB of LDS per block (gfx950: 160 KiB per CU)
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(gb_hist_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024));
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(gb_scatter_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024));
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(gb_cells_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(gb_cells_kernel<512>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(gb_cells_kernel<1024>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
            attr = true;
        }
        // scratch kept with the cloud (a rebuild per sensor frame must not pay hipMalloc / hipFree): records + table + slab counters
        PCTCHK(c->gb_tmp.reserve((size_t)n));
        PCTCHK(c->gb_small.reserve((size_t)blocks * D.nslabs + 3 * (size_t)D.nslabs + 8));
        // level 1 in two passes of fan-out <= 128 when there are many slabs (gridbuild.hpp): pass A sorts by super-slab into the final
        // array (unused until level 2 writes it), pass B by slab inside every super-slab's region into gb_tmp
        uint32_t two_pass_min = 4096;                 // read per build: the tests lower it to reach this path with small clouds
        if (const char *e = std::getenv("PCT_GB_TWO_PASS_MIN_SLABS")) two_pass_min = (uint32_t)std::max(2, std::atoi(e));
        if (D.nslabs >= two_pass_min) {
            Gb2Desc DB{};
            DB.s1 = s1;
            int lg = 0;
            while ((1u << lg) < D.nslabs) lg++;
            DB.sb = std::min(7, (lg + 1) / 2);
            DB.nslabs = D.nslabs;
            DB.nsuper = (D.nslabs + (1u << DB.sb) - 1) >> DB.sb;
            DB.parts = std::max<uint32_t>(1, 512u / DB.nsuper);
            GbDesc DA = D;
            DA.s1 = s1 + DB.sb;
            DA.nslabs = DB.nsuper;
            const size_t nsub = (size_t)1 << DB.sb;
            const size_t need2 = (size_t)blocks * DA.nslabs + 3 * (size_t)DA.nslabs + 8 + (size_t)DB.nsuper * DB.parts * nsub + 3 * (size_t)D.nslabs + 8;
            PCTCHK(c->gb_small.reserve(need2));
            uint32_t *tableA = c->gb_small, *super_total = tableA + (size_t)blocks * DA.nslabs, *super_cursor = super_total + DA.nslabs,
                     *super_start = super_cursor + DA.nslabs, *table2 = super_start + DA.nslabs + 1,
                     *slab_total = table2 + (size_t)DB.nsuper * DB.parts * nsub, *slab_cursor = slab_total + D.nslabs, *slab_start = slab_cursor + D.nslabs;
            hipError_t e = hipSuccess;
            gb_zero_kernel<<<ceil_div(2 * (int64_t)DA.nslabs, 256), 256, 0, s>>>(super_total, 2 * DA.nslabs, nullptr);
            gb_zero_kernel<<<ceil_div(2 * (int64_t)D.nslabs, 256), 256, 0, s>>>(slab_total, 2 * D.nslabs, c->d_gbcheck);
            {
                const size_t ldsA = sizeof(uint32_t) * ((size_t)DA.nslabs + 1);
                gb_hist_kernel<<<blocks, kGbThreads, ldsA, s>>>(G, DA, c->x, c->y, c->z, (uint32_t)n, tableA, super_total);
                gb_scatter_kernel<<<blocks, kGbThreads, ldsA, s>>>(G, DA, c->x, c->y, c->z, (uint32_t)n, tableA, super_total, super_cursor, super_start, c->sorted);
                const dim3 g2(DB.parts, DB.nsuper);
                gb_hist2_kernel<<<g2, kGbThreads, 0, s>>>(G, DB, super_start, c->sorted, table2, slab_total);
                gb_scatter2_kernel<<<g2, kGbThreads, 0, s>>>(G, DB, super_start, c->sorted, table2, slab_total, slab_cursor, slab_start, (uint32_t)n, c->gb_tmp);
                if (cthreads == 256) gb_cells_kernel<256><<<(int)D.nslabs, 256, lds2, s>>>(G, D, slab_start, c->gb_tmp, (uint32_t)n, stage_cap, c->cell_start, c->sorted, c->d_gbcheck);
                else if (cthreads == 512) gb_cells_kernel<512><<<(int)D.nslabs, 512, lds2, s>>>(G, D, slab_start, c->gb_tmp, (uint32_t)n, stage_cap, c->cell_start, c->sorted, c->d_gbcheck);
                else gb_cells_kernel<1024><<<(int)D.nslabs, 1024, lds2, s>>>(G, D, slab_start, c->gb_tmp, (uint32_t)n, stage_cap, c->cell_start, c->sorted, c->d_gbcheck);
                e = hipGetLastError();
            }
            return finish_build(c, G, e, s);
        }
        uint32_t *table = c->gb_small, *slab_total = table + (size_t)blocks * D.nslabs, *slab_cursor = slab_total + D.nslabs,
                 *slab_start = slab_cursor + D.nslabs;
        hipError_t e = hipSuccess;
        gb_zero_kernel<<<ceil_div(2 * (int64_t)D.nslabs, 256), 256, 0, s>>>(slab_total, 2 * D.nslabs, c->d_gbcheck);
        {
            gb_hist_kernel<<<blocks, kGbThreads, lds1, s>>>(G, D, c->x, c->y, c->z, (uint32_t)n, table, slab_total);
            gb_scatter_kernel<<<blocks, kGbThreads, lds1, s>>>(G, D, c->x, c->y, c->z, (uint32_t)n, table, slab_total, slab_cursor, slab_start, c->gb_tmp);
            if (cthreads == 256) gb_cells_kernel<256><<<(int)D.nslabs, 256, lds2, s>>>(G, D, slab_start, c->gb_tmp, (uint32_t)n, stage_cap, c->cell_start, c->sorted, c->d_gbcheck);
            else if (cthreads == 512) gb_cells_kernel<512><<<(int)D.nslabs, 512, lds2, s>>>(G, D, slab_start, c->gb_tmp, (uint32_t)n, stage_cap, c->cell_start, c->sorted, c->d_gbcheck);
            else gb_cells_kernel<1024><<<(int)D.nslabs, 1024, lds2, s>>>(G, D, slab_start, c->gb_tmp, (uint32_t)n, stage_cap, c->cell_start, c->sorted, c->d_gbcheck);
            e = hipGetLastError();
        }
        return finish_build(c, G, e, s);
    }
    // ---- small clouds / very fine user-given cells: one device atomic per point and pass ----
    DevBuf<uint32_t> d_cnt, d_pcell, d_tiles;          // (freed on every return; finish_build has synchronised by then)
    const uint32_t ntiles = (uint32_t)((ncells + kScanTile - 1) / kScanTile);
    PCTCHK(d_cnt.reset(ncells));
    PCTCHK(d_pcell.reset((size_t)n));
    PCTCHK(d_tiles.reset(ntiles));
    hipError_t e = hipMemsetAsync(d_cnt, 0, sizeof(uint32_t) * ncells, s);
    const int pblocks = (int)std::min<int64_t>(4096, (n + 255) / 256);
    if (e == hipSuccess) {
        cell_histogram_kernel<<<pblocks, 256, 0, s>>>(G, c->x, c->y, c->z, (uint32_t)n, d_cnt, d_pcell);
        scan_tiles_kernel<<<ntiles, 256, 0, s>>>(d_cnt, (uint32_t)ncells, c->cell_start, d_tiles);
        scan_tile_sums_kernel<uint32_t><<<1, 256, 0, s>>>(d_tiles, ntiles, ScanDoneNothing{});
        scan_add_kernel<<<ceil_div((int64_t)ncells, 256), 256, 0, s>>>(c->cell_start, (uint32_t)ncells, d_tiles, (uint32_t)n);
        e = hipMemsetAsync(d_cnt, 0, sizeof(uint32_t) * ncells, s);
    }
    if (e == hipSuccess) {
        cell_scatter_kernel<<<pblocks, 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)n, d_pcell, c->cell_start, d_cnt, c->sorted);
        gb_zero_kernel<<<1, 64, 0, s>>>(nullptr, 0, c->d_gbcheck);
        gb_check_kernel<<<(int)std::min<int64_t>(1024, (std::max<int64_t>(n, (int64_t)ncells) + 255) / 256), 256, 0, s>>>(G, c->sorted, c->cell_start, (uint32_t)n, c->d_gbcheck);
        e = hipGetLastError();
    }
    return finish_build(c, G, e, s);
}

void drop_grid(pct_cloud *c)
{
    if (c->has_grid) c->generation++;
    c->has_grid = false;
    c->rs.valid = false;                // every upload, append, build and drop comes through here: the last radius-search result ends
    c->ss.valid = false;                // and the last capsule search's
    c->pl.valid = false;                // and the last free-space polyhedra
    c->has_pyr = false;
}

// Bounding-box pyramid over the freshly built cell index (pyramid.hpp).  Built when the index is sparsely occupied -- surfaces,
// clusters, a window much larger than its contents: the clouds on which the shell walk pays for empty space -- or on request
// (PCT_PYRAMID=1 forces it on any cloud: the tests and the soak run the dense fixtures through the walk that way; =0 never).
int build_pyramid(pct_cloud *c, const GridDesc &G)
{
    c->has_pyr = false;
    c->empty_frac = G.ncells ? (double)c->last_check.empty_cells / (double)G.ncells : 0.0;
    int mode = -1;
    if (const char *e = std::getenv("PCT_PYRAMID")) mode = std::atoi(e);
    double min_empty = 0.25;                      // uniform cloud at 6 points per cell: e^-6 = 0.25 % of the cells are empty
    if (const char *e = std::getenv("PCT_PYRAMID_MIN_EMPTY")) min_empty = std::atof(e);
    if (mode == 0 || (mode < 0 && c->empty_frac < min_empty)) { c->was_sparse = false; return PCT_OK; }
    PyrDesc P{};
    int nlev = 1;
    while (pyr_dim(G.gx, nlev - 1) > 2 || pyr_dim(G.gy, nlev - 1) > 2 || pyr_dim(G.gz, nlev - 1) > 2) nlev++;
    if (nlev > kPyrMaxLevels) return fail(PCT_ERR_INTERNAL, "pyramid deeper than %d levels", kPyrMaxLevels);
    P.nlev = nlev;
    // level l = blocks of 8 children per node of level l + 1 (pyramid.hpp): 8 * |grid of level l + 1| slots
    size_t total = 0, nslots[kPyrMaxLevels] = {};
    for (int l = 0; l < nlev; l++) {
        nslots[l] = 8 * (size_t)pyr_dim(G.gx, l + 1) * pyr_dim(G.gy, l + 1) * pyr_dim(G.gz, l + 1);
        P.off[l] = (uint32_t)total;
        total += nslots[l];
    }
    if (total > 0xFFFFFFF0ull) return PCT_OK;      // cannot be addressed with 32-bit slot offsets: stay with the shell walk
    PCTCHK(c->pyr_nodes.reserve(total));
    hipStream_t s = g_stream;
    pyr_leaf_kernel<<<ceil_div((int64_t)nslots[0], 32), 256, 0, s>>>(G, P, c->sorted, c->cell_start, c->pyr_nodes, (uint32_t)nslots[0]);
    for (int l = 1; l < nlev; l++)
        pyr_up_kernel<<<ceil_div((int64_t)nslots[l], 256), 256, 0, s>>>(G, P, l, c->pyr_nodes, (uint32_t)nslots[l]);
    PCTCHK(c->pyr_hint.reserve((size_t)G.ncells));
    pyr_hint_kernel<<<ceil_div((int64_t)G.ncells, 256), 256, 0, s>>>(G, P, c->pyr_nodes, c->pyr_hint);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    c->P = P;
    c->pyr_total = total;
    c->has_pyr = true;
    c->was_sparse = c->empty_frac > 0.6;
    return PCT_OK;
}

// host AoS -> device SoA slots [dst0, dst0+n)
int upload_range(pct_cloud *c, const void *pts, int64_t n, int64_t stride, int64_t dst0)
{
    if (n == 0) return PCT_OK;
    if (c->host_mapped) {   // plain host stores; every earlier kernel on this cloud has been waited for
        const unsigned char *src = static_cast<const unsigned char *>(pts);
        for (int64_t i = 0; i < n; i++) {
            const float *p = reinterpret_cast<const float *>(src + i * stride);
            c->hx[dst0 + i] = p[0]; c->hy[dst0 + i] = p[1]; c->hz[dst0 + i] = p[2];
        }
        return PCT_OK;
    }
    PCTCHK(ensure_stage(c, (size_t)n * stride + 64));
    HIPCHK(hipMemcpyAsync(c->d_stage, pts, (size_t)n * stride, hipMemcpyHostToDevice, g_stream));
    if (stride == 12 && (dst0 & 3) == 0 && n >= 4) {
        const uint32_t ng = (uint32_t)(n >> 2);
        deinterleave12_kernel<<<ceil_div(ng, 256), 256, 0, g_stream>>>(reinterpret_cast<const float4 *>(c->d_stage.get()), ng,
                                                                        reinterpret_cast<float4 *>(c->x + dst0),
                                                                        reinterpret_cast<float4 *>(c->y + dst0),
                                                                        reinterpret_cast<float4 *>(c->z + dst0));
        const int64_t done = (int64_t)ng * 4;
        if (done < n)
            deinterleave_kernel<<<1, 256, 0, g_stream>>>(c->d_stage + done * 12, 12, (uint32_t)(n - done), c->x, c->y, c->z,
                                                         (uint32_t)(dst0 + done));
    } else {
        deinterleave_kernel<<<ceil_div(n, 256), 256, 0, g_stream>>>(c->d_stage, (uint32_t)stride, (uint32_t)n, c->x, c->y, c->z,
                                                                    (uint32_t)dst0);
    }
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

// Streaming kernels are grid-stride: at most 4 blocks of 256 threads per CU (16 waves per CU),
// so the whole grid is resident in ONE round whatever the kernel's register count -- a grid of
// 8 blocks per CU ran as 7 + 1 rounds at 66 VGPRs and cost almost 2x.
// Q: the batch's size where the caller knows it (0 = unknown).  One or two queries against a DRAM-resident cloud do better with half the
// waves: 512 blocks (2 waves per SIMD) read 100 M points at 0.78-0.80 of the 8 TB/s peak, 1024 at 0.74-0.77, 2048 at 0.72-0.73
// (scripts/probe_stream.py; Q = 4 and the Infinity-Cache-sized 10 M-point cloud are the other way round or level).
int stream_blocks(int64_t n, int64_t Q = 0)
{
    const char *e = std::getenv("PCT_STREAM_BLOCKS");      // tuning knob for scripts/probe.py, scripts/probe_stream.py
    const int cap = e ? std::max(1, std::min(kMaxParts, std::atoi(e))) : ((Q == 1 || Q == 2) && n >= (1ll << 25) ? 512 : 1024);
    const int64_t groups = std::max<int64_t>(n >> 2, 1);
    return (int)std::min<int64_t>(cap, (groups + 255) / 256);
}

void begin_timing(pct_cloud *c, hipStream_t s)
{
    c->ev_valid = false;
    if (c->capturing || c->timing_level < 2) return;     // an event pair costs ~5-9 us of a 190 us batch (same-box A/B)
    if (hipEventRecord(c->ev0, s) == hipSuccess) c->ev_valid = true;
}

void end_timing(pct_cloud *c, hipStream_t s)
{
    if (c->capturing || !c->ev_valid) return;
    if (hipEventRecord(c->ev1, s) != hipSuccess) c->ev_valid = false;
}

// events around the dominant kernel of the batch (what rocprofv3's per-kernel average also measures)
bool dom_ext_on()
{
    static const bool on = [] { const char *e = std::getenv("PCT_DOM_EXT_EVENTS"); return e ? std::atoi(e) != 0 : true; }();
    return on;
}

// ext = the caller launches the kernel with hipExtLaunchKernelGGL(start = ev2, stop = ev3) itself (and calls dom_done): nothing is
// recorded here; that path also honours the sampling stride
void dom_begin(pct_cloud *c, hipStream_t s, bool ext = false)
{
    c->dom_valid = false;
    if (c->capturing || c->timing_level < 1) return;
    if (ext && c->dom_stride > 1 && (c->dom_launch++ % (uint64_t)c->dom_stride) != 0) return;
    const int slot = (int)(c->dom_seq % pct_cloud::kDomRing);
    c->ev2 = c->dom_ring[2 * slot];
    c->ev3 = c->dom_ring[2 * slot + 1];
    if (ext && dom_ext_on()) { c->dom_valid = true; return; }
    if (hipEventRecord(c->ev2, s) == hipSuccess) c->dom_valid = true;
}

void dom_done(pct_cloud *c)
{
    c->dom_valid = false;
    c->dom_seq++;
    c->last2 = c->ev2;
    c->last3 = c->ev3;
}

void dom_end(pct_cloud *c, hipStream_t s)
{
    if (c->capturing || !c->dom_valid) return;
    if (hipEventRecord(c->ev3, s) != hipSuccess) c->dom_valid = false;
    else dom_done(c);
}

// ---- the launch frame -------------------------------------------------------------------------------------------------------
// Every batch search queues its kernels through launch_frame, the one place that says where pct_last_work finds the batch's work,
// zeroes the device counters, records the timing events and asks hipGetLastError.  On the stream, in this order:
//   [memset of the work counters]  [ev0]  prologue  [ev2]  dominant  [ev3]  epilogue  [ev1]
enum class Work {
    Device,        // the kernels add to c->d_work, zeroed here when counting is on
    DeviceKept,    // the NN batch over the bucket table: read from c->d_work as well, but its kernel does not count and the counters are not
                   // zeroed, so pct_last_work reports the last instrumented batch (kept as found; looks like an oversight)
    EveryPoint,    // streaming kernels: every point for every query, Q x n, known on the host
    Untouched      // the streaming radius count says nothing: pct_last_work keeps reporting the batch before it (kept as found)
};
enum class Dom {
    None,          // no events around a dominant kernel
    Events,        // dom_begin / dom_end record them
    Ext            // as Events, but when work is not counted the region is opened for a kernel that carries its own timestamps (launch_dominant)
};
struct Frame { Work work; Dom dom = Dom::Events; };

inline void no_step() {}

// a step of the frame: a callable that returns a status, or nothing when all it does is launch
template <typename F>
int run_step(F step)
{
    if constexpr (std::is_void_v<decltype(step())>) { step(); return PCT_OK; }
    else return step();
}

// prologue / epilogue: inside the timed batch, outside the dominant region.  Q: the batch's size, for Work::EveryPoint.
template <typename P, typename D, typename E>
int launch_frame(pct_cloud *c, hipStream_t s, int64_t Q, Frame f, P prologue, D dominant, E epilogue)
{
    if (f.work == Work::Device || f.work == Work::DeviceKept) c->host_work = false;
    if (f.work == Work::Device && c->count_work) HIPCHK(hipMemsetAsync(c->d_work, 0, sizeof(WorkCounters) * kWorkSlots, s));
    begin_timing(c, s);
    PCTCHK(run_step(prologue));
    if (f.dom != Dom::None) dom_begin(c, s, f.dom == Dom::Ext && !c->count_work);
    PCTCHK(run_step(dominant));
    if (f.dom != Dom::None) dom_end(c, s);
    PCTCHK(run_step(epilogue));
    end_timing(c, s);
    HIPCHK(hipGetLastError());
    if (f.work == Work::EveryPoint) {
        c->host_work = true;
        c->host_points = (uint64_t)Q * (uint64_t)c->count;
    }
    return PCT_OK;
}

template <typename D>
int launch_frame(pct_cloud *c, hipStream_t s, int64_t Q, Frame f, D dominant)
{
    return launch_frame(c, s, Q, f, no_step, dominant, no_step);
}

// The dominant kernel of a Dom::Ext frame (blocks of THREADS threads).  Where dom_begin left the region to the kernel, it is launched
// with its own begin / end timestamps (hipExtLaunchKernel): no marker packets on the stream -- the two hipEventRecord calls of
// dom_begin / dom_end cost ~10 us of a 160 us step.
// (the arguments arrive as the kernel's own parameter types: a buffer is handed over as its device pointer)
template <typename T> struct as_declared { using type = T; };
template <int THREADS = 256, typename... P>
void launch_dominant(pct_cloud *c, hipStream_t s, void (*kernel)(P...), int blocks, typename as_declared<P>::type... args)
{
    if (!c->count_work && c->dom_valid && dom_ext_on()) {
        hipExtLaunchKernelGGL(kernel, dim3(blocks), dim3(THREADS), 0, s, c->ev2, c->ev3, 0, args...);
        dom_done(c);
    } else
        kernel<<<blocks, THREADS, 0, s>>>(args...);
}

// streaming NN over the fp64 queries already in c->d_q64: one slice of at most c->part_q queries starting at qoff
int nn_stream_q64_slice(pct_cloud *c, int64_t qoff, int64_t Q, uint32_t *d_idx, double *d_d2, hipStream_t s)
{
    const double *d_q64 = c->d_q64 + 3 * qoff;
    d_idx += qoff;
    d_d2 += qoff;
    const int blocks = stream_blocks(c->count, Q);
    return launch_frame(c, s, Q, { Work::EveryPoint }, no_step,
        [&] {
            for_each_query_tile(Q, [&](auto qt, int q0, int qcount) {
                nn_stream_kernel<decltype(qt)::value><<<blocks, 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)c->count, d_q64, q0, qcount, c->d_part_d2,
                                                                             c->d_part_idx, blocks);
            });
        },
        [&] {
            nn_reduce_partials_kernel<<<(int)Q, 256, 0, s>>>(c->d_part_d2, c->d_part_idx, blocks, (uint32_t)c->index_base, d_idx, d_d2);
        });
}

int nn_stream_q64(pct_cloud *c, int64_t Q, uint32_t *d_idx, double *d_d2, hipStream_t s)
{
    for (int64_t off = 0; off < Q; off += c->part_q) PCTCHK(nn_stream_q64_slice(c, off, std::min<int64_t>(c->part_q, Q - off), d_idx, d_d2, s));
    c->host_points = (uint64_t)Q * (uint64_t)c->count;
    return PCT_OK;
}

// The sort's blocks for a batch of Q: ~128 blocks: small batches want parallelism (64 K queries: 21 us at 1024 per block, 36 us at 8192),
// large ones want long per-block bucket slices (1 M: 67 us at 8192, 87 us at 1024; with the multiply-free bin 4096 per block still costs
// the step 2.8 us more than 8192, profiles/qsort_bin_ab.txt)
static uint32_t sort_per_block(int64_t Q)
{
    return (uint32_t)std::min<int64_t>(kSortPerBlock, std::max<int64_t>(1024, (Q / 128 + 1023) / 1024 * 1024));
}
// Rows of the slice table that serve every batch of at most qcap queries.  Below kSortPerBlock per block, per_block = 1024 m >= Q / 128
// rounded down, so Q <= 128 * 1024 m + 127 and the batch has at most 129 blocks; at kSortPerBlock it has ceil(Q / kSortPerBlock).
static size_t sort_slice_rows(int64_t qcap)
{
    return (size_t)std::max<int64_t>(129, ceil_div(qcap, (int64_t)kSortPerBlock));
}

// counting sort of the batch by coarse cell (kernels.hpp qsort_*) -> c->d_qsorted; *recs_out = nullptr: small batch, arrival order
int bin_queries(pct_cloud *c, const float *d_q, int64_t Q, hipStream_t s, const float4 **recs_out)
{
    *recs_out = nullptr;
    if (Q < 16384) return PCT_OK;
    const BinDesc &B = c->B;
    int key_shift = 0;
    while ((((uint64_t)B.nbins - 1) >> key_shift) >= (1ull << 20)) key_shift++;
    // two sets of bucket totals used in turn: a batch's histogram pass zeroes the set the NEXT batch will add into (a captured
    // graph replays one set, so it keeps the memset behind its scatter pass instead)
    const bool pingpong = !c->capturing;
    uint32_t *total1 = c->d_sort1 + (c->sort_phase ? kSortBuckets : 0), *total1_next = c->d_sort1 + (c->sort_phase ? 0 : kSortBuckets);
    const uint32_t per_block = sort_per_block(Q);
    const int nb = ceil_div(Q, (int64_t)per_block);
    if ((size_t)nb * kSortBuckets > c->d_slice.capacity()) return fail(PCT_ERR_INVALID, "the sort's slice table has no row for block %d", nb - 1);
    // 16-byte aligned query arrays are fetched four queries (three float4) at a time (kernels.hpp sort_load_items)
    // the bin's arithmetic (query_bin.hpp) is the cloud's choice, made when its index was built: B.fast
    with_bool((reinterpret_cast<uintptr_t>(d_q) & 15u) == 0, [&](auto aligned) {
        with_bool(B.fast != 0, [&](auto fast) {
            constexpr bool A = decltype(aligned)::value, F = decltype(fast)::value;
            qsort_hist_kernel<A, F><<<nb, 1024, 0, s>>>(B, key_shift, d_q, (uint32_t)Q, per_block, total1, c->d_slice, pingpong ? total1_next : nullptr);
            qsort_scatter1_kernel<A, F><<<nb, 1024, 0, s>>>(B, key_shift, d_q, (uint32_t)Q, per_block, total1, c->d_slice, c->d_qsorted);
        });
    });
    if (pingpong) c->sort_phase ^= 1;
    else HIPCHK(hipMemsetAsync(total1, 0, sizeof(uint32_t) * kSortBuckets, s));
    HIPCHK(hipGetLastError());
    *recs_out = c->d_qsorted;
    return PCT_OK;
}

int g_filter_mode = -1;        // pct_debug_set_filter_mode: 0 = never, 1 = whenever valid, -1 = auto

// bounding box of the cloud's current contents, cached per contents version (one reduction + one read-back when stale)
int cloud_bbox_cached(pct_cloud *c)
{
    if (c->bbox_epoch == c->content_epoch) return PCT_OK;
    hipStream_t s = g_stream;
    const int64_t n = c->count;
    const int bblocks = (int)std::min<int64_t>(1024, (n + 255) / 256);
    float *d_part = c->d_bbox;                                         // 1024 x 6 floats, allocated with the cloud
    bbox_partial_kernel<false><<<bblocks, 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)n, d_part);
    std::vector<float> part((size_t)bblocks * 6);
    hipError_t e = hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(float), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(PCT_ERR_HIP, "bbox reduction failed: %s", hipGetErrorString(e));
    for (int k = 0; k < 3; k++) { c->bbox_lo[k] = INFINITY; c->bbox_hi[k] = -INFINITY; }
    for (int b = 0; b < bblocks; b++)
        for (int k = 0; k < 3; k++) {
            c->bbox_lo[k] = std::min(c->bbox_lo[k], part[(size_t)b * 6 + k]);
            c->bbox_hi[k] = std::max(c->bbox_hi[k], part[(size_t)b * 6 + 3 + k]);
        }
    c->bbox_epoch = c->content_epoch;
    return PCT_OK;
}

// Should the brute-force filter take the expanded form (brute2.hpp)?  Only while its absolute error band, ~14 u R^2 (u = 2^-24,
// R = half diagonal of the bounding box), stays small against the squared point spacing of the cloud -- otherwise the band, not
// the sampled bound, decides how many pairs pass.  Fills the centre / R^2 the kernels need.
bool use_expanded_filter(pct_cloud *c, CentreDesc *out)
{
    const int mode = g_filter_mode;
    if (mode == 0 || c->host_mapped || c->capturing || c->count < 4) return false;
    if (mode < 0 && c->count < 200000) return false;             // small clouds: the bounding-box pass would cost more than it saves
    if (cloud_bbox_cached(c) != PCT_OK) return false;
    double h[3], R2 = 0.0, vol = 8.0;
    float ctr[3];
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(c->bbox_lo[k]) || !std::isfinite(c->bbox_hi[k])) return false;
        ctr[k] = (float)(0.5 * ((double)c->bbox_lo[k] + (double)c->bbox_hi[k]));
        h[k] = std::max((double)c->bbox_hi[k] - (double)ctr[k], (double)ctr[k] - (double)c->bbox_lo[k]);
        R2 += h[k] * h[k];
        vol *= h[k];
    }
    R2 *= 1.000001;
    if (!std::isfinite(R2) || R2 > 1e30) return false;
    const double spacing2 = std::pow(vol / (double)c->count, 2.0 / 3.0);
    if (mode < 0 && !(14.0 * 0x1p-24 * R2 <= 0.25 * spacing2)) return false;
    out->cx = ctr[0]; out->cy = ctr[1]; out->cz = ctr[2];
    out->R2 = R2;
    return true;
}

constexpr int kMaxTileParts = 8192;      // tile kernel: at most this many point chunks per launch
constexpr uint32_t kChunkGroupsMax = 3072;   // 3 * 3072 * 16 B = 144 KiB of the CU's 160 KiB LDS

// Default brute-force path: sampled fp32 bound, packed-fp32 filter (expanded form in registers, brute2.hpp, or direct form over
// LDS-staged chunks, kernels.hpp) + exact fp64 recheck of the survivors.  d_qf: the fp32 queries; c->d_q64 must already hold
// their widened copies.
int nn_stream_filtered_slice(pct_cloud *c, const float *d_qf, int64_t qoff, int64_t Q, uint32_t *d_idx, double *d_d2, hipStream_t s)
{
    d_qf += 3 * qoff;
    d_idx += qoff;
    d_d2 += qoff;
    const double *d_q64 = c->d_q64 + 3 * qoff;
    uint32_t *d_bound = c->d_bound + qoff;
    const int64_t ngroups = c->count >> 2;
    // chunk = 1024 groups (4096 points, 48 KiB LDS -> 3 blocks per CU); larger only for huge clouds
    uint32_t chunk = 1024;
    if ((ngroups + chunk - 1) / chunk > kMaxTileParts) chunk = (uint32_t)std::min<int64_t>(kChunkGroupsMax, ((ngroups + kMaxTileParts - 1) / kMaxTileParts + 255) / 256 * 256);
    const int nblocks = (int)std::max<int64_t>(1, (ngroups + chunk - 1) / chunk);
    if (nblocks > kMaxTileParts) return fail(PCT_ERR_INVALID, "cloud of %lld points is too large for the brute-force path", (long long)c->count);
    // sample 1 chunk in 16 (everything for small clouds; sparser for huge ones so the partial buffer fits)
    const uint32_t stride = ngroups >= 256ll * kSampleStride * 8
                                ? (uint32_t)std::max<int64_t>(kSampleStride, (ngroups + 256ll * kMaxParts - 1) / (256ll * kMaxParts))
                                : 1u;
    const int64_t schunks = std::max<int64_t>(1, (ngroups + 256ll * stride - 1) / (256ll * stride));
    const int sblocks = (int)((schunks + kSampleGroups - 1) / kSampleGroups);
    // the sample partials borrow d_part_idx (u32 and float have the same size; [Q][sblocks], sblocks <= kMaxParts);
    // bound_reduce_kernel consumes them before the filter pass overwrites the buffer
    // slices of the batch in grid.y until ~2048 blocks are in flight (the kernels' tile loops are sequential)
    const auto slices_for = [&](int point_blocks, int *qslice) {
        const int tiles = (int)((Q + kTileQ - 1) / kTileQ);
        int slices = std::max(1, std::min(tiles, (2048 + point_blocks - 1) / point_blocks));
        *qslice = ((tiles + slices - 1) / slices) * kTileQ;
        return (int)((Q + *qslice - 1) / *qslice);
    };
    CentreDesc CD{};
    bool expanded = false;
    float4 *qprep = c->d_qsorted + qoff;                         // the query-sort records are idle on this path
    return launch_frame(c, s, Q, { Work::EveryPoint },
        [&]() -> int {
            int sq = 0;
            const int sslices = slices_for(sblocks, &sq);
            nn_sample_bounds_kernel<<<dim3(sblocks, sslices), 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)c->count, stride, d_qf, (int)Q, sq,
                                                                           reinterpret_cast<float *>(c->d_part_idx.get()), sblocks);
            bound_reduce_kernel<<<(int)Q, 256, 0, s>>>(reinterpret_cast<const float *>(c->d_part_idx.get()), sblocks, d_bound);
            expanded = use_expanded_filter(c, &CD);
            if (expanded) {
                // expanded form (brute2.hpp): 3 FMAs per pair on centred coordinates, thresholds widened by the proven error band; the
                // points held in registers (tile_reg_kernel), a block covers 256 * kRegGroups point groups, no LDS
                brute2_prep_kernel<<<ceil_div(Q, 256), 256, 0, s>>>(CD, d_qf, d_bound, (uint32_t)Q, qprep);
                return PCT_OK;
            }
            // survivors of the bound go to per-query candidate lists: no per-tile block reductions, no partial arrays
            static bool attr = false;
            if (!attr) {
                HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(nn_tile_candidates_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(3 * kChunkGroupsMax * sizeof(float4))));
                attr = true;
            }
            return PCT_OK;
        },
        [&] {
            int qs = 0;
            if (expanded) {
                const int rblocks = (int)std::max<int64_t>(1, (ngroups + 256 * kRegGroups - 1) / (256 * kRegGroups));
                const int rslices = slices_for(rblocks, &qs);
                tile_reg_kernel<false><<<dim3(rblocks, rslices), 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)c->count, CD, qprep, d_q64, nullptr, (int)Q, qs,
                                                                               c->d_cand_count, c->d_cand_d2, c->d_cand_idx, nullptr);
            } else {
                const int cslices = slices_for(nblocks, &qs);
                nn_tile_candidates_kernel<<<dim3(nblocks, cslices), 256, 3 * (size_t)chunk * sizeof(float4), s>>>(c->x, c->y, c->z, (uint32_t)c->count, chunk,
                                                                                                                  d_qf, d_q64, d_bound, (int)Q, qs, c->d_cand_count,
                                                                                                                  c->d_cand_d2, c->d_cand_idx);
            }
        },
        [&]() -> int {
            HIPCHK(hipMemsetAsync(c->d_ovf, 0, sizeof(uint32_t), s));
            nn_reduce_candidates_kernel<<<(int)Q, 256, 0, s>>>(c->d_cand_count, c->d_cand_d2, c->d_cand_idx, (uint32_t)c->index_base, c->d_ovf, d_idx, d_d2);
            // overflowed lists (bulk exact ties): exact scan by the whole grid; both kernels return at once when there are none
            nn_overflow_scan_kernel<<<kOvfBlocks, 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)c->count, d_q64, c->d_ovf, c->d_part_d2, c->d_part_idx);
            nn_overflow_fold_kernel<<<(int)Q, 256, 0, s>>>(c->d_ovf, c->d_part_d2, c->d_part_idx, kOvfBlocks, (uint32_t)c->index_base, d_idx, d_d2);
            return PCT_OK;
        });
}

int nn_stream_filtered(pct_cloud *c, const float *d_qf, int64_t Q, uint32_t *d_idx, double *d_d2, hipStream_t s)
{
    for (int64_t off = 0; off < Q; off += c->part_q)
        PCTCHK(nn_stream_filtered_slice(c, d_qf, off, std::min<int64_t>(c->part_q, Q - off), d_idx, d_d2, s));
    c->host_points = (uint64_t)Q * (uint64_t)c->count;
    return PCT_OK;
}

RingView ring_view(const pct_cloud *c);

// ---- which path a batch takes ------------------------------------------------------------------------------------------------
enum class Op {
    NN, Count, KNN, RadiusSearch,
    Segment,       // segment nearest / sweep (segment.hpp)
    Capsule        // capsule count / search (segment_search.hpp)
};
enum class Path {
    Table,         // the rolling-map index (ring.hpp, ring_search.hpp)
    Grid,          // the cell index
    Stream,        // brute force; for NN the fp32 filter + exact fp64 recheck
    StreamExact,   // NN only: brute force with every pair in fp64
    Empty          // the cloud holds no point: pad the outputs (PCT_NO_INDEX / +inf, zero counts, empty rows)
};

// The one place that turns a caller's `algo` into the path of a batch of Q queries, or into PCT_ERR_INVALID with its message
// ("Dispatch of the batch searches").  The searches grew their rules one by one and differ in corners nobody chose;
// each such corner is marked "quirk" here and pinned by tests/test_gpu_dispatch.py, so that changing one is a decision, not an accident.
int resolve_algo(const pct_cloud *c, Op op, int algo, int64_t Q, Path *path)
{
    // quirk: the two segment ops name the values they take in a message of their own, and the segment op -- no grid form, one
    // streaming form -- rejects GRID and STREAM_EXACT before it looks at the cloud (an empty one included)
    if (op == Op::Segment && algo != PCT_ALGO_AUTO && algo != PCT_ALGO_STREAM && algo != PCT_ALGO_RING)
        return fail(PCT_ERR_INVALID, "segment queries take PCT_ALGO_AUTO, PCT_ALGO_STREAM or PCT_ALGO_RING, not algo %d", algo);
    if (op == Op::Capsule && algo != PCT_ALGO_AUTO && algo != PCT_ALGO_STREAM && algo != PCT_ALGO_GRID && algo != PCT_ALGO_RING)
        return fail(PCT_ERR_INVALID, "capsule search takes PCT_ALGO_AUTO, PCT_ALGO_STREAM, PCT_ALGO_GRID or PCT_ALGO_RING, not algo %d", algo);
    // PCT_ALGO_RING names the rolling-map index: it needs a live table, except on a cloud that asked for the index and holds no point
    // yet (the table is sized from the first data: the answer is the empty cloud's)
    if (algo == PCT_ALGO_RING && !c->ring_ready && !(c->ring_on && c->count == 0))
        return fail(PCT_ERR_INVALID, "PCT_ALGO_RING without a rolling-map index (call pct_cloud_ring_index)");
    // quirk: NN, count and k-NN pad an empty cloud's outputs before they look at any other algo value (an unknown one is PCT_OK from
    // the device forms); the radius search and the capsule op validate algo first (the segment op has done so above)
    if (op != Op::RadiusSearch && op != Op::Capsule && c->count == 0) { *path = Path::Empty; return PCT_OK; }
    // quirk: on a rolling map NN takes PCT_ALGO_GRID to mean the bucket table; the other three answer "without a grid"
    if (op == Op::NN && c->ring_ready && algo == PCT_ALGO_GRID) algo = PCT_ALGO_RING;
    if (algo == PCT_ALGO_AUTO) algo = c->ring_ready ? PCT_ALGO_RING : c->has_grid && op != Op::Segment ? PCT_ALGO_GRID : PCT_ALGO_STREAM;
    switch (algo) {
    case PCT_ALGO_RING:
        *path = Path::Table;
        break;
    case PCT_ALGO_GRID:
        // quirk: the count's and the capsule op's message is the short one
        if (!c->has_grid)
            return fail(PCT_ERR_INVALID, op == Op::Count || op == Op::Capsule ? "PCT_ALGO_GRID without a grid" : "PCT_ALGO_GRID without a grid (call pct_cloud_build_grid)");
        *path = Path::Grid;
        break;
    case PCT_ALGO_STREAM:
        // NN, <= 4 queries: the all-fp64 kernel is already HBM-bound (50-62 % of peak); beyond that the packed-fp32 filter wins
        *path = op == Op::NN && Q <= 4 ? Path::StreamExact : Path::Stream;
        break;
    case PCT_ALGO_STREAM_EXACT:
        // quirk: the count called directly rejects STREAM_EXACT; k-NN and the radius search (whose first step is the count) run STREAM
        if (op == Op::Count) return fail(PCT_ERR_INVALID, "unknown algo %d", algo);
        *path = op == Op::NN ? Path::StreamExact : Path::Stream;
        break;
    default:
        return fail(PCT_ERR_INVALID, "unknown algo %d", algo);
    }
    if (op == Op::KNN && *path == Path::Stream && c->capturing)
        return fail(PCT_ERR_INVALID, "the streaming k-NN kernel is not available during graph capture");
    // the radius search and the capsule op, their algo found valid.  quirk: of the host forms that arrive here, the radius search
    // answers an empty cloud with PCT_OK, the capsule op's -- like the segment op's above -- with PCT_ERR_EMPTY (their own line)
    if (c->count == 0) *path = Path::Empty;
    return PCT_OK;
}

// NN of a device-resident batch along `path` (resolve_algo, Op::NN); Q >= 1, within the reserved batch size
int nn_run(pct_cloud *c, Path path, const float *d_q, int64_t Q, uint32_t *d_idx, double *d_d2, hipStream_t s)
{
    switch (path) {
    case Path::Empty:
        fill_empty_kernel<<<ceil_div(Q, 256), 256, 0, s>>>(d_idx, d_d2, (uint32_t)Q);
        HIPCHK(hipGetLastError());
        return PCT_OK;
    case Path::Table:        // rolling-map index: a block per query
        return launch_frame(c, s, Q, { Work::DeviceKept }, [&] {
            ring_batch_kernel<false><<<(int)Q, 256, 0, s>>>(ring_view(c), InflateParams{}, d_q, nullptr, (double)INFINITY, (uint32_t)c->index_base, d_idx, d_d2,
                                                            nullptr, nullptr, ExpressSignal{});
        });
    case Path::Grid: {
        const float4 *recs = nullptr;
        const int blocks = ceil_div(Q, 256 / kCoop);      // 8 lanes per query
        return launch_frame(c, s, Q, { Work::Device, Dom::Ext }, [&] { return bin_queries(c, d_q, Q, s, &recs); },
            [&] {
                with_bool(c->count_work, [&](auto count_work) {
                    constexpr bool CW = decltype(count_work)::value;
                    if (c->has_pyr) {     // sparse occupancy: stage 0, then the bounding-box pyramid instead of cube + shells (pyramid.hpp)
                        // fp32 walk for everybody, then the exact walk for the (few) queries it lists as undecided
                        launch_dominant(c, s, nn_grid_pyr_kernel<CW>, blocks, c->G, c->P, c->pyr_nodes, c->pyr_hint, c->sorted, c->cell_start, d_q, (uint32_t)Q,
                                        (uint32_t)c->index_base, recs, d_idx, d_d2, c->d_work, c->d_todo);
                        nn_grid_pyr_todo_kernel<CW><<<(int)std::min<int64_t>(256, blocks), 256, 0, s>>>(c->G, c->P, c->pyr_nodes, c->pyr_hint, c->sorted, c->cell_start, d_q,
                                                                                                        (uint32_t)c->index_base, recs, d_idx, d_d2, c->d_work, c->d_todo);
                    } else
                        with_bool(narrow_offsets_fit((uint64_t)c->count + kGridPad, (uint64_t)c->G.ncells + 1, (uint64_t)Q), [&](auto narrow) {
                            with_bool(c->nn_block == kNNBlock, [&](auto small_block) {     // the block size is the cloud's (build_grid)
                                constexpr int BLOCK = decltype(small_block)::value ? kNNBlock : 256;
                                launch_dominant<BLOCK>(c, s, nn_grid_coop_kernel<CW, decltype(narrow)::value, BLOCK>, ceil_div(Q, BLOCK / kCoop), c->G, c->sorted,
                                                       c->cell_start, d_q, (uint32_t)Q, (uint32_t)c->index_base, recs, d_idx, d_d2, c->d_work);
                            });
                        });
                });
            }, no_step);
    }
    default:
        widen_queries_kernel<<<ceil_div(3 * Q, 256), 256, 0, s>>>(d_q, (uint32_t)(3 * Q), c->d_q64);
        if (path == Path::StreamExact) return nn_stream_q64(c, Q, d_idx, d_d2, s);
        return nn_stream_filtered(c, d_q, Q, d_idx, d_d2, s);
    }
}

int nn_dev(pct_cloud *c, int algo, const float *d_q, int64_t Q, uint32_t *d_idx, double *d_d2, hipStream_t s)
{
    if (Q == 0) return PCT_OK;
    PCTCHK(require_reserved(c, Q, "batch"));
    Path path;
    PCTCHK(resolve_algo(c, Op::NN, algo, Q, &path));
    return nn_run(c, path, d_q, Q, d_idx, d_d2, s);
}

// radius counts of a device-resident batch along `path` (resolve_algo, Op::Count or Op::RadiusSearch); Q >= 1, within the reserved size
int count_run(pct_cloud *c, Path path, const float *d_q, const float *d_r, int64_t Q, uint32_t *d_count, hipStream_t s)
{
    HIPCHK(hipMemsetAsync(d_count, 0, sizeof(uint32_t) * Q, s));
    switch (path) {
    case Path::Empty:
        return PCT_OK;
    case Path::Table:        // rolling-map index: a block per query over the buckets of the ball's box
        return launch_frame(c, s, Q, { Work::Device }, [&] {
            ring_count_kernel<<<(int)Q, 256, 0, s>>>(ring_view(c), d_q, d_r, d_count, c->count_work ? c->d_work : nullptr);
        });
    case Path::Grid: {
        const float4 *qs = nullptr;
        const int blocks = ceil_div(Q, 256 / kCoop);      // 8 lanes per query
        // Dom::Ext, yet the launch is a plain one: where the region is left to the kernel no begin event is recorded for this batch, and
        // pct_last_kernel_ms pairs its end event with an older begin (kept as found; looks like an oversight)
        return launch_frame(c, s, Q, { Work::Device, Dom::Ext }, [&] { return bin_queries(c, d_q, Q, s, &qs); },
            [&] {
                with_bool(c->count_work, [&](auto count_work) {
                    count_grid_coop_kernel<decltype(count_work)::value><<<blocks, 256, 0, s>>>(c->G, c->sorted, c->cell_start, d_q, d_r, (uint32_t)Q, qs, d_count,
                                                                                               c->d_work);
                });
            }, no_step);
    }
    default:
        break;
    }
    widen_queries_kernel<<<ceil_div(3 * Q, 256), 256, 0, s>>>(d_q, (uint32_t)(3 * Q), c->d_q64);
    CentreDesc CD{};
    if (Q >= 16 && use_expanded_filter(c, &CD)) {
        // packed-fp32 filter in expanded form + exact fp64 test of whatever may lie inside the ball (brute2.hpp tile_reg_kernel<true>)
        const int64_t ngroups = c->count >> 2;
        const int rblocks = (int)std::max<int64_t>(1, (ngroups + 256 * kRegGroups - 1) / (256 * kRegGroups));
        const int tiles = (int)((Q + kTileQ - 1) / kTileQ);
        const int slices = std::max(1, std::min(tiles, (2048 + rblocks - 1) / rblocks));
        const int rq = ((tiles + slices - 1) / slices) * kTileQ;
        const int rslices = (int)((Q + rq - 1) / rq);
        return launch_frame(c, s, Q, { Work::Untouched },
            [&] { brute2_prep_count_kernel<<<ceil_div(Q, 256), 256, 0, s>>>(CD, d_q, d_r, (uint32_t)Q, c->d_qsorted, c->d_r2); },
            [&] {
                tile_reg_kernel<true><<<dim3(rblocks, rslices), 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)c->count, CD, c->d_qsorted, c->d_q64, c->d_r2, (int)Q, rq,
                                                                             nullptr, nullptr, nullptr, d_count);
            }, no_step);
    }
    square_radii_kernel<<<ceil_div(Q, 256), 256, 0, s>>>(d_r, (uint32_t)Q, c->d_r2);
    const int blocks = stream_blocks(c->count);
    return launch_frame(c, s, Q, { Work::Untouched, Dom::None }, [&] {
        for_each_query_tile(Q, [&](auto qt, int q0, int qcount) {
            count_stream_kernel<decltype(qt)::value><<<blocks, 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)c->count, c->d_q64, c->d_r2, q0, qcount, d_count);
        });
    });
}

int count_dev(pct_cloud *c, int algo, const float *d_q, const float *d_r, int64_t Q, uint32_t *d_count, hipStream_t s)
{
    if (Q == 0) return PCT_OK;
    PCTCHK(require_reserved(c, Q, "batch"));
    Path path;
    PCTCHK(resolve_algo(c, Op::Count, algo, Q, &path));
    return count_run(c, path, d_q, d_r, Q, d_count, s);
}

constexpr size_t kKnnPartEntries = 8u << 20;      // partial lists of the streaming k-NN kernel: 96 MiB; larger batches go through in slices

// k-NN rows of a device-resident batch: d_idx / d_d2 are Q x k
int knn_dev(pct_cloud *c, int algo, const float *d_q, int64_t Q, int k, uint32_t *d_idx, double *d_d2, hipStream_t s)
{
    if (Q == 0) return PCT_OK;
    PCTCHK(require_reserved(c, Q, "batch"));
    if (Q * (int64_t)k > 0xFFFFFFFFll) return fail(PCT_ERR_INVALID, "k-NN batch of %lld x %d entries is too large", (long long)Q, k);
    Path path;
    PCTCHK(resolve_algo(c, Op::KNN, algo, Q, &path));
    switch (path) {
    case Path::Empty:
        fill_empty_kernel<<<ceil_div(Q * k, 256), 256, 0, s>>>(d_idx, d_d2, (uint32_t)(Q * k));
        HIPCHK(hipGetLastError());
        return PCT_OK;
    case Path::Table:        // rolling-map index: a block per query over the expanding cube of buckets
        return launch_frame(c, s, Q, { Work::Device }, [&] {
            with_kcap(k, [&](auto kcap) {
                ring_knn_kernel<decltype(kcap)::value><<<(int)Q, 256, 0, s>>>(ring_view(c), d_q, k, (uint32_t)c->index_base, d_idx, d_d2,
                                                                              c->count_work ? c->d_work : nullptr);
            });
        });
    case Path::Grid: {
        const float4 *recs = nullptr;
        return launch_frame(c, s, Q, { Work::Device }, [&] { return bin_queries(c, d_q, Q, s, &recs); },
            [&] {
                with_kcap(k, [&](auto kcap) {
                    knn_grid_kernel<decltype(kcap)::value><<<ceil_div(Q, kKnnGroups), 256, 0, s>>>(c->G, c->sorted, c->cell_start, d_q, (uint32_t)Q, k,
                                                                                                   (uint32_t)c->index_base, recs, d_idx, d_d2,
                                                                                                   c->count_work ? c->d_work : nullptr);
                });
            }, no_step);
    }
    default:
        break;
    }
    if (!c->d_knn_pd2)
        PCTCHK(regrow(c->knn_part_cap, kKnnPartEntries, part(c->d_knn_pd2, kKnnPartEntries), part(c->d_knn_pidx, kKnnPartEntries)));
    // one block per 4096 points, at most 256: a block's four waves then see enough points for their lists to settle
    const int nparts = (int)std::min<int64_t>(256, std::max<int64_t>(1, (c->count + 4095) / 4096));
    const int64_t qslice = std::max<int64_t>(kKnnTile, (int64_t)(c->knn_part_cap / ((size_t)nparts * (size_t)k)) / kKnnTile * kKnnTile);
    return launch_frame(c, s, Q, { Work::EveryPoint }, [&] {
        for (int64_t off = 0; off < Q; off += qslice) {
            const int qn = (int)std::min<int64_t>(qslice, Q - off);
            with_kcap(k, [&](auto kcap) {
                knn_stream_kernel<decltype(kcap)::value><<<dim3(nparts, ceil_div(qn, kKnnTile)), 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)c->count, d_q + 3 * off, qn, k,
                                                                                                              c->d_knn_pd2, c->d_knn_pidx);
            });
            knn_merge_kernel<<<qn, 64, 0, s>>>(c->d_knn_pd2, c->d_knn_pidx, nparts, k, (uint32_t)c->index_base, d_idx + off * k, d_d2 + off * k);
        }
    });
}

// ---- segment queries (segment.hpp) -------------------------------------------------------------------------------------------
// what a batch measures on its rows: the nearest row's (d2, s) | the first blocker's entry parameter t of a swept sphere ("Segment
// sweeps": t travels in d2's place, d_reach holds the radii, there is no s)
enum class SegMeasure { Nearest, Sweep };

// nearest row to every segment of a device-resident batch (d_seg: Q x 6) -- or, for a sweep, the row that stops the sphere, its t in
// d_d2; d_reach == nullptr: reach_all for every segment (a sweep always has its d_reach).  d_d2 / d_s may be NULL.  Q >= 1, within
// the reserved batch size.  path: from resolve_algo(Op::Segment) -- the rolling-map index or the streaming form.
int segment_run(pct_cloud *c, Path path, SegMeasure measure, const double *d_seg, const double *d_reach, double reach_all, int64_t Q,
                uint32_t *d_idx, double *d_d2, double *d_s, hipStream_t s)
{
    const bool sweep = measure == SegMeasure::Sweep;
    switch (path) {
    case Path::Empty:
        if (sweep) sweep_fill_none_kernel<<<ceil_div(Q, 256), 256, 0, s>>>(d_seg, d_reach, d_idx, d_d2, (uint32_t)Q);
        else segment_fill_none_kernel<<<ceil_div(Q, 256), 256, 0, s>>>(d_idx, d_d2, d_s, (uint32_t)Q);
        HIPCHK(hipGetLastError());
        return PCT_OK;
    case Path::Table:        // rolling-map index: a block per segment over the buckets of the capsule's box
        return launch_frame(c, s, Q, { Work::Device }, [&] {
            WorkCounters *work = c->count_work ? c->d_work : nullptr;
            if (sweep) ring_sweep_kernel<<<(int)Q, 256, 0, s>>>(ring_view(c), d_seg, d_reach, (uint32_t)c->index_base, d_idx, d_d2, work);
            else ring_segment_kernel<<<(int)Q, 256, 0, s>>>(ring_view(c), d_seg, d_reach, reach_all, (uint32_t)c->index_base, d_idx, d_d2, d_s, work);
        });
    default:
        break;
    }
    // streaming: slices of part_q segments through the partial buffers; the s partials borrow the filter's candidate distances
    // (part_q x kCandCap doubles, scratch between batches)
    const int parts = (int)std::min<int64_t>(kSegParts, std::max<int64_t>(1, (c->count + 255) / 256));
    return launch_frame(c, s, Q, { Work::EveryPoint }, [&] {
        for (int64_t off = 0; off < Q; off += c->part_q) {
            const int qn = (int)std::min<int64_t>(c->part_q, Q - off);
            const dim3 grid(parts, ceil_div(qn, kSegTile));
            const double *seg = d_seg + 6 * off, *reach = d_reach ? d_reach + off : nullptr;
            double *out_d2 = d_d2 ? d_d2 + off : nullptr;
            if (sweep) {             // two partials, (t, index): there is no third
                segment_stream_kernel<true><<<grid, 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)c->count, seg, reach, reach_all, (uint32_t)qn, c->d_part_d2,
                                                                 c->d_part_idx, nullptr);
                segment_finish_kernel<true><<<qn, 64, 0, s>>>(c->d_part_d2, c->d_part_idx, nullptr, (uint32_t)parts, (uint32_t)c->index_base, seg, reach,
                                                              d_idx + off, out_d2, nullptr);
            } else {
                segment_stream_kernel<false><<<grid, 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)c->count, seg, reach, reach_all, (uint32_t)qn, c->d_part_d2,
                                                                  c->d_part_idx, c->d_cand_d2);
                segment_finish_kernel<false><<<qn, 64, 0, s>>>(c->d_part_d2, c->d_part_idx, c->d_cand_d2, (uint32_t)parts, (uint32_t)c->index_base, nullptr,
                                                               nullptr, d_idx + off, out_d2, d_s ? d_s + off : nullptr);
            }
        }
    });
}

// ---- radius search with lists (rsearch.hpp) ----------------------------------------------------------------------------------
// scan / cursor / queue workspaces, sized with the query workspaces (pct_cloud_reserve_queries)
int rs_ensure_work(pct_cloud *c)
{
    if (c->rs_qcap >= c->qcap && c->rs_off) return PCT_OK;
    PCTCHK(may_grow(c, Wait::Nothing, nullptr, "the list-search workspaces"));
    const size_t q = (size_t)std::max<int64_t>(c->qcap, 256);
    return regrow(c->rs_qcap, q, part(c->rs_off, q + 1), part(c->rs_tiles, q / kRsScanTile + 2), part(c->rs_cursor, q), part(c->rs_queue, q + 1));
}

// room for n entries in L's d2 and, where wanted, idx and s (grow-only; a failed growth leaves none, and a regrowth drops the idx or
// s that its call does not want)
int ensure_lists(pct_cloud *c, ListStore &L, size_t n, bool want_idx, bool want_s)
{
    if (n == 0 || (n <= L.cap && (!want_idx || L.idx) && (!want_s || L.s))) return PCT_OK;
    char what[64];
    std::snprintf(what, sizeof what, "the %s lists", L.what);
    PCTCHK(may_grow(c, Wait::Nothing, nullptr, what));
    n = std::max(n, L.cap);
    return regrow(L.cap, n, part(L.d2, n), want_idx ? part(L.idx, n) : dropped(L.idx), want_s ? part(L.s, n) : dropped(L.s));
}

// entries [first, first + n) of L's last result to the host; idx, d2 or s may be NULL
int read_lists(const ListStore &L, int64_t first, int64_t n, uint32_t *idx, double *d2, double *s)
{
    if (!L.valid) return fail(PCT_ERR_INVALID, "no %s result to read (none yet, or the cloud changed since)", L.what);
    if (first < 0 || n < 0 || first > L.total || n > L.total - first)
        return fail(PCT_ERR_INVALID, "entries [%lld, %lld) lie outside [0, %lld]", (long long)first, (long long)(first + n), (long long)L.total);
    if (n == 0) return PCT_OK;
    if (idx) HIPCHK(hipMemcpyAsync(idx, L.idx + first, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, g_stream));
    if (d2) HIPCHK(hipMemcpyAsync(d2, L.d2 + first, sizeof(double) * n, hipMemcpyDeviceToHost, g_stream));
    if (s) HIPCHK(hipMemcpyAsync(s, L.s + first, sizeof(double) * n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return PCT_OK;
}

// step 2: c->d_count -> exclusive offsets in d_offsets[Q + 1]; the rows longer than sort_min are queued in c->rs_queue for the sort
// (1: a fill that places its hits in arrival order; kRsShort: the cell-pruned fill, which orders shorter rows itself)
int list_scan(pct_cloud *c, int64_t Q, long long *d_offsets, uint32_t sort_min, hipStream_t s)
{
    if (Q > c->rs_qcap || !d_offsets) return fail(PCT_ERR_INTERNAL, "list search without its workspaces");      // rs_ensure_work comes first
    const int ntiles = ceil_div(Q, kRsScanTile);
    HIPCHK(hipMemsetAsync(c->rs_queue, 0, sizeof(uint32_t), s));
    rs_scan_tiles_kernel<<<ntiles, 256, 0, s>>>(c->d_count, (uint32_t)Q, c->rs_tiles);
    scan_tile_sums_kernel<uint64_t><<<1, 256, 0, s>>>(c->rs_tiles, (uint32_t)ntiles, ScanDoneNothing{});
    rs_scan_final_kernel<<<ntiles, 256, 0, s>>>(c->d_count, (uint32_t)Q, c->rs_tiles, d_offsets, sort_min, c->rs_queue);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

// the tiles of a streaming form with `tile` rows to a block, grid.y within every HIP limit: f(first tile, tiles)
template <typename F>
void for_tile_slices(int64_t Q, int tile, F f)
{
    const int64_t tiles = (Q + tile - 1) / tile;
    for (int64_t t0 = 0; t0 < tiles; t0 += 32768) f((uint32_t)t0, (int)std::min<int64_t>(32768, tiles - t0));
}

// steps 1 and 2 of the radius search: row lengths (the radius-count batch, into c->d_count), then the scan, behind the count's frame.
// path: from resolve_algo(Op::RadiusSearch).  Q >= 1.
int rs_count_scan(pct_cloud *c, Path path, const float *d_q, const float *d_r, int64_t Q, long long *d_offsets, hipStream_t s)
{
    PCTCHK(count_run(c, path, d_q, d_r, Q, c->d_count, s));
    return list_scan(c, Q, d_offsets, path == Path::Grid ? (uint32_t)kRsShort : 1u, s);
}

// step 3: the lists, written only when d_offsets[Q] <= cap (tested on the device), then the queued rows put into final order
int rs_fill_sort(pct_cloud *c, Path path, const float *d_q, const float *d_r, int64_t Q, int order, const long long *d_offsets, int64_t cap,
                 uint32_t *d_idx, double *d_d2, hipStream_t s)
{
    if (path == Path::Empty || cap <= 0) return PCT_OK;      // every row is empty, or there is no room for a single entry
    const bool by_dist = order == PCT_ORDER_DISTANCE;
    if (path == Path::Grid) {
        const float4 *recs = nullptr;
        PCTCHK(bin_queries(c, d_q, Q, s, &recs));
        with_bool(by_dist, [&](auto bd) {
            rs_fill_grid_kernel<decltype(bd)::value><<<ceil_div(Q, kKnnGroups), 256, 0, s>>>(c->G, c->sorted, c->cell_start, d_q, d_r, (uint32_t)Q, recs,
                                                                                             (uint32_t)c->index_base, d_offsets, (long long)cap, d_idx, d_d2);
        });
    } else if (path == Path::Table) {
        // the count's walk once more, behind it on the same stream; its work is added to the count's (pct_last_work)
        with_bool(by_dist, [&](auto bd) {
            ring_fill_kernel<decltype(bd)::value><<<(int)Q, 256, 0, s>>>(ring_view(c), d_q, d_r, (uint32_t)Q, (uint32_t)c->index_base, d_offsets, (long long)cap, d_idx,
                                                                         d_d2, c->count_work ? c->d_work : nullptr);
        });
    } else {
        HIPCHK(hipMemsetAsync(c->rs_cursor, 0, sizeof(uint32_t) * Q, s));
        const int nparts = (int)std::min<int64_t>(256, std::max<int64_t>(1, (c->count + 4095) / 4096));
        for_tile_slices(Q, kRsTile, [&](uint32_t t0, int nt) {
            rs_fill_stream_kernel<<<dim3(nparts, nt), 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)c->count, d_q, d_r, (uint32_t)Q, t0,
                                                                   (uint32_t)c->index_base, d_offsets, (long long)cap, c->rs_cursor, d_idx, d_d2);
        });
    }
    with_bool(by_dist, [&](auto bd) {
        rs_sort_rows_kernel<decltype(bd)::value><<<(int)std::min<int64_t>(Q, 8192), 256, 0, s>>>(c->rs_queue, d_offsets, (uint32_t)Q, (long long)cap, d_idx, d_d2);
    });
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

// ---- capsule search (segment_search.hpp): the radius search's frame over segments ----------------------------------------------
int ss_stream_parts(const pct_cloud *c)
{
    return (int)std::min<int64_t>(kSegParts, std::max<int64_t>(1, (c->count + 255) / 256));
}

// row lengths of a device-resident batch (d_seg: Q x 6, d_reach: Q) into d_count along `path`, then `after` inside the same frame
// (the search's scan -- list_scan with sort_min = 1: all three fills place their hits in arrival order -- and, in the device form,
// its fill).  path: from resolve_algo(Op::Capsule).  Q >= 1, within the reserved batch size.
template <typename E>
int ss_count_run(pct_cloud *c, Path path, const double *d_seg, const double *d_reach, int64_t Q, uint32_t *d_count, hipStream_t s, E after)
{
    HIPCHK(hipMemsetAsync(d_count, 0, sizeof(uint32_t) * Q, s));
    WorkCounters *work = c->count_work ? c->d_work : nullptr;
    switch (path) {
    case Path::Empty:
        return run_step(after);
    case Path::Table:        // a block per segment over the buckets of the capsule's box
        return launch_frame(c, s, Q, { Work::Device }, no_step,
            [&] { ss_ring_count_kernel<<<(int)Q, 256, 0, s>>>(ring_view(c), d_seg, d_reach, d_count, work); }, after);
    case Path::Grid:         // a block per segment over the cells of the capsule's box
        return launch_frame(c, s, Q, { Work::Device }, no_step,
            [&] { ss_grid_count_kernel<<<(int)Q, 256, 0, s>>>(c->G, c->sorted, c->cell_start, d_seg, d_reach, d_count, work); }, after);
    default:
        break;
    }
    const int parts = ss_stream_parts(c);
    return launch_frame(c, s, Q, { Work::EveryPoint }, no_step,
        [&] {
            for_tile_slices(Q, kSegTile, [&](uint32_t t0, int nt) {
                ss_stream_count_kernel<<<dim3(parts, nt), 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)c->count, d_seg, d_reach, (uint32_t)Q, t0, d_count);
            });
        }, after);
}

// the lists, written only when d_offsets[Q] <= cap (tested on the device): the count's walk once more (its work is added to the
// count's, pct_last_work), the queued rows put into final order, then s per entry.  d_d2 is not NULL under PCT_ORDER_DISTANCE.
int ss_fill_sort(pct_cloud *c, Path path, const double *d_seg, const double *d_reach, int64_t Q, int order, const long long *d_offsets,
                 int64_t cap, uint32_t *d_idx, double *d_d2, double *d_s, hipStream_t s)
{
    if (path == Path::Empty || cap <= 0) return PCT_OK;      // every row is empty, or there is no room for a single entry
    WorkCounters *work = c->count_work ? c->d_work : nullptr;
    const uint32_t base = (uint32_t)c->index_base;
    if (path == Path::Table) {
        ss_ring_fill_kernel<<<(int)Q, 256, 0, s>>>(ring_view(c), d_seg, d_reach, (uint32_t)Q, base, d_offsets, (long long)cap, d_idx, d_d2, work);
    } else if (path == Path::Grid) {
        ss_grid_fill_kernel<<<(int)Q, 256, 0, s>>>(c->G, c->sorted, c->cell_start, d_seg, d_reach, (uint32_t)Q, base, d_offsets, (long long)cap, d_idx,
                                                   d_d2, work);
    } else {
        HIPCHK(hipMemsetAsync(c->rs_cursor, 0, sizeof(uint32_t) * Q, s));
        const int parts = ss_stream_parts(c);
        for_tile_slices(Q, kSegTile, [&](uint32_t t0, int nt) {
            ss_stream_fill_kernel<<<dim3(parts, nt), 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)c->count, d_seg, d_reach, (uint32_t)Q, t0, base, d_offsets,
                                                                  (long long)cap, c->rs_cursor, d_idx, d_d2);
        });
    }
    const int blocks = (int)std::min<int64_t>(Q, 8192);
    with_bool(order == PCT_ORDER_DISTANCE, [&](auto bd) {
        rs_sort_rows_kernel<decltype(bd)::value><<<blocks, 256, 0, s>>>(c->rs_queue, d_offsets, (uint32_t)Q, (long long)cap, d_idx, d_d2);
    });
    if (d_s) ss_param_kernel<<<blocks, 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)c->count, d_seg, (uint32_t)Q, base, d_offsets, (long long)cap, d_idx, d_s);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

// ---- free-space polyhedra (segment_polyhedron.hpp): a filter over capsule rows ---------------------------------------------------
// room for the support positions of rows of up to row_cap entries (grow-only; both forms)
int poly_ensure_sup(pct_cloud *c, int64_t row_cap)
{
    if ((size_t)row_cap <= c->pl_sup.capacity() && c->pl_sup) return PCT_OK;
    PCTCHK(may_grow(c, Wait::Nothing, nullptr, "the polyhedron support workspace"));
    return c->pl_sup.reserve((size_t)std::max<int64_t>(row_cap, 1));
}

// the supports of the rows (d_rows[Q + 1], d_row_idx: the capsule search's CSR in PCT_ORDER_DISTANCE, made when d_rows[Q] <= row_cap):
// filter -> count per row (c->d_count) -> scan (d_offsets[Q + 1]).  Q >= 1, within the reserved batch size; rs_ensure_work and
// poly_ensure_sup come first.
int poly_filter_scan(pct_cloud *c, const double *d_seg, int64_t Q, const long long *d_rows, int64_t row_cap, const uint32_t *d_row_idx,
                     long long *d_offsets, hipStream_t s)
{
    poly_filter_kernel<<<(int)Q, 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)c->count, d_seg, (uint32_t)Q, (uint32_t)c->index_base, d_rows,
                                              (long long)row_cap, d_row_idx, c->pl_sup, c->d_count);
    return list_scan(c, Q, d_offsets, 0xFFFFFFFFu, s);       // no row is queued: there is nothing to sort
}

// ... and the lists behind it, written only when d_offsets[Q] <= cap (tested on the device); every entry of d_offsets becomes -1
// instead when the rows were never made
int poly_emit(pct_cloud *c, const double *d_seg, int64_t Q, const long long *d_rows, int64_t row_cap, const uint32_t *d_row_idx,
              long long *d_offsets, int64_t cap, uint32_t *d_idx, double *d_d2, double *d_s, double *d_plane, hipStream_t s)
{
    poly_emit_kernel<<<(int)std::min<int64_t>(Q, 8192), 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)c->count, d_seg, (uint32_t)Q, (uint32_t)c->index_base,
                                                                    d_rows, (long long)row_cap, d_row_idx, c->pl_sup, d_offsets, (long long)cap, d_idx,
                                                                    d_d2, d_s, d_plane);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

InflateParams to_dev(const pct_inflate_params *p)
{
    return InflateParams{ p->start[0], p->start[1], p->start[2], p->sample_range, p->search_margin, p->max_radius };
}

// pts64 (device, Q x 3) -> radius/idx/d2 in the cloud's workspaces
// d_pts: the planner points (device-visible), default the staging buffer; d_out != nullptr: results as records in host-mapped memory
// o_radius / o_idx / o_d2: where the results go (default: the cloud's workspaces)
int inflate_dev(pct_cloud *c, const pct_inflate_params *p, int64_t Q, hipStream_t s, const double *d_pts = nullptr, ExpressOut *d_out = nullptr,
                double *o_radius = nullptr, uint32_t *o_idx = nullptr, double *o_d2 = nullptr)
{
    const InflateParams P = to_dev(p);
    if (!o_radius) o_radius = c->d_radius;
    if (!o_idx) o_idx = c->d_idx;
    if (!o_d2) o_d2 = c->d_d2;
    inflate_prologue_kernel<<<ceil_div(Q, 256), 256, 0, s>>>(P, d_pts ? d_pts : c->d_pts64, (uint32_t)Q, c->d_q, c->d_skip);
    if (c->count > 0) PCTCHK(nn_dev(c, PCT_ALGO_AUTO, c->d_q, Q, o_idx, o_d2, s));
    if (d_out)
        inflate_epilogue_out_kernel<<<ceil_div(Q, 256), 256, 0, s>>>(P, (uint32_t)Q, c->d_skip, c->count == 0 ? 1 : 0, o_idx, o_d2, d_out);
    else
        inflate_epilogue_kernel<<<ceil_div(Q, 256), 256, 0, s>>>(P, (uint32_t)Q, c->d_skip, c->count == 0 ? 1 : 0, o_idx, o_d2, o_radius);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

// ---- host buffers of the batch entry points ------------------------------------------------------------------------------------
// A host batch of Q queries (and radii, r != nullptr) into c->d_q (c->d_r).  Up to kMappedMaxQ queries go through host-mapped memory:
// imported by a kernel here, results exported by a kernel and completion by polling in fetch_results -- no DMA copy, no stream
// synchronise (C2's 4096-query batch: 0.63 -> 0.5x ms).  Larger batches by DMA.  *mapped: which, for fetch_results.
int stage_queries(pct_cloud *c, const float *q, const float *r, int64_t Q, bool *mapped)
{
    *mapped = Q <= kMappedMaxQ && mapped_io_on();
    if (!*mapped) {
        HIPCHK(hipMemcpyAsync(c->d_q, q, sizeof(float) * 3 * Q, hipMemcpyHostToDevice, g_stream));
        if (r) HIPCHK(hipMemcpyAsync(c->d_r, r, sizeof(float) * Q, hipMemcpyHostToDevice, g_stream));
        return PCT_OK;
    }
    PCTCHK(ensure_mapped_io(c, Q));
    std::memcpy(c->mq.host(), q, sizeof(float) * 3 * (size_t)Q);
    if (r) std::memcpy(c->mq.host() + 3 * Q, r, sizeof(float) * (size_t)Q);
    import_floats_kernel<<<ceil_div(3 * Q, 256), 256, 0, g_stream>>>(c->mq, (uint32_t)(3 * Q), c->d_q);
    if (r) import_floats_kernel<<<ceil_div(Q, 256), 256, 0, g_stream>>>(c->mq + 3 * Q, (uint32_t)Q, c->d_r);
    return PCT_OK;
}

// n uint32 results (and doubles, d_f64 != nullptr) back to the host by the transport stage_queries chose (DMA for buffers it did not
// stage), and the wait for them
int fetch_results(pct_cloud *c, bool mapped, const uint32_t *d_u32, uint32_t *u32, const double *d_f64, double *f64, int64_t n)
{
    if (!mapped) {
        HIPCHK(hipMemcpyAsync(u32, d_u32, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, g_stream));
        if (d_f64) HIPCHK(hipMemcpyAsync(f64, d_f64, sizeof(double) * n, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
        return PCT_OK;
    }
    export_results_kernel<<<ceil_div(n, 256), 256, 0, g_stream>>>(d_u32, d_f64, (uint32_t)n, c->mi, d_f64 ? c->md : nullptr, next_signal(c));
    HIPCHK(hipGetLastError());
    PCTCHK(express_wait(c));
    std::memcpy(u32, c->mi.host(), sizeof(uint32_t) * (size_t)n);
    if (d_f64) std::memcpy(f64, c->md.host(), sizeof(double) * (size_t)n);
    return PCT_OK;
}

// the records of an express launch (c->xout.host(), host-mapped) into the caller's arrays; a null array is not wanted
void read_express_out(const pct_cloud *c, int64_t n, double *radius, uint32_t *idx, double *d2)
{
    for (int64_t i = 0; i < n; i++) {
        if (radius) radius[i] = c->xout.host()[i].radius;
        if (idx) idx[i] = c->xout.host()[i].idx;
        if (d2) d2[i] = c->xout.host()[i].d2;
    }
}

// (re)capture p's graph: `enqueue` queues the batch on the library's stream, which is under capture meanwhile
template <typename F>
int plan_capture(pct_plan *p, F enqueue)
{
    pct_cloud *c = p->c;
    if (p->exec) { (void)hipGraphExecDestroy(p->exec); p->exec = nullptr; }
    if (p->graph) { (void)hipGraphDestroy(p->graph); p->graph = nullptr; }
    HIPCHK(hipStreamSynchronize(g_stream));
    hipError_t e = hipStreamBeginCapture(g_stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return fail(PCT_ERR_HIP, "hipStreamBeginCapture: %s", hipGetErrorString(e));
    c->capturing = true;
    const int st = enqueue();
    c->capturing = false;
    e = hipStreamEndCapture(g_stream, &p->graph);
    if (st != PCT_OK) return st;
    if (e != hipSuccess || !p->graph) return fail(PCT_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
    e = hipGraphInstantiate(&p->exec, p->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) return fail(PCT_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
    p->generation = c->generation;
    return PCT_OK;
}

// ---- host side of the sampled Bezier check, shared by its entry points (pinned bit for bit by tests/test_gpu_bezier_paths.py) ----
int bezier_check_orders(const pct_bezier_traj *traj)
{
    for (int i = 0; i < traj->nseg; i++)
        if (!bezier_order_ok(traj->orders[i], traj->row_stride))
            return fail(PCT_ERR_INVALID, "segment %d: order %d unsupported", i, traj->orders[i]);
    return PCT_OK;
}

// the layout of a pct_bezier_batch as the host forms demand it: seg_offsets[0] == 0, strictly ascending offsets, sound orders
// (`who`: the entry point, for the message)
int bezier_check_batch_layout(const pct_bezier_batch *batch, const char *who)
{
    if (batch->B > 0 && batch->seg_offsets[0] != 0) return fail(PCT_ERR_INVALID, "%s: seg_offsets[0] = %d, not 0", who, (int)batch->seg_offsets[0]);
    for (int64_t b = 0; b < batch->B; b++) {
        const int32_t s0 = batch->seg_offsets[b], s1 = batch->seg_offsets[b + 1];
        if (s1 <= s0) return fail(PCT_ERR_INVALID, "%s: seg_offsets not strictly ascending at trajectory %lld", who, (long long)b);
        for (int32_t i = s0; i < s1; i++)
            if (!bezier_order_ok(batch->orders[i], batch->row_stride))
                return fail(PCT_ERR_INVALID, "%s: segment %d: order %d unsupported", who, (int)i, (int)batch->orders[i]);
    }
    return PCT_OK;
}

// coefficients, segment times and orders into the cloud's device copies (grow-only) on stream s.  dev_form: earlier work on the
// caller's streams may still read the old buffers, so the device is synchronised before they grow; the host form's earlier
// work has been waited for by the call that queued it.
int bezier_stage_coef(pct_cloud *c, const pct_bezier_traj *traj, hipStream_t s, bool dev_form)
{
    const size_t ncoef = (size_t)traj->nseg * traj->row_stride, nseg = (size_t)traj->nseg;
    if (ncoef > c->d_coef.capacity() || nseg > c->seg_cap) {
        if (dev_form) HIPCHK(hipDeviceSynchronize());
        PCTCHK(c->d_coef.reserve(ncoef));
        if (nseg > c->seg_cap) PCTCHK(regrow(c->seg_cap, nseg, part(c->d_segtime, nseg), part(c->d_orders, nseg)));
    }
    HIPCHK(hipMemcpyAsync(c->d_coef, traj->polycoef, sizeof(double) * ncoef, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_segtime, traj->seg_time, sizeof(double) * nseg, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_orders, traj->orders, sizeof(int) * nseg, hipMemcpyHostToDevice, s));
    return PCT_OK;
}

// the staged check of the staged coefficients on stream s: cleared positions, the samples, their inflation, the first hit.
// d_pos and d_radius are the caller's or the cloud's workspaces; a null d_idx / d_d2 means the cloud's.
int bezier_staged_enqueue(pct_cloud *c, const pct_bezier_traj *traj, const pct_inflate_params *p, double t_start, double stop_time, double dt,
                          int64_t cap, hipStream_t s, double *d_pos, double *d_radius, uint32_t *d_idx, double *d_d2, long long *d_first_hit,
                          int *d_nsamples)
{
    HIPCHK(hipMemsetAsync(d_pos, 0, sizeof(double) * 3 * cap, s));
    BezierDesc B{ c->d_coef, c->d_segtime, c->d_orders, (int)traj->row_stride, traj->nseg, t_start, stop_time, dt, (int)cap };
    const size_t smem = (size_t)cap * (sizeof(double) + sizeof(int));
    bezier_samples_kernel<<<1, 256, smem, s>>>(B, d_pos, d_nsamples);
    PCTCHK(inflate_dev(c, p, cap, s, d_pos, nullptr, d_radius, d_idx, d_d2));
    first_hit_kernel<<<1, 256, 0, s>>>(d_radius, d_nsamples, (int)cap, d_first_hit);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

}  // namespace

#include "ring_host.inc"

// ======================================================================================
//  C ABI
// ======================================================================================
namespace pct_internal {
hipStream_t stream() { return g_stream; }
int require_init() { return ::require_init(); }

// ---- the three kinds of memory (engine_internal.hpp); the only HIP allocation and free calls of the engine's host side ----
namespace {
std::atomic<int64_t> g_live_blocks{ 0 }, g_live_bytes{ 0 };
void count_block(size_t bytes, int sign)
{
    g_live_blocks.fetch_add(sign, std::memory_order_relaxed);
    g_live_bytes.fetch_add(sign * (int64_t)bytes, std::memory_order_relaxed);
}
}  // namespace

int DeviceMem::alloc(size_t bytes, void **host, void **dev)
{
    *host = *dev = nullptr;
    const hipError_t e = hipMalloc(dev, bytes);
    if (e != hipSuccess) { *dev = nullptr; return fail(PCT_ERR_ALLOC, "hipMalloc(%zu bytes) -> %s", bytes, hipGetErrorString(e)); }
    count_block(bytes, 1);
    return PCT_OK;
}
void DeviceMem::release(void *, void *dev, size_t bytes)
{
    (void)hipFree(dev);
    count_block(bytes, -1);
}

int PinnedMem::alloc(size_t bytes, void **host, void **dev)
{
    *host = *dev = nullptr;
    const hipError_t e = hipHostMalloc(host, bytes, hipHostMallocDefault);
    if (e != hipSuccess) { *host = nullptr; return fail(PCT_ERR_ALLOC, "hipHostMalloc(%zu bytes) -> %s", bytes, hipGetErrorString(e)); }
    *dev = *host;
    count_block(bytes, 1);
    return PCT_OK;
}
void PinnedMem::release(void *host, void *, size_t bytes)
{
    (void)hipHostFree(host);
    count_block(bytes, -1);
}

int MappedMem::alloc(size_t bytes, void **host, void **dev)
{
    *host = *dev = nullptr;
    hipError_t e = hipHostMalloc(host, bytes, hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer(dev, *host, 0);
    if (e != hipSuccess) {
        if (*host) (void)hipHostFree(*host);
        *host = *dev = nullptr;
        return fail(PCT_ERR_ALLOC, "hipHostMalloc(mapped, %zu bytes) -> %s", bytes, hipGetErrorString(e));
    }
    count_block(bytes, 1);
    return PCT_OK;
}
void MappedMem::release(void *host, void *, size_t bytes)
{
    (void)hipHostFree(host);
    count_block(bytes, -1);
}
int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace pct_internal

extern "C" {

const char *pct_last_error(void) { return g_err; }

int pct_debug_live_buffers(int64_t *blocks, int64_t *bytes)
{
    if (!blocks || !bytes) return fail(PCT_ERR_INVALID, "null output");
    *blocks = pct_internal::g_live_blocks.load(std::memory_order_relaxed);
    *bytes = pct_internal::g_live_bytes.load(std::memory_order_relaxed);
    return PCT_OK;
}


int pct_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int pct_init(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(PCT_ERR_NO_DEVICE, "no HIP device (%s); this library has no host fallback", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(PCT_ERR_INVALID, "device %d out of range (0..%d)", device, n - 1);
    HIPCHK(hipSetDevice(device));
    if (g_stream && g_device != device) { (void)hipStreamDestroy(g_stream); g_stream = nullptr; }
    if (!g_stream) HIPCHK(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
    g_device = device;
    return PCT_OK;
}

int pct_sync(void)
{
    PCTCHK(require_init());
    HIPCHK(hipDeviceSynchronize());    // the library's stream and any caller stream handed to the *_dev entry points
    return PCT_OK;
}

static int cloud_create_impl(int64_t capacity, bool host_mapped, pct_cloud **out)
{
    if (!out || capacity < 0 || capacity > 0xFFFFFFF0ll) return fail(PCT_ERR_INVALID, "bad capacity");
    PCTCHK(require_init());
    pct_cloud *c = new (std::nothrow) pct_cloud();
    if (!c) return fail(PCT_ERR_ALLOC, "host allocation failed");
    c->cap = capacity;
    c->cap4 = (capacity + 3) & ~3ll;
    c->host_mapped = host_mapped;
    int s = PCT_OK;
    for (int k = 0; k < 3 && !s; k++) s = host_mapped ? c->xyz_map[k].reset((size_t)c->cap4 + 4) : c->xyz_dev[k].reset((size_t)c->cap4 + 4);
    if (host_mapped) {
        c->hx = c->xyz_map[0].host(); c->hy = c->xyz_map[1].host(); c->hz = c->xyz_map[2].host();
        c->x = c->xyz_map[0]; c->y = c->xyz_map[1]; c->z = c->xyz_map[2];
    } else {
        c->x = c->xyz_dev[0]; c->y = c->xyz_dev[1]; c->z = c->xyz_dev[2];
    }
    if (!s) s = c->d_work.reset(kWorkSlots);
    if (!s) s = c->d_bbox.reset((size_t)1024 * 6);
    if (!s) s = c->d_gbcheck.reset(kGbCheckSlots);
    if (!s) s = c->h_gbcheck.reset(kGbCheckSlots);
    if (!s) s = c->xout.reset(kExpressMaxQ);
    if (!s) s = c->xin.reset(3 * kExpressMaxQ);
    if (!s) s = c->xr.reset(kExpressMaxQ);
    if (!s) s = c->xids.reset(kExpressIdsCap);
    if (!s) s = c->xseq.ensure(16);
    if (!s) s = c->d_xcounter.reset(16);
    if (!s && hipMemset(c->d_xcounter, 0, 16 * sizeof(uint32_t)) != hipSuccess) s = fail(PCT_ERR_HIP, "hipMemset failed");
    if (s) {
        pct_cloud_destroy(c);
        return PCT_ERR_ALLOC;
    }
    bool ring_ok = true;
    for (hipEvent_t &e : c->dom_ring) ring_ok = ring_ok && hipEventCreate(&e) == hipSuccess;
    c->ev2 = c->dom_ring[0];
    c->ev3 = c->dom_ring[1];
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess || !ring_ok) {
        pct_cloud_destroy(c);
        return fail(PCT_ERR_HIP, "hipEventCreate failed");
    }
    *out = c;
    return PCT_OK;
}

int pct_cloud_create(int64_t capacity, pct_cloud **out) { return cloud_create_impl(capacity, false, out); }

int pct_cloud_create_small(int64_t capacity, pct_cloud **out)
{
    if (capacity > (1ll << 22)) return fail(PCT_ERR_INVALID, "small (host-mapped) clouds hold at most 4M points");
    return cloud_create_impl(capacity, true, out);
}

int pct_cloud_destroy(pct_cloud *c)
{
    if (!c) return PCT_OK;
    if (g_stream) (void)hipStreamSynchronize(g_stream);
    if (c->ev_mut) (void)hipEventDestroy(c->ev_mut);
    replan_ctx_free(c->rp);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (hipEvent_t e : c->dom_ring) if (e) (void)hipEventDestroy(e);
    delete c;
    return PCT_OK;
}

int64_t pct_cloud_size(const pct_cloud *c) { return c ? c->count : 0; }
int64_t pct_cloud_capacity(const pct_cloud *c) { return c ? c->cap : 0; }

int pct_cloud_set_index_base(pct_cloud *c, int64_t base)
{
    if (!c || base < 0 || base + c->cap > 0xFFFFFFF0ll) return fail(PCT_ERR_INVALID, "bad index base");
    c->index_base = base;
    return PCT_OK;
}

int pct_cloud_upload_aos(pct_cloud *c, const void *pts, int64_t n, int64_t stride_bytes)
{
    if (!c || n < 0 || (n > 0 && !pts) || stride_bytes < 12 || (stride_bytes & 3)) return fail(PCT_ERR_INVALID, "bad upload arguments");
    if (n > c->cap) return fail(PCT_ERR_CAPACITY, "%lld points > capacity %lld", (long long)n, (long long)c->cap);
    drop_grid(c);
    PCTCHK(upload_range(c, pts, n, stride_bytes, 0));
    HIPCHK(hipStreamSynchronize(g_stream));    // the host buffer is the caller's again
    c->count = n;
    c->ring_next = n % std::max<int64_t>(c->cap, 1);
    c->ring_removed_any = false;
    return after_replace(c);
}

// sensor_msgs/PointCloud2 (rcvPointCloudCallBack, sim_planning_demo.cpp:159-167): a byte blob of `n` records of
// `point_step` bytes whose FLOAT32 fields x, y, z sit at arbitrary byte offsets.  Records are repacked on the host
// into 12-byte xyz (one pass; the message is pageable host memory anyway) and take the packed upload path.
int pct_cloud_upload_fields(pct_cloud *c, const void *data, int64_t n, int64_t point_step, int64_t off_x, int64_t off_y, int64_t off_z)
{
    if (!c || n < 0 || (n > 0 && !data) || point_step < 4 || off_x < 0 || off_y < 0 || off_z < 0 || off_x + 4 > point_step ||
        off_y + 4 > point_step || off_z + 4 > point_step)
        return fail(PCT_ERR_INVALID, "bad upload_fields arguments");
    if (off_x == 0 && off_y == 4 && off_z == 8 && (point_step & 3) == 0 && point_step >= 12) return pct_cloud_upload_aos(c, data, n, point_step);
    std::vector<float> packed;
    try { packed.resize((size_t)3 * n); } catch (const std::bad_alloc &) { return fail(PCT_ERR_ALLOC, "host allocation failed"); }
    const unsigned char *src = static_cast<const unsigned char *>(data);
    for (int64_t i = 0; i < n; i++) {
        std::memcpy(&packed[3 * i], src + i * point_step + off_x, 4);
        std::memcpy(&packed[3 * i + 1], src + i * point_step + off_y, 4);
        std::memcpy(&packed[3 * i + 2], src + i * point_step + off_z, 4);
    }
    return pct_cloud_upload_aos(c, packed.data(), n, 12);
}

int pct_cloud_upload_soa_dev(pct_cloud *c, const float *d_x, const float *d_y, const float *d_z, int64_t n)
{
    if (!c || n < 0 || (n > 0 && (!d_x || !d_y || !d_z))) return fail(PCT_ERR_INVALID, "bad upload arguments");
    if (n > c->cap) return fail(PCT_ERR_CAPACITY, "%lld points > capacity %lld", (long long)n, (long long)c->cap);
    drop_grid(c);
    if (n) {
        HIPCHK(hipMemcpyAsync(c->x, d_x, sizeof(float) * n, hipMemcpyDeviceToDevice, g_stream));
        HIPCHK(hipMemcpyAsync(c->y, d_y, sizeof(float) * n, hipMemcpyDeviceToDevice, g_stream));
        HIPCHK(hipMemcpyAsync(c->z, d_z, sizeof(float) * n, hipMemcpyDeviceToDevice, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
    }
    c->count = n;
    c->ring_next = n % std::max<int64_t>(c->cap, 1);
    c->ring_removed_any = false;
    return after_replace(c);
}

}  // extern "C"

namespace {

// append on a cloud without a live rolling-map table: plain stores into the ring slots; a rolling-map cloud gets its table from this first data
int append_unindexed(pct_cloud *c, const void *pts, int64_t n, int64_t stride_bytes)
{
    const int64_t first = std::min(n, c->cap - c->ring_next);
    PCTCHK(upload_range(c, pts, first, stride_bytes, c->ring_next));
    HIPCHK(hipStreamSynchronize(g_stream));   // the staging buffer is reused by the wrapped part
    if (first < n) {
        PCTCHK(upload_range(c, static_cast<const unsigned char *>(pts) + first * stride_bytes, n - first, stride_bytes, 0));
        HIPCHK(hipStreamSynchronize(g_stream));
    }
    c->ring_next = (c->ring_next + n) % c->cap;
    c->count = std::min(c->cap, c->count + n);
    return after_replace(c);
}

// ---- the list searches: radius search (rsearch.hpp) and capsule search (segment_search.hpp) --------------------------------------
// The host form behind its argument checks and resolve_algo: stage the inputs, count and scan -- asked twice after an overrun, before
// the lists are sized: count and fill must see the same table -- the one host read (the total sizes the lists), fill and sort, wait,
// publish in L.  name: the search, for the capacity message.  What differs between the two searches stays with the callers.
template <typename Stage, typename CountScan, typename FillSort>
int list_search_host(pct_cloud *c, ListStore &L, const char *name, bool want_s, int64_t Q, int64_t *offsets, int64_t *total, Stage stage,
                     CountScan count_scan, FillSort fill_sort)
{
    L.valid = false;
    L.total = 0;
    offsets[0] = 0;
    *total = 0;
    if (Q == 0) { L.valid = true; return PCT_OK; }
    PCTCHK(pct_cloud_reserve_queries(c, Q));
    PCTCHK(rs_ensure_work(c));                               // before c->rs_off is handed on
    PCTCHK(run_step(stage));
    PCTCHK(ask_twice_after_overrun(c, [&]() -> int {
        PCTCHK(run_step(count_scan));
        HIPCHK(hipMemcpyAsync(offsets, c->rs_off, sizeof(int64_t) * (Q + 1), hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
        return PCT_OK;
    }));
    *total = offsets[Q];
    if (*total > 0xFFFFFFFFll) return fail(PCT_ERR_CAPACITY, "%s lists %lld entries, more than 2^32 - 1", name, (long long)*total);
    PCTCHK(ensure_lists(c, L, (size_t)*total, true, want_s));
    PCTCHK(run_step(fill_sort));
    HIPCHK(hipStreamSynchronize(g_stream));
    L.total = *total;
    L.valid = true;
    return PCT_OK;
}

// The device forms' prelude behind resolve_algo.  Q == 0: the empty CSR, and the caller returns.  Otherwise the batch must fit the
// reserved size; under PCT_ORDER_DISTANCE without a d_d2 the sort key needs a home -- L's d2, grown to cap entries (want_idx: idx
// with it), which ends the host form's last result -- and the scan's workspaces and the order behind the cloud's mutations follow.
int list_search_dev_prelude(pct_cloud *c, ListStore &L, bool want_idx, int64_t Q, int order, int64_t *d_offsets, int64_t cap, double **d_d2,
                            hipStream_t s)
{
    if (Q == 0) {
        HIPCHK(hipMemsetAsync(d_offsets, 0, sizeof(int64_t), s));
        return PCT_OK;
    }
    PCTCHK(require_reserved(c, Q, "batch"));
    if (order == PCT_ORDER_DISTANCE && !*d_d2 && cap > 0) {
        L.valid = false;
        PCTCHK(ensure_lists(c, L, (size_t)cap, want_idx, false));
        *d_d2 = L.d2;
    }
    PCTCHK(rs_ensure_work(c));
    return order_after_mutations(c, s);
}

// ---- the per-segment host forms ---------------------------------------------------------------------------------------------
// where a per-segment result goes: Q elements of `elem` bytes from `dev` to `host` (NULL: not asked for)
struct SegOut { void *host; const void *dev; size_t elem; };

// segments and reaches (either may be NULL: not staged) into c->d_seg / c->d_r2
int stage_segments(pct_cloud *c, const double *seg, const double *reach, int64_t Q)
{
    if (seg) HIPCHK(hipMemcpyAsync(c->d_seg, seg, sizeof(double) * 6 * Q, hipMemcpyHostToDevice, g_stream));
    if (reach) HIPCHK(hipMemcpyAsync(c->d_r2, reach, sizeof(double) * Q, hipMemcpyHostToDevice, g_stream));
    return PCT_OK;
}

// The host form of a per-segment answer behind its argument checks, resolve_algo and pct_cloud_reserve_queries (the outputs name the
// workspaces it sizes); Q >= 1.  `run` queues the batch on g_stream
// from the staged inputs and is asked once more when the table lost points (overflow-queue overrun: refiled); the outputs are copied
// back and waited for once.  empty_msg: the entry's PCT_ERR_EMPTY message when the cloud holds no point, NULL when it answers PCT_OK.
template <typename Run>
int segment_host_form(pct_cloud *c, const double *seg, const double *reach, int64_t Q, std::initializer_list<SegOut> outs, const char *empty_msg,
                      Run run)
{
    PCTCHK(stage_segments(c, seg, reach, Q));
    PCTCHK(ask_twice_after_overrun(c, [&]() -> int {
        PCTCHK(run_step(run));
        for (const SegOut &o : outs)
            if (o.host) HIPCHK(hipMemcpyAsync(o.host, o.dev, o.elem * (size_t)Q, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
        return PCT_OK;
    }));
    if (empty_msg) return fail(PCT_ERR_EMPTY, "%s", empty_msg);
    return PCT_OK;
}

// the device form of either measure behind its argument check; d_d2 receives t for a sweep, which has no s
int segment_batch_dev(pct_cloud *c, int algo, SegMeasure measure, const double *d_seg, const double *d_reach, int64_t Q, uint32_t *d_idx,
                      double *d_d2, double *d_s, hipStream_t s)
{
    Path path;
    PCTCHK(resolve_algo(c, Op::Segment, algo, Q, &path));
    if (Q == 0) return PCT_OK;
    PCTCHK(require_reserved(c, Q, "batch"));
    PCTCHK(order_after_mutations(c, s));
    return segment_run(c, path, measure, d_seg, d_reach, 0.0, Q, d_idx, d_d2, d_s, s);
}

// the host form of either measure behind its argument check; empty_msg: the entry's own PCT_ERR_EMPTY message
int segment_batch_host(pct_cloud *c, int algo, SegMeasure measure, const double *seg, const double *reach, int64_t Q, uint32_t *idx, double *d2,
                       double *s, const char *empty_msg)
{
    PCTCHK(ring_finish_pending(c));              // rolling map: an append in flight is finished first and the answer sees its frame
    Path path;
    PCTCHK(resolve_algo(c, Op::Segment, algo, Q, &path));
    if (Q == 0) return PCT_OK;
    PCTCHK(pct_cloud_reserve_queries(c, Q));
    double *d_s = measure == SegMeasure::Sweep ? nullptr : (double *)c->d_radius;
    return segment_host_form(c, seg, reach, Q, { { idx, c->d_idx, sizeof(uint32_t) }, { d2, c->d_d2, sizeof(double) }, { s, d_s, sizeof(double) } },
                             path == Path::Empty ? empty_msg : nullptr,
                             [&] { return segment_run(c, path, measure, c->d_seg, c->d_r2, 0.0, Q, c->d_idx, c->d_d2, d_s, g_stream); });
}

// ---- the certified Bezier check (bezier_certify.hpp; contract: pct_engine.h, "Certified Bezier check"): its rooms and its rounds ----
// what a call certifies and where its answers go
struct BcRun {
    BcDesc D;
    double margin;
    int max_depth;
    int64_t piece_cap;
    Path path;                       // of the chord test: resolve_algo(Op::Capsule)
    pct_traj_certificate *cert;      // device memory, B entries
    long long *stats;                // device memory, 3 entries, or NULL
    BcWinDesc W{};                   // the window forms: W.win != NULL
};

template <typename T>
int bc_reserve(pct_cloud *c, DevBuf<T> &buf, size_t need, hipStream_t s)
{
    if (need <= buf.capacity() && buf) return PCT_OK;
    PCTCHK(may_grow(c, Wait::Device, &s, "the certified check's buffers"));
    return buf.reserve(pow2_at_least<size_t>(256, need));
}

// room for `pieces` pieces in set `side`
int bc_room(pct_cloud *c, int side, int64_t pieces, hipStream_t s)
{
    PCTCHK(bc_reserve(c, c->bc_poly[side], (size_t)pieces * kBcPoly, s));
    return bc_reserve(c, c->bc_meta[side], (size_t)pieces, s);
}

// room for a round over nslots slots: its flags and tile sums
int bc_round_room(pct_cloud *c, int64_t nslots, hipStream_t s)
{
    PCTCHK(bc_reserve(c, c->bc_flag, (size_t)nslots, s));
    return bc_reserve(c, c->bc_tile, (size_t)ceil_div(nslots, kBcTile) + 1, s);
}

// room for the state of B trajectories and the control words
int bc_traj_room(pct_cloud *c, int64_t B, hipStream_t s)
{
    PCTCHK(bc_reserve(c, c->bc_traj, (size_t)B, s));
    return bc_reserve(c, c->bc_ctl, 1, s);
}

// defaults, validity and the pieces of depth 0 in set 0; seg_lanes: the segments (the host form) or piece_cap (the device form, whose
// lanes guard on seg_offsets[B])
// behind the init kernel of either call: validity and the pieces of depth 0 in set 0 -- the segments themselves, or (W.win) their
// parts inside each trajectory's window
void bc_seed_pieces(pct_cloud *c, const BcDesc &D, const BcWinDesc &W, int64_t piece_cap, int64_t seg_lanes, hipStream_t s)
{
    if (seg_lanes > 0) bc_valid_kernel<<<ceil_div(seg_lanes, 256), 256, 0, s>>>(D, (long long)piece_cap, c->bc_traj);
    if (W.win) {
        bc_window_kernel<<<ceil_div(seg_lanes + D.B, 256), 256, 0, s>>>(D, W, (long long)piece_cap, (long long)seg_lanes, c->bc_traj);
        if (seg_lanes > 0)
            bc_seed_window_kernel<<<ceil_div(seg_lanes, 256), 256, 0, s>>>(D, (long long)piece_cap, c->bc_traj, W.win, c->bc_poly[0], c->bc_meta[0]);
    } else if (seg_lanes > 0) {
        bc_seed_kernel<<<ceil_div(seg_lanes, 256), 256, 0, s>>>(D, (long long)piece_cap, c->bc_traj, c->bc_poly[0], c->bc_meta[0]);
    }
}

int bc_seed(pct_cloud *c, const BcRun &R, int64_t seg_lanes, hipStream_t s)
{
    bc_init_kernel<<<ceil_div(R.D.B + 1, 256), 256, 0, s>>>(R.D, (long long)R.piece_cap, R.cert, c->bc_traj, c->bc_ctl);
    bc_seed_pieces(c, R.D, R.W, R.piece_cap, seg_lanes, s);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

// the nearest-neighbour path of the index that `path` (resolve_algo, Op::Capsule) names: the end test of the certified check and
// both queries of the clearance
int bc_nn_path(pct_cloud *c, Path path, int64_t Q, Path *nn)
{
    *nn = Path::Empty;
    if (path == Path::Empty) return PCT_OK;
    return resolve_algo(c, Op::NN, path == Path::Table ? PCT_ALGO_RING : path == Path::Grid ? PCT_ALGO_GRID : PCT_ALGO_STREAM, Q, nn);
}

// One round over the first nslots slots of set (round & 1): the queries into the cloud's workspaces (segments in d_seg, reaches in
// d_r2, the 2 * nslots ends in d_q; 2 * nslots <= c->qcap), the capsule count and the nearest-neighbour batch on the index of R.path,
// then classification, compaction and the halving into the other set.
int bc_round(pct_cloud *c, const BcRun &R, int round, int64_t nslots, hipStream_t s)
{
    const int cur = round & 1;
    const uint32_t n = (uint32_t)nslots;
    bc_geometry_kernel<<<ceil_div(nslots, 256), 256, 0, s>>>(c->bc_poly[cur], c->bc_meta[cur], c->bc_ctl, n, R.margin, c->d_seg, c->d_r2, c->d_q);
    HIPCHK(hipGetLastError());
    PCTCHK(ss_count_run(c, R.path, c->d_seg, c->d_r2, nslots, c->d_count, s, no_step));
    Path nn;
    PCTCHK(bc_nn_path(c, R.path, 2 * nslots, &nn));
    PCTCHK(nn_run(c, nn, c->d_q, 2 * nslots, c->d_idx, c->d_d2, s));
    bc_classify_kernel<<<ceil_div(nslots, 256), 256, 0, s>>>(c->bc_meta[cur], c->bc_ctl, n, R.margin, round, c->d_count, c->d_d2, R.cert, c->bc_traj, c->bc_flag);
    const int ntiles = ceil_div(nslots, kBcTile);
    (R.W.win ? bc_mark_kernel<true> : bc_mark_kernel<false>)<<<ntiles, kBcTile, 0, s>>>(c->bc_meta[cur], c->bc_ctl, n, round, R.max_depth, c->d_idx, c->d_d2, R.cert,
                                                                                        c->bc_traj, c->bc_flag, c->bc_tile, R.W.win);
    scan_tile_sums_kernel<uint32_t><<<1, 256, 0, s>>>(c->bc_tile, (uint32_t)ntiles, BcScanDone{ c->bc_ctl, (uint32_t)R.piece_cap });
    if (round < R.max_depth)
        bc_split_kernel<<<ceil_div(2 * nslots, 256), 256, 0, s>>>(c->bc_poly[cur], c->bc_meta[cur], c->bc_poly[cur ^ 1], c->bc_meta[cur ^ 1], c->bc_flag, c->bc_tile,
                                                                 c->bc_ctl, n, c->bc_traj);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

int bc_finish(pct_cloud *c, const BcRun &R, hipStream_t s)
{
    bc_finish_kernel<<<ceil_div(std::max<int64_t>(R.D.B, 1), 256), 256, 0, s>>>(R.D.B, c->bc_traj, c->bc_ctl, R.cert, R.stats);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

// the host window forms: t_start and horizon (either may be NULL) copied to the device, room for win[total_seg]
int bc_window_stage(pct_cloud *c, const double *t_start, const double *horizon, int64_t B, int64_t total_seg, hipStream_t s, BcWinDesc *W)
{
    PCTCHK(bc_reserve(c, c->bc_win, 2 * (size_t)total_seg, s));
    if (t_start) {
        PCTCHK(bc_reserve(c, c->bc_tstart, (size_t)B, s));
        HIPCHK(hipMemcpyAsync(c->bc_tstart, t_start, sizeof(double) * B, hipMemcpyHostToDevice, s));
    }
    if (horizon) {
        PCTCHK(bc_reserve(c, c->bc_horizon, (size_t)B, s));
        HIPCHK(hipMemcpyAsync(c->bc_horizon, horizon, sizeof(double) * B, hipMemcpyHostToDevice, s));
    }
    *W = BcWinDesc{ t_start ? c->bc_tstart.get() : nullptr, horizon ? c->bc_horizon.get() : nullptr, c->bc_win.get() };
    return PCT_OK;
}

bool bc_bad_scalars(double margin, int32_t max_depth, int64_t piece_cap)
{
    return !(margin >= 0.0) || !std::isfinite(margin) || max_depth < 0 || max_depth > kBcMaxDepth || piece_cap < 1 || piece_cap > kBcMaxPieces;
}

// ---- the trajectory clearance (bezier_clearance.hpp; contract: pct_engine.h, "Trajectory clearance"): its rooms and its rounds -----
struct ClRun {
    BcDesc D;
    double tol, cap;
    int max_depth;
    int64_t piece_cap;
    Path path;                       // resolve_algo(Op::Capsule): the certified check's rules and refusals
    pct_traj_clearance *out;         // device memory, B entries
    long long *stats;                // device memory, 3 entries, or NULL
    BcWinDesc W{};                   // the window forms: W.win != NULL
};

// room for a round over nslots slots: the certified check's, and the piece scalars
int cl_round_room(pct_cloud *c, int64_t nslots, hipStream_t s)
{
    PCTCHK(bc_round_room(c, nslots, s));
    return bc_reserve(c, c->cl_geom, (size_t)nslots * kClGeom, s);
}

int cl_traj_room(pct_cloud *c, int64_t B, hipStream_t s)
{
    PCTCHK(bc_traj_room(c, B, s));
    return bc_reserve(c, c->cl_traj, (size_t)B, s);
}

int cl_seed(pct_cloud *c, const ClRun &R, int64_t seg_lanes, hipStream_t s)
{
    cl_init_kernel<<<ceil_div(R.D.B + 1, 256), 256, 0, s>>>(R.D, (long long)R.piece_cap, R.out, c->bc_traj, c->bc_ctl, c->cl_traj);
    bc_seed_pieces(c, R.D, R.W, R.piece_cap, seg_lanes, s);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

// One round over the first nslots slots of set (round & 1): the 2 * nslots end queries into d_q (2 * nslots <= c->qcap), the
// nearest-neighbour batch on the index of R.path, then fold, mark, compaction and the halving into the other set.
int cl_round(pct_cloud *c, const ClRun &R, int round, int64_t nslots, hipStream_t s)
{
    const int cur = round & 1;
    const uint32_t n = (uint32_t)nslots;
    const int lanes = ceil_div(nslots, 256);
    cl_geometry_kernel<<<lanes, 256, 0, s>>>(c->bc_poly[cur], c->bc_meta[cur], c->bc_ctl, n, c->cl_geom, c->d_q);
    HIPCHK(hipGetLastError());
    Path nn;
    PCTCHK(bc_nn_path(c, R.path, 2 * nslots, &nn));
    PCTCHK(nn_run(c, nn, c->d_q, 2 * nslots, c->d_idx, c->d_d2, s));
    cl_fold_kernel<<<lanes, 256, 0, s>>>(c->bc_meta[cur], c->bc_ctl, n, round, c->d_d2, R.out, c->cl_traj);
    cl_attain_kernel<<<lanes, 256, 0, s>>>(c->bc_meta[cur], c->bc_ctl, n, c->d_d2, c->cl_traj, c->bc_traj);
    const int ntiles = ceil_div(nslots, kBcTile);
    (R.W.win ? cl_mark_kernel<true> : cl_mark_kernel<false>)<<<ntiles, kBcTile, 0, s>>>(c->bc_meta[cur], c->bc_ctl, n, round, R.max_depth, R.tol, R.cap, c->d_idx, c->d_d2,
                                                                                        c->cl_geom, R.out, c->bc_traj, c->cl_traj, c->bc_flag, c->bc_tile, R.W.win);
    scan_tile_sums_kernel<uint32_t><<<1, 256, 0, s>>>(c->bc_tile, (uint32_t)ntiles, BcScanDone{ c->bc_ctl, (uint32_t)R.piece_cap });
    if (round < R.max_depth) {
        cl_capped_kernel<<<lanes, 256, 0, s>>>(c->bc_meta[cur], c->bc_ctl, n, c->bc_flag, c->cl_geom, c->bc_traj, c->cl_traj);
        bc_split_kernel<<<ceil_div(2 * nslots, 256), 256, 0, s>>>(c->bc_poly[cur], c->bc_meta[cur], c->bc_poly[cur ^ 1], c->bc_meta[cur ^ 1], c->bc_flag, c->bc_tile,
                                                                 c->bc_ctl, n, c->bc_traj);
    }
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

int cl_finish(pct_cloud *c, const ClRun &R, hipStream_t s)
{
    cl_finish_kernel<<<ceil_div(std::max<int64_t>(R.D.B, 1), 256), 256, 0, s>>>(R.D.B, c->bc_traj, c->bc_ctl, c->cl_traj, R.out, R.stats);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

bool cl_bad_scalars(double tol, double cap, int32_t max_depth, int64_t piece_cap)
{
    return !(tol >= 0.0) || !std::isfinite(tol) || !(cap > 0.0) || max_depth < 0 || max_depth > kBcMaxDepth || piece_cap < 1 || piece_cap > kBcMaxPieces;
}

}  // namespace

extern "C" {

int pct_cloud_append_aos(pct_cloud *c, const void *pts, int64_t n, int64_t stride_bytes)
{
    if (!c || n < 0 || (n > 0 && !pts) || stride_bytes < 12 || (stride_bytes & 3)) return fail(PCT_ERR_INVALID, "bad append arguments");
    if (n > c->cap) return fail(PCT_ERR_CAPACITY, "appending %lld points to a ring of %lld", (long long)n, (long long)c->cap);
    if (c->ring_on && c->dd_res > 0) return ring_append_dedup(c, pts, n, stride_bytes);     // a window of unique voxels (pct_cloud_ring_dedup)
    if (n == 0) return PCT_OK;
    drop_grid(c);
    if (c->ring_ready) return ring_append(c, pts, n, stride_bytes);     // rolling-map index: updated in place
    return append_unindexed(c, pts, n, stride_bytes);
}

int pct_cloud_reserve_queries(pct_cloud *c, int64_t Q)
{
    if (!c || Q < 0) return fail(PCT_ERR_INVALID, "bad reserve");
    if (Q <= c->qcap) return PCT_OK;
    PCTCHK(may_grow(c, Wait::LibraryStream, nullptr, "the query workspaces"));
    const size_t q = (size_t)std::max<int64_t>(Q, 256);
    c->generation++;                    // captured plans hold these pointers
    c->part_q = std::min<int64_t>((int64_t)q, kPartQueries);
    const size_t pq = (size_t)c->part_q;
    PCTCHK(regrow(c->qcap, q, part(c->d_q, 3 * q), part(c->d_r, q), part(c->d_q64, 3 * q), part(c->d_r2, q), part(c->d_d2, q), part(c->d_radius, q),
                  part(c->d_pts64, 3 * q), part(c->d_seg, 6 * q), part(c->d_idx, q), part(c->d_count, q), part(c->d_skip, q), part(c->d_bound, q),
                  part(c->d_qsorted, q),
                  part(c->d_slice, sort_slice_rows(q) * kSortBuckets),       // every hist launch rewrites the rows it uses: never zeroed
                  part(c->d_todo, 2 * q + 16), part(c->d_part_d2, pq * kMaxParts), part(c->d_part_idx, pq * kMaxParts), part(c->d_ovf, pq + 1),
                  part(c->d_cand_count, pq), part(c->d_cand_d2, pq * kCandCap), part(c->d_cand_idx, pq * kCandCap)));
    c->qcap = 0;                        // the group is usable only behind the zeroing below and with the sort's totals
    HIPCHK(hipMemset(c->d_todo, 0, sizeof(uint32_t) * 16));            // count and ticket: the exact-walk kernel leaves them zero after every batch
    if (!c->d_sort1) {
        PCTCHK(c->d_sort1.reset(2 * kSortBuckets));
        HIPCHK(hipMemset(c->d_sort1, 0, sizeof(uint32_t) * 2 * kSortBuckets));   // the sort keeps both sets of totals zero between batches
    }
    HIPCHK(hipMemset(c->d_cand_count, 0, sizeof(uint32_t) * pq));     // the reduce kernel keeps it zero between slices
    c->qcap = (int64_t)q;
    return PCT_OK;
}

// ---- grid ------------------------------------------------------------------------------
int pct_cloud_drop_grid(pct_cloud *c)
{
    if (!c) return fail(PCT_ERR_INVALID, "null cloud");
    drop_grid(c);
    return PCT_OK;
}

int pct_cloud_has_grid(const pct_cloud *c) { return c && c->has_grid ? 1 : 0; }

/* diagnostics (tests): the launch-time choice of nn_run between 32-bit byte offsets and 64-bit addresses; touches no device */
int pct_debug_narrow_offsets(int64_t records, int64_t cell_entries, int64_t queries)
{
    if (records < 0 || cell_entries < 0 || queries < 0) return -1;
    return narrow_offsets_fit((uint64_t)records, (uint64_t)cell_entries, (uint64_t)queries) ? 1 : 0;
}

/* diagnostics (tests): the sort's bin of every query, by the shipped function (query_bin.hpp) compiled for the host, in the form the
 * index build would choose for such a grid; touches no device */
int pct_debug_query_bins(const int32_t dims[3], const float origin[3], float inv_h, int shift, int strip, const float *q, int64_t Q,
                         uint32_t *bins, uint32_t *nbins, int *fast)
{
    if (!dims || !origin || dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || Q < 0 || (Q > 0 && (!q || !bins))) return fail(PCT_ERR_INVALID, "bad query_bins arguments");
    const BinDesc B = bin_desc_make(dims[0], dims[1], dims[2], origin[0], origin[1], origin[2], inv_h, shift, strip);
    for (int64_t i = 0; i < Q; i++)
        bins[i] = B.fast ? query_bin<true>(B, q[3 * i], q[3 * i + 1], q[3 * i + 2]) : query_bin<false>(B, q[3 * i], q[3 * i + 1], q[3 * i + 2]);
    if (nbins) *nbins = B.nbins;
    if (fast) *fast = B.fast;
    return PCT_OK;
}

int pct_cloud_grid_info(const pct_cloud *c, int32_t dims[3], float *cell_size, float origin[3], int64_t *ncells)
{
    if (!c || !c->has_grid) return fail(PCT_ERR_INVALID, "no grid");
    if (dims) { dims[0] = c->G.gx; dims[1] = c->G.gy; dims[2] = c->G.gz; }
    if (cell_size) *cell_size = (float)c->G.hd;
    if (origin) { origin[0] = c->G.ox; origin[1] = c->G.oy; origin[2] = c->G.oz; }
    if (ncells) *ncells = c->G.ncells;
    return PCT_OK;
}

int pct_cloud_build_grid(pct_cloud *c, float cell_size)
{
    if (!c) return fail(PCT_ERR_INVALID, "null cloud");
    if (c->ring_on) return fail(PCT_ERR_INVALID, "this cloud keeps the rolling-map index (pct_cloud_ring_index); drop it before building the cell-sorted one");
    drop_grid(c);
    const int64_t n = c->count;
    if (n == 0) return fail(PCT_ERR_EMPTY, "cannot index an empty cloud");
    hipStream_t s = g_stream;

    // 1. bounding box
    const int bblocks = (int)std::min<int64_t>(1024, (n + 255) / 256);
    PCTCHK(ensure_stage(c, sizeof(float) * (size_t)bblocks * 6));     // the upload staging buffer is idle here: no allocation per build
    float *d_part = reinterpret_cast<float *>(c->d_stage.get());
    bbox_partial_kernel<false><<<bblocks, 256, 0, s>>>(c->x, c->y, c->z, (uint32_t)n, d_part);
    std::vector<float> part((size_t)bblocks * 6);
    hipError_t e = hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(float), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(PCT_ERR_HIP, "bbox reduction failed: %s", hipGetErrorString(e));
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int b = 0; b < bblocks; b++)
        for (int k = 0; k < 3; k++) {
            lo[k] = std::min(lo[k], part[(size_t)b * 6 + k]);
            hi[k] = std::max(hi[k], part[(size_t)b * 6 + 3 + k]);
        }
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(lo[k]) || !std::isfinite(hi[k])) return fail(PCT_ERR_INVALID, "cloud holds non-finite coordinates");

    // 2. cell size: about 2 points per cell over the occupied bounding box, dims capped at 1024/axis
    double ext[3];
    for (int k = 0; k < 3; k++) ext[k] = std::max((double)hi[k] - (double)lo[k], 0.0);
    double h = cell_size;
    if (!(h > 0)) {
        // target points per cell: with the 2x2x2-block-first search (kernels.hpp coop_stage0) larger cells win --
        // the block then decides 99 % of the queries (a wave needs all 8 of its queries decided to skip the cube);
        // same-box A/B on the 10 M uniform cloud against the retired cube-first search at ppc 2: 0.169 ms, ppc 6 + block first 0.134 ms
        // per 1 M queries (retired variants)
        double ppc = 6.0;
        // a cloud that carried the pyramid at its previous build (surfaces, clusters: most cells empty) is rebuilt with cells of
        // half the volume: the walk then scans 52 instead of 89 points per query for one more node visit (10 M pillar surfaces:
        // 0.99 -> 1.10e9 q/s, scripts/probe_pyr.py with PCT_GRID_PPC 3 / 4 / 6 / 9 / 12).  The per-frame rebuild of a sensor cloud
        // (corridor_finder.cpp:93-99) sees the same kind of cloud frame after frame, so the first build's verdict serves the next.
        if (c->was_sparse) ppc = 3.0;
        if (const char *e = std::getenv("PCT_GRID_PPC")) ppc = std::max(0.05, std::atof(e));
        const double diag = std::max({ ext[0], ext[1], ext[2], 1e-6 });
        double vol = 1.0;
        for (int k = 0; k < 3; k++) vol *= std::max(ext[k], diag * 1e-3);
        h = std::cbrt(vol * ppc / (double)n);
    }
    const double max_ext = std::max({ ext[0], ext[1], ext[2] });
    h = std::max(h, max_ext / 1023.0);
    if (!(h > 0)) h = 1.0;   // all points identical
    // The fp32 cell assignment floor((v - o) * inv_h) must stay monotone in v and agree with the fp64 face positions the termination
    // bounds use, whatever the magnitudes:
    //  * inv_h = 1 / h must be finite and h a normal float: cells below 2^-120 are widened to that (coarser cells, same answers);
    //  * v - o overflows to +inf beyond FLT_MAX (a bounding box wider than FLT_MAX: sentinel rows at both ends of the range) and is
    //    clamped into the last cell, so the last cell must BEGIN at or below that threshold: at most floor(3.4e38 / h) + 1 cells per
    //    axis.  The last cell is unbounded above for the search (no face beyond it), so it may hold everything from there on.
    h = std::min(std::max(h, 0x1p-120), 0x1p120);
    const float hf = (float)h;
    GridDesc G{};
    G.ox = lo[0]; G.oy = lo[1]; G.oz = lo[2];
    G.inv_h = 1.0f / hf;
    G.oxd = lo[0]; G.oyd = lo[1]; G.ozd = lo[2];
    G.hd = (double)hf;
    const int gmax = (int)std::min(1024.0, std::floor(3.4e38 / G.hd) + 1.0);
    G.gx = std::max(1, std::min(gmax, (int)std::min(1024.0, std::floor(ext[0] / G.hd)) + 1));
    G.gy = std::max(1, std::min(gmax, (int)std::min(1024.0, std::floor(ext[1] / G.hd)) + 1));
    G.gz = std::max(1, std::min(gmax, (int)std::min(1024.0, std::floor(ext[2] / G.hd)) + 1));
    const uint64_t ncells = (uint64_t)G.gx * G.gy * G.gz;
    if (ncells > 0x7FFFFFF0ull) return fail(PCT_ERR_INVALID, "grid of %llu cells is too large", (unsigned long long)ncells);
    G.ncells = (uint32_t)ncells;

    // 3. counting sort
    PCTCHK(sort_into_cells(c, G));
    PCTCHK(build_pyramid(c, G));
    // block table for stage 0 of the dense batch kernel (kernels.hpp block_corner_kernel).  OFF by default -- measured slower on the
    // headline step (0.126-0.131 ms against 0.120-0.121, profiles/r03_ab_block_table.txt): the 6.7 MB cell table it replaces is served
    // by the L2s, the 56 MB of corner entries are not, and one line that misses costs more than four that hit.  PCT_BLOCK_TABLE=1
    // (read at every build) keeps it selectable and tested.
    G.blocks = nullptr;
    {
        const char *et = std::getenv("PCT_BLOCK_TABLE");
        const bool table_on = et ? std::atoi(et) != 0 : false;
        const uint64_t ncorners = (uint64_t)(G.gx + 1) * (uint64_t)(G.gy + 1) * (uint64_t)(G.gz + 1);
        if (table_on && !c->has_pyr && ncorners < 0x7FFFFFF0ull) {
            PCTCHK(c->blocks.reserve((size_t)(2 * ncorners)));
            block_corner_kernel<<<ceil_div((int64_t)ncorners, 256), 256, 0, s>>>(G, c->cell_start, c->blocks, (uint32_t)ncorners);
            HIPCHK(hipGetLastError());
            PCTCHK(note_mutation(c));            // queued, not awaited: a *_dev call on another stream waits on the event
            G.blocks = c->blocks;
        }
    }
    c->G = G;
    // Block size of the dense NN batch kernel: two waves where the cell-sorted records fit the 256 MiB Infinity Cache, four where the
    // batch waits on HBM (measured at 10 M and 100 M points, kernels.hpp nn_grid_coop_kernel; the line between them is this reasoning,
    // not a sweep).  PCT_NN_BLOCK = 128 / 256 (read at every build) overrides it: same answers either way.
    c->nn_block = (uint64_t)(c->count + kGridPad) * sizeof(float4) <= (256ull << 20) ? kNNBlock : 256;
    if (const char *eb = std::getenv("PCT_NN_BLOCK")) { const int b = std::atoi(eb); if (b == kNNBlock || b == 256) c->nn_block = b; }
    // query bins: (2^shift)^3 cells each
    // (bin_desc_make, query_bin.hpp: clamps the two knobs, prepares the sort kernels' constants and chooses the bin's form)
    int bin_shift = 1, bin_strip = 16;
    if (const char *eb = std::getenv("PCT_BIN_SHIFT")) bin_shift = std::max(0, std::min(4, std::atoi(eb)));
    if (const char *es = std::getenv("PCT_BIN_STRIP")) bin_strip = std::max(1, std::atoi(es));
    c->B = bin_desc_make(G.gx, G.gy, G.gz, G.ox, G.oy, G.oz, G.inv_h, bin_shift, bin_strip);
    // With at most 1024 cells per axis (above) every grid built here takes the multiply-free form; PCT_BIN_FORM=0 (read at every
    // build) selects the generic one, which is otherwise out of the tests' reach on the card.
    if (const char *ef = std::getenv("PCT_BIN_FORM")) if (std::atoi(ef) == 0) c->B.fast = 0;
    c->has_grid = true;
    c->generation++;
    return PCT_OK;
}

// ---- device-buffer entry points --------------------------------------------------------
int pct_nn_batch_dev(pct_cloud *c, int algo, const float *d_q, int64_t Q, uint32_t *d_idx, double *d_d2, void *stream)
{
    if (!c || Q < 0 || (Q > 0 && (!d_q || !d_idx || !d_d2))) return fail(PCT_ERR_INVALID, "bad nn_batch_dev arguments");
    PCTCHK(order_after_mutations(c, (hipStream_t)stream));
    return nn_dev(c, algo, d_q, Q, d_idx, d_d2, (hipStream_t)stream);   // NULL = HIP's null stream (torch's default stream)
}

int pct_radius_count_batch_dev(pct_cloud *c, int algo, const float *d_q, const float *d_r, int64_t Q, uint32_t *d_count, void *stream)
{
    if (!c || Q < 0 || (Q > 0 && (!d_q || !d_r || !d_count))) return fail(PCT_ERR_INVALID, "bad radius_count_batch_dev arguments");
    PCTCHK(order_after_mutations(c, (hipStream_t)stream));
    return count_dev(c, algo, d_q, d_r, Q, d_count, (hipStream_t)stream);
}

// ---- host-buffer entry points ----------------------------------------------------------
int pct_nn_batch_algo(pct_cloud *c, int algo, const float *q, int64_t Q, uint32_t *idx, double *d2)
{
    if (!c || Q < 0 || (Q > 0 && (!q || !idx || !d2))) return fail(PCT_ERR_INVALID, "bad nn_batch arguments");
    if (Q == 0) return PCT_OK;
    Path path;
    PCTCHK(resolve_algo(c, Op::NN, algo, Q, &path));
    if (Q <= kExpressMaxQ && (path == Path::Table || path == Path::Grid)) {
        // small batch on an indexed cloud: one launch, a block per query, arguments/results in mapped memory
        for (int64_t i = 0; i < 3 * Q; i++) c->xin.host()[i] = (double)q[i];
        if (path == Path::Table)
            ring_batch_kernel<false><<<(int)Q, 256, 0, g_stream>>>(ring_view(c), InflateParams{}, nullptr, c->xin, (double)INFINITY, (uint32_t)c->index_base,
                                                                   nullptr, nullptr, nullptr, c->xout, next_signal(c));
        else
            inflate_block_kernel<false><<<(int)Q, 256, 0, g_stream>>>(c->G, c->sorted, c->cell_start, InflateParams{}, c->xin, (double)INFINITY,
                                                                       (uint32_t)c->index_base, c->xout, next_signal(c));
        HIPCHK(hipGetLastError());
        PCTCHK(express_wait(c));
        read_express_out(c, Q, nullptr, idx, d2);
        return PCT_OK;
    }
    PCTCHK(pct_cloud_reserve_queries(c, Q));
    bool mapped = false;
    PCTCHK(stage_queries(c, q, nullptr, Q, &mapped));
    PCTCHK(nn_run(c, path, c->d_q, Q, c->d_idx, c->d_d2, g_stream));
    PCTCHK(fetch_results(c, mapped, c->d_idx, idx, c->d_d2, d2, Q));
    if (path == Path::Empty) return fail(PCT_ERR_EMPTY, "nearest-neighbour query against an empty cloud");
    return PCT_OK;
}

int pct_nn_batch(pct_cloud *c, const float *q, int64_t Q, uint32_t *idx, double *d2)
{
    return pct_nn_batch_algo(c, PCT_ALGO_AUTO, q, Q, idx, d2);
}

// ---- k nearest neighbours ----------------------------------------------------------------
int pct_knn_batch_dev(pct_cloud *c, int algo, const float *d_q, int64_t Q, int32_t k, uint32_t *d_idx, double *d_d2, void *stream)
{
    if (!c || Q < 0 || (Q > 0 && (!d_q || !d_idx || !d_d2))) return fail(PCT_ERR_INVALID, "bad knn_batch_dev arguments");
    if (k < 1 || k > PCT_KNN_MAX_K) return fail(PCT_ERR_INVALID, "k = %d is outside 1 .. %d", (int)k, PCT_KNN_MAX_K);
    PCTCHK(order_after_mutations(c, (hipStream_t)stream));
    return knn_dev(c, algo, d_q, Q, (int)k, d_idx, d_d2, (hipStream_t)stream);
}

int pct_knn_batch_algo(pct_cloud *c, int algo, const float *q, int64_t Q, int32_t k, uint32_t *idx, double *d2)
{
    if (!c || Q < 0 || (Q > 0 && (!q || !idx || !d2))) return fail(PCT_ERR_INVALID, "bad knn_batch arguments");
    if (k < 1 || k > PCT_KNN_MAX_K) return fail(PCT_ERR_INVALID, "k = %d is outside 1 .. %d", (int)k, PCT_KNN_MAX_K);
    if (Q == 0) return PCT_OK;
    PCTCHK(pct_cloud_reserve_queries(c, Q));
    const size_t rows = (size_t)Q * (size_t)k;
    if (rows > c->knn_out_cap) {
        HIPCHK(hipStreamSynchronize(g_stream));
        PCTCHK(regrow(c->knn_out_cap, rows, part(c->d_knn_idx, rows), part(c->d_knn_d2, rows)));
    }
    HIPCHK(hipMemcpyAsync(c->d_q, q, sizeof(float) * 3 * Q, hipMemcpyHostToDevice, g_stream));
    PCTCHK(ask_twice_after_overrun(c, [&] {
        PCTCHK(knn_dev(c, algo, c->d_q, Q, (int)k, c->d_knn_idx, c->d_knn_d2, g_stream));
        return fetch_results(c, false, c->d_knn_idx, idx, c->d_knn_d2, d2, (int64_t)rows);
    }));
    if (c->count == 0) return fail(PCT_ERR_EMPTY, "k-nearest-neighbour query against an empty cloud");
    return PCT_OK;
}

int pct_knn_batch(pct_cloud *c, const float *q, int64_t Q, int32_t k, uint32_t *idx, double *d2)
{
    return pct_knn_batch_algo(c, PCT_ALGO_AUTO, q, Q, k, idx, d2);
}

// ---- radius search with lists --------------------------------------------------------------
int pct_radius_search_batch_dev(pct_cloud *c, int algo, const float *d_q, const float *d_r, int64_t Q, int order, int64_t *d_offsets, int64_t cap,
                                uint32_t *d_idx, double *d_d2, void *stream)
{
    if (!c || Q < 0 || !d_offsets || cap < 0 || (Q > 0 && (!d_q || !d_r)) || (cap > 0 && !d_idx))
        return fail(PCT_ERR_INVALID, "bad radius_search_batch_dev arguments");
    if (order != PCT_ORDER_INDEX && order != PCT_ORDER_DISTANCE) return fail(PCT_ERR_INVALID, "unknown order %d", order);
    Path path;
    PCTCHK(resolve_algo(c, Op::RadiusSearch, algo, Q, &path));
    hipStream_t s = (hipStream_t)stream;
    c->rs.valid = false;                                     // the host form's result ends with the next search of either form
    PCTCHK(list_search_dev_prelude(c, c->rs, true, Q, order, d_offsets, cap, &d_d2, s));      // idx grows with the borrowed d2 (kept as found)
    if (Q == 0) return PCT_OK;
    PCTCHK(rs_count_scan(c, path, d_q, d_r, Q, reinterpret_cast<long long *>(d_offsets), s));
    return rs_fill_sort(c, path, d_q, d_r, Q, order, reinterpret_cast<long long *>(d_offsets), cap, d_idx, d_d2, s);
}

int pct_radius_search_batch(pct_cloud *c, int algo, const float *q, const float *r, int64_t Q, int order, int64_t *offsets, int64_t *total)
{
    if (!c || Q < 0 || !offsets || !total || (Q > 0 && (!q || !r))) return fail(PCT_ERR_INVALID, "bad radius_search_batch arguments");
    if (order != PCT_ORDER_INDEX && order != PCT_ORDER_DISTANCE) return fail(PCT_ERR_INVALID, "unknown order %d", order);
    Path path;
    PCTCHK(resolve_algo(c, Op::RadiusSearch, algo, Q, &path));
    return list_search_host(c, c->rs, "radius search", false, Q, offsets, total,
        [&]() -> int {
            HIPCHK(hipMemcpyAsync(c->d_q, q, sizeof(float) * 3 * Q, hipMemcpyHostToDevice, g_stream));
            HIPCHK(hipMemcpyAsync(c->d_r, r, sizeof(float) * Q, hipMemcpyHostToDevice, g_stream));
            return PCT_OK;
        },
        [&] { return rs_count_scan(c, path, c->d_q, c->d_r, Q, c->rs_off, g_stream); },
        [&] { return rs_fill_sort(c, path, c->d_q, c->d_r, Q, order, c->rs_off, *total, c->rs.idx, c->rs.d2, g_stream); });      // an empty cloud: PCT_OK
}

int pct_radius_search_read(pct_cloud *c, int64_t first, int64_t n, uint32_t *idx, double *d2)
{
    if (!c) return fail(PCT_ERR_INVALID, "no radius-search result to read (none yet, or the cloud changed since)");
    return read_lists(c->rs, first, n, idx, d2, nullptr);
}

int pct_nn_batch_q64(pct_cloud *c, const double *q, int64_t Q, uint32_t *idx, double *d2)
{
    return pct_nn_batch_q64_ties(c, q, Q, idx, d2, nullptr);
}

int pct_nn_batch_q64_ties(pct_cloud *c, const double *q, int64_t Q, uint32_t *idx, double *d2, uint32_t *ties)
{
    if (!c || Q < 0 || (Q > 0 && (!q || !idx || !d2))) return fail(PCT_ERR_INVALID, "bad nn_batch_q64 arguments");
    if (Q == 0) return PCT_OK;
    if (ties) for (int64_t i = 0; i < Q; i++) ties[i] = 0;        // 0 = not counted on this path
    PCTCHK(pct_cloud_reserve_queries(c, Q));
    if (c->count == 0) {
        for (int64_t i = 0; i < Q; i++) { idx[i] = PCT_NO_INDEX; d2[i] = INFINITY; }
        return fail(PCT_ERR_EMPTY, "nearest-neighbour query against an empty cloud");
    }
    if (Q > 1 && Q <= kExpressMaxQ && c->count <= kSmallNNMax) {   // express batch: a block per query, everything in mapped memory
        std::memcpy(c->xin.host(), q, sizeof(double) * 3 * Q);
        nn_small_batch_kernel<<<(int)Q, 256, 0, g_stream>>>(c->x, c->y, c->z, (uint32_t)c->count, c->xin, (uint32_t)c->index_base, c->xout, next_signal(c));
        HIPCHK(hipGetLastError());
        PCTCHK(express_wait(c));
        read_express_out(c, Q, nullptr, idx, d2);
        return PCT_OK;
    }
    if (Q == 1 && c->count <= kSmallNNMax) {   // express: one one-block launch, query by value, result in mapped memory
        nn_small_kernel<<<1, 1024, 0, g_stream>>>(c->x, c->y, c->z, (uint32_t)c->count, q[0], q[1], q[2], (uint32_t)c->index_base, c->xout, next_signal(c));
        HIPCHK(hipGetLastError());
        PCTCHK(express_wait(c));
        idx[0] = c->xout.host()[0].idx;
        d2[0] = c->xout.host()[0].d2;
        if (ties) ties[0] = c->xout.host()[0].count;
        return PCT_OK;
    }
    // The fp32 filter is only valid when the query coordinates themselves are fp32 values
    // (always the case for kd_nearestf); genuinely double queries take the all-fp64 kernel.
    bool f32_exact = true;
    for (int64_t i = 0; i < 3 * Q && f32_exact; i++) f32_exact = (double)(float)q[i] == q[i];
    HIPCHK(hipMemcpyAsync(c->d_q64, q, sizeof(double) * 3 * Q, hipMemcpyHostToDevice, g_stream));
    if (f32_exact && Q > 4) {
        std::vector<float> qf((size_t)3 * Q);
        for (int64_t i = 0; i < 3 * Q; i++) qf[i] = (float)q[i];
        HIPCHK(hipMemcpyAsync(c->d_q, qf.data(), sizeof(float) * 3 * Q, hipMemcpyHostToDevice, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));      // qf goes out of scope below
        PCTCHK(nn_stream_filtered(c, c->d_q, Q, c->d_idx, c->d_d2, g_stream));
    } else {
        PCTCHK(nn_stream_q64(c, Q, c->d_idx, c->d_d2, g_stream));
    }
    return fetch_results(c, false, c->d_idx, idx, c->d_d2, d2, Q);
}

int pct_radius_count_batch_algo(pct_cloud *c, int algo, const float *q, const float *r, int64_t Q, uint32_t *count)
{
    if (!c || Q < 0 || (Q > 0 && (!q || !r || !count))) return fail(PCT_ERR_INVALID, "bad radius_count arguments");
    if (Q == 0) return PCT_OK;
    PCTCHK(pct_cloud_reserve_queries(c, Q));
    bool mapped = false;
    PCTCHK(stage_queries(c, q, r, Q, &mapped));
    return ask_twice_after_overrun(c, [&] {
        PCTCHK(count_dev(c, algo, c->d_q, c->d_r, Q, c->d_count, g_stream));
        return fetch_results(c, mapped, c->d_count, count, nullptr, nullptr, Q);
    });
}

int pct_radius_count_batch(pct_cloud *c, const float *q, const float *r, int64_t Q, uint32_t *count)
{
    return pct_radius_count_batch_algo(c, PCT_ALGO_AUTO, q, r, Q, count);
}

// order-preserving compaction of the points within r of q into c->crop_* (kernels.hpp section 1b)
static int crop_device(pct_cloud *c, const double q[3], double rr, int64_t *total_out)
{
    const uint32_t n = (uint32_t)c->count;
    const uint32_t ntiles = (n + kCropTile - 1) / kCropTile;
    PCTCHK(c->crop_tile.reserve((size_t)ntiles + 1));
    if ((size_t)n > c->crop_cap) {
        const size_t cap = std::max<size_t>((size_t)c->cap, n);
        PCTCHK(regrow(c->crop_cap, cap, part(c->crop_idx, cap), part(c->crop_d2, cap), part(c->crop_x, cap), part(c->crop_y, cap), part(c->crop_z, cap)));
    }
    begin_timing(c, g_stream);
    HIPCHK(hipMemsetAsync(c->crop_tile + ntiles, 0, sizeof(uint32_t), g_stream));
    crop_count_kernel<<<(int)ntiles, 256, 0, g_stream>>>(c->x, c->y, c->z, n, q[0], q[1], q[2], rr, c->crop_tile);
    scan_tile_sums_kernel<uint32_t><<<1, 256, 0, g_stream>>>(c->crop_tile, ntiles + 1, ScanDoneNothing{});       // entry ntiles becomes the grand total
    crop_scatter_kernel<<<(int)ntiles, 256, 0, g_stream>>>(c->x, c->y, c->z, n, q[0], q[1], q[2], rr, (uint32_t)c->index_base, c->crop_tile,
                                                          (uint32_t)c->crop_cap, c->crop_idx, c->crop_d2, c->crop_x, c->crop_y, c->crop_z);
    end_timing(c, g_stream);
    HIPCHK(hipGetLastError());
    uint32_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, c->crop_tile + ntiles, sizeof total, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    *total_out = total;
    return PCT_OK;
}

int pct_radius_indices(pct_cloud *c, const float q[3], float r, uint32_t *idx_out, int64_t cap, int64_t *n_out)
{
    if (!q) return fail(PCT_ERR_INVALID, "bad radius_indices arguments");
    const double qd[3] = { (double)q[0], (double)q[1], (double)q[2] };
    return pct_radius_indices_q64(c, qd, (double)r, idx_out, cap, n_out);
}

int pct_radius_indices_q64(pct_cloud *c, const double q[3], double r, uint32_t *idx_out, int64_t cap, int64_t *n_out)
{
    return pct_radius_indices_r2_q64(c, q, r * r, idx_out, cap, n_out);
}

int pct_radius_indices_r2_q64(pct_cloud *c, const double q[3], double r2, uint32_t *idx_out, int64_t cap, int64_t *n_out)
{
    if (!c || !q || cap < 0 || (cap > 0 && !idx_out) || !n_out) return fail(PCT_ERR_INVALID, "bad radius_indices arguments");
    *n_out = 0;
    if (c->count == 0) return PCT_OK;
    if (c->count <= 4 * kSmallNNMax && c->count <= (int64_t)kExpressIdsCap) {   // express: one launch, ids in mapped memory
        radius_small_kernel<<<1, 1024, 0, g_stream>>>(c->x, c->y, c->z, (uint32_t)c->count, q[0], q[1], q[2], r2, (uint32_t)c->index_base,
                                                       c->xids, kExpressIdsCap, c->xout, next_signal(c));
        HIPCHK(hipGetLastError());
        PCTCHK(express_wait(c));
        // the kernel stores its hits in arrival order, all of them (total <= count <= kExpressIdsCap): a truncated list is the `cap`
        // lowest indices, so every stored hit is sorted before the first `cap` are handed out
        const int64_t total = c->xout.host()[0].count, stored = std::min<int64_t>(total, kExpressIdsCap), got = std::min<int64_t>(stored, cap);
        if (got == stored) {
            std::copy(c->xids.host(), c->xids.host() + stored, idx_out);
            std::sort(idx_out, idx_out + got);
        } else {
            std::vector<uint32_t> all(c->xids.host(), c->xids.host() + stored);
            std::sort(all.begin(), all.end());
            std::copy(all.begin(), all.begin() + got, idx_out);
        }
        *n_out = total;
        return PCT_OK;
    }
    int64_t total = 0;
    PCTCHK(crop_device(c, q, r2, &total));                 // ascending index order, no host sort needed
    const int64_t got = std::min<int64_t>(total, cap);
    if (got > 0) {
        HIPCHK(hipMemcpyAsync(idx_out, c->crop_idx, sizeof(uint32_t) * got, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
    }
    *n_out = total;
    return PCT_OK;
}

// lidar crop with everything its consumer builds from it (camera_sensor.cpp:133-145, 398-401)
int pct_radius_crop(pct_cloud *c, const double q[3], double r, int sort_by_distance, int64_t cap, uint32_t *idx_out, double *d2_out,
                    float *xyz_out, int64_t *n_out)
{
    if (!c || !q || cap < 0 || !n_out) return fail(PCT_ERR_INVALID, "bad radius_crop arguments");
    *n_out = 0;
    if (c->count == 0) return PCT_OK;
    int64_t total = 0;
    PCTCHK(crop_device(c, q, r * r, &total));
    *n_out = total;
    const int64_t got = std::min<int64_t>(total, cap);
    if (got == 0) return PCT_OK;
    if (sort_by_distance && got < total) return fail(PCT_ERR_CAPACITY, "a distance-sorted crop needs room for all %lld hits (cap %lld)", (long long)total, (long long)cap);
    std::vector<uint32_t> hi((size_t)got);
    std::vector<double> hd((size_t)got);
    std::vector<float> hx, hy, hz;
    HIPCHK(hipMemcpyAsync(hi.data(), c->crop_idx, sizeof(uint32_t) * got, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(hd.data(), c->crop_d2, sizeof(double) * got, hipMemcpyDeviceToHost, g_stream));
    if (xyz_out) {
        hx.resize((size_t)got); hy.resize((size_t)got); hz.resize((size_t)got);
        HIPCHK(hipMemcpyAsync(hx.data(), c->crop_x, sizeof(float) * got, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipMemcpyAsync(hy.data(), c->crop_y, sizeof(float) * got, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipMemcpyAsync(hz.data(), c->crop_z, sizeof(float) * got, hipMemcpyDeviceToHost, g_stream));
    }
    HIPCHK(hipStreamSynchronize(g_stream));
    std::vector<uint32_t> order((size_t)got);
    for (int64_t i = 0; i < got; i++) order[(size_t)i] = (uint32_t)i;
    if (sort_by_distance)     // PCL hands back radiusSearch results nearest first; ties keep ascending index (stable)
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hd[a] < hd[b]; });
    for (int64_t i = 0; i < got; i++) {
        const uint32_t k = order[(size_t)i];
        if (idx_out) idx_out[i] = hi[k];
        if (d2_out) d2_out[i] = hd[k];
        if (xyz_out) { xyz_out[3 * i] = hx[k]; xyz_out[3 * i + 1] = hy[k]; xyz_out[3 * i + 2] = hz[k]; }
    }
    return PCT_OK;
}

// dst = the points of src within r of q, in src's order, device to device (known_map_pcl of camera_sensor.cpp:398-401)
int pct_cloud_crop_to(pct_cloud *src, const double q[3], double r, pct_cloud *dst)
{
    if (!src || !dst || !q || src == dst) return fail(PCT_ERR_INVALID, "bad crop_to arguments");
    int64_t total = 0;
    if (src->count) PCTCHK(crop_device(src, q, r * r, &total));
    if (total > dst->cap) return fail(PCT_ERR_CAPACITY, "crop holds %lld points, destination capacity is %lld", (long long)total, (long long)dst->cap);
    return pct_cloud_upload_soa_dev(dst, src->crop_x, src->crop_y, src->crop_z, total);
}

// K range queries against a small cloud in one launch: ids_out[k * cap_per_query + j] (arrival order, not sorted),
// counts_out[k] = number of hits of query k (may exceed cap_per_query: then only the first cap_per_query are stored).
int pct_radius_indices_batch_q64(pct_cloud *c, const double *q, const double *r, int64_t K, uint32_t *ids_out, int64_t cap_per_query,
                                 int64_t *counts_out)
{
    if (!c || K < 0 || (K > 0 && (!q || !r || !ids_out || !counts_out)) || cap_per_query <= 0) return fail(PCT_ERR_INVALID, "bad radius_indices_batch arguments");
    if (K == 0) return PCT_OK;
    if (K > kExpressMaxQ || c->count > 4 * kSmallNNMax) return fail(PCT_ERR_INVALID, "batched range queries serve small clouds (<= 65536 points) and K <= 1024");
    for (int64_t k = 0; k < K; k++) counts_out[k] = 0;
    if (c->count == 0) return PCT_OK;
    const uint32_t cap = (uint32_t)std::min<int64_t>(cap_per_query, kExpressIdsCap / K);
    std::memcpy(c->xin.host(), q, sizeof(double) * 3 * K);
    std::memcpy(c->xr.host(), r, sizeof(double) * K);
    radius_small_batch_kernel<<<(int)K, 256, 0, g_stream>>>(c->x, c->y, c->z, (uint32_t)c->count, c->xin, c->xr, (uint32_t)c->index_base,
                                                            c->xids, cap, c->xout, next_signal(c));
    HIPCHK(hipGetLastError());
    PCTCHK(express_wait(c));
    for (int64_t k = 0; k < K; k++) {
        counts_out[k] = c->xout.host()[k].count;
        const int64_t got = std::min<int64_t>(counts_out[k], cap);
        std::copy(c->xids.host() + k * cap, c->xids.host() + k * cap + got, ids_out + k * cap_per_query);
        if (counts_out[k] > cap) counts_out[k] = -counts_out[k];      // negative = truncated: the caller must re-ask that query alone
    }
    return PCT_OK;
}

int pct_inflate_batch(pct_cloud *c, const pct_inflate_params *p, const double *pts, int64_t Q, double *radius, uint32_t *idx, double *d2)
{
    if (!c || !p || Q < 0 || (Q > 0 && (!pts || !radius))) return fail(PCT_ERR_INVALID, "bad inflate arguments");
    if (Q == 0) return PCT_OK;
    // idx / d2 not wanted: the index searches may stop once everything unseen is beyond max_radius + search_margin
    const double reach = p->max_radius + p->search_margin;
    const double stop_d2 = (idx || d2) ? (double)INFINITY : reach * reach;
    if (c->ring_ready) {          // rolling map: a block per point over the bucket table; small batches through mapped memory
        if (Q <= kExpressMaxQ) {
            std::memcpy(c->xin.host(), pts, sizeof(double) * 3 * Q);
            ring_batch_kernel<true><<<(int)Q, 256, 0, g_stream>>>(ring_view(c), to_dev(p), nullptr, c->xin, stop_d2, (uint32_t)c->index_base, nullptr, nullptr,
                                                                  nullptr, c->xout, next_signal(c));
            HIPCHK(hipGetLastError());
            PCTCHK(express_wait(c));
            read_express_out(c, Q, radius, idx, d2);
            return PCT_OK;
        }
        PCTCHK(pct_cloud_reserve_queries(c, Q));
        HIPCHK(hipMemcpyAsync(c->d_pts64, pts, sizeof(double) * 3 * Q, hipMemcpyHostToDevice, g_stream));
        ring_batch_kernel<true><<<(int)Q, 256, 0, g_stream>>>(ring_view(c), to_dev(p), nullptr, c->d_pts64, stop_d2, (uint32_t)c->index_base, c->d_idx, c->d_d2,
                                                              c->d_radius, nullptr, ExpressSignal{});
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(radius, c->d_radius, sizeof(double) * Q, hipMemcpyDeviceToHost, g_stream));
        if (idx) HIPCHK(hipMemcpyAsync(idx, c->d_idx, sizeof(uint32_t) * Q, hipMemcpyDeviceToHost, g_stream));
        if (d2) HIPCHK(hipMemcpyAsync(d2, c->d_d2, sizeof(double) * Q, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
        return PCT_OK;
    }
    if (Q <= kExpressMaxQ && c->has_grid && c->count > 0) {   // express: one fused launch (a block per point), arguments and results in mapped memory
        std::memcpy(c->xin.host(), pts, sizeof(double) * 3 * Q);
        inflate_block_kernel<true><<<(int)Q, 256, 0, g_stream>>>(c->G, c->sorted, c->cell_start, to_dev(p), c->xin, stop_d2, (uint32_t)c->index_base, c->xout, next_signal(c));
        HIPCHK(hipGetLastError());
        PCTCHK(express_wait(c));
        read_express_out(c, Q, radius, idx, d2);
        return PCT_OK;
    }
    PCTCHK(pct_cloud_reserve_queries(c, Q));
    if (Q <= kExpressMaxQ) {      // small batch on an un-indexed (e.g. rolling) cloud: brute-force kernels, arguments and results in mapped memory
        std::memcpy(c->xin.host(), pts, sizeof(double) * 3 * Q);
        PCTCHK(inflate_dev(c, p, Q, g_stream, c->xin, c->xout));
        HIPCHK(hipStreamSynchronize(g_stream));
        read_express_out(c, Q, radius, idx, d2);
        return PCT_OK;
    }
    HIPCHK(hipMemcpyAsync(c->d_pts64, pts, sizeof(double) * 3 * Q, hipMemcpyHostToDevice, g_stream));
    PCTCHK(inflate_dev(c, p, Q, g_stream));
    HIPCHK(hipMemcpyAsync(radius, c->d_radius, sizeof(double) * Q, hipMemcpyDeviceToHost, g_stream));
    if (idx) HIPCHK(hipMemcpyAsync(idx, c->d_idx, sizeof(uint32_t) * Q, hipMemcpyDeviceToHost, g_stream));
    if (d2) HIPCHK(hipMemcpyAsync(d2, c->d_d2, sizeof(double) * Q, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return PCT_OK;
}

// ---- segment queries and sweeps (include/pct_engine.h, "Segment queries", "Segment sweeps"): one dispatch, frame and staged workspaces ----
int pct_segment_nn_batch_dev(pct_cloud *c, int algo, const double *d_seg, const double *d_reach, int64_t Q, uint32_t *d_idx, double *d_d2,
                             double *d_s, void *stream)
{
    if (!c || Q < 0 || (Q > 0 && (!d_seg || !d_reach || !d_idx))) return fail(PCT_ERR_INVALID, "bad segment_nn_batch_dev arguments");
    return segment_batch_dev(c, algo, SegMeasure::Nearest, d_seg, d_reach, Q, d_idx, d_d2, d_s, (hipStream_t)stream);
}

int pct_segment_nn_batch(pct_cloud *c, int algo, const double *seg, const double *reach, int64_t Q, uint32_t *idx, double *d2, double *s)
{
    if (!c || Q < 0 || (Q > 0 && (!seg || !reach || !idx))) return fail(PCT_ERR_INVALID, "bad segment_nn_batch arguments");
    return segment_batch_host(c, algo, SegMeasure::Nearest, seg, reach, Q, idx, d2, s, "segment query against an empty cloud");
}

int pct_segment_sweep_batch_dev(pct_cloud *c, int algo, const double *d_seg, const double *d_radius, int64_t Q, uint32_t *d_idx, double *d_t,
                                void *stream)
{
    if (!c || Q < 0 || (Q > 0 && (!d_seg || !d_radius || !d_idx))) return fail(PCT_ERR_INVALID, "bad segment_sweep_batch_dev arguments");
    return segment_batch_dev(c, algo, SegMeasure::Sweep, d_seg, d_radius, Q, d_idx, d_t, nullptr, (hipStream_t)stream);
}

int pct_segment_sweep_batch(pct_cloud *c, int algo, const double *seg, const double *radius, int64_t Q, uint32_t *idx, double *t)
{
    if (!c || Q < 0 || (Q > 0 && (!seg || !radius || !idx))) return fail(PCT_ERR_INVALID, "bad segment_sweep_batch arguments");
    return segment_batch_host(c, algo, SegMeasure::Sweep, seg, radius, Q, idx, t, nullptr, "segment sweep against an empty cloud");
}

// ---- capsule search (include/pct_engine.h, "Capsule search") ------------------------------------------------------------------------
int pct_segment_count_batch_dev(pct_cloud *c, int algo, const double *d_seg, const double *d_reach, int64_t Q, uint32_t *d_count, void *stream)
{
    if (!c || Q < 0 || (Q > 0 && (!d_seg || !d_reach || !d_count))) return fail(PCT_ERR_INVALID, "bad segment_count_batch_dev arguments");
    Path path;
    PCTCHK(resolve_algo(c, Op::Capsule, algo, Q, &path));
    if (Q == 0) return PCT_OK;
    PCTCHK(require_reserved(c, Q, "batch"));
    PCTCHK(order_after_mutations(c, (hipStream_t)stream));
    return ss_count_run(c, path, d_seg, d_reach, Q, d_count, (hipStream_t)stream, no_step);
}

int pct_segment_count_batch(pct_cloud *c, int algo, const double *seg, const double *reach, int64_t Q, uint32_t *count)
{
    if (!c || Q < 0 || (Q > 0 && (!seg || !reach || !count))) return fail(PCT_ERR_INVALID, "bad segment_count_batch arguments");
    PCTCHK(ring_finish_pending(c));              // rolling map: an append in flight is finished first and the answer sees its frame
    Path path;
    PCTCHK(resolve_algo(c, Op::Capsule, algo, Q, &path));
    if (Q == 0) return PCT_OK;
    PCTCHK(pct_cloud_reserve_queries(c, Q));
    return segment_host_form(c, seg, reach, Q, { { count, c->d_count, sizeof(uint32_t) } },
                             path == Path::Empty ? "capsule count against an empty cloud" : nullptr,
                             [&] { return ss_count_run(c, path, c->d_seg, c->d_r2, Q, c->d_count, g_stream, no_step); });
}

int pct_segment_search_batch_dev(pct_cloud *c, int algo, const double *d_seg, const double *d_reach, int64_t Q, int order, int64_t *d_offsets,
                                 int64_t cap, uint32_t *d_idx, double *d_d2, double *d_s, void *stream)
{
    if (!c || Q < 0 || !d_offsets || cap < 0 || (Q > 0 && (!d_seg || !d_reach)) || (cap > 0 && !d_idx))
        return fail(PCT_ERR_INVALID, "bad segment_search_batch_dev arguments");
    if (order != PCT_ORDER_INDEX && order != PCT_ORDER_DISTANCE) return fail(PCT_ERR_INVALID, "unknown order %d", order);
    Path path;
    PCTCHK(resolve_algo(c, Op::Capsule, algo, Q, &path));
    hipStream_t s = (hipStream_t)stream;
    PCTCHK(list_search_dev_prelude(c, c->ss, false, Q, order, d_offsets, cap, &d_d2, s));     // the host form's result lasts unless d2 is borrowed
    if (Q == 0) return PCT_OK;
    long long *off = reinterpret_cast<long long *>(d_offsets);
    return ss_count_run(c, path, d_seg, d_reach, Q, c->d_count, s, [&]() -> int {      // scan, fill and sort inside the count's frame
        PCTCHK(list_scan(c, Q, off, 1u, s));
        return ss_fill_sort(c, path, d_seg, d_reach, Q, order, off, cap, d_idx, d_d2, d_s, s);
    });
}

int pct_segment_search_batch(pct_cloud *c, int algo, const double *seg, const double *reach, int64_t Q, int order, int64_t *offsets, int64_t *total)
{
    if (!c || Q < 0 || !offsets || !total || (Q > 0 && (!seg || !reach))) return fail(PCT_ERR_INVALID, "bad segment_search_batch arguments");
    if (order != PCT_ORDER_INDEX && order != PCT_ORDER_DISTANCE) return fail(PCT_ERR_INVALID, "unknown order %d", order);
    PCTCHK(ring_finish_pending(c));
    Path path;
    PCTCHK(resolve_algo(c, Op::Capsule, algo, Q, &path));
    PCTCHK(list_search_host(c, c->ss, "capsule search", true, Q, offsets, total,
        [&] { return stage_segments(c, seg, reach, Q); },
        [&] { return ss_count_run(c, path, c->d_seg, c->d_r2, Q, c->d_count, g_stream, [&] { return list_scan(c, Q, c->rs_off, 1u, g_stream); }); },
        [&] { return ss_fill_sort(c, path, c->d_seg, c->d_r2, Q, order, c->rs_off, *total, c->ss.idx, c->ss.d2, c->ss.s, g_stream); }));
    if (path == Path::Empty && Q > 0) return fail(PCT_ERR_EMPTY, "capsule search against an empty cloud");
    return PCT_OK;
}

int pct_segment_search_read(pct_cloud *c, int64_t first, int64_t n, uint32_t *idx, double *d2, double *s)
{
    if (!c) return fail(PCT_ERR_INVALID, "no capsule-search result to read (none yet, or the cloud changed since)");
    return read_lists(c->ss, first, n, idx, d2, s);
}

// ---- free-space polyhedra (include/pct_engine.h, "Free-space polyhedra") ---------------------------------------------------------------
int pct_polyhedron_lds_rows(void) { return kPolyLds; }

int pct_segment_supports_dev(pct_cloud *c, const double *d_seg, int64_t Q, const int64_t *d_row_offsets, int64_t row_cap, const uint32_t *d_row_idx,
                             int64_t *d_offsets, int64_t cap, uint32_t *d_idx, double *d_d2, double *d_s, double *d_plane, void *stream)
{
    if (!c || Q < 0 || row_cap < 0 || cap < 0 || !d_offsets || (Q > 0 && (!d_seg || !d_row_offsets)) || (Q > 0 && row_cap > 0 && !d_row_idx) ||
        (cap > 0 && !d_idx))
        return fail(PCT_ERR_INVALID, "bad segment_supports_dev arguments");
    hipStream_t s = (hipStream_t)stream;
    if (Q == 0) {
        HIPCHK(hipMemsetAsync(d_offsets, 0, sizeof(int64_t), s));
        return PCT_OK;
    }
    PCTCHK(require_reserved(c, Q, "batch"));
    if (row_cap > 0xFFFFFFFFll) return fail(PCT_ERR_CAPACITY, "rows of %lld entries, more than 2^32 - 1", (long long)row_cap);
    PCTCHK(rs_ensure_work(c));
    PCTCHK(poly_ensure_sup(c, row_cap));
    PCTCHK(order_after_mutations(c, s));
    const long long *rows = reinterpret_cast<const long long *>(d_row_offsets);
    long long *off = reinterpret_cast<long long *>(d_offsets);
    PCTCHK(poly_filter_scan(c, d_seg, Q, rows, row_cap, d_row_idx, off, s));
    return poly_emit(c, d_seg, Q, rows, row_cap, d_row_idx, off, cap, d_idx, d_d2, d_s, d_plane, s);
}

int pct_segment_polyhedron_batch(pct_cloud *c, int algo, const double *seg, const double *reach, int64_t Q, int64_t *offsets, int64_t *total)
{
    if (!c || Q < 0 || !offsets || !total || (Q > 0 && (!seg || !reach))) return fail(PCT_ERR_INVALID, "bad segment_polyhedron_batch arguments");
    PCTCHK(ring_finish_pending(c));
    Path path;
    PCTCHK(resolve_algo(c, Op::Capsule, algo, Q, &path));
    c->pl.valid = false;
    c->pl.total = 0;
    if (Q > 0) PCTCHK(c->pl_off.reserve((size_t)Q + 1));
    // the candidate rows in distance order (no s), then -- inside the same step, before the frame's wait -- the filter, the count and
    // the scan of the supports; the support offsets are the second and last host read
    std::vector<int64_t> rows((size_t)Q + 1);
    int64_t row_total = 0;
    PCTCHK(list_search_host(c, c->pc, "free-space polyhedra", false, Q, rows.data(), &row_total,
        [&] { return stage_segments(c, seg, reach, Q); },
        [&] { return ss_count_run(c, path, c->d_seg, c->d_r2, Q, c->d_count, g_stream, [&] { return list_scan(c, Q, c->rs_off, 1u, g_stream); }); },
        [&]() -> int {
            PCTCHK(ss_fill_sort(c, path, c->d_seg, c->d_r2, Q, PCT_ORDER_DISTANCE, c->rs_off, row_total, c->pc.idx, c->pc.d2, nullptr, g_stream));
            PCTCHK(poly_ensure_sup(c, row_total));
            PCTCHK(poly_filter_scan(c, c->d_seg, Q, c->rs_off, row_total, c->pc.idx, c->pl_off, g_stream));
            HIPCHK(hipMemcpyAsync(offsets, c->pl_off, sizeof(int64_t) * (Q + 1), hipMemcpyDeviceToHost, g_stream));
            return PCT_OK;
        }));
    if (Q == 0) offsets[0] = 0;
    *total = offsets[Q];
    if (*total > 0) {
        PCTCHK(ensure_lists(c, c->pl, (size_t)*total, true, true));
        PCTCHK(c->pl_plane.reserve(4 * (size_t)*total, 4 * c->pl.cap));
        PCTCHK(poly_emit(c, c->d_seg, Q, c->rs_off, row_total, c->pc.idx, c->pl_off, *total, c->pl.idx, c->pl.d2, c->pl.s, c->pl_plane, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
    }
    c->pl.total = *total;
    c->pl.valid = true;
    if (path == Path::Empty && Q > 0) return fail(PCT_ERR_EMPTY, "free-space polyhedra against an empty cloud");
    return PCT_OK;
}

int pct_segment_polyhedron_read(pct_cloud *c, int64_t first, int64_t n, uint32_t *idx, double *d2, double *s, double *plane)
{
    if (!c) return fail(PCT_ERR_INVALID, "no free-space-polyhedron result to read (none yet, or the cloud changed since)");
    PCTCHK(read_lists(c->pl, first, n, idx, d2, s));
    if (plane && n > 0) {
        HIPCHK(hipMemcpyAsync(plane, c->pl_plane + 4 * first, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
    }
    return PCT_OK;
}

// The reach that bounds the capsule inflation's walk.  The contract is unbounded: radius = min(sqrt(d2*) - m, R), d2* the smallest
// finite d2 of the window, m = search_margin, R = max_radius, "min" as the engine writes it (rr < R ? rr : R), and the winner is
// named only when rr < R.  The search returns the window's best row with d2 <= r2 = min(fl(rho * rho), DBL_MAX).  If any row is a
// candidate, the best candidate IS the row of d2* (a smaller d2 passes the same test) and the epilogue applies the formula to it:
// nothing depends on rho.  If no row is a candidate the epilogue reports R and names nobody, which is the contract's answer iff
// every row with a finite d2 > r2 has fl(fl(sqrt(d2)) - m) >= R.  rho = max(fl(fl(R + m) * (1 + 2^-20)), 2^-500) for finite R, m:
//   * fl(rho^2) overflows: r2 = DBL_MAX and no finite d2 is above it -- nothing to show.
//   * otherwise rho >= 2^-500, so rho^2 is normal and r2 >= rho^2 (1 - u), u = 2^-53.  sqrt is correctly rounded, hence monotonic:
//     sd = fl(sqrt(d2)) >= fl(sqrt(r2)) >= rho (1 - u)^(3/2).
//   * t = fl(R + m) > 0: then R + m > 0 and t >= (R + m)(1 - u), rho >= t (1 + 2^-20)(1 - u), so
//     sd >= (R + m)(1 + 2^-20)(1 - u)^(7/2) > R + m; t <= 0: R + m <= 0 <= sd.  Either way sd - m >= R as real numbers, R is
//     representable, and a correctly rounded difference is monotonic: fl(sd - m) >= R.
// A non-finite R or m leaves the walk unbounded (rho = +inf), which is the contract itself.
double segment_inflate_reach(const pct_inflate_params *p)
{
    if (!std::isfinite(p->max_radius) || !std::isfinite(p->search_margin)) return (double)INFINITY;
    const double t = p->max_radius + p->search_margin;
    return std::max(t * (1.0 + 0x1p-20), 0x1p-500);
}

int pct_segment_inflate_batch(pct_cloud *c, const pct_inflate_params *p, const double *seg, int64_t Q, double *radius, uint32_t *idx, double *s)
{
    if (!c || !p || Q < 0 || (Q > 0 && (!seg || !radius))) return fail(PCT_ERR_INVALID, "bad segment_inflate_batch arguments");
    PCTCHK(ring_finish_pending(c));
    if (Q == 0) return PCT_OK;
    Path path;
    PCTCHK(resolve_algo(c, Op::Segment, PCT_ALGO_AUTO, Q, &path));
    PCTCHK(pct_cloud_reserve_queries(c, Q));
    const bool empty = path == Path::Empty;      // the engine's empty-cloud rule, PCT_OK: nothing is staged or searched
    const double reach = segment_inflate_reach(p);
    return segment_host_form(c, empty ? nullptr : seg, nullptr, Q,
                             { { radius, c->d_r2, sizeof(double) }, { idx, c->d_idx, sizeof(uint32_t) }, { s, c->d_radius, sizeof(double) } }, nullptr, [&]() -> int {
        // no start-distance early-out: a segment has no single distance to the start
        if (!empty) PCTCHK(segment_run(c, path, SegMeasure::Nearest, c->d_seg, nullptr, reach, Q, c->d_idx, c->d_d2, c->d_radius, g_stream));
        segment_inflate_epilogue_kernel<<<ceil_div(Q, 256), 256, 0, g_stream>>>(to_dev(p), (uint32_t)Q, empty ? 1 : 0, c->d_idx, c->d_d2, c->d_radius,
                                                                                c->d_r2);
        HIPCHK(hipGetLastError());
        return PCT_OK;
    });
}

// ---- fused RRT* expansion step (kernels.hpp rrt_expand_kernel) ----------------------------------------------------------
int pct_cloud_small_aux(pct_cloud *nodes, double **host_aux)
{
    if (!nodes || !host_aux) return fail(PCT_ERR_INVALID, "null argument");
    if (!nodes->host_mapped) return fail(PCT_ERR_INVALID, "per-node planner data lives beside small (host-mapped) clouds only");
    if (!nodes->aux) PCTCHK(nodes->aux.reset((size_t)4 * (size_t)nodes->cap));
    *host_aux = nodes->aux.host();
    return PCT_OK;
}

int pct_rrt_expand_batch(pct_cloud *nodes, pct_cloud *obstacles, const pct_inflate_params *p, const double *samples, int64_t K,
                         int64_t cap_per_query, pct_expand_result *out, uint32_t *ids)
{
    if (!nodes || !obstacles || !p || K < 0 || (K > 0 && (!samples || !out || !ids)) || cap_per_query <= 0) return fail(PCT_ERR_INVALID, "bad expand arguments");
    if (K == 0) return PCT_OK;
    if (K > kExpressMaxQ) return fail(PCT_ERR_INVALID, "at most %d samples per expansion launch", kExpressMaxQ);
    if (!nodes->host_mapped || (nodes->count > 0 && !nodes->aux.host())) return fail(PCT_ERR_INVALID, "the node set must be a small cloud with per-node planner data (pct_cloud_small_aux)");
    // Rolling map: an append that returned with its insert kernel still queued is finished first -- its status words are read and the
    // bookkeeping they ask for (larger buckets, a re-sized table: new pointers, a new generation) happens BEFORE the view below is
    // taken.  The completion word this call waits on is the node cloud's; it says nothing about the obstacle cloud's append.
    PCTCHK(ring_finish_pending(obstacles));
    const bool ring = obstacles->ring_ready;
    if (!ring && obstacles->count > 0 && !obstacles->has_grid)
        return fail(PCT_ERR_INVALID, "the obstacle cloud has no index (pct_cloud_build_grid or pct_cloud_ring_index): the fused step searches one; "
                                     "the staged queries (pct_nn_batch, pct_inflate_batch, pct_radius_*) answer without");
    if (!nodes->eout) PCTCHK(nodes->eout.reset((size_t)kExpressMaxQ));
    const uint32_t cap = (uint32_t)std::min<int64_t>(cap_per_query, kExpressIdsCap / K);
    std::memcpy(nodes->xin.host(), samples, sizeof(double) * 3 * K);
    const double reach = p->max_radius + p->search_margin;       // only the radius is wanted: stop once everything unseen is beyond it
    // a rolling window that holds nothing (table sized from an extent, nothing appended) is empty by the device's own count; a ring
    // index that has no table yet (no extent, no data) has ring_ready == false and count == 0: the static form's empty rule
    PCTCHK(ask_twice_after_overrun(obstacles, [&]() -> int {     // the table lost points (overflow-queue overrun): refiled, asked once more
        const ExpressSignal sig = K <= 8 ? next_signal(nodes) : ExpressSignal{};
        if (ring)
            rrt_expand_kernel<true><<<(int)K, 256, 0, g_stream>>>(nodes->x, nodes->y, nodes->z, (uint32_t)nodes->count, nodes->aux, nodes->xin,
                                                                  ring_view(obstacles), GridDesc{}, nullptr, nullptr, 0, to_dev(p), reach * reach,
                                                                  nodes->xids, cap, nodes->eout, sig);
        else
            rrt_expand_kernel<false><<<(int)K, 256, 0, g_stream>>>(nodes->x, nodes->y, nodes->z, (uint32_t)nodes->count, nodes->aux, nodes->xin,
                                                                   RingView{}, obstacles->G, obstacles->sorted, obstacles->cell_start,
                                                                   obstacles->count == 0 ? 1 : 0, to_dev(p), reach * reach, nodes->xids, cap,
                                                                   nodes->eout, sig);
        HIPCHK(hipGetLastError());
        // one or a few samples: the completion word (1500 one-sample iterations 37 -> 32 ms); speculative batches of 16-256 blocks:
        // a system-scope fence per block costs more than the stream synchronise saves (2.85 vs 2.60 ms per 1500 iterations at K = 64)
        if (K <= 8) PCTCHK(express_wait(nodes));
        else HIPCHK(hipStreamSynchronize(g_stream));
        return PCT_OK;
    }));
    for (int64_t k = 0; k < K; k++) {
        const ExpandOut &e = nodes->eout.host()[k];
        out[k].center[0] = e.cx; out[k].center[1] = e.cy; out[k].center[2] = e.cz;
        out[k].radius = e.radius;
        out[k].near_idx = e.near_idx == kNoIndex ? -1 : (int32_t)e.near_idx;
        const int64_t got = std::min<int64_t>(e.count, cap);
        out[k].count = e.count > cap ? -(int32_t)e.count : (int32_t)e.count;     // negative = list truncated: ask that range query alone
        std::copy(nodes->xids.host() + k * cap, nodes->xids.host() + k * cap + got, ids + k * cap_per_query);
    }
    return PCT_OK;
}

int pct_bezier_check(pct_cloud *c, const pct_bezier_traj *traj, const pct_inflate_params *p, double t_start, double stop_time, double dt,
                     int64_t *first_hit, int64_t *nsamples, int64_t cap, double *pos, double *radius, double *d2, uint32_t *idx)
{
    if (!c || !traj || !p || !first_hit || !nsamples || !traj->polycoef || !traj->seg_time || !traj->orders || traj->nseg <= 0 ||
        !(dt > 0) || cap <= 0)
        return fail(PCT_ERR_INVALID, "bad bezier_check arguments");
    if (cap > kBezierCapMax) cap = kBezierCapMax;
    PCTCHK(bezier_check_orders(traj));
    if (c->ring_ready) {          // rolling map: the fused planner batch with samples only
        pct_replan_out o{};
        o.sample_pos = pos; o.sample_radius = radius; o.sample_d2 = d2; o.sample_idx = idx;
        PCTCHK(replan_direct(c, p, nullptr, 0, traj, t_start, stop_time, dt, (idx || d2) ? 1 : 0, 0, (int)cap, &o));
        *nsamples = o.nsamples;
        *first_hit = o.first_hit_sample;
        return PCT_OK;
    }
    const size_t ncoef = (size_t)traj->nseg * traj->row_stride;
    if (ncoef + (size_t)traj->nseg <= 3 * (size_t)kExpressMaxQ - 64) {
        // express: the host enumerates the sample times (bezier_enumerate, as thread 0 of bezier_samples_kernel does), then ONE
        // launch evaluates, inflates and searches every sample (bezier_block_kernel)
        double *hd = c->xin.host();                                  // [coef | seg_time | sample_t]
        uint32_t *hu = c->xids.host();                               // [orders | sample_seg]
        std::memcpy(hd, traj->polycoef, sizeof(double) * ncoef);
        std::memcpy(hd + ncoef, traj->seg_time, sizeof(double) * traj->nseg);
        for (int i = 0; i < traj->nseg; i++) hu[i] = (uint32_t)traj->orders[i];
        double *ht = hd + ncoef + traj->nseg;
        uint32_t *hs = hu + traj->nseg;
        const int64_t room = std::min<int64_t>({ cap, (int64_t)kExpressMaxQ, (int64_t)(3 * (size_t)kExpressMaxQ - ncoef - (size_t)traj->nseg) });
        const int64_t n = bezier_enumerate<false>(traj->seg_time, 0, traj->nseg, t_start, stop_time, dt, room, kBezierNoBound,
                                                  [&](long long k, double t, int seg) { ht[k] = t; hs[k] = (uint32_t)seg; });
        const int64_t m = std::min<int64_t>(n, room);
        const bool fits = n <= room || room == cap;             // more samples than one express launch holds: staged path below
        if (fits && m > 0) {
            if (!c->bpos) PCTCHK(c->bpos.reset((size_t)3 * kExpressMaxQ));
            if (c->has_grid && c->count > 0) {        // indexed cloud: everything in ONE launch
                const double reach = p->max_radius + p->search_margin;
                const double stop_d2 = (idx || d2) ? (double)INFINITY : reach * reach;
                bezier_block_kernel<<<(int)m, 256, 0, g_stream>>>(c->G, c->sorted, c->cell_start, to_dev(p), c->xin, (int)traj->row_stride,
                                                                   c->xin + ncoef, c->xids, c->xids + traj->nseg, c->xin + ncoef + traj->nseg,
                                                                   stop_d2, (uint32_t)c->index_base, c->xout, c->bpos, next_signal(c));
                HIPCHK(hipGetLastError());
                PCTCHK(express_wait(c));
            } else {                                      // un-indexed (rolling) cloud: evaluate, then the brute-force inflation; still no copies
                PCTCHK(pct_cloud_reserve_queries(c, m));
                bezier_eval_kernel<<<ceil_div(m, 128), 128, 0, g_stream>>>(c->xin, (int)traj->row_stride, c->xin + ncoef, c->xids, c->xids + traj->nseg,
                                                                           c->xin + ncoef + traj->nseg, (int)m, c->d_pts64, c->bpos);
                PCTCHK(inflate_dev(c, p, m, g_stream, c->d_pts64, c->xout));
                HIPCHK(hipStreamSynchronize(g_stream));
            }
        }
        if (fits) {
            int64_t fh = -1;
            for (int64_t i = 0; i < m; i++) {
                if (fh < 0 && c->xout.host()[i].radius < 0.0) fh = i;
                if (radius) radius[i] = c->xout.host()[i].radius;
                if (d2) d2[i] = c->xout.host()[i].d2;
                if (idx) idx[i] = c->xout.host()[i].idx;
            }
            if (pos && m) std::memcpy(pos, c->bpos.host(), sizeof(double) * 3 * m);
            *nsamples = n;
            *first_hit = fh;
            return PCT_OK;
        }
    }
    PCTCHK(pct_cloud_reserve_queries(c, cap));
    if (!c->d_nsamples) PCTCHK(c->d_nsamples.reset(1));
    if (!c->d_first_hit) PCTCHK(c->d_first_hit.reset(1));
    hipStream_t s = g_stream;
    PCTCHK(bezier_stage_coef(c, traj, s, false));
    PCTCHK(bezier_staged_enqueue(c, traj, p, t_start, stop_time, dt, cap, s, c->d_pts64, c->d_radius, nullptr, nullptr, c->d_first_hit, c->d_nsamples));
    int ns = 0;
    long long fh = -1;
    HIPCHK(hipMemcpyAsync(&ns, c->d_nsamples, sizeof ns, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&fh, c->d_first_hit, sizeof fh, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int64_t m = std::min<int64_t>(ns, cap);
    if (pos && m) HIPCHK(hipMemcpy(pos, c->d_pts64, sizeof(double) * 3 * m, hipMemcpyDeviceToHost));
    if (radius && m) HIPCHK(hipMemcpy(radius, c->d_radius, sizeof(double) * m, hipMemcpyDeviceToHost));
    if (d2 && m) HIPCHK(hipMemcpy(d2, c->d_d2, sizeof(double) * m, hipMemcpyDeviceToHost));
    if (idx && m) HIPCHK(hipMemcpy(idx, c->d_idx, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
    *nsamples = ns;
    *first_hit = fh;
    return PCT_OK;
}

// ---- stream variants of the planner arithmetic: device buffers, asynchronous on the caller's stream ------------------------------
int pct_inflate_batch_dev(pct_cloud *c, const pct_inflate_params *p, const double *d_pts, int64_t Q, double *d_radius, uint32_t *d_idx,
                          double *d_d2, void *stream)
{
    if (!c || !p || Q < 0 || (Q > 0 && (!d_pts || !d_radius))) return fail(PCT_ERR_INVALID, "bad inflate_batch_dev arguments");
    if (Q == 0) return PCT_OK;
    PCTCHK(require_reserved(c, Q, "batch"));
    PCTCHK(order_after_mutations(c, (hipStream_t)stream));
    return inflate_dev(c, p, Q, (hipStream_t)stream, d_pts, nullptr, d_radius, d_idx, d_d2);
}

int pct_bezier_check_dev(pct_cloud *c, const pct_bezier_traj *traj, const pct_inflate_params *p, double t_start, double stop_time, double dt,
                         int64_t cap, double *d_pos, double *d_radius, double *d_d2, uint32_t *d_idx, long long *d_first_hit, int32_t *d_nsamples,
                         void *stream)
{
    if (!c || !traj || !p || !traj->polycoef || !traj->seg_time || !traj->orders || traj->nseg <= 0 || !(dt > 0) || cap <= 0 || !d_radius ||
        !d_first_hit || !d_nsamples)
        return fail(PCT_ERR_INVALID, "bad bezier_check_dev arguments");
    if (cap > kBezierCapMax || cap > c->qcap) return fail(PCT_ERR_INVALID, "cap %lld exceeds %lld (4096, and the reserved batch size)", (long long)cap,
                                                          (long long)std::min<int64_t>(kBezierCapMax, c->qcap));
    PCTCHK(bezier_check_orders(traj));
    hipStream_t s = (hipStream_t)stream;
    PCTCHK(order_after_mutations(c, s));
    PCTCHK(bezier_stage_coef(c, traj, s, true));
    return bezier_staged_enqueue(c, traj, p, t_start, stop_time, dt, cap, s, d_pos ? d_pos : c->d_pts64, d_radius, d_idx, d_d2, d_first_hit, d_nsamples);
}

// ---- the sampled Bezier check for B trajectories at once (bezier_batch.hpp; contract: pct_engine.h, "Batched Bezier check") ------
namespace {
// nsamples_b and m_b of every trajectory, then the offsets: one lane per trajectory, one block-scan over the B + 1 entries
int bb_count_scan(const BbDesc &D, pct_traj_verdict *d_verdict, long long *d_offsets, hipStream_t s)
{
    bb_count_kernel<<<ceil_div(D.B + 1, 256), 256, 0, s>>>(D, d_verdict, d_offsets);
    scan_tile_sums_kernel<uint64_t><<<1, 256, 0, s>>>(reinterpret_cast<uint64_t *>(d_offsets), (uint32_t)(D.B + 1), ScanDoneNothing{});
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

// fill, evaluate and inflate `nslots` slots, then fold every row into its verdict.  Positions, radii, indices and distances stay in the
// cloud's query workspaces (nslots <= c->qcap); (segment, t) per slot borrow d_count / d_r2, which only the radius counts use.
int bb_check_slots(pct_cloud *c, const BbDesc &D, const pct_inflate_params *p, const long long *d_offsets, long long list_cap, int64_t nslots,
                   pct_traj_verdict *d_verdict, hipStream_t s)
{
    if (nslots > 0) {
        const bool pad = c->count > 0;
        bb_fill_kernel<<<ceil_div(D.B, 256), 256, 0, s>>>(D, d_offsets, list_cap, c->d_count, c->d_r2);
        bb_eval_kernel<<<ceil_div(nslots, 128), 128, 0, s>>>(D, d_offsets, list_cap, nslots, c->d_count, c->d_r2, pad ? c->x : nullptr, pad ? c->y : nullptr,
                                                             pad ? c->z : nullptr, c->d_pts64);
        PCTCHK(inflate_dev(c, p, nslots, s));
    }
    bb_verdict_kernel<<<ceil_div(D.B, 4), 256, 0, s>>>(D.B, d_offsets, list_cap, c->d_radius, d_verdict);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}
}  // namespace

int pct_bezier_check_batch(pct_cloud *c, const pct_bezier_batch *batch, const pct_inflate_params *p, double stop_time, double dt, int64_t cap,
                           pct_traj_verdict *verdict, int64_t *offsets, int64_t list_cap, double *pos, double *radius, double *d2, uint32_t *idx)
{
    if (!c || !batch || !p || batch->B < 0 || cap <= 0 || !(dt > 0) || list_cap < 0) return fail(PCT_ERR_INVALID, "bad bezier_check_batch arguments");
    const int64_t B = batch->B;
    if (B > 0 && (!batch->polycoef || !batch->seg_time || !batch->orders || !batch->seg_offsets || !verdict))
        return fail(PCT_ERR_INVALID, "bad bezier_check_batch arguments: a null array");
    if (B >= 0x7FFFFFFFll) return fail(PCT_ERR_INVALID, "bezier_check_batch: B = %lld", (long long)B);
    PCTCHK(bezier_check_batch_layout(batch, "bezier_check_batch"));
    for (int64_t b = 0; b < B; b++) {
        double sum = 0.0;
        for (int32_t i = batch->seg_offsets[b]; i < batch->seg_offsets[b + 1]; i++) sum += batch->seg_time[i];
        // the enumeration must end on the device: a batch for candidate sets, not for logs
        if (!(std::min(stop_time, sum) / dt <= (double)kBbLoopBound))
            return fail(PCT_ERR_INVALID, "bezier_check_batch: trajectory %lld would enumerate more than 2^20 samples", (long long)b);
    }
    if (cap > kBezierCapMax) cap = kBezierCapMax;
    if (B == 0) {
        if (offsets) offsets[0] = 0;
        return PCT_OK;
    }
    PCTCHK(ring_finish_pending(c));              // rolling map: an append in flight is finished first and the answer sees its frame
    hipStream_t s = g_stream;
    const int32_t total_seg = batch->seg_offsets[B];
    const pct_bezier_traj all{ batch->polycoef, batch->row_stride, batch->seg_time, batch->orders, total_seg };
    PCTCHK(bezier_stage_coef(c, &all, s, false));
    if ((size_t)B + 1 > c->bb_cap) {
        HIPCHK(hipStreamSynchronize(s));
        const size_t n = pow2_at_least<size_t>(256, (size_t)B + 1);
        // bb_segoff never shrinks: the certified check may have grown it further on its own (bb_cap is a minimum)
        PCTCHK(regrow(c->bb_cap, n, part(c->bb_segoff, std::max(n, c->bb_segoff.capacity())), part(c->bb_tstart, n), part(c->bb_verdict, n), part(c->bb_off, n)));
    }
    HIPCHK(hipMemcpyAsync(c->bb_segoff, batch->seg_offsets, sizeof(int32_t) * (B + 1), hipMemcpyHostToDevice, s));
    if (batch->t_start) HIPCHK(hipMemcpyAsync(c->bb_tstart, batch->t_start, sizeof(double) * B, hipMemcpyHostToDevice, s));
    const BbDesc D{ c->d_coef, (long long)batch->row_stride, c->d_segtime, c->d_orders, c->bb_segoff, batch->t_start ? c->bb_tstart.get() : nullptr,
                    (long long)B, stop_time, dt, (long long)cap };
    PCTCHK(bb_count_scan(D, c->bb_verdict, c->bb_off, s));
    std::vector<int64_t> own;
    if (!offsets) { own.resize((size_t)B + 1); offsets = own.data(); }
    HIPCHK(hipMemcpyAsync(offsets, c->bb_off, sizeof(int64_t) * (B + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));             // the one host read: the total sizes the workspaces and the launches
    const int64_t total = offsets[B];
    if (total > 0x7FFFFFFFll) return fail(PCT_ERR_CAPACITY, "bezier_check_batch: %lld samples in one batch, more than 2^31 - 1", (long long)total);
    PCTCHK(pct_cloud_reserve_queries(c, total));
    PCTCHK(ask_twice_after_overrun(c, [&]() -> int {
        PCTCHK(bb_check_slots(c, D, p, c->bb_off, total, total, c->bb_verdict, s));
        HIPCHK(hipMemcpyAsync(verdict, c->bb_verdict, sizeof(pct_traj_verdict) * B, hipMemcpyDeviceToHost, s));
        if (own.empty() && total > 0 && total <= list_cap) {
            if (pos) HIPCHK(hipMemcpyAsync(pos, c->d_pts64, sizeof(double) * 3 * total, hipMemcpyDeviceToHost, s));
            if (radius) HIPCHK(hipMemcpyAsync(radius, c->d_radius, sizeof(double) * total, hipMemcpyDeviceToHost, s));
            if (d2) HIPCHK(hipMemcpyAsync(d2, c->d_d2, sizeof(double) * total, hipMemcpyDeviceToHost, s));
            if (idx) HIPCHK(hipMemcpyAsync(idx, c->d_idx, sizeof(uint32_t) * total, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
        return PCT_OK;
    }));
    return PCT_OK;
}

int pct_bezier_check_batch_dev(pct_cloud *c, const pct_bezier_batch *d_batch_fields, const pct_inflate_params *p, double stop_time, double dt,
                               int64_t cap, pct_traj_verdict *d_verdict, int64_t *d_offsets, int64_t list_cap, double *d_pos, double *d_radius,
                               double *d_d2, uint32_t *d_idx, void *stream)
{
    const pct_bezier_batch *bt = d_batch_fields;
    if (!c || !bt || !p || bt->B < 0 || bt->B >= 0x7FFFFFFFll || cap <= 0 || !(dt > 0) || list_cap < 0 || !d_offsets)
        return fail(PCT_ERR_INVALID, "bad bezier_check_batch_dev arguments");
    if (bt->B > 0 && (!bt->polycoef || !bt->seg_time || !bt->orders || !bt->seg_offsets || !d_verdict))
        return fail(PCT_ERR_INVALID, "bad bezier_check_batch_dev arguments: a null array");
    PCTCHK(require_reserved(c, list_cap, "list_cap"));
    if (cap > kBezierCapMax) cap = kBezierCapMax;
    hipStream_t s = (hipStream_t)stream;
    if (bt->B == 0) {
        HIPCHK(hipMemsetAsync(d_offsets, 0, sizeof(int64_t), s));
        return PCT_OK;
    }
    PCTCHK(order_after_mutations(c, s));
    const BbDesc D{ bt->polycoef, (long long)bt->row_stride, bt->seg_time, bt->orders, bt->seg_offsets, bt->t_start, (long long)bt->B, stop_time, dt, (long long)cap };
    long long *off = reinterpret_cast<long long *>(d_offsets);
    PCTCHK(bb_count_scan(D, d_verdict, off, s));
    // the total stays on the device: the per-slot launches are sized from list_cap and every kernel guards on offsets[B]
    PCTCHK(bb_check_slots(c, D, p, off, list_cap, list_cap, d_verdict, s));
    if (list_cap > 0 && (d_pos || d_radius || d_d2 || d_idx)) {
        bb_export_kernel<<<ceil_div(list_cap, 256), 256, 0, s>>>(bt->B, off, list_cap, c->d_pts64, c->d_radius, c->d_d2, c->d_idx, d_pos, d_radius, d_d2, d_idx);
        HIPCHK(hipGetLastError());
    }
    return PCT_OK;
}

// ---- the certified Bezier check (bezier_certify.hpp; contract: pct_engine.h, "Certified Bezier check") ---------------------------
// The host forms of the certified check: whole trajectories (`window` false: horizon and batch->t_start are not read), or the window
// [t_start, t_start + horizon) of each ("Windows of a trajectory").  One frame; the window form differs in what seeds the pieces.
static int certify_host(pct_cloud *c, int algo, const pct_bezier_batch *batch, bool window, const double *horizon, double margin, int32_t max_depth,
                        int64_t piece_cap, pct_traj_certificate *cert, int64_t stats[3], const char *name)
{
    if (!c || !batch || batch->B < 0 || batch->B >= 0x7FFFFFFFll) return fail(PCT_ERR_INVALID, "bad %s arguments", name);
    if (bc_bad_scalars(margin, max_depth, piece_cap))
        return fail(PCT_ERR_INVALID, "%s: margin %g, max_depth %d or piece_cap %lld out of range", name, margin, (int)max_depth, (long long)piece_cap);
    const int64_t B = batch->B;
    if (B > 0 && (!batch->polycoef || !batch->seg_time || !batch->orders || !batch->seg_offsets || !cert))
        return fail(PCT_ERR_INVALID, "bad %s arguments: a null array", name);
    PCTCHK(bezier_check_batch_layout(batch, name));
    const int64_t total_seg = B > 0 ? batch->seg_offsets[B] : 0;
    if (piece_cap < total_seg)
        return fail(PCT_ERR_INVALID, "%s: piece_cap %lld is below the %lld segments", name, (long long)piece_cap, (long long)total_seg);
    PCTCHK(ring_finish_pending(c));              // rolling map: an append in flight is finished first and the answer sees its frame
    Path path;
    PCTCHK(resolve_algo(c, Op::Capsule, algo, total_seg, &path));
    if (B == 0) {
        if (stats) stats[0] = stats[1] = stats[2] = 0;
        return PCT_OK;
    }
    hipStream_t s = g_stream;
    const pct_bezier_traj all{ batch->polycoef, batch->row_stride, batch->seg_time, batch->orders, (int32_t)total_seg };
    PCTCHK(bezier_stage_coef(c, &all, s, false));
    PCTCHK(bc_reserve(c, c->bb_segoff, (size_t)B + 1, s));
    PCTCHK(bc_reserve(c, c->bc_cert, (size_t)B, s));
    PCTCHK(bc_reserve(c, c->bc_stats, 3, s));
    PCTCHK(bc_traj_room(c, B, s));
    HIPCHK(hipMemcpyAsync(c->bb_segoff, batch->seg_offsets, sizeof(int32_t) * (B + 1), hipMemcpyHostToDevice, s));
    BcRun R{ BcDesc{ c->d_coef, (long long)batch->row_stride, c->d_segtime, c->d_orders, c->bb_segoff, (long long)B }, margin, (int)max_depth, piece_cap, path,
             c->bc_cert, c->bc_stats };
    if (window) PCTCHK(bc_window_stage(c, batch->t_start, horizon, B, total_seg, s, &R.W));
    return ask_twice_after_overrun(c, [&]() -> int {
        PCTCHK(bc_room(c, 0, total_seg, s));
        PCTCHK(bc_seed(c, R, total_seg, s));
        int64_t live = total_seg;
        for (int round = 0; round <= R.max_depth && live > 0; round++) {
            // the children of this round's pieces number at most 2 * live and at most piece_cap
            PCTCHK(bc_room(c, (round & 1) ^ 1, std::min<int64_t>(2 * live, piece_cap), s));
            PCTCHK(bc_round_room(c, live, s));
            PCTCHK(pct_cloud_reserve_queries(c, 2 * live));
            PCTCHK(bc_round(c, R, round, live, s));
            BcCtl h{};
            HIPCHK(hipMemcpyAsync(&h, c->bc_ctl, sizeof(BcCtl), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));     // the round's one host read: the live count sizes the next round
            live = h.live;
        }
        PCTCHK(bc_finish(c, R, s));
        HIPCHK(hipMemcpyAsync(cert, c->bc_cert, sizeof(pct_traj_certificate) * B, hipMemcpyDeviceToHost, s));
        if (stats) HIPCHK(hipMemcpyAsync(stats, c->bc_stats, sizeof(int64_t) * 3, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return PCT_OK;
    });
}

int pct_bezier_certify_batch(pct_cloud *c, int algo, const pct_bezier_batch *batch, double margin, int32_t max_depth, int64_t piece_cap,
                             pct_traj_certificate *cert, int64_t stats[3])
{
    return certify_host(c, algo, batch, false, nullptr, margin, max_depth, piece_cap, cert, stats, "bezier_certify_batch");
}

int pct_bezier_certify_window_batch(pct_cloud *c, int algo, const pct_bezier_batch *batch, const double *horizon, double margin, int32_t max_depth,
                                    int64_t piece_cap, pct_traj_certificate *cert, int64_t stats[3])
{
    return certify_host(c, algo, batch, true, horizon, margin, max_depth, piece_cap, cert, stats, "bezier_certify_window_batch");
}

// the device forms of the certified check, whole trajectories or windows, as certify_host
static int certify_dev(pct_cloud *c, int algo, const pct_bezier_batch *bt, bool window, const double *d_horizon, double margin, int32_t max_depth,
                       int64_t piece_cap, pct_traj_certificate *d_cert, int64_t *d_stats, void *stream, const char *name)
{
    if (!c || !bt || bt->B < 0 || bt->B >= 0x7FFFFFFFll) return fail(PCT_ERR_INVALID, "bad %s arguments", name);
    if (bc_bad_scalars(margin, max_depth, piece_cap))
        return fail(PCT_ERR_INVALID, "%s: margin %g, max_depth %d or piece_cap %lld out of range", name, margin, (int)max_depth, (long long)piece_cap);
    if (bt->B > 0 && (!bt->polycoef || !bt->seg_time || !bt->orders || !bt->seg_offsets || !d_cert))
        return fail(PCT_ERR_INVALID, "bad %s arguments: a null array", name);
    Path path;
    PCTCHK(resolve_algo(c, Op::Capsule, algo, piece_cap, &path));
    hipStream_t s = (hipStream_t)stream;
    if (bt->B == 0) {
        if (d_stats) HIPCHK(hipMemsetAsync(d_stats, 0, sizeof(int64_t) * 3, s));
        return PCT_OK;
    }
    // Under capture only the two index paths are served.  The streaming capsule count adds into counts that a memset in front of it
    // clears, and a captured graph was seen to replay that memset without effect (counts piling up from replay to replay, DESIGN.md
    // section 4); the index forms store their counts.  The streaming k-NN kernel is refused under capture in the same way.
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    if ((path == Path::Stream || path == Path::Empty) && (c->capturing || (hipStreamIsCapturing(s, &cst) == hipSuccess && cst != hipStreamCaptureStatusNone)))
        return fail(PCT_ERR_INVALID, "%s: during graph capture the cloud needs its cell index or its rolling-map index", name);
    PCTCHK(require_reserved(c, 2 * piece_cap, "2 * piece_cap"));
    PCTCHK(bc_room(c, 0, piece_cap, s));
    PCTCHK(bc_room(c, 1, piece_cap, s));
    PCTCHK(bc_round_room(c, piece_cap, s));
    PCTCHK(bc_traj_room(c, bt->B, s));
    if (window) PCTCHK(bc_reserve(c, c->bc_win, 2 * (size_t)piece_cap, s));
    PCTCHK(order_after_mutations(c, s));
    BcRun R{ BcDesc{ bt->polycoef, (long long)bt->row_stride, bt->seg_time, bt->orders, bt->seg_offsets, (long long)bt->B }, margin, (int)max_depth, piece_cap,
             path, d_cert, reinterpret_cast<long long *>(d_stats) };
    if (window) R.W = BcWinDesc{ bt->t_start, d_horizon, c->bc_win };
    PCTCHK(bc_seed(c, R, piece_cap, s));
    // the live count stays on the device: every round is sized by piece_cap and every lane guards on it
    for (int round = 0; round <= R.max_depth; round++) PCTCHK(bc_round(c, R, round, piece_cap, s));
    return bc_finish(c, R, s);
}

int pct_bezier_certify_batch_dev(pct_cloud *c, int algo, const pct_bezier_batch *d_batch_fields, double margin, int32_t max_depth, int64_t piece_cap,
                                 pct_traj_certificate *d_cert, int64_t *d_stats, void *stream)
{
    return certify_dev(c, algo, d_batch_fields, false, nullptr, margin, max_depth, piece_cap, d_cert, d_stats, stream, "bezier_certify_batch_dev");
}

int pct_bezier_certify_window_batch_dev(pct_cloud *c, int algo, const pct_bezier_batch *d_batch_fields, const double *d_horizon, double margin,
                                        int32_t max_depth, int64_t piece_cap, pct_traj_certificate *d_cert, int64_t *d_stats, void *stream)
{
    return certify_dev(c, algo, d_batch_fields, true, d_horizon, margin, max_depth, piece_cap, d_cert, d_stats, stream, "bezier_certify_window_batch_dev");
}

// ---- the trajectory clearance (bezier_clearance.hpp; contract: pct_engine.h, "Trajectory clearance") -------------------------------
// the host forms of the clearance, whole trajectories or windows, as certify_host
static int clearance_host(pct_cloud *c, int algo, const pct_bezier_batch *batch, bool window, const double *horizon, double tol, double cap,
                          int32_t max_depth, int64_t piece_cap, pct_traj_clearance *out, int64_t stats[3], const char *name)
{
    if (!c || !batch || batch->B < 0 || batch->B >= 0x7FFFFFFFll) return fail(PCT_ERR_INVALID, "bad %s arguments", name);
    if (cl_bad_scalars(tol, cap, max_depth, piece_cap))
        return fail(PCT_ERR_INVALID, "%s: tol %g, cap %g, max_depth %d or piece_cap %lld out of range", name, tol, cap, (int)max_depth, (long long)piece_cap);
    const int64_t B = batch->B;
    if (B > 0 && (!batch->polycoef || !batch->seg_time || !batch->orders || !batch->seg_offsets || !out))
        return fail(PCT_ERR_INVALID, "bad %s arguments: a null array", name);
    PCTCHK(bezier_check_batch_layout(batch, name));
    const int64_t total_seg = B > 0 ? batch->seg_offsets[B] : 0;
    if (piece_cap < total_seg)
        return fail(PCT_ERR_INVALID, "%s: piece_cap %lld is below the %lld segments", name, (long long)piece_cap, (long long)total_seg);
    PCTCHK(ring_finish_pending(c));              // rolling map: an append in flight is finished first and the answer sees its frame
    Path path;
    PCTCHK(resolve_algo(c, Op::Capsule, algo, total_seg, &path));
    if (B == 0) {
        if (stats) stats[0] = stats[1] = stats[2] = 0;
        return PCT_OK;
    }
    hipStream_t s = g_stream;
    const pct_bezier_traj all{ batch->polycoef, batch->row_stride, batch->seg_time, batch->orders, (int32_t)total_seg };
    PCTCHK(bezier_stage_coef(c, &all, s, false));
    PCTCHK(bc_reserve(c, c->bb_segoff, (size_t)B + 1, s));
    PCTCHK(bc_reserve(c, c->cl_out, (size_t)B, s));
    PCTCHK(bc_reserve(c, c->bc_stats, 3, s));
    PCTCHK(cl_traj_room(c, B, s));
    HIPCHK(hipMemcpyAsync(c->bb_segoff, batch->seg_offsets, sizeof(int32_t) * (B + 1), hipMemcpyHostToDevice, s));
    ClRun R{ BcDesc{ c->d_coef, (long long)batch->row_stride, c->d_segtime, c->d_orders, c->bb_segoff, (long long)B }, tol, cap, (int)max_depth, piece_cap, path,
             c->cl_out, c->bc_stats };
    if (window) PCTCHK(bc_window_stage(c, batch->t_start, horizon, B, total_seg, s, &R.W));
    return ask_twice_after_overrun(c, [&]() -> int {
        PCTCHK(bc_room(c, 0, total_seg, s));
        PCTCHK(cl_seed(c, R, total_seg, s));
        int64_t live = total_seg;
        for (int round = 0; round <= R.max_depth && live > 0; round++) {
            // the children of this round's pieces number at most 2 * live and at most piece_cap
            PCTCHK(bc_room(c, (round & 1) ^ 1, std::min<int64_t>(2 * live, piece_cap), s));
            PCTCHK(cl_round_room(c, live, s));
            PCTCHK(pct_cloud_reserve_queries(c, 2 * live));
            PCTCHK(cl_round(c, R, round, live, s));
            BcCtl h{};
            HIPCHK(hipMemcpyAsync(&h, c->bc_ctl, sizeof(BcCtl), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));     // the round's one host read: the live count sizes the next round
            live = h.live;
        }
        PCTCHK(cl_finish(c, R, s));
        HIPCHK(hipMemcpyAsync(out, c->cl_out, sizeof(pct_traj_clearance) * B, hipMemcpyDeviceToHost, s));
        if (stats) HIPCHK(hipMemcpyAsync(stats, c->bc_stats, sizeof(int64_t) * 3, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return PCT_OK;
    });
}

int pct_bezier_clearance_batch(pct_cloud *c, int algo, const pct_bezier_batch *batch, double tol, double cap, int32_t max_depth, int64_t piece_cap,
                               pct_traj_clearance *out, int64_t stats[3])
{
    return clearance_host(c, algo, batch, false, nullptr, tol, cap, max_depth, piece_cap, out, stats, "bezier_clearance_batch");
}

int pct_bezier_clearance_window_batch(pct_cloud *c, int algo, const pct_bezier_batch *batch, const double *horizon, double tol, double cap,
                                      int32_t max_depth, int64_t piece_cap, pct_traj_clearance *out, int64_t stats[3])
{
    return clearance_host(c, algo, batch, true, horizon, tol, cap, max_depth, piece_cap, out, stats, "bezier_clearance_window_batch");
}

// the device forms of the clearance, whole trajectories or windows
static int clearance_dev(pct_cloud *c, int algo, const pct_bezier_batch *bt, bool window, const double *d_horizon, double tol, double cap, int32_t max_depth,
                         int64_t piece_cap, pct_traj_clearance *d_out, int64_t *d_stats, void *stream, const char *name)
{
    if (!c || !bt || bt->B < 0 || bt->B >= 0x7FFFFFFFll) return fail(PCT_ERR_INVALID, "bad %s arguments", name);
    if (cl_bad_scalars(tol, cap, max_depth, piece_cap))
        return fail(PCT_ERR_INVALID, "%s: tol %g, cap %g, max_depth %d or piece_cap %lld out of range", name, tol, cap, (int)max_depth, (long long)piece_cap);
    if (bt->B > 0 && (!bt->polycoef || !bt->seg_time || !bt->orders || !bt->seg_offsets || !d_out))
        return fail(PCT_ERR_INVALID, "bad %s arguments: a null array", name);
    Path path;
    PCTCHK(resolve_algo(c, Op::Capsule, algo, piece_cap, &path));
    hipStream_t s = (hipStream_t)stream;
    if (bt->B == 0) {
        if (d_stats) HIPCHK(hipMemsetAsync(d_stats, 0, sizeof(int64_t) * 3, s));
        return PCT_OK;
    }
    // under capture only the two index paths are served, as for the certified check: the streaming nearest-neighbour kernels keep
    // partial results in scratch that is sized and cleared outside the graph
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    if ((path == Path::Stream || path == Path::Empty) && (c->capturing || (hipStreamIsCapturing(s, &cst) == hipSuccess && cst != hipStreamCaptureStatusNone)))
        return fail(PCT_ERR_INVALID, "%s: during graph capture the cloud needs its cell index or its rolling-map index", name);
    PCTCHK(require_reserved(c, 2 * piece_cap, "2 * piece_cap"));
    PCTCHK(bc_room(c, 0, piece_cap, s));
    PCTCHK(bc_room(c, 1, piece_cap, s));
    PCTCHK(cl_round_room(c, piece_cap, s));
    PCTCHK(cl_traj_room(c, bt->B, s));
    if (window) PCTCHK(bc_reserve(c, c->bc_win, 2 * (size_t)piece_cap, s));
    PCTCHK(order_after_mutations(c, s));
    ClRun R{ BcDesc{ bt->polycoef, (long long)bt->row_stride, bt->seg_time, bt->orders, bt->seg_offsets, (long long)bt->B }, tol, cap, (int)max_depth, piece_cap,
             path, d_out, reinterpret_cast<long long *>(d_stats) };
    if (window) R.W = BcWinDesc{ bt->t_start, d_horizon, c->bc_win };
    PCTCHK(cl_seed(c, R, piece_cap, s));
    // the live count stays on the device: every round is sized by piece_cap and every lane guards on it
    for (int round = 0; round <= R.max_depth; round++) PCTCHK(cl_round(c, R, round, piece_cap, s));
    return cl_finish(c, R, s);
}

int pct_bezier_clearance_batch_dev(pct_cloud *c, int algo, const pct_bezier_batch *d_batch_fields, double tol, double cap, int32_t max_depth,
                                   int64_t piece_cap, pct_traj_clearance *d_out, int64_t *d_stats, void *stream)
{
    return clearance_dev(c, algo, d_batch_fields, false, nullptr, tol, cap, max_depth, piece_cap, d_out, d_stats, stream, "bezier_clearance_batch_dev");
}

int pct_bezier_clearance_window_batch_dev(pct_cloud *c, int algo, const pct_bezier_batch *d_batch_fields, const double *d_horizon, double tol, double cap,
                                          int32_t max_depth, int64_t piece_cap, pct_traj_clearance *d_out, int64_t *d_stats, void *stream)
{
    return clearance_dev(c, algo, d_batch_fields, true, d_horizon, tol, cap, max_depth, piece_cap, d_out, d_stats, stream, "bezier_clearance_window_batch_dev");
}

// ---- hipGraph plan -----------------------------------------------------------------------
static int plan_capture_nn(pct_plan *p)
{
    pct_cloud *c = p->c;
    PCTCHK(pct_cloud_reserve_queries(c, p->Q));
    return plan_capture(p, [&] {
        (void)hipMemcpyAsync(p->d_q, p->h_q, sizeof(float) * 3 * p->Q, hipMemcpyHostToDevice, g_stream);
        const int st = nn_dev(c, p->algo, p->d_q, p->Q, p->d_idx, p->d_d2, g_stream);
        (void)hipMemcpyAsync(p->h_idx, p->d_idx, sizeof(uint32_t) * p->Q, hipMemcpyDeviceToHost, g_stream);
        (void)hipMemcpyAsync(p->h_d2, p->d_d2, sizeof(double) * p->Q, hipMemcpyDeviceToHost, g_stream);
        return st;
    });
}

int pct_plan_create_nn(pct_cloud *c, int algo, int64_t Q, pct_plan **out)
{
    if (!c || !out || Q <= 0) return fail(PCT_ERR_INVALID, "bad plan arguments");
    PCTCHK(pct_cloud_reserve_queries(c, Q));
    pct_plan *p = new (std::nothrow) pct_plan();
    if (!p) return fail(PCT_ERR_ALLOC, "host allocation failed");
    p->c = c;
    p->Q = Q;
    p->algo = algo;
    int st = p->h_q.reset(3 * Q);
    if (!st) st = p->h_idx.reset(Q);
    if (!st) st = p->h_d2.reset(Q);
    if (!st) st = p->d_q.reset(3 * Q);
    if (!st) st = p->d_idx.reset(Q);
    if (!st) st = p->d_d2.reset(Q);
    if (!st) st = plan_capture_nn(p);
    if (st) { pct_plan_destroy(p); return st; }
    *out = p;
    return PCT_OK;
}

int pct_plan_run(pct_plan *p, const float *q, uint32_t *idx, double *d2)
{
    if (!p || p->kind != 0 || !q || !idx || !d2) return fail(PCT_ERR_INVALID, "bad plan_run arguments");
    // The captured kernels hold the cloud's point count, its index description and its workspace pointers.  When any of them
    // has changed since the capture (upload / append, grid build or drop, a larger batch elsewhere that reallocated the
    // workspaces) the cloud's generation has moved on and the graph is captured again before it runs.
    if (p->generation != p->c->generation) PCTCHK(plan_capture_nn(p));
    memcpy(p->h_q, q, sizeof(float) * 3 * p->Q);
    HIPCHK(hipGraphLaunch(p->exec, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    memcpy(idx, p->h_idx, sizeof(uint32_t) * p->Q);
    memcpy(d2, p->h_d2, sizeof(double) * p->Q);
    return PCT_OK;
}

int pct_plan_destroy(pct_plan *p)
{
    if (!p) return PCT_OK;
    if (g_stream) (void)hipStreamSynchronize(g_stream);
    if (p->exec) (void)hipGraphExecDestroy(p->exec);
    if (p->graph) (void)hipGraphDestroy(p->graph);
    replan_ctx_free(p->rx);
    delete p;
    return PCT_OK;
}

// ---- measurement -------------------------------------------------------------------------
int pct_last_kernel_ms(pct_cloud *c, float *ms)
{
    if (!c || !ms) return fail(PCT_ERR_INVALID, "bad arguments");
    if (!c->last3) return fail(PCT_ERR_INVALID, "no timed batch yet");
    HIPCHK(hipEventSynchronize(c->last3));
    HIPCHK(hipEventElapsedTime(ms, c->last2, c->last3));
    return PCT_OK;
}

// multi-GPU exchange helper (pointcloudtraj_amd/dist.py): cand[i] = idx_local[i] if this rank holds the global minimum, else INT32_MAX
int pct_merge_mask_dev(const double *d_d2_local, const double *d_d2_best, const uint32_t *d_idx_local, int32_t *d_cand, int64_t Q, void *stream)
{
    if (Q < 0 || (Q > 0 && (!d_d2_local || !d_d2_best || !d_idx_local || !d_cand))) return fail(PCT_ERR_INVALID, "bad merge_mask arguments");
    if (Q == 0) return PCT_OK;
    PCTCHK(require_init());
    merge_mask_kernel<<<ceil_div(Q, 256), 256, 0, (hipStream_t)stream>>>(d_d2_local, d_d2_best, d_idx_local, d_cand, (uint32_t)Q);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

int pct_merge_finish_dev(const int32_t *d_cand, uint32_t *d_idx, int64_t Q, void *stream)
{
    if (Q < 0 || (Q > 0 && (!d_cand || !d_idx))) return fail(PCT_ERR_INVALID, "bad merge_finish arguments");
    if (Q == 0) return PCT_OK;
    PCTCHK(require_init());
    merge_finish_kernel<<<ceil_div(Q, 256), 256, 0, (hipStream_t)stream>>>(d_cand, d_idx, (uint32_t)Q);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

// ---- device helpers of the routed multi-GPU form (include/pct_shard.h; host logic in csrc/shard.cpp) ----------------------------
int pct_cloud_upload_aos_dev(pct_cloud *c, const void *d_pts, int64_t n, int64_t stride_bytes)
{
    if (!c || n < 0 || (n > 0 && !d_pts) || stride_bytes < 12 || (stride_bytes & 3)) return fail(PCT_ERR_INVALID, "bad upload arguments");
    if (n > c->cap) return fail(PCT_ERR_CAPACITY, "%lld points > capacity %lld", (long long)n, (long long)c->cap);
    if (c->host_mapped) return fail(PCT_ERR_INVALID, "small (host-mapped) clouds are filled from host buffers");
    drop_grid(c);
    if (n) {
        deinterleave_kernel<<<ceil_div(n, 256), 256, 0, g_stream>>>(static_cast<const unsigned char *>(d_pts), (uint32_t)stride_bytes, (uint32_t)n, c->x, c->y, c->z, 0u);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(g_stream));
    }
    c->count = n;
    c->ring_next = n % std::max<int64_t>(c->cap, 1);
    c->ring_removed_any = false;
    return after_replace(c);
}

static int route_cuts(const double *cuts, int world, int axis, RouteCuts *C)
{
    if (!cuts || world < 1 || world > kRouteMaxWorld || axis < 0 || axis > 2) return fail(PCT_ERR_INVALID, "bad slab description (at most %d ranks)", kRouteMaxWorld);
    C->world = world; C->axis = axis;
    for (int k = 0; k <= world; k++) C->cut[k] = cuts[k];
    return PCT_OK;
}

int pct_route_owner_dev(const double *cuts, int world, int axis, int rank, const float *d_q, int64_t Q, uint32_t *d_counts, uint32_t *d_mine_ids,
                        float *d_mine_q, void *stream)
{
    if (Q < 0 || rank < 0 || rank >= world || (Q > 0 && (!d_q || !d_counts || !d_mine_ids || !d_mine_q))) return fail(PCT_ERR_INVALID, "bad route_owner arguments");
    RouteCuts C{};
    PCTCHK(route_cuts(cuts, world, axis, &C));
    PCTCHK(require_init());
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * (size_t)world, s));
    if (Q) route_owner_kernel<<<ceil_div(Q, 256), 256, 0, s>>>(C, rank, d_q, (uint32_t)Q, d_counts, d_mine_ids, d_mine_q);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

int pct_route_owner_all_dev(const double *cuts, int world, int axis, const float *d_q, int64_t Q, uint32_t *d_counts, unsigned char *d_owner, void *stream)
{
    if (Q < 0 || (Q > 0 && (!d_q || !d_counts || !d_owner))) return fail(PCT_ERR_INVALID, "bad route_owner_all arguments");
    RouteCuts C{};
    PCTCHK(route_cuts(cuts, world, axis, &C));
    PCTCHK(require_init());
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * (size_t)world, s));
    if (Q) route_owner_all_kernel<<<ceil_div(Q, 256), 256, 0, s>>>(C, d_q, (uint32_t)Q, d_counts, d_owner);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

int pct_route_partition_dev(const uint32_t *offsets, int world, const unsigned char *d_owner, const float *d_q, int64_t Q, uint32_t *d_cursors,
                            float *d_out_xyz, uint32_t *d_out_slot, void *stream)
{
    if (!offsets || world < 1 || world > kRouteMaxWorld || Q < 0 || (Q > 0 && (!d_owner || !d_q || !d_cursors || !d_out_xyz || !d_out_slot)))
        return fail(PCT_ERR_INVALID, "bad route_partition arguments");
    RouteOffsets O{};
    for (int k = 0; k < world; k++) O.v[k] = offsets[k];
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(d_cursors, 0, sizeof(uint32_t) * (size_t)world, s));
    if (Q) route_partition_kernel<<<ceil_div(Q, 256), 256, 0, s>>>(O, d_owner, d_q, (uint32_t)Q, d_cursors, d_out_xyz, d_out_slot);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

int pct_route_certify_dev(int axis, double lo_edge, double hi_edge, const float *d_mine_q, const uint32_t *d_mine_ids, int64_t m, const uint32_t *d_lidx,
                          const double *d_ld2, const uint32_t *d_gid, void *d_answers, void *stream)
{
    if (m < 0 || axis < 0 || axis > 2 || (m > 0 && (!d_mine_q || !d_mine_ids || !d_lidx || !d_ld2 || !d_gid || !d_answers))) return fail(PCT_ERR_INVALID, "bad route_certify arguments");
    if (m == 0) return PCT_OK;
    route_certify_kernel<<<ceil_div(m, 256), 256, 0, (hipStream_t)stream>>>(axis, lo_edge, hi_edge, d_mine_q, d_mine_ids, (uint32_t)m, d_lidx, d_ld2, d_gid,
                                                                             static_cast<RouteAnswer *>(d_answers));
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

int pct_route_scatter_dev(const void *d_answers, int64_t n, uint32_t *d_idx, double *d_d2, uint32_t *d_flag_count, uint32_t *d_flag_ids, void *stream)
{
    if (n < 0 || (n > 0 && (!d_answers || !d_idx || !d_d2 || !d_flag_count || !d_flag_ids))) return fail(PCT_ERR_INVALID, "bad route_scatter arguments");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(d_flag_count, 0, sizeof(uint32_t), s));
    if (n) route_scatter_kernel<<<ceil_div(n, 256), 256, 0, s>>>(static_cast<const RouteAnswer *>(d_answers), (uint32_t)n, d_idx, d_d2, d_flag_count, d_flag_ids);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

int pct_route_gather_queries_dev(const float *d_q, const uint32_t *d_ids, int64_t n, float *d_out, void *stream)
{
    if (n < 0 || (n > 0 && (!d_q || !d_ids || !d_out))) return fail(PCT_ERR_INVALID, "bad route_gather arguments");
    if (n) route_gather_queries_kernel<<<ceil_div(n, 256), 256, 0, (hipStream_t)stream>>>(d_q, d_ids, (uint32_t)n, d_out);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

int pct_route_to_global_dev(uint32_t *d_lidx, int64_t n, const uint32_t *d_gid, void *stream)
{
    if (n < 0 || (n > 0 && (!d_lidx || !d_gid))) return fail(PCT_ERR_INVALID, "bad route_to_global arguments");
    if (n) route_to_global_kernel<<<ceil_div(n, 256), 256, 0, (hipStream_t)stream>>>(d_lidx, (uint32_t)n, d_gid);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

int pct_route_put_back_dev(const uint32_t *d_ids, int64_t n, const uint32_t *d_idx, const double *d_d2, uint32_t *d_out_idx, double *d_out_d2, void *stream)
{
    if (n < 0 || (n > 0 && (!d_ids || !d_idx || !d_d2 || !d_out_idx || !d_out_d2))) return fail(PCT_ERR_INVALID, "bad route_put_back arguments");
    if (n) route_put_back_kernel<<<ceil_div(n, 256), 256, 0, (hipStream_t)stream>>>(d_ids, (uint32_t)n, d_idx, d_d2, d_out_idx, d_out_d2);
    HIPCHK(hipGetLastError());
    return PCT_OK;
}

int pct_set_timing(pct_cloud *c, int level)
{
    if (!c || level < 0 || level > 2) return fail(PCT_ERR_INVALID, "timing level must be 0, 1 or 2");
    c->timing_level = level;
    return PCT_OK;
}

int pct_set_timing_stride(pct_cloud *c, int stride)
{
    if (!c || stride < 1) return fail(PCT_ERR_INVALID, "timing stride must be >= 1");
    c->dom_stride = stride;
    c->dom_launch = 0;
    return PCT_OK;
}

int pct_kernel_ms_samples(pct_cloud *c, uint64_t *count)
{
    if (!c || !count) return fail(PCT_ERR_INVALID, "bad arguments");
    *count = c->dom_seq;
    return PCT_OK;
}

int pct_kernel_ms_history(pct_cloud *c, float *ms, int cap, int *n)
{
    if (!c || !ms || !n || cap <= 0) return fail(PCT_ERR_INVALID, "bad arguments");
    const uint64_t have = std::min<uint64_t>(c->dom_seq, pct_cloud::kDomRing);
    const int take = (int)std::min<uint64_t>(have, (uint64_t)cap);
    for (int i = 0; i < take; i++) {                       // oldest of the `take` most recent batches first
        const int slot = (int)((c->dom_seq - take + i) % pct_cloud::kDomRing);
        HIPCHK(hipEventSynchronize(c->dom_ring[2 * slot + 1]));
        HIPCHK(hipEventElapsedTime(&ms[i], c->dom_ring[2 * slot], c->dom_ring[2 * slot + 1]));
    }
    *n = take;
    return PCT_OK;
}

int pct_last_batch_ms(pct_cloud *c, float *ms)
{
    if (!c || !ms) return fail(PCT_ERR_INVALID, "bad arguments");
    if (!c->ev_valid) return fail(PCT_ERR_INVALID, "no timed batch yet");
    HIPCHK(hipEventSynchronize(c->ev1));
    HIPCHK(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return PCT_OK;
}

// test hook: the cell index as built (cell_start: ncells + 1 entries, records: 4 floats per point = x, y, z, bit-cast index)
int pct_debug_read_grid(pct_cloud *c, uint32_t *cell_start, float *records)
{
    if (!c || !c->has_grid) return fail(PCT_ERR_INVALID, "no cell index");
    HIPCHK(hipStreamSynchronize(g_stream));
    if (cell_start) HIPCHK(hipMemcpy(cell_start, c->cell_start, sizeof(uint32_t) * ((size_t)c->G.ncells + 1), hipMemcpyDeviceToHost));
    if (records) HIPCHK(hipMemcpy(records, c->sorted, sizeof(float4) * (size_t)c->count, hipMemcpyDeviceToHost));
    return PCT_OK;
}

int pct_debug_read_bounds(pct_cloud *c, float *out, int64_t Q)
{
    if (!c || !out || Q > c->qcap) return fail(PCT_ERR_INVALID, "bad arguments");
    HIPCHK(hipStreamSynchronize(g_stream));
    HIPCHK(hipMemcpy(out, c->d_bound, sizeof(float) * Q, hipMemcpyDeviceToHost));
    return PCT_OK;
}

int pct_debug_set_filter_mode(int mode)
{
    if (mode < -1 || mode > 1) return fail(PCT_ERR_INVALID, "filter mode must be -1 (automatic), 0 (direct form) or 1 (expanded form)");
    g_filter_mode = mode;
    return PCT_OK;
}

int pct_set_work_counters(pct_cloud *c, int enabled)
{
    if (!c) return fail(PCT_ERR_INVALID, "null cloud");
    c->count_work = enabled != 0;
    return PCT_OK;
}

int pct_last_work(pct_cloud *c, uint64_t *points_scanned, uint64_t *cells_scanned)
{
    if (!c) return fail(PCT_ERR_INVALID, "null cloud");
    uint64_t w[3];
    PCTCHK(pct_last_work_ex(c, w));
    if (points_scanned) *points_scanned = w[0];
    if (cells_scanned) *cells_scanned = w[1];
    return PCT_OK;
}

int pct_last_work_ex(pct_cloud *c, uint64_t out[3])
{
    if (!c || !out) return fail(PCT_ERR_INVALID, "bad arguments");
    out[0] = out[1] = out[2] = 0;
    if (c->host_work) { out[0] = c->host_points; return PCT_OK; }
    WorkCounters slots[kWorkSlots];
    HIPCHK(hipStreamSynchronize(g_stream));
    HIPCHK(hipMemcpy(slots, c->d_work, sizeof slots, hipMemcpyDeviceToHost));
    for (const WorkCounters &k : slots) { out[0] += k.points; out[1] += k.cells; out[2] += k.nodes; }
    return PCT_OK;
}

int pct_cloud_pyramid_info(const pct_cloud *c, int32_t *levels, int64_t *nodes, double *empty_fraction)
{
    if (!c || !c->has_grid) return fail(PCT_ERR_INVALID, "no cell index");
    if (levels) *levels = c->has_pyr ? c->P.nlev : 0;
    if (nodes) *nodes = c->has_pyr ? (int64_t)c->pyr_total : 0;
    if (empty_fraction) *empty_fraction = c->empty_frac;
    return PCT_OK;
}

int pct_debug_verify_grid(pct_cloud *c, uint64_t out[6])
{
    if (!c || !c->has_grid || !out) return fail(PCT_ERR_INVALID, "no cell index");
    const uint32_t n = (uint32_t)c->count;
    DevBuf<uint32_t> bitmap;
    DevBuf<unsigned long long> d_out;
    const size_t words = ((size_t)n + 31) / 32;
    int st = bitmap.reset(words);
    if (!st) st = d_out.reset(6);
    hipError_t e = hipSuccess;
    if (!st) {
        e = hipMemsetAsync(bitmap, 0, sizeof(uint32_t) * std::max<size_t>(words, 1), g_stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * 6, g_stream);
        if (e == hipSuccess) {
            grid_verify_kernel<<<(int)std::min<int64_t>(2048, (std::max<int64_t>(n, (int64_t)c->G.ncells) + 255) / 256), 256, 0, g_stream>>>(c->G, c->sorted, c->cell_start, n, bitmap, d_out);
            e = hipGetLastError();
        }
        unsigned long long h[6] = { 0, 0, 0, 0, 0, 0 };
        if (e == hipSuccess) e = hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, g_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        for (int k = 0; k < 6; k++) out[k] = h[k];
    }
    if (st) return st;
    if (e != hipSuccess) return fail(PCT_ERR_HIP, "verify_grid: %s", hipGetErrorString(e));
    return PCT_OK;
}

}  // extern "C"
