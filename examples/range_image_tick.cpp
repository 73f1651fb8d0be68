// range_image_tick.cpp -- two ticks of a lidar on the rolling map: ObstacleMap::clearSeenThroughRange and appendRangeImage
// (pct_engine.h, paragraph "Range images").  A 16 x 360 full-circle scan sees a wall and a box; tick 1 appends it.  In tick 2 the box
// is gone from the scan: the carve removes exactly the points the box left in the window, the wall stays, and the append files what
// the scan now sees behind the box.
// Self-checking: the window's rows after every step are compared, bit for bit, with a host loop over the contract's formulas
// (un-projection, projection with the two table searches, the seen-through test).  The driver's part -- the tables -- is here too:
// the column edges through pct_range_pseudo_angle, the row edges as tangents, the beams along the middle of their cells.
// Build: pointcloudtraj_amd/build.py (plain g++ with -ffp-contract=off, as the contract's one rounding per operation asks).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pct_obstacle_map.hpp"

static const int W = 360, H = 16;
static const double kPi = 3.14159265358979323846;

struct Scan {
    std::vector<double> col_edge, row_edge, col_dir, row_dir;
    pct_range_view view;
};

// an evenly spaced scan: columns of 1 degree from azimuth 0, rings of 2 degrees between -16 and +16 degrees of elevation
static void make_scan(Scan &s)
{
    s.col_edge.resize(W + 1); s.row_edge.resize(H + 1); s.col_dir.resize(2 * W); s.row_dir.resize(2 * H);
    for (int c = 0; c <= W; c++) { const double a = 2.0 * kPi * c / W; s.col_edge[c] = pct_range_pseudo_angle(std::cos(a), std::sin(a)); }
    s.col_edge[0] = 0.0; s.col_edge[W] = 4.0;                                          // a full circle, by the header's convention
    for (int c = 0; c < W; c++) { const double a = 2.0 * kPi * (c + 0.5) / W; s.col_dir[2 * c] = std::cos(a); s.col_dir[2 * c + 1] = std::sin(a); }
    const double lo = -16.0 * kPi / 180.0, step = 2.0 * kPi / 180.0;
    for (int r = 0; r <= H; r++) s.row_edge[r] = std::tan(lo + step * r);
    for (int r = 0; r < H; r++) { const double e = lo + step * (r + 0.5); s.row_dir[2 * r] = std::cos(e); s.row_dir[2 * r + 1] = std::sin(e); }
    pct_range_view &v = s.view;
    v = pct_range_view{};
    v.t[0] = 0.25; v.t[1] = -0.5; v.t[2] = 1.0;
    v.R[0] = v.R[4] = v.R[8] = 1.0;
    v.near_range = 0.1;
    v.width = W; v.height = H;
    v.col_edge = s.col_edge.data(); v.row_edge = s.row_edge.data(); v.col_dir = s.col_dir.data(); v.row_dir = s.row_dir.data();
}

// the sensor's side, not the library's: what each beam returns from a wall at x = 10 (|y| <= 30) and, when it is there, a box of
// 1 m around (4, 0, 1); +inf where a beam returns nothing
static std::vector<float> render(const Scan &s, bool with_box)
{
    std::vector<float> img((size_t)W * H, INFINITY);
    const double *t = s.view.t;
    for (int r = 0; r < H; r++)
        for (int c = 0; c < W; c++) {
            const double e[3] = { s.row_dir[2 * r] * s.col_dir[2 * c], s.row_dir[2 * r] * s.col_dir[2 * c + 1], s.row_dir[2 * r + 1] };
            double best = INFINITY;
            if (e[0] > 0.0) {
                const double rho = (10.0 - t[0]) / e[0];
                if (std::fabs(t[1] + rho * e[1]) <= 30.0) best = rho;
            }
            if (with_box) {
                const double lo[3] = { 3.5, -0.5, 0.5 }, hi[3] = { 4.5, 0.5, 1.5 };
                double t0 = 0.0, t1 = INFINITY;
                for (int k = 0; k < 3; k++) {
                    if (e[k] == 0.0) { if (t[k] < lo[k] || t[k] > hi[k]) t0 = INFINITY; continue; }
                    double a = (lo[k] - t[k]) / e[k], b = (hi[k] - t[k]) / e[k];
                    if (a > b) std::swap(a, b);
                    t0 = std::max(t0, a); t1 = std::min(t1, b);
                }
                if (t0 <= t1 && t0 > 0.0 && t0 < best) best = t0;
            }
            img[(size_t)r * W + c] = (float)best;
        }
    return img;
}

// ---- the contract on the host ------------------------------------------------------------------------------------------------------
static bool is_finite(double v) { return std::fabs(v) < (double)INFINITY; }

static void host_unproject(const pct_range_view &v, const std::vector<float> &img, double max_range, std::vector<float> &rows)
{
    for (int r = 0; r < v.height; r++)
        for (int c = 0; c < v.width; c++) {
            const double rho = (double)img[(size_t)r * v.width + c];
            if (!(is_finite(rho) && rho >= v.near_range && rho <= max_range)) continue;
            const double e0 = v.row_dir[2 * r] * v.col_dir[2 * c], e1 = v.row_dir[2 * r] * v.col_dir[2 * c + 1], e2 = v.row_dir[2 * r + 1];
            for (int k = 0; k < 3; k++) rows.push_back((float)(v.t[k] + rho * ((e0 * v.R[3 * k] + e1 * v.R[3 * k + 1]) + e2 * v.R[3 * k + 2])));
        }
}

static bool host_seen_through(const pct_range_view &v, const std::vector<float> &img, double margin, const float *p)
{
    const double d0 = (double)p[0] - v.t[0], d1 = (double)p[1] - v.t[1], d2 = (double)p[2] - v.t[2];
    const double r2 = (d0 * d0 + d1 * d1) + d2 * d2;
    const double s0 = (d0 * v.R[0] + d1 * v.R[3]) + d2 * v.R[6];
    const double s1 = (d0 * v.R[1] + d1 * v.R[4]) + d2 * v.R[7];
    const double s2 = (d0 * v.R[2] + d1 * v.R[5]) + d2 * v.R[8];
    const double h = std::sqrt(s0 * s0 + s1 * s1), a = pct_range_pseudo_angle(s0, s1), q = s2 / h;
    if (!(r2 >= v.near_range * v.near_range && r2 < (double)INFINITY && h > 0.0)) return false;
    if (!(a >= v.col_edge[0] && a < v.col_edge[v.width] && q >= v.row_edge[0] && q < v.row_edge[v.height])) return false;
    // the counts of the contract: entries <= the value, minus one
    const int c = (int)(std::upper_bound(v.col_edge, v.col_edge + v.width + 1, a) - v.col_edge) - 1;
    const int r = (int)(std::upper_bound(v.row_edge, v.row_edge + v.height + 1, q) - v.row_edge) - 1;
    const double val = (double)img[(size_t)r * v.width + c];
    if (!is_finite(val)) return false;
    const double w = val - margin;
    return w > 0.0 && r2 < w * w;
}

// the window's live rows in slot order against the host's: (slot, row) pairs; returns the number of differences
static int compare(pct::ObstacleMap &map, const std::vector<float> &rows, const std::vector<char> &gone)
{
    const int64_t cap = (int64_t)rows.size() / 3;
    std::vector<uint32_t> idx((size_t)cap);
    std::vector<float> xyz(3 * (size_t)cap);
    const double origin[3] = { 0, 0, 0 };
    int64_t n = 0;
    if (pct_radius_crop(map.handle(), origin, 1.0e6, 0, cap, idx.data(), nullptr, xyz.data(), &n) != PCT_OK) return 1 << 20;
    int bad = 0;
    int64_t j = 0;
    for (int64_t slot = 0; slot < cap; slot++) {
        if (gone[(size_t)slot]) continue;
        if (j >= n || idx[(size_t)j] != (uint32_t)slot || xyz[3 * j] != rows[3 * slot] || xyz[3 * j + 1] != rows[3 * slot + 1] || xyz[3 * j + 2] != rows[3 * slot + 2]) bad++;
        j++;
    }
    return bad + (j != n);
}

int main()
{
    Scan s;
    make_scan(s);
    const pct_range_view &v = s.view;
    const double margin = 1.0e-3;
    pct::ObstacleMap map(1 << 14);
    map.enableRollingIndex();
    int bad = 0;

    // tick 1: carve (an empty window: nothing to remove), then append
    const std::vector<float> scan1 = render(s, true), scan2 = render(s, false);
    const int64_t removed1 = map.clearSeenThroughRange(v, scan1.data(), margin);
    const int64_t kept1 = map.appendRangeImage(v, scan1.data(), INFINITY);
    std::vector<float> rows;
    host_unproject(v, scan1, INFINITY, rows);
    std::vector<char> gone(rows.size() / 3, 0);
    bad += removed1 != 0;
    bad += kept1 != (int64_t)rows.size() / 3 || map.size() != kept1;
    bad += compare(map, rows, gone);

    // tick 2: the box has left.  The host's prediction: the rows the second scan sees through are the box's returns, all of them
    int64_t box_pixels = 0, expect = 0, not_box = 0;
    {
        size_t j = 0;
        for (size_t i = 0; i < scan1.size(); i++) {
            if (!is_finite((double)scan1[i])) continue;
            const bool box = scan1[i] != scan2[i];
            const bool seen = host_seen_through(v, scan2, margin, &rows[3 * j]);
            box_pixels += box; expect += seen; not_box += seen != box;
            gone[j++] = seen;
        }
    }
    const int64_t removed2 = map.clearSeenThroughRange(v, scan2.data(), margin);
    bad += removed2 != expect || not_box != 0 || box_pixels == 0;
    bad += compare(map, rows, gone);
    const int64_t again = map.clearSeenThroughRange(v, scan2.data(), margin);         // nothing is left to see through
    bad += again != 0;
    const int64_t kept2 = map.appendRangeImage(v, scan2.data(), INFINITY);
    host_unproject(v, scan2, INFINITY, rows);
    gone.resize(rows.size() / 3, 0);
    bad += kept2 != (int64_t)(rows.size() / 3) - kept1 || map.size() != kept1 + kept2;
    bad += compare(map, rows, gone);

    std::printf("scan %d x %d: tick 1 appended %lld returns (%lld on the box); tick 2 carved %lld (the host loop: %lld, not the box's: %lld) "
                "and appended %lld; window %lld slots\n", H, W, (long long)kept1, (long long)box_pixels, (long long)removed2, (long long)expect,
                (long long)not_box, (long long)kept2, (long long)map.size());
    std::printf("%s\n", bad ? "MISMATCH" : "OK");
    return bad ? 1 : 0;
}
