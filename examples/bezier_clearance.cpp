// bezier_clearance.cpp -- "how close does this whole trajectory come to the map": ObstacleMap::trajectoryClearances and
// trajectoryClearance (pct_engine.h, paragraph "Trajectory clearance") on the 4 mm line of README's certify example, on a rolling map
// and on an empty one.  Self-checking: every bracket is held against a dense host sampling of the curve (de Casteljau at 2049 points
// per segment against every row), which the bracket must contain up to the sampling's own spacing.
// Build: pointcloudtraj_amd/build.py (plain g++ with -ffp-contract=off).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pct_obstacle_map.hpp"

static uint64_t sm64(uint64_t &s) { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static double u01(uint64_t &s) { return (double)(sm64(s) >> 11) * 0x1p-53; }

// the smallest distance from 2049 points of every segment of candidate t to any row, and the longest step between two of the points
static double dense_clearance(const std::vector<float> &pts, const pct_bezier_batch &bt, int t, double *step)
{
    double best = INFINITY;
    *step = 0.0;
    for (int i = bt.seg_offsets[t]; i < bt.seg_offsets[t + 1]; i++) {
        const int n = bt.orders[i], m = n + 1;
        double prev[3] = { 0, 0, 0 };
        for (int g = 0; g <= 2048; g++) {
            const double u = g / 2048.0;
            double p[13][3];
            for (int j = 0; j < m; j++)
                for (int k = 0; k < 3; k++) p[j][k] = bt.polycoef[(size_t)i * bt.row_stride + k * m + j] * bt.seg_time[i];
            for (int lev = 1; lev < m; lev++)
                for (int j = 0; j + lev < m; j++)
                    for (int k = 0; k < 3; k++) p[j][k] = p[j][k] * (1.0 - u) + p[j + 1][k] * u;
            if (g > 0) *step = std::fmax(*step, std::sqrt((p[0][0] - prev[0]) * (p[0][0] - prev[0]) + (p[0][1] - prev[1]) * (p[0][1] - prev[1]) + (p[0][2] - prev[2]) * (p[0][2] - prev[2])));
            std::memcpy(prev, p[0], sizeof prev);
            for (size_t r = 0; r < pts.size() / 3; r++) {
                const double dx = pts[3 * r] - p[0][0], dy = pts[3 * r + 1] - p[0][1], dz = pts[3 * r + 2] - p[0][2];
                best = std::fmin(best, std::sqrt(dx * dx + dy * dy + dz * dz));
            }
        }
    }
    return best;
}

int main()
{
    int bad = 0;
    // ---- 1. the 4 mm line: 1 m along x, one obstacle 4 mm off the axis at x = 0.51 -- free for the sampled check at dt = 0.02
    {
        const float row[3] = { 0.51f, 0.004f, 0.0f };
        const double coef[6] = { 0.0, 1.0, 0.0, 0.0, 0.0, 0.0 }, T = 1.0;
        const int32_t order = 1;
        pct::ObstacleMap map(16);
        map.setParam(0.0, 0.005, 1.5, 30.0);
        map.setInput(row, 1, 12, false);
        const double tol = 0.001;
        const pct_traj_clearance r = map.trajectoryClearance(coef, 6, &T, &order, 1, tol);
        const double off = (double)row[1];
        if (r.status != PCT_CLR_DONE || !(r.lo <= off && off <= r.hi && r.hi - r.lo <= tol) || r.at_seg != 0 || r.at_idx != 0) bad++;
        std::printf("4 mm line: status %d depth %d pieces %lld at_u %.17g lo %.17g hi %a (%.9f m)\n", r.status, r.depth, (long long)r.pieces, r.at_u, r.lo, r.hi, r.hi);
        // a cap below the clearance of a far line: one piece, retired at once
        const float far_row[3] = { 0.5f, 2.0f, 0.0f };
        map.setInput(far_row, 1, 12, false);
        const pct_traj_clearance f = map.trajectoryClearance(coef, 6, &T, &order, 1, 0.01, 0.5);
        if (f.status != PCT_CLR_DONE || f.depth != 0 || f.pieces != 1 || !(f.lo >= 0.5 - 0.01) || f.hi != std::sqrt(4.25)) bad++;
    }
    // ---- 2. a rolling map: 400 points in frames of 100, 24 candidates of three segments, orders 0..12 in turn
    const int npts = 400, ntraj = 24;
    uint64_t seed = 43;
    std::vector<float> pts;
    for (int i = 0; i < 3 * npts; i++) pts.push_back((float)(10.0 * u01(seed)));
    const int64_t stride = 39;
    std::vector<double> coef, times;
    std::vector<int32_t> orders, offs{ 0 };
    for (int t = 0; t < ntraj; t++) {
        double w[4][3];
        for (int k = 0; k < 3; k++) w[0][k] = 1.0 + 8.0 * u01(seed);
        for (int s = 1; s < 4; s++)
            for (int k = 0; k < 3; k++) w[s][k] = w[s - 1][k] + 2.4 * (u01(seed) - 0.5);
        for (int s = 0; s < 3; s++) {
            const int n = (3 * t + s) % 13, m = n + 1;
            const double T = 0.5 + 0.25 * ((t + s) % 3);
            std::vector<double> row((size_t)stride, 0.0);
            for (int k = 0; k < 3; k++)
                for (int j = 0; j < m; j++) {
                    double v = m > 1 ? w[s][k] + (w[s + 1][k] - w[s][k]) * j / (double)(m - 1) : w[s][k];
                    if (j > 0 && j < m - 1) v += 0.3 * (u01(seed) - 0.5);
                    row[(size_t)(k * m + j)] = v / T;
                }
            coef.insert(coef.end(), row.begin(), row.end());
            times.push_back(T);
            orders.push_back(n);
        }
        offs.push_back((int32_t)times.size());
    }
    times[4] = 0.0;                                              // candidate 1 is INVALID: a segment time that is not > 0
    const pct_bezier_batch bt{ coef.data(), stride, times.data(), orders.data(), offs.data(), nullptr, ntraj };
    int done = 0, open = 0, invalid = 0;
    double widest = 0.0;
    {
        pct::ObstacleMap map(npts);
        map.setParam(0.0, 0.25, 1.5, 30.0);
        map.enableRollingIndex();
        for (int f = 0; f < 4; f++) map.appendInput(pts.data() + 300 * f, 100, 12);
        const double tol = 0.01;
        std::vector<pct_traj_clearance> rec;
        int64_t stats[3] = { -1, -1, -1 };
        const int64_t not_done = map.trajectoryClearances(bt, rec, tol, INFINITY, 16, 0, stats);
        int64_t pieces = 0;
        for (int t = 0; t < ntraj; t++) {
            const pct_traj_clearance &r = rec[(size_t)t];
            pieces += r.pieces;
            if (r.status == PCT_CLR_INVALID) {
                invalid++;
                if (t != 1 || !std::isnan(r.lo) || !std::isnan(r.hi) || r.pieces != 0 || r.at_seg != -1) bad++;
                continue;
            }
            (r.status == PCT_CLR_DONE ? done : open)++;
            double step;
            const double dense = dense_clearance(pts, bt, t, &step);
            // lo bounds every point of the curve; the curve comes no nearer than a sample minus half the sampling step; hi is a point of it
            if (!(r.lo <= dense) || !(r.hi >= dense - step) || !(r.lo <= r.hi)) bad++;
            if (r.status == PCT_CLR_DONE && !(r.hi - r.lo <= tol)) bad++;
            if (r.at_seg < offs[(size_t)t] || r.at_seg >= offs[(size_t)t + 1] || r.at_idx >= (uint32_t)npts) bad++;
            widest = std::fmax(widest, r.hi - r.lo);
        }
        if (not_done != open + invalid || invalid != 1 || stats[1] != pieces || stats[2] != 0 || stats[0] < 2) bad++;
        // one trajectory alone: the same record as its entry of the batch, up to the segment numbering
        for (int t : { 0, 7 }) {
            const int32_t s0 = offs[(size_t)t];
            const pct_traj_clearance one = map.trajectoryClearance(&coef[(size_t)s0 * stride], stride, &times[(size_t)s0], &orders[(size_t)s0], 3, tol);
            pct_traj_clearance ref = rec[(size_t)t];
            ref.at_seg -= s0;
            if (std::memcmp(&one, &ref, sizeof one) != 0) bad++;
        }
        std::printf("rolling map: %d points, %d candidates: %d DONE, %d OPEN, %d INVALID; %lld rounds, %lld pieces; widest bracket %.6f m\n", npts, ntraj, done,
                    open, invalid, (long long)stats[0], (long long)stats[1], widest);
    }
    // ---- 3. an empty map: nothing to be near to
    {
        pct::ObstacleMap map(16);
        map.setParam(0.0, 0.25, 1.5, 30.0);
        std::vector<pct_traj_clearance> rec;
        int64_t stats[3] = { -1, -1, -1 };
        map.trajectoryClearances(bt, rec, 0.01, INFINITY, 16, 0, stats);
        int inf = 0;
        for (int t = 0; t < ntraj; t++) {
            const pct_traj_clearance &r = rec[(size_t)t];
            if (t == 1) { if (r.status != PCT_CLR_INVALID) bad++; continue; }
            if (r.status != PCT_CLR_DONE || r.depth != 0 || r.pieces != 3 || r.lo != INFINITY || r.hi != INFINITY || r.at_seg != -1 || r.at_idx != PCT_NO_INDEX ||
                !std::isnan(r.at_u))
                bad++;
            else
                inf++;
        }
        if (stats[0] != 1 || stats[1] != 3 * (ntraj - 1) || stats[2] != 0) bad++;
        std::printf("empty map: %d candidates at +inf\n", inf);
    }
    std::printf("3 maps (4 mm line, rolling, empty): %d checks failed\n", bad);
    return bad ? 1 : 0;
}
