// trajectory_generate.cpp -- corridor in, flyable trajectory out: pct::generateTrajectories and ObstacleMap::generateSafeTrajectory
// (pct_trajgen.h, paragraph "Trajectory generation") on a wall with a door and a hand-written corridor of four spheres through it,
// solved under five time scales at once.  Self-checking: what PCT_GEN_OK guarantees is recomputed by a host loop from the returned
// rows alone -- the end states, the C2 joints, every control point inside its sphere, the reported slack and control values -- and the
// map's choice is compared with the shortest candidate that is both OK and certified free.  Prints OK.
// Build: pointcloudtraj_amd/build.py (plain g++ with -ffp-contract=off).
#include <cmath>
#include <cstdio>
#include <vector>

#include "pct_obstacle_map.hpp"

int main()
{
    // the wall x = 0 on a 0.1 m lattice, open where |y| < 1.2
    std::vector<float> pts;
    for (int iy = -40; iy <= 40; iy++)
        for (int iz = 0; iz <= 30; iz++)
            if (std::abs(iy) >= 12) { pts.push_back(0.0f); pts.push_back((float)(iy / 10.0)); pts.push_back((float)(iz / 10.0)); }
    const int m = 4, K = 5;
    const double path[m * 3] = { -2.0, 0, 1.5, -0.7, 0, 1.5, 0.7, 0, 1.5, 2.0, 0, 1.5 };
    const double radius[m] = { 1.2, 1.0, 1.0, 1.2 };
    const int32_t orders[m] = { 7, 7, 7, 7 };
    const double start[9] = { -2.5, 0.2, 1.4, 0.3, 0, 0, 0, 0, 0 }, end[9] = { 2.4, -0.2, 1.6, 0, 0, 0, 0, 0, 0 };
    const double scales[K] = { 0.6, 0.8, 1.0, 1.5, 2.0 };
    const double margin = 0.05, search_margin = 0.2;
    double times[m];
    if (pct_time_allocation(path, radius, m, start, end, start + 3, 1.5, 1.0, times) != PCT_OK) { std::printf("time allocation failed\n"); return 1; }

    pct_trajgen_params prm{ 3, 4000, 25, 2.0, 0.0, margin, 1e-5, 0.0 };
    pct::GeneratedTrajectories gen;
    const int64_t n_ok = pct::generateTrajectories(path, radius, times, orders, m, scales, K, start, end, prm, gen);

    int bad = 0;
    double worst_state = 0.0, worst_joint = 0.0;
    for (int k = 0; k < K; k++) {
        const pct_trajgen_result &r = gen.results[(size_t)k];
        if (r.status != PCT_GEN_OK) continue;
        double slack = INFINITY, vmax = 0.0, amax = 0.0, dur = 0.0;
        for (int s = 0; s < m; s++) {
            const size_t g = (size_t)k * m + (size_t)s;
            const int n = orders[s], cnt = n + 1;
            const double T = gen.seg_time[g], *row = gen.polycoef.data() + g * (size_t)gen.row_stride;
            dur += T;
            auto P = [&](int j, int d) { return row[d * cnt + j] * T; };
            for (int j = 0; j < cnt; j++) {
                const double dx = P(j, 0) - path[3 * s], dy = P(j, 1) - path[3 * s + 1], dz = P(j, 2) - path[3 * s + 2];
                slack = std::fmin(slack, (radius[s] - margin) - std::sqrt((dx * dx + dy * dy) + dz * dz));
                for (int d = 0; d < 3; d++) {
                    if (j < n) vmax = std::fmax(vmax, std::fabs(P(j + 1, d) - P(j, d)) * ((double)n / T));
                    if (j < n - 1) amax = std::fmax(amax, std::fabs((P(j + 2, d) - 2.0 * P(j + 1, d)) + P(j, d)) * ((double)(n * (n - 1)) / (T * T)));
                }
            }
            for (int d = 0; d < 3; d++) {
                // p, v, a at both ends of the segment from its control points
                const double p0 = P(0, d), v0 = n * (P(1, d) - P(0, d)) / T, a0 = n * (n - 1) * (P(2, d) - 2 * P(1, d) + P(0, d)) / (T * T);
                const double p1 = P(n, d), v1 = n * (P(n, d) - P(n - 1, d)) / T, a1 = n * (n - 1) * (P(n, d) - 2 * P(n - 1, d) + P(n - 2, d)) / (T * T);
                if (s == 0) worst_state = std::fmax(worst_state, std::fmax(std::fabs(p0 - start[d]), std::fmax(std::fabs(v0 - start[3 + d]), std::fabs(a0 - start[6 + d]))));
                if (s == m - 1) worst_state = std::fmax(worst_state, std::fmax(std::fabs(p1 - end[d]), std::fmax(std::fabs(v1 - end[3 + d]), std::fabs(a1 - end[6 + d]))));
                if (s + 1 < m) {
                    const double T2 = gen.seg_time[g + 1], *row2 = row + gen.row_stride;
                    const int n2 = orders[s + 1], cnt2 = n2 + 1;
                    auto Q = [&](int j) { return row2[d * cnt2 + j] * T2; };
                    const double q0 = Q(0), w0 = n2 * (Q(1) - Q(0)) / T2, b0 = n2 * (n2 - 1) * (Q(2) - 2 * Q(1) + Q(0)) / (T2 * T2);
                    worst_joint = std::fmax(worst_joint, std::fmax(std::fabs(p1 - q0), std::fmax(std::fabs(v1 - w0), std::fabs(a1 - b0))));
                }
            }
        }
        if (!(slack >= 0.0) || std::fabs(slack - r.sphere_slack) > 1e-12 || std::fabs(vmax - r.max_vel_ctrl) > 1e-9 || std::fabs(amax - r.max_acc_ctrl) > 1e-9 ||
            std::fabs(dur - r.duration) > 1e-12 || !(r.r_prim <= prm.eps) || !(r.r_dual <= prm.eps))
            bad++;
    }
    if (worst_state > 1e-9 || worst_joint > 1e-9 || n_ok < 1) bad++;

    // the same corridor through the map: generate, certify, choose
    pct::ObstacleMap map((int64_t)pts.size() / 3);
    map.setParam(0.0, search_margin, 1.5, 30.0);
    map.setInput(pts.data(), (int64_t)pts.size() / 3, 12, true);
    pct::GeneratedTrajectories flown;
    std::vector<pct_traj_certificate> cert;
    const int64_t chosen = map.generateSafeTrajectory(path, radius, times, orders, m, scales, K, start, end, prm, margin, flown, cert);
    int64_t want = -1, n_free = 0;
    for (int k = 0; k < K; k++) {
        if (flown.results[(size_t)k].status != gen.results[(size_t)k].status || flown.polycoef != gen.polycoef) bad++;
        if (flown.results[(size_t)k].status != PCT_GEN_OK || cert[(size_t)k].status != PCT_CERT_FREE) continue;
        n_free++;
        if (want < 0 || flown.results[(size_t)k].duration < flown.results[(size_t)want].duration) want = k;
    }
    if (chosen != want || chosen < 0) bad++;
    std::printf("%d candidates: %lld OK, %lld OK and certified free, chosen %lld (duration %.3f s, %d iterations); end states within %.1e, joints within %.1e; "
                "%d checks failed\n", K, (long long)n_ok, (long long)n_free, (long long)chosen, chosen >= 0 ? flown.results[(size_t)chosen].duration : 0.0,
                chosen >= 0 ? flown.results[(size_t)chosen].iterations : 0, worst_state, worst_joint, bad);
    if (!bad) std::printf("OK\n");
    return bad ? 1 : 0;
}
