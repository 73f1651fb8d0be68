// Stand-alone run of the polyhedral trajectory generator's kernel text (csrc/trajgen.hpp over csrc/trajgen_poly.hpp) on the CPU
// (tests/test_trajgen_poly_host.py builds it with -fsanitize=address,undefined and runs it): 256 threads stand for the lanes of one
// workgroup, the candidates run one after another, LDS is a global array of sizeof(PolyLds).  No HIP, not loaded into Python.
//   trajgen_poly_check IN OUT
//   IN:  B total_seg total_planes row_stride / minimize_order max_iter check_every max_vel max_acc margin eps rho / seg_offsets /
//        orders / plane_offsets / seg_time / anchors / planes / start_state / end_state
//   OUT: per candidate "status iterations cost duration r_prim r_dual sphere_slack max_vel_ctrl max_acc_ctrl", then every row
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../pointcloudtraj_amd/csrc/trajgen_poly.hpp"

namespace pct_trajgen {
alignas(16) unsigned char smem[sizeof(PolyLds)];
}

namespace {

template <typename T>
bool read_all(FILE *f, std::vector<T> &v, const char *fmt)
{
    for (auto &e : v)
        if (std::fscanf(f, fmt, &e) != 1) return false;
    return true;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    long long B = 0, total = 0, nplanes = 0, stride = 0;
    pct_trajgen_params prm;
    if (std::fscanf(f, "%lld %lld %lld %lld", &B, &total, &nplanes, &stride) != 4) return 2;
    if (std::fscanf(f, "%d %d %d %lf %lf %lf %lf %lf", &prm.minimize_order, &prm.max_iter, &prm.check_every, &prm.max_vel, &prm.max_acc, &prm.margin,
                    &prm.eps, &prm.rho) != 8)
        return 2;
    std::vector<int32_t> offs((size_t)B + 1), orders((size_t)total), po((size_t)total + 1);
    std::vector<double> T((size_t)total), anchors(3 * (size_t)total), planes(4 * (size_t)nplanes), start(9 * (size_t)B), end(9 * (size_t)B);
    if (!read_all(f, offs, "%d") || !read_all(f, orders, "%d") || !read_all(f, po, "%d") || !read_all(f, T, "%lf") || !read_all(f, anchors, "%lf") ||
        !read_all(f, planes, "%lf") || !read_all(f, start, "%lf") || !read_all(f, end, "%lf"))
        return 2;
    std::fclose(f);
    // exactly sized heap blocks: an overrun of a plane, a row or a record is the sanitizer's to report
    std::vector<double> rows((size_t)total * (size_t)stride, -7.0);
    std::vector<pct_trajgen_result> res((size_t)B);
    pct_trajgen_poly_batch in = {anchors.data(), planes.data(), po.data(), T.data(), orders.data(), offs.data(), start.data(), end.data(), B};
    std::barrier<> bar(pct_trajgen::kThreads);
    hip_stub::g_barrier = &bar;
    for (long long b = 0; b < B; b++) {
        std::vector<std::thread> lanes;
        for (int t = 0; t < pct_trajgen::kThreads; t++)
            lanes.emplace_back([&, t] {
                threadIdx.x = (unsigned)t;
                blockIdx.x = (unsigned)b;
                pct_trajgen::trajgen_poly_kernel(in, prm, rows.data(), stride, res.data());
            });
        for (auto &l : lanes) l.join();
    }
    FILE *o = std::fopen(argv[2], "w");
    if (!o) return 2;
    for (long long b = 0; b < B; b++) {
        const pct_trajgen_result &r = res[(size_t)b];
        std::fprintf(o, "%d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", r.status, r.iterations, r.cost, r.duration, r.r_prim, r.r_dual, r.sphere_slack,
                     r.max_vel_ctrl, r.max_acc_ctrl);
    }
    for (size_t i = 0; i < rows.size(); i++) std::fprintf(o, "%.17g%c", rows[i], (i + 1) % (size_t)stride ? ' ' : '\n');
    std::fclose(o);
    return 0;
}
