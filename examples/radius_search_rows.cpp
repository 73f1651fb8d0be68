// radius_search_rows.cpp -- the cone keeper's call pattern (Planner/src/cone_keeper.cpp:92-153) as ONE batch:
//   the previous depth image becomes a cloud with one point (column, row, depth / 1000) per valid pixel, every newly seen marked
//   pixel (x0, y0) asks for the points within 27 of (x0, y0, 0), and the caller walks each returned index list for the nearest
//   depth around the pixel.  The reference asks once per marked point; here the marked points of a frame are one
//   ObstacleMap::radiusSearchBatch call and the walk runs over the rows of its CSR result.
// Self-checking: every row is compared with a host loop over the image.  Build: pointcloudtraj_amd/build.py.
#include <cmath>
#include <cstdio>
#include <vector>

#include "pct_obstacle_map.hpp"

static uint64_t sm64(uint64_t &s) { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static float u01(uint64_t &s) { return (float)(sm64(s) >> 40) * 0x1p-24f; }

int main(int argc, char **argv)
{
    const int width = 640, height = 480, marked = argc > 1 ? std::atoi(argv[1]) : 2000;
    const float depth_coef = 1000.f, radius = 27.f;
    uint64_t seed = 11;
    // a synthetic depth image in millimetres; one pixel in sixteen has no return
    std::vector<float> pixels;                                   // x, y, z per valid pixel, column-major as the reference fills it
    for (int i = 0; i < width; i++)
        for (int j = 0; j < height; j++) {
            const float depth = 500.f + 9500.f * u01(seed);
            if ((sm64(seed) & 15u) == 0) continue;
            pixels.push_back((float)i); pixels.push_back((float)j); pixels.push_back(depth / depth_coef);
        }
    const int64_t n = (int64_t)pixels.size() / 3;
    pct::ObstacleMap image(n);
    image.setInput(pixels.data(), n, 12);                        // builds the cell index: the batch below takes the cell-pruned path

    std::vector<float> queries((size_t)3 * marked), radii((size_t)marked, radius);
    for (int k = 0; k < marked; k++) {
        queries[3 * k] = std::floor(width * u01(seed));
        queries[3 * k + 1] = std::floor(height * u01(seed));
        queries[3 * k + 2] = 0.f;
    }
    std::vector<int64_t> offsets;
    std::vector<uint32_t> index;
    std::vector<double> d2;
    image.radiusSearchBatch(queries.data(), radii.data(), marked, offsets, index, d2, /*sorted=*/false);

    int bad = 0;
    double mean_row = 0.0;
    for (int k = 0; k < marked; k++) {
        // the reference's walk: the nearest depth among the returned pixels (its four quadrant minima reduce to this when all are set)
        double nearest = INFINITY;
        for (int64_t e = offsets[k]; e < offsets[k + 1]; e++) nearest = std::fmin(nearest, (double)pixels[3 * (size_t)index[e] + 2] * depth_coef);
        mean_row += (double)(offsets[k + 1] - offsets[k]) / marked;
        // host check: the same ball over every pixel, in the engine's arithmetic
        double want = INFINITY;
        int64_t hits = 0;
        for (int64_t p = 0; p < n; p++) {
            const double dx = (double)pixels[3 * p] - (double)queries[3 * k], dy = (double)pixels[3 * p + 1] - (double)queries[3 * k + 1],
                         dz = (double)pixels[3 * p + 2] - (double)queries[3 * k + 2];
            if ((dx * dx + dy * dy) + dz * dz <= (double)radius * (double)radius) { hits++; want = std::fmin(want, (double)pixels[3 * p + 2] * depth_coef); }
        }
        if (hits != offsets[k + 1] - offsets[k] || want != nearest) bad++;
    }
    std::printf("%lld pixel points, %d marked points, r = %.0f: %.1f pixels per row, %lld entries, %d rows differ from the host loop\n", (long long)n, marked,
                (double)radius, mean_row, (long long)offsets[(size_t)marked], bad);
    return bad ? 1 : 0;
}
