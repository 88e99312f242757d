// input_map_check.cpp -- stand-alone host check of the input map's table against the fp64 feature path, meant to be built with
// -fsanitize=address,undefined (make -C tnml_amd/host input-map-check): for every geometry below, random byte images (one all 0, one all
// 255) go through reduce() + features_series / features_normal on one side and through integer block sums + feature_table on the other;
// the doubles must be the same bits.  No GPU, no libtnml.so.
#include <cstdio>
#include <cstring>
#include <random>

#include "driver_util.h"

using namespace tnmlh;

static int check(int rows, int cols, long imglen, bool normal, double scale) {
    const int n = 7;
    Dataset raw; raw.rows = rows; raw.cols = cols;
    std::mt19937 rng(rows * 1000 + cols * 10 + (int)imglen);
    raw.pixels.resize((size_t)n * rows * cols);
    for (auto& b : raw.pixels) b = (uint8_t)(rng() & 0xff);
    std::fill(raw.pixels.begin(), raw.pixels.begin() + rows * cols, 0);
    std::fill(raw.pixels.begin() + rows * cols, raw.pixels.begin() + 2 * rows * cols, 255);
    raw.labels.assign(n, 0);
    const DriverInputMap im = make_input_map(raw, imglen, normal, scale);
    const tnml_input_map& g = im.geo;
    Dataset red = raw;
    if (imglen > 0) reduce(red, (int)imglen);
    if (red.npix() != g.out_rows * g.out_cols) { std::printf("%d x %d imglen %ld: %d sites against %d\n", rows, cols, imglen, red.npix(), g.out_rows * g.out_cols); return 1; }
    std::vector<double> phi;
    int maxcode = 0;
    for (int i = 0; i < n; ++i) {
        if (normal) features_normal(red, i, phi); else features_series(red, i, phi, scale);
        for (int oy = 0; oy < g.out_rows; ++oy) for (int ox = 0; ox < g.out_cols; ++ox) {
            int code = 0;
            for (int r = 0; r < g.block; ++r) for (int c = 0; c < g.block; ++c)
                code += raw.pixels[((size_t)i * rows + g.row0 + g.block * oy + r) * cols + g.col0 + g.block * ox + c];
            if (code >= g.ncodes) { std::printf("code %d outside the table of %d rows\n", code, g.ncodes); return 1; }
            maxcode = std::max(maxcode, code);
            const int j = oy * g.out_cols + ox;
            if (std::memcmp(&phi[2 * j], &im.table[2 * (size_t)code], 2 * sizeof(double)) != 0) {
                std::printf("%d x %d imglen %ld %s: image %d site %d code %d: features (%.17g, %.17g), table (%.17g, %.17g)\n", rows, cols, imglen,
                            normal ? "normal" : "series", i, j, code, phi[2 * j], phi[2 * j + 1], im.table[2 * (size_t)code], im.table[2 * (size_t)code + 1]);
                return 1;
            }
        }
    }
    if (maxcode != g.ncodes - 1) { std::printf("the all-255 image did not reach the last table row\n"); return 1; }
    std::printf("%2d x %2d imglen %2ld %-6s scale %-3g: block %d from (%d, %d), %d sites, %d codes, bit-identical\n", rows, cols, imglen, normal ? "normal" : "series",
                scale, g.block, g.row0, g.col0, g.out_rows * g.out_cols, g.ncodes);
    return 0;
}

int main() {
    const struct { int rows, cols; long imglen; } geo[] = {{12, 12, 6}, {13, 13, 4}, {5, 7, 0}, {28, 28, 14}, {28, 28, 10}, {16, 16, 2}, {8, 8, 8}, {8, 8, 4}};
    int bad = 0;
    for (const auto& g : geo) for (int normal = 0; normal < 2; ++normal) for (double scale : {1., 255.}) bad += check(g.rows, g.cols, g.imglen, normal != 0, scale);
    for (long refused : {0L + 29, 0L - 0}) {                  // reduce()'s refusals in its own words
        Dataset raw; raw.rows = raw.cols = 28; raw.pixels.resize(784); raw.labels.assign(1, 0);
        if (refused == 0) { raw.cols = 27; refused = 9; }
        try { make_input_map(raw, refused, false, 1.); std::printf("imglen %ld on %d x %d was not refused\n", refused, raw.rows, raw.cols); ++bad; }
        catch (const std::exception& e) { std::printf("refused as expected: %s\n", e.what()); }
    }
    std::printf(bad ? "FAILED\n" : "input map host check passed\n");
    return bad ? 1 : 0;
}
