// separate_fulltest_main.cpp -- the `separate_fulltest <inputfile>` evaluator of the per-label variant on top of the
// C-ABI (TNML_MODE_SINGLE, tnml_classify).
//
// Keeps the reference's surface (separate_fulltest.cc:7-170): keys `datadir`, `fname`, `imglen` (read, unused there),
// the file `sites`, the ten weight files `L<n>/W<n>`, the t10k idx files, the "normal" feature map (hard-coded in the
// reference, :104-118), and the printed tables: per image the ten overlaps o_n = <W_n|x>, prediction
// argmax_n |o_n| (first maximum), costs[n] += (n == l) ? (o_n - 1)^2 : o_n^2.  Extensions: `feature` (normal | series),
// `device`, `precision`, `Ntest`, `imglen` honoured as block-mean down-sampling, `feature_scale`; `predict` (yes | no,
// default no): a data-less context sized by the ten W alone, the test set streamed through tnml_predict_phi in chunks of
// `predict_chunk` images (0: the library's default), `predict_dtype` (f64 | f32, default f64) choosing the chain kernel's arithmetic; `input_map` (yes | no, default no): the bytes of the idx file through
// tnml_set_input_map and tnml_set_data_u8 / tnml_predict_u8 instead of host features.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "driver_util.h"
#include "init_w.h"
#include "input_group.h"

using namespace tnmlh;

int main(int argc, const char* argv[]) {
    if (argc != 2) { std::printf("Usage: %s inputfile\n", argv[0]); return 0; }       // :89-93
    try {
        InputGroup input(argv[1], "input");
        const std::string datadir = input.getString("datadir", "/Users/mstoudenmire/software/tnml/mllib/MNIST");
        (void)input.getString("fname", "W");
        const long imglen = input.getInt("imglen", 28);                                // :99
        const std::string feature = input.getString("feature", "normal");
        const int device = (int)input.getInt("device", 0);
        const std::string precision = input.getString("precision", "f64");
        const long Ntest = input.getInt("Ntest", 50000);
        const double feature_scale = input.getReal("feature_scale", 1.);
        const bool predict = input.getYesNo("predict", false);
        const long predict_chunk = input.getInt("predict_chunk", 0);
        const std::string predict_dtype = input.getString("predict_dtype", "f64");
        const bool input_map = input.getYesNo("input_map", false);
        int dtype;
        if (!parse_dtype(precision, false, &dtype)) return 1;
        bool normal;
        if (feature == "normal") normal = true; else if (feature == "series") normal = false;
        else { std::printf("feature=%s not recognized\n", feature.c_str()); return 1; }
        const int NLW = 10;
        std::printf("Labels: 0 1 2 3 4 5 6 7 8 9\n");                                   // :108

        Dataset test = read_mnist(datadir, false, Ntest);                              // :124
        Dataset raw;                                                                    // input_map = yes: the bytes of the idx file
        if (input_map) raw = test;
        const bool reducing = imglen > 0 && imglen < test.rows;
        if (reducing) reduce(test, (int)imglen);
        const int N = test.npix();
        if (!sites_match(N)) return 1;                                                  // :128-135
        std::printf("Converting test set to MPS\n");                                   // :137
        const int totNtest = test.size();
        std::printf("Total of %d testing images\n", totNtest);                         // :150

        std::vector<HostMPS> Ws(NLW);
        int wm = 1;
        for (int n = 0; n < NLW; ++n) {                                                // :156-160
            char path[64]; std::snprintf(path, sizeof path, "L%d/W%d", n, n);
            Ws[n] = read_mps(path);
            if (Ws[n].N != N) { std::printf("Mismatched sizes\n"); return 1; }
            for (int j = 1; j <= N; ++j) if (Ws[n].A[j].L != 1) { std::printf("%s carries a Label index\n", path); return 1; }
            wm = std::max(wm, max_link_dim(Ws[n]));
        }
        tnml_config cfg{};
        cfg.device = device; cfg.rank = 0; cfg.nranks = 1; cfg.N = N; cfg.NT_local = predict ? 1 : totNtest; cfg.NT_total = cfg.NT_local;
        cfg.maxm = wm; cfg.dtype = dtype; cfg.svd_backend = TNML_SVD_SYEVD; cfg.mode = TNML_MODE_SINGLE; cfg.target_label = 0;
        tnml_ctx* ctx = nullptr;
        if (tnml_create(&ctx, &cfg)) die(nullptr, "tnml_create");
        std::vector<double> phi;
        if (input_map) { DriverInputMap im = make_input_map(raw, reducing ? imglen : 0, normal, feature_scale); im.print(); im.set(ctx); }
        else phi = all_features(test, normal, feature_scale);
        if (!predict) {
            if (input_map) CK(ctx, tnml_set_data_u8(ctx, raw.pixels.data(), test.labels.data()));
            else CK(ctx, tnml_set_data_phi(ctx, phi.data(), test.labels.data()));
            std::vector<double>().swap(phi);
        }
        std::printf("Running full test\n");                                            // :165
        const bool p32 = predict_dtype_option(ctx, predict, predict_dtype);
        if (predict) std::printf("Device path: streamed chain kernel (%s%s), %d images per chunk\n", input_map ? "tnml_predict_u8" : "tnml_predict_phi", p32 ? ", fp32" : "", predict_chunk_option(ctx, predict_chunk));
        std::vector<std::vector<double>> o(NLW, std::vector<double>(totNtest));        // o[n][image] = overlap(Ws[n], testimg), :38
        for (int n = 0; n < NLW; ++n) {
            upload_mps(ctx, Ws[n]);
            if (predict && input_map) CK(ctx, tnml_predict_u8(ctx, totNtest, raw.pixels.data(), o[n].data(), nullptr));
            else if (predict) CK(ctx, tnml_predict_phi(ctx, totNtest, phi.data(), o[n].data(), nullptr));
            else CK(ctx, tnml_classify(ctx, o[n].data(), nullptr, nullptr, nullptr));
        }
        int64_t counts[10] = {0}, ninc[10] = {0};
        double costs[10] = {0};
        for (int i = 0; i < totNtest; ++i) {                                           // fullTest, :9-59 (order independent sums)
            const int l = test.labels[i];
            counts[l]++;
            int pl = 0; double best = std::fabs(o[0][i]);
            for (int n = 0; n < NLW; ++n) {
                const double on = o[n][i];
                costs[n] += (n == l) ? (on - 1) * (on - 1) : on * on;                  // :40
                if (n > 0 && std::fabs(on) > best) { best = std::fabs(on); pl = n; }   // :39,44 first maximum
            }
            if (pl != l) ++ninc[l];
        }
        print_fulltest_table(counts, ninc);                                            // :61-74
        double tC = 0.;
        std::printf("Cost functions:\n");                                              // :77
        for (int l = 0; l < 10; ++l) { tC += costs[l]; std::printf("  Digit %d C = %.20f\n", l, costs[l]); }   // :81
        std::printf("Total C = %.20f\n", tC);                                          // :83
        tnml_destroy(ctx);
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 1;
    }
    return 0;
}
