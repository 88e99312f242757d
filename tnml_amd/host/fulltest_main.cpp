// fulltest_main.cpp -- the `fulltest <inputfile>` evaluator on top of the C-ABI (include/tnml.h).
//
// Keeps the reference's surface (fulltest.cc:7-100): keys `datadir`, `fname` (default "W"), `feature`
// (series | normal), the files `sites` and <fname> in the working directory, the t10k idx files under
// `datadir`, and the result table of fullTest (util.h:186-199).  The per-image contraction toverlap
// (util.h:19-40) is one tnml_classify call on the device.  Extensions: `device`, `precision`
// (f64 | mixed | f32), `Ntest` (per-label cap; the reference takes the whole test set), `imglen` and
// `feature_scale` as in the fixedL driver (they must match the values W was trained with); `predict` (yes | no,
// default no): a data-less context sized by W alone, the test set streamed through tnml_predict_u8 / tnml_predict_phi
// in chunks of `predict_chunk` images (0: the library's default) and counted on the host, `predict_dtype` (f64 | f32, default f64)
// choosing the chain kernel's arithmetic; `input_map` (yes | no, default no): the
// images reach the device as the bytes of the idx file, the device does reduce(), the feature map and the transpose (tnml_set_input_map);
// `response` (a file name, default none): the site responses of the first `response_n` test images (default 100) for their predicted
// label, through tnml_response_u8 / tnml_response_phi in the input form the run uses, written as a NumPy .npy file of float64
// [n][N][2]; the table is not affected.
#include <algorithm>
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
    if (argc != 2) { std::printf("Usage: %s inputfile\n", argv[0]); return 0; }       // fulltest.cc:10-14
    try {
        InputGroup input(argv[1], "input");
        const std::string datadir = input.getString("datadir", "/Users/mstoudenmire/software/tnml/mllib/MNIST");
        const std::string fname = input.getString("fname", "W");
        const std::string feature = input.getString("feature", "series");
        const int device = (int)input.getInt("device", 0);
        const std::string precision = input.getString("precision", "f64");
        const long Ntest = input.getInt("Ntest", 50000);                               // mllib/mnist.h:452 default NT
        const long imglen = input.getInt("imglen", 0);
        const double feature_scale = input.getReal("feature_scale", 1.);
        const bool predict = input.getYesNo("predict", false);
        const long predict_chunk = input.getInt("predict_chunk", 0);
        const std::string predict_dtype = input.getString("predict_dtype", "f64");
        const bool input_map = input.getYesNo("input_map", false);
        const std::string response = input.getString("response", "");
        const long response_n = input.getInt("response_n", 100);
        int dtype;
        if (!parse_dtype(precision, false, &dtype)) return 1;

        std::printf("Labels: 0 1 2 3 4 5 6 7 8 9\n");                                   // :28
        Dataset raw;                                                                    // input_map = yes: the bytes of the idx file
        Dataset test = read_images(datadir, false, Ntest, imglen, input_map ? &raw : nullptr);   // :30
        const int N = test.npix();
        if (!sites_match(N)) return 1;                                                  // :34-41
        bool normal;
        if (feature == "norm" || feature == "normal") normal = true;                   // :45-56
        else if (feature == "series") normal = false;
        else { std::printf("feature type \"%s\" not recognized\n", feature.c_str()); return 1; }

        std::printf("Converting test set to MPS\n");                                   // :74
        const int totNtest = test.size();
        std::printf("Total of %d testing images\n", totNtest);                         // :85
        if (!file_exists(fname)) { std::printf("Couldn't find file '%s'\n", fname.c_str()); return 1; }   // :88-95
        HostMPS psi = read_mps(fname);
        if (psi.N != N) { std::printf("Mismatched sizes\n"); return 1; }
        int cent = 0;                                                                  // util.h:128-139
        for (int j = 1; j <= N; ++j) if (psi.A[j].L == NL) { cent = j; break; }
        if (cent == 0) { std::printf("expected Label index at some site of psi MPS\n"); return 1; }
        if (cent != N / 2) { std::printf("Label Index not on site %d\n", N / 2); return 1; }

        tnml_config cfg{};
        cfg.device = device; cfg.rank = 0; cfg.nranks = 1; cfg.N = N; cfg.NT_local = predict ? 1 : totNtest; cfg.NT_total = cfg.NT_local;
        cfg.maxm = max_link_dim(psi); cfg.dtype = dtype; cfg.svd_backend = TNML_SVD_SYEVD;
        tnml_ctx* ctx = nullptr;
        if (tnml_create(&ctx, &cfg)) die(nullptr, "tnml_create");
        const bool bytes_in = input_map || (!normal && !test.reduced() && feature_scale == 1.);   // the input map, or the built-in phi = [1, x/4], x = (byte/255)/255
        if (input_map) { DriverInputMap im = make_input_map(raw, imglen, normal, feature_scale); im.print(); im.set(ctx); }
        const uint8_t* bytes = input_map ? raw.pixels.data() : test.pixels.data();
        std::vector<double> phi;
        if (!bytes_in) phi = all_features(test, normal, feature_scale);                // fulltest.cc:57-70
        if (!predict) {
            if (bytes_in) CK(ctx, tnml_set_data_u8(ctx, bytes, test.labels.data()));
            else CK(ctx, tnml_set_data_phi(ctx, phi.data(), test.labels.data()));
        }
        upload_mps(ctx, psi);
        if (!response.empty()) {                                                       // (before predict_dtype is set: site responses are fp64 only)
            const long nr = std::max(0L, std::min<long>(response_n, totNtest));
            std::printf("Device path: site responses (%s), %d images per chunk\n", bytes_in ? "tnml_response_u8" : "tnml_response_phi", TNML_RESPONSE_CHUNK_DEFAULT);
            std::vector<double> resp((size_t)nr * N * 2);
            if (bytes_in) CK(ctx, tnml_response_u8(ctx, nr, bytes, nullptr, resp.data(), nullptr, nullptr));
            else CK(ctx, tnml_response_phi(ctx, nr, phi.data(), nullptr, resp.data(), nullptr, nullptr));
            write_npy_f64_3d(response, resp.data(), nr, N, 2);
        }
        const bool p32 = predict_dtype_option(ctx, predict, predict_dtype);

        std::printf("Running full test of %s\n", fname.c_str());                       // :97
        int64_t counts[10] = {0}, ninc[10] = {0};
        if (!predict) {
            CK(ctx, tnml_classify(ctx, nullptr, nullptr, counts, ninc));
        } else {
            const int chunk = predict_chunk_option(ctx, predict_chunk);
            std::printf("Device path: streamed chain kernel (%s%s), %d images per chunk\n", bytes_in ? "tnml_predict_u8" : "tnml_predict_phi", p32 ? ", fp32" : "", chunk);
            std::vector<int32_t> pred(totNtest);
            if (bytes_in) CK(ctx, tnml_predict_u8(ctx, totNtest, bytes, nullptr, pred.data()));
            else CK(ctx, tnml_predict_phi(ctx, totNtest, phi.data(), nullptr, pred.data()));
            for (int i = 0; i < totNtest; ++i) { const int l = test.labels[i]; counts[l]++; if (pred[i] != l) ++ninc[l]; }
        }
        print_fulltest_table(counts, ninc);                                            // util.h:186-199
        tnml_destroy(ctx);
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 1;
    }
    return 0;
}
