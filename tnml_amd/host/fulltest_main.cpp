// fulltest_main.cpp -- the `fulltest <inputfile>` evaluator on top of the C-ABI (include/tnml.h).
//
// Keeps the reference's surface (fulltest.cc:7-100): keys `datadir`, `fname` (default "W"), `feature`
// (series | normal), the files `sites` and <fname> in the working directory, the t10k idx files under
// `datadir`, and the result table of fullTest (util.h:186-199).  The per-image contraction toverlap
// (util.h:19-40) is one tnml_classify call on the device.  Extensions: `device`, `precision`
// (f64 | mixed | f32), `Ntest` (per-label cap; the reference takes the whole test set), `imglen` and
// `feature_scale` as in the fixedL driver (they must match the values W was trained with).
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
        int dtype;
        if (!parse_dtype(precision, false, &dtype)) return 1;

        std::printf("Labels: 0 1 2 3 4 5 6 7 8 9\n");                                   // :28
        Dataset test = read_images(datadir, false, Ntest, imglen);                      // :30
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
        cfg.device = device; cfg.rank = 0; cfg.nranks = 1; cfg.N = N; cfg.NT_local = totNtest; cfg.NT_total = totNtest;
        cfg.maxm = max_link_dim(psi); cfg.dtype = dtype; cfg.svd_backend = TNML_SVD_SYEVD;
        tnml_ctx* ctx = nullptr;
        if (tnml_create(&ctx, &cfg)) die(nullptr, "tnml_create");
        if (!normal && !test.reduced() && feature_scale == 1.) {
            CK(ctx, tnml_set_data_u8(ctx, test.pixels.data(), test.labels.data()));    // phi = [1, x/4], x = (byte/255)/255
        } else {
            std::vector<double> phi = all_features(test, normal, feature_scale);       // fulltest.cc:57-70
            CK(ctx, tnml_set_data_phi(ctx, phi.data(), test.labels.data()));
        }
        upload_mps(ctx, psi);

        std::printf("Running full test of %s\n", fname.c_str());                       // :97
        int64_t counts[10], ninc[10];
        CK(ctx, tnml_classify(ctx, nullptr, nullptr, counts, ninc));
        print_fulltest_table(counts, ninc);                                            // util.h:186-199
        tnml_destroy(ctx);
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 1;
    }
    return 0;
}
