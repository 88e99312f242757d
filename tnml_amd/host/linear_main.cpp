// linear_main.cpp -- the `linear <inputfile>` command line driver on top of the C-ABI (include/tnml.h, tnml_lin_*).
//
// Keeps the reference's surface (linear.cc:92-240): the keys `datadir`, `Nlinear_iter` (5000), `Ntrain` (60000, the per-label cap of
// read_mnist as in fixedL), `lambda` (0), `label` (mandatory unless `labels` is given), `dotest` (read, never used -- as in the
// reference, :107-108); the files V%d (parameters, read if present), `sites` and W%d (the bond-dimension-2 MPS embedding that fixedL's
// W0..W9 branch reads, fixedL.cc:682-701); the train and t10k idx files under `datadir`; the log lines.  cgrad (:27-90) runs on the GPU
// for all requested labels at once (kernels_linear.hip).
// Extensions (never read by the reference, all optional):
//   labels        = all | L1,L2,...  one process, K label columns sharing the data; files V%d / W%d per label, per-pass lines prefixed "L%d"
//   seed          (1) random start V of label L: uniform [0,1) from mt19937_64(seed + L), normalised (:159-162) -- the same for a label
//                 whether it runs alone or with others
//   device        (0) HIP ordinal
//   cg_block      (64) passes per device round trip: costs are printed in order after each block and the STOP file (:80-85) is looked
//                 for between blocks, so STOP takes effect at a block boundary (cg_block = 1 is the reference's per-pass check)
//   feature_scale absent: the site entries of W%d are the reference's V(j), which evaluate to V.v under fixedL at feature_scale = 255;
//                 present: entries V(j) 255 / feature_scale, so that W%d is the trained model under fixedL's feature map at that scale
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "driver_util.h"
#include "input_group.h"
#include "linear_mps.h"

using namespace tnmlh;

static std::vector<int> parse_labels(const std::string& s) {
    std::vector<int> out;
    if (s == "all") { for (int l = 0; l < 10; ++l) out.push_back(l); return out; }
    std::string t = s;
    for (char& ch : t) if (ch == ',' || ch == ';') ch = ' ';
    std::istringstream is(t);
    for (std::string w; is >> w;) {
        char* end = nullptr;
        const long v = std::strtol(w.c_str(), &end, 10);
        if (*end || v < 0 || v > 9) throw std::runtime_error("labels: expected `all` or a comma-separated list of labels 0..9, got '" + s + "'");
        for (int x : out) if (x == v) throw std::runtime_error("labels: label " + w + " given twice");
        out.push_back((int)v);
    }
    if (out.empty()) throw std::runtime_error("labels: empty list");
    return out;
}

int main(int argc, const char* argv[]) {
    if (argc != 2) { std::printf("Usage: %s inputfile\n", argv[0]); return 0; }        // linear.cc:95
    try {
        InputGroup in(argv[1], "input");                                                 // :97
        const std::string datadir = in.getString("datadir", "/Users/mstoudenmire/software/tnml/mllib/MNIST");
        const long Niter = in.getInt("Nlinear_iter", 5000);
        const long Ntrain = in.getInt("Ntrain", 60000);
        const double lambda = in.getReal("lambda", 0.);
        std::vector<int> labs;
        if (in.has("labels")) labs = parse_labels(in.getString("labels", "all"));        // extension
        else if (in.has("label")) {                                                      // :104 in.getInt("label"), mandatory
            const long L = in.getInt("label", -1);
            if (L < 0 || L > 9) { std::fprintf(stderr, "Error: label = %ld, expected 0..9\n", L); return 1; }
            labs.push_back((int)L);
        } else {
            std::fprintf(stderr, "Error: input key `label` not found (mandatory unless `labels` is given)\n");
            return 1;
        }
        const int d = 2;
        (void)in.getYesNo("dotest", false);                                              // :107-108, never used
        const uint64_t seed = (uint64_t)in.getInt("seed", 1);
        const int device = (int)in.getInt("device", 0);
        const long cg_block = in.getInt("cg_block", 64);
        const bool has_fs = in.has("feature_scale");
        const double feature_scale = in.getReal("feature_scale", 255.);
        if (cg_block < 1) { std::fprintf(stderr, "Error: cg_block must be >= 1\n"); return 1; }
        if (!(feature_scale > 0.)) { std::fprintf(stderr, "Error: feature_scale must be > 0\n"); return 1; }
        const int K = (int)labs.size();

        std::printf("Loading training data...");                                         // :111-114
        std::fflush(stdout);
        Dataset train = read_mnist(datadir, true, Ntrain);
        Dataset test = read_mnist(datadir, false, 1L << 40);
        std::printf("done\n");
        const int N = train.npix();                                                      // :116
        if (test.npix() != N) throw std::runtime_error("test images have a different size than the training images");
        const int size = 1 + N;
        std::printf("Vector size = %d\n", size);                                         // :124
        // an existing `sites` file must describe these images (:194-203): checked before any work, so a mismatch costs no training
        const bool have_sites = file_exists("sites");
        if (have_sites) {
            int Ns, ds; read_sites("sites", &Ns, &ds);
            if (Ns != N || ds != d) {
                std::fprintf(stderr, "Error: sites file has %d sites of dimension %d, the data has %d of dimension %d\n", Ns, ds, N, d);
                return 1;
            }
        }
        std::printf("Setting up training images...");                                    // :146-150
        std::printf("Setting up testing images...");
        std::printf("done\n");

        tnml_lin* ctx = nullptr;
        if (tnml_lin_create(&ctx, device, N) != 0) die(ctx, "tnml_lin_create");         // ctx stays NULL: the create's error
        CK(ctx, tnml_lin_set_data_u8(ctx, train.size(), train.pixels.data(), train.labels.data()));
        CK(ctx, tnml_lin_set_labels(ctx, K, labs.data()));

        std::vector<double> V((size_t)K * size);
        for (int k = 0; k < K; ++k) {                                                    // :152-163
            const int L = labs[k];
            double* v = V.data() + (size_t)k * size;
            char vn[16]; std::snprintf(vn, sizeof vn, "V%d", L);
            if (file_exists(vn)) {
                std::printf("Reading parameters from disk\n");
                std::vector<double> r = read_vec(vn);
                if ((int)r.size() != size) throw std::runtime_error(std::string(vn) + " holds " + std::to_string(r.size()) + " entries, expected " + std::to_string(size));
                std::copy(r.begin(), r.end(), v);
            } else {
                std::mt19937_64 rng(seed + (uint64_t)L);
                std::uniform_real_distribution<double> u(0., 1.);
                double n2 = 0.;
                for (int j = 0; j < size; ++j) { v[j] = u(rng); n2 += v[j] * v[j]; }
                const double nrm = std::sqrt(n2);
                for (int j = 0; j < size; ++j) v[j] /= nrm;
            }
            double n2 = 0.; for (int j = 0; j < size; ++j) n2 += v[j] * v[j];
            if (K > 1) std::printf("L%d ", L);
            std::printf("norm(V) = %.12g\n", std::sqrt(n2));                             // :164 Print(norm(V))
        }

        CK(ctx, tnml_lin_cg_start(ctx, V.data(), lambda));                               // :166 cgrad(V,train,{Npass,lambda})
        std::vector<double> costs;
        for (long done = 0; done < Niter;) {
            const int nb = (int)std::min<long>(cg_block, Niter - done);
            costs.assign((size_t)nb * K, 0.);
            CK(ctx, tnml_lin_cg_run(ctx, nb, costs.data()));
            for (int p = 0; p < nb; ++p)
                for (int k = 0; k < K; ++k) {
                    if (K > 1) std::printf("L%d", labs[k]);
                    std::printf("  %ld C = %.10f\n", done + p + 1, costs[(size_t)p * K + k]);   // :78
                }
            done += nb;
            std::fflush(stdout);
            if (file_exists("STOP")) {                                                   // :80-85, at a block boundary
                std::printf("Found file STOP, exiting\n");
                std::remove("STOP");
                break;
            }
        }
        CK(ctx, tnml_lin_get_v(ctx, V.data()));

        std::vector<int64_t> nc(K);
        std::vector<double> cnl(K);
        auto evaluate = [&](int T) {                                                     // :169-187
            CK(ctx, tnml_lin_evaluate(ctx, V.data(), nc.data(), cnl.data()));
            for (int k = 0; k < K; ++k) {
                if (K > 1) std::printf("Label %d\n", labs[k]);
                const long long ncor = (long long)nc[k], ninc = T - ncor;
                std::printf("Percent correct = %.4f%%, #correct = %lld/%d, #incorrect = %lld/%d\n", ncor * 100. / T, ncor, T, ninc, T);
                const double* v = V.data() + (size_t)k * size;
                double vv = 0.; for (int j = 0; j < size; ++j) vv += v[j] * v[j];
                const double Cl = lambda * vv;
                std::printf("C (= %.10f + %.10f) = %.10f\n", cnl[k], Cl, cnl[k] + Cl);
            }
        };
        std::printf("Evaluating training set\n");                                        // :188
        evaluate(train.size());
        std::printf("Evaluating testing set\n");                                         // :190
        CK(ctx, tnml_lin_set_data_u8(ctx, test.size(), test.pixels.data(), test.labels.data()));
        evaluate(test.size());
        tnml_lin_destroy(ctx);

        for (int k = 0; k < K; ++k) {                                                    // :192
            char vn[16]; std::snprintf(vn, sizeof vn, "V%d", labs[k]);
            write_vec(vn, std::vector<double>(V.begin() + (size_t)k * size, V.begin() + (size_t)(k + 1) * size));
        }
        if (have_sites) std::printf("Reading previous site set from disk\n");          // :194-203 (checked above)
        else write_sites("sites", N, d);

        const double entry_scale = has_fs ? 255. / feature_scale : 1.;
        if (!has_fs) std::printf("W entries are the reference's V(j): they match fixedL at feature_scale = 255\n");
        else std::printf("W entries are V(j)*255/%.6g: they match fixedL at feature_scale = %.6g\n", feature_scale, feature_scale);
        for (int k = 0; k < K; ++k) {                                                    // :205-238
            std::vector<double> v(V.begin() + (size_t)k * size, V.begin() + (size_t)(k + 1) * size);
            HostMPS W = linear_mps(v, entry_scale);
            double vv = v[0] * v[0]; for (int j = 1; j < size; ++j) vv += v[j] * entry_scale * v[j] * entry_scale;
            if (K > 1) std::printf("Label %d\n", labs[k]);
            std::printf("overlap(W,W) = %.12g\n", overlap(W, W));                        // :231
            std::printf("sqr(norm(V)) = %.12g\n", vv);                                   // :232
            char wn[16]; std::snprintf(wn, sizeof wn, "W%d", labs[k]);
            write_mps(wn, W);                                                            // :234
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "Error: %s\n", e.what());
        return 1;
    }
    return 0;
}
