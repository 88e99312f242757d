// driver_util.h -- host plumbing the command line drivers share around the C-ABI (which it includes, with HostMPS and
// Dataset): the error exit, W to and from a context, the `precision` key, image loading, device memory planning, and the
// result lines that more than one driver prints.  The log lines that follow the reference's order stay in each driver.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/tnml.h"
#include "host_mps.h"
#include "init_w.h"
#include "mnist_idx.h"

namespace tnmlh {

// "<call>: <last error>" on stderr, exit status 1.  nullptr stands for no tnml_ctx: tnml_last_error(NULL) is the error of
// the last failed tnml_create or device query.
[[noreturn]] inline void die(const tnml_ctx* c, const char* what) { std::fprintf(stderr, "%s: %s\n", what, tnml_last_error(c)); std::exit(1); }
[[noreturn]] inline void die(const tnml_lin* c, const char* what) { std::fprintf(stderr, "%s: %s\n", what, tnml_lin_last_error(c)); std::exit(1); }
[[noreturn]] inline void die(std::nullptr_t, const char* what) { die(static_cast<const tnml_ctx*>(nullptr), what); }
#define CK(c, call) do { if ((call) != 0) tnmlh::die((c), #call); } while (0)

// W into a context and back; the Label extent follows tnml_site_dims (a per-label context never reports a Label site)
inline void upload_mps(tnml_ctx* ctx, const HostMPS& W) {
    for (int j = 1; j <= W.N; ++j) CK(ctx, tnml_set_site(ctx, j, W.A[j].ml, W.A[j].mr, W.A[j].L == NL, W.A[j].a.data()));
}
inline HostMPS download_mps(tnml_ctx* ctx, int N) {
    HostMPS W(N);
    for (int j = 1; j <= N; ++j) {
        int ml, mr, hl; CK(ctx, tnml_site_dims(ctx, j, &ml, &mr, &hl));
        W.A[j] = Site(ml, mr, hl ? NL : 1);
        CK(ctx, tnml_get_site(ctx, j, W.A[j].a.data()));
    }
    return W;
}
inline int max_link_dim(const HostMPS& W) {
    int m = 1;
    for (int j = 1; j <= W.N; ++j) m = std::max(m, std::max(W.A[j].ml, W.A[j].mr));
    return m;
}

// the key `precision`: f64 (alias strict) | mixed | f32, with allow_bf16 also the study modes bf16x3 | bf16 (forward
// contraction on the bf16 matrix pipe); false after printing the accepted values
inline bool parse_dtype(const std::string& precision, bool allow_bf16, int* dtype) {
    if (precision == "f64" || precision == "strict") *dtype = TNML_F64;
    else if (precision == "mixed") *dtype = TNML_F64_E32;
    else if (precision == "f32") *dtype = TNML_F32;
    else if (allow_bf16 && precision == "bf16x3") *dtype = TNML_BF16X3;
    else if (allow_bf16 && precision == "bf16") *dtype = TNML_BF16;
    else { std::printf(allow_bf16 ? "precision must be f64, mixed, f32, bf16x3 or bf16\n" : "precision must be f64, mixed or f32\n"); return false; }
    return true;
}

// read_mnist, then block-mean down-sampling to imglen x imglen when imglen > 0; raw (nullable) receives the images as the file has them
inline Dataset read_images(const std::string& datadir, bool train, long cap, long imglen, Dataset* raw = nullptr) {
    Dataset d = read_mnist(datadir, train, cap);
    if (raw) *raw = d;
    if (imglen > 0) reduce(d, (int)imglen);
    return d;
}
// the t10k images as the held-out set of a training run, read as its training images were; false after printing a mismatch
inline bool read_heldout(const std::string& datadir, long Ntest, long imglen, const Dataset& train, Dataset* test, Dataset* raw = nullptr) {
    *test = read_images(datadir, false, Ntest, imglen, raw);
    if (test->npix() == train.npix()) return true;
    std::printf("heldout: the t10k images have %d pixels, the training images %d\n", test->npix(), train.npix());
    return false;
}
// The key `input_map` (yes | no, default no) of the drivers: the images go to the device as the bytes of the idx file and the device does
// reduce(), the feature map and the transpose (tnml_set_input_map).  The map of a driver's `feature` / `feature_scale` / `imglen` for raw
// images `raw`: reduce()'s geometry (bsize = side / imglen, blocks from side % bsize) and its refusals in its own words; imglen <= 0
// keeps the image, of any shape, with block 1.
struct DriverInputMap {
    tnml_input_map geo{};
    std::vector<double> table;
    std::string feature;
    void print() const {
        std::printf("Input map: %d x %d bytes -> %d x %d sites (%d x %d block sums from (%d, %d)), feature = %s, %d codes\n", geo.src_rows, geo.src_cols,
                    geo.out_rows, geo.out_cols, geo.block, geo.block, geo.row0, geo.col0, feature.c_str(), geo.ncodes);
    }
    void set(tnml_ctx* ctx) {
        tnml_input_map m = geo; m.table = table.data();
        if (tnml_set_input_map(ctx, &m) != 0) die(ctx, "tnml_set_input_map");
    }
};
inline DriverInputMap make_input_map(const Dataset& raw, long imglen, bool normal, double feature_scale) {
    DriverInputMap im;
    tnml_input_map& g = im.geo;
    g.src_rows = raw.rows; g.src_cols = raw.cols; g.block = 1; g.row0 = g.col0 = 0; g.out_rows = raw.rows; g.out_cols = raw.cols;
    if (imglen > 0) {
        if (raw.rows != raw.cols) throw std::runtime_error("reduce: image is not square");
        if (imglen > raw.rows) throw std::runtime_error("reduce: imglen must be between 1 and the image side");
        if (imglen < raw.rows) { g.block = raw.rows / (int)imglen; g.row0 = g.col0 = raw.rows % g.block; g.out_rows = g.out_cols = (int)imglen; }
    }
    if (g.block > 8) throw std::runtime_error("input_map: imglen gives blocks of more than 8 x 8 pixels");
    g.ncodes = 255 * g.block * g.block + 1;
    im.table.resize((size_t)2 * g.ncodes);
    feature_table(normal, feature_scale, g.block, im.table.data());
    im.feature = normal ? "normal" : "series";
    return im;
}
// the test drivers need a `sites` file of N sites of dimension 2 (fulltest.cc:34-41, util.h:68); false after printing why not
inline bool sites_match(int N) {
    if (!file_exists("sites")) { std::printf("Couldn't find file 'sites'\n"); return false; }
    int Ns, ds; read_sites("sites", &Ns, &ds);
    if (Ns != N || ds != 2) { std::printf("Mismatched sizes\n"); return false; }
    return true;
}

// what the contexts on `device` may plan with: 97 % of its free memory, split evenly between `ways` contexts
inline int64_t device_budget(int device, int ways) {
    int64_t freeb = 0, totb = 0;
    if (tnml_device_memory(device, &freeb, &totb) != 0) die(nullptr, "tnml_device_memory");
    return (int64_t)(0.97 * (double)(freeb / ways));
}
inline int count_devices(int first) {                                           // visible HIP devices from ordinal `first` on
    int n = 0; int64_t f, t;
    while (tnml_device_memory(first + n, &f, &t) == 0) ++n;
    return n;
}
// A held-out context keeps all its environments resident beside the training context: the largest m in [floor_m, hi_m] at
// which the two estimates together fit in budget (tnml_plan_maxm bisects for one context), or -1 when even floor_m does not.
inline int fit_maxm_beside(tnml_config train, tnml_config heldout, int floor_m, int hi_m, int64_t budget) {
    auto fits = [&](int m) { train.maxm = heldout.maxm = m; return tnml_estimate_bytes(&train) + tnml_estimate_bytes(&heldout) <= budget; };
    if (!fits(floor_m)) return -1;
    if (fits(hi_m)) return hi_m;
    int lo_m = floor_m;
    while (hi_m - lo_m > 1) { const int mid = lo_m + (hi_m - lo_m) / 2; if (fits(mid)) lo_m = mid; else hi_m = mid; }
    return lo_m;
}

inline void print_heldout_line(double cost_sum, long long ncorrect, long long count) {
    std::printf("Held-out: Percent correct = %.4f%%, # incorrect = %lld/%lld, Cost = %.10f\n", ncorrect * 100. / count,
                count - ncorrect, count, cost_sum / count);
}
// the key `predict_chunk` of the evaluators: > 0 sets the context option of that name; returns the chunk size in effect
inline int predict_chunk_option(tnml_ctx* ctx, long requested) {
    if (requested <= 0) return TNML_PREDICT_CHUNK_DEFAULT;
    CK(ctx, tnml_set_option(ctx, "predict_chunk", (int)requested));
    return (int)requested;
}
// the key `predict_dtype` of the evaluators (f64 | f32, default f64): under predict = yes sets the context option of that name and returns
// whether the fp32 chain kernel is selected; under predict = no the key has no effect, and f32 is said to be ignored
inline bool predict_dtype_option(tnml_ctx* ctx, bool predict, const std::string& value) {
    if (!predict) {
        if (value == "f32") std::printf("predict_dtype = f32 is ignored: it applies to predict = yes only\n");
        return false;
    }
    if (value != "f64" && value != "f32") { std::printf("predict_dtype=%s not recognized (f64 | f32)\n", value.c_str()); std::exit(1); }
    CK(ctx, tnml_set_option(ctx, "predict_dtype", value == "f32" ? TNML_PREDICT_F32 : TNML_PREDICT_F64));
    return value == "f32";
}
// the key `response` of fulltest: a [n][N][2] array of doubles as a NumPy .npy file (format 1.0, little-endian float64, C order)
inline void write_npy_f64_3d(const std::string& path, const double* a, long n0, long n1, long n2) {
    char dict[128];
    std::snprintf(dict, sizeof dict, "{'descr': '<f8', 'fortran_order': False, 'shape': (%ld, %ld, %ld), }", n0, n1, n2);
    std::string hdr(dict);
    while ((10 + hdr.size() + 1) % 64) hdr += ' ';                              // magic, version and length are 10 bytes; the data start at a multiple of 64
    hdr += '\n';
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::printf("Couldn't write file '%s'\n", path.c_str()); std::exit(1); }
    const unsigned char head[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (unsigned char)(hdr.size() & 255), (unsigned char)(hdr.size() >> 8)};
    const size_t cnt = (size_t)n0 * n1 * n2;
    const bool ok = std::fwrite(head, 1, 10, f) == 10 && std::fwrite(hdr.data(), 1, hdr.size(), f) == hdr.size() && std::fwrite(a, sizeof(double), cnt, f) == cnt;
    if (std::fclose(f) != 0 || !ok) { std::printf("Couldn't write file '%s'\n", path.c_str()); std::exit(1); }
}
// fullTest's result table (util.h:186-199) from the images and the misclassified images per label
inline void print_fulltest_table(const int64_t counts[10], const int64_t nincorrect[10]) {
    long nte = 0, tninc = 0;
    for (int l = 0; l < 10; ++l) { nte += (long)counts[l]; tninc += (long)nincorrect[l]; }
    const long tncor = nte - tninc;
    std::printf("%ld/%ld correct (%.2f%%), %ld/%ld incorrect (%.2f%%)\n", tncor, nte, tncor * 100. / nte, tninc, nte, tninc * 100. / nte);
    for (int l = 0; l < 10; ++l) {
        const long nt = (long)counts[l], ni = (long)nincorrect[l], nc = nt - ni;
        if (nt > 0) std::printf("  Digit %d %ld/%ld correct (%.2f%%), %ld/%ld incorrect (%.2f%%)\n", l, nc, nt, nc * 100. / nt, ni, nt, ni * 100. / nt);
    }
    std::printf("Total # test images = %ld\n", nte);
}

}  // namespace tnmlh
