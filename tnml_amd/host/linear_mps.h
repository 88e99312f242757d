// linear_mps.h -- the `linear` driver's files: the parameter vector V%d and its bond-dimension-2 MPS embedding W%d.
//
//   writeToFile / readFromFile<Vector>(Vname)   linear.cc:155,191   -> own versioned format "TNMLV1" (header, size, fp64 values)
//   "Make MPS version of V"                    linear.cc:205-236   -> linear_mps()
// The embedding, per site j = 1..N (links of dimension 2, column-major A[l][s][r] as host_mps.h, 0-based here):
//   A(0,0,0) = 1,  A(1,0,1) = 1,  A(1,1,0) = V(j)          (linear.cc:219-221: A.set(1,1,1,1.), (2,1,2,1.), (2,2,1,V(j)))
// the left boundary [V(0), 1] contracted into site 1 (:223-226), the right boundary picks r = 0 on site N (:227), then
// W.position(1) (:229).  With the product state [1, x_j/4] per site, W . Phi = V(0) + sum_j V(j) x_j/4 = V . v exactly, and
// overlap(W,W) = |V|^2.  `entry_scale` multiplies the site entries V(j) (j >= 1): 1 is the reference; 255 / feature_scale makes
// W evaluate to the same model under fixedL's feature map [1, feature_scale (b/255/255)/4].
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_mps.h"

namespace tnmlh {

inline HostMPS linear_mps(const std::vector<double>& V, double entry_scale = 1.) {
    const int N = (int)V.size() - 1;
    if (N < 1) throw std::runtime_error("linear_mps: V needs at least two entries");
    HostMPS W(N);
    for (int j = 1; j <= N; ++j) {
        Site A(2, 2, 1);
        A.at(0, 0, 0) = 1.;
        A.at(1, 0, 1) = 1.;
        A.at(1, 1, 0) = V[j] * entry_scale;
        if (j == 1) {                                   // W.Aref(1) *= A0, A0 = [V(0), 1]
            Site B(1, A.mr, 1);
            for (int s = 0; s < 2; ++s) for (int r = 0; r < A.mr; ++r) B.at(0, s, r) = V[0] * A.at(0, s, r) + A.at(1, s, r);
            A = B;
        }
        if (j == N) {                                   // W.Aref(N) *= setElt(links.at(N)(1))
            Site B(A.ml, 1, 1);
            for (int s = 0; s < 2; ++s) for (int l = 0; l < A.ml; ++l) B.at(l, s, 0) = A.at(l, s, 0);
            A = B;
        }
        W.A[j] = A;
    }
    compress(W, 0., 1 << 30, true);                     // W.position(1): orthogonality centre on site 1 (cutoff 0: nothing is dropped)
    return W;
}

inline void write_vec(const std::string& fname, const std::vector<double>& V) {
    std::ofstream f(fname, std::ios::binary | std::ios::trunc);
    if (!f) throw std::runtime_error("Couldn't open " + fname + " for writing");
    const char magic[8] = {'T', 'N', 'M', 'L', 'V', '1', 0, 0};
    f.write(magic, 8);
    const int32_t n = (int32_t)V.size();
    f.write(reinterpret_cast<const char*>(&n), sizeof n);
    f.write(reinterpret_cast<const char*>(V.data()), sizeof(double) * V.size());
    if (!f) throw std::runtime_error("write to " + fname + " failed");
}
inline std::vector<double> read_vec(const std::string& fname) {
    std::ifstream f(fname, std::ios::binary);
    if (!f) throw std::runtime_error("Couldn't open " + fname);
    char magic[8]; int32_t n = 0;
    f.read(magic, 8);
    if (!f || std::memcmp(magic, "TNMLV1", 6) != 0) throw std::runtime_error(fname + " is not a TNMLV1 vector file");
    f.read(reinterpret_cast<char*>(&n), sizeof n);
    if (!f || n < 1) throw std::runtime_error(fname + ": bad header");
    std::vector<double> V(n);
    f.read(reinterpret_cast<char*>(V.data()), sizeof(double) * n);
    if (!f) throw std::runtime_error(fname + ": truncated");
    return V;
}

}  // namespace tnmlh
