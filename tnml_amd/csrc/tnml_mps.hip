// tnml_mps.hip -- MPS algebra on the weight replica: direct sum, compression, overlap.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "tnml_host.h"

// ---- MPS algebra: direct sum, orthogonalize(args), overlap (fixedL.cc:693-697,729) -----------------
int tnml_mps_place(tnml_ctx* c, int j, int ML, int MR, int row0, int col0, int ml, int mr, int label, const double* A) {
    TCK(ho_locked(c, "tnml_mps_place", true));
    if (c->pend_count > 0) return tnml_fail(c, "tnml_mps_place: a bond update is in flight (tnml_bond_update_end first)");
    if (!A) return tnml_fail(c, "tnml_mps_place: null block");
    if (j < 1 || j > c->N) return tnml_fail(c, "tnml_mps_place: site %d out of range", j);
    if (j == c->c0 ? (label < 0 || label >= TNML_NL) : label != -1)
        return tnml_fail(c, j == c->c0 ? "tnml_mps_place: site %d carries the Label index: label must be in 0..9, got %d"
                                       : "tnml_mps_place: site %d has no Label index (it sits on site %d): label must be -1", j, j == c->c0 ? label : c->c0);
    if (ML < 1 || MR < 1 || ML > c->maxm || MR > c->maxm) return tnml_fail(c, "tnml_mps_place: bond dimension outside 1..maxm");
    if ((j == 1 && ML != 1) || (j == c->N && MR != 1)) return tnml_fail(c, "tnml_mps_place: edge sites must have outer dimension 1");
    if (ml < 1 || mr < 1 || row0 < 0 || col0 < 0 || (long)row0 + ml > ML || (long)col0 + mr > MR)
        return tnml_fail(c, "tnml_mps_place: block [%d,%d) x [%d,%d) leaves the %d x %d site %d", row0, row0 + ml, col0, col0 + mr, ML, MR, j);
    HIPCK(c, hipSetDevice(c->cfg.device));
    SiteT& s = c->W[j];
    w_written(c, "tnml_mps_place");
    const int L = j == c->c0 ? TNML_NL : 1;
    if (!s.placed || s.ml != ML || s.mr != MR || s.L != L) {          // the first placement shapes and zeroes the site
        s.ml = ML; s.mr = MR; s.L = L; s.set = true; s.placed = true;
        HIPCK(c, hipMemsetAsync(s.a, 0, sizeof(double) * (size_t)ML * 2 * MR * L, c->stream));
    }
    // the block goes up at its own size (2 ml mr <= 2 maxm^2 doubles: tB2 holds 40 maxm^2); the stream orders the kernel behind the copy,
    // and the next placement's copy behind the kernel
    HIPCK(c, hipMemcpyAsync(c->tB2, A, sizeof(double) * (size_t)ml * 2 * mr, hipMemcpyHostToDevice, c->stream));
    TCK(launch_mps_place(c, c->tB2, ml, mr, s.a, ML, MR, row0, col0, label < 0 ? 0 : label));
    HIPCK(c, hipStreamSynchronize(c->stream));                         // (A is the caller's again; a faulty copy is reported here)
    c->currb = -1; c->p_valid = false; c->sweep_start = false;
    return 0;
}
static int mps_maxbond(const tnml_ctx* c) { int m = 1; for (int j = 1; j < c->N; ++j) m = std::max(m, c->W[j].mr); return m; }
int tnml_mps_compress(tnml_ctx* c, double cutoff, int maxm, tnml_compress_report* rep) {
    if (c->multi()) return tnml_fail(c, "tnml_mps_compress: one rank only -- this context has a communicator (compress on a context of its own and upload the result)");
    if (c->cfg.nranks != 1) return tnml_fail(c, "tnml_mps_compress: one rank only -- this context is rank %d of %d", c->cfg.rank, c->cfg.nranks);
    if (c->pend_count > 0) return tnml_fail(c, "tnml_mps_compress: a bond update is in flight (tnml_bond_update_end first)");
    TCK(ho_locked(c, "tnml_mps_compress", true));
    if (!(cutoff >= 0.)) return tnml_fail(c, "tnml_mps_compress: cutoff must be >= 0");
    HIPCK(c, hipSetDevice(c->cfg.device));
    TCK(check_W(c));
    const int N = c->N;
    const int mx = (maxm <= 0 || maxm > c->maxm) ? c->maxm : maxm;
    const long fb0 = c->svd_fallbacks;
    const int before = mps_maxbond(c);
    c->currb = -1; c->p_valid = false; c->sweep_start = false; c->plan = BondPlan();
    w_written(c, "tnml_mps_compress");
    for (int j = 1; j <= N; ++j) c->W[j].placed = false;
    // pass 1, right to left: sites N..2 become right-orthonormal, nothing is discarded (cutoff 0, minm = maxm = the bond's dimension;
    // the split keeps min(that, rows, columns) columns, so a bond wider than its rank bound shrinks to it)
    for (int b = N - 1; b >= 1; --b) {
        const int k = c->W[b].mr;
        TCK(launch_bond_form(c, c->W[b], c->W[b + 1], c->tB));
        TCK(svd_split_device(c, c->tB, b, 2, 0., k, k, nullptr, nullptr, nullptr, nullptr));
    }
    // pass 2, left to right: truncate(p, n, maxm, 1, cutoff) on every bond; the centre ends on site N
    double tsum = 0.;
    for (int b = 1; b <= N - 1; ++b) {
        double te = 0.; int m = 0;
        TCK(launch_bond_form(c, c->W[b], c->W[b + 1], c->tB));
        TCK(svd_split_device(c, c->tB, b, 1, cutoff, mx, 1, &te, &m, nullptr, nullptr));
        tsum += te;
        if (rep && rep->newm) rep->newm[b - 1] = m;
        if (rep && rep->truncerr) rep->truncerr[b - 1] = te;
    }
    w_written(c, "tnml_mps_compress");                                 // (the splits above have said "a bond update")
    SYNCK(c, c->stream);
    if (rep) { rep->maxm_before = before; rep->maxm_after = mps_maxbond(c); rep->nbonds = N - 1; rep->truncerr_sum = tsum; rep->fallbacks = c->svd_fallbacks - fb0; }
    return 0;
}
int tnml_mps_overlap(tnml_ctx* c, double* ovl) {
    if (!ovl) return tnml_fail(c, "tnml_mps_overlap: null argument");
    if (c->pend_count > 0) return tnml_fail(c, "tnml_mps_overlap: a bond update is in flight (tnml_bond_update_end first)");
    HIPCK(c, hipSetDevice(c->cfg.device));
    TCK(check_W(c));
    for (int j = 1; j <= c->N; ++j) c->W[j].placed = false;
    // E (ml x ml, symmetric) in sS / sCm (maxm^2 each), T = E A in sM (>= 40 maxm^2 >= 20 ml mr): workspaces of the split, idle here
    double* E = c->sS; double* En = c->sCm;
    TCK(launch_fill_f64(c, E, 1.0, 1));
    for (int j = 1; j <= c->N; ++j) {
        const SiteT& s = c->W[j];
        const double* T = s.a;                                         // site 1: E = [1], T = A
        if (s.ml > 1) {
            ProfScope ps(c, KC_SMALLGEMM);
            TCK(split_gemm(c, false, false, s.ml, 2 * s.mr * s.L, s.ml, E, s.ml, s.a, s.ml, c->sM, s.ml, 4));
            T = c->sM;
        } else if (j > 1) {                                            // a 1 x 1 environment in the bulk: T = E[0] A through the same product
            ProfScope ps(c, KC_SMALLGEMM);
            TCK(split_gemm(c, false, false, 1, 2 * s.mr * s.L, 1, E, 1, s.a, 1, c->sM, 1, 1));
            T = c->sM;
        }
        TCK(launch_mps_transfer(c, s.a, T, 2 * s.ml, s.mr, s.L, En));
        std::swap(E, En);
    }
    double* h = hscal_eig(c);
    HIPCK(c, hipMemcpyAsync(h, E, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    SYNCK(c, c->stream);
    *ovl = h[0];
    return 0;
}
