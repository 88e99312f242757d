// tnml_bond.hip -- the solve at one bond: bond plan (TrainStates::setBond), forward pass and gradient, the device CG, the exact
// solver and pinv of the per-label variant, and the entry points that run one of them on a bond tensor from the host.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "tnml_host.h"

// ---- bond plan (TrainStates::setBond, fixedL.cc:159-190: pointer selection only) ---------------
PackDesc bond_pack_desc(const BondPlan& p) {
    PackDesc d;
    d.TO = 2; d.L = p.LB;
    const long mL = p.mL, mR = p.mR;
    if (p.kind == 1) { d.nx = p.mR; d.sx = 4 * mL; d.ss = 2 * mL; d.ny = p.mL; d.sy = 1; d.st = mL; }
    else             { d.nx = p.mL; d.sx = 1; d.ss = mL; d.ny = p.mR; d.sy = 4 * mL; d.st = 2 * mL; }
    d.sl = 4 * mL * mR;
    d.Kp = p.Kp; d.Np = p.Np;
    return d;
}
int tnml_set_bond(tnml_ctx* c, int b) {
    CollScope coll_(c);
    TCK(ho_locked(c, "tnml_set_bond"));
    const int rc = set_bond_impl(c, b);
    if (rc) { c->currb = -1; c->plan = BondPlan(); }          // no dangling environment pointers after a failed setBond: the next use has to set a bond again
    return rc;
}
int set_bond_impl(tnml_ctx* c, int b) {
    if (b < 1 || b > c->N - 1) return tnml_fail(c, "tnml_set_bond: bond %d out of range", b);
    TCK(check_W(c));
    const int lc = b - 1, rc = b + 2;                         // :164-165
    const bool useL = lc > 0, useR = rc < c->N + 1;           // :166-167
    if (useL && !c->env[lc].built()) return tnml_fail(c, "setBond: left environment (site %d) missing", lc);
    if (useR && !c->env[rc].built()) return tnml_fail(c, "setBond: right environment (site %d) missing", rc);
    {
        EnvProtect keep(c, useL ? lc : 0, useR ? rc : 0);
        c->currb = b;                                         // (eviction keeps what is nearest to the bond that is being set)
        if (useL) TCK(env_ensure(c, lc));
        if (useR) TCK(env_ensure(c, rc));
    }
    BondPlan p;
    p.b = b; p.mL = c->W[b].ml; p.mR = c->W[b + 1].mr;
    if ((useL ? c->env[lc].m : 1) != p.mL || (useR ? c->env[rc].m : 1) != p.mR) return tnml_fail(c, "setBond: env dims do not match W at bond %d", b);
    const int LL = useL ? c->env[lc].L : 1, LR = useR ? c->env[rc].L : 1;
    const bool onB = (c->c0 == b || c->c0 == b + 1);
    const void* LE = useL ? c->env[lc].ptr : c->ones;
    const void* RE = useR ? c->env[rc].ptr : c->ones;
    if (c->single()) {          // single.h:581-596: no Label anywhere; runs the "Label on B" kernels with a label extent of 1
        p.kind = 2; p.LB = 1; p.mI = p.mL; p.mO = p.mR; p.EI = LE; p.phiI = phi_site(c, b); p.EX = RE; p.phiO = phi_site(c, b + 1);
    } else if (onB) {
        if (LL != 1 || LR != 1) return tnml_fail(c, "setBond: Label index on an environment and on B at bond %d", b);
        p.kind = 2; p.LB = TNML_NL; p.mI = p.mL; p.mO = p.mR; p.EI = LE; p.phiI = phi_site(c, b); p.EX = RE; p.phiO = phi_site(c, b + 1);
    } else if (LR == TNML_NL && LL == 1) {
        p.kind = 0; p.LB = 1; p.mI = p.mL; p.mO = p.mR; p.EI = LE; p.phiI = phi_site(c, b); p.EX = RE; p.phiO = phi_site(c, b + 1);
    } else if (LL == TNML_NL && LR == 1) {
        p.kind = 1; p.LB = 1; p.mI = p.mR; p.mO = p.mL; p.EI = RE; p.phiI = phi_site(c, b + 1); p.EX = LE; p.phiO = phi_site(c, b);
    } else {
        return tnml_fail(c, "Couldn't find Label index at bond %d", b);       // fixedL.cc:291-296,362
    }
    p.Kp = ru16(2 * p.mI); p.Np = ru16(2 * p.mO);
    if (c->bf16()) p.Kp = (2 * p.mI + 31) / 32 * 32;            // the bf16 MFMA reduces 32 indices at a time
    c->plan = p; c->currb = b;
    return 0;
}
int tnml_bond_dims(tnml_ctx* c, int b, int* mL, int* mR, int* label_on_B) {
    if (b < 1 || b > c->N - 1 || !c->W[b].set || !c->W[b + 1].set) return tnml_fail(c, "tnml_bond_dims: bad bond %d", b);
    *mL = c->W[b].ml; *mR = c->W[b + 1].mr; *label_on_B = (c->c0 == b || c->c0 == b + 1);
    return 0;
}
static size_t bond_elems(const tnml_ctx* c, int b) {
    return (size_t)c->W[b].ml * 4 * c->W[b + 1].mr * ((c->c0 == b || c->c0 == b + 1) ? TNML_NL : 1);
}
int tnml_bond_tensor(tnml_ctx* c, int b, double* B) {
    HIPCK(c, hipSetDevice(c->cfg.device));
    int mL, mR, lab; TCK(tnml_bond_dims(c, b, &mL, &mR, &lab));
    if (c->W[b].mr != c->W[b + 1].ml) return tnml_fail(c, "bond %d: link dimensions differ", b);
    TCK(launch_bond_form(c, c->W[b], c->W[b + 1], c->tB));
    SYNCK(c, c->stream);
    HIPCK(c, hipMemcpy(B, c->tB, sizeof(double) * bond_elems(c, b), hipMemcpyDeviceToHost));
    return 0;
}

// ---- per-image contractions -----------------------------------------------------------------------
// forward pass with the M-layout fp64 vector `vec` as bond tensor: P = vec*t.v, then mode-specific
// reductions into tail[0..11] (device)
int forward_pass(tnml_ctx* c, const double* vec, int mode, double* tail, bool want_P, bool reduce) {      // !reduce: the partial sums stay in c->partials[c->part_n][12]
    const BondPlan& p = c->plan;
    const size_t ustride = (size_t)p.mO * c->NTp;
    LdotArgs a;
    if (p.kind == 2) { a.A = c->U; a.A_lstride = ustride; a.Bv = p.EX; a.a_is_env = 0; }
    else             { a.A = p.EX; a.A_lstride = ustride; a.Bv = c->U; a.a_is_env = 1; }
    a.mq = p.mO; a.NTp = c->NTp; a.label = c->label; a.nl = c->nl(); a.target = c->target();
    a.P = want_P ? (mode == LD_MODE_PAP ? c->Pp : c->P) : nullptr; a.dP = (mode == LD_MODE_PAP) ? nullptr : c->dP; a.mode = mode;
    if (c->f64()) {
        Fgemm64Args f;
        f.EI = p.EI; f.EI_lstride = 0; f.mI = p.mI; f.phiI = p.phiI;
        f.M = vec; f.M_lstride = p.kind == 2 ? (size_t)p.Kp * p.Np : 0; f.Kp = p.Kp; f.Np = p.Np;
        f.phiO = p.phiO;
        f.out = (double*)c->U; f.out_lstride = ustride; f.mO = p.mO;
        f.NTp = c->NTp; f.L = p.LB; f.env64 = c->env64();
        // the bond matrix resident in the registers of a pair of workgroups (kernels_res.hip): from 7 680 images per rank on (the 7 500-image
        // shard of an 8-GPU run: 0.162 ms per bond update against 0.250 for the feature GEMM + label dot pair, profiles/r04_shard7500_res_kernels.txt)
        if (c->fwd_res && c->Ppart && c->env64() && !c->single() && p.kind != 2 && fwd_res_applies(p.mI, p.mO) &&
            (c->fwd_res >= 2 || c->NTp >= 7680) &&
            (size_t)TNML_NL * ustride * sizeof(double) < ((size_t)1 << 32)) {           // (32-bit lane offsets of k_fwd_res: larger shards fall through to the kernels below)
            FwdResArgs fr{(const double*)p.EI, (const double*)p.phiI, vec, (const double*)p.phiO, (const double*)p.EX, ustride, c->NTp, c->NTp / 32, c->Ppart, p.mI, p.mO, p.Kp, p.Np};
            // zero features first in the GEMM waves (120 x 120 bonds): the order table of the site whose feature is phiI -- site b, or b + 1 with the Label on the left
            if (c->fwd_skip && c->zf_ord) fr.ord = c->zf_ord + (size_t)((p.kind == 1 ? p.b + 1 : p.b) - 1) * c->NTp;
            TCK(launch_fwd_res(c, fr));
            PfinishArgs pf{2, c->Ppart, nullptr, nullptr, nullptr, nullptr, c->label, c->NTp, (double*)a.P, (double*)a.dP, mode, c->partials, c->counters, tail, mode == LD_MODE_PAP ? 1 : 0};
            TCK(launch_pfinish(c, pf));
            c->part_n = c->NTp / 64;
            return reduce ? launch_labeldot_reduce(c, c->NTp / 64, tail, mode == LD_MODE_PAP ? 1 : 0) : 0;
        }
        // one persistent kernel for both halves of B*t.v where it pays (kernels_fused.hip)
        if (c->fused_fwd && c->env64() && !c->single() && p.kind != 2 && p.Kp == 240 && p.Np == 240 && p.mI == 120 && p.mO == 120 &&
            (c->fused_fwd >= 2 || c->NTp / 64 >= 224)) {
            FwdFusedArgs ff;
            ff.EI = (const double*)p.EI; ff.mI = p.mI; ff.phiI = (const double*)p.phiI; ff.M = vec; ff.Kp = p.Kp; ff.Np = p.Np;
            ff.phiO = (const double*)p.phiO; ff.EL = (const double*)p.EX; ff.EL_lstride = ustride; ff.mO = p.mO; ff.NTp = c->NTp; ff.ntiles = c->NTp / 64;
            ff.label = c->label; ff.P = (double*)a.P; ff.dP = (double*)a.dP; ff.mode = mode; ff.partials = c->partials;
            TCK(launch_fwd_fused(c, ff));
            c->part_n = ff.ntiles;
            return reduce ? launch_labeldot_reduce(c, ff.ntiles, tail, mode == LD_MODE_PAP ? 1 : 0) : 0;
        }
        TCK(launch_fgemm64(c, f));
    } else {
        if (c->bf16() && c->bf16_once && c->ebt && p.kind != 2) {        // operands converted once per bond / per launch (kernels_bf16e.hip)
            TCK(launch_fgemm_bf16e(c, (const float*)p.EI, p.mI, (const float*)p.phiI, vec, p.Kp, p.Np, (const float*)p.phiO, (float*)c->U, p.mO));
        } else {
            TCK(launch_cvt(c, vec, c->Mf, p.msize()));
            FgemmArgs f;
            f.EI = (const float*)p.EI; f.EI_lstride = 0; f.mI = p.mI; f.phiI = (const float*)p.phiI;
            f.M = c->Mf; f.M_lstride = p.kind == 2 ? (size_t)p.Kp * p.Np : 0; f.Kp = p.Kp; f.Np = p.Np;
            f.phiO = (const float*)p.phiO;
            f.out = (float*)c->U; f.out_lstride = ustride; f.mO = p.mO;
            f.NTp = c->NTp; f.L = p.LB;
            TCK(launch_fgemm(c, f));
        }
    }
    return launch_labeldot(c, a, tail, reduce);
}
// G = sum_n dP_n*dag(t.v) over all ranks for the bond tensor in vB; cost partials ride in the tail.
// weights_pp: the image sum A p = sum_n (p.v_n) v_n instead, weights p.v_n as left in Pp by the pAp pass (fast_conj of the per-label
// variant, single.h:347-379, and the merged CG of every variant); the tail is left as it is
static int grad_eval(tnml_ctx* c, bool from_P_update = false, bool outputs_current = false, bool weights_pp = false, bool reduce = true, bool fold = false, bool p_updated = false) {
    const BondPlan& p = c->plan;
    const size_t n = p.msize();
    if (weights_pp) {}
    else if (outputs_current)    { if (!c->tail_zeroed) HIPCK(c, hipMemsetAsync(c->tail, 0, sizeof(double) * TNML_NSCAL_AR, c->stream)); }   // P/dP already hold B*t.v and the residuals (the pack kernel of tnml_bond_update has cleared the tail)
    else if (from_P_update) { if (!p_updated) TCK(launch_pupdate(c, c->scal + SC_ALPHA, c->tail, !fold)); }   // P += a (p*t.v): no GEMM (p_updated: the CG step kernel has done it)
    else                    TCK(forward_pass(c, c->vB, LD_MODE_COST, c->tail, c->fast_cg)); // keeps P when fast CG is on
    const void* wsrc = weights_pp ? c->Pp : c->dP;           // the per-image weights of the sum
    const bool fuse = c->f64() && c->fuse_z && p.kind != 2;
    if (p.kind != 2 && !fuse) TCK(launch_zprime(c, p.EX, (size_t)p.mO * c->NTp, wsrc, c->Zp, p.mO, c->NTp));
    if (c->f64()) {
        Bgemm64Args g;
        g.EL = nullptr; g.EL_lstride = 0; g.dPz = nullptr; g.env64 = c->env64();
        g.EI = p.EI; g.mI = p.mI; g.phiI = p.phiI; g.phiO = p.phiO; g.mO = p.mO;
        g.Kp = p.Kp; g.Np = p.Np; g.NTp = c->NTp; g.L = p.LB;
        if (p.kind == 2) { g.Zq64 = nullptr; g.Zq32 = p.EX; g.w = (const double*)wsrc; g.w_lstride = c->NTp; }
        else if (fuse)   { g.Zq64 = nullptr; g.Zq32 = nullptr; g.w = nullptr; g.w_lstride = 0; g.EL = p.EX; g.EL_lstride = (size_t)p.mO * c->NTp; g.dPz = (const double*)wsrc; }
        else             { g.Zq64 = (const double*)c->Zp; g.Zq32 = nullptr; g.w = nullptr; g.w_lstride = 0; }
        TCK(launch_bgemm64(c, g, c->vG));
    } else {
        BgemmArgs g;
        g.EI = (const float*)p.EI; g.mI = p.mI; g.phiI = (const float*)p.phiI; g.phiO = (const float*)p.phiO; g.mO = p.mO;
        g.Kp = p.Kp; g.Np = p.Np; g.NTp = c->NTp; g.L = p.LB; g.bf16 = c->bf16() && c->bf16_grad ? c->bf16() : 0;
        if (p.kind == 2) { g.Zq = (const float*)p.EX; g.w = (const float*)wsrc; g.w_lstride = c->NTp; }
        else             { g.Zq = (const float*)c->Zp; g.w = nullptr; g.w_lstride = 0; }
        TCK(launch_bgemm(c, g, c->vG));
    }
    return reduce ? allreduce_packed(c, n) : 0;
}
static int read_scal(tnml_ctx* c, const double* dev, int count, double* host_out) {
    double* h = hscal_trace(c);
    if (count > HREP_TRACE_N) return tnml_fail(c, "read_scal: count too large");
    HIPCK(c, hipMemcpyAsync(h, dev, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    SYNCK(c, c->stream);
    memcpy(host_out, h, sizeof(double) * count);
    return 0;
}

// cgrad, fixedL.cc:349-445, on the bond tensor in vB (M-layout)
// issues the whole CG without a host round trip: the |r| < cconv exit (fixedL.cc:432-436) is a device
// flag that turns the state-changing kernels of later passes into no-ops; the per-pass numbers the
// reference prints are collected in a device trace and fetched once by cgrad_fetch_trace().
int cgrad_device(tnml_ctx* c, int npass, double lambda, double cconv, bool outputs_current) {
    if (npass < 1 || npass > TNML_MAX_PASS) return tnml_fail(c, "cgrad: Npass must be in 1..%d", TNML_MAX_PASS);
    const size_t n = c->plan.msize();
    const bool fastc = c->single() && c->cg_method == 1;   // method = fast_conj of the per-label variant (single.h:290-398)
    // Merged passes (one all-reduce per pass instead of two): with P <- P + a (p*t.v) already in use, the image sum of a pass can be
    // A p = sum_n (p.v_n) v_n -- formed from the pAp pass's own outputs BEFORE alpha is known -- so that it travels with
    // sum_n |p.v_n|^2; the residual then follows nr = r - a (A p + lambda p) instead of being re-summed from the new dP (the same
    // algebra; rounding differs at 1e-16 |r| per pass).  The cost partials of a pass's update ride in the NEXT pass's all-reduce.
    // It is used where it buys something -- when the sum over images is also a sum over ranks (merged_cg = 1) -- because the
    // recurrence is not the reference's literal order: on the reference's own, badly conditioned feature map the fourth step size of
    // a Label-on-B bond moves by 1e-3 (the cost by 1e-10); merged_cg = 2 forces it on a single rank (parity tests), 0 disables it.
    const bool merged = c->fast_cg && !fastc && (c->merged_cg >= 2 || (c->merged_cg == 1 && c->multi()));
    // one rank, literal pass order: the per-block partial sums of a pAp pass / an output update are summed by the CG step kernel that
    // consumes them (k_cg_step2: sum |p.v|^2, k_cg_resid2: the cost of the trace) -- seven k_reduce_partials launches less per bond update
    const bool fold = !c->multi() && !merged && !fastc && c->fast_cg;
    // one rank, fp64: the slab reduction of every gradient GEMM is folded into the CG vector kernel that consumes G, the output update
    // P <- P + a (p*t.v) rides in the CG step kernel, and k_cg_init2's work is split between its neighbours (round 5: eight launches less)
    c->defer_slab = fold && c->f64();
    const bool step_updates = fold && c->f64();
    int rc = grad_eval(c, false, outputs_current);       // :374-385
    if (!rc) rc = launch_cg_init(c, n, lambda, c->single() ? cconv : -1.);   // :386-388 (single.h:200-208 with the entry check)
    for (int pass = 1; !rc && pass <= npass; ++pass) {   // :389
        c->cg_pass = pass;
        rc = forward_pass(c, c->vP, LD_MODE_PAP, c->tail, c->fast_cg || fastc, !fold);   // :394-401 (keeps p*t.v for the fast update)
        if (rc) break;
        if (merged && pass < npass) rc = grad_eval(c, false, false, true);        // A p, all-reduced with the tail
        else if (!fold) rc = allreduce(c, c->tail, TNML_NSCAL_AR);                 // :402
        if (rc) break;
        const bool upd = step_updates && pass < npass;
        const int npp = c->part_n;                       // rows of the pAp pass's partial sums (the update below re-sets part_n)
        rc = launch_cg_step(c, n, lambda, pass, merged, fold ? c->partials : nullptr, npp, upd); // :403-407
        if (rc || pass == npass) break;                  // :409
        if (merged) {
            rc = launch_pupdate(c, c->scal + SC_ALPHA, c->tail);                  // P, dP and the cost partials of the new B (:414-420, without the GEMM)
        } else if (fastc) {                              // single.h:347-379: A p from the p.v of this pass, residual by recurrence
            rc = grad_eval(c, false, false, true);
            if (!rc) rc = launch_cg_fast_resid0(c, n, pass);
        } else rc = grad_eval(c, c->fast_cg, false, false, true, fold, upd);      // :412-421
        if (rc) break;
        rc = launch_cg_resid(c, n, lambda, cconv, pass, merged, fold ? (upd ? c->partials2 : c->partials) : nullptr, c->part_n); // :422-428, :432-436, :442
    }
    c->defer_slab = false; c->slab_pending = 0;
    return rc;
}
// the CG's device scalars and per-pass trace: enqueue the copies, parse after any later synchronisation of the stream
// slot >= 0: into the report block of that bond update in flight (parsed by tnml_bond_update_end: two may be in flight)
int cgrad_trace_enqueue(tnml_ctx* c, int slot) {
    HIPCK(c, hipMemcpyAsync(trace_host(c, slot), c->scal, sizeof(double) * HREP_TRACE_N, hipMemcpyDeviceToHost, c->stream));
    return 0;
}
void cgrad_trace_parse(tnml_ctx* c, int npass, tnml_cg_trace* tr, int slot) {
    memset(tr, 0, sizeof *tr);
    const double* hp = trace_host(c, slot);
    const int done = (int)llround(hp[SC_NPASS]);
    tr->npass_done = done;
    tr->converged = (int)llround(hp[SC_CONV]);
    for (int p = 0; p < done && p < npass; ++p) {
        const double* t = hp + SC_N + 4 * p;
        tr->pAp[p] = t[0]; tr->alpha[p] = t[1]; tr->cost[p] = t[2]; tr->rnorm[p] = t[3];
    }
}
static int cgrad_fetch_trace(tnml_ctx* c, int npass, tnml_cg_trace* tr) {
    if (!tr) return 0;
    TCK(cgrad_trace_enqueue(c));
    SYNCK(c, c->stream);
    cgrad_trace_parse(c, npass, tr);
    return 0;
}
// quadcost, fixedL.cc:280-344, on the bond tensor in vB
// launches only: cost partials, #correct and |B|^2 end up in the 13 doubles behind G (t[0..9] per-label costs, t[10] ncorrect, t[12] |B|^2)
static int quadcost_launch(tnml_ctx* c, bool want_P) {
    const size_t n = c->plan.msize();
    TCK(forward_pass(c, c->vB, LD_MODE_COST, c->tail, want_P));
    TCK(allreduce(c, c->tail, TNML_NSCAL_AR));
    TCK(launch_sqnorm(c, c->vB, n, c->tail + 12));              // |B|^2 rides behind the cost partials (local: written after the reduction)
    return 0;
}
void quadcost_parse(tnml_ctx* c, const double* t, double lambda, double* cost, double* label_cost, double* reg_cost, int64_t* ncorrect) {
    const double bn2 = t[12];
    c->last_bnorm = std::sqrt(bn2);
    const double CR = lambda * bn2;                       // :329
    double C = 0.;
    for (int l = 0; l < TNML_NL; ++l) { if (label_cost) label_cost[l] = t[l]; C += t[l]; }   // :331-336
    C += CR;                                              // :338
    if (cost) *cost = C;
    if (reg_cost) *reg_cost = CR;
    if (ncorrect) *ncorrect = (int64_t)llround(t[SC_NCORR]);
}
int quadcost_device(tnml_ctx* c, double lambda, double* cost, double* label_cost, double* reg_cost, int64_t* ncorrect, bool want_P) {
    TCK(quadcost_launch(c, want_P));
    double t[13];
    TCK(read_scal(c, c->tail, 13, t));
    quadcost_parse(c, t, lambda, cost, label_cost, reg_cost, ncorrect);
    return 0;
}

// One-sided Jacobi (Hestenes) SVD of a tall column-major matrix A (R x C, R >= C), in place on the host: on return column j of A
// is u_j s_j, V (C x C) holds the right singular vectors, s the singular values (unsorted).  Small singular values keep their
// relative accuracy, which the pcut test of the exact solver needs (a Gram matrix loses everything below sqrt(eps) s_max).
static bool hestenes_svd(int R, int C, double* A, double* sv, double* V) {      // false: 60 sweeps did not converge
    for (int j = 0; j < C; ++j) for (int i = 0; i < C; ++i) V[i + (size_t)C * j] = i == j ? 1. : 0.;
    bool converged = false;
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < C - 1; ++p)
            for (int q = p + 1; q < C; ++q) {
                double* ap = A + (size_t)R * p; double* aq = A + (size_t)R * q;
                double alpha = 0., beta = 0., gamma = 0.;
                for (int i = 0; i < R; ++i) { alpha += ap[i] * ap[i]; beta += aq[i] * aq[i]; gamma += ap[i] * aq[i]; }
                if (!(std::fabs(gamma) > 1e-15 * std::sqrt(alpha * beta))) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2. * gamma);
                const double t = (zeta >= 0. ? 1. : -1.) / (std::fabs(zeta) + std::sqrt(1. + zeta * zeta));
                const double cs = 1. / std::sqrt(1. + t * t), sn = cs * t;
                for (int i = 0; i < R; ++i) { const double x = ap[i], y = aq[i]; ap[i] = cs * x - sn * y; aq[i] = sn * x + cs * y; }
                double* vp = V + (size_t)C * p; double* vq = V + (size_t)C * q;
                for (int i = 0; i < C; ++i) { const double x = vp[i], y = vq[i]; vp[i] = cs * x - sn * y; vq[i] = sn * x + cs * y; }
            }
        if (!rotated) { converged = true; break; }
    }
    for (int j = 0; j < C; ++j) { double t = 0.; const double* a = A + (size_t)R * j; for (int i = 0; i < R; ++i) t += a[i] * a[i]; sv[j] = std::sqrt(t); }
    return converged;
}
// exact (single.h:117-160, per-label variant): B = y Phi^+ with the filtered inverse s/(s^2 + lambda) above pcut, Phi = [v_1 ... v_NT]
// (D x NT, D = 4 mL mR).  "Only works for rather small number of training samples" (single.h:114).  The dense per-image tensors
// are not formed on the device here either: row j of Phi is the output vector of ONE forward pass of the unit tensor e_j
// (p.v_n = v_n[j], the pAp pass of the CG).  The D x NT matrix then goes to the host, whose one-sided Jacobi SVD keeps the small
// singular values accurate enough for the reference's `s > pcut` test (pcut = 1E-8 by default).  Result in vB (M-layout) and tB
// (ITensor layout).  One rank only: the images of other ranks would have to be gathered.
int exact_device(tnml_ctx* c, double lambda, double pcut) {
    if (!c->single()) return tnml_fail(c, "exact: only the per-label variant (TNML_MODE_SINGLE) has this solver");
    if (c->cfg.dtype != TNML_F64) return tnml_fail(c, "exact: TNML_F64 contexts only");
    if (c->cfg.nranks > 1) return tnml_fail(c, "exact: one rank only (the design matrix of all images is needed in one place)");
    const BondPlan p = c->plan;
    const PackDesc pd = bond_pack_desc(p);
    const int D = p.mL * 4 * p.mR, NT = c->NT;
    // the one-sided Jacobi below costs ~6 min(D, NT)^2 max(D, NT) flops per sweep on ONE host thread and needs up to a few dozen sweeps
    if (D > 4096 || (double)D * NT > 4e8 || (double)std::min(D, NT) * std::min(D, NT) * std::max(D, NT) > 2e10)
        return tnml_fail(c, "exact: %d unknowns x %d images -- the dense solver is meant for small problems (\"Only works for rather small number of training samples\", single.h:114)", D, NT);
    std::vector<double> Pt((size_t)NT * D);                             // Phi^T, column j = row j of Phi
    std::vector<int> lab((size_t)NT);
    HIPCK(c, hipMemcpyAsync(lab.data(), c->label, sizeof(int) * (size_t)NT, hipMemcpyDeviceToHost, c->stream));
    for (int j = 0; j < D; ++j) {
        HIPCK(c, hipMemsetAsync(c->tB2, 0, sizeof(double) * D, c->stream));
        TCK(launch_fill_f64(c, c->tB2 + j, 1.0, 1));
        TCK(launch_pack(c, pd, c->tB2, c->vP, nullptr));
        TCK(forward_pass(c, c->vP, LD_MODE_PAP, c->tail, true));      // Pp[n] = v_n . e_j
        HIPCK(c, hipMemcpyAsync(Pt.data() + (size_t)NT * j, c->Pp, sizeof(double) * (size_t)NT, hipMemcpyDeviceToHost, c->stream));
    }
    SYNCK(c, c->stream);
    std::vector<double> hB((size_t)D, 0.);
    const int tgt = c->target();
    if (NT >= D) {                                                      // Phi^T = U S V^T: columns u_j s_j (images), V in tensor space
        std::vector<double> V((size_t)D * D), sv((size_t)D);
        if (!hestenes_svd(NT, D, Pt.data(), sv.data(), V.data())) return tnml_fail(c, "exact: the Jacobi SVD of the %d x %d design matrix did not converge in 60 sweeps", NT, D);
        for (int j = 0; j < D; ++j) {
            const double s1 = sv[j];
            if (!(s1 > pcut)) continue;                                 // pseudoInv, single.h:145-153
            double yu = 0.;
            const double* u = Pt.data() + (size_t)NT * j;
            for (int i = 0; i < NT; ++i) if (lab[i] == tgt) yu += u[i];  // y . (u_j s_j)
            const double f = yu / (s1 * s1 + lambda);                   // (y.u_j) s/(s^2+lambda) = (y.u_j s_j)/(s^2+lambda)
            const double* v = V.data() + (size_t)D * j;
            for (int k = 0; k < D; ++k) hB[k] += f * v[k];
        }
    } else {                                                            // more unknowns than images: Phi = V' S U'^T on the D x NT matrix
        std::vector<double> Ph((size_t)D * NT), U((size_t)NT * NT), sv((size_t)NT);
        for (int j = 0; j < D; ++j) for (int i = 0; i < NT; ++i) Ph[j + (size_t)D * i] = Pt[i + (size_t)NT * j];
        if (!hestenes_svd(D, NT, Ph.data(), sv.data(), U.data())) return tnml_fail(c, "exact: the Jacobi SVD of the %d x %d design matrix did not converge in 60 sweeps", D, NT);
        for (int j = 0; j < NT; ++j) {
            const double s1 = sv[j];
            if (!(s1 > pcut)) continue;
            double yu = 0.;
            const double* u = U.data() + (size_t)NT * j;
            for (int i = 0; i < NT; ++i) if (lab[i] == tgt) yu += u[i];
            const double f = yu / (s1 * s1 + lambda);                   // (y.u'_j) s/(s^2+lambda) v'_j with v'_j = column / s
            const double* vs = Ph.data() + (size_t)D * j;
            for (int k = 0; k < D; ++k) hB[k] += f * vs[k];
        }
    }
    HIPCK(c, hipMemcpyAsync(c->tB, hB.data(), sizeof(double) * D, hipMemcpyHostToDevice, c->stream));
    TCK(launch_pack(c, pd, c->tB, c->vB, nullptr));
    SYNCK(c, c->stream);                          // hB is a local
    return 0;
}

static int upload_bond(tnml_ctx* c, const double* B) {     // host ITensor layout -> tB, vB
    if (c->currb < 1) return tnml_fail(c, "setBond has not been called");
    const BondPlan& p = c->plan;
    const size_t ne = (size_t)p.mL * 4 * p.mR * p.LB;
    HIPCK(c, hipMemcpyAsync(c->tB, B, sizeof(double) * ne, hipMemcpyHostToDevice, c->stream));
    return launch_pack(c, bond_pack_desc(p), c->tB, c->vB, nullptr);
}
static int download_bond(tnml_ctx* c, const double* Mvec, double* B) {   // M-layout -> host ITensor layout
    const BondPlan& p = c->plan;
    const size_t ne = (size_t)p.mL * 4 * p.mR * p.LB;
    TCK(launch_unpack(c, bond_pack_desc(p), Mvec, c->tB2));
    SYNCK(c, c->stream);
    HIPCK(c, hipMemcpy(B, c->tB2, sizeof(double) * ne, hipMemcpyDeviceToHost));
    return 0;
}

int tnml_forward(tnml_ctx* c, const double* B, double* P) {
    TCK(ho_locked(c, "tnml_forward"));
    HIPCK(c, hipSetDevice(c->cfg.device));
    c->p_valid = false;
    TCK(upload_bond(c, B));
    TCK(forward_pass(c, c->vB, LD_MODE_COST, c->tail, true));
    const size_t ne = (size_t)TNML_NL * c->NTp;
    std::vector<char> h(ne * c->esz());
    SYNCK(c, c->stream);
    HIPCK(c, hipMemcpy(h.data(), c->P, h.size(), hipMemcpyDeviceToHost));
    const int nl = c->nl();                                // [NT][10], or [NT] in the per-label variant
    for (int i = 0; i < c->NT; ++i)
        for (int l = 0; l < nl; ++l)
            P[(size_t)i * nl + l] = c->f64() ? ((const double*)h.data())[(size_t)l * c->NTp + i] : (double)((const float*)h.data())[(size_t)l * c->NTp + i];
    return 0;
}
int tnml_gradient(tnml_ctx* c, const double* B, double* G) {
    CollScope coll_(c);
    TCK(ho_locked(c, "tnml_gradient"));
    HIPCK(c, hipSetDevice(c->cfg.device));
    c->p_valid = false;
    TCK(upload_bond(c, B));
    TCK(grad_eval(c));
    return download_bond(c, c->vG, G);
}
// sum_n |p.v_n|^2 + lambda |p|^2 for a direction p (fixedL.cc:394-403), collective
int tnml_pAp(tnml_ctx* c, const double* p, double lambda, double* pAp) {
    CollScope coll_(c);
    TCK(ho_locked(c, "tnml_pAp"));
    HIPCK(c, hipSetDevice(c->cfg.device));
    c->p_valid = false;
    TCK(upload_bond(c, p));
    const size_t n = c->plan.msize();
    TCK(forward_pass(c, c->vB, LD_MODE_PAP, c->tail, false));
    TCK(allreduce(c, c->tail, TNML_NSCAL_AR));
    TCK(launch_sqnorm(c, c->vB, n, c->tail + 12));
    double t[13];
    TCK(read_scal(c, c->tail, 13, t));
    if (pAp) *pAp = t[SC_PP] + lambda * t[12];
    return 0;
}
int tnml_quadcost(tnml_ctx* c, const double* B, double lambda, double* cost, double label_cost[TNML_NL], double* reg_cost, int64_t* ncorrect) {
    CollScope coll_(c);
    TCK(ho_locked(c, "tnml_quadcost"));
    HIPCK(c, hipSetDevice(c->cfg.device));
    c->p_valid = false;
    TCK(upload_bond(c, B));
    return quadcost_device(c, lambda, cost, label_cost, reg_cost, ncorrect, false);
}
// pinv (single.h:404-517, per-label variant): subspace iteration on A = sum_n v_n v_n^T from the start V0 (D x r, columns in ITensor
// order).  E_k = A V_k is the CG's own pair of passes -- a forward pass of V_k (its outputs V_k.v_n stay in Pp) and the gradient GEMM
// weighted with them -- so the dense v_n are not formed here either; the r x r algebra (polar factor, SVD of E through a one-sided Jacobi
// on its r columns, the filtered inverse) runs on the host.  The reference starts from a time-seeded random V and only prints the cost of
// the result (single.h:596-601): a diagnostic, with the start an argument here.  One rank only.
int tnml_pinv(tnml_ctx* c, const double* V0, int r, int npass, double lambda, double pcut, double* B, double* ve, int* npass_done, double* Dsv) {
    TCK(ho_locked(c, "tnml_pinv"));
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (!c->single()) return tnml_fail(c, "tnml_pinv: only the per-label variant (TNML_MODE_SINGLE) has this solver");
    if (c->currb < 1) return tnml_fail(c, "tnml_pinv: setBond has not been called");
    if (c->cfg.nranks > 1) return tnml_fail(c, "tnml_pinv: one rank only");
    const BondPlan p = c->plan;
    const int D = p.mL * 4 * p.mR, NT = c->NT;
    if (r < 1 || r > D || r > 64) return tnml_fail(c, "tnml_pinv: Ntarget = %d outside 1..min(%d, 64)", r, D);
    if (npass < 0) return tnml_fail(c, "tnml_pinv: Npass must be >= 0");
    c->p_valid = false;
    std::vector<double> V((size_t)D * r), E((size_t)D * r), A((size_t)D * r), sv((size_t)r), W((size_t)r * r), hp((size_t)c->NTp);
    std::vector<int> lab((size_t)NT);
    HIPCK(c, hipMemcpy(lab.data(), c->label, sizeof(int) * NT, hipMemcpyDeviceToHost));
    // V = polarU(V0) (:458): V0 W = U S  ->  U W^T
    A.assign(V0, V0 + (size_t)D * r);
    if (!hestenes_svd(D, r, A.data(), sv.data(), W.data())) return tnml_fail(c, "tnml_pinv: the Jacobi SVD of the start did not converge");
    auto polar_from = [&](std::vector<double>& out) {                  // columns of A are u_g s_g, W the right vectors: out = U W^T
        for (int g = 0; g < r; ++g) if (!(sv[g] > 0.)) return false;
        for (int k = 0; k < r; ++k) for (int d = 0; d < D; ++d) { double t = 0.; for (int g = 0; g < r; ++g) t += A[d + (size_t)D * g] / sv[g] * W[k + (size_t)r * g]; out[d + (size_t)D * k] = t; }
        return true;
    };
    if (!polar_from(V)) return tnml_fail(c, "tnml_pinv: the start V0 has linearly dependent columns");
    std::vector<double> yus((size_t)r);
    auto make_E = [&](bool want_yus) -> int {                          // E_k = A V_k for all k (:469-473, :482-486); optionally yUS_k (:513-518)
        for (int k = 0; k < r; ++k) {
            TCK(upload_bond(c, V.data() + (size_t)D * k));
            HIPCK(c, hipMemcpyAsync(c->vP, c->vB, sizeof(double) * p.msize(), hipMemcpyDeviceToDevice, c->stream));
            TCK(forward_pass(c, c->vP, LD_MODE_PAP, c->tail, true));   // Pp[n] = V_k . v_n
            if (want_yus) {
                HIPCK(c, hipMemcpyAsync(hp.data(), c->Pp, sizeof(double) * c->NTp, hipMemcpyDeviceToHost, c->stream));
                SYNCK(c, c->stream);
                double t = 0.; for (int n = 0; n < NT; ++n) if (lab[n] == c->target()) t += hp[n];
                yus[k] = t;
            } else {
                TCK(grad_eval(c, false, false, true, false));          // vG = sum_n (V_k . v_n) v_n
                TCK(download_bond(c, c->vG, E.data() + (size_t)D * k));
            }
        }
        return 0;
    };
    auto dotVE = [&]() { double t = 0.; for (size_t i = 0; i < (size_t)D * r; ++i) t += V[i] * E[i]; return t; };
    TCK(make_E(false));
    double last = dotVE();                                             // :475
    if (ve) ve[0] = last;
    int done = 0;
    for (int pass = 1; pass <= npass; ++pass) {
        TCK(make_E(false));
        A = E;                                                         // E^T (D x r): columns E_k; E W = U S -> F[a][g] = W[a + r g], G[g][:] = U[:, g]
        if (!hestenes_svd(D, r, A.data(), sv.data(), W.data())) return tnml_fail(c, "tnml_pinv: the Jacobi SVD of E did not converge");
        // sort by singular value (descending) so that D reads like the reference's PrintData(D)
        std::vector<int> ord((size_t)r); for (int g = 0; g < r; ++g) ord[g] = g;
        std::sort(ord.begin(), ord.end(), [&](int x, int y) { return sv[x] > sv[y]; });
        std::vector<double> A2((size_t)D * r), W2((size_t)r * r), s2((size_t)r);
        for (int g = 0; g < r; ++g) { s2[g] = sv[ord[g]]; std::copy(A.begin() + (size_t)D * ord[g], A.begin() + (size_t)D * (ord[g] + 1), A2.begin() + (size_t)D * g); std::copy(W.begin() + (size_t)r * ord[g], W.begin() + (size_t)r * (ord[g] + 1), W2.begin() + (size_t)r * g); }
        A.swap(A2); W.swap(W2); sv.swap(s2);
        if (!polar_from(V)) {                                          // rank-deficient E: the polar factor over the non-zero part only
            for (int k = 0; k < r; ++k) for (int d = 0; d < D; ++d) { double t = 0.; for (int g = 0; g < r; ++g) if (sv[g] > 0.) t += A[d + (size_t)D * g] / sv[g] * W[k + (size_t)r * g]; V[d + (size_t)D * k] = t; }
        }
        const double VE = dotVE();                                     // :497 (= sum of the singular values)
        done = pass;
        if (ve) ve[pass] = VE;
        if (std::fabs(VE - last) < 1E-4) break;                        // :500
        last = VE;
    }
    if (npass_done) *npass_done = done;
    std::fill(B, B + D, 0.);
    if (done > 0) {
        if (Dsv) std::copy(sv.begin(), sv.end(), Dsv);
        TCK(make_E(true));                                             // yUS with the V of the last pass
        for (int a = 0; a < r; ++a)
            for (int g = 0; g < r; ++g) {
                const double s1 = sv[g];
                if (!(s1 > pcut)) continue;                            // pseudoInv :417-421
                const double cf = yus[a] * W[a + (size_t)r * g] / (s1 * s1 + lambda);   // F[a][g] s/(s^2+lambda) G[g][:], G = column / s
                for (int d = 0; d < D; ++d) B[d] += cf * A[d + (size_t)D * g];
            }
    }
    return 0;
}
int tnml_exact(tnml_ctx* c, double* B, double lambda, double pcut) {   // single.h:117-160 on the bond chosen by tnml_set_bond
    CollScope coll_(c);
    TCK(ho_locked(c, "tnml_exact"));
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (c->currb < 1) return tnml_fail(c, "tnml_exact: setBond has not been called");
    c->p_valid = false;
    TCK(exact_device(c, lambda, pcut));
    return download_bond(c, c->vB, B);
}
int tnml_cgrad(tnml_ctx* c, double* B, int npass, double lambda, double cconv, tnml_cg_trace* trace) {
    CollScope coll_(c);
    TCK(ho_locked(c, "tnml_cgrad"));
    HIPCK(c, hipSetDevice(c->cfg.device));
    c->p_valid = false;
    TCK(upload_bond(c, B));
    TCK(cgrad_device(c, npass, lambda, cconv));
    TCK(cgrad_fetch_trace(c, npass, trace));
    return download_bond(c, c->vB, B);
}
// test entry: what the last tnml_cgrad left on the device.  "R" / "Pv" / "G": the fp64 CG vectors vR / vP / vG in the host layout of B;
// "P" / "Pp" / "dP": [NTp][nl] doubles, padded rows included, widened from the context's type.  A copy after a synchronisation: no CG
// state changes (the vectors pass through the unpack scratch tB2, as every downloaded bond tensor does).
int tnml_cg_state(tnml_ctx* c, const char* which, double* out, int64_t count) {
    if (!c || !which || !out) return tnml_fail(c, "tnml_cg_state: null argument");
    TCK(ho_locked(c, "tnml_cg_state"));
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (c->currb < 1) return tnml_fail(c, "tnml_cg_state: setBond has not been called");
    const BondPlan& p = c->plan;
    const double* vec = !strcmp(which, "R") ? c->vR : !strcmp(which, "Pv") ? c->vP : !strcmp(which, "G") ? c->vG : nullptr;
    if (vec) {
        const int64_t ne = (int64_t)p.mL * 4 * p.mR * p.LB;
        if (count != ne) return tnml_fail(c, "tnml_cg_state: %s has %lld elements, count = %lld", which, (long long)ne, (long long)count);
        return download_bond(c, vec, out);
    }
    const void* src = !strcmp(which, "P") ? c->P : !strcmp(which, "Pp") ? c->Pp : !strcmp(which, "dP") ? c->dP : nullptr;
    if (!src) return tnml_fail(c, "tnml_cg_state: unknown array \"%s\" (R, Pv, G, P, Pp, dP)", which);
    const int nl = c->nl();
    const size_t ne = (size_t)nl * c->NTp;
    if (count != (int64_t)ne) return tnml_fail(c, "tnml_cg_state: %s has %lld elements, count = %lld", which, (long long)ne, (long long)count);
    std::vector<char> h(ne * c->esz());
    SYNCK(c, c->stream);
    HIPCK(c, hipMemcpy(h.data(), src, h.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < c->NTp; ++i)
        for (int l = 0; l < nl; ++l)
            out[(size_t)i * nl + l] = c->f64() ? ((const double*)h.data())[(size_t)l * c->NTp + i] : (double)((const float*)h.data())[(size_t)l * c->NTp + i];
    return 0;
}
int tnml_svd_split(tnml_ctx* c, const double* B, int b, int ha, double cutoff, int maxm, int minm,
                   double* truncerr, int* newm, double* sv, int* nsv) {
    CollScope coll_(c);
    TCK(ho_locked(c, "tnml_svd_split", true));
    c->sweep_start = false;
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (b < 1 || b > c->N - 1 || (ha != 1 && ha != 2)) return tnml_fail(c, "tnml_svd_split: bad bond/half");
    c->p_valid = false;
    HIPCK(c, hipMemcpyAsync(c->tB, B, sizeof(double) * bond_elems(c, b), hipMemcpyHostToDevice, c->stream));
    TCK(svd_split_device(c, c->tB, b, ha, cutoff, maxm, minm, truncerr, newm, sv, nsv));
    c->currb = -1;
    return 0;
}
