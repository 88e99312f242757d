// tnml_update.hip -- one bond update of the reference's mldmrg loop (fixedL.cc:478-540), device-resident and in two halves, with the
// roll-back of a speculative split, and the held-out context that follows it.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "tnml_host.h"

// ---- one iteration of the mldmrg loop body (fixedL.cc:478-540) ------------------------------------
// One iteration of the mldmrg loop body in two halves, so that a sweep can keep the GPU queue full across bond boundaries:
// tnml_bond_update_begin enqueues the whole bond update (it blocks once, inside the split, for the eigenvalues that fix the
// new bond dimension) and returns; tnml_bond_update_end hands out the report once the end-of-bond scalars have landed.  A
// caller may begin bond k+1 before ending bond k (at most two bond updates in flight): the wait of `end` then costs nothing
// because `begin` of the next bond has already passed its own synchronisation point.
int tnml_bond_update_begin(tnml_ctx* c, int b, int ha, const tnml_sweep_params* sp) {
    CollScope coll_(c);
    TCK(ho_locked(c, "tnml_bond_update_begin"));
    HIPCK(c, hipSetDevice(c->cfg.device));
    if (ha != 1 && ha != 2) return tnml_fail(c, "tnml_bond_update: half must be 1 or 2");
    if (c->pend_count >= 2) return tnml_fail(c, "tnml_bond_update_begin: two bond updates are in flight, call tnml_bond_update_end first");
    const int slot = (c->pend_tail + c->pend_count) & 1;
    PendingReport& pr = c->pend[slot];
    tnml_bond_report* rep = &pr.rep;
    memset(rep, 0, sizeof *rep);
    pr.b = b; pr.ha = ha; pr.sp = *sp; pr.spec = false; pr.pred = false; pr.split_n = 0; pr.nundo = 0; pr.ho = false;
    c->sweep_start = false;
    // what the report needs reaches its pinned block through the kernels that compute it (round 5: four copy kernels per bond update less):
    // the CG scalars and trace (k_cg_step2 / k_cg_resid2 of the fp64 literal or merged CG), the norms of the new bond tensor (partial pairs,
    // summed by tnml_bond_update_end), and -- on one rank -- the after-SVD cost partials (k_reduce_partials)
    const bool exact = c->single() && c->cg_method == 2;              // method = exact (single.h:600)
    const bool fastc_ = c->single() && c->cg_method == 1;
    pr.trace_mirrored = !c->single() && !exact && !fastc_ && !sp->report_costs;    // (the per-label variant's entry check writes its flag in k_cg_init2: it keeps the copy)
    pr.carry_direct = !c->multi();
    if (pr.trace_mirrored) { memset(trace_host(c, slot), 0, sizeof(double) * HREP_TRACE_N); c->hmir = trace_host(c, slot); }
    memset(pend_host(c, slot), 0, sizeof(double) * HREP_CARRY_N);
    struct MirrorOff { tnml_ctx* c; ~MirrorOff() { c->hmir = nullptr; } } mirror_off_{c};
    TCK(tnml_set_bond(c, b));                                         // :488
    if (c->env_budget_bytes > 0 && c->env_async) TCK(env_lookahead(c, b, ha));
    const BondPlan p = c->plan;
    const size_t ne = (size_t)p.mL * 4 * p.mR * p.LB;
    rep->bond = b; rep->half = ha; rep->c = (ha == 1) ? b : b + 1;    // :482
    rep->origm = c->W[b].mr;                                          // :493
    rep->mL = p.mL; rep->mR = p.mR; rep->label_on_B = (p.kind == 2);
    const PackDesc pd = bond_pack_desc(p);
    TCK(launch_bond_form(c, c->W[b], c->W[b + 1], c->tB));            // :494
    bool outputs_current = c->reuse_p && c->p_valid;                  // left by the previous bond update's quadcost
    // option spec_predict: a misprediction must repeat this bond update bit for bit as a run without the option computes it -- and that run
    // reuses P / dP here instead of a forward pass of its own (another summation order).  Keep them: two device-to-device copies per bond update.
    pr.p_saved = false;
    if (c->spec_predict && outputs_current && !c->force_safe) {
        const size_t pb = (size_t)TNML_NL * c->NTp * c->esz();
        if (!c->psave) TCK(ctx_alloc_doubles(c, &c->psave, (size_t)4 * TNML_NL * c->NTp));
        char* sv = (char*)c->psave + (size_t)slot * 2 * TNML_NL * c->NTp * sizeof(double);
        HIPCK(c, hipMemcpyAsync(sv, c->P, pb, hipMemcpyDeviceToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(sv + pb, c->dP, pb, hipMemcpyDeviceToDevice, c->stream));
        pr.p_saved = true;
    }
    c->p_valid = false;
    // with carried outputs no label dot rewrites the [cost | ncorrect | pAp] head of the tail before the first all-reduce: the
    // pack kernel clears it on the way
    TCK(launch_pack(c, pd, c->tB, c->vB, nullptr, outputs_current && !sp->report_costs ? c->tail : nullptr, TNML_NSCAL_AR));
    c->tail_zeroed = outputs_current && !sp->report_costs;
    if (sp->report_costs) {                                           // single.h:572,621: norm(oB), quadcost(oB)
        TCK(quadcost_device(c, sp->lambda_cost, &rep->cost_old, nullptr, nullptr, nullptr, true));
        rep->norm_oB = c->last_bnorm;
        outputs_current = c->reuse_p;                                 // that was the forward pass of the first gradient
    }
    if (exact) TCK(exact_device(c, sp->lambda, c->pcut));
    else TCK(cgrad_device(c, sp->npass, sp->lambda, sp->cconv, outputs_current));   // :504
    c->tail_zeroed = false;
    if (sp->report_costs) TCK(quadcost_device(c, sp->lambda_cost, &rep->cost_cg, nullptr, &rep->reg_cost_cg, nullptr, false));   // single.h:622,626
    if (c->carry_slot >= 0) { TCK(allreduce(c, c->tail + TNML_CARRY, TNML_CARRYN)); TCK(carry_deliver(c)); }   // (only when no packed all-reduce ran above: the exact solver)
    TCK(launch_unpack(c, pd, c->vB, c->tB));
    c->hmir = nullptr;
    if (!pr.trace_mirrored) TCK(cgrad_trace_enqueue(c, slot));        // parsed by tnml_bond_update_end
    // held-out context: the split takes spare buffers whose former tensors the held-out stream may still be copying (an empty wait in practice)
    if (c->ho && c->ho->held->copy_recorded) HIPCK(c, hipStreamWaitEvent(c->stream, c->ho->held->ev_copied, 0));
    TCK(svd_split_device(c, c->tB, b, ha, sp->cutoff, sp->maxm, sp->minm, &rep->truncerr, &rep->newm, nullptr, nullptr, slot));   // :519-522 (may run without its host synchronisation: tnml_ctx::spec_split)
    if (c->debug_nudge_rank == c->cfg.rank) TCK(launch_nudge(c, c->W[b].a));
    // replicas: the two site tensors the split just wrote must be bit-identical on every rank.  Their fingerprint goes into the
    // carried slots of the tail as exact integer pieces (mode 1: summed with the next packed all-reduce, checked when the report
    // is handed out -- no collective of its own).  Mode 2 checks at once, BEFORE anything consumes the tensors (bond tensor, P/dP,
    // the shifted environment): on a mismatch rank 0's two tensors replace everybody's, counted.
    pr.fp = c->multi() && c->check_replicas;
    if (pr.fp) {
        TCK(replica_fingerprint(c, b, b + 1, c->tail + TNML_FPSLOT));
        if (c->check_replicas_mode == 2) {
            TCK(allreduce(c, c->tail + TNML_FPSLOT, 8));
            double* hf = pend_host(c, slot) + HREP_FP;
            HIPCK(c, hipMemcpyAsync(hf, c->tail + TNML_FPSLOT, 8 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            SYNCK(c, c->stream);
            if (!fingerprint_agrees(hf, c->cfg.nranks)) {             // every rank sees the same sums: every rank takes this branch together
                for (int j = b; j <= b + 1; ++j) { SiteT& sT = c->W[j]; TCK(bcast_rank0(c, sT.a, (size_t)sT.ml * 2 * sT.mr * sT.L)); }
                c->replica_repairs += 1;
            }
            pr.fp = false;                                            // settled
        }
    }
    if (c->ho) {                                                      // what the held-out context copies once the split is final (tnml_bond_update_end)
        pr.ho = true; pr.ho_site[0] = c->W[b]; pr.ho_site[1] = c->W[b + 1];
        HIPCK(c, hipEventRecord(pr.ev_ho, c->stream));
    }
    TCK(launch_bond_form(c, c->W[b], c->W[b + 1], c->tB2));           // :527
    TCK(launch_pack(c, pd, c->tB2, c->vB, nullptr));
    // :532 quadcost(newB); P and dP stay for the next bond update.  Its cost partials land in the CARRIED slots of the tail.
    if (pr.carry_direct) {
        // one rank: nothing on the device consumes these cost partials -- the per-block sums go straight to the pinned report block and the
        // host adds them (no k_reduce_partials launch, no copy)
        double* dev_partials = c->partials;
        c->partials = c->hcost + (size_t)slot * c->partial_cap * 12;
        const int rc_ = forward_pass(c, c->vB, LD_MODE_COST, c->tail + TNML_CARRY, true, false);
        c->partials = dev_partials;
        TCK(rc_);
        pr.cost_rows = c->part_n;
    } else TCK(forward_pass(c, c->vB, LD_MODE_COST, c->tail + TNML_CARRY, true));
    TCK(launch_diffnorm_host(c, c->tB2, c->tB, ne, dn_host(c, slot), HREP_DN_PAIRS));   // |newB|^2 (slot 12 of quadcost, :528) and |newB - B|^2 (:530) as partial pairs
    pr.dn_pairs = c->last_dn_pairs;
    const bool multi = c->multi();
    if (multi && c->defer_tail) c->carry_slot = slot;                 // summed by the next packed all-reduce (tnml_bond_update_end flushes otherwise)
    else {
        c->carry_slot = slot;
        if (multi) TCK(allreduce(c, c->tail + TNML_CARRY, TNML_CARRYN));
        TCK(carry_deliver(c));
    }
    HIPCK(c, hipEventRecord(pr.ev, c->stream));
    TCK(shift_env_impl(c, b, ha == 1));                               // :540
    pr.lambda_cost = sp->lambda_cost;
    c->pend_count += 1;
    c->p_valid = true;                                                // in stream order: P/dP of the after-SVD quadcost
    return 0;
}
// a speculative split whose deferred check failed: the site tensors it replaced come back, the buffers it wrote return to the pool
static void spec_rollback(tnml_ctx* c, PendingReport& pr) {
    for (int u = pr.nundo - 1; u >= 0; --u) {
        SiteT& S = c->W[pr.undo[u].j];
        ((pr.undo[u].j == c->c0) ? c->spare_big : c->spare_small).push_back(S.a);
        S.a = pr.undo[u].old; S.ml = pr.undo[u].ml; S.mr = pr.undo[u].mr;
        w_written(c, "a bond update");
    }
    pr.nundo = 0; pr.spec = false;
}
// ... verified: the replaced buffers are free again
static void spec_commit(tnml_ctx* c, PendingReport& pr) {
    for (int u = 0; u < pr.nundo; ++u) ((pr.undo[u].j == c->c0) ? c->spare_big : c->spare_small).push_back(pr.undo[u].old);
    pr.nundo = 0; pr.spec = false;
}
static int heldout_step(tnml_ctx* c, const PendingReport& pr);
// the eigenvalues a speculative split has mirrored (ascending), largest first and clamped at 0, through the truncation rule with the bond
// update's maxm / minm clamped to the context's maxm: the kept column count and, when asked for, the truncation error
static int mirror_truncate(tnml_ctx* c, const PendingReport& pr, const double* hm, double* truncerr) {
    const int n = pr.split_n;
    std::vector<double> p(n);
    for (int g = 0; g < n; ++g) { double lam = hm[n - 1 - g]; if (!(lam > 0.)) lam = 0.; p[g] = lam; }
    const int mx = pr.sp.maxm < c->maxm ? pr.sp.maxm : c->maxm;
    return tnml_truncate(p.data(), n, mx, pr.sp.minm < mx ? pr.sp.minm : mx, pr.sp.cutoff, truncerr);
}
// the deferred check of the speculative split in `slot` failed, or its predicted column count was wrong: roll back, run again, end
static int redo_bond_updates(tnml_ctx* c, int slot, bool mispredicted, tnml_bond_report* rep) {
    PendingReport& pr = c->pend[slot];
    // dependent vectors even after re-orthonormalisation (or the test hook): everything this bond update and the one begun after
    // it wrote is dropped -- site tensors back from their spare buffers -- and both run again, this one with the synchronous split
    // and its rocSOLVER fallback.  Rare (a few per sweep), so the repeat may cost what it costs.
    const bool had_next = c->pend_count == 2;
    PendingReport& nx = c->pend[slot ^ 1];
    SYNCK(c, c->stream);
    if (c->copy_stream) HIPCK(c, hipStreamSynchronize(c->copy_stream));
    const int b1 = nx.b, ha1 = nx.ha; const tnml_sweep_params sp1 = nx.sp;
    const int b0 = pr.b, ha0 = pr.ha; const tnml_sweep_params sp0 = pr.sp;
    if (had_next) { if (nx.nundo == 2) spec_rollback(c, nx); else return tnml_fail(c, "bond %d: cannot repeat after a failed split check (the next bond update kept no undo record)", b0); }
    spec_rollback(c, pr);
    c->pend_count = 0; c->carry_slot = -1; c->p_valid = false; c->currb = -1;
    HIPCK(c, hipMemsetAsync(c->tail + TNML_CARRY, 0, sizeof(double) * TNML_CARRYN, c->stream));
    if (pr.p_saved && c->psave) {                             // (option spec_predict) the outputs the first run of this bond update reused
        const size_t pb = (size_t)TNML_NL * c->NTp * c->esz();
        const char* sv = (const char*)c->psave + (size_t)slot * 2 * TNML_NL * c->NTp * sizeof(double);
        HIPCK(c, hipMemcpyAsync(c->P, sv, pb, hipMemcpyDeviceToDevice, c->stream));
        HIPCK(c, hipMemcpyAsync(c->dP, sv + pb, pb, hipMemcpyDeviceToDevice, c->stream));
        c->p_valid = true; pr.p_saved = false;
    }
    c->spec_redos += 1;
    if (mispredicted) c->mispredicted += 1; else c->svd_fallbacks += 1;
    // what a roll-back costs = the device time of the work enqueued again (tnml_split_stats reports count and sum)
    hipEvent_t re0 = nullptr, re1 = nullptr;
    if (hipEventCreate(&re0) == hipSuccess && hipEventCreate(&re1) == hipSuccess) (void)hipEventRecord(re0, c->stream);
    c->force_safe = true;
    int rc = tnml_bond_update_begin(c, b0, ha0, &sp0);        // lands in `slot` again (pend_tail has not moved)
    c->force_safe = false;
    if (rc) return rc;
    if (had_next) TCK(tnml_bond_update_begin(c, b1, ha1, &sp1));
    if (re0 && re1) { (void)hipEventRecord(re1, c->stream); (mispredicted ? c->pred_redo_events : c->redo_events).push_back({re0, re1}); }
    return tnml_bond_update_end(c, rep);
}
// the split of the bond update in `slot` is settled: its report from what has landed in the pinned blocks
static int assemble_report(tnml_ctx* c, int slot) {
    PendingReport& pr = c->pend[slot];
    double* hq = pend_host(c, slot);
    const bool exact = c->single() && c->cg_method == 2;
    cgrad_trace_parse(c, pr.sp.npass, &pr.rep.cg, slot);
    if (exact) memset(&pr.rep.cg, 0, sizeof pr.rep.cg);              // no CG ran
    if (pr.fp && !fingerprint_agrees(hq + TNML_FPSLOT, c->cfg.nranks))   // every rank sees the same sums
        return tnml_fail(c, "bond %d: replicas of W.A(%d), W.A(%d) differ between ranks after the split", pr.rep.bond, pr.rep.bond, pr.rep.bond + 1);
    double t[13];
    if (pr.carry_direct) {
        const double* hp = c->hcost + (size_t)slot * c->partial_cap * 12;
        for (int l = 0; l < 12; ++l) { double a = 0.; for (int r = 0; r < pr.cost_rows; ++r) a += hp[(size_t)r * 12 + l]; t[l] = a; }
    } else for (int l = 0; l < 12; ++l) t[l] = hq[TNML_CARRY + l];
    double nb2 = 0., df2 = 0.;                                        // the partial pairs of k_diffnorm1, in workgroup order
    { const double* dp = dn_host(c, slot); for (int k = 0; k < pr.dn_pairs; ++k) { nb2 += dp[2 * k]; df2 += dp[2 * k + 1]; } }
    t[12] = nb2;
    quadcost_parse(c, t, pr.lambda_cost, &pr.rep.cost_after_svd, pr.rep.label_cost, &pr.rep.reg_cost, &pr.rep.ncorrect);
    pr.rep.norm_newB = std::sqrt(nb2); pr.rep.diff_B_newB = std::sqrt(df2);
    c->sweep_start = pr.b == 1 && pr.ha == 2;                         // (tnml_sweepnext ends a sweep after bond 1 of half 2)
    if (pr.ho && c->ho && heldout_step(c, pr)) return tnml_fail(c, "held-out context: %s", c->ho->err.c_str());
    if (pr.split_n > 0 && pr.b >= 1 && pr.b < (int)c->bond_hist.size()) {   // the history the prediction reads: what this call reports, after any roll-back
        tnml_ctx::BondHist& hs = c->bond_hist[pr.b];
        hs.n[1] = hs.n[0]; hs.m[1] = hs.m[0]; hs.n[0] = pr.split_n; hs.m[0] = pr.rep.newm;
    }
    return 0;
}
int tnml_bond_update_end(tnml_ctx* c, tnml_bond_report* rep) {
    CollScope coll_(c);
    if (c->pend_count < 1) return tnml_fail(c, "tnml_bond_update_end: no bond update in flight");
    const int slot = c->pend_tail;
    PendingReport& pr = c->pend[slot];
    if (c->carry_slot == slot) {                                      // nothing followed that would have carried them: one small all-reduce
        TCK(allreduce(c, c->tail + TNML_CARRY, TNML_CARRYN));
        TCK(carry_deliver(c));
    }
    HIPCK(c, hipEventSynchronize(pr.ev));
    HIPCK(c, hipEventSynchronize(pr.ev2));
    // a collective of this bond update that gave up waiting for a peer left its buffer unsummed: say so before anything below reads
    // the sums (it would show up as a failed replica check or a failed split check otherwise)
    TCK(ipc_comm_check(c));
    if (pr.spec) {
        // the deferred check of the speculative split: its verdict came with the carried slots (summed over the ranks: every rank sees the same number)
        const double* hq = pend_host(c, slot);
        const double* hm = hrep_eig(c, slot);
        const double* hc = hrep_check(c, slot, pr.split_n);
        const bool check_failed = (c->multi() ? hq[TNML_SPECSLOT] : hc[HC_BAD]) != 0.;   // (one rank: straight from the mirror of the check values)
        // a predicted split (option spec_predict): k_truncate_verdict has left the count the truncation rule keeps behind the check values and its
        // verdict in a carried word of its own.  The host applies the rule to the mirrored eigenvalues as it does for every speculative split;
        // its count must be the kernel's.  A wrong guess takes the roll-back below -- the repeat is the synchronous split, so nothing differs
        // from a run without the option -- but is no fallback of the eigensolver.
        bool wrong_count = false;
        if (pr.pred) {
            const int m_host = mirror_truncate(c, pr, hm, nullptr);
            if ((double)m_host != hc[HC_MKEPT])
                return tnml_fail(c, "bond %d: the truncation rule keeps %d columns on the host and %g on the device", pr.rep.bond, m_host, hc[HC_MKEPT]);
            wrong_count = (c->multi() ? hq[TNML_PREDSLOT] : hc[HC_WRONG]) != 0.;         // (summed over the ranks: every rank rolls back together)
            if (!wrong_count && m_host != pr.m_pred) return tnml_fail(c, "bond %d: the verdict passed a predicted split of %d columns, the truncation rule says %d", pr.rep.bond, pr.m_pred, m_host);
        }
        if (check_failed || wrong_count) return redo_bond_updates(c, slot, wrong_count && !check_failed, rep);
        spec_commit(c, pr);
        // what the synchronous form does right after its host round trip: truncation error from the eigenvalues, statistics
        double te = 0.;
        const int m = mirror_truncate(c, pr, hm, &te);
        if (m != pr.rep.newm) return tnml_fail(c, "bond %d: speculative split kept %d columns, the truncation rule says %d", pr.rep.bond, pr.rep.newm, m);
        pr.rep.truncerr = te;
        c->svd_last_dev0 = hc[HC_DEV0]; c->svd_last_dev1 = 0.75 * hc[HC_DEV0] * hc[HC_DEV0];
        if (hc[HC_CHOLQR] != 0.) c->svd_cholqr += 1;
    } else spec_commit(c, pr);                                        // synchronous split: verified when it ran
    c->pend_tail ^= 1; c->pend_count -= 1;
    TCK(assemble_report(c, slot));
    if (rep) *rep = pr.rep;
    return 0;
}
int tnml_bond_update(tnml_ctx* c, int b, int ha, const tnml_sweep_params* sp, tnml_bond_report* rep) {
    if (c->pend_count != 0) return tnml_fail(c, "tnml_bond_update: a pipelined bond update is still in flight");
    TCK(tnml_bond_update_begin(c, b, ha, sp));
    return tnml_bond_update_end(c, rep);
}

// ---- held-out evaluation during training ------------------------------------------------------------
// A held-out context follows the sweep of the training context it is attached to: it keeps its own environments, receives the two site
// tensors of every bond update once the split is final, and on its OWN stream evaluates the new bond tensor on its images (the forward
// pass and the cost / #correct reduction of the training context's after-SVD quadcost) and shifts its environments as training does.
// Its work overlaps the training context's next bond update; the training stream waits for it only before a split, whose spare buffers
// may still be being copied by the held-out stream.
void heldout_release(tnml_ctx* c) {              // c: the training context
    tnml_ctx* h = c->ho;
    if (!h) return;
    HeldOut* s = h->held;
    (void)hipSetDevice(h->cfg.device);
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamSynchronize(c->stream);              // (a wait of the training stream on ev_copied is settled before the event goes)
    if (s) {
        if (s->ev_copied) (void)hipEventDestroy(s->ev_copied);
        for (auto& e : s->ev_done) if (e) (void)hipEventDestroy(e);
        if (s->host) (void)hipHostFree(s->host);
        delete s;
    }
    h->held = nullptr; c->ho = nullptr;
}
// the forward pass of the held-out images at bond b of the held-out context's W and its reduction -> the next result slot (in stream order)
static int heldout_eval(tnml_ctx* h, int bond, int half, int b) {
    HeldOut* s = h->held;
    if (set_bond_impl(h, b)) { h->currb = -1; h->plan = BondPlan(); return 1; }
    TCK(launch_bond_form(h, h->W[b], h->W[b + 1], h->tB));
    TCK(launch_pack(h, bond_pack_desc(h->plan), h->tB, h->vB, nullptr));
    TCK(forward_pass(h, h->vB, LD_MODE_COST, h->tail, false));         // tail[0..9] cost per label, [10] #correct
    const int k = s->slot ^ 1;
    HIPCK(h, hipMemcpyAsync(s->host + 16 * k, h->tail, sizeof(double) * 12, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipEventRecord(s->ev_done[k], h->stream));
    s->slot = k; s->bond[k] = bond; s->half[k] = half;
    return 0;
}
// the bond update `pr` of the training context c has been verified: its two site tensors go to the held-out context, which evaluates
// them and shifts its environments (errors land in the held-out context's message)
static int heldout_step(tnml_ctx* c, const PendingReport& pr) {
    tnml_ctx* h = c->ho;
    HeldOut* s = h->held;
    HIPCK(h, hipStreamWaitEvent(h->stream, pr.ev_ho, 0));
    for (int u = 0; u < 2; ++u) {
        const SiteT& src = pr.ho_site[u];
        SiteT& dst = h->W[pr.b + u];
        dst.ml = src.ml; dst.mr = src.mr; dst.L = src.L; dst.set = true;
        w_written(h, "a bond update of the training context");
        HIPCK(h, hipMemcpyAsync(dst.a, src.a, sizeof(double) * (size_t)src.ml * 2 * src.mr * src.L, hipMemcpyDeviceToDevice, h->stream));
    }
    HIPCK(h, hipEventRecord(s->ev_copied, h->stream));
    s->copy_recorded = true;
    TCK(heldout_eval(h, pr.b, pr.ha, pr.b));
    return shift_env_impl(h, pr.b, pr.ha == 1);
}
int tnml_heldout_attach(tnml_ctx* c, tnml_ctx* h) {
    if (!c || !h) return tnml_fail(c, "tnml_heldout_attach: null argument");
    if (c == h) return tnml_fail(c, "tnml_heldout_attach: a context cannot be its own held-out set");
    if (c->held) return tnml_fail(c, "tnml_heldout_attach: train is itself attached as a held-out set");
    if (c->ho) return tnml_fail(c, "tnml_heldout_attach: train already has a held-out context");
    if (h->held) return tnml_fail(c, "tnml_heldout_attach: heldout is already attached to a training context");
    if (h->ho) return tnml_fail(c, "tnml_heldout_attach: heldout has a held-out context of its own");
    if (h->cfg.device != c->cfg.device) return tnml_fail(c, "tnml_heldout_attach: device differs (train %d, heldout %d)", c->cfg.device, h->cfg.device);
    if (h->N != c->N) return tnml_fail(c, "tnml_heldout_attach: N differs (train %d, heldout %d)", c->N, h->N);
    if (h->cfg.mode != c->cfg.mode) return tnml_fail(c, "tnml_heldout_attach: mode differs (train %d, heldout %d)", c->cfg.mode, h->cfg.mode);
    if (c->single() && h->cfg.target_label != c->cfg.target_label)
        return tnml_fail(c, "tnml_heldout_attach: target_label differs (train %d, heldout %d)", c->cfg.target_label, h->cfg.target_label);
    if (h->cfg.dtype != c->cfg.dtype) return tnml_fail(c, "tnml_heldout_attach: dtype differs (train %d, heldout %d)", c->cfg.dtype, h->cfg.dtype);
    if (h->maxm < c->maxm) return tnml_fail(c, "tnml_heldout_attach: heldout maxm = %d is smaller than train's maxm = %d", h->maxm, c->maxm);
    if (h->cfg.nranks != 1) return tnml_fail(c, "tnml_heldout_attach: heldout has nranks = %d; it must be one rank (each rank attaches its own shard)", h->cfg.nranks);
    if (!h->data_set) return tnml_fail(c, "tnml_heldout_attach: heldout has no image data (tnml_set_data_*)");
    if (c->pend_count) return tnml_fail(c, "tnml_heldout_attach: a bond update of train is in flight (tnml_bond_update_end first)");
    if (!c->sweep_start)
        return tnml_fail(c, "tnml_heldout_attach: train is not at a sweep start (after tnml_env_init, or after the last bond update of a sweep)");
    TCK(check_W(c));
    HIPCK(c, hipSetDevice(c->cfg.device));
    SYNCK(c, c->stream);
    HeldOut* s = new HeldOut();
    s->train = c;
    int rc = 0;
    if (hipEventCreateWithFlags(&s->ev_copied, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s->ev_done[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&s->ev_done[1], hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc((void**)&s->host, sizeof(double) * 32) != hipSuccess) rc = tnml_fail(h, "event / pinned buffer allocation failed");
    for (int k = 0; k < 2 && !rc; ++k)
        if (!c->pend[k].ev_ho && hipEventCreateWithFlags(&c->pend[k].ev_ho, hipEventDisableTiming) != hipSuccess) rc = tnml_fail(h, "hipEventCreate failed");
    h->held = s; c->ho = h;
    h->p_valid = false;
    for (int j = 1; j <= c->N && !rc; ++j) {               // train's W replica, device to device
        const SiteT& src = c->W[j];
        SiteT& dst = h->W[j];
        dst.ml = src.ml; dst.mr = src.mr; dst.L = src.L; dst.set = true;
        w_written(h, "tnml_heldout_attach");
        if (hipMemcpyAsync(dst.a, src.a, sizeof(double) * (size_t)src.ml * 2 * src.mr * src.L, hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
            rc = tnml_fail(h, "copy of site %d failed", j);
    }
    if (!rc) rc = env_init_impl(h);                          // the environments as tnml_env_init builds them
    if (!rc) rc = heldout_eval(h, 0, 0, 1);                  // bond 0: W as it is now
    if (!rc) rc = tnml_synchronize(h);
    if (rc) {
        std::string msg = h->err;
        heldout_release(c);
        return tnml_fail(c, "tnml_heldout_attach: %s", msg.c_str());
    }
    return 0;
}
int tnml_heldout_detach(tnml_ctx* c) {
    if (!c) return tnml_fail(c, "tnml_heldout_detach: null argument");
    heldout_release(c);
    return 0;
}
int tnml_heldout_read(tnml_ctx* c, tnml_heldout_report* rep) {
    if (!c || !rep) return tnml_fail(c, "tnml_heldout_read: null argument");
    if (!c->ho) return tnml_fail(c, "tnml_heldout_read: no held-out context is attached");
    const tnml_ctx* h = c->ho;
    const HeldOut* s = h->held;
    const int k = s->slot;
    HIPCK(c, hipEventSynchronize(s->ev_done[k]));
    const double* t = s->host + 16 * k;
    memset(rep, 0, sizeof *rep);
    rep->bond = s->bond[k]; rep->half = s->half[k];
    rep->count = h->NT;
    rep->ncorrect = (int64_t)llround(t[SC_NCORR]);
    double C = 0.;
    for (int l = 0; l < TNML_NL; ++l) { rep->label_cost[l] = t[l]; C += t[l]; }
    rep->cost = C;
    return 0;
}
