// capi_match_f64.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the float64 yardstick of the matching losses (k_match_f64.h) -- the one-shot on two clouds, and the trainer's float64
// gradients with the matching term, or its mix with the Chamfer term, as the seed of the reverse pass (capi_grad_f64.h:
// train_grad_f64_body with the TR_LOSS_MATCH and TR_LOSS_CHAMFER_MATCH kinds; ka64_run is declared ahead of it).

// drp_cloud_match's contract with p as doubles and, optionally, the pairs given: the kernel the trainer's yardstick runs.  The
// buffer is the one-shots' (c->cloud_io) in a layout of its own (train_host.h: match64_layout): the caller's partners go up
// with the inputs and six blocks come back, which cloud_begin's layout has no room for
int drp_cloud_match_f64(drp_ctx* c, const double* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N, int M,
                        const int32_t* match_in, double* terms_out, double* grad_p_out, int32_t* match_pq_out, int32_t* match_qp_out,
                        double* dual_out, double* cost_out) {
    CHK(cloud_check(c, p, n_p, q, n_q, B, N, M, terms_out, KA_MAX_POINTS, KA_MAX_POINTS, " for a matching"));
    long bad = first_nonfinite_row(p, n_p, B, N);
    if (bad >= 0) return fail(c, DRP_EINVAL, "p[%ld][%ld] is not finite", bad / N, bad % N);
    bad = first_nonfinite_row(q, n_q, B, M);
    if (bad >= 0) return fail(c, DRP_EINVAL, "q[%ld][%ld] is not finite", bad / M, bad % M);
    if (match_in)
        for (int b = 0; b < B; ++b) {
            int row;
            const int why = check_matching(match_in + (size_t)b * N, n_p[b], n_q[b], N, &row);
            if (why != MATCH_OK) return fail(c, DRP_EINVAL, "match_in: sample %d step 0 row %d %s", b, row, matching_fault(why));
        }
    HIPCHK(c, hipSetDevice(c->device));
    const Match64Layout lay = match64_layout(B, N, M, match_in != nullptr);
    CHK(ensure(c, c->cloud_io, lay.bytes));
    std::vector<char> stage(lay.in_bytes);              // read until the wait below
    memcpy(stage.data() + lay.pts_p, p, (size_t)B * N * 3 * sizeof(double));
    memcpy(stage.data() + lay.pts_q, q, (size_t)B * M * 3 * sizeof(float));
    memcpy(stage.data() + lay.n_p, n_p, (size_t)B * sizeof(int32_t));
    memcpy(stage.data() + lay.n_q, n_q, (size_t)B * sizeof(int32_t));
    if (match_in) memcpy(stage.data() + lay.match_in, match_in, (size_t)B * N * sizeof(int32_t));
    CHK(h2d(c, c->cloud_io, stage.data(), lay.in_bytes));
    char* const io = ptr<char>(c->cloud_io);
    void* const outs[6] = {terms_out, grad_p_out, match_pq_out, match_qp_out, dual_out, cost_out};
    Ka64Args a{};
    a.pred = reinterpret_cast<const double*>(io + lay.pts_p);
    a.cp.p_bstride = (size_t)N * 3; a.cp.p_tstride = 0;
    a.cp.q = reinterpret_cast<const float*>(io + lay.pts_q); a.cp.q_bstride = (size_t)M * 3; a.cp.q_tstride = 0;
    a.cp.n_p = reinterpret_cast<const int*>(io + lay.n_p);
    a.cp.n_q = reinterpret_cast<const int*>(io + lay.n_q); a.cp.nq_bstride = 1; a.cp.nq_tstride = 0;
    a.cp.N = N; a.cp.M = M;
    a.b_off = 0; a.B = B; a.scale = 1.0; a.keep = 0.0;
    a.match_in = match_in ? reinterpret_cast<const int*>(io + lay.match_in) : nullptr;
    a.terms = reinterpret_cast<double*>(io + lay.out[0]);
    a.grad = outs[1] ? reinterpret_cast<double*>(io + lay.out[1]) : nullptr;
    a.match_pq = outs[2] ? reinterpret_cast<int*>(io + lay.out[2]) : nullptr;
    a.match_qp = outs[3] ? reinterpret_cast<int*>(io + lay.out[3]) : nullptr;
    a.dual = outs[4] ? reinterpret_cast<double*>(io + lay.out[4]) : nullptr;
    a.cost = outs[5] ? reinterpret_cast<double*>(io + lay.out[5]) : nullptr;
    int rl;
    {
        ProbeScope ps(c, KC_LOSS);
        rl = ka64_run(c, dim3(B, 1), a);
    }
    if (rl != DRP_OK || hipGetLastError() != hipSuccess) { (void)drp_sync(c); return fail(c, DRP_EHIP, "ka64_match launch"); }   // (the staging vector is still being read)
    int rc = DRP_OK;
    for (int k = 0; k < 6; ++k)
        if (rc == DRP_OK && outs[k]) rc = d2h(c, outs[k], io + lay.out[k], lay.out_bytes[k]);
    const int rw = guarded_wait(c, nullptr);            // also on an error above: the staging vector goes out of scope
    return rc != DRP_OK ? rc : rw;
}

// drp_train_grad_f64_untracked's body with the matching term, or the mix, as each step's term: the one-shot contract of that call
int drp_train_grad_f64_match(drp_ctx* c, const float* states, const float* states_delta, const float* actions, const float* attrs,
                             const int32_t* particle_nums, const float* particle_dens, int B, int N, int n_rollout,
                             const float* targets, const int32_t* target_nums, int M, int loss_kind, double match_weight,
                             const int32_t* match_in, double* loss_out, double* loss_terms_out, double* grad_out,
                             double* grad_state_out, int32_t* match_out, double* cost_out, double* margin_out) {
    if (!c) return DRP_EINVAL;
    if (loss_kind != DRP_LOSS_MATCH && loss_kind != DRP_LOSS_CHAMFER_MATCH)
        return fail(c, DRP_EINVAL, "bad loss_kind=%d (the matching kinds: %d, %d)", loss_kind, DRP_LOSS_MATCH, DRP_LOSS_CHAMFER_MATCH);
    ImpulseSource src;
    CHK(impulse_source(c, states_delta, actions, src));
    TrLoss lk = TrLoss::against(loss_kind, targets, target_nums, M);
    lk.match_weight = match_weight; lk.match_in = match_in; lk.match_out = match_out; lk.cost_out = cost_out;
    lk.margin_out = margin_out;
    return train_grad_f64_body(c, states, src.impulses, src.by_actions, attrs, particle_nums,
                               particle_dens, B, N, n_rollout, lk, loss_out, loss_terms_out, grad_out, grad_state_out);
}
