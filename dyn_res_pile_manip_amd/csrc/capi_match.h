// capi_match.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the stand-alone one-to-one matching distance of two padded cloud batches (k_match.h; the trainer's use of the kernel is
// capi_train.h's).

// A one-shot in a buffer of its own (c->ma_io; train_host.h: cm_layout): no weights, no session begun or ended, nothing of the
// engine, the dispatch marks or the trainer touched.
int drp_cloud_match(drp_ctx* c, const float* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N, int M,
                    double* terms_out, float* grad_p_out, int32_t* match_pq_out, int32_t* match_qp_out, double* dual_out) {
    if (!c) return DRP_EINVAL;
    CHK(check_bn(c, B, N));
    if (N > KA_MAX_POINTS) return fail(c, DRP_EINVAL, "bad shape N=%d (1..%d for a matching)", N, KA_MAX_POINTS);
    if (M <= 0 || M > KA_MAX_POINTS) return fail(c, DRP_EINVAL, "bad shape M=%d (1..%d for a matching)", M, KA_MAX_POINTS);
    if (!p || !n_p || !q || !n_q || !terms_out) return fail(c, DRP_EINVAL, "null argument");
    for (int b = 0; b < B; ++b) {
        if (n_p[b] <= 0 || n_p[b] > N) return fail(c, DRP_EINVAL, "n_p[%d]=%d outside 1..%d", b, n_p[b], N);
        if (n_q[b] <= 0 || n_q[b] > M) return fail(c, DRP_EINVAL, "n_q[%d]=%d outside 1..%d", b, n_q[b], M);
    }
    // the kernel ends after the same number of steps whatever it reads; a matching of points that are no numbers means nothing
    long bad = first_nonfinite_row(p, n_p, B, N);
    if (bad >= 0) return fail(c, DRP_EINVAL, "p[%ld][%ld] is not finite", bad / N, bad % N);
    bad = first_nonfinite_row(q, n_q, B, M);
    if (bad >= 0) return fail(c, DRP_EINVAL, "q[%ld][%ld] is not finite", bad / M, bad % M);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bn = (size_t)B * N, bm = (size_t)B * M;
    const CmLayout lay = cm_layout(B, N, M);
    CHK(ensure(c, c->ma_io, lay.bytes));
    std::vector<char> stage(lay.in_bytes);
    memcpy(stage.data() + lay.pts_p, p, bn * 3 * sizeof(float));
    memcpy(stage.data() + lay.pts_q, q, bm * 3 * sizeof(float));
    memcpy(stage.data() + lay.n_p, n_p, (size_t)B * sizeof(int));
    memcpy(stage.data() + lay.n_q, n_q, (size_t)B * sizeof(int));
    CHK(h2d(c, c->ma_io, stage.data(), lay.in_bytes));
    char* io = ptr<char>(c->ma_io);
    KaArgs a{};
    a.pred = reinterpret_cast<const float*>(io + lay.pts_p); a.p_bstride = (size_t)N * 3; a.p_tstride = 0;
    a.tgt = reinterpret_cast<const float*>(io + lay.pts_q); a.q_bstride = (size_t)M * 3; a.q_tstride = 0;
    a.n_p = reinterpret_cast<const int*>(io + lay.n_p);
    a.n_q = reinterpret_cast<const int*>(io + lay.n_q); a.nq_bstride = 1; a.nq_tstride = 0;
    a.N = N; a.M = M; a.scale = 1.0; a.keep = 0.0;
    a.grad = grad_p_out ? reinterpret_cast<float*>(io + lay.grad) : nullptr;
    a.terms = reinterpret_cast<double*>(io + lay.terms);
    a.match_pq = match_pq_out ? reinterpret_cast<int*>(io + lay.pq) : nullptr;
    a.match_qp = match_qp_out ? reinterpret_cast<int*>(io + lay.qp) : nullptr;
    a.dual = dual_out ? reinterpret_cast<double*>(io + lay.dual) : nullptr;
    {
        ProbeScope ps(c, KC_LOSS);
        ka_launch<false>(dim3(B, 1), c->stream, a);
    }
    if (hipGetLastError() != hipSuccess) { (void)drp_sync(c); return fail(c, DRP_EHIP, "ka_match launch"); }   // (the staging vector is still being read)
    int rc = d2h(c, terms_out, io + lay.terms, (size_t)B * sizeof(double));
    if (rc == DRP_OK && grad_p_out) rc = d2h(c, grad_p_out, io + lay.grad, bn * 3 * sizeof(float));
    if (rc == DRP_OK && match_pq_out) rc = d2h(c, match_pq_out, io + lay.pq, bn * sizeof(int));
    if (rc == DRP_OK && match_qp_out) rc = d2h(c, match_qp_out, io + lay.qp, bm * sizeof(int));
    if (rc == DRP_OK && dual_out) rc = d2h(c, dual_out, io + lay.dual, (bn + bm) * sizeof(double));
    const int rw = guarded_wait(c, nullptr);            // also on an error above: the staging vector goes out of scope
    return rc != DRP_OK ? rc : rw;
}
