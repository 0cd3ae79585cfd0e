// capi_chamfer.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the stand-alone Chamfer metric of two padded cloud batches (k_chamfer.h; the trainer's use of the kernel is capi_train.h's).

// A one-shot in a buffer of its own (c->ch_io): no weights, no session begun or ended, nothing of the engine, the dispatch marks
// or the trainer touched.
int drp_cloud_chamfer(drp_ctx* c, const float* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N, int M,
                      double* terms_out, float* grad_p_out, int32_t* nn_pq_out, int32_t* nn_qp_out) {
    if (!c) return DRP_EINVAL;
    CHK(check_bn(c, B, N));
    if (M <= 0 || M > KC_MAX_POINTS) return fail(c, DRP_EINVAL, "bad shape M=%d (1..%d)", M, KC_MAX_POINTS);
    if (!p || !n_p || !q || !n_q || !terms_out) return fail(c, DRP_EINVAL, "null argument");
    for (int b = 0; b < B; ++b) {
        if (n_p[b] <= 0 || n_p[b] > N) return fail(c, DRP_EINVAL, "n_p[%d]=%d outside 1..%d", b, n_p[b], N);
        if (n_q[b] <= 0 || n_q[b] > M) return fail(c, DRP_EINVAL, "n_q[%d]=%d outside 1..%d", b, n_q[b], M);
    }
    HIPCHK(c, hipSetDevice(c->device));
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t bn = (size_t)B * N, bm = (size_t)B * M;
    // up: p | q | n_p | n_q;  down: terms | gradient | a(.) | c(.)
    const size_t o_p = 0, o_q = up(o_p + bn * 3 * sizeof(float)), o_np = up(o_q + bm * 3 * sizeof(float)),
                 o_nq = up(o_np + (size_t)B * sizeof(int)), in_bytes = up(o_nq + (size_t)B * sizeof(int));
    const size_t o_terms = in_bytes, o_grad = up(o_terms + (size_t)B * 2 * sizeof(double)), o_pq = up(o_grad + bn * 3 * sizeof(float)),
                 o_qp = up(o_pq + bn * sizeof(int)), bytes = up(o_qp + bm * sizeof(int));
    CHK(ensure(c, c->ch_io, bytes));
    std::vector<char> stage(in_bytes);
    memcpy(stage.data() + o_p, p, bn * 3 * sizeof(float));
    memcpy(stage.data() + o_q, q, bm * 3 * sizeof(float));
    memcpy(stage.data() + o_np, n_p, (size_t)B * sizeof(int));
    memcpy(stage.data() + o_nq, n_q, (size_t)B * sizeof(int));
    CHK(h2d(c, c->ch_io, stage.data(), in_bytes));
    char* io = ptr<char>(c->ch_io);
    KcArgs a{};
    a.pred = reinterpret_cast<const float*>(io + o_p); a.p_bstride = (size_t)N * 3; a.p_tstride = 0;
    a.tgt = reinterpret_cast<const float*>(io + o_q); a.q_bstride = (size_t)M * 3; a.q_tstride = 0;
    a.n_p = reinterpret_cast<const int*>(io + o_np);
    a.n_q = reinterpret_cast<const int*>(io + o_nq); a.nq_bstride = 1; a.nq_tstride = 0;
    a.N = N; a.M = M; a.scale = 1.0f;
    a.grad = grad_p_out ? reinterpret_cast<float*>(io + o_grad) : nullptr;
    a.terms = reinterpret_cast<double*>(io + o_terms);
    a.nn_pq = nn_pq_out ? reinterpret_cast<int*>(io + o_pq) : nullptr;
    a.nn_qp = nn_qp_out ? reinterpret_cast<int*>(io + o_qp) : nullptr;
    {
        ProbeScope ps(c, KC_LOSS);
        hipLaunchKernelGGL((kc_chamfer<false>), dim3(B, 1), dim3(KC_THREADS), 0, c->stream, a);
    }
    if (hipGetLastError() != hipSuccess) { (void)drp_sync(c); return fail(c, DRP_EHIP, "kc_chamfer launch"); }   // (the staging vector is still being read)
    int rc = d2h(c, terms_out, io + o_terms, (size_t)B * 2 * sizeof(double));
    if (rc == DRP_OK && grad_p_out) rc = d2h(c, grad_p_out, io + o_grad, bn * 3 * sizeof(float));
    if (rc == DRP_OK && nn_pq_out) rc = d2h(c, nn_pq_out, io + o_pq, bn * sizeof(int));
    if (rc == DRP_OK && nn_qp_out) rc = d2h(c, nn_qp_out, io + o_qp, bm * sizeof(int));
    const int rw = guarded_wait(c, nullptr);            // also on an error above: the staging vector goes out of scope
    return rc != DRP_OK ? rc : rw;
}

// drp_cloud_chamfer in float64 (k_chamfer_f64.h), with every direction's smallest arg-min margin: the same contract, in a buffer of
// its own (c->ch64_io)
int drp_cloud_chamfer_f64(drp_ctx* c, const float* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N, int M,
                          double* terms_out, double* grad_p_out, int32_t* nn_pq_out, int32_t* nn_qp_out, double* margin_out) {
    if (!c) return DRP_EINVAL;
    CHK(check_bn(c, B, N));
    if (M <= 0 || M > KC64_MAX_POINTS) return fail(c, DRP_EINVAL, "bad shape M=%d (1..%d)", M, KC64_MAX_POINTS);
    if (!p || !n_p || !q || !n_q || !terms_out) return fail(c, DRP_EINVAL, "null argument");
    for (int b = 0; b < B; ++b) {
        if (n_p[b] <= 0 || n_p[b] > N) return fail(c, DRP_EINVAL, "n_p[%d]=%d outside 1..%d", b, n_p[b], N);
        if (n_q[b] <= 0 || n_q[b] > M) return fail(c, DRP_EINVAL, "n_q[%d]=%d outside 1..%d", b, n_q[b], M);
    }
    HIPCHK(c, hipSetDevice(c->device));
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t bn = (size_t)B * N, bm = (size_t)B * M;
    // up: p | q | n_p | n_q;  down: terms | margins | gradient | a(.) | c(.)
    const size_t o_p = 0, o_q = up(o_p + bn * 3 * sizeof(float)), o_np = up(o_q + bm * 3 * sizeof(float)),
                 o_nq = up(o_np + (size_t)B * sizeof(int)), in_bytes = up(o_nq + (size_t)B * sizeof(int));
    const size_t o_terms = in_bytes, o_mar = up(o_terms + (size_t)B * 2 * sizeof(double)), o_grad = up(o_mar + (size_t)B * 2 * sizeof(double)),
                 o_pq = up(o_grad + bn * 3 * sizeof(double)), o_qp = up(o_pq + bn * sizeof(int)), bytes = up(o_qp + bm * sizeof(int));
    CHK(ensure(c, c->ch64_io, bytes));
    std::vector<char> stage(in_bytes);
    memcpy(stage.data() + o_p, p, bn * 3 * sizeof(float));
    memcpy(stage.data() + o_q, q, bm * 3 * sizeof(float));
    memcpy(stage.data() + o_np, n_p, (size_t)B * sizeof(int));
    memcpy(stage.data() + o_nq, n_q, (size_t)B * sizeof(int));
    CHK(h2d(c, c->ch64_io, stage.data(), in_bytes));
    char* io = ptr<char>(c->ch64_io);
    Kc64Args a{};
    a.p32 = reinterpret_cast<const float*>(io + o_p); a.p_bstride = (size_t)N * 3; a.p_tstride = 0;
    a.tgt = reinterpret_cast<const float*>(io + o_q); a.q_bstride = (size_t)M * 3; a.q_tstride = 0;
    a.n_p = reinterpret_cast<const int*>(io + o_np);
    a.n_q = reinterpret_cast<const int*>(io + o_nq); a.nq_bstride = 1; a.nq_tstride = 0;
    a.b_off = 0; a.B = B; a.N = N; a.M = M; a.scale = 1.0;
    a.grad = grad_p_out ? reinterpret_cast<double*>(io + o_grad) : nullptr;
    a.terms = reinterpret_cast<double*>(io + o_terms);
    a.margin = margin_out ? reinterpret_cast<double*>(io + o_mar) : nullptr;
    a.nn_pq = nn_pq_out ? reinterpret_cast<int*>(io + o_pq) : nullptr;
    a.nn_qp = nn_qp_out ? reinterpret_cast<int*>(io + o_qp) : nullptr;
    hipLaunchKernelGGL((kc64_chamfer<false>), dim3(B, 1), dim3(KC64_THREADS), 0, c->stream, a);
    if (hipGetLastError() != hipSuccess) { (void)drp_sync(c); return fail(c, DRP_EHIP, "kc64_chamfer launch"); }   // (the staging vector is still being read)
    int rc = d2h(c, terms_out, io + o_terms, (size_t)B * 2 * sizeof(double));
    if (rc == DRP_OK && margin_out) rc = d2h(c, margin_out, io + o_mar, (size_t)B * 2 * sizeof(double));
    if (rc == DRP_OK && grad_p_out) rc = d2h(c, grad_p_out, io + o_grad, bn * 3 * sizeof(double));
    if (rc == DRP_OK && nn_pq_out) rc = d2h(c, nn_pq_out, io + o_pq, bn * sizeof(int));
    if (rc == DRP_OK && nn_qp_out) rc = d2h(c, nn_qp_out, io + o_qp, bm * sizeof(int));
    const int rw = guarded_wait(c, nullptr);            // also on an error above: the staging vector goes out of scope
    return rc != DRP_OK ? rc : rw;
}
