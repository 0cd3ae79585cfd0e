// capi_match.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the stand-alone one-to-one matching distance of two padded cloud batches (k_match.h; the trainer's use of the kernel is
// capi_train.h's).

// A one-shot on two clouds (capi_pipeline.h: cloud_check, cloud_begin, cloud_finish; train_host.h: cm_layout)
int drp_cloud_match(drp_ctx* c, const float* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N, int M,
                    double* terms_out, float* grad_p_out, int32_t* match_pq_out, int32_t* match_qp_out, double* dual_out) {
    CHK(cloud_check(c, p, n_p, q, n_q, B, N, M, terms_out, KA_MAX_POINTS, KA_MAX_POINTS, " for a matching"));
    // the kernel ends after the same number of steps whatever it reads; a matching of points that are no numbers means nothing
    long bad = first_nonfinite_row(p, n_p, B, N);
    if (bad >= 0) return fail(c, DRP_EINVAL, "p[%ld][%ld] is not finite", bad / N, bad % N);
    bad = first_nonfinite_row(q, n_q, B, M);
    if (bad >= 0) return fail(c, DRP_EINVAL, "q[%ld][%ld] is not finite", bad / M, bad % M);
    void* const outs[] = {terms_out, grad_p_out, match_pq_out, match_qp_out, dual_out};
    CloudCall k;
    CHK(cloud_begin(c, k, cm_layout(B, N, M), outs, p, n_p, q, n_q, B, N, M));
    KaArgs a{};
    a.cp = k.cp; a.pred = k.p<float>(); a.scale = 1.0; a.keep = 0.0;
    a.terms = k.out<double>(0); a.grad = k.out<float>(1); a.match_pq = k.out<int>(2); a.match_qp = k.out<int>(3); a.dual = k.out<double>(4);
    {
        ProbeScope ps(c, KC_LOSS);
        ka_launch<false>(dim3(B, 1), c->stream, a);
    }
    return cloud_finish(c, k, "ka_match");
}
