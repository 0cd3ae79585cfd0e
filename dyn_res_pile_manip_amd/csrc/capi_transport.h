// capi_transport.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the stand-alone entropy-regularised transport distance of two padded cloud batches (k_sinkhorn.h), and the trainer's
// entry point for it (capi_train.h: train_step_body with the TR_LOSS_TRANSPORT kind, check_transport_params).

// A one-shot on two clouds (capi_pipeline.h: cloud_check, cloud_begin, cloud_finish; train_host.h: transport_layout)
int drp_cloud_transport(drp_ctx* c, const float* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N, int M,
                        const double* eps, int iters, double* terms_out, float* grad_p_out, double* dual_out, double* col_err_out) {
    CHK(cloud_check(c, p, n_p, q, n_q, B, N, M, terms_out, KT_MAX_POINTS, KT_MAX_POINTS, " for a transport"));
    CHK(check_transport_params(c, eps, B, iters));
    // the kernel ends after the same number of steps whatever it reads; a plan between points that are no numbers means nothing
    long bad = first_nonfinite_row(p, n_p, B, N);
    if (bad >= 0) return fail(c, DRP_EINVAL, "p[%ld][%ld] is not finite", bad / N, bad % N);
    bad = first_nonfinite_row(q, n_q, B, M);
    if (bad >= 0) return fail(c, DRP_EINVAL, "q[%ld][%ld] is not finite", bad / M, bad % M);
    void* const outs[] = {terms_out, grad_p_out, dual_out, col_err_out, nullptr};      // (the fifth block is eps: it only goes up)
    CloudCall k;
    CHK(cloud_begin(c, k, transport_layout(B, N, M), outs, p, n_p, q, n_q, B, N, M));
    double* const eps_dev = reinterpret_cast<double*>(k.io + k.lay.out[4]);
    HIPCHK(c, hipMemcpyAsync(eps_dev, eps, (size_t)B * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SkArgs32 a{};
    a.cp = k.cp; a.pred = k.p<float>(); a.b_off = 0; a.B = B; a.eps = eps_dev; a.iters = iters; a.scale = 1.0;
    a.terms = k.out<double>(0); a.grad = k.out<float>(1); a.dual = k.out<double>(2); a.col_err = k.out<double>(3);
    {
        ProbeScope ps(c, KC_LOSS);
        hipLaunchKernelGGL((kt_transport<false>), dim3(B, 1), dim3(KT_THREADS), 0, c->stream, a);
    }
    return cloud_finish(c, k, "kt_transport");
}

// drp_train_step_loss's body with the transport term: two more fields of TrLoss and the problems' col_err
int drp_train_step_transport(drp_ctx* c, const float* states, const float* states_delta, const float* actions, const float* attrs,
                             const int32_t* particle_nums, const float* particle_dens, int B, int N, const float* targets,
                             const int32_t* target_nums, int M, const double* eps, int iters, int mode, double* loss_out,
                             float* grad_out, double* col_err_out) {
    if (!c) return DRP_EINVAL;
    c->tr_grad_fresh = false; c->wgrad_tap_on = false;
    ImpulseSource src;
    CHK(impulse_source(c, states_delta, actions, src));
    const TrLoss lk = TrLoss::sinkhorn(TR_LOSS_TRANSPORT, targets, target_nums, M, eps, iters, col_err_out);
    return train_step_body(c, states, src.impulses, src.by_actions, attrs, particle_nums, particle_dens, B, N, lk,
                           mode, loss_out, grad_out);
}
