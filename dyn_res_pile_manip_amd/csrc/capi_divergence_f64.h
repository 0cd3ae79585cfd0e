// capi_divergence_f64.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the float64 yardstick of the Sinkhorn divergence (k_divergence_f64.h) -- the one-shot on two clouds, and the trainer's
// float64 gradients with the divergence as the seed of the reverse pass (capi_grad_f64.h: train_grad_f64_body with the
// TR_LOSS_DIVERGENCE kind).

// drp_cloud_divergence's contract with p as doubles: the instantiation the trainer's yardstick runs.  The buffer is the one-shots'
// (c->cloud_io) in a layout of its own (train_host.h: divergence64_layout): p does not fit cloud_begin's floats
// drp_cloud_divergence_unbalanced_f64 (`reach`: rho, mass_q and transported_out are read) is the same call with the second
// instantiation of the kernels: one body, so that the two cannot drift apart
namespace {
int cloud_divergence_f64_body(drp_ctx* c, const double* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N, int M,
                              const double* eps, bool reach, const double* rho, const double* mass_q, int iters, double* terms_out,
                              double* grad_p_out, double* dual_out, double* col_err_out, double* self_err_out, double* transported_out) {
    CHK(cloud_check(c, p, n_p, q, n_q, B, N, M, terms_out, KT_MAX_POINTS, KT_MAX_POINTS, " for a divergence"));
    CHK(check_transport_params(c, eps, B, iters));
    if (reach) CHK(check_reach_params(c, eps, rho, mass_q, B, 1));
    long bad = first_nonfinite_row(p, n_p, B, N);
    if (bad >= 0) return fail(c, DRP_EINVAL, "p[%ld][%ld] is not finite", bad / N, bad % N);
    bad = first_nonfinite_row(q, n_q, B, M);
    if (bad >= 0) return fail(c, DRP_EINVAL, "q[%ld][%ld] is not finite", bad / M, bad % M);
    HIPCHK(c, hipSetDevice(c->device));
    const Div64Layout lay = divergence64_layout(B, N, M, reach);
    CHK(ensure(c, c->cloud_io, lay.bytes));
    std::vector<char> stage(lay.in_bytes);              // read until the wait below
    memcpy(stage.data() + lay.pts_p, p, (size_t)B * N * 3 * sizeof(double));
    memcpy(stage.data() + lay.eps, eps, (size_t)B * sizeof(double));
    if (reach) {
        memcpy(stage.data() + lay.rho, rho, (size_t)B * sizeof(double));
        memcpy(stage.data() + lay.mass_q, mass_q, (size_t)B * sizeof(double));
    }
    memcpy(stage.data() + lay.pts_q, q, (size_t)B * M * 3 * sizeof(float));
    memcpy(stage.data() + lay.n_p, n_p, (size_t)B * sizeof(int32_t));
    memcpy(stage.data() + lay.n_q, n_q, (size_t)B * sizeof(int32_t));
    CHK(h2d(c, c->cloud_io, stage.data(), lay.in_bytes));
    char* const io = ptr<char>(c->cloud_io);
    void* const outs[5] = {terms_out, grad_p_out, dual_out, col_err_out, self_err_out};
    auto out = [&](int k) { return outs[k] ? reinterpret_cast<double*>(io + lay.out[k]) : (double*)nullptr; };
    Kd64Args a{};
    a.pred = reinterpret_cast<const double*>(io + lay.pts_p);
    a.cp.p_bstride = (size_t)N * 3; a.cp.p_tstride = 0;
    a.cp.q = reinterpret_cast<const float*>(io + lay.pts_q); a.cp.q_bstride = (size_t)M * 3; a.cp.q_tstride = 0;
    a.cp.n_p = reinterpret_cast<const int*>(io + lay.n_p);
    a.cp.n_q = reinterpret_cast<const int*>(io + lay.n_q); a.cp.nq_bstride = 1; a.cp.nq_tstride = 0;
    a.cp.N = N; a.cp.M = M;
    a.b_off = 0; a.B = B;
    a.eps = reinterpret_cast<const double*>(io + lay.eps); a.iters = iters; a.scale = 1.0;
    a.vals = reinterpret_cast<double*>(io + lay.vals);
    a.grad = out(1);
    a.gsum = a.grad != nullptr ? reinterpret_cast<double*>(io + lay.gsum) : nullptr;
    a.terms = out(0); a.dual = out(2); a.col_err = out(3); a.self_err = out(4);
    if (reach) {
        a.rho = reinterpret_cast<const double*>(io + lay.rho);
        a.mass_q = reinterpret_cast<const double*>(io + lay.mass_q);
        a.transported = transported_out != nullptr ? reinterpret_cast<double*>(io + lay.transported) : nullptr;
    }
    {
        ProbeScope ps(c, KC_LOSS);
        if (reach) {
            hipLaunchKernelGGL(kd64_sweeps_unbalanced, dim3(B, 1, 3), dim3(KT_THREADS), 0, c->stream, a);
            hipLaunchKernelGGL(kd64_combine_unbalanced, dim3(B, 1), dim3(KD_COMBINE_THREADS), 0, c->stream, a);
        } else {
            hipLaunchKernelGGL(kd64_sweeps, dim3(B, 1, 3), dim3(KT_THREADS), 0, c->stream, a);
            hipLaunchKernelGGL(kd64_combine, dim3(B, 1), dim3(KD_COMBINE_THREADS), 0, c->stream, a);
        }
    }
    if (hipGetLastError() != hipSuccess) { (void)drp_sync(c); return fail(c, DRP_EHIP, "kd64_sweeps launch"); }   // (the staging vector is still being read)
    int rc = DRP_OK;
    for (int k = 0; k < 5; ++k)
        if (rc == DRP_OK && outs[k]) rc = d2h(c, outs[k], io + lay.out[k], lay.out_bytes[k]);
    if (rc == DRP_OK && reach && transported_out) rc = d2h(c, transported_out, io + lay.transported, (size_t)B * sizeof(double));
    const int rw = guarded_wait(c, nullptr);            // also on an error above: the staging vector goes out of scope
    return rc != DRP_OK ? rc : rw;
}
}  // namespace

int drp_cloud_divergence_f64(drp_ctx* c, const double* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N, int M,
                             const double* eps, int iters, double* terms_out, double* grad_p_out, double* dual_out,
                             double* col_err_out, double* self_err_out) {
    return cloud_divergence_f64_body(c, p, n_p, q, n_q, B, N, M, eps, false, nullptr, nullptr, iters, terms_out, grad_p_out, dual_out,
                                     col_err_out, self_err_out, nullptr);
}

// drp_cloud_divergence_unbalanced's contract with p as doubles: the checks are drp_cloud_divergence_f64's, in its order, then the
// two new arrays' (capi_train.h: check_reach_params)
int drp_cloud_divergence_unbalanced_f64(drp_ctx* c, const double* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N,
                                        int M, const double* eps, const double* rho, const double* mass_q, int iters, double* terms_out,
                                        double* grad_p_out, double* dual_out, double* col_err_out, double* self_err_out,
                                        double* transported_out) {
    return cloud_divergence_f64_body(c, p, n_p, q, n_q, B, N, M, eps, true, rho, mass_q, iters, terms_out, grad_p_out, dual_out,
                                     col_err_out, self_err_out, transported_out);
}

// drp_train_grad_f64_untracked's body with the divergence as each step's term: the one-shot contract of that call
int drp_train_grad_f64_divergence(drp_ctx* c, const float* states, const float* states_delta, const float* actions,
                                  const float* attrs, const int32_t* particle_nums, const float* particle_dens, int B, int N,
                                  int n_rollout, const float* targets, const int32_t* target_nums, int M, const double* eps, int iters,
                                  double* loss_out, double* loss_terms_out, double* grad_out, double* grad_state_out,
                                  double* col_err_out, double* self_err_out) {
    if (!c) return DRP_EINVAL;
    ImpulseSource src;
    CHK(impulse_source(c, states_delta, actions, src));
    TrLoss lk = TrLoss::sinkhorn(TR_LOSS_DIVERGENCE, targets, target_nums, M, eps, iters, col_err_out, self_err_out);
    return train_grad_f64_body(c, states, src.impulses, src.by_actions, attrs, particle_nums,
                               particle_dens, B, N, n_rollout, lk, loss_out, loss_terms_out, grad_out, grad_state_out);
}

// drp_train_grad_f64_divergence with the reaches and the targets' masses in TrLoss: tr64_chunk launches the unbalanced kernels
int drp_train_grad_f64_divergence_unbalanced(drp_ctx* c, const float* states, const float* states_delta, const float* actions,
                                             const float* attrs, const int32_t* particle_nums, const float* particle_dens, int B, int N,
                                             int n_rollout, const float* targets, const int32_t* target_nums, int M, const double* eps,
                                             const double* rho, const double* mass_q, int iters, double* loss_out, double* loss_terms_out,
                                             double* grad_out, double* grad_state_out, double* col_err_out, double* self_err_out,
                                             double* transported_out) {
    if (!c) return DRP_EINVAL;
    ImpulseSource src;
    CHK(impulse_source(c, states_delta, actions, src));
    if (!rho || !mass_q) return fail(c, DRP_EINVAL, "null argument");
    TrLoss lk = TrLoss::sinkhorn(TR_LOSS_DIVERGENCE, targets, target_nums, M, eps, iters, col_err_out, self_err_out);
    lk.rho = rho; lk.mass_q = mass_q; lk.transported_out = transported_out;
    return train_grad_f64_body(c, states, src.impulses, src.by_actions, attrs, particle_nums,
                               particle_dens, B, N, n_rollout, lk, loss_out, loss_terms_out, grad_out, grad_state_out);
}
