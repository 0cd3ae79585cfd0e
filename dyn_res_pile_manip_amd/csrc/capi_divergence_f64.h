// capi_divergence_f64.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the float64 yardstick of the Sinkhorn divergence (k_sinkhorn.h: kd64_*) -- the one-shot on two clouds, and the trainer's
// float64 gradients with the divergence as the seed of the reverse pass (capi_grad_f64.h: train_grad_f64_body with the
// TR_LOSS_DIVERGENCE kind).

// drp_cloud_divergence's contract with p as doubles: the instantiation the trainer's yardstick runs, through the one body of
// capi_divergence.h (cloud_divergence_body<double>) and the one-shots' buffer in divergence_layout's blocks with 8-byte elements
int drp_cloud_divergence_f64(drp_ctx* c, const double* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N, int M,
                             const double* eps, int iters, double* terms_out, double* grad_p_out, double* dual_out,
                             double* col_err_out, double* self_err_out) {
    return cloud_divergence_body(c, p, n_p, q, n_q, B, N, M, eps, false, nullptr, nullptr, iters, terms_out, grad_p_out, dual_out,
                                     col_err_out, self_err_out, nullptr);
}

// drp_cloud_divergence_unbalanced's contract with p as doubles: the checks are drp_cloud_divergence_f64's, in its order, then the
// two new arrays' (capi_train.h: check_reach_params)
int drp_cloud_divergence_unbalanced_f64(drp_ctx* c, const double* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N,
                                        int M, const double* eps, const double* rho, const double* mass_q, int iters, double* terms_out,
                                        double* grad_p_out, double* dual_out, double* col_err_out, double* self_err_out,
                                        double* transported_out) {
    return cloud_divergence_body(c, p, n_p, q, n_q, B, N, M, eps, true, rho, mass_q, iters, terms_out, grad_p_out, dual_out,
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
