// capi_divergence.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the stand-alone Sinkhorn divergence of two padded cloud batches (k_sinkhorn.h), and the trainer's entry point for it
// (capi_train.h: train_step_body with the TR_LOSS_DIVERGENCE kind, check_transport_params).

// A one-shot on two clouds (capi_pipeline.h: cloud_check, cloud_begin, cloud_finish; train_host.h: divergence_layout), ONE body
// behind the four of them so that they cannot drift apart.  T: p's and the gradient's scalar -- float: drp_cloud_divergence and
// drp_cloud_divergence_unbalanced; double: their float64 yardsticks (capi_divergence_f64.h).  `reach`: rho, mass_q and
// transported_out are read, and the second instantiation of the kernels runs (k_sinkhorn.h: UNBAL)
namespace {
extern "C++" template <typename T>
int cloud_divergence_body(drp_ctx* c, const T* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N, int M,
                          const double* eps, bool reach, const double* rho, const double* mass_q, int iters, double* terms_out,
                          T* grad_p_out, double* dual_out, double* col_err_out, double* self_err_out, double* transported_out) {
    constexpr bool f64 = sizeof(T) == sizeof(double);
    CHK(cloud_check(c, p, n_p, q, n_q, B, N, M, terms_out, KT_MAX_POINTS, KT_MAX_POINTS, " for a divergence"));
    CHK(check_transport_params(c, eps, B, iters));
    if (reach) CHK(check_reach_params(c, eps, rho, mass_q, B, 1));
    // as drp_cloud_transport: the kernels end after the same number of steps whatever they read
    long bad = first_nonfinite_row(p, n_p, B, N);
    if (bad >= 0) return fail(c, DRP_EINVAL, "p[%ld][%ld] is not finite", bad / N, bad % N);
    bad = first_nonfinite_row(q, n_q, B, M);
    if (bad >= 0) return fail(c, DRP_EINVAL, "q[%ld][%ld] is not finite", bad / M, bad % M);
    void* const outs[] = {terms_out, grad_p_out, dual_out, col_err_out, self_err_out};
    const DivLayout lay = divergence_layout(B, N, M, reach, sizeof(T));
    CloudCall k;
    CHK(cloud_begin(c, k, lay.cloud, outs, p, n_p, q, n_q, B, N, M));
    // eps alone goes up from the caller's array; eps | rho | mass_q lie side by side: one staging vector, one copy (read until
    // cloud_finish's wait)
    std::vector<double> up;
    if (reach) {
        up.insert(up.end(), eps, eps + B);
        up.insert(up.end(), rho, rho + B);
        up.insert(up.end(), mass_q, mass_q + B);
    }
    const size_t n_up = reach ? up.size() : (size_t)B;
    if (hipMemcpyAsync(k.io + lay.eps, reach ? up.data() : eps, n_up * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        (void)drp_sync(c);                                  // (cloud_begin's staging vector is still being read)
        return fail(c, DRP_EHIP, reach ? "hipMemcpyAsync of eps, rho and mass_q" : "hipMemcpyAsync of eps");
    }
    SkArgs<T, T> a{};
    a.cp = k.cp; a.pred = k.p<T>(); a.b_off = 0; a.B = B;
    a.eps = reinterpret_cast<double*>(k.io + lay.eps); a.iters = iters; a.scale = 1.0;
    a.vals = reinterpret_cast<double*>(k.io + lay.vals);
    a.grad = k.out<T>(1);
    a.gsum = a.grad != nullptr ? reinterpret_cast<double*>(k.io + lay.gsum) : nullptr;
    a.terms = k.out<double>(0); a.dual = k.out<double>(2); a.col_err = k.out<double>(3); a.self_err = k.out<double>(4);
    const bool moved = reach && transported_out != nullptr;
    if (reach) {
        a.rho = reinterpret_cast<double*>(k.io + lay.rho); a.mass_q = reinterpret_cast<double*>(k.io + lay.mass_q);
        a.transported = moved ? reinterpret_cast<double*>(k.io + lay.transported) : nullptr;
    }
    const dim3 sweeps(B, 1, 3), combine(B, 1);
    {
        ProbeScope ps(c, KC_LOSS);
        if constexpr (f64) {
            if (reach) {
                hipLaunchKernelGGL(kd64_sweeps_unbalanced, sweeps, dim3(KT_THREADS), 0, c->stream, a);
                hipLaunchKernelGGL(kd64_combine_unbalanced, combine, dim3(KD_COMBINE_THREADS), 0, c->stream, a);
            } else {
                hipLaunchKernelGGL(kd64_sweeps, sweeps, dim3(KT_THREADS), 0, c->stream, a);
                hipLaunchKernelGGL(kd64_combine, combine, dim3(KD_COMBINE_THREADS), 0, c->stream, a);
            }
        } else {
            if (reach) {
                hipLaunchKernelGGL(kd_sweeps_unbalanced, sweeps, dim3(KT_THREADS), 0, c->stream, a);
                hipLaunchKernelGGL((kd_combine<false, true>), combine, dim3(KD_COMBINE_THREADS), 0, c->stream, a);
            } else {
                hipLaunchKernelGGL(kd_sweeps, sweeps, dim3(KT_THREADS), 0, c->stream, a);
                hipLaunchKernelGGL((kd_combine<false>), combine, dim3(KD_COMBINE_THREADS), 0, c->stream, a);
            }
        }
    }
    const int rc = moved ? d2h(c, transported_out, k.io + lay.transported, (size_t)B * sizeof(double)) : DRP_OK;
    const int rf = cloud_finish(c, k, f64 ? "kd64_sweeps" : reach ? "kd_sweeps_unbalanced" : "kd_sweeps");     // the wait, also behind an error above
    return rc != DRP_OK ? rc : rf;
}
}  // namespace

int drp_cloud_divergence(drp_ctx* c, const float* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N, int M,
                         const double* eps, int iters, double* terms_out, float* grad_p_out, double* dual_out, double* col_err_out,
                         double* self_err_out) {
    return cloud_divergence_body(c, p, n_p, q, n_q, B, N, M, eps, false, nullptr, nullptr, iters, terms_out, grad_p_out, dual_out,
                                 col_err_out, self_err_out, nullptr);
}

// The checks are drp_cloud_divergence's, in its order, then the two new arrays' (capi_train.h: check_reach_params)
int drp_cloud_divergence_unbalanced(drp_ctx* c, const float* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N, int M,
                                    const double* eps, const double* rho, const double* mass_q, int iters, double* terms_out,
                                    float* grad_p_out, double* dual_out, double* col_err_out, double* self_err_out,
                                    double* transported_out) {
    return cloud_divergence_body(c, p, n_p, q, n_q, B, N, M, eps, true, rho, mass_q, iters, terms_out, grad_p_out, dual_out, col_err_out,
                                 self_err_out, transported_out);
}

// drp_train_step_divergence with the reaches and the targets' masses in TrLoss: train_step_body launches the unbalanced kernels
int drp_train_step_divergence_unbalanced(drp_ctx* c, const float* states, const float* states_delta, const float* actions,
                                         const float* attrs, const int32_t* particle_nums, const float* particle_dens, int B, int N,
                                         const float* targets, const int32_t* target_nums, int M, const double* eps, const double* rho,
                                         const double* mass_q, int iters, int mode, double* loss_out, float* grad_out,
                                         double* col_err_out, double* self_err_out, double* transported_out) {
    if (!c) return DRP_EINVAL;
    c->tr_grad_fresh = false; c->wgrad_tap_on = false;
    ImpulseSource src;
    CHK(impulse_source(c, states_delta, actions, src));
    if (!rho || !mass_q) return fail(c, DRP_EINVAL, "null argument");
    TrLoss lk = TrLoss::sinkhorn(TR_LOSS_DIVERGENCE, targets, target_nums, M, eps, iters, col_err_out, self_err_out);
    lk.rho = rho; lk.mass_q = mass_q; lk.transported_out = transported_out;
    return train_step_body(c, states, src.impulses, src.by_actions, attrs, particle_nums, particle_dens, B, N, lk,
                           mode, loss_out, grad_out);
}

// drp_train_step_transport's body with the divergence as each step's term: one more certificate
int drp_train_step_divergence(drp_ctx* c, const float* states, const float* states_delta, const float* actions, const float* attrs,
                              const int32_t* particle_nums, const float* particle_dens, int B, int N, const float* targets,
                              const int32_t* target_nums, int M, const double* eps, int iters, int mode, double* loss_out,
                              float* grad_out, double* col_err_out, double* self_err_out) {
    if (!c) return DRP_EINVAL;
    c->tr_grad_fresh = false; c->wgrad_tap_on = false;
    ImpulseSource src;
    CHK(impulse_source(c, states_delta, actions, src));
    TrLoss lk = TrLoss::sinkhorn(TR_LOSS_DIVERGENCE, targets, target_nums, M, eps, iters, col_err_out, self_err_out);
    return train_step_body(c, states, src.impulses, src.by_actions, attrs, particle_nums, particle_dens, B, N, lk,
                           mode, loss_out, grad_out);
}
