// capi_optim.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the trainer's optimiser seam behind DRP_TRAIN_GRAD (k_optim.h): several passes' gradients summed in float64 on the
// device, one Adam step on the scaled and clipped sum, and Adam's state in and out.  drp_train_begin allocates (capi_train.h:
// optim_begin); the "fresh gradient" mark is set by train_step_body and cleared by everything that writes tr_grad.

// acc += weight x the gradient the last DRP_TRAIN_GRAD pass left in tr_grad: one launch, no copy and no wait of its own (the
// pass has waited already; whatever comes next on the context's stream waits behind this launch)
int drp_train_accumulate(drp_ctx* c, double weight) {
    if (!c || !c->tr_on) return fail(c, DRP_ESTATE, "drp_train_begin not called");
    if (!std::isfinite(weight) || !(weight > 0.0)) return fail(c, DRP_EINVAL, "weight=%g is not a positive finite number", weight);
    if (!c->tr_grad_fresh)
        return fail(c, DRP_ESTATE, "no fresh gradient: the last trainer call must be a DRP_TRAIN_GRAD pass that returned DRP_OK, "
                                   "and a pass is accumulated once");
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(ko_accumulate, dim3(KO_BLOCKS((int)W_TOTAL)), dim3(KO_THREADS), 0, c->stream, ptr<double>(c->tr_acc),
                       ptr<const float>(c->tr_grad), (int)W_TOTAL, weight);
    HIPCHK(c, hipGetLastError());
    c->tr_grad_fresh = false;
    c->tr_acc_n += 1;
    return DRP_OK;
}

// norm -> clip -> scale -> Adam -> re-pack in one chain of launches and ONE host wait: the norm never comes to the host between
// the reduction and the Adam launch (ko_norm_final leaves it where ko_adam_scaled reads it, and in opt_pin for the caller).  The
// bias corrections, the w_pin copy and the re-pack are train_attempt's; the accumulator is cleared by ko_adam_scaled itself
int drp_train_apply(drp_ctx* c, double scale, double max_norm, double* norm_out, double* clip_out, int* applied_out, float* grad_out) {
    if (!c || !c->tr_on) return fail(c, DRP_ESTATE, "drp_train_begin not called");
    if (!std::isfinite(scale) || !(scale > 0.0)) return fail(c, DRP_EINVAL, "scale=%g is not a positive finite number", scale);
    if (!(max_norm > 0.0)) return fail(c, DRP_EINVAL, "max_norm=%g is not a positive number (+inf: no clipping)", max_norm);
    if (c->tr_acc_n == 0) return fail(c, DRP_ESTATE, "nothing accumulated since the last drp_train_apply / drp_train_begin");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->repack_device) CHK(ensure_repack_maps(c));       // (allocates w_pin; waits the first time only)
    const int n = (int)W_TOTAL, n_part = KO_BLOCKS(n);
    double* const part = ptr<double>(c->tr_opt);
    KoStep* const step_dev = reinterpret_cast<KoStep*>(part + n_part);
    KoStep* const step_host = ptr<KoStep>(c->opt_pin);
    c->tr_grad_fresh = false;
    c->tr_acc_n = 0;
    DrainOnError drain(c);
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(ko_norm_partial, dim3(n_part), dim3(KO_THREADS), 0, st, ptr<const double>(c->tr_acc), n, scale, part);
    hipLaunchKernelGGL(ko_norm_final, dim3(1), dim3(KO_THREADS), 0, st, (const double*)part, n_part, scale, max_norm, step_dev, step_host);
    const long iter = c->tr_iter + 1;
    const double bc1 = 1.0 - pow(c->tr_beta1, (double)iter), bc2 = 1.0 - pow(0.999, (double)iter);
    const float inf = __builtin_inff();
    hipLaunchKernelGGL(ko_adam_scaled, dim3(n_part), dim3(KO_THREADS), 0, st, ptr<float>(c->w_raw), ptr<double>(c->tr_acc),
                       ptr<float>(c->tr_m), ptr<float>(c->tr_v), n, (float)(c->tr_lr / bc1), (float)sqrt(bc2), (float)c->tr_beta1,
                       -inf, inf, (const KoStep*)step_dev, ptr<float>(c->tr_g32),
                       c->repack_device ? ptr<float>(c->w_pin) : (float*)nullptr);
    if (hipGetLastError() != hipSuccess) return fail(c, DRP_EHIP, "drp_train_apply: kernel launch");
    c->f64_w_valid = false;               // as after drp_train_step's update: the next *_f64 call widens the blob again
    if (grad_out) CHK(d2h(c, grad_out, c->tr_g32.p, (size_t)n * sizeof(float)));
    // the engines read packed copies of the weights: rebuilt from the blob on the device (the same bits if nothing moved)
    if (c->repack_device) CHK(repack_on_device(c, true));
    CHK(drp_sync(c));
    const bool applied = step_host->skip == 0u;
    if (applied) {
        if (c->repack_device) {
            CHK(finish_repack(c));
        } else {                          // DRP_NO_REPACK_DEVICE=1: the blob comes back and the host packers run
            std::vector<float> blob((size_t)n);
            CHK(d2h(c, blob.data(), c->w_raw.p, (size_t)n * sizeof(float)));
            CHK(guarded_wait(c, nullptr));
            CHK(install_weights(c, blob));
        }
        c->tr_iter += 1;
        end_sessions(c);                  // as every update: a planner session would go on with constants of the old weights
    }
    if (norm_out) *norm_out = step_host->norm;
    if (clip_out) *clip_out = step_host->clip;
    if (applied_out) *applied_out = applied ? 1 : 0;
    return drain.ok();
}

// Adam's moments in drp_get_weights' layout and the steps taken; the accumulator is no part of the state
int drp_train_get_state(drp_ctx* c, float* m_out, float* v_out, int64_t* iter_out) {
    if (!c || !c->tr_on) return fail(c, DRP_ESTATE, "drp_train_begin not called");
    if (!m_out || !v_out || !iter_out) return fail(c, DRP_EINVAL, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(d2h(c, m_out, c->tr_m.p, (size_t)W_TOTAL * sizeof(float)));
    CHK(d2h(c, v_out, c->tr_v.p, (size_t)W_TOTAL * sizeof(float)));
    CHK(guarded_wait(c, nullptr));
    *iter_out = (int64_t)c->tr_iter;
    return DRP_OK;
}

int drp_train_set_state(drp_ctx* c, const float* m, const float* v, int64_t iter) {
    if (!c || !c->tr_on) return fail(c, DRP_ESTATE, "drp_train_begin not called");
    if (!m || !v) return fail(c, DRP_EINVAL, "null argument");
    if (iter < 0 || iter > (int64_t)0x7fffffff) return fail(c, DRP_EINVAL, "iter=%lld outside 0..2^31-1", (long long)iter);
    for (int i = 0; i < (int)W_TOTAL; ++i) {
        if (!std::isfinite(m[i])) return fail(c, DRP_EINVAL, "m[%d]=%g is not finite", i, (double)m[i]);
        if (!std::isfinite(v[i]) || v[i] < 0.0f) return fail(c, DRP_EINVAL, "v[%d]=%g is not a finite number >= 0", i, (double)v[i]);
    }
    HIPCHK(c, hipSetDevice(c->device));
    CHK(h2d(c, c->tr_m, m, (size_t)W_TOTAL * sizeof(float)));
    CHK(h2d(c, c->tr_v, v, (size_t)W_TOTAL * sizeof(float)));
    CHK(guarded_wait(c, nullptr));          // the caller's arrays are free again
    c->tr_iter = (int)iter;
    return DRP_OK;
}
