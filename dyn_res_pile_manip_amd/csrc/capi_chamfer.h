// capi_chamfer.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the stand-alone Chamfer metric of two padded cloud batches (k_chamfer.h; the trainer's use of the kernel is capi_train.h's),
// and its float64 yardstick: one-shots on two clouds (capi_pipeline.h: cloud_check, cloud_begin, cloud_finish).

int drp_cloud_chamfer(drp_ctx* c, const float* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N, int M,
                      double* terms_out, float* grad_p_out, int32_t* nn_pq_out, int32_t* nn_qp_out) {
    CHK(cloud_check(c, p, n_p, q, n_q, B, N, M, terms_out, 0, KC_MAX_POINTS, ""));
    void* const outs[] = {terms_out, grad_p_out, nn_pq_out, nn_qp_out};
    CloudCall k;
    CHK(cloud_begin(c, k, chamfer_layout(B, N, M), outs, p, n_p, q, n_q, B, N, M));
    KcArgs a{};
    a.cp = k.cp; a.pred = k.p<float>(); a.scale = 1.0f;
    a.terms = k.out<double>(0); a.grad = k.out<float>(1); a.nn_pq = k.out<int>(2); a.nn_qp = k.out<int>(3);
    {
        ProbeScope ps(c, KC_LOSS);
        hipLaunchKernelGGL((kc_chamfer<false>), dim3(B, 1), dim3(KC_THREADS), 0, c->stream, a);
    }
    return cloud_finish(c, k, "kc_chamfer");
}

// drp_cloud_chamfer in float64 (k_chamfer_f64.h), with every direction's smallest arg-min margin: the same contract
int drp_cloud_chamfer_f64(drp_ctx* c, const float* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N, int M,
                          double* terms_out, double* grad_p_out, int32_t* nn_pq_out, int32_t* nn_qp_out, double* margin_out) {
    CHK(cloud_check(c, p, n_p, q, n_q, B, N, M, terms_out, 0, KC64_MAX_POINTS, ""));
    void* const outs[] = {terms_out, margin_out, grad_p_out, nn_pq_out, nn_qp_out};
    CloudCall k;
    CHK(cloud_begin(c, k, chamfer64_layout(B, N, M), outs, p, n_p, q, n_q, B, N, M));
    Kc64Args a{};
    a.cp = k.cp; a.p32 = k.p<float>(); a.b_off = 0; a.B = B; a.scale = 1.0;
    a.terms = k.out<double>(0); a.margin = k.out<double>(1); a.grad = k.out<double>(2); a.nn_pq = k.out<int>(3); a.nn_qp = k.out<int>(4);
    hipLaunchKernelGGL((kc64_chamfer<false>), dim3(B, 1), dim3(KC64_THREADS), 0, c->stream, a);
    return cloud_finish(c, k, "kc64_chamfer");
}
