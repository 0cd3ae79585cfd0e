// capi_train_f64.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the training loop body in float64 (drp_train_grad_f64; kernels: k_prop_f64.h forward, k_gd_f64.h backward, k_train_f64.h
// loss and weight gradients), the yardstick of drp_train_step's gradients (row y3).  Like the other *_f64 calls it is no engine
// and no session: it works in buffers of its own under F64Scope, needs no drp_train_begin and leaves the context -- the
// trainer's Adam state included -- as it found it.

namespace {

// a chunk's workspace, carved from one allocation: base == nullptr only measures
struct Tr64Ws {
    // the tape: a step's intermediates (k_prop_f64.h: KF_BYTES_PER_PARTICLE), states, impulses and lists
    double *pe, *re, *eff, *agg, *erel, *pred;          // [H] blocks each
    double *state, *sd;                                 // [H+1][pn,3], [H][pn,3]
    int16_t* idx; uint8_t* cnt;                         // [H][pn,10], [H][pn]
    // the reverse pass of one step
    double *g_eff, *g_pre, *g_agg, *g_pe, *g_re, *gr, *gs, *g_sd, *g_diff, *g_state;
    int *rev_off, *rev;
    // what the backward kernels leave for the weight gradients: hidden layers, their masked gradients, the narrow inputs
    double *pr_h, *pr_gh, *pe_h, *pe_gh, *pe_in, *re_h1, *re_h2, *re_g1, *re_g2, *re_in;
    double* acc;                                        // [bc][W_TOTAL]: a sample's gradient
    size_t bytes;
};
Tr64Ws tr64_carve(void* base, size_t bc, size_t N, size_t H) {
    Tr64Ws w{};
    size_t off = 0;
    auto take = [&](auto*& p, size_t n) {
        typedef typename std::remove_reference<decltype(*p)>::type T;
        p = base ? reinterpret_cast<T*>(static_cast<char*>(base) + off) : nullptr;
        off += (n * sizeof(T) + 255) & ~(size_t)255;
    };
    const size_t pn = bc * N, en = pn * DRP_K;
    take(w.pe, H * pn * 64); take(w.re, H * en * 64); take(w.eff, H * pn * 3 * 64); take(w.agg, H * pn * 3 * 64);
    take(w.erel, H * en * 3 * 64); take(w.pred, H * pn * 3);
    take(w.state, (H + 1) * pn * 3); take(w.sd, H * pn * 3); take(w.idx, H * en); take(w.cnt, H * pn);
    take(w.g_eff, pn * 64); take(w.g_pre, pn * 64); take(w.g_agg, pn * 64); take(w.g_pe, pn * 64);
    take(w.g_re, en * 64); take(w.gr, en * 64); take(w.gs, en * 64);
    take(w.g_sd, pn * 3); take(w.g_diff, en * 3); take(w.g_state, H * pn * 3);
    take(w.rev_off, bc * (N + 1)); take(w.rev, en);
    take(w.pr_h, pn * 64); take(w.pr_gh, pn * 64); take(w.pe_h, pn * 64); take(w.pe_gh, pn * 64); take(w.pe_in, pn * 5);
    take(w.re_h1, en * 64); take(w.re_h2, en * 64); take(w.re_g1, en * 64); take(w.re_g2, en * 64); take(w.re_in, en * 6);
    take(w.acc, bc * (size_t)W_TOTAL);
    w.bytes = off;
    return w;
}

// the batch on the device: the caller's arrays, a_cur = attrs[:, 0] gathered, then the results
struct Tr64Io {
    const float *states, *sdelta, *attr, *dens;
    const int* nums;
    double *terms, *total;          // [H][B], [W_TOTAL]
};

// forward with tape, loss, reverse pass with weight gradients of the samples [b0, b0 + bc): launches and the state gradient's copy
int tr64_chunk(drp_ctx* c, const Tr64Ws& k, const Tr64Io& io, int b0, int bc, int N, int B, int H, double* grad_state_out) {
    hipStream_t st = c->stream;
    const double* w = ptr<double>(c->f64_w);
    const int rows = bc * N, erows = rows * DRP_K, R_e = N * DRP_K;
    const size_t pn = (size_t)rows, en = (size_t)erows;
    const dim3 tblk(64 * KG_WAVES);
    const dim3 pgrid((rows + 16 * KG_WAVES - 1) / (16 * KG_WAVES)), egrid((erows + 16 * KG_WAVES - 1) / (16 * KG_WAVES));
    const dim3 lin3((unsigned)((pn * 3 + 255) / 256));
    const float* attr = io.attr + (size_t)b0 * N;
    const float* dens = io.dens + b0;
    hipLaunchKernelGGL(kt64_init_state, lin3, dim3(256), 0, st, io.states, b0, N, H, (long)(pn * 3), k.state);
    // ---- forward: the impulse is data; the lists from the fp32 graph build (the trainer's padded mode) on the roundings
    for (int t = 0; t < H; ++t) {
        const double* s_t = k.state + (size_t)t * pn * 3;
        double* sd_t = k.sd + (size_t)t * pn * 3;
        int16_t* idx = k.idx + (size_t)t * en;
        uint8_t* cnt = k.cnt + (size_t)t * pn;
        hipLaunchKernelGGL(kt64_stage_step, lin3, dim3(256), 0, st, s_t, io.sdelta, b0, N, H, t, (long)(pn * 3), sd_t, ptr<float>(c->s_in),
                           ptr<float>(c->s_delta));
        const GraphPlan g = plan_graph(c->pol, c->n_cu, c->engine, bc, N, true, false, false, true);
        launch_graph(c, st, g, ptr<float>(c->s_in), bc, (size_t)N * 3, (const float*)nullptr, (size_t)0, ptr<float>(c->s_delta), bc, N,
                     idx, cnt, 0);
        f64_launch_step<double>(c, w, s_t, sd_t, attr, dens, idx, cnt, N, rows, k.pe + (size_t)t * pn * 64, k.re + (size_t)t * en * 64,
                                k.eff + (size_t)t * pn * 3 * 64, k.agg + (size_t)t * pn * 3 * 64, k.erel + (size_t)t * en * 3 * 64,
                                k.pred + (size_t)t * pn * 3, k.state + (size_t)(t + 1) * pn * 3);
        HIPCHK(c, hipGetLastError());
    }
    // ---- every step's loss term and its seed of the reverse pass; the samples' accumulators start at zero
    hipLaunchKernelGGL(kt64_mse, dim3(bc, H), dim3(256), 0, st, k.state, io.states, io.nums, b0, bc, B, N, H, io.terms, k.g_state);
    HIPCHK(c, hipMemsetAsync(k.acc, 0, (size_t)bc * W_TOTAL * sizeof(double), st));
    // a layer's weight gradient: its 64-wide blocks on the matrix instruction, bias and density column as chains
    auto job = [&](const double* g, const double* m, int g_div, int R, int b_off, int d_off, int ld) {
        Kt64Job j{};
        j.g = g; j.m = m; j.g_div = g_div; j.N = N; j.R = R; j.ld = ld; j.b_off = b_off; j.d_off = d_off;
        return j;
    };
    auto block = [&](Kt64Job j, const double* x, int x_mode, int w_off, const int16_t* idx, const uint8_t* cnt) {
        j.x = x; j.x_mode = x_mode; j.w_off = w_off; j.idx = idx; j.cnt = cnt;
        hipLaunchKernelGGL(kt64_wgrad64, dim3(4, bc), dim3(256), 0, st, j, k.acc);
    };
    auto bias = [&](const Kt64Job& j) { hipLaunchKernelGGL(kt64_wgrad_bias, dim3(bc), dim3(128), 0, st, j, dens, k.acc); };
    auto narrow = [&](const double* G, int gw, const double* X, int xw, int R, int w_off, int b_off) {
        hipLaunchKernelGGL(kt64_wgrad_narrow, dim3((unsigned)((gw * (xw + 1) + 255) / 256), bc), dim3(256), 0, st, G, gw, X, xw, R, w_off,
                           b_off, k.acc);
    };
    // ---- reverse pass, step by step (the kernels of capi_gd_f64.h; the state gradient is seeded by the loss, the impulse is data)
    for (int t = H - 1; t >= 0; --t) {
        const double* s_t = k.state + (size_t)t * pn * 3;
        const double* g_out = k.g_state + (size_t)t * pn * 3;
        const int16_t* idx = k.idx + (size_t)t * en;
        const uint8_t* cnt = k.cnt + (size_t)t * pn;
        const double* pe = k.pe + (size_t)t * pn * 64;
        const double* re = k.re + (size_t)t * en * 64;
        const double* eff = k.eff + (size_t)t * pn * 3 * 64;
        const double* agg = k.agg + (size_t)t * pn * 3 * 64;
        const double* erel = k.erel + (size_t)t * en * 3 * 64;
        const bool rev_lds = N <= KB_REV_LDS_MAX_N;
        if (N <= 512)
            hipLaunchKernelGGL(kb_reverse_lists<256>, dim3(bc), dim3(256), KB_REV_LDS(N, rev_lds), st, idx, cnt, N, k.rev_off, k.rev,
                               rev_lds ? 1 : 0, (const int*)nullptr, 0);
        else
            hipLaunchKernelGGL(kb_reverse_lists<1024>, dim3(bc), dim3(1024), KB_REV_LDS(N, rev_lds), st, idx, cnt, N, k.rev_off, k.rev,
                               rev_lds ? 1 : 0, (const int*)nullptr, 0);
        const double* eff_last = eff + (size_t)(DRP_PSTEP - 1) * pn * 64;
        hipLaunchKernelGGL(kg_predict_bwd, pgrid, tblk, 0, st, w, eff_last, g_out, rows, k.g_eff, k.pr_h, k.pr_gh);
        narrow(g_out, 3, k.pr_h, 64, N, W_PR1_W, W_PR1_B);
        {
            const Kt64Job j = job(k.pr_gh, nullptr, 1, N, W_PR0_B, -1, 64);
            block(j, eff_last, KT64_X_ROW, W_PR0_W, nullptr, nullptr);
            bias(j);
        }
        for (int p = DRP_PSTEP - 1; p >= 0; --p) {
            const int first = p == DRP_PSTEP - 1;
            const double* eff_prev = p == 0 ? pe : eff + (size_t)(p - 1) * pn * 64;
            const double* erel_p = erel + (size_t)p * en * 64;
            hipLaunchKernelGGL(kg_pprop_bwd, pgrid, tblk, 0, st, w, eff + (size_t)p * pn * 64, k.g_eff, rows, k.g_pre, k.g_agg, k.g_pe, first);
            {
                const Kt64Job j = job(k.g_pre, nullptr, 1, N, W_PP_B, W_PP_W + 128, 129);
                block(j, pe, KT64_X_ROW, W_PP_W, nullptr, nullptr);
                block(j, agg + (size_t)p * pn * 64, KT64_X_ROW, W_PP_W + 64, nullptr, nullptr);
                bias(j);
            }
            hipLaunchKernelGGL(kg_rprop_bwd, egrid, tblk, 0, st, w, erel_p, k.g_agg, erows, k.g_re, k.gr, k.gs, first);
            {
                const Kt64Job j = job(k.g_agg, erel_p, DRP_K, R_e, W_RP_B, W_RP_W + 192, 193);
                block(j, re, KT64_X_ROW, W_RP_W, idx, cnt);
                block(j, eff_prev, KT64_X_RECV, W_RP_W + 64, idx, cnt);
                block(j, eff_prev, KT64_X_SEND, W_RP_W + 128, idx, cnt);
                bias(j);
            }
            hipLaunchKernelGGL(kg_gather_bwd, dim3((unsigned)((pn * 64 + 255) / 256)), dim3(256), 0, st, k.g_pre, k.gr, k.gs, cnt,
                               k.rev_off, k.rev, N, rows, p == 0 ? k.g_pe : (const double*)nullptr, k.g_eff);
        }
        hipLaunchKernelGGL(kg_pencode_bwd, pgrid, tblk, 0, st, w, k.sd + (size_t)t * pn * 3, attr, dens, pe, k.g_eff, N, rows, k.g_sd,
                           k.pe_in, k.pe_h, k.pe_gh);
        {
            const Kt64Job j = job(k.g_eff, pe, 1, N, W_PE2_B, -1, 64);
            block(j, k.pe_h, KT64_X_ROW, W_PE2_W, nullptr, nullptr);
            bias(j);
            narrow(k.pe_gh, 64, k.pe_in, 5, N, W_PE0_W, W_PE0_B);
        }
        // the relation encoder's hidden gradients at t == 0 too: its weights need them
        hipLaunchKernelGGL(kg_rencode_bwd, egrid, tblk, 0, st, w, s_t, attr, dens, idx, cnt, re, k.g_re, N, erows, k.g_diff, k.re_in,
                           k.re_h1, k.re_h2, k.re_g1, k.re_g2);
        {
            const Kt64Job j4 = job(k.g_re, re, 1, R_e, W_RE4_B, -1, 64);
            block(j4, k.re_h2, KT64_X_ROW, W_RE4_W, nullptr, nullptr);
            bias(j4);
            const Kt64Job j2 = job(k.re_g2, nullptr, 1, R_e, W_RE2_B, -1, 64);
            block(j2, k.re_h1, KT64_X_ROW, W_RE2_W, nullptr, nullptr);
            bias(j2);
            narrow(k.re_g1, 64, k.re_in, 6, R_e, W_RE0_W, W_RE0_B);
        }
        if (t > 0)
            hipLaunchKernelGGL(kt64_state_bwd, dim3((unsigned)((pn + 255) / 256)), dim3(256), 0, st, g_out, k.g_diff, cnt, k.rev_off, k.rev,
                               N, rows, k.g_state + (size_t)(t - 1) * pn * 3);
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(kt64_total, dim3((W_TOTAL + 255) / 256), dim3(256), 0, st, k.acc, bc, io.total);
    HIPCHK(c, hipGetLastError());
    if (grad_state_out) {
        // chunk layout [H][bc,N,3] -> caller layout [B,H,N,3]
        const size_t row = (size_t)N * 3 * sizeof(double);
        for (int t = 0; t < H; ++t)
            HIPCHK(c, hipMemcpy2DAsync(grad_state_out + ((size_t)b0 * H + t) * N * 3, (size_t)H * row, k.g_state + (size_t)t * pn * 3, row,
                                       row, bc, hipMemcpyDeviceToHost, st));
    }
    return DRP_OK;
}

}  // namespace

int drp_train_grad_f64(drp_ctx* c, const float* states, const float* states_delta, const float* attrs, const int32_t* particle_nums,
                       const float* particle_dens, int B, int N, int n_rollout, double* loss_out, double* loss_terms_out,
                       double* grad_out, double* grad_state_out) {
    CHK(need(c, true, false, false));
    CHK(check_bn(c, B, N));
    if (!states || !states_delta || !attrs || !particle_nums || !particle_dens) return fail(c, DRP_EINVAL, "null argument");
    if (n_rollout < 1 || n_rollout > 64) return fail(c, DRP_EINVAL, "bad n_rollout=%d", n_rollout);
    for (int b = 0; b < B; ++b)
        if (particle_nums[b] <= 0 || particle_nums[b] > N)
            return fail(c, DRP_EINVAL, "particle_nums[%d]=%d outside 1..%d", b, particle_nums[b], N);
    HIPCHK(c, hipSetDevice(c->device));
    F64Scope scope(c);
    if (!c->f64_w_valid) CHK(f64_refresh_weights(c));
    const int H = n_rollout;
    // samples per chunk under the cap (tape, reverse pass and accumulators together); one sample is the smallest chunk
    const size_t one = tr64_carve(nullptr, 1, (size_t)N, (size_t)H).bytes;
    size_t Bc = std::min<size_t>({(size_t)B, std::max<size_t>(1, c->f64_cap / one), std::max<size_t>(1, ((size_t)1 << 24) / ((size_t)N * DRP_K))});
    while (Bc > 1 && tr64_carve(nullptr, Bc, (size_t)N, (size_t)H).bytes > c->f64_cap) --Bc;
    CHK(ensure(c, c->tr64_ws, tr64_carve(nullptr, Bc, (size_t)N, (size_t)H).bytes));
    const Tr64Ws k = tr64_carve(c->tr64_ws.p, Bc, (size_t)N, (size_t)H);
    // the whole batch's inputs in one upload: states | impulses | attrs[:, 0] | densities | particle counts, then the results
    const size_t n_st = (size_t)B * (H + 1) * N * 3, n_sd = (size_t)B * H * N * 3, n_at = (size_t)B * N;
    std::vector<float> host(n_st + n_sd + n_at + (size_t)B + (size_t)B);
    memcpy(host.data(), states, n_st * sizeof(float));
    memcpy(host.data() + n_st, states_delta, n_sd * sizeof(float));
    for (int b = 0; b < B; ++b) memcpy(host.data() + n_st + n_sd + (size_t)b * N, attrs + (size_t)b * (H + 1) * N, (size_t)N * sizeof(float));
    memcpy(host.data() + n_st + n_sd + n_at, particle_dens, (size_t)B * sizeof(float));
    memcpy(host.data() + n_st + n_sd + n_at + B, particle_nums, (size_t)B * sizeof(int32_t));
    const size_t in_bytes = (host.size() * sizeof(float) + 255) & ~(size_t)255;
    const size_t n_terms = (size_t)H * B;
    CHK(ensure(c, c->tr64_io, in_bytes + (n_terms + (size_t)W_TOTAL) * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(c->tr64_io.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    Tr64Io io{};
    io.states = ptr<float>(c->tr64_io); io.sdelta = io.states + n_st; io.attr = io.sdelta + n_sd; io.dens = io.attr + n_at;
    io.nums = reinterpret_cast<const int*>(io.dens + B);
    io.terms = reinterpret_cast<double*>(static_cast<char*>(c->tr64_io.p) + in_bytes);
    io.total = io.terms + n_terms;
    HIPCHK(c, hipMemsetAsync(io.total, 0, (size_t)W_TOTAL * sizeof(double), c->stream));
    // the fp32 graph build's staging (the scope's buffers) for a chunk
    CHK(ensure_step_ws(c, (int)Bc, N, -1));
    CHK(ensure(c, c->s_in, Bc * N * 3 * sizeof(float)));
    CHK(ensure(c, c->s_delta, Bc * N * 3 * sizeof(float)));
    for (int b0 = 0; b0 < B; b0 += (int)Bc)
        CHK(tr64_chunk(c, k, io, b0, std::min((int)Bc, B - b0), N, B, H, grad_state_out));
    std::vector<double> terms(n_terms);
    CHK(d2h(c, terms.data(), io.terms, n_terms * sizeof(double)));
    if (grad_out) CHK(d2h(c, grad_out, io.total, (size_t)W_TOTAL * sizeof(double)));
    CHK(guarded_wait(c, nullptr));          // (the upload's host block lives until here)
    if (loss_terms_out) memcpy(loss_terms_out, terms.data(), n_terms * sizeof(double));
    if (loss_out) {
        double total = 0.0;                 // fixed order: step-major, then sample (as drp_train_step)
        for (size_t q = 0; q < n_terms; ++q) total += terms[q];
        *loss_out = total;
    }
    return DRP_OK;
}
