// capi_gd_f64.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: one iteration of the gradient-descent planner in float64 (drp_gd_grad_f64; kernels: k_prop_f64.h forward, k_gd_f64.h), the
// yardstick of the tape engines' gradient (row y2).  Like the one-step calls of capi_f64.h it is no engine and no session: it
// works in buffers of its own under F64Scope and leaves the context as it found it.

namespace {

// a chunk's workspace, carved from one allocation: base == nullptr only measures
struct Gd64Ws {
    // the tape: a step's intermediates (k_prop_f64.h: KF_BYTES_PER_PARTICLE), states, impulses and lists
    double *pe, *re, *eff, *agg, *erel, *pred;          // [H] blocks each
    double *state, *sd;                                 // [H+1][pn,3], [H][pn,3]
    int16_t* idx; uint8_t* cnt;                         // [H][pn,10], [H][pn]
    // the reverse pass
    double *g_eff, *g_pre, *g_agg, *g_pe, *g_re, *gr, *gs, *g_sd, *g_diff, *g_state, *part;
    int *rev_off, *rev;
    // the reward
    double *px, *py, *gx, *gy, *r1t, *dist;
    int* arg;
    size_t bytes;
};
Gd64Ws gd64_carve(void* base, size_t bc, size_t N, size_t H, size_t M) {
    Gd64Ws w{};
    size_t off = 0;
    auto take = [&](auto*& p, size_t n) {
        typedef typename std::remove_reference<decltype(*p)>::type T;
        p = base ? reinterpret_cast<T*>(static_cast<char*>(base) + off) : nullptr;
        off += (n * sizeof(T) + 255) & ~(size_t)255;
    };
    const size_t pn = bc * N;
    take(w.pe, H * pn * 64); take(w.re, H * pn * DRP_K * 64); take(w.eff, H * pn * 3 * 64); take(w.agg, H * pn * 3 * 64);
    take(w.erel, H * pn * 3 * DRP_K * 64); take(w.pred, H * pn * 3);
    take(w.state, (H + 1) * pn * 3); take(w.sd, H * pn * 3); take(w.idx, H * pn * DRP_K); take(w.cnt, H * pn);
    take(w.g_eff, pn * 64); take(w.g_pre, pn * 64); take(w.g_agg, pn * 64); take(w.g_pe, pn * 64);
    take(w.g_re, pn * DRP_K * 64); take(w.gr, pn * DRP_K * 64); take(w.gs, pn * DRP_K * 64);
    take(w.g_sd, pn * 3); take(w.g_diff, pn * DRP_K * 3); take(w.g_state, H * pn * 3); take(w.part, pn * 4);
    take(w.rev_off, bc * (N + 1)); take(w.rev, pn * DRP_K);
    take(w.px, pn); take(w.py, pn); take(w.gx, pn); take(w.gy, pn); take(w.r1t, pn); take(w.dist, bc * M); take(w.arg, bc * M);
    w.bytes = off;
    return w;
}

// forward with tape, reward, reverse pass of the rows [b0, b0 + bc): launches and the copies of its results
int gd64_chunk(drp_ctx* c, const Gd64Ws& k, int b0, int bc, int nb, int N, int B, int H, const float* s0, const float* attr_x,
               const float* dens_x, const float* actions, double* rewards, double* g_act, double* grad_state_out) {
    hipStream_t st = c->stream;
    const double* w = ptr<double>(c->f64_w);
    const int rows = bc * N, erows = rows * DRP_K, M = c->goal_m;
    const size_t pn = (size_t)rows;
    const dim3 tblk(64 * KG_WAVES);
    const dim3 pgrid((rows + 16 * KG_WAVES - 1) / (16 * KG_WAVES)), egrid((erows + 16 * KG_WAVES - 1) / (16 * KG_WAVES));
    const float* attr = attr_x + (size_t)b0 * N;
    const float* dens = dens_x + b0;
    const float* act = actions + (size_t)b0 * H * 4;
    hipLaunchKernelGGL(kg_init_state, dim3((unsigned)((pn * 3 + 255) / 256)), dim3(256), 0, st, s0, nb, b0, N, (long)(pn * 3), k.state);
    // ---- forward: gen_s_delta in double, the lists from the fp32 graph build on the roundings, the step in double
    for (int t = 0; t < H; ++t) {
        const double* s_t = k.state + (size_t)t * pn * 3;
        double* sd_t = k.sd + (size_t)t * pn * 3;
        int16_t* idx = k.idx + (size_t)t * pn * DRP_K;
        uint8_t* cnt = k.cnt + (size_t)t * pn;
        hipLaunchKernelGGL(kg_sdelta, dim3(bc), dim3(256), 0, st, s_t, act + (size_t)t * 4, (size_t)H * 4, N, c->cam, sd_t,
                           ptr<float>(c->s_in), ptr<float>(c->s_delta));
        const GraphPlan g = plan_graph(c->pol, c->n_cu, c->engine, bc, N, false, false, false, true);
        launch_graph(c, st, g, ptr<float>(c->s_in), bc, (size_t)N * 3, (const float*)nullptr, (size_t)0, ptr<float>(c->s_delta), bc, N,
                     idx, cnt, 0);
        f64_launch_step<double>(c, w, s_t, sd_t, attr, dens, idx, cnt, N, rows, k.pe + (size_t)t * pn * 64,
                                k.re + (size_t)t * pn * DRP_K * 64, k.eff + (size_t)t * pn * 3 * 64, k.agg + (size_t)t * pn * 3 * 64,
                                k.erel + (size_t)t * pn * 3 * DRP_K * 64, k.pred + (size_t)t * pn * 3, k.state + (size_t)(t + 1) * pn * 3);
        HIPCHK(c, hipGetLastError());
    }
    // ---- reward of the final state and its gradient
    hipLaunchKernelGGL(kg_reward, dim3(bc), dim3(256), 0, st, k.state + (size_t)H * pn * 3, N, ptr<float>(c->goal_field), c->goal_h,
                       c->goal_w, ptr<float>(c->goal_coor), M, c->cam, k.px, k.py, k.gx, k.gy, k.r1t, k.dist, k.arg, rewards + b0,
                       k.g_state + (size_t)(H - 1) * pn * 3);
    // ---- reverse pass, step by step
    for (int t = H - 1; t >= 0; --t) {
        const double* s_t = k.state + (size_t)t * pn * 3;
        const double* g_out = k.g_state + (size_t)t * pn * 3;
        const int16_t* idx = k.idx + (size_t)t * pn * DRP_K;
        const uint8_t* cnt = k.cnt + (size_t)t * pn;
        const double* pe = k.pe + (size_t)t * pn * 64;
        const double* re = k.re + (size_t)t * pn * DRP_K * 64;
        const double* eff = k.eff + (size_t)t * pn * 3 * 64;
        const double* erel = k.erel + (size_t)t * pn * 3 * DRP_K * 64;
        // the reversed lists of this step (k_graph.h: reverse_lists), into the call's own buffers
        const bool rev_lds = N <= KB_REV_LDS_MAX_N;
        if (N <= 512)
            hipLaunchKernelGGL(kb_reverse_lists<256>, dim3(bc), dim3(256), KB_REV_LDS(N, rev_lds), st, idx, cnt, N, k.rev_off, k.rev,
                               rev_lds ? 1 : 0, (const int*)nullptr, 0);
        else
            hipLaunchKernelGGL(kb_reverse_lists<1024>, dim3(bc), dim3(1024), KB_REV_LDS(N, rev_lds), st, idx, cnt, N, k.rev_off, k.rev,
                               rev_lds ? 1 : 0, (const int*)nullptr, 0);
        hipLaunchKernelGGL(kg_predict_bwd, pgrid, tblk, 0, st, w, eff + (size_t)(DRP_PSTEP - 1) * pn * 64, g_out, rows, k.g_eff);
        for (int p = DRP_PSTEP - 1; p >= 0; --p) {
            const int first = p == DRP_PSTEP - 1;
            hipLaunchKernelGGL(kg_pprop_bwd, pgrid, tblk, 0, st, w, eff + (size_t)p * pn * 64, k.g_eff, rows, k.g_pre, k.g_agg, k.g_pe, first);
            hipLaunchKernelGGL(kg_rprop_bwd, egrid, tblk, 0, st, w, erel + (size_t)p * pn * DRP_K * 64, k.g_agg, erows, k.g_re, k.gr,
                               k.gs, first);
            // effect_0 is the particle encoding itself: its gradient joins the propagators' (p == 0)
            hipLaunchKernelGGL(kg_gather_bwd, dim3((unsigned)((pn * 64 + 255) / 256)), dim3(256), 0, st, k.g_pre, k.gr, k.gs, cnt,
                               k.rev_off, k.rev, N, rows, p == 0 ? k.g_pe : (const double*)nullptr, k.g_eff);
        }
        hipLaunchKernelGGL(kg_pencode_bwd, pgrid, tblk, 0, st, w, k.sd + (size_t)t * pn * 3, attr, dens, pe, k.g_eff, N, rows, k.g_sd);
        if (t > 0)
            hipLaunchKernelGGL(kg_rencode_bwd, egrid, tblk, 0, st, w, s_t, attr, dens, idx, cnt, re, k.g_re, N, erows, k.g_diff);
        hipLaunchKernelGGL(kg_sdelta_bwd, dim3(bc), dim3(256), 0, st, s_t, act + (size_t)t * 4, (size_t)H * 4, k.g_sd, g_out, k.g_diff, cnt,
                           k.rev_off, k.rev, N, c->cam, k.part, g_act + (size_t)b0 * H * 4 + (size_t)t * 4, (size_t)H * 4,
                           t > 0 ? k.g_state + (size_t)(t - 1) * pn * 3 : (double*)nullptr);
        HIPCHK(c, hipGetLastError());
    }
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

int drp_gd_grad_f64(drp_ctx* c, const float* s0, const float* attr, const float* dens, int nb, int N, const float* actions, int B,
                    int H, double* rewards_out, double* grad_act_out, double* grad_state_out) {
    CHK(need(c, true, true, true));
    CHK(check_bn(c, B, N));
    if (!s0 || !attr || !dens || !actions) return fail(c, DRP_EINVAL, "null argument");
    if (H < 1 || H > 64) return fail(c, DRP_EINVAL, "bad horizon H=%d", H);
    if (nb <= 0 || B % nb != 0) return fail(c, DRP_EINVAL, "B must be a multiple of n_batch");
    HIPCHK(c, hipSetDevice(c->device));
    F64Scope scope(c);
    if (!c->f64_w_valid) CHK(f64_refresh_weights(c));
    // rows per chunk under the cap (tape and reverse pass together); one row is the smallest chunk
    const size_t M = (size_t)c->goal_m;
    const size_t one = gd64_carve(nullptr, 1, (size_t)N, (size_t)H, M).bytes;
    size_t Bc = std::min<size_t>({(size_t)B, std::max<size_t>(1, c->f64_cap / one), std::max<size_t>(1, ((size_t)1 << 24) / (size_t)N)});
    while (Bc > 1 && gd64_carve(nullptr, Bc, (size_t)N, (size_t)H, M).bytes > c->f64_cap) --Bc;
    CHK(ensure(c, c->gd64_ws, gd64_carve(nullptr, Bc, (size_t)N, (size_t)H, M).bytes));
    const Gd64Ws k = gd64_carve(c->gd64_ws.p, Bc, (size_t)N, (size_t)H, M);
    // the whole batch's inputs (attributes and densities per row: row = traj * nb + batch) and results
    const size_t n_s0 = (size_t)nb * N * 3, n_attr = (size_t)B * N, n_act = (size_t)B * H * 4;
    std::vector<float> host(n_s0 + n_attr + (size_t)B + n_act);
    memcpy(host.data(), s0, n_s0 * sizeof(float));
    for (int b = 0; b < B; ++b) {
        memcpy(host.data() + n_s0 + (size_t)b * N, attr + (size_t)(b % nb) * N, (size_t)N * sizeof(float));
        host[n_s0 + n_attr + b] = dens[b % nb];
    }
    memcpy(host.data() + n_s0 + n_attr + B, actions, n_act * sizeof(float));
    const size_t in_bytes = (host.size() * sizeof(float) + 255) & ~(size_t)255;
    CHK(ensure(c, c->gd64_io, in_bytes + ((size_t)B + n_act) * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(c->gd64_io.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const float* d_in = ptr<float>(c->gd64_io);
    double* d_rew = reinterpret_cast<double*>(static_cast<char*>(c->gd64_io.p) + in_bytes);
    double* d_gact = d_rew + B;
    // the fp32 graph build's staging (the scope's buffers) for a chunk
    CHK(ensure_step_ws(c, (int)Bc, N, -1));
    CHK(ensure(c, c->s_in, Bc * N * 3 * sizeof(float)));
    CHK(ensure(c, c->s_delta, Bc * N * 3 * sizeof(float)));
    for (int b0 = 0; b0 < B; b0 += (int)Bc)
        CHK(gd64_chunk(c, k, b0, std::min((int)Bc, B - b0), nb, N, B, H, d_in, d_in + n_s0, d_in + n_s0 + n_attr,
                       d_in + n_s0 + n_attr + B, d_rew, d_gact, grad_state_out));
    if (rewards_out) CHK(d2h(c, rewards_out, d_rew, (size_t)B * sizeof(double)));
    if (grad_act_out) CHK(d2h(c, grad_act_out, d_gact, n_act * sizeof(double)));
    return guarded_wait(c, nullptr);        // (the upload's host block lives until here)
}
