// capi_grad_f64.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the two float64 gradients -- one iteration of the gradient-descent planner (drp_gd_grad_f64, the yardstick of the tape
// engines' gradient, row y2) and the training loop body (drp_train_grad_f64, the yardstick of drp_train_step's gradients, row
// y3) -- on ONE tape and ONE reverse pass (kernels: k_prop_f64.h forward, k_gd_f64.h backward; k_train_f64.h loss and weight
// gradients).  They differ in where a step's impulse comes from (the push, or data), in the loss that seeds the reverse pass, in
// the tail of a reverse step, and in the trainer's weight-gradient launches in between (F64Wgrad).  drp_train_grad_f64_untracked is the
// trainer's body with the Chamfer loss of k_chamfer_f64.h as the seed (row u1's yardstick); everything behind the seed is the
// same code, and drp_train_grad_f64_divergence (capi_divergence_f64.h) is it with the Sinkhorn divergence of k_sinkhorn.h
// (row u4), drp_train_grad_f64_match (capi_match_f64.h) with the matching term of k_match_f64.h or its mix with the Chamfer term
// (row u2).  Like the one-step calls of
// capi_f64.h they are no engine and no session: they work in buffers of their own under F64Scope, keep nothing between calls
// and leave the context -- the trainer's Adam state included -- as they found it.

namespace {

// buffers from one allocation, each rounded up to 256 bytes; a null base only measures
extern "C++" struct F64Carver {
    char* base;
    size_t off = 0;
    template <typename T> void take(T*& p, size_t n) {
        p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (n * sizeof(T) + 255) & ~(size_t)255;
    }
};

// the tape: every step's intermediates (k_prop_f64.h: KF_BYTES_PER_PARTICLE), states, impulses and lists
struct F64Tape {
    double *pe, *re, *eff, *agg, *erel, *pred;          // [H] blocks each
    double *state, *sd;                                 // [H+1][pn,3], [H][pn,3]
    int16_t* idx; uint8_t* cnt;                         // [H][pn,10], [H][pn]
    void carve(F64Carver& a, size_t pn, size_t H) {
        a.take(pe, H * pn * 64); a.take(re, H * pn * DRP_K * 64); a.take(eff, H * pn * 3 * 64); a.take(agg, H * pn * 3 * 64);
        a.take(erel, H * pn * 3 * DRP_K * 64); a.take(pred, H * pn * 3);
        a.take(state, (H + 1) * pn * 3); a.take(sd, H * pn * 3); a.take(idx, H * pn * DRP_K); a.take(cnt, H * pn);
    }
    // step t's slices in a chunk of pn rows: `state` is the step's input, state + pn * 3 its output
    F64Tape step(int t, size_t pn) const {
        const size_t o = (size_t)t * pn;
        return F64Tape{pe + o * 64, re + o * DRP_K * 64, eff + o * 3 * 64, agg + o * 3 * 64, erel + o * 3 * DRP_K * 64, pred + o * 3,
                       state + o * 3, sd + o * 3, idx + o * DRP_K, cnt + o};
    }
};

// the reverse pass of one step, and the state gradient of every step
struct F64Rev {
    double *g_eff, *g_pre, *g_agg, *g_pe, *g_re, *gr, *gs, *g_sd, *g_diff;
    double* g_state;                                    // [H][pn,3]
    double* part;                                       // the planner's scratch of kg_sdelta_bwd [pn,4]; the trainer: n_part = 0
    int *rev_off, *rev;
    void carve(F64Carver& a, size_t bc, size_t N, size_t H, size_t n_part) {
        const size_t pn = bc * N;
        a.take(g_eff, pn * 64); a.take(g_pre, pn * 64); a.take(g_agg, pn * 64); a.take(g_pe, pn * 64);
        a.take(g_re, pn * DRP_K * 64); a.take(gr, pn * DRP_K * 64); a.take(gs, pn * DRP_K * 64);
        a.take(g_sd, pn * 3); a.take(g_diff, pn * DRP_K * 3); a.take(g_state, H * pn * 3); a.take(part, n_part);
        a.take(rev_off, bc * (N + 1)); a.take(rev, pn * DRP_K);
    }
};

// Samples per chunk under the cap and the caller's row limit (one is the smallest chunk; bytes_of(bc): the caller's measuring
// carve), with the workspace for them and the fp32 graph build's staging (the scope's buffers)
extern "C++" template <typename F> int f64_size_chunks(drp_ctx* c, int B, int N, size_t row_limit, F bytes_of, size_t* chunk) {
    size_t Bc = std::min<size_t>({(size_t)B, std::max<size_t>(1, c->f64_cap / bytes_of(1)), std::max<size_t>(1, row_limit)});
    while (Bc > 1 && bytes_of(Bc) > c->f64_cap) --Bc;
    CHK(ensure(c, c->grad64_ws, bytes_of(Bc)));
    CHK(ensure_step_ws(c, c->ws, (int)Bc, N, -1));
    CHK(ensure(c, c->ws.s_in, Bc * N * 3 * sizeof(float)));
    *chunk = Bc;
    return DRP_OK;
}

// the whole batch's packed inputs in one upload, `n_res` doubles of results behind a 256-byte boundary (returned)
int f64_upload_batch(drp_ctx* c, const std::vector<float>& host, size_t n_res, double** res) {
    const size_t in_bytes = (host.size() * sizeof(float) + 255) & ~(size_t)255;
    CHK(ensure(c, c->grad64_io, in_bytes + n_res * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(c->grad64_io.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    *res = reinterpret_cast<double*>(static_cast<char*>(c->grad64_io.p) + in_bytes);
    return DRP_OK;
}

// forward with tape over H steps from tape.state[0]: stage(t, s) puts step t's impulse in double into s.sd and the fp32
// roundings of s.state and of the impulse where the graph build reads them; the lists from the fp32 graph build (`padded`: the
// trainer's mode) on those roundings; the step in double
extern "C++" template <typename Stage>
int f64_tape_forward(drp_ctx* c, const F64Tape& tape, int bc, int N, int H, const float* attr, const float* dens, bool padded,
                     Stage stage) {
    const int rows = bc * N;
    for (int t = 0; t < H; ++t) {
        const F64Tape s = tape.step(t, (size_t)rows);
        stage(t, s);
        const GraphPlan g = plan_graph(c->pol, c->n_cu, c->engine, bc, N, padded, false, false, true);
        launch_graph(c, c->stream, g, ptr<float>(c->ws.s_in), bc, (size_t)N * 3, (const float*)nullptr, (size_t)0, ptr<float>(c->ws.s_delta),
                     bc, N, s.idx, s.cnt, 0);
        f64_launch_step<double>(c, ptr<double>(c->f64_w), s.state, s.sd, attr, dens, s.idx, s.cnt, N, rows, s.pe, s.re, s.eff, s.agg,
                                s.erel, s.pred, s.state + (size_t)rows * 3);
        HIPCHK(c, hipGetLastError());
    }
    return DRP_OK;
}

// the reversed lists of `sets` samples' neighbour lists (k_graph.h: reverse_lists) into the call's own buffers
void f64_reverse_lists(hipStream_t st, const int16_t* idx, const uint8_t* cnt, int N, int sets, int* rev_off, int* rev) {
    const bool rev_lds = N <= KB_REV_LDS_MAX_N;
    if (N <= 512)
        hipLaunchKernelGGL(kb_reverse_lists<256>, dim3(sets), dim3(256), KB_REV_LDS(N, rev_lds), st, idx, cnt, N, rev_off, rev,
                           rev_lds ? 1 : 0, (const int*)nullptr, 0);
    else
        hipLaunchKernelGGL(kb_reverse_lists<1024>, dim3(sets), dim3(1024), KB_REV_LDS(N, rev_lds), st, idx, cnt, N, rev_off, rev,
                           rev_lds ? 1 : 0, (const int*)nullptr, 0);
}

// The trainer's weight gradients of a reverse step: what the backward kernels leave for them (hidden layers, their masked
// gradients, the narrow inputs), the samples' accumulators, and the launches.  A layer's weight gradient: its 64-wide blocks
// on the matrix instruction, bias and density column as chains.
struct F64Wgrad {
    hipStream_t st;
    int bc, N;
    const float* dens;
    double *pr_h, *pr_gh, *pe_h, *pe_gh, *pe_in, *re_h1, *re_h2, *re_g1, *re_g2, *re_in;
    double* acc;                                        // [bc][W_TOTAL]: a sample's gradient
    Kt64Job job(const double* g, const double* m, int g_div, int R, int b_off, int d_off, int ld) const {
        Kt64Job j{};
        j.g = g; j.m = m; j.g_div = g_div; j.N = N; j.R = R; j.ld = ld; j.b_off = b_off; j.d_off = d_off;
        return j;
    }
    void block(Kt64Job j, const double* x, int x_mode, int w_off, const int16_t* idx, const uint8_t* cnt) const {
        j.x = x; j.x_mode = x_mode; j.w_off = w_off; j.idx = idx; j.cnt = cnt;
        hipLaunchKernelGGL(kt64_wgrad64, dim3(4, bc), dim3(256), 0, st, j, acc);
    }
    void bias(const Kt64Job& j) const { hipLaunchKernelGGL(kt64_wgrad_bias, dim3(bc), dim3(128), 0, st, j, dens, acc); }
    void narrow(const double* G, int gw, const double* X, int xw, int R, int w_off, int b_off) const {
        hipLaunchKernelGGL(kt64_wgrad_narrow, dim3((unsigned)((gw * (xw + 1) + 255) / 256), bc), dim3(256), 0, st, G, gw, X, xw, R, w_off,
                           b_off, acc);
    }
};

// The reverse pass of rollout step t, from g_out = d loss / d the step's output state [bc*N,3] down to r.g_sd (d / d impulse)
// and r.g_diff (d / d (s_r - s_s) per slot; without `wg` only where a step before this one reads it, t > 0): the reversed
// lists, the predictor, the propagation steps, the encoders.  s: the tape's slices of the step.  `wg` (nullable): the
// trainer's weight gradients, queued behind the kernel that leaves their operands; the relation encoder then runs at t == 0
// too, its weights need its hidden gradients.  The step's share of d loss / d input state is the caller's tail.
void f64_reverse_step(drp_ctx* c, const F64Tape& s, const F64Rev& r, const double* g_out, int t, int bc, int N, const float* attr,
                      const float* dens, const F64Wgrad* wg) {
    hipStream_t st = c->stream;
    const double* w = ptr<double>(c->f64_w);
    const int rows = bc * N, erows = rows * DRP_K, R_e = N * DRP_K;
    const size_t pn = (size_t)rows, en = (size_t)erows;
    const dim3 tblk(64 * KG_WAVES);
    const dim3 pgrid((rows + 16 * KG_WAVES - 1) / (16 * KG_WAVES)), egrid((erows + 16 * KG_WAVES - 1) / (16 * KG_WAVES));
    const F64Wgrad d = wg ? *wg : F64Wgrad{};           // the kernels' dump pointers: null without weight gradients
    f64_reverse_lists(st, s.idx, s.cnt, N, bc, r.rev_off, r.rev);
    const double* eff_last = s.eff + (size_t)(DRP_PSTEP - 1) * pn * 64;
    hipLaunchKernelGGL(kg_predict_bwd, pgrid, tblk, 0, st, w, eff_last, g_out, rows, r.g_eff, d.pr_h, d.pr_gh);
    if (wg) {
        wg->narrow(g_out, 3, wg->pr_h, 64, N, W_PR1_W, W_PR1_B);
        const Kt64Job j = wg->job(wg->pr_gh, nullptr, 1, N, W_PR0_B, -1, 64);
        wg->block(j, eff_last, KT64_X_ROW, W_PR0_W, nullptr, nullptr);
        wg->bias(j);
    }
    for (int p = DRP_PSTEP - 1; p >= 0; --p) {
        const int first = p == DRP_PSTEP - 1;
        const double* eff_prev = p == 0 ? s.pe : s.eff + (size_t)(p - 1) * pn * 64;
        const double* erel_p = s.erel + (size_t)p * en * 64;
        hipLaunchKernelGGL(kg_pprop_bwd, pgrid, tblk, 0, st, w, s.eff + (size_t)p * pn * 64, r.g_eff, rows, r.g_pre, r.g_agg, r.g_pe, first);
        if (wg) {
            const Kt64Job j = wg->job(r.g_pre, nullptr, 1, N, W_PP_B, W_PP_W + 128, 129);
            wg->block(j, s.pe, KT64_X_ROW, W_PP_W, nullptr, nullptr);
            wg->block(j, s.agg + (size_t)p * pn * 64, KT64_X_ROW, W_PP_W + 64, nullptr, nullptr);
            wg->bias(j);
        }
        hipLaunchKernelGGL(kg_rprop_bwd, egrid, tblk, 0, st, w, erel_p, r.g_agg, erows, r.g_re, r.gr, r.gs, first);
        if (wg) {
            const Kt64Job j = wg->job(r.g_agg, erel_p, DRP_K, R_e, W_RP_B, W_RP_W + 192, 193);
            wg->block(j, s.re, KT64_X_ROW, W_RP_W, s.idx, s.cnt);
            wg->block(j, eff_prev, KT64_X_RECV, W_RP_W + 64, s.idx, s.cnt);
            wg->block(j, eff_prev, KT64_X_SEND, W_RP_W + 128, s.idx, s.cnt);
            wg->bias(j);
        }
        // effect_0 is the particle encoding itself: its gradient joins the propagators' (p == 0)
        hipLaunchKernelGGL(kg_gather_bwd, dim3((unsigned)((pn * 64 + 255) / 256)), dim3(256), 0, st, r.g_pre, r.gr, r.gs, s.cnt, r.rev_off,
                           r.rev, N, rows, p == 0 ? r.g_pe : (const double*)nullptr, r.g_eff);
    }
    hipLaunchKernelGGL(kg_pencode_bwd, pgrid, tblk, 0, st, w, s.sd, attr, dens, s.pe, r.g_eff, N, rows, r.g_sd, d.pe_in, d.pe_h, d.pe_gh);
    if (wg) {
        const Kt64Job j = wg->job(r.g_eff, s.pe, 1, N, W_PE2_B, -1, 64);
        wg->block(j, wg->pe_h, KT64_X_ROW, W_PE2_W, nullptr, nullptr);
        wg->bias(j);
        wg->narrow(wg->pe_gh, 64, wg->pe_in, 5, N, W_PE0_W, W_PE0_B);
    }
    if (wg || t > 0)
        hipLaunchKernelGGL(kg_rencode_bwd, egrid, tblk, 0, st, w, s.state, attr, dens, s.idx, s.cnt, s.re, r.g_re, N, erows, r.g_diff,
                           d.re_in, d.re_h1, d.re_h2, d.re_g1, d.re_g2);
    if (wg) {
        const Kt64Job j4 = wg->job(r.g_re, s.re, 1, R_e, W_RE4_B, -1, 64);
        wg->block(j4, wg->re_h2, KT64_X_ROW, W_RE4_W, nullptr, nullptr);
        wg->bias(j4);
        const Kt64Job j2 = wg->job(wg->re_g2, nullptr, 1, R_e, W_RE2_B, -1, 64);
        wg->block(j2, wg->re_h1, KT64_X_ROW, W_RE2_W, nullptr, nullptr);
        wg->bias(j2);
        wg->narrow(wg->re_g1, 64, wg->re_in, 6, R_e, W_RE0_W, W_RE0_B);
    }
}

// the state gradient of the samples [b0, b0 + bc): chunk layout [H][bc,N,3] -> caller layout [B,H,N,3]
int f64_copy_state_grad(drp_ctx* c, const double* g_state, int b0, int bc, int N, int H, double* grad_state_out) {
    const size_t row = (size_t)N * 3 * sizeof(double);
    for (int t = 0; t < H; ++t)
        HIPCHK(c, hipMemcpy2DAsync(grad_state_out + ((size_t)b0 * H + t) * N * 3, (size_t)H * row, g_state + (size_t)t * bc * N * 3, row,
                                   row, bc, hipMemcpyDeviceToHost, c->stream));
    return DRP_OK;
}

// ---- the planner's gradient ---------------------------------------------------------------------------------------------
// a chunk's workspace: the shared parts, then the reward's scratch
struct Gd64Ws {
    F64Tape tape;
    F64Rev rev;
    double *px, *py, *gx, *gy, *r1t, *dist;
    int* arg;
    double* seed_mid;               // seeded: the caller's seeds of the steps before the last [H-1][pn,3] (kg_seed_in); else nothing
    size_t carve(void* base, size_t bc, size_t N, size_t H, size_t M, bool seeded = false) {         // -> its bytes
        F64Carver a{static_cast<char*>(base)};
        const size_t pn = bc * N;
        tape.carve(a, pn, H);
        rev.carve(a, bc, N, H, pn * 4);
        a.take(px, pn); a.take(py, pn); a.take(gx, pn); a.take(gy, pn); a.take(r1t, pn); a.take(dist, bc * M); a.take(arg, bc * M);
        a.take(seed_mid, seeded ? (H - 1) * pn * 3 : 0);
        return a.off;
    }
};
// what takes the reward's place (drp_gd_predict_f64, drp_gd_grad_f64_seeded): nothing -- the forward alone, every step's state to
// grad_state_out -- or the caller's seed, the whole batch's on the device [B][H][N][3], sliced per chunk by kg_seed_in
struct Gd64Given { bool predict = false; const double* seed = nullptr; };

// forward with tape, reward, reverse pass of the rows [b0, b0 + bc): launches and the copies of its results
int gd64_chunk(drp_ctx* c, const Gd64Ws& k, int b0, int bc, int nb, int N, int H, const float* s0, const float* attr_x,
               const float* dens_x, const float* actions, double* rewards, double* g_act, double* grad_state_out,
               const Gd64Given& given = Gd64Given{}) {
    hipStream_t st = c->stream;
    const size_t pn = (size_t)bc * N;
    const float* attr = attr_x + (size_t)b0 * N;
    const float* dens = dens_x + b0;
    const float* act = actions + (size_t)b0 * H * 4;
    hipLaunchKernelGGL(kg_init_state, dim3((unsigned)((pn * 3 + 255) / 256)), dim3(256), 0, st, s0, nb, b0, N, (long)(pn * 3), k.tape.state);
    // ---- forward: gen_s_delta in double
    CHK(f64_tape_forward(c, k.tape, bc, N, H, attr, dens, false, [&](int t, const F64Tape& s) {
        hipLaunchKernelGGL(kg_sdelta, dim3(bc), dim3(256), 0, st, s.state, act + (size_t)t * 4, (size_t)H * 4, N, c->cam, s.sd,
                           ptr<float>(c->ws.s_in), ptr<float>(c->ws.s_delta));
    }));
    if (given.predict) return f64_copy_state_grad(c, k.tape.state + pn * 3, b0, bc, N, H, grad_state_out);
    // ---- reward of the final state and its gradient, or the caller's seed in its place
    if (given.seed)
        hipLaunchKernelGGL(kg_seed_in, dim3(bc, H), dim3(256), 0, st, given.seed, b0, N, k.seed_mid, k.rev.g_state + (size_t)(H - 1) * pn * 3);
    else
        hipLaunchKernelGGL(kg_reward, dim3(bc), dim3(256), 0, st, k.tape.state + (size_t)H * pn * 3, N, ptr<float>(c->goal_field), c->goal_h,
                           c->goal_w, ptr<float>(c->goal_coor), c->goal_m, c->cam, k.px, k.py, k.gx, k.gy, k.r1t, k.dist, k.arg, rewards + b0,
                           k.rev.g_state + (size_t)(H - 1) * pn * 3);
    // ---- reverse pass, step by step; its tail: gen_s_delta backward and the step's share of d loss / d input state
    for (int t = H - 1; t >= 0; --t) {
        const F64Tape s = k.tape.step(t, pn);
        const double* g_out = k.rev.g_state + (size_t)t * pn * 3;
        f64_reverse_step(c, s, k.rev, g_out, t, bc, N, attr, dens, nullptr);
        hipLaunchKernelGGL(kg_sdelta_bwd, dim3(bc), dim3(256), 0, st, s.state, act + (size_t)t * 4, (size_t)H * 4, k.rev.g_sd, g_out,
                           k.rev.g_diff, s.cnt, k.rev.rev_off, k.rev.rev, N, c->cam, k.rev.part, g_act + (size_t)b0 * H * 4 + (size_t)t * 4,
                           (size_t)H * 4, t > 0 ? k.rev.g_state + (size_t)(t - 1) * pn * 3 : (double*)nullptr,
                           t > 0 && given.seed ? k.seed_mid + (size_t)(t - 1) * pn * 3 : (const double*)nullptr);
        HIPCHK(c, hipGetLastError());
    }
    if (grad_state_out) CHK(f64_copy_state_grad(c, k.rev.g_state, b0, bc, N, H, grad_state_out));
    return DRP_OK;
}

// ---- the trainer's gradients --------------------------------------------------------------------------------------------
// ka64_match on grid (samples, steps): its dynamic LDS at the cap is above what a function may use unasked, so the context sets
// the function's attribute once, at first use
int ka64_run(drp_ctx* c, dim3 grid, const Ka64Args& a) {
    if (!c->ka64_ready) {
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&ka64_match), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)KA64_LDS(KA_MAX_POINTS)));
        c->ka64_ready = true;
    }
    ka64_launch(grid, c->stream, a);
    return DRP_OK;
}

// a chunk's workspace: the shared parts, then the weight gradients' operands and accumulators (wg's; the chunk fills in the rest)
struct Tr64Ws {
    F64Tape tape;
    F64Rev rev;
    F64Wgrad wg;
    double *div_vals, *div_gsum;    // the Sinkhorn divergence: kd64_sweeps' scratch, the table's two scratch rows at B = bc
    size_t carve(void* base, size_t bc, size_t N, size_t H, const TrShape& shape) {  // -> its bytes
        F64Carver a{static_cast<char*>(base)};
        const size_t pn = bc * N, en = pn * DRP_K;
        const TrBlocks t = tr_blocks(shape, (int)bc, (int)H, (int)N, false, true);
        tape.carve(a, pn, H);
        rev.carve(a, bc, N, H, 0);
        a.take(wg.pr_h, pn * 64); a.take(wg.pr_gh, pn * 64); a.take(wg.pe_h, pn * 64); a.take(wg.pe_gh, pn * 64); a.take(wg.pe_in, pn * 5);
        a.take(wg.re_h1, en * 64); a.take(wg.re_h2, en * 64); a.take(wg.re_g1, en * 64); a.take(wg.re_g2, en * 64); a.take(wg.re_in, en * 6);
        a.take(wg.acc, bc * (size_t)W_TOTAL);
        a.take(div_vals, t.count[TRB_VALS]); a.take(div_gsum, t.count[TRB_GSUM]);
        return a.off;
    }
};

// the batch on the device beside the loss's blocks (train_host.h: TrView): the caller's arrays with a_cur = attrs[:, 0] gathered,
// and the weight-gradient sums
struct Tr64Io {
    const float *states, *sdelta, *attr, *dens;     // sdelta: the impulses [B][H][N][3], or with `actions` the pushes [B][H][4]
    bool actions;
    const int* nums;
    double* total;                  // [W_TOTAL]
    bool predict;                   // the forward alone: the chunk's predictions to the caller, no loss, nothing reversed
};

// Every step's loss term and its seed of the reverse pass for the samples [b0, b0 + bc): whatever the kind, the same slot of the
// stream, the same grid (bc, H), the same seed buffer and terms; p and the seed are the chunk's (the tape's own double states),
// every block of `v` the BATCH's (the kernels index them by b_off + b)
int tr64_launch_loss(drp_ctx* c, const Tr64Ws& k, const Tr64Io& io, const TrLoss& lk, const TrView& v, int b0, int bc, int N, int B, int H) {
    hipStream_t st = c->stream;
    const size_t pn = (size_t)bc * N;
    const double scale = 1.0 / ((double)H * (double)B);
    const dim3 grid(bc, H);
    if (lk.given()) {                   // the caller's seed at the chunk's sample offset, no term
        hipLaunchKernelGGL(k64_seed_given, grid, dim3(256), 0, st, static_cast<const double*>(v.seed), io.nums, b0, bc, N, H, k.rev.g_state);
        return DRP_OK;
    }
    if (lk.kind == TR_LOSS_MSE) {
        hipLaunchKernelGGL(kt64_mse, grid, dim3(256), 0, st, k.tape.state, io.states, io.nums, b0, bc, B, N, H, v.terms, k.rev.g_state);
        return DRP_OK;
    }
    // slice t + 1 of the tape's states against step t of the target clouds
    const CloudPair cp = tr_cloud_pair((size_t)N * 3, pn * 3, io.nums, v.targets, v.tnums, H, N, lk.M);
    if (lk.divergence()) {              // the plans from the tape's own double states (k_sinkhorn.h)
        SkArgs64 a{};
        a.cp = cp; a.pred = k.tape.state + pn * 3;
        a.b_off = b0; a.B = B;
        a.eps = v.eps; a.iters = lk.iters;
        a.scale = scale;
        a.vals = k.div_vals; a.gsum = k.div_gsum;
        a.grad = k.rev.g_state; a.terms = v.terms; a.col_err = v.col_err; a.self_err = v.self_err;
        if (lk.unbalanced()) {
            a.rho = v.rho; a.mass_q = v.mass_q; a.transported = v.transported;
            hipLaunchKernelGGL(kd64_sweeps_unbalanced, dim3(bc, H, 3), dim3(KT_THREADS), 0, st, a);
            hipLaunchKernelGGL(kd64_combine_unbalanced, grid, dim3(KD_COMBINE_THREADS), 0, st, a);
        } else {
            hipLaunchKernelGGL(kd64_sweeps, dim3(bc, H, 3), dim3(KT_THREADS), 0, st, a);
            hipLaunchKernelGGL(kd64_combine, grid, dim3(KD_COMBINE_THREADS), 0, st, a);
        }
        return DRP_OK;
    }
    if (lk.chamfer()) {                 // the arg-mins taken here in double
        Kc64Args a{};
        a.cp = cp; a.p64 = k.tape.state + pn * 3;
        a.b_off = b0; a.B = B;
        a.scale = scale;
        a.grad = k.rev.g_state; a.terms = v.terms; a.margin = v.margin;
        hipLaunchKernelGGL((kc64_chamfer<true>), grid, dim3(KC64_THREADS), 0, st, a);
    }
    if (lk.match()) {
        // the assignment solved here in double (k_match_f64.h), the term and the seed on the caller's pairs where there are any.  The
        // mix: behind a Chamfer-only step's terms and seed the kernel turns each element into (1 - w) x it + w x its own share, in
        // double: one writer per element, stream order (the fp32 trainer's scheme)
        Ka64Args a{};
        a.cp = cp; a.pred = k.tape.state + pn * 3;
        a.b_off = b0; a.B = B;
        a.scale = lk.chamfer() ? scale * lk.match_weight : scale;
        a.keep = lk.chamfer() ? 1.0 - lk.match_weight : 0.0;
        a.match_in = v.match_in;
        a.grad = k.rev.g_state; a.terms = v.terms; a.match_pq = v.match; a.cost = v.cost;
        CHK(ka64_run(c, grid, a));
    }
    return DRP_OK;
}

// forward with tape, loss, reverse pass with weight gradients of the samples [b0, b0 + bc): launches and the state gradient's copy
// (io.predict: grad_state_out receives the predictions [B][H][N][3] instead -- the tape's slices 1..H lie as the seed does)
int tr64_chunk(drp_ctx* c, const Tr64Ws& k, const Tr64Io& io, const TrLoss& lk, const TrView& v, int b0, int bc, int N, int B, int H,
               double* grad_state_out) {
    hipStream_t st = c->stream;
    const size_t pn = (size_t)bc * N;
    const dim3 lin3((unsigned)((pn * 3 + 255) / 256));
    const float* attr = io.attr + (size_t)b0 * N;
    const float* dens = io.dens + b0;
    hipLaunchKernelGGL(kt64_init_state, lin3, dim3(256), 0, st, io.states, b0, N, H, (long)(pn * 3), k.tape.state);
    // ---- forward: the impulse is data, or the batch's push on the step's own input (padded rows zero)
    CHK(f64_tape_forward(c, k.tape, bc, N, H, attr, dens, true, [&](int t, const F64Tape& s) {
        if (io.actions)
            hipLaunchKernelGGL(kt64_sdelta_actions, dim3(bc), dim3(256), 0, st, s.state, io.sdelta, io.nums, b0, N, H, t, c->cam, s.sd,
                               ptr<float>(c->ws.s_in), ptr<float>(c->ws.s_delta));
        else
            hipLaunchKernelGGL(kt64_stage_step, lin3, dim3(256), 0, st, s.state, io.sdelta, b0, N, H, t, (long)(pn * 3), s.sd,
                               ptr<float>(c->ws.s_in), ptr<float>(c->ws.s_delta));
    }));
    if (io.predict) return f64_copy_state_grad(c, k.tape.state + pn * 3, b0, bc, N, H, grad_state_out);
    // ---- every step's loss term and its seed of the reverse pass; the samples' accumulators start at zero
    CHK(tr64_launch_loss(c, k, io, lk, v, b0, bc, N, B, H));
    HIPCHK(c, hipMemsetAsync(k.wg.acc, 0, (size_t)bc * W_TOTAL * sizeof(double), st));
    F64Wgrad wg = k.wg;
    wg.st = st; wg.bc = bc; wg.N = N; wg.dens = dens;
    // ---- reverse pass, step by step; its tail: the step's share of d loss / d input state on top of the loss's seed
    for (int t = H - 1; t >= 0; --t) {
        const F64Tape s = k.tape.step(t, pn);
        const double* g_out = k.rev.g_state + (size_t)t * pn * 3;
        f64_reverse_step(c, s, k.rev, g_out, t, bc, N, attr, dens, &wg);
        if (t > 0)
            hipLaunchKernelGGL(kt64_state_bwd, dim3((unsigned)((pn + 255) / 256)), dim3(256), 0, st, g_out, k.rev.g_diff, s.cnt,
                               k.rev.rev_off, k.rev.rev, N, bc * N, k.rev.g_state + (size_t)(t - 1) * pn * 3);
        if (t > 0 && io.actions)            // the push's share, on top of that sum
            hipLaunchKernelGGL(kt64_push_bwd, dim3(bc), dim3(256), 0, st, s.state, io.sdelta, io.nums, b0, N, H, t, c->cam, k.rev.g_sd,
                               k.rev.g_state + (size_t)(t - 1) * pn * 3);
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(kt64_total, dim3((W_TOTAL + 255) / 256), dim3(256), 0, st, k.wg.acc, bc, io.total);
    HIPCHK(c, hipGetLastError());
    if (grad_state_out) CHK(f64_copy_state_grad(c, k.rev.g_state, b0, bc, N, H, grad_state_out));
    return DRP_OK;
}

}  // namespace

// drp_gd_grad_f64, drp_gd_predict_f64 and drp_gd_grad_f64_seeded: one body.  `seed` (host, [B][H][N][3]) / `predict`: what
// takes the reward's place (Gd64Given); neither reads the goal
static int gd_grad_f64_body(drp_ctx* c, const float* s0, const float* attr, const float* dens, int nb, int N, const float* actions, int B,
                            int H, const double* seed, bool predict, double* rewards_out, double* grad_act_out, double* grad_state_out) {
    const bool goal = !seed && !predict;
    CHK(need(c, true, true, goal));
    CHK(check_bn(c, B, N));
    if (!s0 || !attr || !dens || !actions) return fail(c, DRP_EINVAL, "null argument");
    if (H < 1 || H > 64) return fail(c, DRP_EINVAL, "bad horizon H=%d", H);
    if (nb <= 0 || B % nb != 0) return fail(c, DRP_EINVAL, "B must be a multiple of n_batch");
    HIPCHK(c, hipSetDevice(c->device));
    F64Scope scope(c);
    if (!c->f64_w_valid) CHK(f64_refresh_weights(c));
    // rows per chunk: tape, reverse pass and reward scratch together
    const size_t M = goal ? (size_t)c->goal_m : 0;
    Gd64Ws k{};
    auto bytes_of = [&](size_t bc) { return k.carve(nullptr, bc, (size_t)N, (size_t)H, M, seed != nullptr); };
    size_t Bc;
    CHK(f64_size_chunks(c, B, N, ((size_t)1 << 24) / (size_t)N, bytes_of, &Bc));
    k.carve(c->grad64_ws.p, Bc, (size_t)N, (size_t)H, M, seed != nullptr);
    // the whole batch's inputs (attributes and densities per row: row = traj * nb + batch) and results
    const size_t n_s0 = (size_t)nb * N * 3, n_attr = (size_t)B * N, n_act = (size_t)B * H * 4;
    std::vector<float> host(n_s0 + n_attr + (size_t)B + n_act);
    memcpy(host.data(), s0, n_s0 * sizeof(float));
    for (int b = 0; b < B; ++b) {
        memcpy(host.data() + n_s0 + (size_t)b * N, attr + (size_t)(b % nb) * N, (size_t)N * sizeof(float));
        host[n_s0 + n_attr + b] = dens[b % nb];
    }
    memcpy(host.data() + n_s0 + n_attr + B, actions, n_act * sizeof(float));
    double* d_rew;
    const size_t n_seed = seed ? (size_t)B * H * N * 3 : 0;
    CHK(f64_upload_batch(c, host, (size_t)B + n_act + n_seed, &d_rew));
    const float* d_in = ptr<float>(c->grad64_io);
    double* d_gact = d_rew + B;
    Gd64Given given{};
    given.predict = predict;
    if (seed) {                             // the whole batch's seed behind the results, as it lies at the caller's
        HIPCHK(c, hipMemcpyAsync(d_gact + n_act, seed, n_seed * sizeof(double), hipMemcpyHostToDevice, c->stream));
        given.seed = d_gact + n_act;
    }
    for (int b0 = 0; b0 < B; b0 += (int)Bc)
        CHK(gd64_chunk(c, k, b0, std::min((int)Bc, B - b0), nb, N, H, d_in, d_in + n_s0, d_in + n_s0 + n_attr, d_in + n_s0 + n_attr + B,
                       d_rew, d_gact, grad_state_out, given));
    if (rewards_out) CHK(d2h(c, rewards_out, d_rew, (size_t)B * sizeof(double)));
    if (grad_act_out) CHK(d2h(c, grad_act_out, d_gact, n_act * sizeof(double)));
    return guarded_wait(c, nullptr);        // (the upload's host block lives until here)
}

int drp_gd_grad_f64(drp_ctx* c, const float* s0, const float* attr, const float* dens, int nb, int N, const float* actions, int B,
                    int H, double* rewards_out, double* grad_act_out, double* grad_state_out) {
    return gd_grad_f64_body(c, s0, attr, dens, nb, N, actions, B, H, nullptr, false, rewards_out, grad_act_out, grad_state_out);
}

int drp_gd_predict_f64(drp_ctx* c, const float* s0, const float* attr, const float* dens, int nb, int N, const float* actions, int B,
                       int H, double* states_out) {
    if (c && !states_out) return fail(c, DRP_EINVAL, "null buffer");
    return gd_grad_f64_body(c, s0, attr, dens, nb, N, actions, B, H, nullptr, true, nullptr, nullptr, states_out);
}

int drp_gd_grad_f64_seeded(drp_ctx* c, const float* s0, const float* attr, const float* dens, int nb, int N, const float* actions,
                           int B, int H, const double* seed, double* grad_act_out, double* grad_state_out) {
    if (c && !seed) return fail(c, DRP_EINVAL, "null seed");
    if (c && s0 && attr && dens && actions && B > 0 && N > 0 && N <= 4096 && H >= 1 && H <= 64) {
        const long bad = first_bad_plan_seed(seed, B, H, N);
        if (bad >= 0)
            return fail(c, DRP_EINVAL, "the seed of row %ld, step %ld, particle %ld is infinite or not a number", bad / ((long)H * N),
                        (bad / N) % H, bad % N);
    }
    return gd_grad_f64_body(c, s0, attr, dens, nb, N, actions, B, H, seed, false, nullptr, grad_act_out, grad_state_out);
}

namespace {
// drp_train_grad_f64, drp_train_grad_f64_actions and drp_train_grad_f64_untracked: one body; `impulses` is states_delta
// [B][H][N][3], or with `actions` the pushes [B][H][4]; the loss kind and the targets in `lk` (capi_train.h: TrLoss) -- the tracked
// MSE, the Chamfer loss against untracked target clouds (k_chamfer_f64.h), or the Sinkhorn divergence to them
// (k_sinkhorn.h), or the matching kinds (k_match_f64.h: the matching term, or its mix with the Chamfer term); the transport
// loss has no yardstick
int train_grad_f64_body(drp_ctx* c, const float* states, const float* impulses, bool actions, const float* attrs,
                        const int32_t* particle_nums, const float* particle_dens, int B, int N, int n_rollout, const TrLoss& lk,
                        double* loss_out, double* loss_terms_out, double* grad_out, double* grad_state_out,
                        double* pred_out = nullptr /* drp_train_predict_f64: the forward alone, every step's prediction [B][H][N][3] */) {
    CHK(need(c, true, actions, false));
    if (lk.transport()) return fail(c, DRP_EINVAL, "no float64 yardstick for loss kind %d", lk.kind);
    CHK(check_bn(c, B, N));
    if (!states || !impulses || !attrs || !particle_nums || !particle_dens) return fail(c, DRP_EINVAL, "null argument");
    if (n_rollout < 1 || n_rollout > 64) return fail(c, DRP_EINVAL, "bad n_rollout=%d", n_rollout);
    CHK(check_particle_nums(c, particle_nums, B, N));
    if (lk.chamfer() || lk.match()) {
        CHK(check_target_clouds(c, lk, lk.chamfer() ? KC64_MAX_POINTS : KA_MAX_POINTS, "shape"));
        if (lk.match()) CHK(check_match_loss(c, lk, N));
        CHK(check_target_nums(c, lk, B, n_rollout));
    }
    if (lk.match() && lk.match_in)          // [H][B][N]: drp_train_step_loss's match_out layout
        for (int t = 0; t < n_rollout; ++t)
            for (int b = 0; b < B; ++b) {
                int row;
                const int why = check_matching(lk.match_in + ((size_t)t * B + b) * N, particle_nums[b],
                                               lk.target_nums[(size_t)b * n_rollout + t], N, &row);
                if (why != MATCH_OK)
                    return fail(c, DRP_EINVAL, "match_in: sample %d step %d row %d %s", b, t, row, matching_fault(why));
            }
    if (lk.divergence()) {
        CHK(check_target_clouds(c, lk, KT_MAX_POINTS, "shape"));
        if (N > KT_MAX_POINTS) return fail(c, DRP_EINVAL, "the Sinkhorn divergence takes at most %d points per cloud (N=%d)", KT_MAX_POINTS, N);
        CHK(check_target_nums(c, lk, B, n_rollout));
        CHK(check_transport_params(c, lk.eps, B, lk.iters));
        if (lk.unbalanced()) CHK(check_reach_params(c, lk.eps, lk.rho, lk.mass_q, B, n_rollout));
    }
    if (actions) CHK(check_pushes(c, impulses, B, n_rollout));
    if (lk.given()) {
        if (!lk.seed64) return fail(c, DRP_EINVAL, "null argument");
        const long bad = first_bad_seed(lk.seed64, particle_nums, B, n_rollout, N);
        if (bad >= 0)
            return fail(c, DRP_EINVAL, "seed: sample %d step %d row %d is not finite", (int)(bad / N / n_rollout),
                        (int)(bad / N % n_rollout), (int)(bad % N));
    }
    HIPCHK(c, hipSetDevice(c->device));
    F64Scope scope(c);
    if (!c->f64_w_valid) CHK(f64_refresh_weights(c));
    const int H = n_rollout;
    // samples per chunk: tape, reverse pass, weight gradients' operands and accumulators together
    Tr64Ws k{};
    const TrShape shape = lk.shape();
    auto bytes_of = [&](size_t bc) { return k.carve(nullptr, bc, (size_t)N, (size_t)H, shape); };
    size_t Bc;
    CHK(f64_size_chunks(c, B, N, ((size_t)1 << 24) / ((size_t)N * DRP_K), bytes_of, &Bc));
    k.carve(c->grad64_ws.p, Bc, (size_t)N, (size_t)H, shape);
    // the whole batch's inputs in one upload and the results behind them (train_host.h: tr_blocks; of the attributes a_cur = attrs[:, 0])
    const TrBlocks lay = tr_blocks(shape, B, H, N, actions, true);
    std::vector<float> host(lay.bytes / sizeof(float));
    char* const up = reinterpret_cast<char*>(host.data());
    memcpy(up + lay.off[TRB_STATES], states, lay.size(TRB_STATES));
    memcpy(up + lay.off[TRB_IMPULSES], impulses, lay.size(TRB_IMPULSES));
    for (int b = 0; b < B; ++b)
        memcpy(up + lay.off[TRB_ATTRS] + (size_t)b * N * sizeof(float), attrs + (size_t)b * (H + 1) * N, (size_t)N * sizeof(float));
    memcpy(up + lay.off[TRB_DENS], particle_dens, lay.size(TRB_DENS));
    memcpy(up + lay.off[TRB_NUMS], particle_nums, lay.size(TRB_NUMS));
    tr_stage_loss_inputs(up, lay, lk);
    double* res;
    CHK(f64_upload_batch(c, host, lay.res_bytes / sizeof(double), &res));
    const TrView v = tr_view(c->grad64_io.p, res, lay);
    auto staged = [&](int id) { return reinterpret_cast<const float*>(static_cast<const char*>(c->grad64_io.p) + lay.off[id]); };
    const Tr64Io io{staged(TRB_STATES), staged(TRB_IMPULSES), staged(TRB_ATTRS), staged(TRB_DENS), actions,
                    reinterpret_cast<const int*>(staged(TRB_NUMS)), v.total, pred_out != nullptr};
    HIPCHK(c, hipMemsetAsync(io.total, 0, (size_t)W_TOTAL * sizeof(double), c->stream));
    for (int b0 = 0; b0 < B; b0 += (int)Bc)
        CHK(tr64_chunk(c, k, io, lk, v, b0, std::min((int)Bc, B - b0), N, B, H, io.predict ? pred_out : grad_state_out));
    if (io.predict) return guarded_wait(c, nullptr);        // (the upload's host block lives until here)
    const size_t n_terms = lay.count[TRB_TERMS];
    std::vector<double> terms(n_terms);
    if (!lk.given()) CHK(d2h(c, terms.data(), v.terms, n_terms * sizeof(double)));      // (a given seed has no terms: none were written)
    if (grad_out) CHK(d2h(c, grad_out, io.total, (size_t)W_TOTAL * sizeof(double)));
    CHK(tr_read_results(lay, res, lk, [c](void* dst, const void* src, size_t n) { return d2h(c, dst, src, n); }));
    CHK(guarded_wait(c, nullptr));          // (the upload's host block lives until here)
    if (loss_terms_out) memcpy(loss_terms_out, terms.data(), n_terms * sizeof(double));
    if (loss_out) {
        double total = 0.0;                 // fixed order: step-major, then sample (as drp_train_step)
        for (size_t q = 0; q < n_terms; ++q) total += terms[q];
        *loss_out = total;
    }
    return DRP_OK;
}
}  // namespace

int drp_train_grad_f64(drp_ctx* c, const float* states, const float* states_delta, const float* attrs, const int32_t* particle_nums,
                       const float* particle_dens, int B, int N, int n_rollout, double* loss_out, double* loss_terms_out,
                       double* grad_out, double* grad_state_out) {
    return train_grad_f64_body(c, states, states_delta, false, attrs, particle_nums, particle_dens, B, N, n_rollout, TrLoss{},
                               loss_out, loss_terms_out, grad_out, grad_state_out);
}

// the float64 forward alone, and the reverse pass from a seed of the caller's: train_grad_f64_body with TR_LOSS_GIVEN
int drp_train_predict_f64(drp_ctx* c, const float* states, const float* states_delta, const float* actions, const float* attrs,
                          const int32_t* particle_nums, const float* particle_dens, int B, int N, int n_rollout,
                          double* states_pred_out) {
    if (!c) return DRP_EINVAL;
    ImpulseSource src;
    CHK(impulse_source(c, states_delta, actions, src));
    if (!states_pred_out) return fail(c, DRP_EINVAL, "null argument");
    return train_grad_f64_body(c, states, src.impulses, src.by_actions, attrs, particle_nums,
                               particle_dens, B, N, n_rollout, TrLoss{}, nullptr, nullptr, nullptr, nullptr, states_pred_out);
}

int drp_train_grad_f64_seeded(drp_ctx* c, const float* states, const float* states_delta, const float* actions, const float* attrs,
                              const int32_t* particle_nums, const float* particle_dens, int B, int N, int n_rollout,
                              const double* seed, double* grad_out, double* grad_state_out) {
    if (!c) return DRP_EINVAL;
    ImpulseSource src;
    CHK(impulse_source(c, states_delta, actions, src));
    TrLoss lk;
    lk.kind = TR_LOSS_GIVEN; lk.seed64 = seed;
    return train_grad_f64_body(c, states, src.impulses, src.by_actions, attrs, particle_nums,
                               particle_dens, B, N, n_rollout, lk, nullptr, nullptr, grad_out, grad_state_out);
}

int drp_train_grad_f64_actions(drp_ctx* c, const float* states, const float* actions, const float* attrs,
                               const int32_t* particle_nums, const float* particle_dens, int B, int N, int n_rollout,
                               double* loss_out, double* loss_terms_out, double* grad_out, double* grad_state_out) {
    return train_grad_f64_body(c, states, actions, true, attrs, particle_nums, particle_dens, B, N, n_rollout, TrLoss{}, loss_out,
                               loss_terms_out, grad_out, grad_state_out);
}

int drp_train_grad_f64_untracked(drp_ctx* c, const float* states, const float* states_delta, const float* actions,
                                 const float* attrs, const int32_t* particle_nums, const float* particle_dens, int B, int N,
                                 int n_rollout, const float* targets, const int32_t* target_nums, int M, double* loss_out,
                                 double* loss_terms_out, double* grad_out, double* grad_state_out, double* margin_out) {
    if (!c) return DRP_EINVAL;
    ImpulseSource src;
    CHK(impulse_source(c, states_delta, actions, src));
    TrLoss lk = TrLoss::against(TR_LOSS_CHAMFER, targets, target_nums, M);
    lk.margin_out = margin_out;
    return train_grad_f64_body(c, states, src.impulses, src.by_actions, attrs, particle_nums,
                               particle_dens, B, N, n_rollout, lk, loss_out, loss_terms_out, grad_out, grad_state_out);
}
