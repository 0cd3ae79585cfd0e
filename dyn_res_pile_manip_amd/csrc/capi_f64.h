// capi_f64.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the float64 evaluation of one step (drp_forward_f64, drp_step_f64, drp_f64_tap; kernels: k_prop_f64.h) and the accuracy
// probe that holds an engine against it (drp_accuracy_probe).  Not an engine of drp_set_engine: no plan, no dispatch variant.

namespace {

// While a *_f64 call runs, the step workspace the one-shot entry points stage their inputs in (and run_step / launch_graph
// work in) is the surface's OWN (c->f64_ws): the context's is swapped out whole and comes back untouched when the scope ends, so
// a planner session whose state lives in it goes on as if nothing had happened.  The same holds for what a step leaves behind
// on the host side (StepMarks: the dispatch marks, the shapes of the last call, the probed class) and the degree statistic.
struct F64Scope {
    drp_ctx* c;
    StepMarks marks;
    unsigned long long deg_val = 0;
    explicit F64Scope(drp_ctx* ctx) : c(ctx), marks(ctx->marks) {
        if (c->deg_stat.p) deg_val = *ptr<volatile unsigned long long>(c->deg_stat);
        c->marks.probe_cls = -1;
        std::swap(c->ws, c->f64_ws);
    }
    ~F64Scope() {
        (void)guarded_wait(c, nullptr);         // nothing of this call is in flight when the buffers change hands again
        std::swap(c->ws, c->f64_ws);
        if (c->deg_stat.p) *ptr<volatile unsigned long long>(c->deg_stat) = deg_val;
        c->marks = marks;
    }
};

int f64_check_inputs(drp_ctx* c, const float* a_cur, const float* s_cur, const float* s_delta, const float* dens, int B, int N) {
    CHK(need(c, true, false, false));
    CHK(check_bn(c, B, N));
    if (!a_cur || !s_cur || !s_delta || !dens) return fail(c, DRP_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    return DRP_OK;
}

// the four inputs into the (scope's) step workspaces, as step_common stages them
int f64_upload(drp_ctx* c, const float* a_cur, const float* s_cur, const float* s_delta, const float* dens, int B, int N, int engine) {
    const size_t bn = (size_t)B * N;
    CHK(ensure_step_ws(c, c->ws, B, N, engine));
    CHK(h2d(c, c->ws.s_in, s_cur, bn * 3 * sizeof(float)));
    CHK(h2d(c, c->ws.s_delta, s_delta, bn * 3 * sizeof(float)));
    CHK(h2d(c, c->ws.attr, a_cur, bn * sizeof(float)));
    CHK(h2d(c, c->ws.dens, dens, (size_t)B * sizeof(float)));
    return DRP_OK;
}

// the library's own fp32 graph build on the staged inputs (as drp_build_graph): lists into the workspace
int f64_build_lists(drp_ctx* c, int B, int N) {
    const GraphPlan g = plan_graph(c->pol, c->n_cu, c->engine, B, N, false, false, false, true);
    launch_graph(c, c->stream, g, ptr<float>(c->ws.s_in), B, (size_t)N * 3, (const float*)nullptr, (size_t)0, ptr<float>(c->ws.s_delta), B, N,
                 ptr<int16_t>(c->ws.nbr_idx), ptr<uint8_t>(c->ws.nbr_cnt), 0);
    HIPCHK(c, hipGetLastError());
    return DRP_OK;
}

// The launches of one step over `rows` particles (whole samples of N): its intermediates into pe [rows,64], re [rows,10,64],
// eff and agg [3][rows,64], erel [3][rows,10,64], pred [rows,3], the new positions into s_pred [rows,3].  TS: the type of the
// positions and impulses, float (the one-step calls) or double (the rollouts of capi_grad_f64.h, whose intermediates are its tape).
extern "C++" template <typename TS>
void f64_launch_step(drp_ctx* c, const double* w, const TS* s_cur, const TS* s_delta, const float* attr, const float* dens,
                     const int16_t* idx, const uint8_t* cnt, int N, int rows, double* pe, double* re, double* eff, double* agg,
                     double* erel, double* pred, double* s_pred) {
    const int erows = rows * DRP_K;
    const dim3 blk(64 * KF_WAVES);
    const dim3 pgrid((rows + 16 * KF_WAVES - 1) / (16 * KF_WAVES)), egrid((erows + 16 * KF_WAVES - 1) / (16 * KF_WAVES));
    const size_t p64 = (size_t)rows * 64, e64 = (size_t)erows * 64;      // a propagation step's slice of the effects / relation effects
    hipStream_t st = c->stream;
    hipLaunchKernelGGL((kf_particle_encode<TS>), pgrid, blk, 0, st, w, s_delta, attr, dens, N, rows, pe);
    hipLaunchKernelGGL((kf_relation_encode<TS>), egrid, blk, 0, st, w, s_cur, attr, dens, idx, cnt, N, erows, re);
    for (int p = 0; p < DRP_PSTEP; ++p) {
        const double* eff_prev = p == 0 ? pe : eff + (size_t)(p - 1) * p64;
        hipLaunchKernelGGL(kf_relation_prop, egrid, blk, 0, st, w, re, eff_prev, dens, idx, cnt, N, erows, erel + (size_t)p * e64);
        hipLaunchKernelGGL(kf_particle_prop, pgrid, blk, 0, st, w, pe, erel + (size_t)p * e64, eff_prev, dens, cnt, N, rows,
                           agg + (size_t)p * p64, eff + (size_t)p * p64);
    }
    hipLaunchKernelGGL((kf_predict<TS>), pgrid, blk, 0, st, w, eff + (size_t)(DRP_PSTEP - 1) * p64, s_cur, rows, pred, s_pred);
}

// model/gnn_dyn.py:147-198 in float64 on the staged inputs and lists -> c->f64_out [B,N,3]; launches only.
// Samples are independent and a row's arithmetic does not know its tile: walking the batch in chunks changes no bit.
int f64_forward_dev(drp_ctx* c, int B, int N) {
    if (!c->f64_w_valid) CHK(f64_refresh_weights(c));
    const size_t per_sample = (size_t)N * KF_BYTES_PER_PARTICLE;
    const size_t fit = std::max<size_t>(1, c->f64_cap / per_sample);
    const int Bc = (int)std::min<size_t>({(size_t)B, fit, std::max<size_t>(1, ((size_t)1 << 24) / (size_t)N)});
    const size_t pn = (size_t)Bc * N;
    CHK(ensure(c, c->f64_pe, pn * 64 * sizeof(double)));
    CHK(ensure(c, c->f64_eff, pn * 3 * 64 * sizeof(double)));
    CHK(ensure(c, c->f64_agg, pn * 3 * 64 * sizeof(double)));
    CHK(ensure(c, c->f64_re, pn * DRP_K * 64 * sizeof(double)));
    CHK(ensure(c, c->f64_erel, pn * 3 * DRP_K * 64 * sizeof(double)));
    CHK(ensure(c, c->f64_pred, pn * 3 * sizeof(double)));
    CHK(ensure(c, c->f64_out, (size_t)B * N * 3 * sizeof(double)));
    const double* w = ptr<double>(c->f64_w);
    int chunks = 0;
    for (int b0 = 0; b0 < B; b0 += Bc, ++chunks) {
        const int bc = std::min(Bc, B - b0);
        const int rows = bc * N;
        const size_t ro = (size_t)b0 * N;
        const float* s_cur = ptr<float>(c->ws.s_in) + ro * 3;
        const float* s_delta = ptr<float>(c->ws.s_delta) + ro * 3;
        const float* attr = ptr<float>(c->ws.attr) + ro;
        const float* dens = ptr<float>(c->ws.dens) + b0;
        const int16_t* idx = ptr<int16_t>(c->ws.nbr_idx) + ro * DRP_K;
        const uint8_t* cnt = ptr<uint8_t>(c->ws.nbr_cnt) + ro;
        f64_launch_step<float>(c, w, s_cur, s_delta, attr, dens, idx, cnt, N, rows, ptr<double>(c->f64_pe), ptr<double>(c->f64_re),
                               ptr<double>(c->f64_eff), ptr<double>(c->f64_agg), ptr<double>(c->f64_erel), ptr<double>(c->f64_pred),
                               ptr<double>(c->f64_out) + ro * 3);
        HIPCHK(c, hipGetLastError());
    }
    c->f64_lastB = B; c->f64_lastN = N; c->f64_chunks = chunks;
    return DRP_OK;
}

int f64_finish(drp_ctx* c, int B, int N, double* s_pred_out) {
    CHK(d2h(c, s_pred_out, c->f64_out.p, (size_t)B * N * 3 * sizeof(double)));
    return guarded_wait(c, nullptr);
}

}  // namespace

int drp_forward_f64(drp_ctx* c, const float* a_cur, const float* s_cur, const float* s_delta, const float* dens,
                    const int16_t* nbr_idx, const uint8_t* nbr_cnt, int B, int N, double* s_pred_out) {
    CHK(f64_check_inputs(c, a_cur, s_cur, s_delta, dens, B, N));
    if (!nbr_idx || !nbr_cnt || !s_pred_out) return fail(c, DRP_EINVAL, "null buffer");
    const size_t bn = (size_t)B * N;
    for (size_t r = 0; r < bn; ++r) {
        if (nbr_cnt[r] > DRP_K) return fail(c, DRP_EINVAL, "neighbour count %d of row %zu above %d", (int)nbr_cnt[r], r, DRP_K);
        for (int k = 0; k < (int)nbr_cnt[r]; ++k)
            if (nbr_idx[r * DRP_K + k] < 0 || nbr_idx[r * DRP_K + k] >= N)
                return fail(c, DRP_EINVAL, "neighbour list entry %d of row %zu outside 0..%d", (int)nbr_idx[r * DRP_K + k], r, N - 1);
    }
    F64Scope scope(c);
    CHK(f64_upload(c, a_cur, s_cur, s_delta, dens, B, N, -1));
    CHK(h2d(c, c->ws.nbr_idx, nbr_idx, bn * DRP_K * sizeof(int16_t)));
    CHK(h2d(c, c->ws.nbr_cnt, nbr_cnt, bn));
    CHK(f64_forward_dev(c, B, N));
    return f64_finish(c, B, N, s_pred_out);
}

int drp_step_f64(drp_ctx* c, const float* a_cur, const float* s_cur, const float* s_delta, const float* dens, int B, int N,
                 double* s_pred_out) {
    CHK(f64_check_inputs(c, a_cur, s_cur, s_delta, dens, B, N));
    if (!s_pred_out) return fail(c, DRP_EINVAL, "null buffer");
    F64Scope scope(c);
    CHK(f64_upload(c, a_cur, s_cur, s_delta, dens, B, N, -1));
    CHK(f64_build_lists(c, B, N));
    CHK(f64_forward_dev(c, B, N));
    return f64_finish(c, B, N, s_pred_out);
}

int drp_f64_tap(drp_ctx* c, const char* name, double* out, size_t n) {
    if (!c || !name || !out) return DRP_EINVAL;
    if (c->f64_chunks < 1) return fail(c, DRP_ESTATE, "no *_f64 call yet");
    if (c->f64_chunks > 1)
        return fail(c, DRP_ESTATE, "the last *_f64 call walked its batch in %d chunks: the intermediates of one chunk only remain "
                    "(raise the workspace cap or tap a smaller batch)", c->f64_chunks);
    const size_t pn = (size_t)c->f64_lastB * c->f64_lastN;
    // particle_encode and relation_encode stand where the factored engines keep c_node and c_edge: both names are taken
    const char* const per_step[3] = {"effect_rel_", "agg_", "effect_"};
    const void* src = nullptr;
    size_t count = 0;
    if (!strcmp(name, "particle_encode") || !strcmp(name, "c_node")) { src = c->f64_pe.p; count = pn * 64; }
    else if (!strcmp(name, "relation_encode") || !strcmp(name, "c_edge")) { src = c->f64_re.p; count = pn * DRP_K * 64; }
    else if (!strcmp(name, "particle_pred")) { src = c->f64_pred.p; count = pn * 3; }
    else {
        const char* rest = !strncmp(name, "particle_effect_", 16) ? name + 9 : name;       // particle_effect_p: the fixture's name of effect_p
        for (int q = 0; q < 3 && !src; ++q) {
            const size_t l = strlen(per_step[q]);
            if (strncmp(rest, per_step[q], l) || rest[l] < '0' || rest[l] >= '0' + DRP_PSTEP || rest[l + 1]) continue;
            const size_t p = (size_t)(rest[l] - '0');
            if (q == 0) { count = pn * DRP_K * 64; src = ptr<double>(c->f64_erel) + p * count; }
            else { count = pn * 64; src = ptr<double>(q == 1 ? c->f64_agg : c->f64_eff) + p * count; }
        }
    }
    if (!src) return fail(c, DRP_EINVAL, "unknown float64 tap '%s'", name);
    if (n != count) return fail(c, DRP_EINVAL, "float64 tap '%s' holds %zu doubles, not %zu", name, count, n);
    HIPCHK(c, hipSetDevice(c->device));
    CHK(d2h(c, out, src, count * sizeof(double)));
    return guarded_wait(c, nullptr);
}

int drp_debug_set_f64_cap(drp_ctx* c, size_t bytes) {
    if (!c) return DRP_EINVAL;
    c->f64_cap = bytes ? bytes : (size_t)256 << 20;
    return DRP_OK;
}

int drp_accuracy_probe(drp_ctx* c, int engine, const float* a_cur, const float* s_cur, const float* s_delta, const float* dens,
                       int B, int N, double out[4]) {
    CHK(f64_check_inputs(c, a_cur, s_cur, s_delta, dens, B, N));
    if (!out) return fail(c, DRP_EINVAL, "null buffer");
    if (engine != DRP_ENGINE_VALU && engine != DRP_ENGINE_MFMA && engine != DRP_ENGINE_SPLIT && engine != DRP_ENGINE_FUSED &&
        engine != DRP_ENGINE_LITE)
        return fail(c, DRP_EINVAL, "engine %d not available in this build", engine);
    F64Scope scope(c);
    // drp_step's path on that engine: the range check, the lists from the graph build, the step
    CHK(range_check(c, engine, max_abs(a_cur, (size_t)B * N), max_abs(dens, (size_t)B), max_abs(s_delta, (size_t)B * N * 3)));
    CHK(f64_upload(c, a_cur, s_cur, s_delta, dens, B, N, engine));
    const size_t bn = (size_t)B * N;
    CHK(ensure(c, c->ws.s_out, bn * 3 * sizeof(float)));
    StepArgs a = step_args(c, engine);
    a.s_prev = ptr<float>(c->ws.s_in); a.prev_mod = B; a.prev_stride = (size_t)N * 3;
    a.attr = ptr<float>(c->ws.attr); a.attr_mod = B;
    a.dens = ptr<float>(c->ws.dens); a.dens_mod = B;
    a.actions = nullptr; a.act_stride = 0;
    a.build_graph = true;
    a.s_out = ptr<float>(c->ws.s_out); a.out_stride = (size_t)N * 3;
    a.B = B; a.N = N;
    CHK(run_step(c, a));
    // the float64 evaluation on the same inputs and the lists that step built
    CHK(f64_forward_dev(c, B, N));
    const long per = std::max<long>(KF_RED_THREADS, ((long)bn + KF_RED_PARTS_MAX - 1) / KF_RED_PARTS_MAX);
    const int parts = (int)(((long)bn + per - 1) / per);
    CHK(ensure(c, c->f64_red, ((size_t)parts * 3 + 4) * sizeof(double)));
    double* part = ptr<double>(c->f64_red);
    double* res = part + (size_t)parts * 3;
    for (int phase = 0; phase < 2; ++phase)
        hipLaunchKernelGGL(kf_probe_reduce, dim3(phase == 0 ? parts : 1), dim3(KF_RED_THREADS), 0, c->stream, ptr<float>(c->ws.s_out),
                           ptr<double>(c->f64_out), ptr<float>(c->ws.s_in), (long)bn, per, part, parts, res, phase);
    HIPCHK(c, hipGetLastError());
    CHK(d2h(c, out, res, 4 * sizeof(double)));
    return guarded_wait(c, nullptr);
}
