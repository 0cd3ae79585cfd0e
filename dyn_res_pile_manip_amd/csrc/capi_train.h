// capi_train.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: training on the same kernels (row f4): forward with tape, reverse mode with weight gradients, Adam, re-packing.

// ---- training on the same kernels (row f4) ------------------------------------------------------
namespace {
#define TR_GRAD_PAD ((W_TOTAL + 63) & ~63)      // tr_grad: the gradient blob, then (from here) kmb_step_bwd's barrier counters
// (train_host.h: TrLoss, the description of the loss both trainers read, and tr_blocks, the table of the blocks a call stages in
// c->tr_arena and brings back from c->tr_loss)
extern "C++" template <typename T> const T* tr_staged(const drp_ctx* c, const TrBlocks& lay, int id) {
    return reinterpret_cast<const T*>(static_cast<const char*>(c->tr_arena.p) + lay.off[id]);
}
static_assert(W_TOTAL == DRP_N_WEIGHTS, "the table's row of the float64 weight-gradient sums");
static_assert(KT_MAX_ITERS == DRP_TRANSPORT_MAX_ITERS, "include/drp.h states the kernel's cap");
// The impulse source of an entry point that takes both pointers: exactly one of states_delta and actions is given
struct ImpulseSource { const float* impulses; bool by_actions; };
int impulse_source(drp_ctx* c, const float* states_delta, const float* actions, ImpulseSource& src) {
    if ((states_delta != nullptr) == (actions != nullptr))
        return fail(c, DRP_EINVAL, "exactly one of states_delta and actions must be given");
    src.by_actions = actions != nullptr;
    src.impulses = src.by_actions ? actions : states_delta;
    return DRP_OK;
}
// ---- the checks both trainers make of a batch and its loss; each body calls them where its own order of refusals has them ----
int check_particle_nums(drp_ctx* c, const int32_t* particle_nums, int B, int N) {
    for (int b = 0; b < B; ++b)
        if (particle_nums[b] <= 0 || particle_nums[b] > N)
            return fail(c, DRP_EINVAL, "particle_nums[%d]=%d outside 1..%d", b, particle_nums[b], N);
    return DRP_OK;
}
// the target clouds are there and no larger than the loss kernel's `m_cap` (`what`: the caller's word for M) ...
int check_target_clouds(drp_ctx* c, const TrLoss& lk, int m_cap, const char* what) {
    if (!lk.targets || !lk.target_nums) return fail(c, DRP_EINVAL, "null argument");
    if (lk.M <= 0 || lk.M > m_cap) return fail(c, DRP_EINVAL, "bad %s M=%d (1..%d)", what, lk.M, m_cap);
    return DRP_OK;
}
// ... and every (sample, step) has 1..M real rows
int check_target_nums(drp_ctx* c, const TrLoss& lk, int B, int H) {
    for (int e = 0; e < B * H; ++e)
        if (lk.target_nums[e] <= 0 || lk.target_nums[e] > lk.M)
            return fail(c, DRP_EINVAL, "target_nums[%d][%d]=%d outside 1..%d", e / H, e % H, lk.target_nums[e], lk.M);
    return DRP_OK;
}
// a matching loss's sizes and the mix's weight
int check_match_loss(drp_ctx* c, const TrLoss& lk, int N) {
    if (N > KA_MAX_POINTS || lk.M > KA_MAX_POINTS)
        return fail(c, DRP_EINVAL, "a matching loss takes clouds of 1..%d points: N=%d M=%d", KA_MAX_POINTS, N, lk.M);
    if (lk.kind == TR_LOSS_CHAMFER_MATCH && !(lk.match_weight > 0.0 && lk.match_weight < 1.0))
        return fail(c, DRP_EINVAL, "match_weight %g outside (0, 1)", lk.match_weight);
    return DRP_OK;
}
// eps [B] and iters as drp_cloud_transport and drp_train_step_transport refuse them
int check_transport_params(drp_ctx* c, const double* eps, int B, int iters) {
    if (!eps) return fail(c, DRP_EINVAL, "null argument");
    const int bad = first_bad_eps(eps, B);
    if (bad >= 0) return fail(c, DRP_EINVAL, "eps[%d]=%g is not a positive finite number", bad, eps[bad]);
    if (iters < 1 || iters > KT_MAX_ITERS) return fail(c, DRP_EINVAL, "iters=%d outside 1..%d", iters, KT_MAX_ITERS);
    return DRP_OK;
}
// rho [B] and mass_q [n_steps][B] as drp_cloud_divergence_unbalanced (n_steps = 1) and drp_train_step_divergence_unbalanced
// refuse them (train_host.h: check_reach); behind check_transport_params: eps is positive and finite
int check_reach_params(drp_ctx* c, const double* eps, const double* rho, const double* mass_q, int B, int n_steps) {
    if (!rho || !mass_q) return fail(c, DRP_EINVAL, "null argument");
    for (int t = 0; t < n_steps; ++t)
        for (int b = 0; b < B; ++b) {
            const double w = mass_q[(size_t)t * B + b];
            switch (check_reach(eps[b], rho[b], w)) {
            case REACH_RHO:
                return fail(c, DRP_EINVAL, "rho[%d]=%g is neither +inf nor a finite number of at least eps[%d]/1024 = %g", b, rho[b], b,
                            eps[b] * KD_MIN_REACH_PER_EPS);
            case REACH_MASS:
                return fail(c, DRP_EINVAL, "mass_q[%d][%d]=%g outside %g..%g", t, b, w, KD_MIN_MASS, KD_MAX_MASS);
            case REACH_INF_MASS:
                return fail(c, DRP_EINVAL, "mass_q[%d][%d]=%g with rho[%d]=+inf: balanced transport needs equal masses (mass_q = 1)", t, b, w, b);
            default: break;
            }
        }
    return DRP_OK;
}
// step t of the predictions (p's strides) against step t of the target clouds [B][H][M][3] and their counts [B][H] as staged
CloudPair tr_cloud_pair(size_t p_bstride, size_t p_tstride, const int* nums, const float* targets, const int* tnums, int H, int N, int M) {
    CloudPair cp{};
    cp.p_bstride = p_bstride; cp.p_tstride = p_tstride;
    cp.q = targets; cp.q_bstride = (size_t)H * M * 3; cp.q_tstride = (size_t)M * 3;
    cp.n_p = nums;
    cp.n_q = tnums; cp.nq_bstride = H; cp.nq_tstride = 1;
    cp.N = N; cp.M = M;
    return cp;
}
// one pass over a staged batch: everything train_forward_backward reads beside the shapes and the session
struct TrainPass {
    int engine = DRP_ENGINE_FUSED;  // which engine writes the tape (pick_tape_engine)
    bool backward = false;          // false: the forward pass and the loss alone
    bool predict = false;           // with `backward`: the pass ends behind its forward -- the one a backward pass would follow, tape
                                    //   and all (drp_train_predict) -- with no loss kernel and nothing reversed
    bool defer = false;             // the weight gradients wait for the end of the pass (and the dumps have a buffer per step)
    double* loss_terms = nullptr;   // [H][B], where the loss kernel stores: c->tr_loss, or pinned host memory the caller reads
    TrBlocks lay{};                 // the call's blocks: the batch in c->tr_arena, the results in c->tr_loss (train_host.h)
    TrLoss lk;
    bool actions = false;           // the impulse source: false, data (the impulse block holds [B][H][N][3]); true, the pushes there
                                    // ([B][H][4]) evaluated on the state each step reads (kt_sdelta_actions, kb_sdelta_pos)
};
// The loss of every step and d loss / d s_pred_t (train/train_gnn_dyn.py:184-186, :203): whatever the kind, the same slot of the
// stream, the same grid (B, H), the same seed buffer and terms, and one kernel that zero-fills the gradient blob with
// kmb_step_bwd's counters behind it.  `v`: the loss's blocks in the staged batch and in c->tr_loss (train_host.h: tr_view)
void train_launch_loss(drp_ctx* c, int B, int N, const TrainPass& tp, const TrView& v) {
    const int H = c->tr_nroll;
    const TrLoss& lk = tp.lk;
    hipStream_t st = c->stream;
    const int* nums = tr_staged<int>(c, tp.lay, TRB_NUMS);
    float* states = ptr<float>(c->states);
    float* g_state = ptr<float>(c->g_state);
    double* loss = tp.loss_terms;
    const float scale = 1.0f / (float)(H * B);
    const size_t hstride = (size_t)H * N * 3;                 // predicted states [B][H][N][3]
    float* const zero = tp.backward ? ptr<float>(c->tr_grad) : (float*)nullptr;
    const size_t n_zero = (size_t)TR_GRAD_PAD + (size_t)H * c->n_cu + 1;
    const dim3 grid(B, H);
    if (lk.given()) {                   // the caller's seed as staged behind the batch
        hipLaunchKernelGGL(kt_seed_given, grid, dim3(256), 0, st, static_cast<const float*>(v.seed), nums, N, g_state, zero, n_zero);
        return;
    }
    if (lk.kind == TR_LOSS_MSE) {       // against the given next states [B][H+1][N][3]
        hipLaunchKernelGGL(kt_mse_grad, grid, dim3(256), 0, st, states, hstride, tr_staged<float>(c, tp.lay, TRB_STATES) + (size_t)N * 3,
                           (size_t)(H + 1) * N * 3, nums, N, scale, g_state, loss, zero, n_zero);
        return;
    }
    // step t of the predictions against step t of the staged target clouds
    const CloudPair cp = tr_cloud_pair(hstride, (size_t)N * 3, nums, v.targets, v.tnums, H, N, lk.M);
    if (lk.chamfer()) {
        KcArgs a{};
        a.cp = cp; a.pred = states;
        a.scale = scale;               // (the mix too: the matching kernel weighs what this one leaves, in double)
        a.grad = g_state; a.terms = loss;
        a.zero = zero; a.n_zero = n_zero;
        hipLaunchKernelGGL((kc_chamfer<true>), grid, dim3(KC_THREADS), 0, st, a);
    }
    if (lk.match()) {
        // alone: the Chamfer kernel's outputs and zero-fill; in the mix: behind it in the stream, turning the gradient and the
        // terms it finds into (1 - w) x them + its own share -- one writer per element, so the sum's order is fixed, and
        // the Chamfer share is (1 - w) x the bits of a Chamfer-only step whatever w is
        KaArgs a{};
        a.cp = cp; a.pred = states;
        a.scale = lk.chamfer() ? (double)scale * lk.match_weight : (double)scale;
        a.keep = lk.chamfer() ? 1.0 - lk.match_weight : 0.0;
        a.grad = g_state; a.terms = loss;
        a.match_pq = v.match;
        a.zero = lk.chamfer() ? (float*)nullptr : zero; a.n_zero = n_zero;
        ka_launch<true>(grid, st, a);
    }
    if (lk.sinkhorn()) {
        // the Chamfer kernel's outputs and zero-fill; a certificate is formed where the caller asked for it
        SkArgs32 a{};
        a.cp = cp; a.pred = states; a.b_off = 0; a.B = B;
        a.eps = v.eps; a.iters = lk.iters;
        a.scale = (double)scale;
        a.grad = g_state; a.terms = loss;
        a.col_err = lk.col_err_out != nullptr ? v.col_err : (double*)nullptr;
        a.zero = zero; a.n_zero = n_zero;
        if (lk.transport()) {
            hipLaunchKernelGGL((kt_transport<true>), grid, dim3(KT_THREADS), 0, st, a);
            return;
        }
        // the divergence: the sweeps leave their sums in the scratch, kd_combine does the zero-fill on the other kernels' grid
        a.vals = v.vals; a.gsum = v.gsum;
        a.self_err = lk.self_err_out != nullptr ? v.self_err : (double*)nullptr;
        if (lk.unbalanced()) {
            a.rho = v.rho; a.mass_q = v.mass_q;
            a.transported = lk.transported_out != nullptr ? v.transported : (double*)nullptr;
            hipLaunchKernelGGL(kd_sweeps_unbalanced, dim3(B, H, 3), dim3(KT_THREADS), 0, st, a);
            hipLaunchKernelGGL((kd_combine<true, true>), grid, dim3(KD_COMBINE_THREADS), 0, st, a);
        } else {
            hipLaunchKernelGGL(kd_sweeps, dim3(B, H, 3), dim3(KT_THREADS), 0, st, a);
            hipLaunchKernelGGL((kd_combine<true>), grid, dim3(KD_COMBINE_THREADS), 0, st, a);
        }
    }
}
// forward over n_rollout steps (+ loss), optionally the backward pass with weight gradients
int train_forward_backward(drp_ctx* c, int B, int N, const TrainPass& tp) {
    const int H = c->tr_nroll;
    const bool backward = tp.backward, defer = tp.defer;
    WgradQueue& wq = *c->wgrad;
    wq.begin(defer);
    const size_t bn = (size_t)B * N, bn64 = bn * 64, bnk = bn * DRP_K;
    const size_t hstride = (size_t)H * N * 3;                 // predicted states [B][H][N][3]
    const size_t in_stride = (size_t)(H + 1) * N * 3;         // given states     [B][H+1][N][3]
    hipStream_t st = c->stream;
    float* states = ptr<float>(c->states);
    const float* given = tr_staged<float>(c, tp.lay, TRB_STATES);
    const int* nums = tr_staged<int>(c, tp.lay, TRB_NUMS);
    const float* acts = tp.actions ? tr_staged<float>(c, tp.lay, TRB_IMPULSES) : nullptr;
    float* g_state = ptr<float>(c->g_state);
    {
        const float* cself = nullptr;
        const uint8_t* cself_ok = nullptr;
        CHK(prepare_cself(c, B, N, B, &cself, &cself_ok, tp.engine));
        TapeFwd f{};
        f.s0 = given; f.s0_mod = B; f.s0_stride = in_stride;
        f.mod = B;
        f.actions = nullptr;            // this step's impulses are data (train/train_gnn_dyn.py:181): the step-major copy kt_unpack_inputs left
        f.masked_actions = acts;        //   -- or the batch's pushes on the step's own input, written there ahead of each step
        f.nums = nums;
        f.padded = true;                // collate_fn pads with zero rows: coincident particles
        f.tape = backward; f.agg_hist = true;
        f.cself = cself; f.cself_ok = cself_ok;
        CHK(run_tape_forward(c, tp.engine, B, N, H, f));
    }
    if (tp.predict) {
        HIPCHK(c, hipGetLastError());
        return DRP_OK;
    }
    train_launch_loss(c, B, N, tp, tr_view(c->tr_arena.p, c->tr_loss.p, tp.lay));
    HIPCHK(c, hipGetLastError());
    if (!backward) return DRP_OK;

    float* G = ptr<float>(c->tr_grad);
    // a training batch is a handful of samples: the edge terms' kernel splits each sample's rows over workgroups (one
    // receiver per 16 lanes)
    int chunks16 = (N + 15) / 16;
    if (chunks16 > 4096 / B) chunks16 = 4096 / B;
    if (chunks16 < 1) chunks16 = 1;
    const dim3 egrid((unsigned)(B * chunks16));
    const float* dens = ptr<float>(c->ws.dens);
    // the reversed lists of ALL rollout steps in one launch (the tape holds every step's lists; a training batch is a handful
    // of workgroups per step).  Data impulses: padded receivers are left out, their gradient is identically zero while no zero
    // row neighbours a real one.  With pushes every receiver is listed, as in the GD planner: the pass stays exact where a pile
    // lies around the camera-frame origin and a zero row is a real row's sender (d loss / d s_pred of that zero row is not zero)
    launch_reverse_lists(c, ptr<int16_t>(c->tape_idx), ptr<uint8_t>(c->tape_cnt), N, B * H, acts != nullptr ? nullptr : nums, B);
    // deferred weight gradients: what a job reads keeps a buffer per rollout step t (g_eff and g_proj: per propagation step
    // too; slot 0 of g_eff is the transient copy the predictor writes and the particle encoder reads)
    const size_t per_t = defer ? 1 : 0;
    // the node stages of a rollout step in ONE launch (kmb_step_bwd<dump>) or a launch per stage (dispatch.h: plan_train_backward)
    const TrainBwdPlan k = plan_train_backward(c->pol, c->n_cu, B, N, defer);
    const bool fused = k.fused, f_coop = k.coop;
    const int f_spw = k.spw, f_groups = k.groups, f_parts = k.parts;
    unsigned* const f_bar = reinterpret_cast<unsigned*>(G + TR_GRAD_PAD);        // [H][f_groups] arrival counters, then the give-up flag
    for (int t = H - 1; t >= 0; --t) {
        const size_t tt = per_t * (size_t)t;
        KbEdgeDump ed{ptr<float>(c->ed_re) + tt * bnk * 64, ptr<float>(c->ed_a2) + tt * bnk * 64, ptr<float>(c->ed_a1) + tt * bnk * 64,
                      ptr<float>(c->ed_x0) + tt * bnk * 8, ptr<float>(c->ed_gce) + tt * bnk * 64, ptr<float>(c->ed_g3) + tt * bnk * 64,
                      ptr<float>(c->ed_g2) + tt * bnk * 64, ptr<float>(c->ed_g1) + tt * bnk * 64};
        const float* s_prev = (t == 0) ? given : states + (size_t)(t - 1) * N * 3;
        const size_t prev_stride = (t == 0) ? in_stride : hstride;
        const int16_t* idx = ptr<int16_t>(c->tape_idx) + (size_t)t * bnk;
        float* g_out = g_state + (size_t)t * bn * 3;
        BwdStep s{};
        s.B = B; s.N = N; s.mod = B;
        s.eht = ptr<float>(c->eff_hist) + (size_t)t * 4 * bn64;
        s.mht = ptr<unsigned>(c->tape_mask) + (size_t)t * DRP_PSTEP * bnk * 2;
        s.cnt = ptr<uint8_t>(c->tape_cnt) + (size_t)t * bn;
        s.rev_off = ptr<int>(c->rev_off) + (size_t)t * B * (N + 1);
        s.rev = ptr<int>(c->rev) + (size_t)t * bnk;
        s.sdelta = ptr<float>(c->tape_sdelta) + (size_t)t * bn * 3;
        s.g_out = g_out;
        s.gah = ptr<float>(c->g_agg_hist);
        s.ge_tmp = ptr<float>(c->g_eff);
        s.g_cnode = ptr<float>(c->g_cnode) + tt * bn64;
        s.d.hact = ptr<float>(c->tr_hact) + tt * bn64; s.d.gh = ptr<float>(c->tr_gh) + tt * bn64;
        for (int v = 0; v < 3; ++v) {           // v = 0, 1, 2: propagation steps 2, 1, 0 of ge; p = v of gp
            s.d.ge[v] = ptr<float>(c->g_eff) + per_t * ((size_t)(t * 3 + v) + 1) * bn64;
            s.d.gp[v] = ptr<float>(c->g_proj) + per_t * (size_t)(t * 3 + v) * bn64 * 2;
        }
        s.d.gpe = ptr<float>(c->tr_gpe) + tt * bn64; s.d.a1n = ptr<float>(c->tr_a1n) + tt * bn64;
        s.d.gh1 = ptr<float>(c->tr_gh1) + tt * bn64; s.d.xn = ptr<float>(c->tr_xn) + tt * bn * 8;
        const NodeWgrad wg{wq, G, ptr<float>(c->agg_hist) + (size_t)t * 3 * bn64, dens};
        if (fused) {
            // everything between the loss gradient and the relation encoder's backward in ONE launch (kmb_step_bwd<DUMP>): the
            // operands of the weight gradients are its dumps; the jobs in the stage kernels' queue order
            c->dv(k.variant());
#define STEP_BWD_ARGS ptr<float>(c->w_mfma), ptr<float>(c->w_mfma_bwd), s.eht, s.mht, s.cnt, s.rev_off, s.rev, g_out, (size_t)N * 3, \
                      s.sdelta, ptr<float>(c->ws.attr), B, dens, B, N, B, f_spw, s.ge_tmp, s.g_cnode, s.gah, ptr<float>(c->g_sdelta), s.d, \
                      f_parts, f_bar + (size_t)t * f_groups, f_bar + (size_t)H * f_groups
            if (f_coop)
                hipLaunchKernelGGL((kmb_step_bwd<true, true>), dim3((unsigned)(f_groups * f_parts)), dim3(64 * KMB_FUSED_WAVES), KMB_COOP_LDS, st, STEP_BWD_ARGS);
            else
                hipLaunchKernelGGL((kmb_step_bwd<true, false>), dim3((unsigned)(f_groups * f_parts)), dim3(64 * KMB_FUSED_WAVES), KMB_FUSED_LDS, st, STEP_BWD_ARGS);
#undef STEP_BWD_ARGS
            wg.predictor(s);
            for (int p = DRP_PSTEP - 1; p >= 0; --p) {
                wg.update(s, p);
                wg.edge_terms(s, p);
            }
            wg.cnode(s);
            wg.encoder(s);
        } else {
            c->dv(k.variant());
            launch_node_stages(c, s, egrid, chunks16, &wg);
        }
        // the previous step's output feeds this step as s_cur: residual + relation encoder
        float* g_prev = t > 0 ? g_state + (size_t)(t - 1) * bn * 3 : nullptr;
        c->dv(DV_BWD_EDGE_MFMA);
        launch_edge_encode_mfma(c, s_prev, B, prev_stride, B, idx, s.cnt, s.gah, s.mht, bn, N, B,
                                g_prev != nullptr ? ptr<float>(c->gpos_edge) : (float*)nullptr, ed);
        // the residual's share: nothing touches g_prev before kb_gather_pos, which adds it first
        if (g_prev != nullptr)
            hipLaunchKernelGGL(kb_gather_pos, dim3((N + 255) / 256, B), dim3(256), 0, st, ptr<float>(c->gpos_edge),
                               s.rev_off, s.rev, N, g_prev, (size_t)N * 3, s.cnt, (const float*)g_out);
        // the push's share, last: the impulse of this step was evaluated on s_pred_{t-1} (c->g_sdelta: the node stages' d / d impulse)
        if (g_prev != nullptr && acts != nullptr)
            hipLaunchKernelGGL(kb_sdelta_pos, dim3(B), dim3(256), 0, st, s_prev, prev_stride, acts + (size_t)t * 4, (size_t)H * 4,
                               ptr<float>(c->g_sdelta), nums, N, c->cam, g_prev, (size_t)N * 3);
        wq.push<64>(ed.gce, 64, ed.re, 64, (long)bnk, G + W_RP_W, 193, 1, G + W_RP_B, G + W_RP_W + 192, dens, B,
                    (long)N * DRP_K);
        wq.push<64>(ed.g3, 64, ed.a2, 64, (long)bnk, G + W_RE4_W, 64, 1, G + W_RE4_B, nullptr, nullptr, 1, 1);
        wq.push<64>(ed.g2, 64, ed.a1, 64, (long)bnk, G + W_RE2_W, 64, 1, G + W_RE2_B, nullptr, nullptr, 1, 1);
        wq.push<6>(ed.g1, 64, ed.x0, 8, (long)bnk, G + W_RE0_W, 6, 1, G + W_RE0_B, nullptr, nullptr, 1, 1);
        wq.flush();                                  // the next rollout step rewrites the dumps these jobs read
    }
    wq.flush();
    // bias of the predictor's last layer: the column sums of every step's d loss / d s_pred (all final by now), one launch
    hipLaunchKernelGGL(kt_colsum3, dim3(1), dim3(1024), 0, st, g_state, (long)(H * bn), G + W_PR1_B);
    if (defer) {
        CHK(wq.flush_all());
        wq.tap_G = G; wq.tap_cs_g = g_state; wq.tap_cs_M = (long)(H * bn); wq.tap_dens = dens; wq.tap_dens_n = B;
    }
    HIPCHK(c, hipGetLastError());
    return DRP_OK;
}

// The packed copies of the weights follow an optimiser step without a round trip of the packers through the host
// (k_train.h): only the blob itself comes back -- the split relation encoder's range shift is a function of the
// weights (set_split_range), and drp_get_weights serves the host copy.
int ensure_repack_maps(drp_ctx* c) {
    if (c->repack_maps_ready) return DRP_OK;
    std::vector<float> probe((size_t)W_TOTAL);
    for (int i = 0; i < (int)W_TOTAL; ++i) probe[i] = (float)(i + 1);          // exact in fp32 (38 403 < 2^24)
    auto to_map = [](const std::vector<float>& packed) {
        std::vector<int> m(packed.size());
        for (size_t i = 0; i < packed.size(); ++i)
            m[i] = packed[i] == 0.0f ? 0 : (packed[i] < 0.0f ? -1 : (int)packed[i]);
        return m;
    };
    std::vector<float> v, m, mb;
    pack_valu(probe.data(), v);
    pack_mfma(probe.data(), m);
    pack_mfma_bwd(probe.data(), mb);
    const std::vector<int> mv = to_map(v), mm = to_map(m), mmb = to_map(mb);
    CHK(h2d(c, c->map_valu, mv.data(), mv.size() * sizeof(int)));
    CHK(h2d(c, c->map_mfma, mm.data(), mm.size() * sizeof(int)));
    CHK(h2d(c, c->map_mfma_bwd, mmb.data(), mmb.size() * sizeof(int)));
    CHK(guarded_wait(c, nullptr));                   // the vectors go out of scope
    CHK(ensure_pinned(c, c->w_pin, ((size_t)W_TOTAL + 4) * sizeof(float)));      // one size for the context's life: never replaced
    c->repack_maps_ready = true;
    return DRP_OK;
}

// launches only: the caller's final wait brings the blob and the device's shift back (finish_repack)
int repack_on_device(drp_ctx* c, bool blob_in_pin = false /* k_adam has written the updated blob to w_pin already */) {
    CHK(ensure_repack_maps(c));
    CHK(ensure(c, c->re_shift_dev, sizeof(int)));
    hipStream_t st = c->stream;
    const float* w = ptr<float>(c->w_raw);
    RepackAll a{};
    a.map_v = ptr<int>(c->map_valu); a.dst_v = ptr<float>(c->w_valu); a.n_v = (int)V_TOTAL;
    a.map_m = ptr<int>(c->map_mfma); a.dst_m = ptr<float>(c->w_mfma); a.n_m = (int)M_TOTAL;
    a.map_mb = ptr<int>(c->map_mfma_bwd); a.dst_mb = ptr<float>(c->w_mfma_bwd); a.n_mb = (int)MB_TOTAL;
    a.out6 = ptr<uint16_t>(c->w_split6); a.out6b = ptr<uint16_t>(c->w_split6_bwd);
    a.forced_shift = c->re_shift_env; a.shift_out = ptr<int>(c->re_shift_dev);
    hipLaunchKernelGGL(kt_repack_all, dim3(KT_REPACK_ALL_BLOCKS((int)V_TOTAL, (int)M_TOTAL, (int)MB_TOTAL)), dim3(256), 0, st, w, a);
    // the relation encoder's range shift depends on the new weights: the launch above derived it; the blob itself comes
    // back too (it is the host copy drp_get_weights serves, and the host's own range for the calls to come)
    hipLaunchKernelGGL(kt_repack_split, dim3(4 * 16), dim3(256), 0, st, w, 0, ptr<uint16_t>(c->w_split), ptr<int>(c->re_shift_dev),
                       blob_in_pin ? ptr<int>(c->w_pin) + W_TOTAL : (int*)nullptr);
    if (!blob_in_pin) {
        HIPCHK(c, hipMemcpyAsync(c->w_pin.p, c->w_raw.p, (size_t)W_TOTAL * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(ptr<float>(c->w_pin) + W_TOTAL, c->re_shift_dev.p, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipGetLastError());
    return DRP_OK;
}
// after the wait: the host's copy of the blob and its range; host and device derive the shift by the same operations --
// should they ever disagree, the fragments are packed again with the host's
int finish_repack(drp_ctx* c) {
    c->w_host.assign(ptr<float>(c->w_pin), ptr<float>(c->w_pin) + W_TOTAL);
    set_split_range(c, c->w_host.data());
    int dev_shift;
    memcpy(&dev_shift, ptr<float>(c->w_pin) + W_TOTAL, sizeof(int));
    if (dev_shift != c->re_range.shift) {
        hipLaunchKernelGGL(kt_repack_split, dim3(4 * 16), dim3(256), 0, c->stream, ptr<float>(c->w_raw), c->re_range.shift,
                           ptr<uint16_t>(c->w_split), (const int*)nullptr);
        HIPCHK(c, hipGetLastError());
        CHK(guarded_wait(c, nullptr));
    }
    return DRP_OK;
}

int install_weights(drp_ctx* c, const std::vector<float>& blob) {
    std::vector<float> tmp(blob);
    return drp_load_weights(c, tmp.data(), tmp.size(), c->adj_thresh);
}

// the optimiser seam's buffers (capi_optim.h) at their one size, the accumulator zeroed: launches only, drp_train_begin waits
int optim_begin(drp_ctx* c) {
    const size_t n_part = (size_t)KO_BLOCKS((int)W_TOTAL);
    CHK(ensure(c, c->tr_acc, (size_t)W_TOTAL * sizeof(double)));
    CHK(ensure(c, c->tr_opt, n_part * sizeof(double) + sizeof(KoStep)));
    CHK(ensure(c, c->tr_g32, (size_t)W_TOTAL * sizeof(float)));
    CHK(ensure_pinned(c, c->opt_pin, sizeof(KoStep)));      // one size for the context's life: never replaced
    HIPCHK(c, hipMemsetAsync(c->tr_acc.p, 0, (size_t)W_TOTAL * sizeof(double), c->stream));
    return DRP_OK;
}
}  // namespace

int drp_train_begin(drp_ctx* c, int n_rollout, double lr, double beta1) {
    CHK(need(c, true, false, false));
    if (n_rollout < 1 || n_rollout > 64 || !(lr > 0.0) || !(beta1 >= 0.0 && beta1 < 1.0))
        return fail(c, DRP_EINVAL, "bad training arguments n_rollout=%d lr=%g beta1=%g", n_rollout, lr, beta1);
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ensure(c, c->tr_grad, ((size_t)TR_GRAD_PAD + (size_t)n_rollout * c->n_cu + 1) * sizeof(float)));
    CHK(ensure(c, c->tr_m, (size_t)W_TOTAL * sizeof(float)));
    CHK(ensure(c, c->tr_v, (size_t)W_TOTAL * sizeof(float)));
    CHK(ensure(c, c->wgrad->tr_part, (size_t)KT_WGRAD_MAX_JOBS * KT_WGRAD_MAX_BLOCKS * 66 * 64 * sizeof(float)));
    HIPCHK(c, hipMemsetAsync(c->tr_m.p, 0, (size_t)W_TOTAL * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(c->tr_v.p, 0, (size_t)W_TOTAL * sizeof(float), c->stream));
    CHK(optim_begin(c));                // the optimiser seam's accumulator, zeroed (capi_optim.h)
    CHK(guarded_wait(c, nullptr));
    c->tr_nroll = n_rollout; c->tr_lr = lr; c->tr_beta1 = beta1; c->tr_iter = 0;
    c->tr_grad_fresh = false; c->tr_acc_n = 0;
    c->tr_on = true;
    c->gd_on = false;
    c->mpc_on = false;
    return DRP_OK;
}

namespace {
// ---- drp_train_step and drp_train_step_untracked: one body (train_step_body), the loss kind and the targets in `lk` ----
// `impulses`: states_delta [B][H][N][3], or with `actions` the pushes [B][H][4]
int train_check_args(drp_ctx* c, const float* states, const float* impulses, bool actions, const float* attrs,
                     const int32_t* particle_nums, const float* particle_dens, int B, int N, const TrLoss& lk, int mode) {
    if (!c || !c->tr_on) return fail(c, DRP_ESTATE, "drp_train_begin not called");
    CHK(check_bn(c, B, N));
    if (!states || !impulses || !attrs || !particle_nums || !particle_dens) return fail(c, DRP_EINVAL, "null argument");
    if (actions) {
        if (!c->have_cam) return fail(c, DRP_ESTATE, "camera not set (drp_set_camera)");
        // a zero-length push is 0 / 0 in every impulse (planners.py:240) and from there in every weight; the dataset path
        // refuses such a push too (dataset_gnn_dyn.py:148-153)
        CHK(check_pushes(c, impulses, B, c->tr_nroll));
    }
    if (mode < DRP_TRAIN_EVAL || mode > DRP_TRAIN_UPDATE) return fail(c, DRP_EINVAL, "bad mode %d", mode);
    CHK(check_particle_nums(c, particle_nums, B, N));
    if (lk.given()) {
        // the caller's seed: there, for a reverse pass, and a number on every real row
        if (!lk.seed) return fail(c, DRP_EINVAL, "null argument");
        if (mode == DRP_TRAIN_EVAL)
            return fail(c, DRP_EINVAL, "drp_train_step_seeded runs a reverse pass (DRP_TRAIN_GRAD, DRP_TRAIN_UPDATE): the forward alone is drp_train_predict");
        const int H = c->tr_nroll;
        const long bad = first_bad_seed(lk.seed, particle_nums, B, H, N);
        if (bad >= 0)
            return fail(c, DRP_EINVAL, "seed: sample %d step %d row %d is not finite", (int)(bad / N / H), (int)(bad / N % H), (int)(bad % N));
    }
    if (lk.targeted()) {
        CHK(check_target_clouds(c, lk, KC_MAX_POINTS, "target size"));
        if (lk.match()) CHK(check_match_loss(c, lk, N));
        if (lk.sinkhorn()) {
            if (N > KT_MAX_POINTS || lk.M > KT_MAX_POINTS)
                return fail(c, DRP_EINVAL, "the %s takes clouds of 1..%d points: N=%d M=%d",
                            lk.divergence() ? "Sinkhorn divergence" : "transport loss", KT_MAX_POINTS, N, lk.M);
            CHK(check_transport_params(c, lk.eps, B, lk.iters));
            if (lk.unbalanced()) CHK(check_reach_params(c, lk.eps, lk.rho, lk.mass_q, B, c->tr_nroll));
        }
        CHK(check_target_nums(c, lk, B, c->tr_nroll));
    }
    return DRP_OK;
}

// every buffer of the step at its size, and whether the weight gradients of its backward pass are deferred (tp.defer)
int train_ensure_workspace(drp_ctx* c, int B, int N, TrainPass& tp) {
    const int H = c->tr_nroll;
    const size_t bn = (size_t)B * N, bn64 = bn * 64, bnk = bn * DRP_K;
    // behind the batch in tr_pin: what comes BACK after the one wait -- the loss terms [H][B] and the give-up flag of kmb_step_bwd's
    // barrier (pinned: the copies are asynchronous, nothing on the way touches pageable memory or the caller's frame)
    // kernels read and write tr_pin directly; no wait before it goes: every earlier call has waited for or drained its work (DrainOnError)
    CHK(ensure_pinned(c, c->tr_pin, tp.lay.bytes + (size_t)H * B * sizeof(double) + 16));
    CHK(ensure(c, c->tr_arena, tp.lay.bytes));
    CHK(ensure(c, c->ws.attr, bn * sizeof(float)));
    CHK(ensure(c, c->ws.dens, (size_t)B * sizeof(float)));
    CHK(ensure(c, c->tape_sdelta, (size_t)H * bn * 3 * sizeof(float)));
    CHK(ensure_step_ws(c, c->ws, B, N, tp.engine));
    CHK(ensure(c, c->states, (size_t)H * bn * 3 * sizeof(float)));
    CHK(ensure(c, c->g_state, (size_t)H * bn * 3 * sizeof(float)));
    tp.defer = false;
    if (tp.backward) {
        // deferred weight gradients keep every job's operands until the end of the backward pass: H copies of the node-level
        // dumps (3 H + 1 of g_eff, 3 H of g_proj) and of the relation encoder's dumps -- 0.24 GB per rollout step at 32 x 300
        const size_t keep_bytes = (size_t)H * (16 * bn64 + 7 * bnk * 64 + bnk * 8 + bn * 8) * sizeof(float);
        const bool defer = tp.defer = c->wgrad_defer && keep_bytes <= ((size_t)8 << 30);
        const size_t kt = defer ? (size_t)H : 1;
        CHK(ensure_tape(c, B, N, H, H));
        CHK(ensure(c, c->agg_hist, (size_t)H * 3 * bn64 * sizeof(float)));
        CHK(ensure(c, c->g_eff, (defer ? 3 * kt + 1 : 1) * bn64 * sizeof(float)));
        CHK(ensure(c, c->g_cnode, kt * bn64 * sizeof(float)));
        CHK(ensure(c, c->g_proj, (defer ? 3 * kt : 1) * bn64 * 2 * sizeof(float)));
        DevBuf* node64[] = {&c->tr_hact, &c->tr_gh, &c->tr_gpe, &c->tr_a1n, &c->tr_gh1};
        for (DevBuf* b : node64) CHK(ensure(c, *b, kt * bn64 * sizeof(float)));
        CHK(ensure(c, c->tr_xn, kt * bn * 8 * sizeof(float)));
        DevBuf* edge64[] = {&c->ed_re, &c->ed_a2, &c->ed_a1, &c->ed_gce, &c->ed_g3, &c->ed_g2, &c->ed_g1};
        for (DevBuf* b : edge64) CHK(ensure(c, *b, kt * bnk * 64 * sizeof(float)));
        CHK(ensure(c, c->ed_x0, kt * bnk * 8 * sizeof(float)));
    }
    CHK(ensure(c, c->tr_loss, tp.lay.res_bytes));       // the terms, the loss's other results and its scratch (train_host.h)
    return DRP_OK;
}

// the batch in one copy: packed into pinned staging in the caller's layouts, unpacked by one launch (kt_unpack_inputs)
int train_stage_batch(drp_ctx* c, const float* states, const float* impulses, const float* attrs, const int32_t* particle_nums,
                      const float* particle_dens, int B, int N, const TrainPass& tp) {
    const int H = c->tr_nroll;
    const TrBlocks& lay = tp.lay;
    char* pin = ptr<char>(c->tr_pin);
    const void* const five[] = {states, impulses, attrs, particle_dens, particle_nums};
    for (int id = TRB_STATES; id <= TRB_NUMS; ++id) memcpy(pin + lay.off[id], five[id], lay.size(id));
    tr_stage_loss_inputs(pin, lay, tp.lk);
    // the unpacking launch IS the upload: it reads the staged batch from the pinned host buffer (device-visible) and leaves
    // the arena copy for the kernels that read the given states; DRP_TRAIN_COPY_UPLOAD=1: a copy on the stream first
    const bool by_kernel = !c->train_copy_upload;
    if (!by_kernel) CHK(h2d(c, c->tr_arena, c->tr_pin.p, lay.bytes));
    const char* ar = by_kernel ? ptr<const char>(c->tr_pin) : static_cast<const char*>(c->tr_arena.p);
    const size_t total = (size_t)H * B * N * 3;
    hipLaunchKernelGGL(kt_unpack_inputs, dim3((unsigned)std::min<size_t>((total + 255) / 256, 1024)), dim3(256), 0, c->stream,
                       tp.actions ? (const float*)nullptr : reinterpret_cast<const float*>(ar + lay.off[TRB_IMPULSES]),
                       reinterpret_cast<const float*>(ar + lay.off[TRB_ATTRS]),
                       reinterpret_cast<const float*>(ar + lay.off[TRB_DENS]), B, H, N, ptr<float>(c->tape_sdelta), ptr<float>(c->ws.attr),
                       ptr<float>(c->ws.dens), by_kernel ? ptr<const float4>(c->tr_pin) : (const float4*)nullptr,
                       by_kernel ? static_cast<float4*>(c->tr_arena.p) : (float4*)nullptr, by_kernel ? lay.bytes / 16 : (size_t)0);
    return DRP_OK;
}

// One pass over the staged batch, the optimiser step, the re-pack, the wait.  `back`: the loss terms [H][B] and the give-up flag
// in tr_pin; *gave_up: kmb_step_bwd's barrier among the workgroups of a group gave up after two seconds (k_backward_mfma.h)
// and set the flag behind its counters -- the gradient of such a pass is partial.  The optimiser step reads the flag ON THE
// DEVICE and moves nothing when it is set (k_adam's `skip`); the iteration count advances only once it has come back clear.
int train_attempt(drp_ctx* c, int B, int N, const TrainPass& tp, int mode, bool want_loss, float* grad_out, double* back, bool* gave_up) {
    const int H = c->tr_nroll;
    unsigned* const flag_host = reinterpret_cast<unsigned*>(back + (size_t)H * B);
    CHK(train_forward_backward(c, B, N, tp));
    const int f_spw = (B + c->n_cu - 1) / c->n_cu, f_groups = (B + f_spw - 1) / f_spw;
    const unsigned* const flag_dev = reinterpret_cast<const unsigned*>(ptr<float>(c->tr_grad) + TR_GRAD_PAD + (size_t)H * f_groups);
    *flag_host = 0;
    // update iterations end WITHOUT a copy on the stream: the loss terms are stored to pinned host memory by the loss kernel,
    // the optimiser step writes the updated blob and the barrier's flag there, kt_repack_split the range shift -- a copy
    // engine's transfer between kernels costs tens of microseconds of hand-over (tools/train_trace.sh)
    const bool direct = mode == DRP_TRAIN_UPDATE && c->repack_device && !c->train_copy_upload;
    if (c->debug_force_giveup && tp.backward) {        // tests: the flag as a timed-out barrier would leave it, once
        HIPCHK(c, hipMemsetAsync(const_cast<unsigned*>(flag_dev), 1, sizeof(unsigned), c->stream));
        c->debug_force_giveup = false;
    }
    if (want_loss && tp.loss_terms != back) CHK(d2h(c, back, c->tr_loss.p, (size_t)H * B * sizeof(double)));
    if (grad_out && tp.backward) CHK(d2h(c, grad_out, c->tr_grad.p, (size_t)W_TOTAL * sizeof(float)));
    CHK(tr_read_results(tp.lay, c->tr_loss.p, tp.lk, [c](void* dst, const void* src, size_t n) { return d2h(c, dst, src, n); }));
    if (tp.backward && !direct) CHK(d2h(c, flag_host, flag_dev, sizeof(unsigned)));
    bool repacked = false;
    if (mode == DRP_TRAIN_UPDATE) {
        const long iter = c->tr_iter + 1;
        const double bc1 = 1.0 - pow(c->tr_beta1, (double)iter), bc2 = 1.0 - pow(0.999, (double)iter);
        const float inf = __builtin_inff();
        if (direct) CHK(ensure_repack_maps(c));          // (allocates w_pin)
        hipLaunchKernelGGL(k_adam, dim3((W_TOTAL + 255) / 256), dim3(256), 0, c->stream, ptr<float>(c->w_raw),
                           ptr<float>(c->tr_grad), ptr<float>(c->tr_m), ptr<float>(c->tr_v), (int)W_TOTAL,
                           (float)(c->tr_lr / bc1), (float)sqrt(bc2), make_float4(-inf, -inf, -inf, -inf),
                           make_float4(inf, inf, inf, inf), (float)c->tr_beta1, direct ? ptr<float>(c->w_pin) : (float*)nullptr, flag_dev,
                           direct ? flag_host : (unsigned*)nullptr);
        if (hipGetLastError() != hipSuccess) return fail(c, DRP_EHIP, "k_adam launch");
        c->f64_w_valid = false;           // the float64 copy is of the old blob: the next *_f64 call widens the new one
        // the engines read packed copies of the weights: rebuild them from the blob (unchanged if the step was skipped)
        if (c->repack_device) {
            CHK(repack_on_device(c, direct));
            repacked = true;
        } else {
            std::vector<float> blob((size_t)W_TOTAL);
            CHK(d2h(c, blob.data(), c->w_raw.p, (size_t)W_TOTAL * sizeof(float)));
            CHK(guarded_wait(c, nullptr));
            CHK(install_weights(c, blob));
        }
    }
    CHK(drp_sync(c));
    *gave_up = *flag_host != 0;
    if (repacked && !*gave_up) CHK(finish_repack(c));      // (a skipped step wrote no blob: the weights are what they were)
    if (!*gave_up && mode == DRP_TRAIN_UPDATE) c->tr_iter += 1;
    return DRP_OK;
}

int train_step_body(drp_ctx* c, const float* states, const float* impulses, bool actions, const float* attrs,
                    const int32_t* particle_nums, const float* particle_dens, int B, int N, const TrLoss& lk, int mode,
                    double* loss_out, float* grad_out, float* pred_out = nullptr /* drp_train_predict: the forward alone */) {
    if (c) c->tr_grad_fresh = false;    // every trainer pass, refused ones included, ends what drp_train_accumulate could take
    if (c) c->wgrad_tap_on = false;     //   and what the "train_wgrad_*" taps could show
    CHK(train_check_args(c, states, impulses, actions, attrs, particle_nums, particle_dens, B, N, lk, mode));
    HIPCHK(c, hipSetDevice(c->device));
    end_sessions(c);
    const int H = c->tr_nroll;
    TrainPass tp;
    {
        float amax = 0.0f;                                    // a_cur = attrs[:, 0]
        for (int b = 0; b < B; ++b) amax = fmaxf(amax, max_abs(attrs + (size_t)b * (H + 1) * N, (size_t)N));
        // the largest impulse: the data's, or what the pushes can cause on any state
        const float sd_max = actions ? push_len_bound(c, impulses, (size_t)B * H) : max_abs(impulses, (size_t)B * H * N * 3);
        CHK(pick_tape_engine(c, amax, max_abs(particle_dens, (size_t)B), sd_max, &tp.engine));
    }
    tp.backward = mode != DRP_TRAIN_EVAL;
    tp.predict = pred_out != nullptr;
    tp.lay = tr_blocks(lk.shape(), B, H, N, actions, false);
    tp.lk = lk;
    tp.actions = actions;
    CHK(train_ensure_workspace(c, B, N, tp));
    c->marks.lastH = H;
    double* const back = reinterpret_cast<double*>(ptr<char>(c->tr_pin) + tp.lay.bytes);
    tp.loss_terms = (loss_out && !c->train_copy_upload) ? back : ptr<double>(c->tr_loss);   // pinned: the terms land where this call reads them
    DrainOnError drain(c);
    CHK(train_stage_batch(c, states, impulses, attrs, particle_nums, particle_dens, B, N, tp));
    bool gave_up = false;
    if (tp.predict) {
        // the forward a DRP_TRAIN_GRAD pass runs, then the predicted states as they lie, [B][H][N][3]; nothing else happens
        CHK(train_forward_backward(c, B, N, tp));
        CHK(d2h(c, pred_out, c->states.p, (size_t)B * H * N * 3 * sizeof(float)));
        CHK(drp_sync(c));
    } else {
        // a pass whose barrier gave up runs again with one workgroup per group (no barrier to wait at) -- for the rest of the
        // context's life
        CHK(train_attempt(c, B, N, tp, mode, loss_out != nullptr, grad_out, back, &gave_up));
    }
    if (gave_up && c->pol.train_parts != 1) {
        c->pol.train_parts = 1;                     // the device is shared or masked: the groups' workgroups are not all resident
        c->dv(DV_TRAIN_BARRIER_RETRY);
        CHK(train_attempt(c, B, N, tp, mode, loss_out != nullptr, grad_out, back, &gave_up));
    }
    if (gave_up)
        return fail(c, DRP_EHIP, "kmb_step_bwd: a workgroup waited two seconds for the others of its group, with one workgroup per group too");
    if (loss_out) {
        double total = 0.0;                     // fixed order: step-major, then sample
        for (size_t q = 0; q < (size_t)H * B; ++q) total += back[q];
        *loss_out = total;
    }
    c->tr_grad_fresh = mode == DRP_TRAIN_GRAD && !tp.predict;       // tr_grad is whole and the weights are where it was taken
    c->wgrad_tap_on = tp.backward && tp.defer && !tp.predict;       // every operand of the pass's deferred jobs is still in place
    return drain.ok();
}
}  // namespace

int drp_train_step(drp_ctx* c, const float* states, const float* states_delta, const float* attrs,
                   const int32_t* particle_nums, const float* particle_dens, int B, int N, int mode, double* loss_out,
                   float* grad_out) {
    return train_step_body(c, states, states_delta, false, attrs, particle_nums, particle_dens, B, N, TrLoss{}, mode, loss_out, grad_out);
}

int drp_train_step_untracked(drp_ctx* c, const float* states, const float* states_delta, const float* attrs,
                             const int32_t* particle_nums, const float* particle_dens, int B, int N, const float* targets,
                             const int32_t* target_nums, int M, int mode, double* loss_out, float* grad_out) {
    return train_step_body(c, states, states_delta, false, attrs, particle_nums, particle_dens, B, N,
                           TrLoss::against(TR_LOSS_CHAMFER, targets, target_nums, M), mode, loss_out, grad_out);
}

// the same body with each step's impulse evaluated from the batch's pushes on the state the step reads (TrainPass::actions)
int drp_train_step_actions(drp_ctx* c, const float* states, const float* actions, const float* attrs, const int32_t* particle_nums,
                           const float* particle_dens, int B, int N, const float* targets, const int32_t* target_nums, int M,
                           int mode, double* loss_out, float* grad_out) {
    const bool untracked = targets != nullptr || target_nums != nullptr || M != 0;
    const TrLoss lk = untracked ? TrLoss::against(TR_LOSS_CHAMFER, targets, target_nums, M) : TrLoss{};
    return train_step_body(c, states, actions, true, attrs, particle_nums, particle_dens, B, N, lk, mode, loss_out, grad_out);
}

// drp_train_step_untracked / drp_train_step_actions with the loss kind and the mix's weight as arguments: the same body, two more
// fields of TrLoss
int drp_train_step_loss(drp_ctx* c, const float* states, const float* states_delta, const float* actions, const float* attrs,
                        const int32_t* particle_nums, const float* particle_dens, int B, int N, const float* targets,
                        const int32_t* target_nums, int M, int loss_kind, double match_weight, int mode, double* loss_out,
                        float* grad_out, int32_t* match_out) {
    if (!c) return DRP_EINVAL;
    c->tr_grad_fresh = false; c->wgrad_tap_on = false;       // (a call refused below ends both, as one refused in train_step_body)
    ImpulseSource src;
    CHK(impulse_source(c, states_delta, actions, src));
    if (loss_kind != DRP_LOSS_CHAMFER && loss_kind != DRP_LOSS_MATCH && loss_kind != DRP_LOSS_CHAMFER_MATCH)
        return fail(c, DRP_EINVAL, "bad loss_kind %d", loss_kind);
    TrLoss lk = TrLoss::against(loss_kind, targets, target_nums, M);
    lk.match_weight = match_weight; lk.match_out = match_out;
    return train_step_body(c, states, src.impulses, src.by_actions, attrs, particle_nums, particle_dens, B, N, lk,
                           mode, loss_out, grad_out);
}

// the forward of a DRP_TRAIN_GRAD pass alone -- the tape engine, the tape, the padded mode -- and every step's prediction out
int drp_train_predict(drp_ctx* c, const float* states, const float* states_delta, const float* actions, const float* attrs,
                      const int32_t* particle_nums, const float* particle_dens, int B, int N, float* states_pred_out) {
    if (!c) return DRP_EINVAL;
    c->tr_grad_fresh = false; c->wgrad_tap_on = false;       // (a call refused below ends both, as one refused in train_step_body)
    ImpulseSource src;
    CHK(impulse_source(c, states_delta, actions, src));
    if (!states_pred_out) return fail(c, DRP_EINVAL, "null argument");
    return train_step_body(c, states, src.impulses, src.by_actions, attrs, particle_nums, particle_dens, B, N,
                           TrLoss{}, DRP_TRAIN_GRAD, nullptr, nullptr, states_pred_out);
}

// the same body with the caller's d loss / d s_pred in the loss kernel's place (TR_LOSS_GIVEN): everything behind the seed is
// train_forward_backward's and train_attempt's
int drp_train_step_seeded(drp_ctx* c, const float* states, const float* states_delta, const float* actions, const float* attrs,
                          const int32_t* particle_nums, const float* particle_dens, int B, int N, const float* seed, int mode,
                          float* grad_out) {
    if (!c) return DRP_EINVAL;
    c->tr_grad_fresh = false; c->wgrad_tap_on = false;       // (a call refused below ends both, as one refused in train_step_body)
    ImpulseSource src;
    CHK(impulse_source(c, states_delta, actions, src));
    TrLoss lk;
    lk.kind = TR_LOSS_GIVEN; lk.seed = seed;
    return train_step_body(c, states, src.impulses, src.by_actions, attrs, particle_nums, particle_dens, B, N, lk,
                           mode, nullptr, grad_out);
}

int drp_train_set_lr(drp_ctx* c, double lr) {
    if (!c || !c->tr_on) return fail(c, DRP_ESTATE, "drp_train_begin not called");
    if (!(lr > 0.0)) return fail(c, DRP_EINVAL, "bad lr %g", lr);
    c->tr_lr = lr;
    return DRP_OK;
}

int drp_get_weights(drp_ctx* c, float* blob_out, size_t n_floats) {
    CHK(need(c, true, false, false));
    if (!blob_out || n_floats != (size_t)W_TOTAL) return fail(c, DRP_EINVAL, "blob_out must hold %d floats", (int)W_TOTAL);
    memcpy(blob_out, c->w_host.data(), n_floats * sizeof(float));
    return DRP_OK;
}
