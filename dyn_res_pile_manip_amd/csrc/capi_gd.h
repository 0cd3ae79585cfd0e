// capi_gd.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the gradient-descent planner (row f1): forward with tape, reverse mode, Adam, drp_gd_*.

// ---- gradient-descent planner (row f1) ----------------------------------------------------------
namespace {
// relation encoder backward on the matrix cores (kmb_edge_encode): one tile of 32 edge slots per wave, the tiles of a
// small batch spread one per CU
void launch_edge_encode_mfma(drp_ctx* c, const float* s_prev, int prev_mod, size_t prev_stride, int nb, const int16_t* idx,
                             const uint8_t* cnt, const float* gah, const unsigned* mht, size_t bn, int N, int B, float* gpos_edge,
                             const KbEdgeDump& dump) {
    const long ntiles = (long)B * (((long)N * DRP_K + 31) / 32);
    const unsigned grid = (unsigned)(ntiles < (long)c->n_cu ? ntiles : (long)c->n_cu);
    hipLaunchKernelGGL(kmb_edge_encode, dim3(grid), dim3(64 * MFMA_WAVES), KMB_EDGE_ENCODE_LDS, c->stream, ptr<float>(c->w_mfma),
                       ptr<float>(c->w_mfma_bwd), s_prev, prev_mod, prev_stride, ptr<float>(c->ws.attr), nb, ptr<float>(c->ws.dens), nb, idx,
                       cnt, gah, mht, bn, N, B, gpos_edge, dump);
}
// what one pass of the session does beside the gradients: the optimiser step that rides on the last kb_sdelta launch (a null
// adam.act: gradients only) and where kb_reward also stores the rewards (pinned host memory; null: the device buffer only)
// `seeded`: no reward -- the caller's d loss / d s_pred (staged in c->gd_seed_in, [B][H][N][3]) seeds the reverse pass in kb_reward's
// place.  Step H-1's slice IS d loss / d state_{H-1}, as kb_reward's gradient is; the slice of a step t < H-1 joins d loss /
// d state_t where that is summed: residual share (the copy of g_out), THEN THE SEED, then the relation encoder's own slots and
// reversed lists (kb_gather_pos: its g_add, "added first"), then gen_s_delta's position share (kb_sdelta).  `forward_only`: the tape's
// forward alone (drp_gd_predict).
struct GdPass { KbAdam adam = KbAdam{}; float* host_rewards = nullptr; bool seeded = false; bool forward_only = false; };
int gd_forward_backward(drp_ctx* c, const GdPass& pass) {
    const int nb = c->gd_nb, N = c->gd_N, B = c->gd_B, H = c->gd_H;
    const size_t bn = (size_t)B * N;
    const size_t hstride = (size_t)H * N * 3;
    hipStream_t st = c->stream;
    float* states = ptr<float>(c->states);
    auto d2d = [&](void* dst, const void* src, size_t bytes) -> int {
        HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
        return DRP_OK;
    };
    // the self-edge constants depend on attributes and densities only: computed once per GD problem,
    // again only if a rollout in between has reused the buffer
    if (c->gd_cself_tag != c->cself_tag || c->gd_cself_tag == 0) {
        const int rc = prepare_cself(c, nb, N, B, &c->gd_cself, &c->gd_cself_ok, c->gd_engine);
        c->gd_cself_tag = c->cself_tag;
        CHK(rc);
    }
    // ---- forward on the fused engine with tape
    bool rev_built = false;
    {
        TapeFwd f{};
        f.s0 = ptr<float>(c->ws.s_in); f.s0_mod = nb; f.s0_stride = (size_t)N * 3;
        f.mod = nb;
        f.actions = ptr<float>(c->actions);
        f.tape = true;
        f.cself = c->gd_cself; f.cself_ok = c->gd_cself_ok;
        if (H == 1) { f.rev_off = ptr<int>(c->rev_off); f.rev = ptr<int>(c->rev); f.rev_built = &rev_built; }   // one set of reversed lists: the only step's
        CHK(run_tape_forward(c, c->gd_engine, B, N, H, f));
    }
    if (pass.forward_only) { HIPCHK(c, hipGetLastError()); return DRP_OK; }
    // reward of the final step only (planners.py:436-438) and its gradient, in one launch
    float* g_state = ptr<float>(c->g_state);                 // [H][B,N,3]
    const float* seed_mid = nullptr;                         // [H-1][B,N,3]: the seeds of the steps before the last
    if (pass.seeded) {
        CHK(ensure(c, c->gd_seed, (size_t)(H > 1 ? H - 1 : 1) * bn * 3 * sizeof(float)));
        seed_mid = ptr<float>(c->gd_seed);
        ProbeScope ps(c, KC_BWD_REWARD);
        hipLaunchKernelGGL(kb_seed_stage, dim3(B, H), dim3(256), 0, st, ptr<float>(c->gd_seed_in), N, ptr<float>(c->gd_seed),
                           g_state + (size_t)(H - 1) * bn * 3);
    } else if (c->gd_cloud) {       // the installed cloud goal (capi_cloud_goal.h): rewards and g_state[H-1] in kb_reward's place, no seed staged
        ProbeScope ps(c, KC_BWD_REWARD);
        c->dv(DV_BWD_REWARD);
        CHK(cloud_goal_session_launch(c, B, N, H, nb, ptr<float>(c->rewards), 1, pass.host_rewards, g_state + (size_t)(H - 1) * bn * 3));
    } else {
        ProbeScope ps(c, KC_BWD_REWARD);
        c->dv(DV_BWD_REWARD);
        if (c->gd_S > 0) {          // a goal per row: row r belongs to scene (r / gd_scene_nb) % gd_S (drp_gd_begin_scenes)
            hipLaunchKernelGGL(kb_reward_scenes, dim3(B), dim3(256), KB_REWARD_LDS(N), st, states + (size_t)(H - 1) * N * 3, hstride,
                               N, goal_table(c, c->gd_scene_nb, 1), c->gt_h, c->gt_w, c->cam,
                               1, g_state + (size_t)(H - 1) * bn * 3, (size_t)N * 3, ptr<float>(c->rewards), pass.host_rewards);
        } else {
            hipLaunchKernelGGL(kb_reward, dim3(B), dim3(256), KB_REWARD_LDS(N), st, states + (size_t)(H - 1) * N * 3, hstride,
                               N, ptr<float>(c->goal_field), c->goal_h, c->goal_w, ptr<float>(c->goal_coor), c->goal_m, c->cam,
                               1, g_state + (size_t)(H - 1) * bn * 3, (size_t)N * 3, ptr<float>(c->rewards), pass.host_rewards);
        }
    }
    for (int t = H - 1; t >= 0; --t) {
        const float* s_prev = (t == 0) ? ptr<float>(c->ws.s_in) : states + (size_t)(t - 1) * N * 3;
        const int prev_mod = (t == 0) ? nb : B;
        const size_t prev_stride = (t == 0) ? (size_t)N * 3 : hstride;
        const int16_t* idx = ptr<int16_t>(c->tape_idx) + (size_t)t * bn * DRP_K;
        float* g_out = g_state + (size_t)t * bn * 3;
        BwdStep s{};
        s.B = B; s.N = N; s.mod = nb;
        s.eht = ptr<float>(c->eff_hist) + (size_t)t * 4 * bn * 64;
        s.mht = ptr<unsigned>(c->tape_mask) + (size_t)t * DRP_PSTEP * bn * DRP_K * 2;
        s.cnt = ptr<uint8_t>(c->tape_cnt) + (size_t)t * bn;
        s.rev_off = ptr<int>(c->rev_off); s.rev = ptr<int>(c->rev);
        s.sdelta = ptr<float>(c->tape_sdelta) + (size_t)t * bn * 3;
        s.g_out = g_out;
        s.gah = ptr<float>(c->g_agg_hist);
        s.ge_tmp = ptr<float>(c->g_eff); s.g_cnode = ptr<float>(c->g_cnode);
        for (int v = 0; v < 3; ++v) { s.d.ge[v] = ptr<float>(c->g_eff); s.d.gp[v] = ptr<float>(c->g_proj); }
        if (!rev_built) launch_reverse_lists(c, idx, s.cnt, N, B, nullptr, 0);
        // rows kernel, whole samples in one launch, or a launch per stage (dispatch.h: plan_backward)
        const BwdPlan k = plan_backward(c->pol, c->n_cu, B, N);
        c->dv(k.variant());
        if (k.kind == BwdPlan::ROWS) {
            ProbeScope ps(c, KC_BWD_NODE);
            hipLaunchKernelGGL(kmb_rows_bwd, dim3((unsigned)k.grid), dim3(64 * KMB_FUSED_WAVES),
                               KMB_ROWS_LDS, st, ptr<float>(c->w_mfma), ptr<float>(c->w_mfma_bwd), ptr<uint16_t>(c->w_split6),
                               ptr<uint16_t>(c->w_split6_bwd), s.eht, s.mht, s.cnt, s.rev_off, s.rev, g_out, (size_t)N * 3, s.sdelta,
                               ptr<float>(c->ws.attr), nb, ptr<float>(c->ws.dens), nb, N, B, k.gps, t > 0 ? s.gah : (float*)nullptr,
                               ptr<float>(c->g_sdelta));
        } else if (k.kind == BwdPlan::STEP) {
            ProbeScope ps(c, KC_BWD_NODE);
            hipLaunchKernelGGL((kmb_step_bwd<false, false>), dim3((unsigned)k.grid), dim3(64 * KMB_FUSED_WAVES), KMB_FUSED_LDS, st,
                               ptr<float>(c->w_mfma), ptr<float>(c->w_mfma_bwd), s.eht, s.mht, s.cnt, s.rev_off, s.rev,
                               g_out, (size_t)N * 3, s.sdelta, ptr<float>(c->ws.attr), nb,
                               ptr<float>(c->ws.dens), nb, N, B, k.spw, s.ge_tmp, s.g_cnode, s.gah,
                               ptr<float>(c->g_sdelta), KmbDump{}, 1, (unsigned*)nullptr, (unsigned*)nullptr);
        } else {
            launch_node_stages(c, s, dim3(B), 1, nullptr);
        }
        float* g_prev = nullptr;
        if (t > 0) {
            // d loss / d state[t-1] = residual share + relation encoder + gen_s_delta's position dependence
            g_prev = g_state + (size_t)(t - 1) * bn * 3;
            CHK(d2d(g_prev, g_out, bn * 3 * sizeof(float)));
            { ProbeScope ps(c, KC_BWD_EDGE);
            c->dv(DV_BWD_EDGE_MFMA);
            launch_edge_encode_mfma(c, s_prev, prev_mod, prev_stride, nb, idx, s.cnt, s.gah, s.mht, bn, N, B, ptr<float>(c->gpos_edge), KbEdgeDump{});
            }
            { ProbeScope ps(c, KC_BWD_EDGE);
            hipLaunchKernelGGL(kb_gather_pos, dim3((N + 255) / 256, B), dim3(256), 0, st, ptr<float>(c->gpos_edge),
                               s.rev_off, s.rev, N, g_prev, (size_t)N * 3, s.cnt,
                               seed_mid ? seed_mid + (size_t)(t - 1) * bn * 3 : (const float*)nullptr);
            }
        }
        { ProbeScope ps(c, KC_BWD_PUSH);
        hipLaunchKernelGGL(kb_sdelta, dim3(B), dim3(256), 0, st, s_prev, prev_mod, prev_stride,
                           ptr<float>(c->actions) + (size_t)t * 4, (size_t)H * 4, ptr<float>(c->g_sdelta), N, c->cam,
                           ptr<float>(c->g_act) + (size_t)t * 4, (size_t)H * 4, g_prev, (size_t)N * 3, t == 0 ? pass.adam : KbAdam{});
        }
    }
    HIPCHK(c, hipGetLastError());
    return DRP_OK;
}
}  // namespace

// S = 0: drp_gd_begin (the single goal).  S >= 1: drp_gd_begin_scenes -- nb is then S * (columns per scene).  S = -1:
// drp_gd_begin_cost -- a single-scene session that reads no goal
static int gd_begin_common(drp_ctx* c, int S_or_cost, const float* s0, const float* attr, const float* dens, int nb, int N,
                           const float* actions, int B, int H, double lr, const float act_lo[4], const float act_hi[4]) {
    const bool cost = S_or_cost < 0;
    const int S = cost ? 0 : S_or_cost;
    CHK(check_bn(c, B, N));
    if (!s0 || !attr || !dens || !actions || !act_lo || !act_hi) return fail(c, DRP_EINVAL, "null argument");
    if (H < 1 || H > 64) return fail(c, DRP_EINVAL, "bad horizon H=%d", H);
    if (nb <= 0 || B % nb != 0) return fail(c, DRP_EINVAL, S > 0 ? "B must be a multiple of S * n_batch" : "B must be a multiple of n_batch");
    HIPCHK(c, hipSetDevice(c->device));
    {
        // Adam moves the pushes, the clip keeps them in the box: bound by the box's diagonals and by the initial pushes
        const float box[8] = {act_lo[0], act_lo[1], act_hi[2], act_hi[3], act_hi[0], act_hi[1], act_lo[2], act_lo[3]};
        CHK(pick_tape_engine(c, max_abs(attr, (size_t)nb * N), max_abs(dens, (size_t)nb),
                             fmaxf(push_len_bound(c, box, 2), push_len_bound(c, actions, (size_t)B * H)), &c->gd_engine));
    }
    const size_t bn = (size_t)B * N;
    CHK(h2d(c, c->ws.s_in, s0, (size_t)nb * N * 3 * sizeof(float)));
    CHK(h2d(c, c->ws.attr, attr, (size_t)nb * N * sizeof(float)));
    CHK(h2d(c, c->ws.dens, dens, (size_t)nb * sizeof(float)));
    CHK(h2d(c, c->actions, actions, (size_t)B * H * 4 * sizeof(float)));
    CHK(ensure_step_ws(c, c->ws, B, N, c->gd_engine));
    CHK(ensure(c, c->states, (size_t)H * bn * 3 * sizeof(float)));
    CHK(ensure(c, c->rewards, (size_t)B * sizeof(float)));
    CHK(ensure_tape(c, B, N, H, 1));
    CHK(ensure(c, c->g_eff, bn * 64 * sizeof(float)));
    CHK(ensure(c, c->g_cnode, bn * 64 * sizeof(float)));
    CHK(ensure(c, c->g_proj, bn * 128 * sizeof(float)));
    CHK(ensure(c, c->g_state, (size_t)H * bn * 3 * sizeof(float)));
    CHK(ensure(c, c->g_act, (size_t)B * H * 4 * sizeof(float)));
    CHK(ensure(c, c->adam_m, (size_t)B * H * 4 * sizeof(float)));
    CHK(ensure(c, c->adam_v, (size_t)B * H * 4 * sizeof(float)));
    HIPCHK(c, hipMemsetAsync(c->adam_m.p, 0, (size_t)B * H * 4 * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(c->adam_v.p, 0, (size_t)B * H * 4 * sizeof(float), c->stream));
    CHK(guarded_wait(c, nullptr));
    c->gd_S = S; c->gd_scene_nb = S > 0 ? nb / S : 0;
    c->gd_cost = cost;
    c->gd_cloud = false;            // (drp_gd_begin_cloud sets it behind this)
    c->gd_nb = nb; c->gd_N = N; c->gd_B = B; c->gd_H = H; c->gd_iter = 0; c->gd_lr = lr;
    for (int q = 0; q < DRP_GD_SLOTS; ++q) c->gd_pending[q] = false;           // a new problem drops what the last one left in flight
    c->gd_cself_tag = 0;
    memcpy(c->gd_lo, act_lo, 4 * sizeof(float));
    memcpy(c->gd_hi, act_hi, 4 * sizeof(float));
    c->marks.lastH = H;
    c->gd_on = true;
    c->mpc_on = false;
    return DRP_OK;
}

int drp_gd_begin(drp_ctx* c, const float* s0, const float* attr, const float* dens, int nb, int N,
                 const float* actions, int B, int H, double lr, const float act_lo[4], const float act_hi[4]) {
    CHK(need(c, true, true, true));
    return gd_begin_common(c, 0, s0, attr, dens, nb, N, actions, B, H, lr, act_lo, act_hi);
}

int drp_gd_begin_cost(drp_ctx* c, const float* s0, const float* attr, const float* dens, int nb, int N,
                      const float* actions, int B, int H, double lr, const float act_lo[4], const float act_hi[4]) {
    CHK(need(c, true, true, false));
    return gd_begin_common(c, -1, s0, attr, dens, nb, N, actions, B, H, lr, act_lo, act_hi);
}

// drp_gd_begin with the installed cloud goal in the image's place (capi_cloud_goal.h)
int drp_gd_begin_cloud(drp_ctx* c, const float* s0, const float* attr, const float* dens, int nb, int N,
                       const float* actions, int B, int H, double lr, const float act_lo[4], const float act_hi[4]) {
    CHK(need(c, true, true, false));
    CHK(cloud_goal_session_check(c, N));
    CHK(gd_begin_common(c, 0, s0, attr, dens, nb, N, actions, B, H, lr, act_lo, act_hi));
    c->gd_on = false;               // until the goal's tables are in
    CHK(cloud_goal_session_begin(c, dens, nb, B, N, true));
    c->gd_cloud = true;
    c->gd_on = true;
    return DRP_OK;
}

int drp_gd_begin_scenes(drp_ctx* c, int S, const float* s0, const float* attr, const float* dens, int nb, int N,
                        const float* actions, int B, int H, double lr, const float act_lo[4], const float act_hi[4]) {
    CHK(need(c, true, true, false));
    if (S < 1 || S > DRP_MAX_SCENES) return fail(c, DRP_EINVAL, "%d scenes outside 1..%d", S, DRP_MAX_SCENES);
    if (c->gt_S <= 0) return fail(c, DRP_ESTATE, "no goal table installed (drp_set_goal_scenes)");
    if (c->gt_S != S) return fail(c, DRP_EINVAL, "a session of %d scenes on a goal table of %d", S, c->gt_S);
    if (nb <= 0 || nb > 0x7fffffff / S) return fail(c, DRP_EINVAL, "bad n_batch %d", nb);
    return gd_begin_common(c, S, s0, attr, dens, S * nb, N, actions, B, H, lr, act_lo, act_hi);
}

// what a session begun by drp_gd_begin_cost cannot do: everything that reads the built-in reward
static int no_cost_session(drp_ctx* c, const char* what) {
    if (c->gd_cost)
        return fail(c, DRP_ESTATE, "%s: the session was begun by drp_gd_begin_cost and has no reward of its own "
                                   "(drp_gd_predict, drp_gd_grad_seeded, drp_gd_step_seeded)", what);
    return DRP_OK;
}

// device layout [H][B,N,3] -> caller layout [B,H,N,3]
static int gd_copy_state_grad(drp_ctx* c, float* grad_state_out) {
    const size_t bn = (size_t)c->gd_B * c->gd_N;
    const size_t row = (size_t)c->gd_N * 3 * sizeof(float);
    for (int t = 0; t < c->gd_H; ++t)
        HIPCHK(c, hipMemcpy2DAsync(grad_state_out + (size_t)t * c->gd_N * 3, (size_t)c->gd_H * row,
                                   ptr<float>(c->g_state) + (size_t)t * bn * 3, row, row, c->gd_B,
                                   hipMemcpyDeviceToHost, c->stream));
    return DRP_OK;
}

int drp_gd_grad(drp_ctx* c, float* rewards_out, float* grad_act_out, float* grad_state_out) {
    if (!c || !c->gd_on) return fail(c, DRP_ESTATE, "drp_gd_begin not called");
    CHK(no_cost_session(c, "drp_gd_grad"));
    HIPCHK(c, hipSetDevice(c->device));
    DrainOnError drain(c);
    CHK(gd_forward_backward(c, GdPass{}));
    if (rewards_out) CHK(d2h(c, rewards_out, c->rewards.p, (size_t)c->gd_B * sizeof(float)));
    if (grad_act_out) CHK(d2h(c, grad_act_out, c->g_act.p, (size_t)c->gd_B * c->gd_H * 4 * sizeof(float)));
    if (grad_state_out) CHK(gd_copy_state_grad(c, grad_state_out));
    CHK(drp_sync(c));
    return drain.ok();
}

namespace {
// one iteration on the stream: forward, backward, Adam, clip -- the optimiser step of a row in the kb_sdelta launch that
// completes the row's gradient (rollout step 0's, the last of the backward pass): one launch fewer per iteration.
// host_rewards / host_actions (pinned; null for none): where the iteration's kernels also store its rewards and updated pushes
int gd_iteration(drp_ctx* c, float* host_rewards, float* host_actions, bool seeded = false /* drp_gd_step_seeded */) {
    // torch.optim.Adam: step_size = lr / (1 - beta1^t), denom = sqrt(v) / sqrt(1 - beta2^t) + eps
    const double it = (double)(c->gd_iter + 1);
    const double bc1 = 1.0 - pow(0.9, it), bc2 = 1.0 - pow(0.999, it);
    GdPass pass{KbAdam{}, host_rewards};
    pass.seeded = seeded;
    KbAdam& a = pass.adam;
    a.act = ptr<float>(c->actions); a.m = ptr<float>(c->adam_m); a.v = ptr<float>(c->adam_v); a.act_copy = host_actions;
    a.n_row = c->gd_H * 4;
    a.step_size = (float)(c->gd_lr / bc1); a.bc2_sqrt = (float)sqrt(bc2); a.b1 = 0.9f;
    a.lo = make_float4(c->gd_lo[0], c->gd_lo[1], c->gd_lo[2], c->gd_lo[3]);
    a.hi = make_float4(c->gd_hi[0], c->gd_hi[1], c->gd_hi[2], c->gd_hi[3]);
    CHK(gd_forward_backward(c, pass));
    c->gd_iter += 1;
    HIPCHK(c, hipGetLastError());
    return DRP_OK;
}
}  // namespace

int drp_gd_step(drp_ctx* c, float* rewards_out) {
    if (!c || !c->gd_on) return fail(c, DRP_ESTATE, "drp_gd_begin not called");
    CHK(no_cost_session(c, "drp_gd_step"));
    HIPCHK(c, hipSetDevice(c->device));
    DrainOnError drain(c);
    CHK(gd_iteration(c, nullptr, nullptr));
    if (rewards_out) {
        CHK(d2h(c, rewards_out, c->rewards.p, (size_t)c->gd_B * sizeof(float)));
        CHK(drp_sync(c));
    }
    return drain.ok();
}

// The planner's loop needs every iteration's rewards and updated pushes on the host (per-column bookkeeping,
// planners.py:721-727), but no iteration waits for the host: slot s of two takes the iteration's results into pinned
// memory behind the kernels, the caller enqueues the NEXT iteration before it waits for this one.
int drp_gd_step_async(drp_ctx* c, int slot) {
    if (!c || !c->gd_on) return fail(c, DRP_ESTATE, "drp_gd_begin not called");
    CHK(no_cost_session(c, "drp_gd_step_async"));
    if (slot < 0 || slot >= DRP_GD_SLOTS) return fail(c, DRP_EINVAL, "slot must be 0 .. %d", DRP_GD_SLOTS - 1);
    if (c->gd_pending[slot]) return fail(c, DRP_ESTATE, "slot %d holds an iteration nobody has waited for", slot);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nr = (size_t)c->gd_B, na = (size_t)c->gd_B * c->gd_H * 4;
    for (int q = 0; q < DRP_GD_SLOTS; ++q) {
        // a slot's block goes only while nothing is in flight: the kernels of a pending iteration write into it
        if (c->gd_pin[q].cap < (nr + na) * sizeof(float) && c->gd_pending[q])
            return fail(c, DRP_ESTATE, "the batch grew while an iteration was in flight");
        CHK(ensure_pinned(c, c->gd_pin[q], (nr + na) * sizeof(float)));
        HIPCHK(c, c->gd_ev[q].create(hipEventDisableTiming));
    }
    // the iteration's own kernels write the slot (pinned host memory is device-visible): kb_reward the rewards, k_adam
    // the updated pushes -- two copies fewer on the stream per iteration (they were 27 of 197 us at 20 particles)
    DrainOnError drain(c);                  // (an exit that leaves gd_pending[slot] false leaves nothing writing the slot either)
    CHK(gd_iteration(c, ptr<float>(c->gd_pin[slot]), ptr<float>(c->gd_pin[slot]) + nr));
    HIPCHK(c, hipEventRecord(c->gd_ev[slot].ev, c->stream));
    c->gd_pending[slot] = true;
    return drain.ok();
}

int drp_gd_wait(drp_ctx* c, int slot, float* rewards_out, float* actions_out) {
    if (!c) return DRP_EINVAL;
    if (c->gd_on) CHK(no_cost_session(c, "drp_gd_wait"));
    if (slot < 0 || slot >= DRP_GD_SLOTS || !c->gd_pending[slot]) return fail(c, DRP_ESTATE, "no iteration in flight in slot %d", slot);
    HIPCHK(c, hipSetDevice(c->device));
    c->gd_pending[slot] = false;
    CHK(guarded_wait(c, c->gd_ev[slot].ev));
    const size_t nr = (size_t)c->gd_B, na = (size_t)c->gd_B * c->gd_H * 4;
    if (rewards_out) memcpy(rewards_out, c->gd_pin[slot].p, nr * sizeof(float));
    if (actions_out) memcpy(actions_out, ptr<float>(c->gd_pin[slot]) + nr, na * sizeof(float));
    return DRP_OK;
}

// ---- planning on a caller's cost: every step's predicted state out, the caller's d loss / d s_pred in (GdPass: seeded) ----------
// Stateless between the calls, as the trainer's pair is: each seeded call runs the forward again (deterministic: the bits
// drp_gd_predict returned), so nothing has to mark the tape valid across whatever else touches the workspace in between.
namespace {
// a single-scene GD session, of either kind
int gd_seeded_session(drp_ctx* c, const char* what) {
    if (!c) return DRP_EINVAL;
    if (!c->gd_on) return fail(c, DRP_ESTATE, "%s: no GD session (drp_gd_begin, drp_gd_begin_cost)", what);
    if (c->gd_S > 0) return fail(c, DRP_ESTATE, "%s: a session of %d scenes takes no seed (drp_gd_begin, drp_gd_begin_cost)", what, c->gd_S);
    return DRP_OK;
}
// the seed's check and its one upload, the caller's layout (kb_seed_stage re-lays it on the device)
int gd_stage_seed(drp_ctx* c, const float* seed) {
    const int B = c->gd_B, H = c->gd_H, N = c->gd_N;
    const long bad = first_bad_plan_seed(seed, B, H, N);
    if (bad >= 0)
        return fail(c, DRP_EINVAL, "the seed of row %ld, step %ld, particle %ld is infinite or not a number", bad / ((long)H * N),
                    (bad / N) % H, bad % N);
    return h2d(c, c->gd_seed_in, seed, (size_t)B * H * N * 3 * sizeof(float));
}
}  // namespace

int drp_gd_predict(drp_ctx* c, float* states_out) {
    CHK(gd_seeded_session(c, "drp_gd_predict"));
    if (!states_out) return fail(c, DRP_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    DrainOnError drain(c);
    GdPass pass{};
    pass.forward_only = true;
    CHK(gd_forward_backward(c, pass));
    // the rollout's own layout is the caller's: [B][H][N][3]
    CHK(d2h(c, states_out, c->states.p, (size_t)c->gd_B * c->gd_H * c->gd_N * 3 * sizeof(float)));
    CHK(drp_sync(c));
    return drain.ok();
}

int drp_gd_grad_seeded(drp_ctx* c, const float* seed, float* grad_act_out, float* grad_state_out) {
    CHK(gd_seeded_session(c, "drp_gd_grad_seeded"));
    if (!seed) return fail(c, DRP_EINVAL, "null seed");
    HIPCHK(c, hipSetDevice(c->device));
    DrainOnError drain(c);
    CHK(gd_stage_seed(c, seed));
    GdPass pass{};
    pass.seeded = true;
    CHK(gd_forward_backward(c, pass));
    if (grad_act_out) CHK(d2h(c, grad_act_out, c->g_act.p, (size_t)c->gd_B * c->gd_H * 4 * sizeof(float)));
    if (grad_state_out) CHK(gd_copy_state_grad(c, grad_state_out));
    CHK(drp_sync(c));
    return drain.ok();
}

int drp_gd_step_seeded(drp_ctx* c, const float* seed, float* actions_out) {
    CHK(gd_seeded_session(c, "drp_gd_step_seeded"));
    if (!seed) return fail(c, DRP_EINVAL, "null seed");
    HIPCHK(c, hipSetDevice(c->device));
    DrainOnError drain(c);
    CHK(gd_stage_seed(c, seed));
    CHK(gd_iteration(c, nullptr, nullptr, true));
    if (actions_out) CHK(d2h(c, actions_out, c->actions.p, (size_t)c->gd_B * c->gd_H * 4 * sizeof(float)));
    CHK(drp_sync(c));
    return drain.ok();
}

int drp_gd_get(drp_ctx* c, float* actions_out) {
    if (!c || !c->gd_on) return fail(c, DRP_ESTATE, "drp_gd_begin not called");
    if (!actions_out) return fail(c, DRP_EINVAL, "null buffer");
    CHK(d2h(c, actions_out, c->actions.p, (size_t)c->gd_B * c->gd_H * 4 * sizeof(float)));
    return drp_sync(c);
}
