// capi_cloud_goal.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the planners' goal as a device-resident target cloud (k_cloud_goal.h; host arithmetic: cloud_goal_host.h):
// drp_set_goal_cloud, what a cloud session stages at its begin and launches for its rewards (drp_mpc_begin_cloud is capi_mpc.h's,
// drp_gd_begin_cloud capi_gd.h's, beside the sessions they are forms of), and the one-shot drp_cloud_goal_eval.

namespace {
const cloud_goal::Limits kCloudLimits{KC_MAX_POINTS, KT_MAX_POINTS, KT_MAX_ITERS};

int need_cloud_goal(drp_ctx* c) {
    if (!c->have_cloud_goal) return fail(c, DRP_ESTATE, "no cloud goal installed (drp_set_goal_cloud)");
    return DRP_OK;
}

// before a cloud session's begin touches anything: the goal, and the pile's size against the kind's limit
int cloud_goal_session_check(drp_ctx* c, int N) {
    CHK(need_cloud_goal(c));
    char msg[160];
    if (!cloud_goal::check_pred_points(c->cg_kind, N, kCloudLimits, msg, sizeof(msg))) return fail(c, DRP_EINVAL, "%s", msg);
    return DRP_OK;
}

// the installed goal's share of a launch's arguments; tab: eps [nb] then the target's self problem's value sums [nb]
void cloud_goal_fill(const drp_ctx* c, KgArgs& a, int N, const double* tab, int nb, double* scratch, int rows) {
    a.q = ptr<float>(c->cg_q); a.N = N; a.M = c->cg_M; a.weight = c->cg_weight;
    a.eps = tab; a.self_q = tab + nb; a.n_batch = nb; a.iters = c->cg_iters;
    a.vals = scratch; a.gsum = scratch + 2 * (size_t)rows;
}

// the target's self problem once per start column (the Sinkhorn kind; nothing for Chamfer): eps is already in tab[0 .. nb)
int cloud_goal_target_self(drp_ctx* c, double* tab, int nb) {
    if (c->cg_kind != cloud_goal::SINKHORN) return DRP_OK;
    KgArgs a{};
    cloud_goal_fill(c, a, 0, tab, nb, nullptr, 0);
    ProbeScope ps(c, KC_LOSS);
    hipLaunchKernelGGL(kg_target_self, dim3(nb), dim3(KT_THREADS), 0, c->stream, a, tab + nb);
    HIPCHK(c, hipGetLastError());
    return DRP_OK;
}

// behind a cloud session's begin: eps and the target's self problem per start column, the scratch of the session's launches
int cloud_goal_session_begin(drp_ctx* c, const float* dens, int nb, int rows, int N, bool grad) {
    if (c->cg_kind != cloud_goal::SINKHORN) return DRP_OK;
    std::vector<double> eps((size_t)nb);
    const int bad = cloud_goal::eps_table(c->cg_eps_scale, dens, nb, eps.data());
    if (bad >= 0) return fail(c, DRP_EINVAL, "dens[%d]=%g gives eps=%g, not a positive finite number", bad, (double)dens[bad], eps[(size_t)bad]);
    CHK(ensure(c, c->cg_tab, 2 * (size_t)nb * sizeof(double)));
    CHK(ensure(c, c->cg_scratch, (2 * (size_t)rows + (grad ? 2 * (size_t)rows * N * 3 : 0)) * sizeof(double)));
    const int rc = h2d(c, c->cg_tab, eps.data(), (size_t)nb * sizeof(double));
    const int rs = rc == DRP_OK ? cloud_goal_target_self(c, ptr<double>(c->cg_tab), nb) : rc;
    const int rw = guarded_wait(c, nullptr);            // (the staging vector is read until here)
    return rs != DRP_OK ? rs : rw;
}

// the reward of `rows` clouds against the installed goal: the caller fills where the clouds lie and where the results go, and
// holds the ProbeScope and the dispatch mark of the launch it stands for
int cloud_goal_launch(drp_ctx* c, KgArgs a, int rows, int N, bool grad, const double* tab, int nb, double* scratch) {
    cloud_goal_fill(c, a, N, tab, nb, scratch, rows);
    if (c->cg_kind == cloud_goal::CHAMFER) {
        if (grad) hipLaunchKernelGGL((kg_chamfer<true>), dim3(rows), dim3(KC_THREADS), 0, c->stream, a);
        else hipLaunchKernelGGL((kg_chamfer<false>), dim3(rows), dim3(KC_THREADS), 0, c->stream, a);
    } else if (grad) {
        hipLaunchKernelGGL((kg_sinkhorn<true>), dim3(rows, 2), dim3(KT_THREADS), 0, c->stream, a);
        hipLaunchKernelGGL((kg_sinkhorn_combine<true>), dim3(rows), dim3(KD_COMBINE_THREADS), 0, c->stream, a);
    } else {
        hipLaunchKernelGGL((kg_sinkhorn<false>), dim3(rows, 2), dim3(KT_THREADS), 0, c->stream, a);
        hipLaunchKernelGGL((kg_sinkhorn_combine<false>), dim3(rows), dim3(KD_COMBINE_THREADS), 0, c->stream, a);
    }
    HIPCHK(c, hipGetLastError());
    return DRP_OK;
}

// a session's launch: the final step of c->states [rows][H][N][3]; rewards at `rewards` with `reward_stride`; with g_last
// (GD) the gradient [rows][N][3] and the pinned copy of the rewards
int cloud_goal_session_launch(drp_ctx* c, int rows, int N, int H, int nb, float* rewards, size_t reward_stride, float* host_rewards,
                              float* g_last) {
    KgArgs a{};
    a.states = ptr<float>(c->states) + (size_t)(H - 1) * N * 3; a.row_stride = (size_t)H * N * 3;
    a.rewards = rewards; a.reward_stride = reward_stride; a.host_rewards = host_rewards;
    a.grad = g_last; a.grad_stride = (size_t)N * 3;
    return cloud_goal_launch(c, a, rows, N, g_last != nullptr, ptr<double>(c->cg_tab), nb, ptr<double>(c->cg_scratch));
}
}  // namespace

int drp_set_goal_cloud(drp_ctx* c, const float* q, int M, const drp_cloud_goal_params* p) {
    if (!c) return DRP_EINVAL;
    if (!q || !p) return fail(c, DRP_EINVAL, "null argument");
    char msg[160];
    if (!cloud_goal::check_params(p->kind, p->weight, p->eps_scale, p->iters, M, kCloudLimits, msg, sizeof(msg)))
        return fail(c, DRP_EINVAL, "%s", msg);
    const long bad = cloud_goal::first_nonfinite(q, (size_t)M * 3);
    if (bad >= 0) return fail(c, DRP_EINVAL, "q[%ld][%ld] is not finite", bad / 3, bad % 3);
    HIPCHK(c, hipSetDevice(c->device));
    // a running cloud session reads the goal it began on (its tables are that goal's): a new goal ends it
    if (c->mpc_on && c->mpc_cloud) c->mpc_on = false;
    if (c->gd_on && c->gd_cloud) c->gd_on = false;
    c->have_cloud_goal = false;
    CHK(h2d(c, c->cg_q, q, (size_t)M * 3 * sizeof(float)));
    CHK(guarded_wait(c, nullptr));                      // (the caller's array is free when this returns)
    c->cg_kind = p->kind; c->cg_M = M; c->cg_weight = p->weight;
    c->cg_eps_scale = p->kind == cloud_goal::SINKHORN ? p->eps_scale : 1.0;
    c->cg_iters = p->kind == cloud_goal::SINKHORN ? p->iters : 0;
    c->have_cloud_goal = true;
    return DRP_OK;
}

// The installed goal on the caller's clouds.  Nothing of a session is read or written: inputs, tables, scratch and results lie
// in c->cg_io, the call ends in a wait.  A non-finite coordinate is NOT refused: its row's reward is NaN (the planner's
// winner re-rollout of a diverged model must come back), every other row is untouched by it.
int drp_cloud_goal_eval(drp_ctx* c, const float* p, const int32_t* n_p, const float* dens, int B, int N, float* rewards_out,
                        double* values_out, float* grad_out) {
    if (!c) return DRP_EINVAL;
    CHK(need_cloud_goal(c));
    CHK(check_bn(c, B, N));
    char msg[160];
    if (!cloud_goal::check_pred_points(c->cg_kind, N, kCloudLimits, msg, sizeof(msg))) return fail(c, DRP_EINVAL, "%s", msg);
    if (!p) return fail(c, DRP_EINVAL, "null argument");
    const int badn = cloud_goal::first_bad_count(n_p, B, N);
    if (badn >= 0) return fail(c, DRP_EINVAL, "n_p[%d]=%d outside 1..%d", badn, n_p[badn], N);
    const bool sink = c->cg_kind == cloud_goal::SINKHORN, grad = grad_out != nullptr;
    std::vector<double> eps;
    if (sink) {
        if (!dens) return fail(c, DRP_EINVAL, "null dens (the Sinkhorn kind's eps is eps_scale / dens[row])");
        eps.resize((size_t)B);
        const int bad = cloud_goal::eps_table(c->cg_eps_scale, dens, B, eps.data());
        if (bad >= 0) return fail(c, DRP_EINVAL, "dens[%d]=%g gives eps=%g, not a positive finite number", bad, (double)dens[bad], eps[(size_t)bad]);
    }
    HIPCHK(c, hipSetDevice(c->device));
    // doubles first, then the 4-byte blocks: tab [2B] | scratch [2B (+ 2B N 3)] | values [B] | p | grad | rewards | n_p
    const size_t bn3 = (size_t)B * N * 3;
    const size_t n_scr = sink ? 2 * (size_t)B + (grad ? 2 * bn3 : 0) : 0;
    const size_t off_tab = 0, off_scr = off_tab + 2 * (size_t)B * 8, off_val = off_scr + n_scr * 8, off_p = off_val + (size_t)B * 8;
    const size_t off_grad = off_p + bn3 * 4, off_rew = off_grad + bn3 * 4, off_np = off_rew + (size_t)B * 4, bytes = off_np + (size_t)B * 4;
    CHK(ensure(c, c->cg_io, bytes));
    char* io = ptr<char>(c->cg_io);
    double* tab = reinterpret_cast<double*>(io + off_tab);
    int rc = DRP_OK;
    auto up = [&](size_t off, const void* src, size_t n) {
        if (rc == DRP_OK && hipMemcpyAsync(io + off, src, n, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            rc = fail(c, DRP_EHIP, "hipMemcpyAsync of the one-shot's inputs");
    };
    up(off_p, p, bn3 * 4);
    if (n_p) up(off_np, n_p, (size_t)B * 4);
    if (sink) up(off_tab, eps.data(), (size_t)B * 8);
    if (rc == DRP_OK) rc = cloud_goal_target_self(c, tab, B);
    if (rc == DRP_OK) {
        KgArgs a{};
        a.states = reinterpret_cast<const float*>(io + off_p); a.row_stride = (size_t)N * 3;
        a.n_p = n_p ? reinterpret_cast<const int*>(io + off_np) : nullptr;
        a.rewards = reinterpret_cast<float*>(io + off_rew); a.reward_stride = 1;
        a.values = reinterpret_cast<double*>(io + off_val);
        a.grad = grad ? reinterpret_cast<float*>(io + off_grad) : nullptr; a.grad_stride = (size_t)N * 3;
        ProbeScope ps(c, KC_LOSS);
        rc = cloud_goal_launch(c, a, B, N, grad, tab, B, reinterpret_cast<double*>(io + off_scr));
    }
    if (rc == DRP_OK && rewards_out) rc = d2h(c, rewards_out, io + off_rew, (size_t)B * 4);
    if (rc == DRP_OK && values_out) rc = d2h(c, values_out, io + off_val, (size_t)B * 8);
    if (rc == DRP_OK && grad) rc = d2h(c, grad_out, io + off_grad, bn3 * 4);
    const int rw = guarded_wait(c, nullptr);            // also behind an error: the caller's arrays and eps are read until here
    return rc != DRP_OK ? rc : rw;
}
