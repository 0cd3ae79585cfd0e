// capi_core.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: life cycle, model constants and the single operations on host buffers (drp_create ... drp_reward).

int drp_create(int device, drp_ctx** out) {
    if (!out) return fail(nullptr, DRP_EINVAL, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, DRP_EHIP, "no HIP device available: %s", hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(nullptr, DRP_EINVAL, "device %d out of range (%d)", device, n);
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, DRP_EHIP, "hipSetDevice: %s", hipGetErrorString(e));
    std::unique_ptr<drp_ctx> c(new drp_ctx());      // a failure exit below destroys it, its stream included
    c->device = device;
    c->wgrad.reset(new WgradQueue(c.get()));
    e = hipStreamCreateWithFlags(&c->stream.s, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(nullptr, DRP_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        c->n_cu = prop.multiProcessorCount;
    c->pol = policy_from_env();       // the DRP_* switches of the dispatch (dispatch.h: env_switches)
    c->repack_device = getenv("DRP_NO_REPACK_DEVICE") == nullptr;
    c->wgrad_defer = getenv("DRP_NO_WGRAD_DEFER") == nullptr;
    c->debug_force_giveup = getenv("DRP_DEBUG_FORCE_GIVEUP") != nullptr;
    c->train_copy_upload = getenv("DRP_TRAIN_COPY_UPLOAD") != nullptr;
    c->comm_always = getenv("DRP_COMM_ALWAYS") != nullptr;
    if (const char* e = getenv("DRP_COMM_TIMEOUT_S")) { const double v = atof(e); if (v > 0.0) c->comm_timeout_s = v; }
    if (const char* e = getenv("DRP_COMM_INIT_TIMEOUT_S")) { const double v = atof(e); if (v > 0.0) c->comm_init_timeout_s = v; }
    if (hipFuncSetAttribute((const void*)k_graph, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void*)k_graph_q4, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void*)km_graph_q4_encode<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void*)km_graph_q4_encode<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void*)k_elite_local, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void*)k_elite_update, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void*)k_graph_strips_q<GRAPH_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void*)k_graph_strips_q<256>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void*)kb_reward, hipFuncAttributeMaxDynamicSharedMemorySize, (int)KB_REWARD_LDS(4096)) != hipSuccess ||
        hipFuncSetAttribute((const void*)kb_reward_scenes, hipFuncAttributeMaxDynamicSharedMemorySize, (int)KB_REWARD_LDS(4096)) != hipSuccess ||
        hipFuncSetAttribute((const void*)kb_reverse_lists<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)KB_REV_LDS(KB_REV_LDS_MAX_N, 1)) != hipSuccess ||
        hipFuncSetAttribute((const void*)kb_reverse_lists<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)KB_REV_LDS(KB_REV_LDS_MAX_N, 1)) != hipSuccess ||
        hipFuncSetAttribute((const void*)k_aggregate_lds, hipFuncAttributeMaxDynamicSharedMemorySize,
                            K_AGG_LDS_MAX_N * 256) != hipSuccess)
        return fail(nullptr, DRP_EHIP, "hipFuncSetAttribute (dynamic LDS size of k_graph, kb_reverse_lists or k_aggregate_lds) failed");
    // the MFMA kernels keep packed weights + per-wave transposition tiles in LDS (> 64 KiB)
    if (hipFuncSetAttribute((const void*)km_edge_encode, hipFuncAttributeMaxDynamicSharedMemorySize, KM_EDGE_LDS) != hipSuccess ||
        hipFuncSetAttribute((const void*)km_node_encode, hipFuncAttributeMaxDynamicSharedMemorySize, KM_NODE_LDS) != hipSuccess ||
        hipFuncSetAttribute((const void*)km_edge_encode_split, hipFuncAttributeMaxDynamicSharedMemorySize, KM_EDGE_SPLIT_LDS) != hipSuccess ||
        hipFuncSetAttribute((const void*)km_node_encode_split<false>, hipFuncAttributeMaxDynamicSharedMemorySize, KM_NODE_SPLIT_LDS) != hipSuccess ||
        hipFuncSetAttribute((const void*)km_node_encode_split<true>, hipFuncAttributeMaxDynamicSharedMemorySize, KM_NODE_SPLIT_LDS) != hipSuccess ||
        !prop_tables_ready() ||               // km_prop / km_prop3 / km_rollout: every instantiation of the launch tables
        hipFuncSetAttribute((const void*)kmb_step_bwd<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, KMB_FUSED_LDS) != hipSuccess ||
        hipFuncSetAttribute((const void*)kmb_step_bwd<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, KMB_FUSED_LDS) != hipSuccess ||
        hipFuncSetAttribute((const void*)kmb_step_bwd<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, KMB_COOP_LDS) != hipSuccess ||
        hipFuncSetAttribute((const void*)kmb_rows_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, KMB_ROWS_LDS) != hipSuccess ||
        hipFuncSetAttribute((const void*)kmb_edge_encode, hipFuncAttributeMaxDynamicSharedMemorySize, KMB_EDGE_ENCODE_LDS) != hipSuccess ||
        hipFuncSetAttribute((const void*)kt_wgrad_multi, hipFuncAttributeMaxDynamicSharedMemorySize, KT_WGRAD_MULTI_LDS) != hipSuccess ||
        hipFuncSetAttribute((const void*)kt_wgrad_mfma_multi, hipFuncAttributeMaxDynamicSharedMemorySize, KT_WGRAD_MULTI_LDS) != hipSuccess ||
        hipFuncSetAttribute((const void*)km_update<false>, hipFuncAttributeMaxDynamicSharedMemorySize, KM_UPD_LDS) != hipSuccess ||
        hipFuncSetAttribute((const void*)km_update<true>, hipFuncAttributeMaxDynamicSharedMemorySize, KM_UPD_LDS) != hipSuccess)
        return fail(nullptr, DRP_EHIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    c->engine = DRP_ENGINE_FUSED;
    *out = c.release();
    return DRP_OK;
}

void drp_destroy(drp_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)guarded_wait(c, nullptr);           // a collective that cannot finish must not keep the destructor
    helpers_wait(5.0, c);                     // no helper thread of this context (an abort, an init) inside RCCL while its stream goes away
    if (c->comm) { RcclApi* R = rccl_api(); if (R) (void)R->CommDestroy(c->comm); c->comm = nullptr; }
    delete c;                                 // every member frees what it owns (capi_ctx.h), the stream last
}

const char* drp_last_error(const drp_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int drp_sync(drp_ctx* c) {
    if (!c) return DRP_EINVAL;
    return guarded_wait(c, nullptr);
}

int drp_set_engine(drp_ctx* c, int engine) {
    if (!c) return DRP_EINVAL;
    if (engine == DRP_ENGINE_VALU) { c->engine = engine; return DRP_OK; }
    if (engine == DRP_ENGINE_MFMA || engine == DRP_ENGINE_SPLIT || engine == DRP_ENGINE_FUSED || engine == DRP_ENGINE_LITE) {
        c->engine = engine;
        return DRP_OK;
    }
    return fail(c, DRP_EINVAL, "engine %d not available in this build", engine);
}

int drp_device_info(drp_ctx* c, char* name, size_t name_len, int* n_cu, size_t* hbm_bytes) {
    if (!c) return DRP_EINVAL;
    hipDeviceProp_t p;
    HIPCHK(c, hipGetDeviceProperties(&p, c->device));
    if (name && name_len) snprintf(name, name_len, "%s (%s)", p.name, p.gcnArchName);
    if (n_cu) *n_cu = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = p.totalGlobalMem;
    return DRP_OK;
}

int drp_load_weights(drp_ctx* c, const float* blob, size_t n_floats, double adj_thresh) {
    if (!c || !blob) return DRP_EINVAL;
    if (n_floats != (size_t)W_TOTAL)
        return fail(c, DRP_EINVAL, "weight blob has %zu floats, expected %d", n_floats, (int)W_TOTAL);
    HIPCHK(c, hipSetDevice(c->device));
    // the packed host images: every upload below is only enqueued, so they live until the one wait
    std::vector<float> v, m, mbv;
    std::vector<uint16_t> sp, sp6;
    pack_valu(blob, v);
    CHK(h2d(c, c->w_raw, blob, n_floats * sizeof(float)));
    CHK(h2d(c, c->w_valu, v.data(), v.size() * sizeof(float)));
    pack_mfma(blob, m);
    CHK(h2d(c, c->w_mfma, m.data(), m.size() * sizeof(float)));
    pack_mfma_bwd(blob, mbv);
    CHK(h2d(c, c->w_mfma_bwd, mbv.data(), mbv.size() * sizeof(float)));
    set_split_range(c, blob);
    pack_split(blob, sp, c->re_range.shift);
    CHK(h2d(c, c->w_split, sp.data(), sp.size() * sizeof(uint16_t)));
    pack_split6(blob, sp6);
    CHK(h2d(c, c->w_split6, sp6.data(), sp6.size() * sizeof(uint16_t)));
    // the transposed layers of the GD planner's backward pass in the same split: packed on the device from the raw blob
    CHK(ensure(c, c->w_split6_bwd, (size_t)SB6_TOTAL * 16));
    hipLaunchKernelGGL(kt_repack_split6_bwd, dim3(6 * 16), dim3(256), 0, c->stream, ptr<float>(c->w_raw), ptr<uint16_t>(c->w_split6_bwd));
    CHK(f64_refresh_weights(c));          // the float64 yardstick's copy (capi_f64.h)
    CHK(guarded_wait(c, nullptr));
    c->w_host.assign(blob, blob + n_floats);
    c->adj_thresh = adj_thresh;
    // threshold = adj_thresh * adj_thresh in Python doubles, then an fp32 scalar (model/gnn_dyn.py:229,236): the radius
    // arrives as the double it is there -- squaring its fp32 rounding gives another threshold at 0.05, 0.1, 0.7
    c->thr = (float)(adj_thresh * adj_thresh);
    c->have_weights = true;
    c->tr_grad_fresh = false;             // a gradient taken at the old weights is nothing drp_train_accumulate may add
    return DRP_OK;
}

int drp_set_camera(drp_ctx* c, const float m34[12], float global_scale, const float intr[4]) {
    if (!c || !m34 || !intr) return DRP_EINVAL;
    memcpy(c->cam.m, m34, 12 * sizeof(float));
    c->cam.gs = global_scale;
    c->cam.fx = intr[0]; c->cam.fy = intr[1]; c->cam.cx = intr[2]; c->cam.cy = intr[3];
    c->have_cam = true;
    return DRP_OK;
}

int drp_set_goal(drp_ctx* c, const float* field, int h, int w, const float* goal_coor, int m) {
    if (!c || !field || !goal_coor || h <= 0 || w <= 0 || m <= 0) return fail(c, DRP_EINVAL, "bad goal");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(h2d(c, c->goal_field, field, (size_t)h * w * sizeof(float)));
    CHK(h2d(c, c->goal_coor, goal_coor, (size_t)m * 2 * sizeof(float)));
    CHK(guarded_wait(c, nullptr));
    c->goal_h = h; c->goal_w = w; c->goal_m = m;
    c->have_goal = true;
    return DRP_OK;
}

// A new table ends the sessions that read the old one (their kernels take the table's shape at every launch).
static void end_scene_sessions(drp_ctx* c) {
    if (c->mpc_on && c->mpc_S > 0) { c->mpc_on = false; c->mpc_pending[0] = c->mpc_pending[1] = false; }
    if (c->gd_on && c->gd_S > 0) { c->gd_on = false; for (int q = 0; q < DRP_GD_SLOTS; ++q) c->gd_pending[q] = false; }
}

int drp_set_goal_scenes(drp_ctx* c, int S, const float* fields, int h, int w, const float* goal_coor, const int32_t* m, int m_max) {
    if (!c || !fields || !goal_coor || !m || h <= 0 || w <= 0 || m_max <= 0) return fail(c, DRP_EINVAL, "bad goal table");
    if (S < 1 || S > DRP_MAX_SCENES) return fail(c, DRP_EINVAL, "%d scenes outside 1..%d", S, DRP_MAX_SCENES);
    for (int k = 0; k < S; ++k)
        if (m[k] < 1 || m[k] > m_max) return fail(c, DRP_EINVAL, "scene %d has %d goal pixels, outside 1..m_max=%d", k, (int)m[k], m_max);
    HIPCHK(c, hipSetDevice(c->device));
    end_scene_sessions(c);
    c->gt_S = 0;
    CHK(h2d(c, c->gt_fields, fields, (size_t)S * h * w * sizeof(float)));
    CHK(h2d(c, c->gt_coor, goal_coor, (size_t)S * m_max * 2 * sizeof(float)));
    CHK(h2d(c, c->gt_m, m, (size_t)S * sizeof(int32_t)));
    CHK(guarded_wait(c, nullptr));
    c->gt_S = S; c->gt_h = h; c->gt_w = w; c->gt_m_max = m_max;
    return DRP_OK;
}

int drp_gen_s_delta(drp_ctx* c, const float* s_cur, const float* action, int B, int N, float* out) {
    CHK(need(c, false, true, false));
    CHK(check_bn(c, B, N));
    if (!s_cur || !action || !out) return fail(c, DRP_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    end_sessions(c);
    CHK(h2d(c, c->ws.s_in, s_cur, (size_t)B * N * 3 * sizeof(float)));
    CHK(h2d(c, c->actions, action, (size_t)B * 4 * sizeof(float)));
    CHK(ensure(c, c->ws.s_delta, (size_t)B * N * 3 * sizeof(float)));
    hipLaunchKernelGGL(k_sdelta, dim3(B), dim3(256), 0, c->stream, ptr<float>(c->ws.s_in),
                       ptr<float>(c->actions), N, ptr<float>(c->ws.s_delta), c->cam);
    HIPCHK(c, hipGetLastError());
    CHK(d2h(c, out, c->ws.s_delta.p, (size_t)B * N * 3 * sizeof(float)));
    return drp_sync(c);
}

int drp_build_graph(drp_ctx* c, const float* s_cur, const float* s_delta, int B, int N,
                    int16_t* nbr_idx_out, uint8_t* nbr_cnt_out) {
    CHK(need(c, true, false, false));
    CHK(check_bn(c, B, N));
    if (!s_cur || !s_delta || !nbr_idx_out || !nbr_cnt_out) return fail(c, DRP_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    end_sessions(c);
    CHK(ensure_step_ws(c, c->ws, B, N));
    CHK(h2d(c, c->ws.s_in, s_cur, (size_t)B * N * 3 * sizeof(float)));
    CHK(h2d(c, c->ws.s_delta, s_delta, (size_t)B * N * 3 * sizeof(float)));
    {
    ProbeScope ps(c, KC_GRAPH);
    const GraphPlan g = plan_graph(c->pol, c->n_cu, c->engine, B, N, false, false, false, true);    // the lists alone: no launch to share
    c->dv(g.variant());
    launch_graph(c, c->stream, g, ptr<float>(c->ws.s_in), B, (size_t)N * 3, (const float*)nullptr, (size_t)0,
                 ptr<float>(c->ws.s_delta), B, N, ptr<int16_t>(c->ws.nbr_idx), ptr<uint8_t>(c->ws.nbr_cnt), 0);
    }
    HIPCHK(c, hipGetLastError());
    CHK(d2h(c, nbr_idx_out, c->ws.nbr_idx.p, (size_t)B * N * DRP_K * sizeof(int16_t)));
    CHK(d2h(c, nbr_cnt_out, c->ws.nbr_cnt.p, (size_t)B * N));
    return drp_sync(c);
}

static int step_common(drp_ctx* c, const float* a_cur, const float* s_cur, const float* s_delta,
                       const float* dens, const int16_t* nbr_idx, const uint8_t* nbr_cnt, int B, int N,
                       float* s_pred_out) {
    CHK(need(c, true, false, false));
    CHK(check_bn(c, B, N));
    if (!a_cur || !s_cur || !s_delta || !dens || !s_pred_out) return fail(c, DRP_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    end_sessions(c);
    CHK(range_check(c, c->engine, max_abs(a_cur, (size_t)B * N), max_abs(dens, (size_t)B), max_abs(s_delta, (size_t)B * N * 3)));
    CHK(ensure_step_ws(c, c->ws, B, N));
    const size_t bn = (size_t)B * N;
    CHK(h2d(c, c->ws.s_in, s_cur, bn * 3 * sizeof(float)));
    CHK(h2d(c, c->ws.s_delta, s_delta, bn * 3 * sizeof(float)));
    CHK(h2d(c, c->ws.attr, a_cur, bn * sizeof(float)));
    CHK(h2d(c, c->ws.dens, dens, (size_t)B * sizeof(float)));
    CHK(ensure(c, c->ws.s_out, bn * 3 * sizeof(float)));
    if (nbr_idx) {
        CHK(h2d(c, c->ws.nbr_idx, nbr_idx, bn * DRP_K * sizeof(int16_t)));
        CHK(h2d(c, c->ws.nbr_cnt, nbr_cnt, bn));
    }
    StepArgs a = step_args(c, c->engine);
    a.s_prev = ptr<float>(c->ws.s_in); a.prev_mod = B; a.prev_stride = (size_t)N * 3;
    a.attr = ptr<float>(c->ws.attr); a.attr_mod = B;
    a.dens = ptr<float>(c->ws.dens); a.dens_mod = B;
    a.actions = nullptr; a.act_stride = 0;
    a.build_graph = (nbr_idx == nullptr);
    a.s_out = ptr<float>(c->ws.s_out); a.out_stride = (size_t)N * 3;
    a.B = B; a.N = N;
    CHK(run_step(c, a));
    CHK(d2h(c, s_pred_out, c->ws.s_out.p, bn * 3 * sizeof(float)));
    return drp_sync(c);
}

int drp_step(drp_ctx* c, const float* a_cur, const float* s_cur, const float* s_delta,
             const float* dens, int B, int N, float* s_pred_out) {
    return step_common(c, a_cur, s_cur, s_delta, dens, nullptr, nullptr, B, N, s_pred_out);
}

int drp_forward(drp_ctx* c, const float* a_cur, const float* s_cur, const float* s_delta,
                const float* dens, const int16_t* nbr_idx, const uint8_t* nbr_cnt, int B, int N,
                float* s_pred_out) {
    if (!nbr_idx || !nbr_cnt) return fail(c, DRP_EINVAL, "null neighbour lists");
    return step_common(c, a_cur, s_cur, s_delta, dens, nbr_idx, nbr_cnt, B, N, s_pred_out);
}

int drp_rollout(drp_ctx* c, const float* s0, const float* attr, const float* dens, int nb, int N,
                const float* actions, int B, int H, float* states_out, float* reward_out) {
    CHK(need(c, true, true, reward_out != nullptr));
    CHK(check_bn(c, B, N));
    if (!s0 || !attr || !dens || !actions) return fail(c, DRP_EINVAL, "null buffer");
    if (nb <= 0 || H <= 0 || B % nb != 0)
        return fail(c, DRP_EINVAL, "bad rollout shape nb=%d B=%d H=%d (B must be a multiple of nb)", nb, B, H);
    HIPCHK(c, hipSetDevice(c->device));
    end_sessions(c);
    CHK(range_check(c, c->engine, max_abs(attr, (size_t)nb * N), max_abs(dens, (size_t)nb), push_len_bound(c, actions, (size_t)B * H)));
    CHK(h2d(c, c->ws.s_in, s0, (size_t)nb * N * 3 * sizeof(float)));
    CHK(h2d(c, c->ws.attr, attr, (size_t)nb * N * sizeof(float)));
    CHK(h2d(c, c->ws.dens, dens, (size_t)nb * sizeof(float)));
    CHK(h2d(c, c->actions, actions, (size_t)B * H * 4 * sizeof(float)));
    CHK(run_rollout(c, nb, N, B, H, reward_out != nullptr, false));
    if (states_out) CHK(d2h(c, states_out, c->states.p, (size_t)B * H * N * 3 * sizeof(float)));
    if (reward_out) CHK(d2h(c, reward_out, c->rewards.p, (size_t)B * H * sizeof(float)));
    return drp_sync(c);
}

int drp_reward(drp_ctx* c, const float* state, int Bp, int N, int normalize, float* reward_out) {
    CHK(need(c, false, true, true));
    CHK(check_bn(c, Bp, N));
    if (!state || !reward_out) return fail(c, DRP_EINVAL, "null buffer");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(h2d(c, c->ws.s_out, state, (size_t)Bp * N * 3 * sizeof(float)));
    CHK(ensure(c, c->scratch, (size_t)Bp * sizeof(float)));
    CHK(run_reward(c, ptr<float>(c->ws.s_out), (size_t)N * 3, Bp, N, normalize, ptr<float>(c->scratch)));
    CHK(d2h(c, reward_out, c->scratch.p, (size_t)Bp * sizeof(float)));
    return drp_sync(c);
}

int drp_reward_scenes(drp_ctx* c, const float* state, const int32_t* scene, int Bp, int N, int normalize, float* reward_out) {
    CHK(need(c, false, true, false));
    if (c->gt_S <= 0) return fail(c, DRP_ESTATE, "no goal table installed (drp_set_goal_scenes)");
    CHK(check_bn(c, Bp, N));
    if (!state || !scene || !reward_out) return fail(c, DRP_EINVAL, "null buffer");
    for (int r = 0; r < Bp; ++r)
        if (scene[r] < 0 || scene[r] >= c->gt_S) return fail(c, DRP_EINVAL, "row %d names scene %d, outside the table's 0..%d", r, (int)scene[r], c->gt_S - 1);
    HIPCHK(c, hipSetDevice(c->device));
    CHK(h2d(c, c->ws.s_out, state, (size_t)Bp * N * 3 * sizeof(float)));
    CHK(h2d(c, c->gt_rows, scene, (size_t)Bp * sizeof(int32_t)));
    CHK(ensure(c, c->scratch, (size_t)Bp * sizeof(float)));
    CHK(run_reward(c, ptr<float>(c->ws.s_out), (size_t)N * 3, Bp, N, normalize, ptr<float>(c->scratch), c->gt_S, 1, 1, ptr<int>(c->gt_rows)));
    CHK(d2h(c, reward_out, c->scratch.p, (size_t)Bp * sizeof(float)));
    return drp_sync(c);
}
