// capi_debug.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: measurement and debugging entry points (probes, dispatch introspection, range info, buffer fetch).

// ---- measurement / debugging -----------------------------------------------------------------
#ifdef PROP_STAMPS
int drp_debug_prop_stamps(drp_ctx* c, unsigned long long* out8, int reset) {
    (void)c;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    std::vector<unsigned long long> h(4096 * 8);
    if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_prop_stamps), h.size() * 8) != hipSuccess) return -1;
    if (out8) {
        for (int q = 0; q < 8; ++q) out8[q] = 0;
        for (size_t i = 0; i < h.size(); ++i) out8[i & 7] += h[i];
    }
    if (reset) {
        std::fill(h.begin(), h.end(), 0ull);
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_prop_stamps), h.data(), h.size() * 8) != hipSuccess) return -1;
    }
    return 0;
}
#endif

#ifdef PROP_STAMPS
int drp_debug_prop_span(drp_ctx* c, unsigned long long* out, int n) {
    (void)c;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (n > 4096 * 2) n = 4096 * 2;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prop_span), (size_t)n * 8) == hipSuccess ? 0 : -1;
}
#endif

int drp_probe_begin(drp_ctx* c, const char* kernel_class) {
    if (!c) return DRP_EINVAL;
    c->marks.probe_cls = -1;
    c->probe_used = 0;
    c->probe_prop_kernels = 0;
    c->probe_count = false;
    c->work_lite = c->work_full = false;
    if (!kernel_class || !*kernel_class) return DRP_OK;
    if (strcmp(kernel_class, "prop+work") == 0) { kernel_class = "prop"; c->probe_count = true; }
    for (int i = 0; i < KC_COUNT; ++i)
        if (strcmp(kernel_class, kclass_names[i]) == 0) {
            if (i == KC_PROP && c->probe_count) {
                HIPCHK(c, hipSetDevice(c->device));
                CHK(ensure(c, c->probe_work, PROP_WORK_SHARDS * PROP_WORK_STRIDE * sizeof(unsigned long long)));
                HIPCHK(c, hipMemsetAsync(c->probe_work.p, 0, PROP_WORK_SHARDS * PROP_WORK_STRIDE * sizeof(unsigned long long), c->stream));
            }
            c->marks.probe_cls = i;
            return DRP_OK;
        }
    return fail(c, DRP_EINVAL, "unknown kernel class '%s'", kernel_class);
}

int drp_probe_work(drp_ctx* c, unsigned long long out[8]) {
    if (!c || !out) return fail(c, DRP_EINVAL, "null argument");
    if (c->marks.probe_cls != KC_PROP || !c->probe_count || !c->probe_work.p) return fail(c, DRP_ESTATE, "drp_probe_begin(\"prop+work\") not running");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<unsigned long long> sh((size_t)PROP_WORK_SHARDS * PROP_WORK_STRIDE);
    CHK(d2h(c, sh.data(), c->probe_work.p, sh.size() * sizeof(unsigned long long)));
    CHK(guarded_wait(c, nullptr));
    unsigned long long w[PROP_WORK_COUNT] = {};
    for (int q = 0; q < PROP_WORK_SHARDS; ++q)
        for (int i = 0; i < PROP_WORK_COUNT; ++i) w[i] += sh[(size_t)q * PROP_WORK_STRIDE + i];
    for (int i = 0; i < PROP_WORK_COUNT; ++i) out[i] = w[i];
    // the matrix instructions those units are made of (k_mlp_split.h: the chain of an edge slot, the node layers of a tile), by the
    // term counts of the engine the counted launches ran on
    if (c->work_lite && c->work_full)
        return fail(c, DRP_ESTATE, "the counted launches ran on both the fused and the lite engine: their units weigh differently; count one engine per drp_probe_begin");
    const bool lite = c->work_lite;
    out[5] = (unsigned long long)prop_mfma_chain(lite) * w[PROP_WORK_CHAIN_SLOTS] + (unsigned long long)prop_mfma_node(lite) * w[PROP_WORK_TILES] +
             (unsigned long long)prop_mfma_node_last(lite) * w[PROP_WORK_TILES_LAST] + (unsigned long long)prop_mfma_enc(lite) * w[PROP_WORK_ENC_TILES];
    // shader-clock cycles and 100 MHz ticks between entry and exit, summed over the workgroups of the counted launches
    out[6] = 0; out[7] = 0;
    for (int q = 0; q < PROP_WORK_SHARDS; ++q) {
        out[6] += sh[(size_t)q * PROP_WORK_STRIDE + PROP_WORK_CLK_CYCLES];
        out[7] += sh[(size_t)q * PROP_WORK_STRIDE + PROP_WORK_CLK_TICKS];
    }
    return DRP_OK;
}

int drp_probe_prop_launches(drp_ctx* c, long* kernels) {
    if (!c || !kernels) return fail(c, DRP_EINVAL, "null argument");
    *kernels = c->marks.probe_cls == KC_PROP ? c->probe_prop_kernels : 0;
    return DRP_OK;
}

int drp_probe_read(drp_ctx* c, double* total_ms, long* launches) {
    if (!c) return DRP_EINVAL;
    CHK(guarded_wait(c, nullptr));
    double tot = 0.0;
    long n = 0;
    for (size_t i = 0; i + 1 < c->probe_used; i += 2) {
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->probe_ev[i].ev, c->probe_ev[i + 1].ev));
        tot += ms;
        ++n;
    }
    c->probe_used = 0;
    if (total_ms) *total_ms = tot;
    if (launches) *launches = n;
    return DRP_OK;
}

// holds the context's stream for `ms` milliseconds (a kernel spinning on the 100 MHz real-time counter): what a
// collective waiting for a dead peer looks like to the host.  tests/test_gpu_errors.py drives the deadline of
// guarded_wait with it.  ms <= 10 000.
__global__ void k_debug_stall(unsigned long long ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

int drp_dispatch_reset(drp_ctx* c) {
    if (!c) return DRP_EINVAL;
    memset(c->marks.dv_hit, 0, sizeof(c->marks.dv_hit));
    return DRP_OK;
}

static long dv_join(const unsigned char* hit, bool default_only, char* out, size_t out_len) {
    std::string all;
    char name[96];
    for (int id = 0; id < DV_COUNT; ++id) {
        bool dflt = true;
        dv_name(id, name, sizeof(name), &dflt);
        if (hit ? !hit[id] : (default_only && !dflt)) continue;
        if (!all.empty()) all += ';';
        all += name;
    }
    if (out && out_len) snprintf(out, out_len, "%s", all.c_str());
    return (long)all.size();
}

long drp_last_dispatch(drp_ctx* c, char* out, size_t out_len) {
    if (!c) return DRP_EINVAL;
    return dv_join(c->marks.dv_hit, false, out, out_len);
}

long drp_dispatch_variants(int default_only, char* out, size_t out_len) { return dv_join(nullptr, default_only != 0, out, out_len); }

int drp_range_info(drp_ctx* c, int* shift, double* bound, double* wmax, int* ok) {
    CHK(need(c, true, false, false));
    const SplitRange& r = c->re_range;
    if (shift) *shift = r.shift;
    if (bound) *bound = split_range_bound(r, r.env_attr, r.env_delta, r.env_dens);
    if (wmax) *wmax = (double)r.wmax;
    if (ok) *ok = c->re_ok ? 1 : 0;
    return DRP_OK;
}

int drp_debug_stall(drp_ctx* c, int ms) {
    if (!c || ms < 0 || ms > 10000) return fail(c, DRP_EINVAL, "stall of %d ms outside 0..10000", ms);
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_debug_stall, dim3(1), dim3(1), 0, c->stream, (unsigned long long)ms * 100000ull);
    HIPCHK(c, hipGetLastError());
    return DRP_OK;
}

// The weight-gradient sums of the last trainer pass that deferred them (WgradQueue::flush_all), read-only: `what` is the
// name behind "train_wgrad_".  "jobs": one record of WGRAD_TAP_FIELDS int64 per job in queue order -- M, in, rows_per_sample,
// dens_mod, blocks, lane_stride, k_stride, the offsets in floats of dW, db and dwd inside the gradient blob (-1: null), whether
// the densities are read -- and one more for the kt_colsum3 call (M, and its target as the db offset; in = 3, the rest 0 / -1).
// No device pointer leaves.  "g:<q>" / "x:<q>": job q's operand rows, dense [M][64] / [M][in] float32 whatever ldg / ldx are;
// "g:<jobs>": the colsum's [M][3].  "dens": the density vector the jobs read.  Valid while c->wgrad_tap_on (capi_ctx.h).
constexpr int WGRAD_TAP_FIELDS = 11;
static long fetch_wgrad_tap(drp_ctx* c, const char* what, const char* name, void* out, size_t out_bytes) {
    const WgradQueue& wq = *c->wgrad;
    if (!c->wgrad_tap_on || wq.tap_jobs.empty() || !wq.tap_G)
        return fail(c, DRP_ESTATE, "buffer '%s' not populated (the last trainer call ran no reverse pass with deferred weight gradients, "
                                   "or a later call has reused its buffers)", name);
    const long n = (long)wq.tap_jobs.size();
    const void* src = nullptr;
    size_t width = 0, pitch = 0, rows = 0;              // bytes of a dense row, bytes between rows on the device, rows
    if (!strcmp(what, "jobs")) {
        const size_t bytes = (size_t)(n + 1) * WGRAD_TAP_FIELDS * sizeof(int64_t);
        if (out_bytes < bytes) return fail(c, DRP_EINVAL, "buffer '%s' needs %zu bytes", name, bytes);
        int64_t* r = static_cast<int64_t*>(out);
        auto off = [&](const float* p) -> int64_t { return p ? (int64_t)(p - wq.tap_G) : -1; };
        for (long q = 0; q < n; ++q, r += WGRAD_TAP_FIELDS) {
            const WgradJob& j = wq.tap_jobs[q];
            r[0] = j.M; r[1] = j.in; r[2] = j.rows_per_sample; r[3] = j.dens_mod; r[4] = j.blocks; r[5] = j.lane_stride; r[6] = j.k_stride;
            r[7] = off(j.dW); r[8] = off(j.db); r[9] = off(j.dwd); r[10] = (j.dwd && j.dens) ? 1 : 0;
        }
        r[0] = wq.tap_cs_M; r[1] = 3; r[2] = 0; r[3] = 0; r[4] = 0; r[5] = 0; r[6] = 0;
        r[7] = -1; r[8] = (int64_t)W_PR1_B; r[9] = -1; r[10] = 0;
        return (long)bytes;
    }
    if (!strcmp(what, "dens")) { src = wq.tap_dens; width = pitch = (size_t)wq.tap_dens_n * 4; rows = 1; }
    else if ((what[0] == 'g' || what[0] == 'x') && what[1] == ':' && what[2] >= '0' && what[2] <= '9') {
        char* end = nullptr;
        const long q = strtol(what + 2, &end, 10);
        if (*end || q < 0 || q > n || (q == n && what[0] == 'x'))
            return fail(c, DRP_EINVAL, "buffer '%s': the last pass queued jobs 0..%ld (and the column sums' rows as g:%ld)", name, n - 1, n);
        if (q == n) { src = wq.tap_cs_g; width = pitch = 3 * 4; rows = (size_t)wq.tap_cs_M; }
        else {
            const WgradJob& j = wq.tap_jobs[q];
            rows = (size_t)j.M;
            if (what[0] == 'g') { src = j.g; width = 64 * 4; pitch = (size_t)j.ldg * 4; }
            else { src = j.x; width = (size_t)j.in * 4; pitch = (size_t)j.ldx * 4; }
        }
    } else return fail(c, DRP_EINVAL, "unknown buffer '%s'", name);
    const size_t bytes = width * rows;
    if (!src || bytes == 0) return fail(c, DRP_ESTATE, "buffer '%s' not populated", name);
    if (out_bytes < bytes) return fail(c, DRP_EINVAL, "buffer '%s' needs %zu bytes", name, bytes);
    HIPCHK(c, hipSetDevice(c->device));
    if (pitch == width) HIPCHK(c, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, c->stream));
    else HIPCHK(c, hipMemcpy2DAsync(out, width, src, pitch, width, rows, hipMemcpyDeviceToHost, c->stream));
    { const int rc = guarded_wait(c, nullptr); if (rc != DRP_OK) return rc; }
    return (long)bytes;
}

long drp_debug_fetch(drp_ctx* c, const char* name, void* out, size_t out_bytes) {
    if (!c || !name || !out) return DRP_EINVAL;
    if (!strncmp(name, "train_wgrad_", 12)) return fetch_wgrad_tap(c, name + 12, name, out, out_bytes);
    const size_t bn = (size_t)c->marks.lastB * c->marks.lastN;
    const DevBuf* b = nullptr;
    bool part = false;              // fetch `view` (a part of a buffer, not owned; view_cap bytes from there on) instead of *b
    const void* view = nullptr;
    size_t view_cap = 0;
    size_t bytes = 0;
    if (!strcmp(name, "s_delta")) { b = &c->ws.s_delta; bytes = bn * 3 * 4; }
    else if (!strcmp(name, "nbr_idx")) { b = &c->ws.nbr_idx; bytes = bn * DRP_K * 2; }
    else if (!strcmp(name, "nbr_cnt")) { b = &c->ws.nbr_cnt; bytes = bn; }
    else if (!strcmp(name, "effect")) { b = &c->ws.eff; bytes = bn * 64 * 4; }
    else if (!strcmp(name, "c_node")) { b = &c->ws.c_node; bytes = bn * 64 * 4; }
    else if (!strcmp(name, "c_edge")) { b = &c->ws.c_edge; bytes = bn * DRP_K * 64 * 4; }
    else if (!strcmp(name, "proj")) { b = &c->ws.proj; bytes = bn * 128 * 4; }
    else if (!strcmp(name, "agg")) { b = &c->ws.agg; bytes = bn * 64 * 4; }
    else if (!strcmp(name, "stats")) { b = &c->stats; bytes = 8 * sizeof(double); }
    // the blob and its packed copies (tests: the device re-pack after an optimiser step against the host packers)
    else if (!strcmp(name, "w_raw")) { b = &c->w_raw; bytes = (size_t)W_TOTAL * 4; }
    else if (!strcmp(name, "w_valu")) { b = &c->w_valu; bytes = (size_t)V_TOTAL * 4; }
    else if (!strcmp(name, "w_mfma")) { b = &c->w_mfma; bytes = (size_t)M_TOTAL * 4; }
    else if (!strcmp(name, "w_mfma_bwd")) { b = &c->w_mfma_bwd; bytes = (size_t)MB_TOTAL * 4; }
    else if (!strcmp(name, "w_split")) { b = &c->w_split; bytes = (size_t)S_ALLOC * 16; }
    else if (!strcmp(name, "w_split6")) { b = &c->w_split6; bytes = (size_t)S6_TOTAL * 16; }
    else if (!strcmp(name, "w_split6_bwd")) { b = &c->w_split6_bwd; bytes = (size_t)SB6_TOTAL * 16; }
    else if (!strcmp(name, "rev_off")) { b = &c->rev_off; bytes = (size_t)c->marks.lastB * (c->marks.lastN + 1) * 4; }
    else if (!strcmp(name, "rev")) { b = &c->rev; bytes = bn * DRP_K * 4; }
    // the last training step's predicted states, sample-major [B][H][N][3], and impulses, step-major [H][B][N][3] (tests: the
    // padded rows of drp_train_step_actions)
    else if (!strcmp(name, "train_states")) { b = &c->states; bytes = (size_t)c->marks.lastH * bn * 3 * 4; }
    else if (!strcmp(name, "train_sdelta")) { b = &c->tape_sdelta; bytes = (size_t)c->marks.lastH * bn * 3 * 4; }
    // d loss / d s_pred as the last trainer call's loss kernel left it, step-major [H][B][N][3]: the loss's own seed after
    // DRP_TRAIN_EVAL, which runs no reverse pass over it (a reverse pass adds every later step's share below the last step's slice)
    else if (!strcmp(name, "train_seed")) { b = &c->g_state; bytes = (size_t)c->marks.lastH * bn * 3 * 4; }
    // the last taped pass's neighbour lists of every step, step-major [H][B][N][10] / [H][B][N] (tests: the reversed lists of a
    // training batch, whose rev_off / rev hold lastH sets [H][B][N+1] / [H][B][N*10]: "train_rev_off", "train_rev")
    else if (!strcmp(name, "train_nbr_idx")) { b = &c->tape_idx; bytes = (size_t)c->marks.lastH * bn * DRP_K * 2; }
    else if (!strcmp(name, "train_nbr_cnt")) { b = &c->tape_cnt; bytes = (size_t)c->marks.lastH * bn; }
    else if (!strcmp(name, "train_rev_off")) { b = &c->rev_off; bytes = (size_t)c->marks.lastH * c->marks.lastB * (c->marks.lastN + 1) * 4; }
    else if (!strcmp(name, "train_rev")) { b = &c->rev; bytes = (size_t)c->marks.lastH * bn * DRP_K * 4; }
    // the resolution regressor's post-activation taps of its last forward (NHWC [B][H][W][C] for the convolutions)
    else if (!strncmp(name, "rgr_c", 5) && name[5] >= '1' && name[5] <= '5' && !name[6]) {
        b = &c->rgr_a[name[5] - '1']; bytes = rgr_conv_out_floats(name[5] - '1', c->rgr_lastB) * 4;
    } else if (!strncmp(name, "rgr_f", 5) && name[5] >= '1' && name[5] <= '4' && !name[6]) {
        b = &c->rgr_f[name[5] - '1']; bytes = (size_t)c->rgr_lastB * RGR_FC_OUT[name[5] - '1'] * 4;
    }
    // the GNN dataset's intermediates of its last batch: foreground counts [B] and sampler picks [B][4097] (int32),
    // recentered points [B][n_max][3] (float64), nearest frame-0 particles [B][n_max] (int32)
    // (c->pd_kind 1); "pdf_*": the same buffers after a drp_ptcl_dataset_frames (c->pd_kind 2), [B * T] images in (b, t) order.
    // The two calls share the buffers: a tap of the call that did not run last is not populated
    else if (!strncmp(name, "pd_", 3) || !strncmp(name, "pdf_", 4)) {
        const bool frames = name[2] == 'f';
        const char* what = name + (frames ? 4 : 3);
        const size_t nb = c->pd_kind == (frames ? 2 : 1) ? (size_t)c->pd_lastB : 0;      // 0: refused below as not populated
        if (!strcmp(what, "nfg")) {
            b = &c->pd_meta; part = true; view = ptr<long long>(c->pd_meta) + nb; view_cap = c->pd_meta.cap; bytes = nb * 4;
        } else if (!strcmp(what, "chosen")) { b = &c->pd_chosen; bytes = nb * (PD_CAP + 1) * 4; }
        else if (!strcmp(what, "recenter")) { b = &c->pd_rec; bytes = nb * c->pd_nmax * 3 * 8; }
        else if (!frames && !strcmp(what, "nearest")) { b = &c->pd_near; bytes = nb * c->pd_nmax * 4; }
        else return fail(c, DRP_EINVAL, "unknown buffer '%s'", name);
    }
    else return fail(c, DRP_EINVAL, "unknown buffer '%s'", name);
    // a GD session keeps every step's impulses and lists in its tape, not in the step workspace: the last step's
    if (c->gd_on && c->gd_H > 0 && bn == (size_t)c->gd_B * c->gd_N) {
        const size_t t = (size_t)c->gd_H - 1;
        if (b == &c->ws.s_delta) { part = true; view = ptr<float>(c->tape_sdelta) + t * bn * 3; view_cap = bytes; }
        else if (b == &c->ws.nbr_idx) { part = true; view = ptr<int16_t>(c->tape_idx) + t * bn * DRP_K; view_cap = bytes; }
        else if (b == &c->ws.nbr_cnt) { part = true; view = ptr<uint8_t>(c->tape_cnt) + t * bn; view_cap = bytes; }
    }
    const void* src = part ? view : b->p;
    const size_t cap = part ? view_cap : b->cap;
    if (!src || bytes == 0 || bytes > cap) return fail(c, DRP_ESTATE, "buffer '%s' not populated", name);
    if (out_bytes < bytes) return fail(c, DRP_EINVAL, "buffer '%s' needs %zu bytes", name, bytes);
    if (hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        return fail(c, DRP_EHIP, "debug fetch failed");
    { const int rc = guarded_wait(c, nullptr); if (rc != DRP_OK) return rc; }
    return (long)bytes;
}
