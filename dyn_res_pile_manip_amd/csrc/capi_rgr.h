// capi_rgr.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip inside extern "C", after
// capi_comm.h and before capi_debug.h).
// Here: the resolution regressor (model/res_regressor.py, the particle count of every MPC step, env/flex_env.py:981-998):
// weight load + repack, the input stack from two masks, the forward pass (kernels: k_rgr.h).

namespace {
// state_dict of MPCResRgrNoPool / MPCResCls: model.{0,2,4,6,8}.{weight,bias} (conv), model.{11,13,15,17,19} (linear)
const int RGR_CONV_CIN[5] = {6, 64, 128, 256, 512};
const int RGR_CONV_COUT[5] = {64, 128, 256, 512, 512};
const int RGR_CONV_IN[5] = {224, 112, 56, 28, 14};
const int RGR_CONV_SPLIT[5] = {1, 2, 4, 8, 32};        // split-K per layer: fixed, whatever the batch (k_rgr.h)
const int RGR_FC_IN[5] = {25088, 4096, 1024, 256, 64};
const int RGR_FC_OUT[4] = {4096, 1024, 256, 64};
const size_t RGR_SLAB_FLOATS = (size_t)RGR_BMAX * 3136 * 128 * 2;   // = every conv's S x M x Cout and FC1's at B = 64

struct RgrOffsets { size_t cw[5], cb[5], fw[5], fb[5], total; };
RgrOffsets rgr_offsets(int n_out) {
    RgrOffsets o;
    size_t p = 0;
    for (int l = 0; l < 5; ++l) {
        o.cw[l] = p; p += (size_t)RGR_CONV_COUT[l] * RGR_CONV_CIN[l] * 16;
        o.cb[l] = p; p += RGR_CONV_COUT[l];
    }
    for (int l = 0; l < 5; ++l) {
        const int out = l < 4 ? RGR_FC_OUT[l] : n_out;
        o.fw[l] = p; p += (size_t)out * RGR_FC_IN[l];
        o.fb[l] = p; p += out;
    }
    o.total = p;
    return o;
}

size_t rgr_conv_out_floats(int l, int B) {
    const int oh = RGR_CONV_IN[l] / 2;
    return (size_t)B * oh * oh * RGR_CONV_COUT[l];
}

// INTER_AREA tables of one axis (downscale ssize -> dsize), computed in double, stored as float: destination d covers
// [d s, (d+1) s), s = ssize / dsize; a source pixel's weight is the part of it the cell covers over the cell width
// min(s, ssize - d s); covers <= 1e-3 are dropped.
void rgr_area_tab(int ssize, int dsize, std::vector<int>& off, std::vector<int>& si, std::vector<float>& a) {
    const double scale = (double)ssize / dsize;
    off.assign(1, 0);
    si.clear();
    a.clear();
    for (int d = 0; d < dsize; ++d) {
        const double f1 = d * scale, f2 = f1 + scale;
        const double cell = std::min(scale, ssize - f1);
        int s2 = std::min((int)std::floor(f2), ssize - 1);
        int s1 = std::min((int)std::ceil(f1), s2);
        if (s1 - f1 > 1e-3) { si.push_back(s1 - 1); a.push_back((float)((s1 - f1) / cell)); }
        for (int sx = s1; sx < s2; ++sx) { si.push_back(sx); a.push_back((float)(1.0 / cell)); }
        if (f2 - s2 > 1e-3) { si.push_back(s2); a.push_back((float)(std::min(std::min(f2 - s2, 1.0), cell) / cell)); }
        off.push_back((int)si.size());
    }
}

int rgr_check_loaded(drp_ctx* c) {
    if (c->rgr_nout == 0) return fail(c, DRP_ESTATE, "resolution regressor: no weights loaded (drp_rgr_load)");
    return DRP_OK;
}

// the forward pass of B samples from c->rgr_x into c->rgr_out (enqueued only); parts: 1 the convolutions, 2 FC1 (its GEMV and
// split-K reduction), 4 FC2..head
int rgr_run_forward(drp_ctx* c, int B, int parts = 7) {
    hipStream_t st = c->stream;
    const RgrOffsets o = rgr_offsets(c->rgr_nout);
    const float* W = ptr<float>(c->rgr_w);
    float* slab = ptr<float>(c->rgr_slab);
    const float* in = ptr<float>(c->rgr_x);
    for (int l = 0; l < 5; ++l) {
        if (!(parts & 1)) { in = ptr<float>(c->rgr_a[4]); break; }
        const int oh = RGR_CONV_IN[l] / 2, cout = RGR_CONV_COUT[l], S = RGR_CONV_SPLIT[l];
        const int M = B * oh * oh;
        const dim3 grid((M + RGR_CT - 1) / RGR_CT, cout / RGR_CT, S);
        float* out = ptr<float>(c->rgr_a[l]);
        const float* w = W + o.cw[l];
        const float* b = W + o.cb[l];
        switch (l) {
        case 0: hipLaunchKernelGGL((k_rgr_conv<6, true>), grid, dim3(256), 0, st, in, B, RGR_CONV_IN[l], w, b, cout, out, slab); break;
        case 1: hipLaunchKernelGGL((k_rgr_conv<64, false>), grid, dim3(256), 0, st, in, B, RGR_CONV_IN[l], w, b, cout, out, slab); break;
        case 2: hipLaunchKernelGGL((k_rgr_conv<128, false>), grid, dim3(256), 0, st, in, B, RGR_CONV_IN[l], w, b, cout, out, slab); break;
        case 3: hipLaunchKernelGGL((k_rgr_conv<256, false>), grid, dim3(256), 0, st, in, B, RGR_CONV_IN[l], w, b, cout, out, slab); break;
        default: hipLaunchKernelGGL((k_rgr_conv<512, false>), grid, dim3(256), 0, st, in, B, RGR_CONV_IN[l], w, b, cout, out, slab); break;
        }
        if (S > 1) {
            const size_t mn = (size_t)M * cout;
            hipLaunchKernelGGL(k_rgr_splitk_reduce, dim3((unsigned)((mn / 4 + 255) / 256)), dim3(256), 0, st, slab, S, mn, cout,
                               b, out);
        }
        in = out;
    }
    const unsigned ng = (unsigned)((B + 15) / 16);
    // FC1: 16 splits of 1568, 256 rows per workgroup (16 x 16 x ng workgroups); FC2: 16 splits of 256; FC3: 4; FC4: none
    if (parts & 2) {
        hipLaunchKernelGGL((k_rgr_fc<25088, 16, 16, 8>), dim3(4096 / 256, 16, ng), dim3(1024), (size_t)16 * (1568 + 4) * 4, st,
                           W + o.fw[0], in, B, 4096, W + o.fb[0], (float*)nullptr, slab);
        hipLaunchKernelGGL(k_rgr_splitk_reduce, dim3((unsigned)(((size_t)B * 4096 / 4 + 255) / 256)), dim3(256), 0, st, slab, 16,
                           (size_t)B * 4096, 4096, W + o.fb[0], ptr<float>(c->rgr_f[0]));
    }
    if (!(parts & 4)) { HIPCHK(c, hipGetLastError()); return DRP_OK; }
    hipLaunchKernelGGL((k_rgr_fc<4096, 16, 4, 8>), dim3(1024 / 64, 16, ng), dim3(256), (size_t)16 * (256 + 4) * 4, st,
                       W + o.fw[1], ptr<float>(c->rgr_f[0]), B, 1024, W + o.fb[1], (float*)nullptr, slab);
    hipLaunchKernelGGL(k_rgr_splitk_reduce, dim3((unsigned)(((size_t)B * 1024 / 4 + 255) / 256)), dim3(256), 0, st, slab, 16,
                       (size_t)B * 1024, 1024, W + o.fb[1], ptr<float>(c->rgr_f[1]));
    hipLaunchKernelGGL((k_rgr_fc<1024, 4, 4, 8>), dim3(256 / 64, 4, ng), dim3(256), (size_t)16 * (256 + 4) * 4, st,
                       W + o.fw[2], ptr<float>(c->rgr_f[1]), B, 256, W + o.fb[2], (float*)nullptr, slab);
    hipLaunchKernelGGL(k_rgr_splitk_reduce, dim3((unsigned)(((size_t)B * 256 / 4 + 255) / 256)), dim3(256), 0, st, slab, 4,
                       (size_t)B * 256, 256, W + o.fb[2], ptr<float>(c->rgr_f[2]));
    hipLaunchKernelGGL((k_rgr_fc<256, 1, 4, 8>), dim3(1, 1, ng), dim3(256), (size_t)16 * (256 + 4) * 4, st,
                       W + o.fw[3], ptr<float>(c->rgr_f[2]), B, 64, W + o.fb[3], ptr<float>(c->rgr_f[3]), (float*)nullptr);
    hipLaunchKernelGGL(k_rgr_head, dim3((unsigned)((B * c->rgr_nout + 63) / 64)), dim3(64), 0, st, W + o.fw[4], W + o.fb[4],
                       ptr<float>(c->rgr_f[3]), B, c->rgr_nout, ptr<float>(c->rgr_out));
    HIPCHK(c, hipGetLastError());
    c->rgr_lastB = B;
    return DRP_OK;
}

// masks (host, [h][w], nonzero = 1) -> the stack in c->rgr_x[0] (enqueued only)
int rgr_run_stack(drp_ctx* c, const uint8_t* init, const uint8_t* goal, int h, int w, int mode) {
    if (!init || !goal) return fail(c, DRP_EINVAL, "null argument");
    if (h < RGR_S || w < RGR_S)
        return fail(c, DRP_EINVAL, "masks of %d x %d: the regressor downscales to %d x %d, smaller masks are not supported", h, w,
                    RGR_S, RGR_S);
    if (mode != DRP_DT_CV5 && mode != DRP_DT_EXACT) return fail(c, DRP_EINVAL, "unknown distance transform mode %d", mode);
    if (mode == DRP_DT_CV5 && (size_t)3 * (w + 4) * sizeof(int) > 60000)
        return fail(c, DRP_EINVAL, "image width %d too large for the chamfer kernel", w);
    if (mode == DRP_DT_EXACT && (size_t)w * sizeof(int) > 60000) return fail(c, DRP_EINVAL, "image width %d too large", w);
    hipStream_t st = c->stream;
    const size_t npix = (size_t)h * w;
    CHK(ensure(c, c->rgr_mask, 2 * npix));
    HIPCHK(c, hipMemcpyAsync(c->rgr_mask.p, init, npix, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(ptr<uint8_t>(c->rgr_mask) + npix, goal, npix, hipMemcpyHostToDevice, st));
    CHK(ensure(c, c->rgr_dtmp, 2 * npix * sizeof(int)));
    CHK(ensure(c, c->rgr_dist, 2 * npix * sizeof(float)));
    const bool fast = h % RGR_S == 0 && w % RGR_S == 0;
    std::vector<int> xo, xs, yo, ys;
    std::vector<float> xa, ya;
    rgr_area_tab(w, RGR_S, xo, xs, xa);
    rgr_area_tab(h, RGR_S, yo, ys, ya);
    const size_t ni = xo.size() + xs.size() + yo.size() + ys.size(), nf = xa.size() + ya.size();
    if (c->rgr_tab_h != h || c->rgr_tab_w != w) {
        std::vector<int>& pack = c->rgr_tab_host;        // kept by the context: the upload reads it until the call's wait
        pack.assign(ni + nf, 0);
        size_t p = 0;
        for (const std::vector<int>* v : {&xo, &xs, &yo, &ys}) { std::copy(v->begin(), v->end(), pack.begin() + p); p += v->size(); }
        for (const std::vector<float>* v : {&xa, &ya}) { memcpy(pack.data() + p, v->data(), v->size() * 4); p += v->size(); }
        c->rgr_tab_h = c->rgr_tab_w = 0;
        CHK(h2d(c, c->rgr_tab, pack.data(), pack.size() * sizeof(int)));
        c->rgr_tab_h = h; c->rgr_tab_w = w;
    }
    RgrTabs t;
    const int* ib = ptr<int>(c->rgr_tab);
    t.xoff = ib; t.xsi = t.xoff + xo.size(); t.yoff = t.xsi + xs.size(); t.ysi = t.yoff + yo.size();
    t.xa = reinterpret_cast<const float*>(t.ysi + ys.size()); t.ya = t.xa + xa.size();
    const uint8_t* m = ptr<uint8_t>(c->rgr_mask);
    if (mode == DRP_DT_CV5) {
        hipLaunchKernelGGL(k_rgr_dt_cv5_pair, dim3(2), dim3(DT_THREADS), (size_t)3 * (w + 4) * sizeof(int), st, m, h, w,
                           ptr<int>(c->rgr_dtmp), ptr<float>(c->rgr_dist));
    } else {
        hipLaunchKernelGGL(k_rgr_edt_cols_pair, dim3((w + 255) / 256, 2), dim3(256), 0, st, m, h, w, ptr<int>(c->rgr_dtmp));
        hipLaunchKernelGGL(k_rgr_edt_rows_pair, dim3(h, 2), dim3(256), (size_t)w * sizeof(int), st, ptr<int>(c->rgr_dtmp), h, w,
                           ptr<float>(c->rgr_dist));
    }
    const int fx = w / RGR_S, fy = h / RGR_S;
    hipLaunchKernelGGL(k_rgr_stack, dim3(RGR_S), dim3(256), 0, st, m, ptr<float>(c->rgr_dist), h, w, t, fast ? 1 : 0, fx, fy,
                       1.0f / (float)(fx * fy), ptr<float>(c->rgr_x));
    HIPCHK(c, hipGetLastError());
    return DRP_OK;
}
}  // namespace

int drp_rgr_load(drp_ctx* c, const float* blob, size_t n_floats, int n_out) {
    if (!c || !blob) return fail(c, DRP_EINVAL, "null argument");
    if (n_out != DRP_RGR_REGRESSOR && n_out != DRP_RGR_CLASSIFIER)
        return fail(c, DRP_EINVAL, "n_out=%d: the regressor head has %d output, the classifier's %d", n_out, DRP_RGR_REGRESSOR,
                    DRP_RGR_CLASSIFIER);
    const RgrOffsets o = rgr_offsets(n_out);
    if (n_floats != o.total)
        return fail(c, DRP_EINVAL, "regressor blob of %zu floats, %zu expected for n_out=%d", n_floats, o.total, n_out);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    c->rgr_nout = 0;
    c->rgr_tr_on = false;               // a fresh model: any training in progress ends with its optimiser (capi_rgr_train.h)
    c->rgr_tr_lastB = 0;
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rgr_fc<25088, 16, 16, 8>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 16 * (1568 + 4) * 4));
    CHK(ensure(c, c->rgr_w, o.total * sizeof(float)));
    CHK(ensure(c, c->rgr_x, (size_t)RGR_BMAX * 6 * RGR_S * RGR_S * sizeof(float)));
    for (int l = 0; l < 5; ++l) CHK(ensure(c, c->rgr_a[l], rgr_conv_out_floats(l, RGR_BMAX) * sizeof(float)));
    for (int l = 0; l < 4; ++l) CHK(ensure(c, c->rgr_f[l], (size_t)RGR_BMAX * RGR_FC_OUT[l] * sizeof(float)));
    CHK(ensure(c, c->rgr_slab, RGR_SLAB_FLOATS * sizeof(float)));
    CHK(ensure(c, c->rgr_out, (size_t)RGR_BMAX * DRP_RGR_CLASSIFIER * sizeof(float)));
    // the blob as given, then the device's layouts at the same offsets
    CHK(h2d(c, c->rgr_raw, blob, o.total * sizeof(float)));
    const float* raw = ptr<float>(c->rgr_raw);
    float* w = ptr<float>(c->rgr_w);
    HIPCHK(c, hipMemcpyAsync(w, raw, o.total * sizeof(float), hipMemcpyDeviceToDevice, st));
    for (int l = 0; l < 5; ++l)
        hipLaunchKernelGGL(k_rgr_repack_conv, dim3(1024), dim3(256), 0, st, raw + o.cw[l], RGR_CONV_COUT[l], RGR_CONV_CIN[l],
                           w + o.cw[l]);
    hipLaunchKernelGGL(k_rgr_repack_fc1, dim3(4096), dim3(256), 0, st, raw + o.fw[0], w + o.fw[0]);
    HIPCHK(c, hipGetLastError());
    CHK(guarded_wait(c, nullptr));
    // the staging copy is not kept (457 MB)
    HIPCHK(c, c->rgr_raw.release());
    c->rgr_nout = n_out;
    c->rgr_lastB = 0;
    return DRP_OK;
}

int drp_rgr_forward(drp_ctx* c, const float* x, int B, float* out) {
    if (!c) return DRP_EINVAL;
    CHK(rgr_check_loaded(c));
    if (B < 1 || B > RGR_BMAX) return fail(c, DRP_EINVAL, "batch %d outside 1..%d", B, RGR_BMAX);
    if (!x || !out) return fail(c, DRP_EINVAL, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->rgr_x.p, x, (size_t)B * 6 * RGR_S * RGR_S * sizeof(float), hipMemcpyHostToDevice, c->stream));
    CHK(rgr_run_forward(c, B));
    CHK(d2h(c, out, c->rgr_out.p, (size_t)B * c->rgr_nout * sizeof(float)));
    return guarded_wait(c, nullptr);
}

int drp_rgr_stack(drp_ctx* c, const uint8_t* init, const uint8_t* goal, int h, int w, int dt_mode, float* x_out) {
    if (!c) return DRP_EINVAL;
    CHK(rgr_check_loaded(c));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(rgr_run_stack(c, init, goal, h, w, dt_mode));
    if (x_out) CHK(d2h(c, x_out, c->rgr_x.p, (size_t)6 * RGR_S * RGR_S * sizeof(float)));
    return guarded_wait(c, nullptr);
}

int drp_rgr_infer(drp_ctx* c, const uint8_t* init, const uint8_t* goal, int h, int w, int dt_mode, float* out) {
    if (!c || !out) return fail(c, DRP_EINVAL, "null argument");
    CHK(rgr_check_loaded(c));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(rgr_run_stack(c, init, goal, h, w, dt_mode));
    CHK(rgr_run_forward(c, 1));
    CHK(d2h(c, out, c->rgr_out.p, (size_t)c->rgr_nout * sizeof(float)));
    return guarded_wait(c, nullptr);
}

int drp_rgr_time(drp_ctx* c, int parts, int B, int iters, float* ms_out) {
    if (!c || !ms_out) return fail(c, DRP_EINVAL, "null argument");
    CHK(rgr_check_loaded(c));
    if (B < 1 || B > RGR_BMAX) return fail(c, DRP_EINVAL, "batch %d outside 1..%d", B, RGR_BMAX);
    if (parts < 1 || parts > 7 || iters < 1 || iters > 10000) return fail(c, DRP_EINVAL, "bad parts=%d iters=%d", parts, iters);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<Event> ev(iters + 1);
    for (Event& e : ev) HIPCHK(c, e.create());
    // a partial forward leaves the taps of the last whole one in place
    struct LastB { drp_ctx* c; int keep; ~LastB() { c->rgr_lastB = keep; } } last_b{c, c->rgr_lastB};
    (void)hipEventRecord(ev[0].ev, c->stream);
    for (int i = 0; i < iters; ++i) {
        CHK(rgr_run_forward(c, B, parts));
        (void)hipEventRecord(ev[i + 1].ev, c->stream);
    }
    if (parts == 7) last_b.keep = B;
    CHK(guarded_wait(c, nullptr));
    for (int i = 0; i < iters; ++i)
        HIPCHK(c, hipEventElapsedTime(&ms_out[i], ev[i].ev, ev[i + 1].ev));
    return DRP_OK;
}
