// capi_rgr_train.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip inside extern "C", after
// capi_rgr.h).
// Here: training the resolution regressor (train/train_res_rgr.py:100-222, loss and update :150-183): the forward with its
// stored activations (rgr_run_forward, unchanged), the loss, the backward pass and Adam (kernels: k_rgr_bwd.h).  Everything
// lives in the forward's device layouts; gradients and weights are put back into torch's layouts only on their way out.

namespace {
const int RGR_WG_SPLIT[5] = {256, 32, 8, 2, 1};     // conv wgrad: split-K of K = B OH OW per layer (fixed)
const int RGR_FCT_SPLIT[4] = {32, 16, 8, 4};        // FC dX: row slices of W per layer (fixed)
const size_t RGR_GF_OFF[5] = {0, 4096, 5120, 5376, 5440};   // per-sample offsets of the FC pre-activation gradients
const int RGR_L1_CAP = 8192;                        // float64 partials of sum |W| (at most 7 313 per step)
const int RGR_BPART_CAP = 65536;                    // column-sum partials (conv1 at B = 64: 784 chunks x 64)

size_t rgr_n_weights(int n_out) {                   // the element count n_W of the L1 term: the 10 weights, no biases
    size_t n = 0;
    for (int l = 0; l < 5; ++l) n += (size_t)RGR_CONV_COUT[l] * RGR_CONV_CIN[l] * 16;
    for (int l = 0; l < 5; ++l) n += (size_t)(l < 4 ? RGR_FC_OUT[l] : n_out) * RGR_FC_IN[l];
    return n;
}

// the device weights (or gradients) at `src`, device layouts -> torch layouts at `dst` (same offsets); enqueued only
void rgr_unpack(drp_ctx* c, const float* src, float* dst, const RgrOffsets& o) {
    hipStream_t st = c->stream;
    (void)hipMemcpyAsync(dst, src, o.total * sizeof(float), hipMemcpyDeviceToDevice, st);
    for (int l = 0; l < 5; ++l)
        hipLaunchKernelGGL(k_rgr_unpack_conv, dim3(1024), dim3(256), 0, st, src + o.cw[l], RGR_CONV_COUT[l], RGR_CONV_CIN[l],
                           dst + o.cw[l]);
    hipLaunchKernelGGL(k_rgr_unpack_fc1, dim3(4096), dim3(256), 0, st, src + o.fw[0], dst + o.fw[0]);
}

void rgr_colsum(drp_ctx* c, const float* dz, int rows, int N, float* g) {
    const int nchunk = (rows + RGR_CS_CHUNK - 1) / RGR_CS_CHUNK;
    float* part = ptr<float>(c->rgr_bpart);
    hipLaunchKernelGGL(k_rgr_colsum_part, dim3(nchunk, (N + 255) / 256), dim3(256), 0, c->stream, dz, rows, N, part);
    hipLaunchKernelGGL(k_rgr_colsum_fin, dim3((N + 255) / 256), dim3(256), 0, c->stream, part, nchunk, N, g);
}

// One training step on what c->rgr_x and c->rgr_tgt hold (enqueued only).  bwd: the backward pass; update: the Adam step;
// full: every gradient to c->rgr_gfull (device layouts, blob offsets), otherwise FC1's is never stored and the others go to
// c->rgr_g (blob offsets with FC1's weight range cut out).  ev (nullable): 4 events around forward | loss + FC backward (with
// FC1's Adam step) | conv backward + the other parameters' Adam step.  *nl1 = the number of |W| partials in c->rgr_l1.
int rgr_enqueue_step(drp_ctx* c, int B, bool bwd, bool update, bool full, Event* ev, int* nl1_out) {
    hipStream_t st = c->stream;
    const int nout = c->rgr_nout;
    const RgrOffsets o = rgr_offsets(nout);
    const size_t nfc1 = (size_t)RGR_FC_OUT[0] * RGR_FC_IN[0];
    float* W = ptr<float>(c->rgr_w);
    float* M = ptr<float>(c->rgr_m);
    float* V = ptr<float>(c->rgr_v);
    float* G = full ? ptr<float>(c->rgr_gfull) : ptr<float>(c->rgr_g);
    auto gp = [&](size_t off) { return G + ((full || off < o.fw[0]) ? off : off - nfc1); };
    float* slab = ptr<float>(c->rgr_slab);
    double* l1 = ptr<double>(c->rgr_l1);
    int nl1 = 0;
    const float coef = (float)(c->rgr_tr_lam / (double)rgr_n_weights(nout));
    const long iter = c->rgr_tr_iter + 1;
    const float step_size = (float)(c->rgr_tr_lr / (1.0 - pow(c->rgr_tr_beta1, (double)iter)));
    const float bc2_sqrt = (float)sqrt(1.0 - pow(0.999, (double)iter));
    const float b1 = (float)c->rgr_tr_beta1;

    if (ev) (void)hipEventRecord(ev[0].ev, st);
    CHK(rgr_run_forward(c, B));
    if (ev) (void)hipEventRecord(ev[1].ev, st);

    // sum |W| of every weight (biases excluded) before any update; FC1..FC4's come from their wgrad pass when there is one
    auto l1_of = [&](size_t off, size_t n, int blocks) {
        hipLaunchKernelGGL(k_rgr_l1, dim3(blocks), dim3(256), 0, st, W + off, n, l1 + nl1);
        nl1 += blocks;
    };
    for (int l = 0; l < 5; ++l) l1_of(o.cw[l], (size_t)RGR_CONV_COUT[l] * RGR_CONV_CIN[l] * 16, 128);
    l1_of(o.fw[4], (size_t)nout * 64, 128);
    if (!bwd)
        for (int j = 0; j < 4; ++j) l1_of(o.fw[j], (size_t)RGR_FC_OUT[j] * RGR_FC_IN[j], j == 0 ? 1024 : 128);

    const float* tgt = ptr<float>(c->rgr_tgt);
    float* gf = ptr<float>(c->rgr_gf);
    float* dzf[4];
    for (int j = 0; j < 4; ++j) dzf[j] = gf + (size_t)RGR_BMAX * RGR_GF_OFF[j];
    hipLaunchKernelGGL(k_rgr_loss_head, dim3(1), dim3(256), 0, st, ptr<float>(c->rgr_out), B, nout, tgt, tgt + RGR_BMAX,
                       reinterpret_cast<const int*>(tgt + 2 * RGR_BMAX), W + o.fw[4], ptr<float>(c->rgr_f[3]),
                       ptr<double>(c->rgr_lossp), bwd ? 1 : 0, coef, gp(o.fw[4]), gp(o.fb[4]), dzf[3]);
    if (bwd) {
        const unsigned ng = (unsigned)((B + 15) / 16);
        float* dz5 = ptr<float>(c->rgr_dz[0]);
        for (int j = 3; j >= 0; --j) {
            const int N = RGR_FC_OUT[j], K = RGR_FC_IN[j], S = RGR_FCT_SPLIT[j], R = N / S;
            const float* X = j ? ptr<float>(c->rgr_f[j - 1]) : ptr<float>(c->rgr_a[4]);
            rgr_colsum(c, dzf[j], B, N, gp(o.fb[j]));
            // dX through the pre-update weights, then the layer's weight gradient (FC1: fused with its Adam step)
            hipLaunchKernelGGL(k_rgr_fct, dim3((K + 1023) / 1024, S, ng), dim3(256), (size_t)R * 16 * sizeof(float), st,
                               W + o.fw[j], dzf[j], B, N, K, R, slab);
            const size_t n = (size_t)B * K;
            hipLaunchKernelGGL(k_rgr_dreduce, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, slab, S, n, X,
                               j ? dzf[j - 1] : dz5);
            const dim3 grid(K / 256, N / 64);
            if (j == 0 && update)
                hipLaunchKernelGGL(k_rgr_fc_wgrad<true>, grid, dim3(256), 0, st, W + o.fw[0], X, dzf[0], B, N, K, coef,
                                   (float*)nullptr, M + o.fw[0], V + o.fw[0], step_size, bc2_sqrt, b1, l1 + nl1);
            else
                hipLaunchKernelGGL(k_rgr_fc_wgrad<false>, grid, dim3(256), 0, st, W + o.fw[j], X, dzf[j], B, N, K, coef,
                                   (j > 0 || full) ? gp(o.fw[j]) : (float*)nullptr, (float*)nullptr, (float*)nullptr, 0.0f,
                                   1.0f, b1, l1 + nl1);
            nl1 += (int)(grid.x * grid.y);
        }
        if (ev) (void)hipEventRecord(ev[2].ev, st);
        for (int l = 4; l >= 0; --l) {
            const int IH = RGR_CONV_IN[l], OH = IH / 2, cout = RGR_CONV_COUT[l], cin = RGR_CONV_CIN[l], S = RGR_WG_SPLIT[l];
            const float* dz = ptr<float>(c->rgr_dz[l & 1]);
            const float* X = l ? ptr<float>(c->rgr_a[l - 1]) : ptr<float>(c->rgr_x);
            rgr_colsum(c, dz, B * OH * OH, cout, gp(o.cb[l]));
            const dim3 wg(cout / RGR_CT, (16 * cin + RGR_CT - 1) / RGR_CT, S);
            switch (l) {
            case 0: hipLaunchKernelGGL((k_rgr_conv_wgrad<6, true>), wg, dim3(256), 0, st, dz, X, B, IH, cout, slab); break;
            case 1: hipLaunchKernelGGL((k_rgr_conv_wgrad<64, false>), wg, dim3(256), 0, st, dz, X, B, IH, cout, slab); break;
            case 2: hipLaunchKernelGGL((k_rgr_conv_wgrad<128, false>), wg, dim3(256), 0, st, dz, X, B, IH, cout, slab); break;
            case 3: hipLaunchKernelGGL((k_rgr_conv_wgrad<256, false>), wg, dim3(256), 0, st, dz, X, B, IH, cout, slab); break;
            default: hipLaunchKernelGGL((k_rgr_conv_wgrad<512, false>), wg, dim3(256), 0, st, dz, X, B, IH, cout, slab); break;
            }
            const size_t nw = (size_t)cout * 16 * cin;
            hipLaunchKernelGGL(k_rgr_wreduce, dim3((unsigned)((nw / 4 + 255) / 256)), dim3(256), 0, st, slab, S, nw, W + o.cw[l],
                               coef, gp(o.cw[l]));
            if (l == 0) break;                          // the input needs no gradient
            const dim3 dg((B * OH * OH + RGR_CT - 1) / RGR_CT, cin / RGR_CT, 4);
            float* out = ptr<float>(c->rgr_dz[(l - 1) & 1]);
            const float* act = ptr<float>(c->rgr_a[l - 1]);
            const float* wt = W + o.cw[l];
            switch (l) {
            case 1: hipLaunchKernelGGL((k_rgr_conv_dgrad<64, 128>), dg, dim3(256), 0, st, dz, wt, act, B, IH, out); break;
            case 2: hipLaunchKernelGGL((k_rgr_conv_dgrad<128, 256>), dg, dim3(256), 0, st, dz, wt, act, B, IH, out); break;
            case 3: hipLaunchKernelGGL((k_rgr_conv_dgrad<256, 512>), dg, dim3(256), 0, st, dz, wt, act, B, IH, out); break;
            default: hipLaunchKernelGGL((k_rgr_conv_dgrad<512, 512>), dg, dim3(256), 0, st, dz, wt, act, B, IH, out); break;
            }
        }
        if (update) {                                   // every parameter but FC1's weight: one elementwise pass each side
            const float inf = __builtin_inff();
            const float4 lo = make_float4(-inf, -inf, -inf, -inf), hi = make_float4(inf, inf, inf, inf);
            const size_t n0 = o.fw[0], n1 = o.total - o.fb[0];
            hipLaunchKernelGGL(k_adam, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st, W, gp(0), M, V, (int)n0, step_size,
                               bc2_sqrt, lo, hi, b1, (float*)nullptr, (const unsigned*)nullptr, (unsigned*)nullptr);
            hipLaunchKernelGGL(k_adam, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, W + o.fb[0], gp(o.fb[0]), M + o.fb[0],
                               V + o.fb[0], (int)n1, step_size, bc2_sqrt, lo, hi, b1, (float*)nullptr, (const unsigned*)nullptr,
                               (unsigned*)nullptr);
        }
    } else if (ev) {
        (void)hipEventRecord(ev[2].ev, st);
    }
    if (ev) (void)hipEventRecord(ev[3].ev, st);
    HIPCHK(c, hipGetLastError());
    *nl1_out = nl1;
    return DRP_OK;
}

int rgr_check_training(drp_ctx* c) {
    CHK(rgr_check_loaded(c));
    if (!c->rgr_tr_on) return fail(c, DRP_ESTATE, "resolution regressor: drp_rgr_train_begin not called since drp_rgr_load");
    return DRP_OK;
}
}  // namespace

int drp_rgr_train_begin(drp_ctx* c, double lr, double beta1, double lam_reg) {
    if (!c) return DRP_EINVAL;
    CHK(rgr_check_loaded(c));
    if (!(lr > 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(lam_reg >= 0.0))
        return fail(c, DRP_EINVAL, "bad lr %g / beta1 %g / lam_reg %g", lr, beta1, lam_reg);
    HIPCHK(c, hipSetDevice(c->device));
    const RgrOffsets o = rgr_offsets(c->rgr_nout);
    const size_t nfc1 = (size_t)RGR_FC_OUT[0] * RGR_FC_IN[0];
    c->rgr_tr_on = false;
    CHK(ensure(c, c->rgr_m, o.total * sizeof(float)));
    CHK(ensure(c, c->rgr_v, o.total * sizeof(float)));
    CHK(ensure(c, c->rgr_g, (o.total - nfc1) * sizeof(float)));
    CHK(ensure(c, c->rgr_dz[0], rgr_conv_out_floats(0, RGR_BMAX) * sizeof(float)));
    CHK(ensure(c, c->rgr_dz[1], rgr_conv_out_floats(1, RGR_BMAX) * sizeof(float)));
    CHK(ensure(c, c->rgr_gf, (size_t)RGR_BMAX * RGR_GF_OFF[4] * sizeof(float)));
    CHK(ensure(c, c->rgr_bpart, (size_t)RGR_BPART_CAP * sizeof(float)));
    CHK(ensure(c, c->rgr_l1, (size_t)RGR_L1_CAP * sizeof(double)));
    CHK(ensure(c, c->rgr_lossp, (size_t)RGR_BMAX * sizeof(double)));
    CHK(ensure(c, c->rgr_tgt, (size_t)3 * RGR_BMAX * sizeof(float)));
    HIPCHK(c, hipMemsetAsync(c->rgr_m.p, 0, o.total * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(c->rgr_v.p, 0, o.total * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(c->rgr_tgt.p, 0, (size_t)3 * RGR_BMAX * sizeof(float), c->stream));
    CHK(guarded_wait(c, nullptr));
    c->rgr_tr_lr = lr;
    c->rgr_tr_beta1 = beta1;
    c->rgr_tr_lam = lam_reg;
    c->rgr_tr_iter = 0;
    c->rgr_tr_lastB = 0;
    c->rgr_tr_on = true;
    return DRP_OK;
}

int drp_rgr_train_step(drp_ctx* c, const float* x, const float* y, const float* conf, const int32_t* label, int B, int mode,
                       double* loss_out, float* grad_out) {
    if (!c) return DRP_EINVAL;
    CHK(rgr_check_training(c));
    if (B < 1 || B > RGR_BMAX) return fail(c, DRP_EINVAL, "batch %d outside 1..%d", B, RGR_BMAX);
    if (mode != DRP_TRAIN_EVAL && mode != DRP_TRAIN_GRAD && mode != DRP_TRAIN_UPDATE)
        return fail(c, DRP_EINVAL, "unknown mode %d", mode);
    if (!x) return fail(c, DRP_EINVAL, "null argument");
    if (grad_out && mode != DRP_TRAIN_GRAD) return fail(c, DRP_EINVAL, "grad_out is written in DRP_TRAIN_GRAD mode only");
    const int nout = c->rgr_nout;
    if (nout == DRP_RGR_REGRESSOR) {
        if (!y || !conf) return fail(c, DRP_EINVAL, "the regressor needs y and conf");
        if (label) return fail(c, DRP_EINVAL, "the regressor takes no label");
    } else {
        if (!label) return fail(c, DRP_EINVAL, "the classifier needs label");
        if (y || conf) return fail(c, DRP_EINVAL, "the classifier takes no y / conf");
        for (int b = 0; b < B; ++b)
            if (label[b] < 0 || label[b] >= DRP_RGR_CLASSIFIER)
                return fail(c, DRP_EINVAL, "label[%d] = %d outside 0..%d", b, (int)label[b], DRP_RGR_CLASSIFIER - 1);
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const RgrOffsets o = rgr_offsets(nout);
    const bool bwd = mode != DRP_TRAIN_EVAL, full = grad_out != nullptr;
    if (full) {
        CHK(ensure(c, c->rgr_gfull, o.total * sizeof(float)));
        CHK(ensure(c, c->rgr_raw, o.total * sizeof(float)));
    }
    HIPCHK(c, hipMemcpyAsync(c->rgr_x.p, x, (size_t)B * 6 * RGR_S * RGR_S * sizeof(float), hipMemcpyHostToDevice, st));
    float* tgt = ptr<float>(c->rgr_tgt);
    if (nout == DRP_RGR_REGRESSOR) {
        HIPCHK(c, hipMemcpyAsync(tgt, y, (size_t)B * sizeof(float), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(tgt + RGR_BMAX, conf, (size_t)B * sizeof(float), hipMemcpyHostToDevice, st));
    } else {
        HIPCHK(c, hipMemcpyAsync(tgt + 2 * RGR_BMAX, label, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    int nl1 = 0;
    CHK(rgr_enqueue_step(c, B, bwd, mode == DRP_TRAIN_UPDATE, full, nullptr, &nl1));
    if (mode == DRP_TRAIN_UPDATE) c->rgr_tr_iter += 1;
    c->rgr_tr_lastB = B;
    std::vector<double> lp((size_t)B), l1((size_t)nl1);
    CHK(d2h(c, lp.data(), c->rgr_lossp.p, lp.size() * sizeof(double)));
    CHK(d2h(c, l1.data(), c->rgr_l1.p, l1.size() * sizeof(double)));
    if (full) {
        rgr_unpack(c, ptr<float>(c->rgr_gfull), ptr<float>(c->rgr_raw), o);
        HIPCHK(c, hipGetLastError());
        CHK(d2h(c, grad_out, c->rgr_raw.p, o.total * sizeof(float)));
    }
    CHK(guarded_wait(c, nullptr));
    if (loss_out) {
        double main = 0.0, reg = 0.0;                   // fixed orders: sample-ascending, partial-ascending
        for (int b = 0; b < B; ++b) main += lp[b];
        main /= (double)B;
        for (int i = 0; i < nl1; ++i) reg += l1[i];
        reg /= (double)rgr_n_weights(nout);
        loss_out[0] = main + c->rgr_tr_lam * reg;
        loss_out[1] = main;
        loss_out[2] = reg;
    }
    return DRP_OK;
}

int drp_rgr_train_set_lr(drp_ctx* c, double lr) {
    if (!c) return DRP_EINVAL;
    CHK(rgr_check_training(c));
    if (!(lr > 0.0)) return fail(c, DRP_EINVAL, "bad lr %g", lr);
    c->rgr_tr_lr = lr;
    return DRP_OK;
}

int drp_rgr_get_weights(drp_ctx* c, float* blob_out, size_t n_floats) {
    if (!c) return DRP_EINVAL;
    CHK(rgr_check_loaded(c));
    const RgrOffsets o = rgr_offsets(c->rgr_nout);
    if (!blob_out || n_floats != o.total) return fail(c, DRP_EINVAL, "blob_out must hold %zu floats", o.total);
    HIPCHK(c, hipSetDevice(c->device));
    const bool keep = c->rgr_gfull.p != nullptr;        // GRAD with grad_out keeps its staging buffer; otherwise it goes again
    CHK(ensure(c, c->rgr_raw, o.total * sizeof(float)));
    rgr_unpack(c, ptr<float>(c->rgr_w), ptr<float>(c->rgr_raw), o);
    HIPCHK(c, hipGetLastError());
    CHK(d2h(c, blob_out, c->rgr_raw.p, o.total * sizeof(float)));
    CHK(guarded_wait(c, nullptr));
    if (!keep) {
        HIPCHK(c, c->rgr_raw.release());
    }
    return DRP_OK;
}

int drp_rgr_train_time(drp_ctx* c, int B, int iters, float* ms_out) {
    if (!c || !ms_out) return fail(c, DRP_EINVAL, "null argument");
    CHK(rgr_check_training(c));
    if (B < 1 || B != c->rgr_tr_lastB)
        return fail(c, DRP_ESTATE, "batch %d: time the batch of the last drp_rgr_train_step (%d), whose inputs are staged", B,
                    c->rgr_tr_lastB);
    if (iters < 1 || iters > 1000) return fail(c, DRP_EINVAL, "bad iters=%d", iters);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<Event> ev((size_t)4 * iters);
    for (Event& e : ev) HIPCHK(c, e.create());
    for (int i = 0; i < iters; ++i) {
        int nl1 = 0;
        CHK(rgr_enqueue_step(c, B, true, true, false, &ev[(size_t)4 * i], &nl1));
        c->rgr_tr_iter += 1;
    }
    CHK(guarded_wait(c, nullptr));
    for (int i = 0; i < iters; ++i)
        for (int p = 0; p < 3; ++p)
            HIPCHK(c, hipEventElapsedTime(&ms_out[(size_t)3 * i + p], ev[(size_t)4 * i + p].ev, ev[(size_t)4 * i + p + 1].ev));
    return DRP_OK;
}
