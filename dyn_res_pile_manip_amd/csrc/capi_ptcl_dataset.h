// capi_ptcl_dataset.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip inside extern "C", after
// capi_rgr_train.h).
// Here: GNN training batches from recorded episodes (row x4, dataset/dataset_gnn_dyn.py:86-201; kernels: k_ptcl_dataset.h).
// drp_ptcl_dataset_frames (row x4 / u1) runs the same chain on every frame of a window and shares these workspaces; c->pd_kind
// says whose bytes they hold, so a debug tap never hands back the other call's.
// The call owns its workspaces (c->pd_*): the PropNet weights, a training / planning session, the regressor and the
// particle-extraction buffers of drp_obs2ptcl are never touched.

namespace {
const int PD_BMAX = 1024;
const int PD_NEV = 7;           // events: start | upload | compaction | fps_rad | recenter | track + pack | download

size_t pd_align(size_t x) { return (x + 255) & ~(size_t)255; }

struct PdLayout {               // the upload arena (pinned staging and its device copy)
    size_t depth, ptcl, radius, push, init, nptcl, ptcl_off, bytes;
};

PdLayout pd_layout(int B, size_t npix, size_t ptcl_floats, int T) {
    PdLayout L;
    size_t o = 0;
    L.depth = o; o = pd_align(o + (size_t)B * npix * sizeof(uint16_t));
    L.ptcl = o; o = pd_align(o + ptcl_floats * sizeof(float));
    L.radius = o; o = pd_align(o + (size_t)B * sizeof(double));
    L.push = o; o = pd_align(o + (size_t)B * (T - 1) * PD_PUSH * sizeof(double));
    L.init = o; o = pd_align(o + (size_t)B * sizeof(int));
    L.nptcl = o; o = pd_align(o + (size_t)B * sizeof(int));
    L.ptcl_off = o; o = pd_align(o + (size_t)B * sizeof(long long));
    L.bytes = o;
    return L;
}

int pd_pin_ensure(drp_ctx* c, size_t bytes) {
    // nothing of an earlier call may still copy from / to the block that goes
    if (c->pd_pin.p && c->pd_pin.cap < bytes) (void)hipStreamSynchronize(c->stream);
    return ensure_pinned(c, c->pd_pin, bytes);
}

int pd_name(const int32_t* episode, int b) { return episode ? episode[b] : b; }
}  // namespace

int drp_ptcl_dataset_batch(drp_ctx* c, int B, const uint16_t* depth, int h, int w, double global_scale, const double cam[4],
                           const double T_cam[16], int T, const int32_t* n_ptcl, const float* particles, const double* radius,
                           const int32_t* init_idx, const int32_t* n_fg_host, const double* push, const int32_t* episode,
                           int n_cap, float* states_out, float* sdelta_out, int32_t* counts_out, int* n_max_out) {
    if (!c || !depth || !cam || !T_cam || !n_ptcl || !particles || !radius || !init_idx || !n_fg_host || !push || !states_out ||
        !sdelta_out || !counts_out || !n_max_out)
        return fail(c, DRP_EINVAL, "null argument");
    if (B < 1 || B > PD_BMAX) return fail(c, DRP_EINVAL, "batch %d outside 1..%d", B, PD_BMAX);
    if (h <= 0 || w <= 0 || (size_t)h * w > (1u << 26)) return fail(c, DRP_EINVAL, "bad image size %d x %d", h, w);
    if (T < 2) return fail(c, DRP_EINVAL, "a sample needs at least 2 frames (n_his + n_rollout), got %d", T);
    if (!(global_scale > 0.0)) return fail(c, DRP_EINVAL, "bad global_scale %g", global_scale);
    if (n_cap < 1) return fail(c, DRP_EINVAL, "bad output capacity %d", n_cap);
    size_t ptcl_floats = 0, fg_total = 0;
    std::vector<long long> ptcl_off(B);
    for (int b = 0; b < B; ++b) {
        if (n_ptcl[b] <= 0) return fail(c, DRP_EINVAL, "episode %d: %d particles in its files", pd_name(episode, b), n_ptcl[b]);
        if (init_idx[b] < 0) return fail(c, DRP_EINVAL, "episode %d: sampler start %d", pd_name(episode, b), init_idx[b]);
        if (!(radius[b] > 0.0) || !std::isfinite(radius[b]))
            return fail(c, DRP_EINVAL, "episode %d: bad fps radius %g", pd_name(episode, b), radius[b]);
        for (int t = 0; t + 1 < T; ++t) {
            const double* pu = push + ((size_t)b * (T - 1) + t) * PD_PUSH;
            // dataset_gnn_dyn.py:148-153: a zero-length push divides by zero, a push off the table plane exits
            if (!(pu[9] > 0.0) || !std::isfinite(pu[9]))
                return fail(c, DRP_EINVAL, "episode %d: push %d has length %g", pd_name(episode, b), t, pu[9]);
            if (!(std::fabs(pu[8]) < 1e-6))
                return fail(c, DRP_EINVAL, "episode %d: push %d leaves the table plane (|push_dir_cam z| = %g >= 1e-6)",
                            pd_name(episode, b), t, std::fabs(pu[8]));
        }
        if (n_fg_host[b] < 0 || (size_t)n_fg_host[b] > (size_t)h * w)
            return fail(c, DRP_EINVAL, "episode %d: host foreground count %d", pd_name(episode, b), n_fg_host[b]);
        fg_total += (size_t)n_fg_host[b];
        ptcl_off[b] = (long long)ptcl_floats;
        ptcl_floats += (size_t)T * n_ptcl[b] * 4;
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (c->pd_pin.p) CHK(guarded_wait(c, nullptr));     // a call that failed before its wait may still copy from the staging
    for (int e = 0; e < PD_NEV; ++e)
        HIPCHK(c, c->pd_ev[e].create());
    c->pd_timed = false;
    c->pd_kind = 0;                 // the shared buffers are rewritten from here on: no tap until this call has its counts
    const size_t npix = (size_t)h * w;
    const PdLayout L = pd_layout(B, npix, ptcl_floats, T);
    const size_t meta_bytes = (size_t)2 * B * sizeof(int);
    CHK(pd_pin_ensure(c, std::max(L.bytes, meta_bytes)));
    char* pin = ptr<char>(c->pd_pin);
    memcpy(pin + L.depth, depth, (size_t)B * npix * sizeof(uint16_t));
    memcpy(pin + L.ptcl, particles, ptcl_floats * sizeof(float));
    memcpy(pin + L.radius, radius, (size_t)B * sizeof(double));
    memcpy(pin + L.push, push, (size_t)B * (T - 1) * PD_PUSH * sizeof(double));
    memcpy(pin + L.init, init_idx, (size_t)B * sizeof(int));
    memcpy(pin + L.nptcl, n_ptcl, (size_t)B * sizeof(int));
    memcpy(pin + L.ptcl_off, ptcl_off.data(), (size_t)B * sizeof(long long));
    HIPCHK(c, hipEventRecord(c->pd_ev[0].ev, st));
    CHK(h2d(c, c->pd_in, pin, L.bytes));
    HIPCHK(c, hipEventRecord(c->pd_ev[1].ev, st));
    const char* in = static_cast<const char*>(c->pd_in.p);
    const uint16_t* d_depth = reinterpret_cast<const uint16_t*>(in + L.depth);
    const float* d_ptcl = reinterpret_cast<const float*>(in + L.ptcl);
    const double* d_radius = reinterpret_cast<const double*>(in + L.radius);
    const double* d_push = reinterpret_cast<const double*>(in + L.push);
    const int* d_init = reinterpret_cast<const int*>(in + L.init);
    const int* d_nptcl = reinterpret_cast<const int*>(in + L.nptcl);
    const long long* d_poff = reinterpret_cast<const long long*>(in + L.ptcl_off);
    PdCam pc;
    for (int i = 0; i < 16; ++i) pc.M[i] = T_cam[i];
    pc.gs = global_scale;
    pc.fx = cam[0]; pc.fy = cam[1]; pc.cx = cam[2]; pc.cy = cam[3];

    // 1. depth -> clouds: tile counts, one scan over all images' tiles, compaction
    const int nblk = px_nblk(npix);
    const size_t ntile = (size_t)B * nblk;
    CHK(ensure(c, c->pd_blk, (2 * ntile + 2) * sizeof(unsigned long long)));
    unsigned long long* cnt = ptr<unsigned long long>(c->pd_blk);
    unsigned long long* off = cnt + ntile;
    CHK(ensure(c, c->pd_meta, (size_t)B * (2 * sizeof(int) + sizeof(long long))));
    long long* d_pcd_off = ptr<long long>(c->pd_meta);
    int* d_nfg = reinterpret_cast<int*>(d_pcd_off + B);
    int* d_counts = d_nfg + B;
    // sized by the host's counts; the kernels write and read nothing beyond them if the device disagrees (an error below)
    const long long pcd_cap = (long long)std::max(fg_total, (size_t)1);
    CHK(ensure(c, c->pd_pcd, (size_t)pcd_cap * 3 * sizeof(double)));
    CHK(ensure(c, c->pd_dist, (size_t)pcd_cap * sizeof(double)));
    hipLaunchKernelGGL(k_pd_count, dim3(nblk, B), dim3(PX_BLOCK), 0, st, d_depth, npix, global_scale * 1000.0, cnt);
    hipLaunchKernelGGL(k_px_scan_u64, dim3(1), dim3(1024), 0, st, cnt, (int)ntile, off);
    hipLaunchKernelGGL(k_pd_compact, dim3(nblk, B), dim3(PX_BLOCK), 0, st, d_depth, npix, w, pc, off, pcd_cap, ptr<double>(c->pd_pcd));
    hipLaunchKernelGGL(k_pd_meta, dim3((B + 255) / 256), dim3(256), 0, st, off, nblk, B, d_nfg, d_pcd_off);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->pd_ev[2].ev, st));

    // 2. fps_rad, one workgroup per sample
    const int cap = PD_CAP + 1;
    CHK(ensure(c, c->pd_chosen, (size_t)B * cap * sizeof(int)));
    hipLaunchKernelGGL(k_pd_fps_rad, dim3(B), dim3(1024), 0, st, ptr<double>(c->pd_pcd), pcd_cap, d_pcd_off, d_nfg, d_init,
                       d_radius, cap, ptr<double>(c->pd_dist), ptr<int>(c->pd_chosen), d_counts);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->pd_ev[3].ev, st));
    // the one wait before the download: foreground and particle counts size the rest
    CHK(d2h(c, pin, d_nfg, meta_bytes));
    CHK(guarded_wait(c, nullptr));
    const int* nfg = reinterpret_cast<const int*>(pin);
    const int* counts = nfg + B;
    c->pd_lastB = B;
    c->pd_nmax = 0;
    c->pd_kind = 1;
    for (int b = 0; b < B; ++b) {
        if (nfg[b] == 0) return fail(c, DRP_EINVAL, "episode %d: the depth image has no foreground pixel", pd_name(episode, b));
        if (n_fg_host && n_fg_host[b] != nfg[b])
            return fail(c, DRP_EINVAL, "episode %d: %d foreground pixels on the host, %d on the device", pd_name(episode, b),
                        n_fg_host[b], nfg[b]);
        if (init_idx[b] >= nfg[b])
            return fail(c, DRP_EINVAL, "episode %d: sampler start %d outside the cloud of %d points", pd_name(episode, b),
                        init_idx[b], nfg[b]);
        if (counts[b] > PD_CAP)
            return fail(c, DRP_EINVAL, "episode %d: fps_rad reached the cap of %d particles (radius %g)", pd_name(episode, b),
                        PD_CAP, radius[b]);
    }
    int n_max = 0;
    for (int b = 0; b < B; ++b) { counts_out[b] = counts[b]; n_max = std::max(n_max, counts[b]); }
    if (n_max > n_cap) return fail(c, DRP_EINVAL, "the batch needs %d particle slots, the outputs hold %d", n_max, n_cap);
    *n_max_out = n_max;
    c->pd_nmax = n_max;

    // 3. recenter (float64)
    CHK(ensure(c, c->pd_rec, (size_t)B * n_max * 3 * sizeof(double)));
    hipLaunchKernelGGL(k_pd_recenter, dim3((B * n_max + 3) / 4), dim3(256), 0, st, ptr<double>(c->pd_pcd), d_pcd_off, d_nfg,
                       ptr<int>(c->pd_chosen), cap, d_counts, d_radius, n_max, B, ptr<double>(c->pd_rec));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->pd_ev[4].ev, st));

    // 4. track and pack
    const size_t n_states = (size_t)B * T * n_max * 3, n_sdelta = (size_t)B * (T - 1) * n_max * 3;
    CHK(ensure(c, c->pd_near, (size_t)B * n_max * sizeof(int)));
    CHK(ensure(c, c->pd_out, (n_states + n_sdelta) * sizeof(float)));
    const unsigned jb = (unsigned)((n_max + 255) / 256);
    hipLaunchKernelGGL(k_pd_nearest, dim3(jb, B), dim3(256), 0, st, ptr<double>(c->pd_rec), d_counts, n_max, d_ptcl, d_poff,
                       d_nptcl, pc, ptr<int>(c->pd_near));
    hipLaunchKernelGGL(k_pd_pack, dim3(jb, T, B), dim3(256), 0, st, ptr<int>(c->pd_near), d_counts, n_max, T, d_ptcl, d_poff,
                       d_nptcl, d_push, pc, ptr<float>(c->pd_out), ptr<float>(c->pd_out) + n_states);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->pd_ev[5].ev, st));

    // 5. one download through the pinned staging
    CHK(pd_pin_ensure(c, (n_states + n_sdelta) * sizeof(float)));
    CHK(d2h(c, c->pd_pin.p, c->pd_out.p, (n_states + n_sdelta) * sizeof(float)));
    HIPCHK(c, hipEventRecord(c->pd_ev[6].ev, st));
    CHK(guarded_wait(c, nullptr));
    const float* res = ptr<const float>(c->pd_pin);
    memcpy(states_out, res, n_states * sizeof(float));
    memcpy(sdelta_out, res + n_states, n_sdelta * sizeof(float));
    c->pd_timed = true;
    return DRP_OK;
}

// Untracked samples straight from the depth frames: depth2fgpcd -> fps_rad -> recenter on every frame of B windows of T frames
// (dataset_gnn_dyn.py:97-101 per frame), the B * T images in (b, t) order through the kernels of drp_ptcl_dataset_batch.
int drp_ptcl_dataset_frames(drp_ctx* c, int B, int T, const uint16_t* depth, int h, int w, double global_scale, const double cam[4],
                            const double* radius, const int32_t* init_idx, const int32_t* n_fg_host, const int32_t* episode,
                            int n_cap, float* clouds_out, int32_t* counts_out, int* n_max_out) {
    if (!c || !depth || !cam || !radius || !init_idx || !n_fg_host || !clouds_out || !counts_out || !n_max_out)
        return fail(c, DRP_EINVAL, "null argument");
    if (B < 1 || T < 1 || (long long)B * T > PD_BMAX)
        return fail(c, DRP_EINVAL, "%d samples x %d frames: a call takes 1..%d images", B, T, PD_BMAX);
    if (h <= 0 || w <= 0 || (size_t)h * w > (1u << 26)) return fail(c, DRP_EINVAL, "bad image size %d x %d", h, w);
    if (!(global_scale > 0.0)) return fail(c, DRP_EINVAL, "bad global_scale %g", global_scale);
    if (n_cap < 1) return fail(c, DRP_EINVAL, "bad output capacity %d", n_cap);
    const int BT = B * T;
    size_t fg_total = 0;
    for (int i = 0; i < BT; ++i) {
        const int ep = pd_name(episode, i / T), t = i % T;
        if (init_idx[i] < 0) return fail(c, DRP_EINVAL, "episode %d frame %d: sampler start %d", ep, t, init_idx[i]);
        if (!(radius[i] > 0.0) || !std::isfinite(radius[i]))
            return fail(c, DRP_EINVAL, "episode %d frame %d: bad fps radius %g", ep, t, radius[i]);
        if (n_fg_host[i] < 0 || (size_t)n_fg_host[i] > (size_t)h * w)
            return fail(c, DRP_EINVAL, "episode %d frame %d: host foreground count %d", ep, t, n_fg_host[i]);
        fg_total += (size_t)n_fg_host[i];
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (c->pd_pin.p) CHK(guarded_wait(c, nullptr));     // a call that failed before its wait may still copy from the staging
    for (int e = 0; e < PD_NEV; ++e)
        HIPCHK(c, c->pd_ev[e].create());
    c->pd_timed = false;
    c->pd_kind = 0;
    const size_t npix = (size_t)h * w;
    // the upload arena: depth [BT][npix] | radius [BT] | init [BT]
    const size_t o_radius = pd_align((size_t)BT * npix * sizeof(uint16_t));
    const size_t o_init = pd_align(o_radius + (size_t)BT * sizeof(double));
    const size_t in_bytes = pd_align(o_init + (size_t)BT * sizeof(int));
    const size_t meta_bytes = (size_t)2 * BT * sizeof(int);
    CHK(pd_pin_ensure(c, std::max(in_bytes, meta_bytes)));
    char* pin = ptr<char>(c->pd_pin);
    memcpy(pin, depth, (size_t)BT * npix * sizeof(uint16_t));
    memcpy(pin + o_radius, radius, (size_t)BT * sizeof(double));
    memcpy(pin + o_init, init_idx, (size_t)BT * sizeof(int));
    HIPCHK(c, hipEventRecord(c->pd_ev[0].ev, st));
    CHK(h2d(c, c->pd_in, pin, in_bytes));
    HIPCHK(c, hipEventRecord(c->pd_ev[1].ev, st));
    const char* in = static_cast<const char*>(c->pd_in.p);
    const uint16_t* d_depth = reinterpret_cast<const uint16_t*>(in);
    const double* d_radius = reinterpret_cast<const double*>(in + o_radius);
    const int* d_init = reinterpret_cast<const int*>(in + o_init);
    PdCam pc;
    for (int i = 0; i < 16; ++i) pc.M[i] = 0.0;         // no particle file: the extrinsics are not used
    pc.gs = global_scale;
    pc.fx = cam[0]; pc.fy = cam[1]; pc.cx = cam[2]; pc.cy = cam[3];

    // 1. depth -> clouds: tile counts, one scan over all images' tiles in (b, t) order, compaction
    const int nblk = px_nblk(npix);
    const size_t ntile = (size_t)BT * nblk;
    CHK(ensure(c, c->pd_blk, (2 * ntile + 2) * sizeof(unsigned long long)));
    unsigned long long* cnt = ptr<unsigned long long>(c->pd_blk);
    unsigned long long* off = cnt + ntile;
    CHK(ensure(c, c->pd_meta, (size_t)BT * (2 * sizeof(int) + sizeof(long long))));
    long long* d_pcd_off = ptr<long long>(c->pd_meta);
    int* d_nfg = reinterpret_cast<int*>(d_pcd_off + BT);
    int* d_counts = d_nfg + BT;
    // sized by the host's counts; the kernels write and read nothing beyond them if the device disagrees (an error below)
    const long long pcd_cap = (long long)std::max(fg_total, (size_t)1);
    CHK(ensure(c, c->pd_pcd, (size_t)pcd_cap * 3 * sizeof(double)));
    CHK(ensure(c, c->pd_dist, (size_t)pcd_cap * sizeof(double)));
    hipLaunchKernelGGL(k_pd_count, dim3(nblk, BT), dim3(PX_BLOCK), 0, st, d_depth, npix, global_scale * 1000.0, cnt);
    hipLaunchKernelGGL(k_px_scan_u64, dim3(1), dim3(1024), 0, st, cnt, (int)ntile, off);
    hipLaunchKernelGGL(k_pd_compact, dim3(nblk, BT), dim3(PX_BLOCK), 0, st, d_depth, npix, w, pc, off, pcd_cap, ptr<double>(c->pd_pcd));
    hipLaunchKernelGGL(k_pd_meta, dim3((BT + 255) / 256), dim3(256), 0, st, off, nblk, BT, d_nfg, d_pcd_off);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->pd_ev[2].ev, st));

    // 2. fps_rad, one workgroup per (sample, frame)
    const int cap = PD_CAP + 1;
    CHK(ensure(c, c->pd_chosen, (size_t)BT * cap * sizeof(int)));
    hipLaunchKernelGGL(k_pd_fps_rad, dim3(BT), dim3(1024), 0, st, ptr<double>(c->pd_pcd), pcd_cap, d_pcd_off, d_nfg, d_init,
                       d_radius, cap, ptr<double>(c->pd_dist), ptr<int>(c->pd_chosen), d_counts);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->pd_ev[3].ev, st));
    // the one wait before the download: foreground and particle counts size the rest
    CHK(d2h(c, pin, d_nfg, meta_bytes));
    CHK(guarded_wait(c, nullptr));
    const int* nfg = reinterpret_cast<const int*>(pin);
    const int* counts = nfg + BT;
    c->pd_lastB = BT;
    c->pd_nmax = 0;
    c->pd_kind = 2;
    int n_max = 0;
    for (int i = 0; i < BT; ++i) {
        const int ep = pd_name(episode, i / T), t = i % T;
        if (nfg[i] == 0) return fail(c, DRP_EINVAL, "episode %d frame %d: the depth image has no foreground pixel", ep, t);
        if (n_fg_host[i] != nfg[i])
            return fail(c, DRP_EINVAL, "episode %d frame %d: %d foreground pixels on the host, %d on the device", ep, t,
                        n_fg_host[i], nfg[i]);
        if (init_idx[i] >= nfg[i])
            return fail(c, DRP_EINVAL, "episode %d frame %d: sampler start %d outside the cloud of %d points", ep, t, init_idx[i],
                        nfg[i]);
        if (counts[i] > PD_CAP)
            return fail(c, DRP_EINVAL, "episode %d frame %d: fps_rad reached the cap of %d particles (radius %g)", ep, t, PD_CAP,
                        radius[i]);
        n_max = std::max(n_max, counts[i]);
    }
    if (n_max > n_cap) {
        int worst = 0;
        for (int i = 1; i < BT; ++i) if (counts[i] > counts[worst]) worst = i;
        return fail(c, DRP_EINVAL, "episode %d frame %d: the call needs %d particle slots, the outputs hold %d",
                    pd_name(episode, worst / T), worst % T, n_max, n_cap);
    }
    for (int i = 0; i < BT; ++i) counts_out[i] = counts[i];
    *n_max_out = n_max;
    c->pd_nmax = n_max;

    // 3. recenter (float64), one wavefront per (sample, frame, particle)
    CHK(ensure(c, c->pd_rec, (size_t)BT * n_max * 3 * sizeof(double)));
    hipLaunchKernelGGL(k_pd_recenter, dim3((BT * n_max + 3) / 4), dim3(256), 0, st, ptr<double>(c->pd_pcd), d_pcd_off, d_nfg,
                       ptr<int>(c->pd_chosen), cap, d_counts, d_radius, n_max, BT, ptr<double>(c->pd_rec));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->pd_ev[4].ev, st));

    // 4. pack: one rounding to float32, +0.0f beyond each count
    const size_t n_clouds = (size_t)BT * n_max * 3;
    CHK(ensure(c, c->pd_out, n_clouds * sizeof(float)));
    hipLaunchKernelGGL(k_pd_pack_frames, dim3((unsigned)((n_max + 255) / 256), BT), dim3(256), 0, st, ptr<double>(c->pd_rec),
                       d_counts, n_max, ptr<float>(c->pd_out));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->pd_ev[5].ev, st));

    // 5. one download through the pinned staging
    CHK(pd_pin_ensure(c, n_clouds * sizeof(float)));
    CHK(d2h(c, c->pd_pin.p, c->pd_out.p, n_clouds * sizeof(float)));
    HIPCHK(c, hipEventRecord(c->pd_ev[6].ev, st));
    CHK(guarded_wait(c, nullptr));
    memcpy(clouds_out, c->pd_pin.p, n_clouds * sizeof(float));
    c->pd_timed = true;
    return DRP_OK;
}

int drp_ptcl_dataset_time(drp_ctx* c, float* ms_out) {
    if (!c || !ms_out) return fail(c, DRP_EINVAL, "null argument");
    if (!c->pd_timed) return fail(c, DRP_ESTATE, "no drp_ptcl_dataset_batch or drp_ptcl_dataset_frames has completed");
    for (int e = 0; e + 1 < PD_NEV; ++e)
        if (hipEventElapsedTime(&ms_out[e], c->pd_ev[e].ev, c->pd_ev[e + 1].ev) != hipSuccess)
            return fail(c, DRP_EHIP, "hipEventElapsedTime failed");
    return DRP_OK;
}
