// capi_ptcl_dataset.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip inside extern "C", after
// capi_rgr_train.h).
// Here: GNN training batches from recorded episodes (row x4, dataset/dataset_gnn_dyn.py:86-201; kernels: k_ptcl_dataset.h).
// drp_ptcl_dataset_batch (one depth image per sample) and drp_ptcl_dataset_frames (row x4 / u1: every frame of a window) are one
// chain over n_img images, depth2fgpcd -> fps_rad -> recenter (pd_chain_begin, pd_chain_recenter, pd_chain_finish); an entry point
// keeps its argument checks, its own arena blocks, its n_cap refusal and its fourth stage.  They share the workspaces; c->pd_kind
// says whose bytes they hold, so a debug tap never hands back the other call's.
// The calls own their workspaces (c->pd_*): the PropNet weights, a training / planning session, the regressor and the
// particle-extraction buffers of drp_obs2ptcl are never touched.  The arena's layout and the per-image checks: ptcl_dataset_host.h.

namespace {
const int PD_BMAX = 1024;
const int PD_NEV = 7;           // events: start | upload | compaction | fps_rad | recenter | track + pack | download

int pd_pin_ensure(drp_ctx* c, size_t bytes) {
    // nothing of an earlier call may still copy from / to the block that goes
    if (c->pd_pin.p && c->pd_pin.cap < bytes) (void)hipStreamSynchronize(c->stream);
    return ensure_pinned(c, c->pd_pin, bytes);
}

struct PdCall {                 // a call over n_img images
    int kind;                   // c->pd_kind once its counts are in: 1 drp_ptcl_dataset_batch, 2 drp_ptcl_dataset_frames
    int n_img, T;               // kind 1: image b is sample b's, of T frames in its files; kind 2: image i is frame i % T of sample i / T
    const uint16_t* depth;      // [n_img][h][w]
    const int32_t* episode;     // the samples' names in a message, or null: their indices
    const double* radius;       // per image, as init_idx and n_fg_host
    const int32_t *init_idx, *n_fg_host;
    int h, w;
    double gs;                  // global_scale
    const double *cam, *T_cam;  // intrinsics [4]; extrinsics [16] or null (no particle file: not used)
    const int32_t* n_ptcl;      // kind 1 only, for the per-image checks: particles per sample, pushes [n_img][T-1][PD_PUSH]
    const double* push;
};
struct PdChain {                // what pd_chain_begin leaves for the stages behind it
    const char* in;             // the arena on the device
    PdCam pc;
    const double* d_radius;
    const long long* d_pcd_off;
    const int *d_nfg, *d_counts;
    const int* counts;          // on the host, in the pinned block until pd_chain_finish
    int n_max;
};

// "episode 12" / "episode 12 frame 3": image i of the call in a message
extern "C++" std::string pd_who(const PdCall& k, int i) {
    const int s = k.kind == 2 ? i / k.T : i;
    std::string who = "episode " + std::to_string(k.episode ? k.episode[s] : s);
    return k.kind == 2 ? who + " frame " + std::to_string(i % k.T) : who;
}

int pd_refuse(drp_ctx* c, const PdCall& k, const PdBad& bad, const int* nfg) {
    const int i = bad.img;
    const std::string name = pd_who(k, i);
    const char* who = name.c_str();
    switch (bad.fault) {
    case PD_NO_PTCL: return fail(c, DRP_EINVAL, "%s: %d particles in its files", who, k.n_ptcl[i]);
    case PD_BAD_INIT: return fail(c, DRP_EINVAL, "%s: sampler start %d", who, k.init_idx[i]);
    case PD_BAD_RADIUS: return fail(c, DRP_EINVAL, "%s: bad fps radius %g", who, k.radius[i]);
    case PD_PUSH_LEN:
        return fail(c, DRP_EINVAL, "%s: push %d has length %g", who, bad.push, k.push[((size_t)i * (k.T - 1) + bad.push) * PD_PUSH + 9]);
    case PD_PUSH_PLANE:
        return fail(c, DRP_EINVAL, "%s: push %d leaves the table plane (|push_dir_cam z| = %g >= 1e-6)", who, bad.push,
                    std::fabs(k.push[((size_t)i * (k.T - 1) + bad.push) * PD_PUSH + 8]));
    case PD_BAD_NFG: return fail(c, DRP_EINVAL, "%s: host foreground count %d", who, k.n_fg_host[i]);
    case PD_NO_FG: return fail(c, DRP_EINVAL, "%s: the depth image has no foreground pixel", who);
    case PD_NFG_DIFFERS:
        return fail(c, DRP_EINVAL, "%s: %d foreground pixels on the host, %d on the device", who, k.n_fg_host[i], nfg[i]);
    case PD_INIT_OUTSIDE:
        return fail(c, DRP_EINVAL, "%s: sampler start %d outside the cloud of %d points", who, k.init_idx[i], nfg[i]);
    default: return fail(c, DRP_EINVAL, "%s: fps_rad reached the cap of %d particles (radius %g)", who, PD_CAP, k.radius[i]);
    }
}

// Stages 0-2 and the one wait before the download: the per-image checks, the arena (fill_own(pin) stages the caller's own blocks
// of L) up, depth -> clouds, fps_rad, the counts back and checked.  ch.n_max: the most particles of an image
extern "C++" template <class Fill>
int pd_chain_begin(drp_ctx* c, const PdCall& k, const PdLayout& L, Fill fill_own, PdChain& ch) {
    const int n = k.n_img;
    const size_t npix = (size_t)k.h * k.w;
    const PdBad bad = pd_first_bad(n, npix, k.radius, k.init_idx, k.n_fg_host, k.n_ptcl, k.push, k.T);
    if (bad.fault != PD_FINE) return pd_refuse(c, k, bad, nullptr);
    size_t fg_total = 0;
    for (int i = 0; i < n; ++i) fg_total += (size_t)k.n_fg_host[i];
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (c->pd_pin.p) CHK(guarded_wait(c, nullptr));     // a call that failed before its wait may still copy from the staging
    for (int e = 0; e < PD_NEV; ++e)
        HIPCHK(c, c->pd_ev[e].create());
    c->pd_timed = false;
    c->pd_kind = 0;                 // the shared buffers are rewritten from here on: no tap until this call has its counts
    const size_t meta_bytes = (size_t)2 * n * sizeof(int);
    CHK(pd_pin_ensure(c, std::max(L.bytes, meta_bytes)));
    char* pin = ptr<char>(c->pd_pin);
    memcpy(pin + L.depth, k.depth, (size_t)n * npix * sizeof(uint16_t));
    memcpy(pin + L.radius, k.radius, (size_t)n * sizeof(double));
    memcpy(pin + L.init, k.init_idx, (size_t)n * sizeof(int));
    fill_own(pin);
    HIPCHK(c, hipEventRecord(c->pd_ev[0].ev, st));
    CHK(h2d(c, c->pd_in, pin, L.bytes));
    HIPCHK(c, hipEventRecord(c->pd_ev[1].ev, st));
    ch.in = static_cast<const char*>(c->pd_in.p);
    const uint16_t* d_depth = reinterpret_cast<const uint16_t*>(ch.in + L.depth);
    const int* d_init = reinterpret_cast<const int*>(ch.in + L.init);
    ch.d_radius = reinterpret_cast<const double*>(ch.in + L.radius);
    for (int i = 0; i < 16; ++i) ch.pc.M[i] = k.T_cam ? k.T_cam[i] : 0.0;
    ch.pc.gs = k.gs;
    ch.pc.fx = k.cam[0]; ch.pc.fy = k.cam[1]; ch.pc.cx = k.cam[2]; ch.pc.cy = k.cam[3];

    // 1. depth -> clouds: tile counts, one scan over all images' tiles in image order, compaction
    const int nblk = px_nblk(npix);
    const size_t ntile = (size_t)n * nblk;
    CHK(ensure(c, c->pd_blk, (2 * ntile + 2) * sizeof(unsigned long long)));
    unsigned long long* cnt = ptr<unsigned long long>(c->pd_blk);
    unsigned long long* off = cnt + ntile;
    CHK(ensure(c, c->pd_meta, (size_t)n * (2 * sizeof(int) + sizeof(long long))));
    long long* d_pcd_off = ptr<long long>(c->pd_meta);
    int* d_nfg = reinterpret_cast<int*>(d_pcd_off + n);
    int* d_counts = d_nfg + n;
    // sized by the host's counts; the kernels write and read nothing beyond them if the device disagrees (an error below)
    const long long pcd_cap = (long long)std::max(fg_total, (size_t)1);
    CHK(ensure(c, c->pd_pcd, (size_t)pcd_cap * 3 * sizeof(double)));
    CHK(ensure(c, c->pd_dist, (size_t)pcd_cap * sizeof(double)));
    hipLaunchKernelGGL(k_pd_count, dim3(nblk, n), dim3(PX_BLOCK), 0, st, d_depth, npix, k.gs * 1000.0, cnt);
    hipLaunchKernelGGL(k_px_scan_u64, dim3(1), dim3(1024), 0, st, cnt, (int)ntile, off);
    hipLaunchKernelGGL(k_pd_compact, dim3(nblk, n), dim3(PX_BLOCK), 0, st, d_depth, npix, k.w, ch.pc, off, pcd_cap, ptr<double>(c->pd_pcd));
    hipLaunchKernelGGL(k_pd_meta, dim3((n + 255) / 256), dim3(256), 0, st, off, nblk, n, d_nfg, d_pcd_off);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->pd_ev[2].ev, st));

    // 2. fps_rad, one workgroup per image
    const int cap = PD_CAP + 1;
    CHK(ensure(c, c->pd_chosen, (size_t)n * cap * sizeof(int)));
    hipLaunchKernelGGL(k_pd_fps_rad, dim3(n), dim3(1024), 0, st, ptr<double>(c->pd_pcd), pcd_cap, d_pcd_off, d_nfg, d_init,
                       ch.d_radius, cap, ptr<double>(c->pd_dist), ptr<int>(c->pd_chosen), d_counts);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->pd_ev[3].ev, st));
    // the one wait before the download: foreground and particle counts size the rest
    CHK(d2h(c, pin, d_nfg, meta_bytes));
    CHK(guarded_wait(c, nullptr));
    const int* nfg = reinterpret_cast<const int*>(pin);
    ch.counts = nfg + n;
    ch.d_pcd_off = d_pcd_off; ch.d_nfg = d_nfg; ch.d_counts = d_counts;
    c->pd_lastB = n;
    c->pd_nmax = 0;
    c->pd_kind = k.kind;
    const PdBad late = pd_first_bad_counts(n, nfg, ch.counts, k.n_fg_host, k.init_idx, PD_CAP);
    if (late.fault != PD_FINE) return pd_refuse(c, k, late, nfg);
    ch.n_max = *std::max_element(ch.counts, ch.counts + n);
    return DRP_OK;
}

// 3. recenter (float64), one wavefront per (image, particle), once the caller has found room for ch.n_max particles per image
int pd_chain_recenter(drp_ctx* c, const PdCall& k, const PdChain& ch) {
    c->pd_nmax = ch.n_max;
    CHK(ensure(c, c->pd_rec, (size_t)k.n_img * ch.n_max * 3 * sizeof(double)));
    hipLaunchKernelGGL(k_pd_recenter, dim3((k.n_img * ch.n_max + 3) / 4), dim3(256), 0, c->stream, ptr<double>(c->pd_pcd),
                       ch.d_pcd_off, ch.d_nfg, ptr<int>(c->pd_chosen), PD_CAP + 1, ch.d_counts, ch.d_radius, ch.n_max, k.n_img,
                       ptr<double>(c->pd_rec));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->pd_ev[4].ev, c->stream));
    return DRP_OK;
}

// 5. behind the caller's fourth stage: one download of c->pd_out through the pinned staging, where it then lies
int pd_chain_finish(drp_ctx* c, size_t bytes) {
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->pd_ev[5].ev, c->stream));
    CHK(pd_pin_ensure(c, bytes));
    CHK(d2h(c, c->pd_pin.p, c->pd_out.p, bytes));
    HIPCHK(c, hipEventRecord(c->pd_ev[6].ev, c->stream));
    CHK(guarded_wait(c, nullptr));
    c->pd_timed = true;
    return DRP_OK;
}
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
    size_t ptcl_floats = 0;
    std::vector<long long> ptcl_off(B);                 // of a sample without particles too: the chain refuses it before any use
    for (int b = 0; b < B; ++b) {
        ptcl_off[b] = (long long)ptcl_floats;
        ptcl_floats += (size_t)T * n_ptcl[b] * 4;
    }
    const PdCall k = {1, B, T, depth, episode, radius, init_idx, n_fg_host, h, w, global_scale, cam, T_cam, n_ptcl, push};
    const PdLayout L = pd_layout(B, (size_t)h * w, ptcl_floats, T);
    PdChain ch;
    CHK(pd_chain_begin(c, k, L, [&](char* pin) {
        memcpy(pin + L.ptcl, particles, ptcl_floats * sizeof(float));
        memcpy(pin + L.push, push, (size_t)B * (T - 1) * PD_PUSH * sizeof(double));
        memcpy(pin + L.nptcl, n_ptcl, (size_t)B * sizeof(int));
        memcpy(pin + L.ptcl_off, ptcl_off.data(), (size_t)B * sizeof(long long));
    }, ch));
    const int n_max = ch.n_max;
    for (int b = 0; b < B; ++b) counts_out[b] = ch.counts[b];
    if (n_max > n_cap) return fail(c, DRP_EINVAL, "the batch needs %d particle slots, the outputs hold %d", n_max, n_cap);
    *n_max_out = n_max;
    CHK(pd_chain_recenter(c, k, ch));

    // 4. track and pack
    const float* d_ptcl = reinterpret_cast<const float*>(ch.in + L.ptcl);
    const double* d_push = reinterpret_cast<const double*>(ch.in + L.push);
    const int* d_nptcl = reinterpret_cast<const int*>(ch.in + L.nptcl);
    const long long* d_poff = reinterpret_cast<const long long*>(ch.in + L.ptcl_off);
    const size_t n_states = (size_t)B * T * n_max * 3, n_sdelta = (size_t)B * (T - 1) * n_max * 3;
    CHK(ensure(c, c->pd_near, (size_t)B * n_max * sizeof(int)));
    CHK(ensure(c, c->pd_out, (n_states + n_sdelta) * sizeof(float)));
    const unsigned jb = (unsigned)((n_max + 255) / 256);
    hipLaunchKernelGGL(k_pd_nearest, dim3(jb, B), dim3(256), 0, c->stream, ptr<double>(c->pd_rec), ch.d_counts, n_max, d_ptcl,
                       d_poff, d_nptcl, ch.pc, ptr<int>(c->pd_near));
    hipLaunchKernelGGL(k_pd_pack, dim3(jb, T, B), dim3(256), 0, c->stream, ptr<int>(c->pd_near), ch.d_counts, n_max, T, d_ptcl,
                       d_poff, d_nptcl, d_push, ch.pc, ptr<float>(c->pd_out), ptr<float>(c->pd_out) + n_states);
    CHK(pd_chain_finish(c, (n_states + n_sdelta) * sizeof(float)));
    const float* res = ptr<const float>(c->pd_pin);
    memcpy(states_out, res, n_states * sizeof(float));
    memcpy(sdelta_out, res + n_states, n_sdelta * sizeof(float));
    return DRP_OK;
}

// Untracked samples straight from the depth frames: depth2fgpcd -> fps_rad -> recenter on every frame of B windows of T frames
// (dataset_gnn_dyn.py:97-101 per frame), the B * T images in (b, t) order through the chain of drp_ptcl_dataset_batch.
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
    const PdCall k = {2, BT, T, depth, episode, radius, init_idx, n_fg_host, h, w, global_scale, cam, nullptr, nullptr, nullptr};
    PdChain ch;
    CHK(pd_chain_begin(c, k, pd_layout(BT, (size_t)h * w), [](char*) {}, ch));
    const int n_max = ch.n_max;
    if (n_max > n_cap) {
        const int worst = (int)(std::max_element(ch.counts, ch.counts + BT) - ch.counts);
        return fail(c, DRP_EINVAL, "%s: the call needs %d particle slots, the outputs hold %d", pd_who(k, worst).c_str(), n_max, n_cap);
    }
    for (int i = 0; i < BT; ++i) counts_out[i] = ch.counts[i];
    *n_max_out = n_max;
    CHK(pd_chain_recenter(c, k, ch));

    // 4. pack: one rounding to float32, +0.0f beyond each count
    const size_t n_clouds = (size_t)BT * n_max * 3;
    CHK(ensure(c, c->pd_out, n_clouds * sizeof(float)));
    hipLaunchKernelGGL(k_pd_pack_frames, dim3((unsigned)((n_max + 255) / 256), BT), dim3(256), 0, c->stream, ptr<double>(c->pd_rec),
                       ch.d_counts, n_max, ptr<float>(c->pd_out));
    CHK(pd_chain_finish(c, n_clouds * sizeof(float)));
    memcpy(clouds_out, c->pd_pin.p, n_clouds * sizeof(float));
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
