// capi_ctx.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: the kernel-variant names, the run-time RCCL binding and the context (struct drp_ctx): every workspace, session and switch.

namespace {

std::string g_create_error;

enum KClass { KC_GRAPH = 0, KC_NODE_ENCODE, KC_EDGE_ENCODE, KC_PROJECT, KC_AGGREGATE, KC_UPDATE,
              KC_PREDICT, KC_REWARD, KC_MPPI, KC_PROP, KC_TAPE_COPY, KC_BWD_REWARD, KC_BWD_LISTS, KC_BWD_NODE, KC_BWD_EDGE,
              KC_BWD_PUSH, KC_OPT, KC_LOSS, KC_COUNT };
const char* const kclass_names[KC_COUNT] = {"graph", "node_encode", "edge_encode", "project",
                                            "aggregate", "update", "predict", "reward", "mppi", "prop",
                                            "tape_copy", "bwd_reward", "bwd_lists", "bwd_node", "bwd_edge", "bwd_push", "opt", "loss"};

// the variant names (DispatchVariant, dv_name), the dispatch policy and the plan functions: host-only, csrc/dispatch.h
using namespace dispatch;
static_assert(ENGINE_VALU == DRP_ENGINE_VALU && ENGINE_MFMA == DRP_ENGINE_MFMA && ENGINE_SPLIT == DRP_ENGINE_SPLIT && ENGINE_FUSED == DRP_ENGINE_FUSED && ENGINE_LITE == DRP_ENGINE_LITE &&
              K == DRP_K && GRAPH_THREADS_ == GRAPH_THREADS && GC_MAX_BANDS_ == GC_MAX_BANDS && GC_THREADS_ == GC_THREADS && PROP_WAVES_ == PROP_WAVES &&
              EC_UNITS_ == EC_UNITS && ROLLOUT_MAX_ROWS == KM_ROLLOUT_MAX_ROWS && BWD_ROWS_MAX == KMB_ROWS_MAX && COOP_SLOTS == KMB_COOP_SLOTS &&
              AGG_LDS_MAX_N == K_AGG_LDS_MAX_N && DEG_STAT_ROWS == DEG_STAT_MAX_ROWS && spread_grid(33) == SPREAD_GRID(33),
              "dispatch.h plans with the kernels' own constants");

// ---- what a context allocates: each resource is owned by the member that holds it ---------------------------------------
// Move-only; the destructor frees, release() frees now and leaves the owner empty.  A view into somebody else's memory is a
// plain pointer, never one of these.
struct DevBuf {                     // device memory (ensure() grows it)
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DevBuf() { (void)release(); }
    hipError_t release() { const hipError_t e = p ? hipFree(p) : hipSuccess; p = nullptr; cap = 0; return e; }
};

struct PinBuf {                     // pinned host memory (ensure_pinned() grows it); cap in bytes
    void* p = nullptr;
    size_t cap = 0;
    unsigned flags = hipHostMallocDefault;
    explicit PinBuf(unsigned f = hipHostMallocDefault) : flags(f) {}
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    PinBuf(PinBuf&& o) noexcept : p(o.p), cap(o.cap), flags(o.flags) { o.p = nullptr; o.cap = 0; }
    PinBuf& operator=(PinBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(flags, o.flags); return *this; }
    ~PinBuf() { (void)release(); }
    hipError_t release() { const hipError_t e = p ? hipHostFree(p) : hipSuccess; p = nullptr; cap = 0; return e; }
};

struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : ev(o.ev) { o.ev = nullptr; }
    Event& operator=(Event&& o) noexcept { std::swap(ev, o.ev); return *this; }
    ~Event() { (void)release(); }
    hipError_t create(unsigned flags = hipEventDefault) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags); }   // once
    hipError_t release() { const hipError_t e = ev ? hipEventDestroy(ev) : hipSuccess; ev = nullptr; return e; }
};

struct Stream {                     // the context's one stream; reads as the hipStream_t it holds
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value &&
              !std::is_copy_constructible<PinBuf>::value && !std::is_copy_assignable<PinBuf>::value &&
              !std::is_copy_constructible<Event>::value && !std::is_copy_assignable<Event>::value &&
              !std::is_copy_constructible<Stream>::value && !std::is_copy_assignable<Stream>::value,
              "a resource has one owner");

// ---- RCCL, bound at run time -----------------------------------------------------------------------------------
// libdrp.so does not link librccl: a process must not end up with two copies of it (PyTorch ships its own
// librccl.so beside the one under /opt/rocm; which of two mapped copies answered a call used to depend on the import
// order).  The first call that needs RCCL takes, in this order: $DRP_RCCL_LIB, the librccl that sits NEXT TO THE HIP RUNTIME
// this library itself runs on (dladdr of hipGetDeviceCount), a librccl the process has already mapped (dl_iterate_phdr),
// /opt/rocm/lib/librccl.so.1 (include/drp.h says the same).
// Only entry points whose ABI has been stable since NCCL 2.4 are used (no ncclConfig_t crosses the boundary).
struct RcclApi {
    void* handle = nullptr;
    std::string path, error;
    int version = 0;
    ncclResult_t (*GetVersion)(int*) = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*CommGetAsyncError)(ncclComm_t, ncclResult_t*) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

int rccl_find_mapped(struct dl_phdr_info* info, size_t, void* data) {
    const char* name = info->dlpi_name;
    if (name && *name) {
        const char* base = strrchr(name, '/');
        base = base ? base + 1 : name;
        if (strncmp(base, "librccl.so", 10) == 0) {
            *static_cast<std::string*>(data) = name;
            return 1;
        }
    }
    return 0;
}

RcclApi g_rccl;
RcclApi* rccl_api() {
    RcclApi& api = g_rccl;
    static std::once_flag once;
    std::call_once(once, [&api] {
        std::vector<std::string> tries;
        if (const char* e = getenv("DRP_RCCL_LIB")) tries.push_back(e);
        // The RCCL that belongs to the HIP runtime THIS library runs on comes first: a process can hold two HIP runtimes
        // (PyTorch's wheel ships its own copy next to its librccl; imported after this library it does not replace the
        // system runtime this library is already bound to), and an RCCL talking to the other one finds no device
        // (ncclCommInitRank: "no ROCm-capable device is detected").
        {
            Dl_info hi;
            if (dladdr(reinterpret_cast<void*>(&hipGetDeviceCount), &hi) && hi.dli_fname) {
                std::string dir(hi.dli_fname);
                const size_t slash = dir.rfind('/');
                if (slash != std::string::npos) {
                    dir.resize(slash + 1);
                    tries.push_back(dir + "librccl.so.1");
                    tries.push_back(dir + "librccl.so");
                }
            }
        }
        std::string mapped;
        dl_iterate_phdr(rccl_find_mapped, &mapped);
        if (!mapped.empty()) tries.push_back(mapped);
        tries.push_back("librccl.so.1");
        tries.push_back("/opt/rocm/lib/librccl.so.1");
        tries.push_back("librccl.so");
        for (const std::string& t : tries) {
            api.handle = dlopen(t.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (api.handle) break;
            const char* de = dlerror();
            api.error += t + ": " + (de ? de : "?") + "; ";
        }
        if (!api.handle) return;
        bool ok = true;
        auto sym = [&](const char* n) { void* p = dlsym(api.handle, n); if (!p) { ok = false; api.error += std::string(n) + " missing; "; } return p; };
        api.GetVersion = reinterpret_cast<decltype(api.GetVersion)>(sym("ncclGetVersion"));
        api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(sym("ncclGetUniqueId"));
        api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(sym("ncclCommInitRank"));
        api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
        api.CommAbort = reinterpret_cast<decltype(api.CommAbort)>(sym("ncclCommAbort"));
        api.CommCount = reinterpret_cast<decltype(api.CommCount)>(sym("ncclCommCount"));
        api.CommUserRank = reinterpret_cast<decltype(api.CommUserRank)>(sym("ncclCommUserRank"));
        api.CommGetAsyncError = reinterpret_cast<decltype(api.CommGetAsyncError)>(sym("ncclCommGetAsyncError"));
        api.AllGather = reinterpret_cast<decltype(api.AllGather)>(sym("ncclAllGather"));
        api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
        if (!ok) { dlclose(api.handle); api.handle = nullptr; return; }
        Dl_info di;
        if (dladdr(reinterpret_cast<void*>(api.AllGather), &di) && di.dli_fname) api.path = di.dli_fname;
        (void)api.GetVersion(&api.version);
    });
    return api.handle ? &api : nullptr;
}

struct WgradQueue;                  // capi_pipeline.h: its methods use the context
double now_s() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

}  // namespace

// One step's workspace (run_step, launch_graph, the rollouts' rows): the staged inputs, the impulses, the neighbour lists, the
// stage kernels' intermediates, the output.  A *_f64 call swaps the context's against one of its own (capi_f64.h: F64Scope).
struct StepWs {
    DevBuf s_in, attr, dens, s_delta, nbr_idx, nbr_cnt, eff, c_node, agg, proj, proj2, c_edge, s_out;
    DevBuf ecache;                  // the edge-chain cache of the whole-sample kernels (dispatch.h: cut_blocks)
};

// What a step leaves behind on the host side (F64Scope saves and restores it by value)
struct StepMarks {
    int lastB = 0, lastN = 0, lastH = 0;            // last shapes (for debug fetch)
    int probe_cls = -1;                             // the probed kernel class (drp_probe_begin)
    unsigned deg_tick = 0;                          // note_degrees: every eighth launch refreshes deg_stat
    unsigned char dv_hit[DV_COUNT] = {};            // kernel variants launched since drp_dispatch_reset (DispatchVariant)
};

struct drp_ctx {
    Stream stream;                  // declared first, so destroyed last: every buffer, pinned block and event below goes before it
    int device = 0;
    std::string err;
    int engine = DRP_ENGINE_VALU;
    int n_cu = 256;
    DispatchPolicy pol;             // every threshold and switch that decides which kernel runs (dispatch.h; policy_from_env)
    bool comm_always = false;       // DRP_COMM_ALWAYS=1: a one-rank communicator still goes through ncclAllGather (bench.py --force-comm)
    bool train_copy_upload = false; // DRP_TRAIN_COPY_UPLOAD=1: the training batch goes up by a copy on the stream instead of inside kt_unpack_inputs
    bool debug_force_giveup = false; // DRP_DEBUG_FORCE_GIVEUP=1 (tests): drp_train_step's first pass ends as if kmb_step_bwd's barrier had timed out
    // the mean in-degree the last lists of a shape had (k_deg_stat, every few launches): sum | rows << 24 | N << 48 in host memory
    // the device writes; the plans take it decoded (deg()), as an input
    PinBuf deg_stat{hipHostMallocMapped};
    unsigned long long* deg_stat_dev = nullptr;     // the device's address of deg_stat
    DegStat deg() const { return deg_stat.p ? decode_deg_stat(*static_cast<volatile const unsigned long long*>(deg_stat.p)) : DegStat{}; }

    // model constants
    bool have_weights = false, have_cam = false, have_goal = false;
    double adj_thresh = 0.08;       // the radius as the caller gave it (a Python float): the threshold squares THIS value
    float thr = 0.0064f;
    SplitRange re_range{};          // range shift 2^k of the split relation encoder and the bound it rests on
    float re_scale = 1.0f, re_inv = 1.0f;
    bool re_ok = true;
    int re_shift_env = 0x7fffffff;  // a fixed shift k instead of the one derived from the weights (experiments)
    DevBuf w_raw, w_valu, w_mfma, w_mfma_bwd, w_split, w_split6, w_split6_bwd;
    DrpCam cam{};
    DevBuf goal_field, goal_coor, cself;
    unsigned cself_tag = 0;         // bumped by every prepare_cself: who filled c->cself last
    int goal_h = 0, goal_w = 0, goal_m = 0;
    // the goal table of multi-scene sessions (drp_set_goal_scenes / drp_set_goal_image_scenes): gt_S goals of one image size,
    // fields [S][h][w], pixels [S][m_max][2] with counts gt_m [S]; gt_S = 0: none installed.  The single goal above is another thing.
    DevBuf gt_fields, gt_coor, gt_m, gt_rows, scene_seeds;
    int gt_S = 0, gt_h = 0, gt_w = 0, gt_m_max = 0;

    // workspaces: a step's engine and buffers are run_step's arguments (StepArgs); `ws` is what the selected engine's calls pass
    StepWs ws;
    StepMarks marks;
    DevBuf states, actions, rewards, scratch;

    // MPC state
    bool mpc_on = false;
    unsigned mpc_cself_tag = 0;     // the session's self-edge constants are in c->cself while this equals cself_tag
    const float* mpc_cself = nullptr;
    const uint8_t* mpc_cself_ok = nullptr;
    float sess_attr_max = 0.0f, sess_dens_max = 0.0f;   // of the running MPC session (range check of later uploads)
    drp_mpc_params mpc{};
    int mpc_S = 0;                  // scenes of the running session (drp_mpc_begin_scenes); 0: a single-scene session on the single goal
    DevBuf nominal, noise, partials, gathered, stats, elite, elite_all, xchg;
    int n_ranks = 1, rank = 0;
    ncclComm_t comm = nullptr;
    bool comm_failed = false;            // a wait gave up or RCCL reported an error: the communicator is gone and every entry point
    int comm_failed_ranks = 0;           // that would use it answers DRP_ECOMM until drp_comm_destroy / a fresh drp_comm_init
    double comm_timeout_s = 60.0;        // DRP_COMM_TIMEOUT_S: a wait behind a collective gives up after this long (guarded_wait)
    double comm_init_timeout_s = 300.0;  // DRP_COMM_INIT_TIMEOUT_S: ncclCommInitRank (every rank must arrive)

    // gradient-descent planner state
    int gd_engine = DRP_ENGINE_FUSED;        // which engine writes the session's tape (pick_tape_engine)
    bool gd_on = false;
    int gd_nb = 0, gd_N = 0, gd_B = 0, gd_H = 0, gd_iter = 0;
    int gd_S = 0, gd_scene_nb = 0;           // drp_gd_begin_scenes: scenes and columns per scene (gd_nb = gd_S * gd_scene_nb); 0: the single goal
    PinBuf gd_pin[DRP_GD_SLOTS];             // drp_gd_step_async: pinned host copies [B rewards | B*H*4 pushes] of the iterations in flight,
    Event gd_ev[DRP_GD_SLOTS];               //   written by the iteration's own kernels (kb_reward, k_adam): no copy on the stream
    bool gd_pending[DRP_GD_SLOTS] = {};
    PinBuf mpc_pin[2];                       // drp_mpc_fetch_async: [B*H*4 pushes | B final rewards] of two iterations in flight
    Event mpc_ev[2];
    bool mpc_pending[2] = {false, false};
    unsigned gd_cself_tag = 0;      // the self-edge constants of this GD problem are in c->cself while the tags match
    const float* gd_cself = nullptr;
    const uint8_t* gd_cself_ok = nullptr;
    double gd_lr = 0.05;
    float gd_lo[4] = {0, 0, 0, 0}, gd_hi[4] = {0, 0, 0, 0};
    DevBuf eff_hist, g_eff, g_cnode, g_agg, g_proj, g_state, g_sdelta, g_act, adam_m, adam_v;
    DevBuf tape_sdelta, tape_idx, tape_cnt, tape_mask, g_agg_hist, rev_off, rev, gpos_edge;
    // planning on a caller's cost (drp_gd_begin_cost, drp_gd_*_seeded; drp_mpc_begin_cost, drp_mpc_set_rewards)
    bool gd_cost = false;           // the GD session was begun without a goal: the built-in reward's calls are refused
    DevBuf gd_seed_in, gd_seed;     // the caller's seed as it arrives [B][H][N][3], and steps 0 .. H-2 of it step-major [H-1][B,N,3]
    bool mpc_cost = false;          // the sampling session was begun without a goal: its rollout runs no reward kernel
    bool mpc_rewards_ok = true;     // a cost session: the final-step rewards of the last rollout are in (drp_mpc_set_rewards)
    // planning to a target cloud (capi_cloud_goal.h: drp_set_goal_cloud, drp_mpc_begin_cloud, drp_gd_begin_cloud): one cloud beside
    // the image goal and the goal table (cg_q), its kind and parameters; cg_tab: the running cloud session's tables per start
    // column, eps [n_batch] then the target's self problem's value sums [n_batch]; cg_scratch: kg_sinkhorn's [2][rows] value sums and, in a GD
    // session, [2][rows][N][3] gradient sums; cg_io: the one-shot's inputs, tables, scratch and results (it shares nothing with a session)
    bool have_cloud_goal = false;
    int cg_kind = 0, cg_M = 0, cg_iters = 0;
    double cg_weight = 1.0, cg_eps_scale = 1.0;
    DevBuf cg_q, cg_tab, cg_scratch, cg_io;
    bool mpc_cloud = false;         // the sampling session was begun by drp_mpc_begin_cloud: its rollout ends in the cloud reward kernel
    bool gd_cloud = false;          // the GD session was begun by drp_gd_begin_cloud: the cloud kernel stands in kb_reward's place

    // particle extraction (row f2)
    DevBuf px_depth, px_mask, px_blk, px_bmin, px_bmax, px_grid, px_pcd, px_keys, px_cellcnt, px_cellfill,
        px_celloff, px_list, px_down, px_down32, px_init, px_dist, px_chosen, px_pts, px_r, px_rr, px_out;

    // training (row f4)
    bool tr_on = false;
    int tr_nroll = 0, tr_iter = 0;
    double tr_lr = 1e-3, tr_beta1 = 0.9;
    std::vector<float> w_host;
    std::unique_ptr<WgradQueue> wgrad;      // the weight-gradient jobs of a backward pass and their buffers (capi_pipeline.h; from drp_create on)
    bool wgrad_defer = true;        // DRP_NO_WGRAD_DEFER=1 turns the deferred weight gradients off
    bool wgrad_tap_on = false;      // the operands of the last deferred pass still lie where its jobs read them (capi_debug.h:
                                    // "train_wgrad_*"); set by a trainer pass that returned DRP_OK, cleared by whatever may write them next
    // INVARIANT of the "train_wgrad_*" taps: whatever writes (or re-allocates) an operand of the deferred weight-gradient jobs --
    // agg_hist, tr_hact .. tr_xn and ed_* here; eff_hist, g_eff, g_proj, g_cnode, g_state and ws.dens elsewhere in this struct --
    // clears wgrad_tap_on first.  Today every such writer stages a step through ensure_step_ws (capi_pipeline.h), which clears
    // it; a new writer that does not go through there must clear it itself.
    DevBuf tr_grad, tr_m, tr_v, tr_loss, agg_hist, tr_hact, tr_gh, tr_gpe, tr_a1n,
        tr_gh1, tr_xn, ed_re, ed_a2, ed_a1, ed_x0, ed_gce, ed_g3, ed_g2, ed_g1;
    // the optimiser seam (capi_optim.h: drp_train_accumulate, drp_train_apply); allocated by drp_train_begin
    DevBuf tr_acc;                  // the float64 accumulator [W_TOTAL]
    DevBuf tr_opt;                  // ko_norm_partial's partials [KO_BLOCKS(W_TOTAL)] doubles, then ko_norm_final's KoStep
    DevBuf tr_g32;                  // the scaled, clipped gradient the last drp_train_apply stepped on [W_TOTAL]
    PinBuf opt_pin;                 // pinned: the KoStep of the last drp_train_apply, written by ko_norm_final
    bool tr_grad_fresh = false;     // tr_grad holds the gradient of a DRP_TRAIN_GRAD pass that returned DRP_OK and has not been accumulated
    int tr_acc_n = 0;               // passes accumulated since the last drp_train_apply / drp_train_begin

    // goal pre-processing (row f3)
    DevBuf gl_goal, gl_seg, gl_tmp, gl_dist, gl_blk, gl_pix, gl_fps;

    // resolution regressor (capi_rgr.h): its own weights and workspaces, nothing shared with the PropNet state
    DevBuf rgr_w, rgr_raw, rgr_x, rgr_a[5], rgr_f[4], rgr_slab, rgr_out, rgr_mask, rgr_dtmp, rgr_dist, rgr_tab;
    int rgr_nout = 0;               // 0: nothing loaded
    int rgr_lastB = 0;              // batch of the last forward (debug taps)
    int rgr_tab_h = 0, rgr_tab_w = 0;   // the image size rgr_tab was built for
    std::vector<int> rgr_tab_host;      // its host image (INTER_AREA tables: offsets and indices, then the float weights)
    // its training (capi_rgr_train.h): allocated from drp_rgr_train_begin on
    DevBuf rgr_m, rgr_v, rgr_g, rgr_gfull, rgr_dz[2], rgr_gf, rgr_bpart, rgr_l1, rgr_lossp, rgr_tgt;
    bool rgr_tr_on = false;             // drp_rgr_train_begin since the last drp_rgr_load
    double rgr_tr_lr = 0.0, rgr_tr_beta1 = 0.9, rgr_tr_lam = 0.0;
    long rgr_tr_iter = 0;               // Adam steps taken
    int rgr_tr_lastB = 0;               // batch of the last training step (its inputs stay staged on the device)

    // GNN training batches from recorded episodes (capi_ptcl_dataset.h, row x4): workspaces of its own
    DevBuf pd_in, pd_blk, pd_meta, pd_pcd, pd_dist, pd_chosen, pd_rec, pd_near, pd_out;
    PinBuf pd_pin;                  // pinned staging: the upload arena, then the counts, then the download
    Event pd_ev[7];                 // stage boundaries of the last drp_ptcl_dataset_batch / _frames (drp_ptcl_dataset_time)
    bool pd_timed = false;
    int pd_lastB = 0, pd_nmax = 0;  // shapes of the last batch (debug taps); for a frames call pd_lastB = B * T images
    int pd_kind = 0;                // whose bytes the shared pd_* buffers hold: 0 nobody's (a call is under way or failed), 1
                                    // drp_ptcl_dataset_batch ("pd_*" taps), 2 drp_ptcl_dataset_frames ("pdf_*" taps)

    // float64 one-step evaluation and the accuracy probe (k_prop_f64.h, capi_f64.h): weights, staging and workspaces of its own,
    // nothing shared with the sessions' state -- a *_f64 call or a probe ends no session
    DevBuf f64_w;                   // the blob widened [W_TOTAL], then its nine 64x64 blocks in MFMA fragment order, then in the transposed order (KF_W_ALL doubles)
    bool f64_w_valid = false;       // drp_load_weights refreshes it; an optimiser step on the device clears it, the next *_f64 call rebuilds
    size_t f64_cap = (size_t)256 << 20;     // bytes of float64 workspace a call may hold: the batch is walked in sample chunks under it
    StepWs f64_ws;                  // stands in for `ws` while a *_f64 call runs (capi_f64.h: F64Scope)
    DevBuf f64_pe, f64_eff, f64_agg, f64_re, f64_erel, f64_pred, f64_out, f64_red;
    int f64_lastB = 0, f64_lastN = 0, f64_chunks = 0;       // of the last *_f64 call (drp_f64_tap)
    DevBuf grad64_ws, grad64_io;    // drp_gd_grad_f64 and drp_train_grad_f64 (capi_grad_f64.h; one-shots that keep nothing between calls): a chunk's tape
                                    // and reverse pass (the trainer: and its samples' gradient accumulators); the batch's inputs and results

    DevBuf cloud_io;                // drp_cloud_chamfer, drp_cloud_chamfer_f64, drp_cloud_match (capi_pipeline.h: cloud_begin; one-shots that
                                    // end in a wait and keep nothing between calls): the running call's inputs and results
    bool ka64_ready = false;        // ka64_match's dynamic LDS size is set (capi_match_f64.h: ka64_run, at first use)

    // re-packing after an optimiser step on the device (k_train.h): gather maps of the plain packers, pinned copy of the blob
    DevBuf map_valu, map_mfma, map_mfma_bwd;
    bool repack_maps_ready = false;
    PinBuf w_pin;                   // pinned: the blob after an optimiser step [W_TOTAL], then the device's range shift (one int)
    PinBuf tr_pin;                  // pinned staging of a training batch (drp_train_step: one upload)
    DevBuf tr_arena, re_shift_dev;  // the batch as uploaded; the shift kt_repack_all derived
    bool repack_device = true;      // DRP_NO_REPACK_DEVICE=1: fetch the blob and run the host packers (the round-2 path)

    // km_rollout's argument block (device copy + what it holds)
    DevBuf roll_args;
    std::vector<RolloutArgs> roll_args_host;
    bool roll_args_valid = false;

    void dv(int id) { marks.dv_hit[id] = 1; }

    // probe
    DevBuf probe_work;              // PROP_WORK_* counters of the propagation kernels while their class is probed
    bool probe_count = false;       // drp_probe_begin("prop+work"): the kernels count what they execute (not for timed regions: the
                                    // counting costs the 300-particle launch 8 %)
    bool work_lite = false, work_full = false;   // which term counts the counted launches ran with (drp_probe_work weighs the units by them)
    unsigned long long* work_ptr() const { return (marks.probe_cls == KC_PROP && probe_count) ? static_cast<unsigned long long*>(probe_work.p) : nullptr; }
    std::vector<Event> probe_ev;
    size_t probe_used = 0;
    long probe_prop_kernels = 0;    // kernel launches inside the regions of the "prop" probe (drp_probe_prop_launches)
};

