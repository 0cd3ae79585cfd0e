// capi_pipeline.h -- a section of the C ABI's translation unit (textually included by drp_capi.hip, which has the order of the sections).
// Here: internal helpers and pipelines: guarded waits, probes, the graph build, one predict_one_step on every engine (run_step), reward, rollouts (run_rollout), weight packing, deferred weight gradients, the range check, what a one-shot on two clouds does around its launch.

namespace {

int fail(drp_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

#define HIPCHK(c, expr)                                                                    \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail((c), DRP_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                               \
    } while (0)

#define CHK(expr)                  \
    do {                           \
        int rc_ = (expr);          \
        if (rc_ != DRP_OK) return rc_; \
    } while (0)

int guarded_wait(drp_ctx* c, hipEvent_t ev);
int ensure(drp_ctx* c, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap) return DRP_OK;
    // hipFree waits for the device: behind a collective that cannot finish it would never return
    if (b.p && c && c->comm != nullptr && (c->n_ranks > 1 || c->comm_always)) CHK(guarded_wait(c, nullptr));
    HIPCHK(c, b.release());
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) return fail(c, DRP_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    b.cap = bytes;
    return DRP_OK;
}

// Pinned host memory: nothing happens when the capacity suffices; otherwise the block goes, a new one comes and the owner records
// its size.  The caller says, at the call, why nothing can still be reading or writing the old block.
int ensure_pinned(drp_ctx* c, PinBuf& b, size_t bytes) {
    if (bytes <= b.cap) return DRP_OK;
    HIPCHK(c, b.release());
    HIPCHK(c, hipHostMalloc(&b.p, bytes, b.flags));
    b.cap = bytes;
    return DRP_OK;
}

template <typename T>
T* ptr(const DevBuf& b) { return static_cast<T*>(b.p); }
template <typename T>
T* ptr(const PinBuf& b) { return static_cast<T*>(b.p); }

int h2d(drp_ctx* c, DevBuf& b, const void* src, size_t bytes) {
    CHK(ensure(c, b, bytes));
    HIPCHK(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return DRP_OK;
}

int d2h(drp_ctx* c, void* dst, const void* src, size_t bytes) {
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    return DRP_OK;
}

// ---- waits that cannot hang on a dead peer --------------------------------------------------------------------
// With a communicator attached, the stream may hold an ncclAllGather that never completes (a rank died, a rank took
// another branch).  Every host wait of the context then polls instead of blocking: the stream / event, the
// communicator's asynchronous error, and a deadline (DRP_COMM_TIMEOUT_S, default 60 s).  On error or timeout the
// communicator is ABORTED (ncclCommAbort ends the collective's kernel on this rank), the context falls back to one
// rank and the call returns DRP_ECOMM: the process can report and exit instead of sitting in hipStreamSynchronize.
bool comm_live(const drp_ctx* c) { return c->comm != nullptr && (c->n_ranks > 1 || c->comm_always); }

// Helper threads (ncclCommAbort behind a dead collective, ncclCommInitRank waiting for its peers) are tracked: drp_destroy,
// drp_comm_destroy and process exit give them a bounded time to finish, so that none is still inside RCCL when the stream,
// the context or the HIP / RCCL libraries' own statics go away.
struct HelperState { std::atomic<int> done{0}; const void* owner = nullptr; };   // owner: the context the thread works for
std::mutex g_helpers_mu;
std::vector<std::shared_ptr<HelperState>> g_helpers;
std::shared_ptr<HelperState> helper_register(const void* owner) {
    auto h = std::make_shared<HelperState>();
    h->owner = owner;
    std::lock_guard<std::mutex> lk(g_helpers_mu);
    static bool at_exit = false;
    if (!at_exit) {
        at_exit = true;
        atexit([] {
            const double t0 = now_s();
            for (;;) {
                bool busy = false;
                { std::lock_guard<std::mutex> lk2(g_helpers_mu); for (auto& q : g_helpers) busy = busy || !q->done.load(std::memory_order_acquire); }
                if (!busy || now_s() - t0 > 5.0) return;
                usleep(1000);
            }
        });
    }
    g_helpers.erase(std::remove_if(g_helpers.begin(), g_helpers.end(), [](const std::shared_ptr<HelperState>& q) { return q->done.load() != 0; }), g_helpers.end());
    g_helpers.push_back(h);
    return h;
}
// the helper threads of ONE context (another context's communicator still waiting for its peers is not this one's business)
void helpers_wait(double seconds, const void* owner) {
    const double t0 = now_s();
    for (;;) {
        bool busy = false;
        { std::lock_guard<std::mutex> lk(g_helpers_mu); for (auto& q : g_helpers) busy = busy || (q->owner == owner && !q->done.load(std::memory_order_acquire)); }
        if (!busy || now_s() - t0 > seconds) return;
        usleep(500);
    }
}

void comm_abort(drp_ctx* c) {
    RcclApi* R = rccl_api();
    // ncclCommAbort raises the communicator's abort flag (a collective's kernel spinning on a peer sees it and ends) and
    // then waits for the device to drain: on a helper thread, so that the caller gets its error code NOW
    if (c->comm && R) {
        ncclComm_t comm = c->comm;
        const int dev = c->device;
        auto h = helper_register(c);
        std::thread([R, comm, dev, h] { (void)hipSetDevice(dev); (void)R->CommAbort(comm); h->done.store(1, std::memory_order_release); }).detach();
    }
    // the failure is STICKY: the ranks' shards are no longer combined, so nothing that would have used the communicator may
    // quietly carry on with this rank's data alone
    c->comm_failed = true;
    c->comm_failed_ranks = c->n_ranks;
    c->comm = nullptr;
    c->n_ranks = 1;
    c->rank = 0;
}
int comm_failed_error(drp_ctx* c) {
    return fail(c, DRP_ECOMM, "the communicator of %d ranks was aborted after a failed wait or an RCCL error: call drp_comm_destroy "
                "(continue alone) or drp_comm_init with a fresh id before the next collective step", c->comm_failed_ranks);
}

int guarded_wait(drp_ctx* c, hipEvent_t ev) {
    if (!comm_live(c)) {
        const hipError_t e = ev ? hipEventSynchronize(ev) : hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, DRP_EHIP, "%s failed: %s", ev ? "hipEventSynchronize" : "hipStreamSynchronize", hipGetErrorString(e));
        return DRP_OK;
    }
    RcclApi* R = rccl_api();
    const double t0 = now_s();
    for (unsigned spin = 0;; ++spin) {
        const hipError_t e = ev ? hipEventQuery(ev) : hipStreamQuery(c->stream);
        if (e == hipSuccess) return DRP_OK;
        if (e != hipErrorNotReady) return fail(c, DRP_EHIP, "%s failed: %s", ev ? "hipEventQuery" : "hipStreamQuery", hipGetErrorString(e));
        if ((spin & 63) == 63) {
            ncclResult_t ae = ncclSuccess;
            if (R && R->CommGetAsyncError(c->comm, &ae) == ncclSuccess && ae != ncclSuccess && ae != ncclInProgress) {
                comm_abort(c);
                return fail(c, DRP_ECOMM, "RCCL reported an asynchronous error (%s); communicator aborted", R->GetErrorString(ae));
            }
            const double dt = now_s() - t0;
            if (dt > c->comm_timeout_s) {
                const int nr = c->n_ranks, rk = c->rank;
                comm_abort(c);
                return fail(c, DRP_ECOMM, "rank %d of %d waited %.1f s behind a collective (DRP_COMM_TIMEOUT_S=%g): a peer is gone "
                            "or took another path; communicator aborted", rk, nr, dt, c->comm_timeout_s);
            }
            if (dt > 2e-3) usleep(50);            // past the length of any iteration's tail: stop burning the core
            else sched_yield();
        }
    }
}

// probe bracket: an event before and one after the launches of the probed class
struct ProbeScope {
    drp_ctx* c;
    bool on;
    ProbeScope(drp_ctx* ctx, int cls) : c(ctx), on(ctx->marks.probe_cls == cls) {
        if (on) rec();
    }
    ~ProbeScope() {
        if (on) rec();
    }
    void rec() {
        if (c->probe_used == c->probe_ev.size()) {
            Event e;
            if (e.create() != hipSuccess) { on = false; return; }
            c->probe_ev.push_back(std::move(e));
        }
        (void)hipEventRecord(c->probe_ev[c->probe_used++].ev, c->stream);
    }
    void launched() { if (on) ++c->probe_prop_kernels; }      // a kernel of the "prop" class inside this region
};

int ensure_step_ws(drp_ctx* c, StepWs& ws, int B, int N, int engine = -1) {
    if (engine < 0) engine = c->engine;
    c->wgrad_tap_on = false;        // every call that stages a step's inputs comes through here: the densities, the tape and the
                                    // reverse pass's buffers are about to be rewritten (or grown: their contents are gone)
    // (ws.s_in, ws.attr, ws.dens and ws.s_out grow with the upload that fills them, ws.ecache with the plan that wants it)
    const size_t bn = (size_t)B * N;
    CHK(ensure(c, ws.s_delta, bn * 3 * sizeof(float)));
    CHK(ensure(c, ws.nbr_idx, bn * DRP_K * sizeof(int16_t)));
    CHK(ensure(c, ws.nbr_cnt, bn));
    CHK(ensure(c, ws.eff, bn * 64 * sizeof(float)));
    CHK(ensure(c, ws.c_node, bn * 64 * sizeof(float)));
    CHK(ensure(c, ws.agg, bn * 64 * sizeof(float)));
    CHK(ensure(c, ws.proj, bn * 128 * sizeof(float)));
    CHK(ensure(c, ws.proj2, bn * 128 * sizeof(float)));
    // edge constants [B,N,10,64] for the engines that materialise them; the fused engine only parks the graph build's
    // sorted positions and strip starts there (launch_graph)
    const size_t graph_scratch = (size_t)B * (((size_t)N + 3) & ~(size_t)3) * 16 + (size_t)B * (GC_MAX_BANDS * GC_XS + 1) * sizeof(int);
    CHK(ensure(c, ws.c_edge, engine_is_fused(engine) ? graph_scratch : std::max(graph_scratch, bn * DRP_K * 64 * sizeof(float))));
    c->marks.lastB = B;
    c->marks.lastN = N;
    return DRP_OK;
}

// Every few launches whose pairing depends on it (dispatch.h: PairRule), the mean in-degree of the lists just built goes to host
// memory behind the launch: the next launches of this shape read it there, without waiting for anything.
static void note_degrees(drp_ctx* c, const uint8_t* nbr_cnt, long spw, long N, long B) {
    const long rows = spw * N;
    if (rows > c->pol.prop_pair_rows || rows <= c->pol.prop_pair_always) return;
    if ((c->marks.deg_tick++ & 7u) != 0) return;
    if (!c->deg_stat.p) {                       // mapped (its flags): the device writes it, the host reads it; without it the plans see no degree
        if (ensure_pinned(c, c->deg_stat, sizeof(unsigned long long)) != DRP_OK) {
            (void)hipGetLastError();
            return;
        }
        *ptr<unsigned long long>(c->deg_stat) = 0ull;
        if (hipHostGetDevicePointer(reinterpret_cast<void**>(&c->deg_stat_dev), c->deg_stat.p, 0) != hipSuccess) {
            (void)c->deg_stat.release();
            (void)hipGetLastError();
            return;
        }
    }
    hipLaunchKernelGGL(k_deg_stat, dim3(1), dim3(1024), 0, c->stream, nbr_cnt,
                       (int)std::min(B * N, (long)DEG_STAT_MAX_ROWS), (int)N, c->deg_stat_dev);
}

struct StepArgs {
    const float* s_prev; int prev_mod; size_t prev_stride;   // state read by sample b: row b % prev_mod
    const float* attr; int attr_mod;
    const float* dens; int dens_mod;
    const float* actions; size_t act_stride;                  // null: s_delta already in workspace
    bool build_graph;                                         // false: nbr lists already in workspace
    float* s_out; size_t out_stride;
    int B, N;
    int engine;                                               // which engine runs the step
    float* s_delta; int16_t* nbr_idx; uint8_t* nbr_cnt;       // where the step's impulses and neighbour lists are (or go)
    // tape for the backward pass (fused engine only, km_prop<., TAPE>):
    float* eff_hist = nullptr;      // [4][B*N*64]: effect after the encoder and after every propagation step
    unsigned* mask_hist = nullptr;  // [3][B*N*10][2]: ReLU masks of the relation effects of every propagation step
    float* agg_hist = nullptr;      // [3][B*N*64]: aggregated edge effects of every propagation step (training), nullable
    const float* cself = nullptr;   // [B,64] self-edge constant + per-sample validity (fused engine, k_cself)
    const uint8_t* cself_ok = nullptr;
    bool padded = false;            // training batches: zero-padded (coincident) particles -> plain k_graph
    int* rev_off = nullptr;         // the GD planner's forward, samples of one graph chunk: the reversed lists in the lists' own launch
    int* rev = nullptr;             //   (k_graph_rev); run_step says in rev_built whether it did
    bool* rev_built = nullptr;
};
// a step on the selected engine whose impulses and lists are the context's workspace (sized before: ensure_step_ws)
StepArgs step_args(const drp_ctx* c, int engine) {
    StepArgs a{};
    a.engine = engine; a.s_delta = ptr<float>(c->ws.s_delta); a.nbr_idx = ptr<int16_t>(c->ws.nbr_idx); a.nbr_cnt = ptr<uint8_t>(c->ws.nbr_cnt);
    return a;
}

// neighbour lists as planned (plan_graph): cells, x strips, four threads per receiver, or the plain sweep; the two builds
// that share their launch with something else (k_graph_rev, km_graph_q4_encode) are run_step's
void launch_graph(drp_ctx* c, hipStream_t st, const GraphPlan& g, const float* s_prev, int prev_mod, size_t prev_stride,
                  const float* actions, size_t act_stride, float* s_delta, int B, int N, int16_t* nbr_idx, uint8_t* nbr_cnt,
                  int self_first) {
    // sorted positions and strip / cell starts live in the edge-constant buffer: whatever uses it runs after the lists exist
    const size_t Np = ((size_t)N + 3) & ~(size_t)3;
    float4* sorted = reinterpret_cast<float4*>(c->ws.c_edge.p);
    int* starts = reinterpret_cast<int*>(sorted + (size_t)B * Np);
    const dim3 grid((unsigned)g.grid);
    switch (g.kind) {
    case GraphPlan::CELLS:
        // two-dimensional cells: y bands, 1-cm x strips inside a band
        hipLaunchKernelGGL(k_graph_sort2, dim3(B), dim3(GRAPH_SORT_THREADS), 0, st, s_prev, prev_mod, prev_stride, actions,
                           act_stride, s_delta, N, c->cam, g.gy, g.inv_hb, sorted, starts);
        hipLaunchKernelGGL(k_graph_cells, grid, dim3(GC_THREADS), GRAPH_CELLS_LDS(g.gy * GC_XS), st,
                           (const float4*)sorted, (const int*)starts, N, g.gy, g.inv_hb, nbr_idx, nbr_cnt, c->thr, g.chunks,
                           B * g.chunks, self_first, g.halo);
        break;
    case GraphPlan::STRIPS128:
    case GraphPlan::STRIPS256:
        hipLaunchKernelGGL(k_graph_sort, dim3(B), dim3(GRAPH_SORT_THREADS), 0, st, s_prev, prev_mod, prev_stride, actions,
                           act_stride, s_delta, N, c->cam, sorted, starts);
        if (g.kind == GraphPlan::STRIPS256)
            hipLaunchKernelGGL(k_graph_strips_q<256>, grid, dim3(256), GRAPH_STRIPS_LDS(N, 256), st,
                               (const float4*)sorted, (const int*)starts, N, nbr_idx, nbr_cnt, c->thr, g.chunks, B * g.chunks, self_first);
        else
            hipLaunchKernelGGL(k_graph_strips_q<GRAPH_THREADS>, grid, dim3(GRAPH_THREADS), GRAPH_STRIPS_LDS(N, GRAPH_THREADS), st,
                               (const float4*)sorted, (const int*)starts, N, nbr_idx, nbr_cnt, c->thr, g.chunks, B * g.chunks, self_first);
        break;
    case GraphPlan::Q4:
        // a handful of samples (training batches): four threads per receiver, each over a quarter of the senders
        hipLaunchKernelGGL(k_graph_q4, grid, dim3(GRAPH_Q4_THREADS), GRAPH_Q4_LDS(N), st, s_prev, prev_mod,
                           prev_stride, actions, act_stride, s_delta, N, nbr_idx, nbr_cnt, c->cam, c->thr, g.chunks, self_first);
        break;
    default:
        hipLaunchKernelGGL(k_graph, grid, dim3(GRAPH_THREADS), (size_t)4 * N * sizeof(float), st, s_prev,
                           prev_mod, prev_stride, actions, act_stride, s_delta, N, nbr_idx, nbr_cnt, c->cam, c->thr,
                           g.chunks, B * g.chunks, self_first);
        break;
    }
}

void launch_aggregate(drp_ctx* c, const AggPlan& g, const int16_t* nbr_idx, const uint8_t* nbr_cnt, int B, int N) {
    ProbeScope ps(c, KC_AGGREGATE);
    if (g.lds)
        hipLaunchKernelGGL(k_aggregate_lds, dim3(B), dim3(512), (size_t)N * 256, c->stream,
                           ptr<float>(c->ws.c_edge), ptr<float>(c->ws.proj), nbr_idx, nbr_cnt, N, ptr<float>(c->ws.agg));
    else
        hipLaunchKernelGGL(k_aggregate, dim3(B * g.chunks), dim3(256), 0, c->stream, ptr<float>(c->ws.c_edge),
                           ptr<float>(c->ws.proj), nbr_idx, nbr_cnt, N, ptr<float>(c->ws.agg), g.chunks);
}

// kernels whose tile loop is workgroup-cyclic first (tile = block + grid x (wave + 8 round)): one workgroup per tile up to the chip
int mfma_grid_spread(drp_ctx* c, long ntiles) {
    const long cap = (long)c->n_cu;
    return (int)(ntiles < cap ? (ntiles > 0 ? ntiles : 1) : cap);
}
int mfma_grid(drp_ctx* c, long ntiles) {
    long blocks = (ntiles + MFMA_WAVES - 1) / MFMA_WAVES;
    long cap = (long)c->n_cu;
    return (int)(blocks < cap ? (blocks > 0 ? blocks : 1) : cap);
}

// The instantiations of km_prop / km_prop3 / km_rollout by their flags' index (dispatch.h), filled from the lists that
// declare and instantiate them (k_prop_inst.h): a launch is table[flags.index()]
struct PropTables {
    decltype(&km_prop<false, false, false, false>) prop[PropFlags::COUNT];
    decltype(&km_prop3<false, false, false, false, false>) prop3[Prop3Flags::COUNT];
    decltype(&km_rollout<false, false, false, false>) rollout[RolloutFlags::COUNT];
    // the reduced-product instantiations (ENGINE_LITE), by lite_index()
    decltype(&km_prop<false, false, false, false>) prop_lite[PropFlags::LITE_COUNT];
    decltype(&km_prop3<false, false, false, false, false>) prop3_lite[Prop3Flags::LITE_COUNT];
    decltype(&km_rollout<false, false, false, false>) rollout_lite[RolloutFlags::LITE_COUNT];
    int filled = 0;
    auto of(const PropFlags& f) const { return f.lite ? prop_lite[f.lite_index()] : prop[f.index()]; }
    auto of(const Prop3Flags& f) const { return f.lite ? prop3_lite[f.lite_index()] : prop3[f.index()]; }
    auto of(const RolloutFlags& f) const { return f.lite ? rollout_lite[f.lite_index()] : rollout[f.index()]; }
};
const PropTables& prop_tables() {
    static const PropTables tables = [] {
        PropTables t{};
#define KM_TAB_PROP(L, T, P, W) t.prop[PropFlags{L, T, P, W}.index()] = km_prop<L, T, P, W>; ++t.filled;
#define KM_TAB_PROP3(T, P, E, W, O) t.prop3[Prop3Flags{T, P, (E) ? ((O) ? 2 : 1) : 0, W}.index()] = km_prop3<T, P, E, W, O>; ++t.filled;
#define KM_TAB_ROLLOUT(P, E, W, O) t.rollout[RolloutFlags{P, (E) ? ((O) ? 2 : 1) : 0, W}.index()] = km_rollout<P, E, W, O>; ++t.filled;
        KM_PROP_LIST_TAPE(KM_TAB_PROP, false)
        KM_PROP_LIST_TAPE(KM_TAB_PROP, true)
        KM_PROP3_LIST_TAPE(KM_TAB_PROP3, false)
        KM_PROP3_LIST_TAPE(KM_TAB_PROP3, true)
        KM_ROLLOUT_LIST(KM_TAB_ROLLOUT)
#define KM_TAB_PROP_LITE(L, T, P, W) t.prop_lite[PropFlags{L, T, P, W, true}.lite_index()] = km_prop<L, T, P, W, true>; ++t.filled;
#define KM_TAB_PROP3_LITE(T, P, E, W, O) t.prop3_lite[Prop3Flags{T, P, (E) ? ((O) ? 2 : 1) : 0, W, true}.lite_index()] = km_prop3<T, P, E, W, O, true>; ++t.filled;
#define KM_TAB_ROLLOUT_LITE(P, E, W, O) t.rollout_lite[RolloutFlags{P, (E) ? ((O) ? 2 : 1) : 0, W, true}.lite_index()] = km_rollout<P, E, W, O, true>; ++t.filled;
        KM_PROP_LIST_TAPE(KM_TAB_PROP_LITE, false)
        KM_PROP3_LIST_TAPE(KM_TAB_PROP3_LITE, false)
        KM_ROLLOUT_LIST(KM_TAB_ROLLOUT_LITE)
#undef KM_TAB_PROP_LITE
#undef KM_TAB_PROP3_LITE
#undef KM_TAB_ROLLOUT_LITE
#undef KM_TAB_PROP
#undef KM_TAB_PROP3
#undef KM_TAB_ROLLOUT
        return t;
    }();
    return tables;
}
static_assert(sizeof(PropTables::prop) / sizeof(void*) == PropFlags::COUNT && sizeof(PropTables::prop3) / sizeof(void*) == Prop3Flags::COUNT &&
              sizeof(PropTables::rollout) / sizeof(void*) == RolloutFlags::COUNT, "a table entry per index of the family's flags");
// drp_create: every entry is there, and may use its dynamic LDS
bool prop_tables_ready() {
    const PropTables& t = prop_tables();
    bool ok = t.filled == PropFlags::COUNT + Prop3Flags::COUNT + RolloutFlags::COUNT + PropFlags::LITE_COUNT + Prop3Flags::LITE_COUNT + RolloutFlags::LITE_COUNT;
    for (int q = 0; q < PropFlags::LITE_COUNT && ok; ++q)
        ok = t.prop_lite[q] && hipFuncSetAttribute((const void*)t.prop_lite[q], hipFuncAttributeMaxDynamicSharedMemorySize, KM_PROP_LDS(PropFlags::from_lite_index(q).last)) == hipSuccess;
    for (int q = 0; q < Prop3Flags::LITE_COUNT && ok; ++q)
        ok = t.prop3_lite[q] && hipFuncSetAttribute((const void*)t.prop3_lite[q], hipFuncAttributeMaxDynamicSharedMemorySize, KM_PROP3_LDS) == hipSuccess;
    for (int q = 0; q < RolloutFlags::LITE_COUNT && ok; ++q)
        ok = t.rollout_lite[q] && hipFuncSetAttribute((const void*)t.rollout_lite[q], hipFuncAttributeMaxDynamicSharedMemorySize, KM_ROLLOUT_LDS) == hipSuccess;
    for (int q = 0; q < PropFlags::COUNT && ok; ++q)
        ok = t.prop[q] && hipFuncSetAttribute((const void*)t.prop[q], hipFuncAttributeMaxDynamicSharedMemorySize, KM_PROP_LDS(PropFlags::from_index(q).last)) == hipSuccess;
    for (int q = 0; q < Prop3Flags::COUNT && ok; ++q)
        ok = t.prop3[q] && hipFuncSetAttribute((const void*)t.prop3[q], hipFuncAttributeMaxDynamicSharedMemorySize, KM_PROP3_LDS) == hipSuccess;
    for (int q = 0; q < RolloutFlags::COUNT && ok; ++q)
        ok = t.rollout[q] && hipFuncSetAttribute((const void*)t.rollout[q], hipFuncAttributeMaxDynamicSharedMemorySize, KM_ROLLOUT_LDS) == hipSuccess;
    return ok;
}

StepShape step_shape(const drp_ctx* c, const StepArgs& a) {
    StepShape s;
    s.engine = a.engine; s.B = a.B; s.N = a.N;
    s.tape = a.eff_hist != nullptr;
    s.prev_mod = a.prev_mod; s.attr_mod = a.attr_mod; s.dens_mod = a.dens_mod;
    s.work = c->work_ptr() != nullptr;
    s.build_graph = a.build_graph; s.padded = a.padded; s.has_actions = a.actions != nullptr; s.wants_rev = a.rev_off != nullptr;
    s.deg = c->deg();
    return s;
}

// MLP stages of one step on the matrix-core kernels as planned (graph already built, s_delta in workspace)
int run_step_mfma(drp_ctx* c, const StepArgs& a, const StepPlan& k) {
    const int B = a.B, N = a.N;
    hipStream_t st = c->stream;
    const float* mw = ptr<float>(c->w_mfma);
    const dim3 blk(64 * MFMA_WAVES);
    const long node_tiles = (long)B * ((N + 31) / 32);
    const long edge_tiles = (long)B * ((N * DRP_K + 31) / 32);
    const size_t bn64 = (size_t)B * N * 64;
    const bool tape = k.tape;
    // the tape of the reverse-mode kernels: km_prop<., TAPE> on the fused engine; on the fp32 matrix engine (what the
    // gradient-descent planner and the trainer fall back to when the split-fp16 relation encoder refuses the weights or the
    // inputs) the stage kernels run as always and the tape is copied / written beside them (tape_mfma below)
    if (tape && a.engine != DRP_ENGINE_FUSED && a.engine != DRP_ENGINE_MFMA)       // (run_tape_forward passes one of the two)
        return fail(c, DRP_ESTATE, "the backward tape is written by the fused or the fp32 matrix engine");
    float* eff0 = (tape && !k.tape_mfma) ? a.eff_hist : ptr<float>(c->ws.eff);
    if (k.node_encode) {
        ProbeScope ps(c, KC_NODE_ENCODE);
        if (k.fused)
            hipLaunchKernelGGL(k.lite ? km_node_encode_split<true> : km_node_encode_split<false>, dim3(mfma_grid_spread(c, node_tiles)), blk, KM_NODE_SPLIT_LDS, st,
                               ptr<uint16_t>(c->w_split6), mw, a.s_delta, a.attr, a.attr_mod, a.dens,
                               a.dens_mod, N, B, eff0, ptr<float>(c->ws.c_node), ptr<float>(c->ws.proj));
        else
            hipLaunchKernelGGL(km_node_encode, dim3(mfma_grid(c, node_tiles)), blk, KM_NODE_LDS, st, mw,
                               a.s_delta, a.attr, a.attr_mod, a.dens, a.dens_mod, N, B,
                               ptr<float>(c->ws.eff), ptr<float>(c->ws.c_node), ptr<float>(c->ws.proj));
    }
    if (k.fused) {
        // the relation encoder is recomputed inside the propagation kernels and c_edge is never materialised
        float* pa = ptr<float>(c->ws.proj);
        float* pb = ptr<float>(c->ws.proj2);
        unsigned long long* const wk = c->work_ptr();    // not null: the counting instantiations (drp_probe_begin("prop+work"))
        if (wk) (k.lite ? c->work_lite : c->work_full) = true;
        const dim3 pblk(64 * PROP_WAVES);
        if (k.prop3) {
            // one launch per block of samples (dispatch.h: cut_blocks) -- the tape's launches too: the history buffers are laid
            // out for the whole batch, a block starts `ro` rows into every slot and the kernel takes the slots' stride as an
            // argument (hist_rows)
            ProbeScope ps(c, KC_PROP);
            if (k.blocks.cache) CHK(ensure(c, c->ws.ecache, k.blocks.cache_bytes));
            note_degrees(c, a.nbr_cnt, k.spw, N, B);
            for (int q = 0; q < k.blocks.n; ++q) {
                const Block b = k.blocks.block(q);
                // the block's view of every per-sample buffer: inputs replicated over the batch columns (row b reads column
                // b % mod) keep their base -- a block starts at a multiple of mod --, everything indexed by the row moves on
                const size_t ro = (size_t)b.b_off * N;
                const bool own_prev = a.prev_mod >= B, own_attr = a.attr_mod >= B, own_dens = a.dens_mod >= B;
                if (b.cache_bytes > c->ws.ecache.cap) CHK(ensure(c, c->ws.ecache, b.cache_bytes));
                hipLaunchKernelGGL(prop_tables().of(k.prop3_flags(b)), dim3((unsigned)b.grid), pblk, KM_PROP3_LDS, st,
                                   ptr<uint16_t>(c->w_split), ptr<uint16_t>(c->w_split6), mw,
                                   own_prev ? a.s_prev + (size_t)b.b_off * a.prev_stride : a.s_prev, own_prev ? b.Bc : a.prev_mod, a.prev_stride,
                                   own_attr ? a.attr + ro : a.attr, own_attr ? b.Bc : a.attr_mod,
                                   own_dens ? a.dens + b.b_off : a.dens, own_dens ? b.Bc : a.dens_mod,
                                   a.nbr_idx + ro * DRP_K, a.nbr_cnt + ro, pa + ro * 128, pb + ro * 128,
                                   ptr<float>(c->ws.c_node) + ro * 64, (tape ? a.eff_hist : ptr<float>(c->ws.eff)) + ro * 64, N, b.Bc, b.spw,
                                   k.phase_e ? (const float*)(a.s_delta + ro * 3) : (const float*)nullptr,
                                   a.s_out + (size_t)b.b_off * a.out_stride, a.out_stride,
                                   a.cself ? a.cself + (size_t)b.b_off * 64 : (const float*)nullptr,
                                   a.cself_ok ? a.cself_ok + b.b_off : (const uint8_t*)nullptr,
                                   tape ? a.mask_hist + ro * DRP_K * 2 : (unsigned*)nullptr,
                                   (tape && a.agg_hist) ? a.agg_hist + ro * 64 : (float*)nullptr, c->re_scale, c->re_inv,
                                   (c->pol.prop3_order ? 1 : 0), ptr<float4>(c->ws.ecache), b.ec_stride, wk, tape ? (size_t)B * N : (size_t)0);
                ps.launched();
            }
        }
        for (int p = 0; p < DRP_PSTEP && !k.prop3; ++p) {
            const bool last = (p + 1 == DRP_PSTEP);
            ProbeScope ps(c, KC_PROP);
            hipLaunchKernelGGL(prop_tables().of(k.prop_flags(last)), dim3((unsigned)k.grid), pblk, KM_PROP_LDS(last), st,
                               ptr<uint16_t>(c->w_split), ptr<uint16_t>(c->w_split6), mw, a.s_prev, a.prev_mod, a.prev_stride,
                               a.attr, a.attr_mod, a.dens, a.dens_mod, a.nbr_idx, a.nbr_cnt, pa,
                               ptr<float>(c->ws.c_node), tape ? a.eff_hist + (size_t)p * bn64 : ptr<float>(c->ws.eff),
                               tape ? a.eff_hist + (size_t)(p + 1) * bn64 : ptr<float>(c->ws.eff), N, B, pb, a.s_out, a.out_stride, a.cself, a.cself_ok,
                               tape ? a.mask_hist + (size_t)p * B * N * DRP_K * 2 : (unsigned*)nullptr,
                               (tape && a.agg_hist) ? a.agg_hist + (size_t)p * bn64 : (float*)nullptr,
                               c->re_scale, c->re_inv, k.spread, wk);
            ps.launched();
            float* tmp = pa; pa = pb; pb = tmp;
        }
        return DRP_OK;
    }
    {
        ProbeScope ps(c, KC_EDGE_ENCODE);
        if (k.split_encoders)
            hipLaunchKernelGGL(km_edge_encode_split, dim3(mfma_grid(c, edge_tiles)), blk, KM_EDGE_SPLIT_LDS, st,
                               ptr<uint16_t>(c->w_split), mw, a.s_prev, a.prev_mod, a.prev_stride, a.attr,
                               a.attr_mod, a.dens, a.dens_mod, a.nbr_idx,
                               a.nbr_cnt, N, B, ptr<float>(c->ws.c_edge), c->re_scale, c->re_inv);
        else
            hipLaunchKernelGGL(km_edge_encode, dim3(mfma_grid(c, edge_tiles)), blk, KM_EDGE_LDS, st, mw,
                               a.s_prev, a.prev_mod, a.prev_stride, a.attr, a.attr_mod, a.dens, a.dens_mod,
                               a.nbr_idx, a.nbr_cnt, N, B, ptr<float>(c->ws.c_edge));
    }
    if (k.tape_mfma) HIPCHK(c, hipMemcpyAsync(a.eff_hist, c->ws.eff.p, bn64 * sizeof(float), hipMemcpyDeviceToDevice, st));
    for (int p = 0; p < DRP_PSTEP; ++p) {
        if (k.tape_mfma) {
            // the aggregate that also leaves the edges' ReLU bits; the aggregated rows and the effects are copied into the tape
            ProbeScope pa(c, KC_AGGREGATE);
            hipLaunchKernelGGL(k_aggregate_tape, dim3(B * k.agg.chunks), dim3(256), 0, st, ptr<float>(c->ws.c_edge), ptr<float>(c->ws.proj),
                               a.nbr_idx, a.nbr_cnt, N, ptr<float>(c->ws.agg), k.agg.chunks,
                               a.mask_hist + (size_t)p * B * N * DRP_K * 2);
            if (a.agg_hist)
                HIPCHK(c, hipMemcpyAsync(a.agg_hist + (size_t)p * bn64, c->ws.agg.p, bn64 * sizeof(float), hipMemcpyDeviceToDevice, st));
        } else {
            launch_aggregate(c, k.agg, a.nbr_idx, a.nbr_cnt, B, N);
        }
        {
        ProbeScope ps(c, p + 1 < DRP_PSTEP ? KC_UPDATE : KC_PREDICT);
        if (p + 1 < DRP_PSTEP)
            hipLaunchKernelGGL(km_update<false>, dim3(mfma_grid(c, node_tiles)), blk, KM_UPD_LDS, st, mw,
                               ptr<float>(c->ws.agg), ptr<float>(c->ws.c_node), ptr<float>(c->ws.eff), N, B,
                               ptr<float>(c->ws.proj), a.s_prev, a.prev_mod, a.prev_stride, a.s_out, a.out_stride);
        else
            hipLaunchKernelGGL(km_update<true>, dim3(mfma_grid(c, node_tiles)), blk, KM_UPD_LDS, st, mw,
                               ptr<float>(c->ws.agg), ptr<float>(c->ws.c_node), ptr<float>(c->ws.eff), N, B,
                               ptr<float>(c->ws.proj), a.s_prev, a.prev_mod, a.prev_stride, a.s_out, a.out_stride);
        }
        // the step's effect is the next tape entry (km_update keeps it in place, the last step's too)
        if (k.tape_mfma)
            HIPCHK(c, hipMemcpyAsync(a.eff_hist + (size_t)(p + 1) * bn64, c->ws.eff.p, bn64 * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    return DRP_OK;
}

// One predict_one_step (model/gnn_dyn.py:209-254) [+ gen_s_delta, planners.py:346] for B samples: planned once
// (dispatch.h: plan_step), every variant the plan launches marked here, then carried out
int run_step(drp_ctx* c, const StepArgs& a) {
    const int B = a.B, N = a.N;
    hipStream_t st = c->stream;
    float* s_delta = a.s_delta;
    int16_t* nbr_idx = a.nbr_idx;
    uint8_t* nbr_cnt = a.nbr_cnt;
    const float* vw = ptr<float>(c->w_valu);
    const StepPlan k = plan_step(c->pol, c->n_cu, step_shape(c, a));
    k.mark(c->marks.dv_hit);
    if (a.build_graph) {
        ProbeScope ps(c, KC_GRAPH);
        const int self_first = (engine_is_fused(a.engine) && a.cself != nullptr) ? 1 : 0;
        switch (k.graph.kind) {
        case GraphPlan::REV:
            // the GD planner's forward, samples of one graph chunk: the reversed lists in the lists' own launch
            hipLaunchKernelGGL(k_graph_rev, dim3((unsigned)k.graph.grid), dim3(GRAPH_THREADS), (size_t)12 * N * sizeof(int), st, a.s_prev,
                               a.prev_mod, a.prev_stride, a.actions, a.act_stride, s_delta, N, nbr_idx, nbr_cnt, c->cam, c->thr,
                               B, self_first, a.rev_off, a.rev);
            if (a.rev_built) *a.rev_built = true;
            break;
        case GraphPlan::Q4_ENCODE:
            // a handful of samples whose impulses are data (the trainer's forward pass): the lists and the particle encoder
            // read nothing of one another -- one launch (k_rollout.h)
            hipLaunchKernelGGL(k.graph.lite ? km_graph_q4_encode<true> : km_graph_q4_encode<false>, dim3((unsigned)(k.graph.grid + mfma_grid_spread(c, (long)B * ((N + 31) / 32)))), dim3(GRAPH_Q4_THREADS),
                               KM_GRAPH_Q4_ENCODE_LDS(N), st, a.s_prev, a.prev_mod, a.prev_stride, s_delta, N, B, nbr_idx, nbr_cnt, c->cam,
                               c->thr, k.graph.chunks, self_first, (int)k.graph.grid, ptr<uint16_t>(c->w_split6), ptr<float>(c->w_mfma), a.attr, a.attr_mod,
                               a.dens, a.dens_mod, k.tape ? a.eff_hist : ptr<float>(c->ws.eff), ptr<float>(c->ws.c_node), ptr<float>(c->ws.proj));
            break;
        default:
            launch_graph(c, st, k.graph, a.s_prev, a.prev_mod, a.prev_stride, a.actions, a.act_stride, s_delta, B, N, nbr_idx, nbr_cnt, self_first);
            break;
        }
    }
    if (a.engine != DRP_ENGINE_VALU) {
        int rc = run_step_mfma(c, a, k);
        if (rc != DRP_OK) return rc;
        HIPCHK(c, hipGetLastError());
        return DRP_OK;
    }
    {
        ProbeScope ps(c, KC_NODE_ENCODE);
        hipLaunchKernelGGL(k_node_encode<8>, dim3(B), dim3(256), 0, st, vw, s_delta, a.attr,
                           a.attr_mod, a.dens, a.dens_mod, N, ptr<float>(c->ws.eff), ptr<float>(c->ws.c_node));
    }
    {
        ProbeScope ps(c, KC_EDGE_ENCODE);
        hipLaunchKernelGGL(k_edge_encode, dim3(B), dim3(256), (6 * 64 + 3 * 4096) * sizeof(float), st,
                           vw, a.s_prev, a.prev_mod, a.prev_stride, a.attr, a.attr_mod, a.dens,
                           a.dens_mod, nbr_idx, nbr_cnt, N, ptr<float>(c->ws.c_edge));
    }
    for (int p = 0; p < DRP_PSTEP; ++p) {
        {
            ProbeScope ps(c, KC_PROJECT);
            hipLaunchKernelGGL(k_project<8>, dim3(B), dim3(256), 0, st, vw, ptr<float>(c->ws.eff), N,
                               ptr<float>(c->ws.proj));
        }
        launch_aggregate(c, k.agg, a.nbr_idx, a.nbr_cnt, B, N);
        {
            ProbeScope ps(c, KC_UPDATE);
            hipLaunchKernelGGL(k_update<8>, dim3(B), dim3(256), 0, st, vw, ptr<float>(c->ws.agg),
                               ptr<float>(c->ws.c_node), N, ptr<float>(c->ws.eff));
        }
    }
    {
        ProbeScope ps(c, KC_PREDICT);
        hipLaunchKernelGGL(k_predict<8>, dim3(B), dim3(256), 0, st, vw, ptr<float>(c->ws.eff), a.s_prev,
                           a.prev_mod, a.prev_stride, N, a.s_out, a.out_stride);
    }
    HIPCHK(c, hipGetLastError());
    return DRP_OK;
}

// the installed goal table as the scene kernels take it: rows of the session layout (nb columns per scene, `div` rows per
// sample row), or an explicit scene per row
GoalTable goal_table(const drp_ctx* c, int nb, int div, const int* scene_of_row = nullptr) {
    GoalTable t{};
    t.fields = static_cast<const float*>(c->gt_fields.p); t.coor = static_cast<const float*>(c->gt_coor.p);
    t.m = static_cast<const int*>(c->gt_m.p); t.scene_of_row = scene_of_row;
    t.field_stride = (size_t)c->gt_h * c->gt_w; t.m_max = c->gt_m_max; t.S = c->gt_S; t.nb = nb > 0 ? nb : 1; t.div = div > 0 ? div : 1;
    return t;
}

// scenes > 0: a goal per row from the goal table (k_reward_scenes; scene_nb columns per scene, div rows per sample row, or
// scene_of_row); else the single goal
int run_reward(drp_ctx* c, const float* state, size_t row_stride, int rows, int N, int normalize,
               float* out, int scenes = 0, int scene_nb = 1, int div = 1, const int* scene_of_row = nullptr) {
    ProbeScope ps(c, KC_REWARD);
    c->dv(DV_REWARD);
    if (scenes > 0) {
        hipLaunchKernelGGL(k_reward_scenes, dim3(rows), dim3(256), (2 * ((N + 3) & ~3) + 8) * sizeof(float), c->stream, state,
                           row_stride, N, goal_table(c, scene_nb, div, scene_of_row), c->gt_h, c->gt_w, c->cam, normalize, out);
        HIPCHK(c, hipGetLastError());
        return DRP_OK;
    }
    hipLaunchKernelGGL(k_reward, dim3(rows), dim3(256), (2 * ((N + 3) & ~3) + 8) * sizeof(float), c->stream, state,
                       row_stride, N, ptr<float>(c->goal_field), c->goal_h, c->goal_w,
                       ptr<float>(c->goal_coor), c->goal_m, c->cam, normalize, out);
    HIPCHK(c, hipGetLastError());
    return DRP_OK;
}

// H-step rollout over device-resident s0/attr/dens (in s_in/attr/dens, nb rows) and actions.
// Self-edge constant of the fused engine (k_cself): one vector per sample, constant over a whole
// rollout (it depends on the attributes and the density only).  Null pointers when it does not apply.
int prepare_cself(drp_ctx* c, int attr_mod, int N, int B, const float** cself, const uint8_t** cself_ok, int engine = -1) {
    if (engine < 0) engine = c->engine;
    *cself = nullptr;
    *cself_ok = nullptr;
    if (engine_is_fused(engine) && c->pol.self_const) {
        CHK(ensure(c, c->cself, (size_t)B * 64 * sizeof(float) + (size_t)B));
        float* cs = ptr<float>(c->cself);
        uint8_t* ok = reinterpret_cast<uint8_t*>(cs + (size_t)B * 64);
        hipLaunchKernelGGL(k_cself, dim3(B), dim3(64), 0, c->stream, ptr<float>(c->w_valu), ptr<float>(c->ws.attr), attr_mod,
                           ptr<float>(c->ws.dens), attr_mod, N, cs, ok);
        *cself = cs;
        *cself_ok = ok;
        ++c->cself_tag;
    }
    return DRP_OK;
}

// scenes > 0 (a multi-scene session): nb = scenes * scene_nb columns, and the rewards read the goal of the row's scene
int run_rollout(drp_ctx* c, int nb, int N, int B, int H, bool reward_all, bool reward_last, bool session = false,
                int scenes = 0, int scene_nb = 1) {
    CHK(ensure_step_ws(c, c->ws, B, N));
    CHK(ensure(c, c->states, (size_t)B * H * N * 3 * sizeof(float)));
    CHK(ensure(c, c->rewards, (size_t)B * H * sizeof(float)));
    c->marks.lastH = H;
    float* states = ptr<float>(c->states);
    const size_t hstride = (size_t)H * N * 3;
    const float* cself = nullptr;
    const uint8_t* cself_ok = nullptr;
    // the self-edge constants depend on attributes and densities only: an MPC session computes them once (its first
    // rollout) and keeps them while nobody else has refilled the buffer
    if (session && c->mpc_cself_tag != 0 && c->mpc_cself_tag == c->cself_tag) {
        cself = c->mpc_cself;
        cself_ok = c->mpc_cself_ok;
    } else {
        CHK(prepare_cself(c, nb, N, B, &cself, &cself_ok));
        if (session) { c->mpc_cself_tag = c->cself_tag; c->mpc_cself = cself; c->mpc_cself_ok = cself_ok; }
    }
    // small piles on the fused engine: the whole rollout is ONE launch per block of samples (dispatch.h: plan_rollout)
    const RolloutPlan k = plan_rollout(c->pol, c->n_cu, c->engine, B, N, nb, c->work_ptr() != nullptr, c->deg());
    k.mark(c->marks.dv_hit);
    const bool one_launch = k.one_launch;
    if (one_launch) {
        const int n_chunks = k.blocks.n;
        std::vector<RolloutArgs> blocks((size_t)n_chunks);
        if (k.blocks.cache) CHK(ensure(c, c->ws.ecache, k.blocks.cache_bytes));
        for (int q = 0; q < n_chunks; ++q) {
            const Block b = k.blocks.block(q);
            const long b_off = b.b_off;
            const size_t ro = (size_t)b_off * N;
            RolloutArgs& ra = blocks[(size_t)q];
            ra = RolloutArgs{};
            ra.sw = ptr<uint16_t>(c->w_split); ra.sw6 = ptr<uint16_t>(c->w_split6); ra.mw = ptr<float>(c->w_mfma);
            // the first state, the attributes and the densities are replicated over the batch columns (row b reads column b % nb;
            // a block starts at a multiple of nb): same base for every block; everything indexed by the row moves on
            ra.s_in = ptr<float>(c->ws.s_in); ra.attr = ptr<float>(c->ws.attr); ra.dens = ptr<float>(c->ws.dens);
            ra.states = states + ro * 3 * H;
            ra.actions = ptr<float>(c->actions) + (size_t)b_off * H * 4;
            ra.s_delta = ptr<float>(c->ws.s_delta) + ro * 3; ra.nbr_idx = ptr<int16_t>(c->ws.nbr_idx) + ro * DRP_K;
            ra.nbr_cnt = ptr<uint8_t>(c->ws.nbr_cnt) + ro; ra.proj_a = ptr<float>(c->ws.proj) + ro * 128; ra.proj_b = ptr<float>(c->ws.proj2) + ro * 128;
            ra.c_node = ptr<float>(c->ws.c_node) + ro * 64; ra.eff = ptr<float>(c->ws.eff) + ro * 64;
            ra.cself = cself ? cself + (size_t)b_off * 64 : nullptr; ra.cself_ok = cself_ok ? cself_ok + b_off : nullptr;
            ra.N = N; ra.B = b.Bc; ra.spw = b.spw; ra.nb = nb; ra.H = H; ra.order_rows = (c->pol.prop3_order ? 1 : 0);
            ra.thr = c->thr; ra.re_scale = c->re_scale; ra.re_inv = c->re_inv; ra.cam = c->cam;
            ra.ec_stride = b.ec_stride;
            ra.ecache = k.blocks.cache ? ptr<float4>(c->ws.ecache) : nullptr;
            ra.work = c->work_ptr();
            if (ra.work) (k.lite ? c->work_lite : c->work_full) = true;
        }
        // the argument blocks sit in device memory; they are uploaded when they change (every iteration of an MPC session
        // passes the same ones), behind whatever still runs on the stream
        if (!c->roll_args_valid || c->roll_args_host.size() != blocks.size() ||
            memcmp(blocks.data(), c->roll_args_host.data(), blocks.size() * sizeof(RolloutArgs)) != 0) {
            c->roll_args_host = blocks;
            c->roll_args_valid = false;
            CHK(h2d(c, c->roll_args, c->roll_args_host.data(), blocks.size() * sizeof(RolloutArgs)));
            c->roll_args_valid = true;
        }
        ProbeScope ps(c, KC_PROP);
        for (int q = 0; q < n_chunks; ++q) {
            const Block b = k.blocks.block(q);
            hipLaunchKernelGGL(prop_tables().of(k.flags(b)), dim3((unsigned)b.grid), dim3(64 * PROP_WAVES), KM_ROLLOUT_LDS,
                               c->stream, ptr<RolloutArgs>(c->roll_args) + q);
            ps.launched();
        }
        HIPCHK(c, hipGetLastError());
        note_degrees(c, ptr<uint8_t>(c->ws.nbr_cnt), k.spw, N, B);           // the last step's lists
    }
    for (int t = 0; t < H && !one_launch; ++t) {
        StepArgs a = step_args(c, c->engine);
        a.cself = cself; a.cself_ok = cself_ok;
        if (t == 0) {
            a.s_prev = ptr<float>(c->ws.s_in); a.prev_mod = nb; a.prev_stride = (size_t)N * 3;
        } else {
            a.s_prev = states + (size_t)(t - 1) * N * 3; a.prev_mod = B; a.prev_stride = hstride;
        }
        a.attr = ptr<float>(c->ws.attr); a.attr_mod = nb;
        a.dens = ptr<float>(c->ws.dens); a.dens_mod = nb;
        a.actions = ptr<float>(c->actions) + (size_t)t * 4; a.act_stride = (size_t)H * 4;
        a.build_graph = true;
        a.s_out = states + (size_t)t * N * 3; a.out_stride = hstride;
        a.B = B; a.N = N;
        CHK(run_step(c, a));
    }
    if (reward_all) {
        // rows = B*H consecutive [N,3] blocks
        CHK(run_reward(c, states, (size_t)N * 3, B * H, N, 1, ptr<float>(c->rewards), scenes, scene_nb, H));
    } else if (reward_last) {
        // only the last step's state of every sample; written at rewards[b*H + H-1]
        CHK(ensure(c, c->scratch, (size_t)B * sizeof(float)));
        CHK(run_reward(c, states + (size_t)(H - 1) * N * 3, hstride, B, N, 1, ptr<float>(c->scratch), scenes, scene_nb, 1));
        HIPCHK(c, hipMemcpy2DAsync(ptr<float>(c->rewards) + (H - 1), H * sizeof(float), c->scratch.p,
                                   sizeof(float), sizeof(float), B, hipMemcpyDeviceToDevice, c->stream));
    }
    return DRP_OK;
}

void pack_valu(const float* w, std::vector<float>& v) {
    v.assign(V_TOTAL, 0.0f);
    auto T = [&](int dst, int src, int out, int in, int ld, int col0) {
        // dst[k][o] = w[src + o*ld + col0 + k]
        for (int o = 0; o < out; ++o)
            for (int k = 0; k < in; ++k) v[dst + k * 64 + o] = w[src + o * ld + col0 + k];
    };
    auto C = [&](int dst, int src, int n) { for (int i = 0; i < n; ++i) v[dst + i] = w[src + i]; };
    T(V_PE0_T, W_PE0_W, 64, 5, 5, 0);   C(V_PE0_B, W_PE0_B, 64);
    T(V_PE2_T, W_PE2_W, 64, 64, 64, 0); C(V_PE2_B, W_PE2_B, 64);
    T(V_PPE_T, W_PP_W, 64, 64, 129, 0);
    for (int o = 0; o < 64; ++o) v[V_PP_WD + o] = w[W_PP_W + o * 129 + 128];
    C(V_PP_B, W_PP_B, 64);
    T(V_AGG_T, W_PP_W, 64, 64, 129, 64);
    T(V_RE0_T, W_RE0_W, 64, 6, 6, 0);   C(V_RE0_B, W_RE0_B, 64);
    T(V_RE2_T, W_RE2_W, 64, 64, 64, 0); C(V_RE2_B, W_RE2_B, 64);
    T(V_RE4_T, W_RE4_W, 64, 64, 64, 0); C(V_RE4_B, W_RE4_B, 64);
    T(V_RPE_T, W_RP_W, 64, 64, 193, 0);
    for (int o = 0; o < 64; ++o) v[V_RP_WD + o] = w[W_RP_W + o * 193 + 192];
    C(V_RP_B, W_RP_B, 64);
    T(V_RPR_T, W_RP_W, 64, 64, 193, 64);
    T(V_RPS_T, W_RP_W, 64, 64, 193, 128);
    T(V_PR0_T, W_PR0_W, 64, 64, 64, 0); C(V_PR0_B, W_PR0_B, 64);
    C(V_PR1_W, W_PR1_W, 192);
    C(V_PR1_B, W_PR1_B, 3);
}

int need(drp_ctx* c, bool weights, bool cam, bool goal) {
    if (!c) return DRP_EINVAL;
    if (weights && !c->have_weights) return fail(c, DRP_ESTATE, "weights not loaded (drp_load_weights)");
    if (cam && !c->have_cam) return fail(c, DRP_ESTATE, "camera not set (drp_set_camera)");
    if (goal && !c->have_goal) return fail(c, DRP_ESTATE, "goal not set (drp_set_goal)");
    return DRP_OK;
}

// Weight-gradient jobs are queued and go out together (flush): one pair of launches for all the jobs whose inputs exist at
// that point of the stream.  flush() must run before a kernel overwrites a queued job's g or x.
// DEFERRED weight gradients (training, DRP_NO_WGRAD_DEFER=1 turns it off): every operand of an iteration's jobs keeps a
// buffer of its own (per rollout step, per propagation step), the jobs queue up for the whole backward pass and go out
// in a handful of launches at its end (flush_all) instead of 25 pairs in between.  The mode is fixed for a pass by begin().
struct WgradQueue {
    drp_ctx* const c;
    std::vector<WgradJob> wg_jobs;              // waiting for the next flush
    bool defer = false;
    DevBuf wg_jobs_dev, wg_idx_dev;             // flush_all's jobs and lists on the device
    std::vector<unsigned char> wg_uploaded;     // what they hold (re-uploaded when the iteration's jobs change)
    DevBuf tr_part;                             // the jobs' partial sums
    // read-only tap of the last flush_all (capi_debug.h: "train_wgrad_*", valid while c->wgrad_tap_on): the jobs in queue order,
    // the one kt_colsum3 call beside them, the gradient blob the targets point into and the densities the jobs read
    std::vector<WgradJob> tap_jobs;
    const float* tap_G = nullptr; const float* tap_cs_g = nullptr; const float* tap_dens = nullptr;
    long tap_cs_M = 0; int tap_dens_n = 0;
    explicit WgradQueue(drp_ctx* ctx) : c(ctx) {}
    void begin(bool defer_pass) { wg_jobs.clear(); defer = defer_pass; }
    template <int IN>
    void push(const float* g, int ldg, const float* x, int ldx, long M, float* dW, int lane_stride, int k_stride, float* db,
              float* dwd, const float* dens, int dens_mod, long rows_per_sample) {
        long blocks = (M + 63) / 64;
        if (blocks > KT_WGRAD_MAX_BLOCKS) blocks = KT_WGRAD_MAX_BLOCKS;
        if (blocks < 1) blocks = 1;
        if ((int)wg_jobs.size() == KT_WGRAD_MAX_JOBS) flush();
        WgradJob q{};
        q.g = g; q.x = x; q.dW = dW; q.db = db; q.dwd = dwd; q.dens = dens; q.part = nullptr;
        q.M = M; q.rows_per_sample = rows_per_sample;
        q.ldg = ldg; q.ldx = ldx; q.lane_stride = lane_stride; q.k_stride = k_stride; q.dens_mod = dens_mod; q.in = IN;
        q.blocks = (int)blocks;
        wg_jobs.push_back(q);
    }
    // the queued jobs now -- unless the pass defers them: then they wait for flush_all
    void flush() {
        const int n = (int)wg_jobs.size();
        if (n == 0 || defer) return;
        WgradJobs J{};
        int max_blocks = 1;
        for (int q = 0; q < n; ++q) {
            J.j[q] = wg_jobs[q];
            J.j[q].part = static_cast<float*>(tr_part.p) + (size_t)q * KT_WGRAD_MAX_BLOCKS * 66 * 64;
            if (J.j[q].blocks > max_blocks) max_blocks = J.j[q].blocks;
        }
        c->dv(c->pol.wgrad_mfma ? DV_WGRAD_MFMA : DV_WGRAD_VALU);
        if (c->pol.wgrad_mfma)
            hipLaunchKernelGGL(kt_wgrad_mfma_multi, dim3((unsigned)max_blocks, (unsigned)n), dim3(256), KT_WGRAD_MULTI_LDS, c->stream, J);
        else
            hipLaunchKernelGGL(kt_wgrad_multi, dim3((unsigned)max_blocks, (unsigned)n), dim3(256), KT_WGRAD_MULTI_LDS, c->stream, J);
        hipLaunchKernelGGL(kt_wgrad_reduce_multi, dim3(66, (unsigned)n), dim3(256), 0, c->stream, J);
        wg_jobs.clear();
    }
    // The deferred jobs of a whole backward pass, as planned (dispatch.h: plan_wgrad_lists).  Jobs of one size go through one
    // launch (blockIdx.y walks that size's slice of `order`); then ONE reduction launch in which a block owns a target dW and
    // adds its jobs' sums in queue order -- what the in-between flushes did launch after launch, so the gradients keep their bits.
    int flush_all() {
        const int n = (int)wg_jobs.size();
        if (n == 0) return DRP_OK;
        std::vector<int> blocks(n);
        std::vector<const void*> target(n);
        for (int q = 0; q < n; ++q) { blocks[q] = wg_jobs[q].blocks; target[q] = wg_jobs[q].dW; }
        const WgradListPlan k = plan_wgrad_lists(blocks, target);
        CHK(ensure(c, tr_part, std::max(k.part_floats, (size_t)KT_WGRAD_MAX_JOBS * KT_WGRAD_MAX_BLOCKS * 66 * 64) * sizeof(float)));
        for (int q = 0; q < n; ++q) wg_jobs[q].part = static_cast<float*>(tr_part.p) + k.part_off[q];
        // upload when anything changed (the same shape queues the same jobs iteration after iteration)
        const size_t jb = (size_t)n * sizeof(WgradJob), ib = k.idx.size() * sizeof(int);
        std::vector<unsigned char> img(jb + ib);
        memcpy(img.data(), wg_jobs.data(), jb);
        memcpy(img.data() + jb, k.idx.data(), ib);
        if (img != wg_uploaded) {
            wg_uploaded.swap(img);                  // the copies' source stays alive in the queue
            CHK(h2d(c, wg_jobs_dev, wg_uploaded.data(), jb));
            CHK(h2d(c, wg_idx_dev, wg_uploaded.data() + jb, ib));
        }
        c->dv(DV_WGRAD_DEFERRED);
        c->dv(c->pol.wgrad_mfma ? DV_WGRAD_MFMA : DV_WGRAD_VALU);
        const WgradJob* jd = static_cast<const WgradJob*>(wg_jobs_dev.p);
        const int* od = static_cast<const int*>(wg_idx_dev.p);
        for (int a = 0; a < n;) {
            int b = a;
            while (b < n && blocks[k.order[b]] == blocks[k.order[a]]) ++b;
            const dim3 grid((unsigned)blocks[k.order[a]], (unsigned)(b - a));
            if (c->pol.wgrad_mfma) hipLaunchKernelGGL(kt_wgrad_mfma_list, grid, dim3(256), KT_WGRAD_MULTI_LDS, c->stream, jd, od, a);
            else hipLaunchKernelGGL(kt_wgrad_list, grid, dim3(256), KT_WGRAD_MULTI_LDS, c->stream, jd, od, a);
            a = b;
        }
        hipLaunchKernelGGL(kt_wgrad_reduce_lists, dim3(66, (unsigned)k.n_targets), dim3(256), 0, c->stream, jd, od + n, od + n + k.n_targets + 1);
        tap_jobs.swap(wg_jobs);                     // (the tap keeps them; nothing is copied)
        wg_jobs.clear();
        HIPCHK(c, hipGetLastError());
        return DRP_OK;
    }
};

// Kernels of the planner's and the trainer's entry points read and write pinned host memory (the staged batch, the results' slots).
// Constructed before the first such launch and disarmed by the DRP_OK return (ok()), this waits for the stream on every other way
// out: no call returns with work of its own in flight.  The caller still sees the first failure's text, not the wait's.
struct DrainOnError {
    drp_ctx* c;
    bool armed = true;
    explicit DrainOnError(drp_ctx* ctx) : c(ctx) {}
    ~DrainOnError() {
        if (!armed) return;
        std::string first = std::move(c->err);
        (void)guarded_wait(c, nullptr);
        c->err = std::move(first);
    }
    int ok() { armed = false; return DRP_OK; }
};

// ---- reverse mode, shared by the gradient-descent planner (capi_gd.h) and the trainer (capi_train.h) ------------------

// the tape of H steps of B x N and the backward pass's buffers, sized alike for both; `rev_sets` steps' reversed lists
// (the planner builds them step by step, the trainer all at once)
int ensure_tape(drp_ctx* c, int B, int N, int H, int rev_sets) {
    const size_t bn = (size_t)B * N;
    CHK(ensure(c, c->eff_hist, (size_t)H * 4 * bn * 64 * sizeof(float)));
    CHK(ensure(c, c->tape_sdelta, (size_t)H * bn * 3 * sizeof(float)));
    CHK(ensure(c, c->tape_idx, (size_t)H * bn * DRP_K * sizeof(int16_t)));
    CHK(ensure(c, c->tape_cnt, (size_t)H * bn));
    CHK(ensure(c, c->tape_mask, (size_t)H * DRP_PSTEP * bn * DRP_K * 2 * sizeof(unsigned)));
    CHK(ensure(c, c->g_agg_hist, (size_t)DRP_PSTEP * bn * 64 * sizeof(float)));
    CHK(ensure(c, c->rev_off, (size_t)rev_sets * B * (N + 1) * sizeof(int)));
    CHK(ensure(c, c->rev, (size_t)rev_sets * bn * DRP_K * sizeof(int)));
    CHK(ensure(c, c->gpos_edge, bn * DRP_K * 4 * sizeof(float)));
    CHK(ensure(c, c->g_sdelta, bn * 3 * sizeof(float)));
    return DRP_OK;
}

// The forward pass of H steps on `engine` into c->states.  Step t's impulses are tape_sdelta's slice t; with `tape` its
// neighbour lists are the tape's slices too (StepArgs names the slices: nothing is copied afterwards), and km_prop<., TAPE> leaves beside them what the backward pass needs: the effect after the encoder
// and after every propagation step, the ReLU masks of the edges, with `agg_hist` the aggregated edge effects.
struct TapeFwd {
    const float* s0; int s0_mod; size_t s0_stride;   // the first step's input; the later steps read the step before's output
    int mod;                                         // attributes and densities: sample b reads row b % mod
    const float* actions;                            // [B][H][4], or null: the impulses are data, already in tape_sdelta
    const float* masked_actions = nullptr;           // the trainer's pushes [B][H][4] (with `actions` null): a launch ahead of each step
    const int* nums = nullptr;                       //   writes tape_sdelta's slice from the step's input, zeros on rows >= nums[b]
    bool padded;
    bool tape;                                       // false: the forward pass alone
    bool agg_hist;
    const float* cself; const uint8_t* cself_ok;
    int* rev_off = nullptr; int* rev = nullptr;      // horizon 1: the reversed lists in the lists' own launch where it can
    bool* rev_built = nullptr;                       //   (StepArgs)
};
int run_tape_forward(drp_ctx* c, int engine, int B, int N, int H, const TapeFwd& f) {
    const size_t bn = (size_t)B * N, hstride = (size_t)H * N * 3;
    float* states = ptr<float>(c->states);
    for (int t = 0; t < H; ++t) {
        StepArgs a = step_args(c, engine);
        if (t == 0) { a.s_prev = f.s0; a.prev_mod = f.s0_mod; a.prev_stride = f.s0_stride; }
        else { a.s_prev = states + (size_t)(t - 1) * N * 3; a.prev_mod = B; a.prev_stride = hstride; }
        a.attr = ptr<float>(c->ws.attr); a.attr_mod = f.mod;
        a.dens = ptr<float>(c->ws.dens); a.dens_mod = f.mod;
        if (f.actions) { a.actions = f.actions + (size_t)t * 4; a.act_stride = (size_t)H * 4; }
        a.build_graph = true;
        a.s_out = states + (size_t)t * N * 3; a.out_stride = hstride;
        a.B = B; a.N = N;
        a.cself = f.cself; a.cself_ok = f.cself_ok;
        a.padded = f.padded;
        a.rev_off = f.rev_off; a.rev = f.rev; a.rev_built = f.rev_built;
        a.s_delta = ptr<float>(c->tape_sdelta) + (size_t)t * bn * 3;
        if (f.masked_actions)           // the step itself reads the slice as it reads data impulses: the graph kernels' push path knows no padding
            hipLaunchKernelGGL(kt_sdelta_actions, dim3(B), dim3(256), 0, c->stream, a.s_prev, a.prev_stride, f.masked_actions + (size_t)t * 4,
                               (size_t)H * 4, f.nums, N, a.s_delta, c->cam);
        if (f.tape) {
            a.nbr_idx = ptr<int16_t>(c->tape_idx) + (size_t)t * bn * DRP_K;
            a.nbr_cnt = ptr<uint8_t>(c->tape_cnt) + (size_t)t * bn;
            a.eff_hist = ptr<float>(c->eff_hist) + (size_t)t * 4 * bn * 64;
            a.mask_hist = ptr<unsigned>(c->tape_mask) + (size_t)t * DRP_PSTEP * bn * DRP_K * 2;
            if (f.agg_hist) a.agg_hist = ptr<float>(c->agg_hist) + (size_t)t * 3 * bn * 64;
        }
        CHK(run_step(c, a));
    }
    return DRP_OK;
}

// the reversed lists of `sets` samples' neighbour lists into rev_off / rev, a workgroup each; `nums` (nullable): the
// particle counts, set s reading nums[s % nums_mod] (0: nums[s])
void launch_reverse_lists(drp_ctx* c, const int16_t* idx, const uint8_t* cnt, int N, int sets, const int* nums, int nums_mod) {
    const bool rev_lds = N <= KB_REV_LDS_MAX_N && !c->pol.rev_global_only;
    ProbeScope ps(c, KC_BWD_LISTS);
    c->dv(N <= 512 ? DV_REV_256 : DV_REV_1024);
    if (N <= 512)
        hipLaunchKernelGGL(kb_reverse_lists<256>, dim3(sets), dim3(256), KB_REV_LDS(N, rev_lds), c->stream, idx, cnt, N,
                           ptr<int>(c->rev_off), ptr<int>(c->rev), rev_lds ? 1 : 0, nums, nums_mod);
    else
        hipLaunchKernelGGL(kb_reverse_lists<1024>, dim3(sets), dim3(1024), KB_REV_LDS(N, rev_lds), c->stream, idx, cnt, N,
                           ptr<int>(c->rev_off), ptr<int>(c->rev), rev_lds ? 1 : 0, nums, nums_mod);
}

// one rollout step of the backward pass, as its node stages read and write it
struct BwdStep {
    int B, N;
    int mod;                        // attributes and densities: sample b reads row b % mod
    const float* eht;               // the step's tape: effects [4][B*N][64], ReLU masks [3][B*N*10][2], neighbour counts
    const unsigned* mht;
    const uint8_t* cnt;
    const int* rev_off; const int* rev;
    const float* sdelta;            // the step's impulses [B*N][3]
    const float* g_out;             // d loss / d the step's output state [B][N*3]
    float* gah;                     // g_agg of the three propagation steps [3][B*N][64]
    float* ge_tmp;                  // the predictor's gradient, which the particle encoder's reads
    float* g_cnode;
    KmbDump d;                      // d.ge / d.gp: the propagation steps' pre-activation gradients and edge terms (one buffer for
                                    // all of them, or one each for the trainer's deferred weight gradients); the dumps for the
                                    // weight gradients, null for none
};

// The trainer's weight-gradient jobs of a rollout step's node stages, each to be queued once its operands exist: behind
// the predictor; per propagation step p = 2, 1, 0 behind its update and behind its edge terms; behind the last update;
// behind the particle encoder
struct NodeWgrad {
    WgradQueue& wq;
    float* G;                       // the gradient blob
    const float* aht;               // the step's aggregated edge effects [3][B*N][64]
    const float* dens;
    void predictor(const BwdStep& s) const {
        const size_t bn = (size_t)s.B * s.N;
        wq.push<64>(s.d.gh, 64, s.eht + 3 * bn * 64, 64, (long)bn, G + W_PR0_W, 64, 1, G + W_PR0_B, nullptr, nullptr, 1, 1);
        wq.push<3>(s.d.hact, 64, s.g_out, 3, (long)bn, G + W_PR1_W, 1, 64, nullptr, nullptr, nullptr, 1, 1);
    }
    void update(const BwdStep& s, int p) const {       // particle propagator, aggregate columns
        const size_t bn = (size_t)s.B * s.N;
        wq.push<64>(s.d.ge[DRP_PSTEP - 1 - p], 64, aht + (size_t)p * bn * 64, 64, (long)bn, G + W_PP_W + 64, 129, 1,
                        nullptr, nullptr, nullptr, 1, 1);
    }
    void edge_terms(const BwdStep& s, int p) const {   // relation propagator, receiver and sender columns
        const size_t bn = (size_t)s.B * s.N;
        wq.push<64>(s.d.gp[p], 128, s.eht + (size_t)p * bn * 64, 64, (long)bn, G + W_RP_W + 64, 193, 1,
                        nullptr, nullptr, nullptr, 1, 1);
        wq.push<64>(s.d.gp[p] + 64, 128, s.eht + (size_t)p * bn * 64, 64, (long)bn, G + W_RP_W + 128, 193, 1,
                        nullptr, nullptr, nullptr, 1, 1);
    }
    void cnode(const BwdStep& s) const {               // particle propagator, encoder columns + density column + bias
        const size_t bn = (size_t)s.B * s.N;
        wq.push<64>(s.g_cnode, 64, s.eht, 64, (long)bn, G + W_PP_W, 129, 1, G + W_PP_B, G + W_PP_W + 128, dens, s.B,
                        (long)s.N);
    }
    void encoder(const BwdStep& s) const {             // particle encoder
        const size_t bn = (size_t)s.B * s.N;
        wq.push<64>(s.d.gpe, 64, s.d.a1n, 64, (long)bn, G + W_PE2_W, 64, 1, G + W_PE2_B, nullptr, nullptr, 1, 1);
        wq.push<5>(s.d.gh1, 64, s.d.xn, 8, (long)bn, G + W_PE0_W, 5, 1, G + W_PE0_B, nullptr, nullptr, 1, 1);
    }
};

// The node stages of a rollout step's backward pass, a launch per stage on the matrix cores: the predictor, the update of
// the last propagation step, then per propagation step the edge terms (kb_edge_terms on `egrid`, `chunks` workgroups per
// sample) and in one launch the projection of this step with the update of the one before, the particle encoder.
// `wg` (nullable): weight-gradient jobs to queue in between.
void launch_node_stages(drp_ctx* c, const BwdStep& s, dim3 egrid, int chunks, const NodeWgrad* wg) {
    hipStream_t st = c->stream;
    const int B = s.B, N = s.N;
    const size_t bn = (size_t)B * N, bn64 = bn * 64;
    const KmbDump& d = s.d;
    const float* mw = ptr<float>(c->w_mfma);
    const float* mb = ptr<float>(c->w_mfma_bwd);
    const dim3 ngrid(mfma_grid_spread(c, (long)B * ((N + 31) / 32))), nblk(64 * MFMA_WAVES);
    { ProbeScope ps(c, KC_BWD_NODE);
    hipLaunchKernelGGL(kmb_predict, ngrid, nblk, KMB_PREDICT_LDS, st, mw, mb, s.eht + 3 * bn64, s.g_out, (size_t)N * 3, N, B,
                       s.ge_tmp, d.hact, d.gh);
    }
    if (wg) wg->predictor(s);
    { ProbeScope ps(c, KC_BWD_NODE);
    hipLaunchKernelGGL((kmb_node_step<false, true>), ngrid, nblk, KMB_STEP_LDS(false, true), st, mb, s.ge_tmp, d.ge[0],
                       (const float*)nullptr, s.eht + (size_t)DRP_PSTEP * bn64, s.g_cnode, 1, s.gah + (size_t)(DRP_PSTEP - 1) * bn64, N, B);
    }
    for (int p = DRP_PSTEP - 1; p >= 0; --p) {
        if (wg) wg->update(s, p);
        { ProbeScope ps(c, KC_BWD_EDGE);
        hipLaunchKernelGGL(kb_edge_terms, egrid, dim3(256), 0, st, s.gah + (size_t)p * bn64, s.mht + (size_t)p * bn * DRP_K * 2,
                           s.cnt, s.rev_off, s.rev, N, d.gp[p], chunks);
        }
        if (wg) {
            wg->edge_terms(s, p);
            wg->wq.flush();                              // (not deferred:) before the next kernel overwrites g_eff (and, next step, g_proj)
        }
        ProbeScope ps(c, KC_BWD_NODE);
        if (p > 0)
            hipLaunchKernelGGL((kmb_node_step<true, true>), ngrid, nblk, KMB_STEP_LDS(true, true), st, mb, d.ge[DRP_PSTEP - 1 - p],
                               d.ge[DRP_PSTEP - p], d.gp[p], s.eht + (size_t)p * bn64, s.g_cnode, 0, s.gah + (size_t)(p - 1) * bn64, N, B);
        else
            hipLaunchKernelGGL((kmb_node_step<true, false>), ngrid, nblk, KMB_STEP_LDS(true, false), st, mb, d.ge[DRP_PSTEP - 1],
                               s.ge_tmp, d.gp[0], (const float*)nullptr, (float*)nullptr, 0, (float*)nullptr, N, B);
    }
    if (wg) wg->cnode(s);
    { ProbeScope ps(c, KC_BWD_NODE);
    hipLaunchKernelGGL(kmb_node_encode, ngrid, nblk, KMB_NODE_ENCODE_LDS, st, mw, mb, s.sdelta, ptr<float>(c->ws.attr), s.mod,
                       ptr<float>(c->ws.dens), s.mod, s.eht, s.ge_tmp, s.g_cnode, N, B, ptr<float>(c->g_sdelta), d.gpe, d.a1n, d.gh1, d.xn);
    }
    if (wg) {
        wg->encoder(s);
        wg->wq.flush();
    }
}

// The one-shot entry points stage their inputs in the buffers the planner sessions keep their state in
// (s_in, attr, dens, actions, states): a session interrupted by one of them is over -- its next call returns
// DRP_ESTATE instead of results computed from overwritten inputs.
void end_sessions(drp_ctx* c) {
    c->mpc_on = false;
    c->gd_on = false;
    for (int q = 0; q < DRP_GD_SLOTS; ++q) c->gd_pending[q] = false;
    c->mpc_pending[0] = c->mpc_pending[1] = false;
}

// The split relation encoder's range shift was proven for an envelope of inputs (drp_load_weights); a call
// whose attributes, densities or impulses leave it is refused instead of risking a saturated fp16 piece.
float max_abs(const float* p, size_t n) {
    float m = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        const float v = fabsf(p[i]);
        if (v > m || v != v) m = (v != v) ? INFINITY : v;
    }
    return m;
}
// largest |s_delta| a push can cause (planners.py:238-254: the impulse is at most the push's own length in the
// camera frame): actions [n][4] = (sx, sy, ex, ey) in world units
float push_len_bound(const drp_ctx* c, const float* actions, size_t n) {
    // spectral norm of the world -> camera map's 3x3 part (1 for the rotation a camera is; the Frobenius norm used
    // until round 2 is sqrt(3) too large, which put the DEFAULT clip box outside the proven envelope): sqrt of the
    // largest eigenvalue of M^T M
    double A[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double v = 0.0;
            for (int k = 0; k < 3; ++k) v += (double)c->cam.m[k * 4 + i] * (double)c->cam.m[k * 4 + j];
            A[i][j] = v;
        }
    // largest eigenvalue of the symmetric 3x3 in closed form (the trigonometric solution of its cubic): an upper bound of
    // the impulse must not come from an iteration that converges from BELOW (a map with two close singular values)
    double lam;
    const double p1 = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double q = (A[0][0] + A[1][1] + A[2][2]) / 3.0;
    if (p1 == 0.0) {
        lam = fmax(A[0][0], fmax(A[1][1], A[2][2]));
    } else {
        const double p2 = (A[0][0] - q) * (A[0][0] - q) + (A[1][1] - q) * (A[1][1] - q) + (A[2][2] - q) * (A[2][2] - q) + 2.0 * p1;
        const double p = sqrt(p2 / 6.0);
        double Bm[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Bm[i][j] = (A[i][j] - (i == j ? q : 0.0)) / p;
        double r = 0.5 * (Bm[0][0] * (Bm[1][1] * Bm[2][2] - Bm[1][2] * Bm[2][1]) - Bm[0][1] * (Bm[1][0] * Bm[2][2] - Bm[1][2] * Bm[2][0]) +
                          Bm[0][2] * (Bm[1][0] * Bm[2][1] - Bm[1][1] * Bm[2][0]));
        r = fmin(1.0, fmax(-1.0, r));
        lam = q + 2.0 * p * cos(acos(r) / 3.0);
    }
    // rounding slack of the formula, never above the Frobenius norm (itself a bound)
    const double frob = sqrt(A[0][0] + A[1][1] + A[2][2]);
    const float fro = (float)fmin(frob, sqrt(fmax(lam, 0.0)) * (1.0 + 1e-6));
    float l2 = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        const float dx = actions[i * 4 + 2] - actions[i * 4 + 0], dy = actions[i * 4 + 3] - actions[i * 4 + 1];
        const float v = dx * dx + dy * dy;
        if (v > l2 || v != v) l2 = (v != v) ? INFINITY : v;
    }
    return fro * sqrtf(l2) / c->cam.gs;
}
// the trainer's pushes [B][H][4] (drp_train_step_actions, drp_train_grad_f64_actions): one of zero length, or of none, is refused
// (train_host.h: first_bad_push)
int check_pushes(drp_ctx* c, const float* actions, int B, int H) {
    float len = 0.0f;
    const long e = first_bad_push(c->cam.m, c->cam.gs, actions, (size_t)B * H, &len);
    if (e >= 0) return fail(c, DRP_EINVAL, "actions[%d][%d]: a push of length %g", (int)(e / H), (int)(e % H), (double)len);
    return DRP_OK;
}
// engine: the one the caller runs (the gradient-descent planner's and the trainer's forward pass write their tape with the
// fused one whatever drp_set_engine chose)
int range_check(drp_ctx* c, int engine, float max_attr, float max_dens, float max_sdelta) {
    if (!engine_is_fused(engine) && engine != DRP_ENGINE_SPLIT) return DRP_OK;
    const double A = max_attr, dm = max_dens / DRP_DENS_SCALE, D = c->adj_thresh + 2.0 * max_sdelta;
    const SplitRange& r = c->re_range;
    if (!c->re_ok)
        return fail(c, DRP_ERANGE, "weights outside the range of the split-fp16 relation encoder (largest |w| %g, activation "
                    "bound %g, shift %d): use DRP_ENGINE_MFMA", (double)r.wmax, split_range_bound(r, r.env_attr, r.env_delta, r.env_dens), r.shift);
    if (A <= r.env_attr && dm <= r.env_dens && D <= r.env_delta) return DRP_OK;
    const double bound = split_range_bound(r, A, D, dm);
    if (ldexp(bound, r.shift) <= 65504.0) return DRP_OK;       // outside the envelope, still provably inside fp16
    return fail(c, DRP_ERANGE, "inputs beyond the range the split-fp16 relation encoder is scaled for (max |attr| %g, "
                "density %g, |s_delta| %g; activation bound %g x 2^%d): use DRP_ENGINE_MFMA for this call",
                A, (double)max_dens, (double)max_sdelta, bound, r.shift);
}

// Which engine writes the tape of the gradient-descent planner / the trainer: the fused one (km_prop<., TAPE>) unless the
// caller has selected an fp32 engine (drp_set_engine) or the split-fp16 relation encoder would refuse these weights or
// inputs -- then the fp32 matrix engine's stage kernels with k_aggregate_tape: several times slower, no range limit.  The
// live planner of the reference IS the gradient-descent one (env/flex_env.py:973-976): it must not stop on DRP_ERANGE.
int pick_tape_engine(drp_ctx* c, float max_attr, float max_dens, float max_sdelta, int* engine) {
    if (c->engine == DRP_ENGINE_MFMA || c->engine == DRP_ENGINE_VALU) { *engine = DRP_ENGINE_MFMA; return DRP_OK; }
    const int rc = range_check(c, DRP_ENGINE_FUSED, max_attr, max_dens, max_sdelta);
    if (rc == DRP_ERANGE) { *engine = DRP_ENGINE_MFMA; c->err.clear(); return DRP_OK; }
    *engine = DRP_ENGINE_FUSED;
    return rc;
}

// range shift of the split relation encoder: proven for |attr| <= 2 (the reference's are 0), |s_r - s_s| <= 1.5
// per coordinate (radius 0.08 + two impulses; the default clip box's longest push is 8.5 sqrt(2) / 24 = 0.50
// camera-frame units, the whole workspace diagonal 0.59: 0.08 + 2 x 0.59 = 1.26), density <= 10 000 (training
// range: 15 .. 6 500); calls beyond are re-checked one by one (range_check)
void set_split_range(drp_ctx* c, const float* blob) {
    split_range_init(blob, c->re_range, SPLIT_ENV_ATTR, SPLIT_ENV_DELTA, SPLIT_ENV_DENS);
    if (c->re_shift_env != 0x7fffffff) c->re_range.shift = c->re_shift_env;
    // weights no shift can carry (a matrix entry beyond fp16, NaN): the split engines refuse every call
    // (range_check); the fp32 engines are unaffected
    c->re_ok = c->re_range.finite && c->re_range.wmax < 6.0e4f &&
               ldexp(split_range_bound(c->re_range, 2.0, 1.5, 2.0), c->re_range.shift) <= 65504.0;
    c->re_scale = ldexpf(1.0f, c->re_range.shift);
    c->re_inv = ldexpf(1.0f, -c->re_range.shift);
}

// the float64 copy of the weights (k_prop_f64.h) from the device's current fp32 blob: enqueued, not waited for
int f64_refresh_weights(drp_ctx* c) {
    CHK(ensure(c, c->f64_w, (size_t)KF_W_ALL * sizeof(double)));
    hipLaunchKernelGGL(kf_widen_weights, dim3((KF_W_ALL + 255) / 256), dim3(256), 0, c->stream, ptr<float>(c->w_raw), ptr<double>(c->f64_w));
    HIPCHK(c, hipGetLastError());
    c->f64_w_valid = true;
    return DRP_OK;
}

int check_bn(drp_ctx* c, int B, int N) {
    if (B <= 0 || N <= 0 || N > 4096) return fail(c, DRP_EINVAL, "bad shape B=%d N=%d (N <= 4096)", B, N);
    return DRP_OK;
}

// ---- a one-shot on two clouds: checks, staging, copies back --------------------------------------------------------------
// One buffer for the three of them (c->cloud_io; train_host.h: CloudLayout): every call ends in a wait, keeps nothing, and reads
// back only blocks its own kernel wrote.  No weights, no session begun or ended, nothing of the engine, the dispatch marks or the
// trainer touched.

// the arguments every one of them refuses, in this order (p: floats, or drp_cloud_divergence_f64's doubles); n_cap: the cap on N beyond check_bn's (0: none), `what`: the caps' suffix
int cloud_check(drp_ctx* c, const void* p, const int32_t* n_p, const float* q, const int32_t* n_q, int B, int N, int M,
                const double* terms_out, int n_cap, int m_cap, const char* what) {
    if (!c) return DRP_EINVAL;
    CHK(check_bn(c, B, N));
    if (n_cap > 0 && N > n_cap) return fail(c, DRP_EINVAL, "bad shape N=%d (1..%d%s)", N, n_cap, what);
    if (M <= 0 || M > m_cap) return fail(c, DRP_EINVAL, "bad shape M=%d (1..%d%s)", M, m_cap, what);
    if (!p || !n_p || !q || !n_q || !terms_out) return fail(c, DRP_EINVAL, "null argument");
    for (int b = 0; b < B; ++b) {
        if (n_p[b] <= 0 || n_p[b] > N) return fail(c, DRP_EINVAL, "n_p[%d]=%d outside 1..%d", b, n_p[b], N);
        if (n_q[b] <= 0 || n_q[b] > M) return fail(c, DRP_EINVAL, "n_q[%d]=%d outside 1..%d", b, n_q[b], M);
    }
    return DRP_OK;
}

struct CloudCall {
    CloudLayout lay{};
    void* const* outs = nullptr;    // the caller's arrays, one per block of lay.out (null: not asked for)
    std::vector<char> stage;        // the inputs as uploaded: read until cloud_finish's wait
    char* io = nullptr;             // c->cloud_io
    CloudPair cp{};                 // the pair on the device, step strides 0
    const void* p_dev = nullptr;    // p's rows there: lay.p_elem bytes an element
    template <typename T>
    const T* p() const { return static_cast<const T*>(p_dev); }
    // block k on the device for the kernel to write, null where the caller did not ask for it
    template <typename T>
    T* out(int k) const { return outs[k] ? reinterpret_cast<T*>(io + lay.out[k]) : nullptr; }
};
// the inputs staged and on their way up, the view filled
int cloud_begin(drp_ctx* c, CloudCall& k, const CloudLayout& lay, void* const* outs, const void* p, const int32_t* n_p,
                const float* q, const int32_t* n_q, int B, int N, int M) {
    HIPCHK(c, hipSetDevice(c->device));
    k.lay = lay; k.outs = outs;
    CHK(ensure(c, c->cloud_io, lay.bytes));
    k.stage.resize(lay.in_bytes);
    memcpy(k.stage.data() + lay.pts_p, p, (size_t)B * N * 3 * lay.p_elem);
    memcpy(k.stage.data() + lay.pts_q, q, (size_t)B * M * 3 * sizeof(float));
    memcpy(k.stage.data() + lay.n_p, n_p, (size_t)B * sizeof(int));
    memcpy(k.stage.data() + lay.n_q, n_q, (size_t)B * sizeof(int));
    CHK(h2d(c, c->cloud_io, k.stage.data(), lay.in_bytes));
    k.io = ptr<char>(c->cloud_io);
    k.p_dev = k.io + lay.pts_p;
    k.cp.p_bstride = (size_t)N * 3; k.cp.p_tstride = 0;
    k.cp.q = reinterpret_cast<const float*>(k.io + lay.pts_q); k.cp.q_bstride = (size_t)M * 3; k.cp.q_tstride = 0;
    k.cp.n_p = reinterpret_cast<const int*>(k.io + lay.n_p);
    k.cp.n_q = reinterpret_cast<const int*>(k.io + lay.n_q); k.cp.nq_bstride = 1; k.cp.nq_tstride = 0;
    k.cp.N = N; k.cp.M = M;
    return DRP_OK;
}
// behind the launch of `kernel`: every block asked for comes back, then the wait
int cloud_finish(drp_ctx* c, const CloudCall& k, const char* kernel) {
    if (hipGetLastError() != hipSuccess) { (void)drp_sync(c); return fail(c, DRP_EHIP, "%s launch", kernel); }   // (the staging vector is still being read)
    int rc = DRP_OK;
    for (int b = 0; b < k.lay.n_out; ++b)
        if (rc == DRP_OK && k.outs[b]) rc = d2h(c, k.outs[b], k.io + k.lay.out[b], k.lay.out_bytes[b]);
    const int rw = guarded_wait(c, nullptr);            // also on an error above: the staging vector goes out of scope
    return rc != DRP_OK ? rc : rw;
}

}  // namespace
