// dispatch.h -- which kernel serves a call and how a batch is cut, decided on the host by pure functions.
// Nothing here touches HIP: the header compiles on its own with a plain C++17 compiler (tests/test_dispatch_plan.py does
// that and runs the plan functions without a GPU).  It holds
//   * DispatchPolicy: every threshold and switch that influences the choice, with the measurement behind it;
//   * policy_from_env(): the ONE table of the DRP_* environment switches that set them (DESIGN_NOTES.md 9c is held equal to it);
//   * the variant names (DispatchVariant, dv_name) and the template flags of km_prop / km_prop3 / km_rollout with their index;
//   * plan_graph / plan_step / plan_rollout / plan_backward / plan_train_backward: shapes in, plain structs out.
// The launch sites (capi_pipeline.h, capi_gd.h, capi_train.h) ask for a plan at their top and carry it out.
#ifndef DRP_DISPATCH_H
#define DRP_DISPATCH_H
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

namespace dispatch {

// constants of the kernels the plans depend on (capi_ctx.h asserts each against the kernel header's own)
constexpr int ENGINE_VALU = 0, ENGINE_MFMA = 1, ENGINE_SPLIT = 2, ENGINE_FUSED = 3, ENGINE_LITE = 4;     // include/drp.h
// ENGINE_LITE is the fused engine with fewer product terms in its kernels (k_mlp_split.h: TERMS): every plan below decides as for
// ENGINE_FUSED -- the same kernels, cuts, grids and thresholds -- and only carries the flag on to the launch tables and the names.
constexpr bool engine_is_fused(int engine) { return engine == ENGINE_FUSED || engine == ENGINE_LITE; }
constexpr int engine_for_plan(int engine) { return engine == ENGINE_LITE ? ENGINE_FUSED : engine; }
constexpr int K = 10;
constexpr int GRAPH_THREADS_ = 128, GC_MAX_BANDS_ = 32, GC_THREADS_ = 256;
constexpr int PROP_WAVES_ = 8, EC_UNITS_ = 512;
constexpr int ROLLOUT_MAX_ROWS = 3072, BWD_ROWS_MAX = 256, COOP_SLOTS = 2, AGG_LDS_MAX_N = 600;
constexpr long DEG_STAT_ROWS = 65536;
constexpr long spread_grid(long n_items) { return (n_items + 31) & ~31L; }             // SPREAD_GRID of k_graph.h

// ---- which kernel variant served a launch (drp_last_dispatch) ---------------------------------------------------
// Every place that chooses between kernels or template instantiations marks the variant it launched in the context; the
// host asks for the names (drp_last_dispatch) and for the whole list (drp_dispatch_variants).  tests/test_gpu_fuzz_oracle.py
// draws shapes under the default dispatch, checks each against the oracle and fails if a variant in the list was never hit:
// a threshold change that orphans an instantiation turns the suite red.
enum DispatchVariant {
    DV_GRAPH_PLAIN = 0, DV_GRAPH_Q4, DV_GRAPH_Q4_ENCODE, DV_GRAPH_STRIPS, DV_GRAPH_STRIPS256, DV_GRAPH_CELLS, DV_GRAPH_REV, DV_GRAPH_IN_ROLLOUT,
    DV_VALU_STEP, DV_NODE_ENCODE, DV_NODE_ENCODE_SPLIT, DV_EDGE_ENCODE, DV_EDGE_ENCODE_SPLIT, DV_AGGREGATE, DV_AGGREGATE_LDS,
    DV_AGGREGATE_TAPE, DV_UPDATE,
    DV_PROP,                        // + PropFlags::index()
    DV_PROP3 = DV_PROP + 16,        // + Prop3Flags::index()
    DV_ROLLOUT = DV_PROP3 + 24,     // + RolloutFlags::index()
    DV_REWARD = DV_ROLLOUT + 12, DV_BWD_REWARD, DV_REV_256, DV_REV_1024, DV_BWD_ROWS, DV_BWD_STEP, DV_BWD_STAGES_MFMA,
    DV_BWD_EDGE_MFMA, DV_TRAIN_NODE_FUSED, DV_TRAIN_NODE_FUSED_COOP, DV_TRAIN_NODE_MFMA, DV_WGRAD_MFMA, DV_WGRAD_VALU,
    DV_WGRAD_DEFERRED, DV_MPPI_SOFTMAX, DV_ELITE_SORT, DV_ELITE_ROUNDS, DV_FPS_REG, DV_FPS_MEM, DV_DT_CV5, DV_DT_EXACT,
    DV_TRAIN_BARRIER_RETRY,
    // the reduced-product instantiations of ENGINE_LITE (forward only: no tape), behind everything else so that no id moves
    DV_PROP_LITE,                                   // + PropFlags::lite_index()
    DV_PROP3_LITE = DV_PROP_LITE + 8,               // + Prop3Flags::lite_index()
    DV_ROLLOUT_LITE = DV_PROP3_LITE + 12,           // + RolloutFlags::lite_index()
    DV_NODE_ENCODE_SPLIT_LITE = DV_ROLLOUT_LITE + 12, DV_GRAPH_Q4_ENCODE_LITE,
    DV_COUNT
};

// The template flags of the three families, in one place: the launch tables (capi_pipeline.h), the names and the marks all
// go through index() / from_index().  cache: 0 off, 1 on, 2 on with a tile's rows kept in registers between the steps.
// lite: the reduced-product instantiation (never with tape); those have a table and an id range of their own (lite_index, variant).
struct PropFlags {
    bool last, tape, pair, work, lite = false;
    static constexpr int COUNT = 16, LITE_COUNT = 8;
    constexpr int index() const { return 8 * (last ? 1 : 0) + 4 * (tape ? 1 : 0) + 2 * (pair ? 1 : 0) + (work ? 1 : 0); }
    constexpr int lite_index() const { return 4 * (last ? 1 : 0) + 2 * (pair ? 1 : 0) + (work ? 1 : 0); }
    constexpr int variant() const { return lite ? DV_PROP_LITE + lite_index() : DV_PROP + index(); }
    static constexpr PropFlags from_index(int f) { return PropFlags{(f & 8) != 0, (f & 4) != 0, (f & 2) != 0, (f & 1) != 0}; }
    static constexpr PropFlags from_lite_index(int f) { return PropFlags{(f & 4) != 0, false, (f & 2) != 0, (f & 1) != 0, true}; }
};
struct Prop3Flags {
    bool tape, pair; int cache; bool work, lite = false;
    static constexpr int COUNT = 24, LITE_COUNT = 12;
    constexpr int index() const { return 12 * (tape ? 1 : 0) + 6 * (pair ? 1 : 0) + 2 * cache + (work ? 1 : 0); }
    constexpr int lite_index() const { return 6 * (pair ? 1 : 0) + 2 * cache + (work ? 1 : 0); }
    constexpr int variant() const { return lite ? DV_PROP3_LITE + lite_index() : DV_PROP3 + index(); }
    static constexpr Prop3Flags from_index(int f) { return Prop3Flags{f / 12 != 0, ((f / 6) & 1) != 0, (f % 6) / 2, (f & 1) != 0}; }
    static constexpr Prop3Flags from_lite_index(int f) { return Prop3Flags{false, f / 6 != 0, (f % 6) / 2, (f & 1) != 0, true}; }
};
struct RolloutFlags {
    bool pair; int cache; bool work, lite = false;
    static constexpr int COUNT = 12, LITE_COUNT = 12;
    constexpr int index() const { return 6 * (pair ? 1 : 0) + 2 * cache + (work ? 1 : 0); }
    constexpr int lite_index() const { return index(); }
    constexpr int variant() const { return lite ? DV_ROLLOUT_LITE + lite_index() : DV_ROLLOUT + index(); }
    static constexpr RolloutFlags from_index(int f) { return RolloutFlags{f / 6 != 0, (f % 6) / 2, (f & 1) != 0}; }
    static constexpr RolloutFlags from_lite_index(int f) { return RolloutFlags{f / 6 != 0, (f % 6) / 2, (f & 1) != 0, true}; }
};
static_assert(DV_PROP3 - DV_PROP == PropFlags::COUNT && DV_ROLLOUT - DV_PROP3 == Prop3Flags::COUNT && DV_REWARD - DV_ROLLOUT == RolloutFlags::COUNT &&
              DV_PROP3_LITE - DV_PROP_LITE == PropFlags::LITE_COUNT && DV_ROLLOUT_LITE - DV_PROP3_LITE == Prop3Flags::LITE_COUNT &&
              DV_NODE_ENCODE_SPLIT_LITE - DV_ROLLOUT_LITE == RolloutFlags::LITE_COUNT,
              "the variant ids leave each family its index range");

// name of variant `id`; *by_default = reachable without an environment switch (DRP_NO_* / drp_probe_begin("prop+work")) or an
// engine chosen by hand (the lite names)
inline void dv_name(int id, char* buf, size_t n, bool* by_default) {
    bool dflt = true;
    static const char* const cache_names[3] = {"", ",cache", ",cache+rows"};
    if (id >= DV_PROP_LITE && id < DV_PROP3_LITE) {
        const PropFlags f = PropFlags::from_lite_index(id - DV_PROP_LITE);
        snprintf(buf, n, "km_prop<%s%s%s,lite>", f.last ? "last" : "mid", f.pair ? ",pair" : "", f.work ? ",work" : "");
        dflt = false;
    } else if (id >= DV_PROP3_LITE && id < DV_ROLLOUT_LITE) {
        const Prop3Flags f = Prop3Flags::from_lite_index(id - DV_PROP3_LITE);
        snprintf(buf, n, "km_prop3<plain%s%s%s,lite>", f.pair ? ",pair" : "", cache_names[f.cache], f.work ? ",work" : "");
        dflt = false;
    } else if (id >= DV_ROLLOUT_LITE && id < DV_NODE_ENCODE_SPLIT_LITE) {
        const RolloutFlags f = RolloutFlags::from_lite_index(id - DV_ROLLOUT_LITE);
        snprintf(buf, n, "km_rollout<%s%s%s,lite>", f.pair ? "pair" : "tile32", cache_names[f.cache], f.work ? ",work" : "");
        dflt = false;
    } else if (id >= DV_PROP && id < DV_PROP3) {
        const PropFlags f = PropFlags::from_index(id - DV_PROP);
        snprintf(buf, n, "km_prop<%s%s%s%s>", f.last ? "last" : "mid", f.tape ? ",tape" : "", f.pair ? ",pair" : "", f.work ? ",work" : "");
        dflt = !f.work;
    } else if (id >= DV_PROP3 && id < DV_ROLLOUT) {
        const Prop3Flags f = Prop3Flags::from_index(id - DV_PROP3);
        snprintf(buf, n, "km_prop3<%s%s%s%s>", f.tape ? "tape" : "plain", f.pair ? ",pair" : "", cache_names[f.cache], f.work ? ",work" : "");
        // paired tiles mean at most 128 rows per workgroup: the cache always fits and the rows stay in registers, unless
        // DRP_ECACHE_MAX_MB says otherwise
        dflt = !f.work && !(f.pair && f.cache != 2);
    } else if (id >= DV_ROLLOUT && id < DV_REWARD) {
        const RolloutFlags f = RolloutFlags::from_index(id - DV_ROLLOUT);
        snprintf(buf, n, "km_rollout<%s%s%s>", f.pair ? "pair" : "tile32", cache_names[f.cache], f.work ? ",work" : "");
        dflt = !f.work && !(f.pair && f.cache != 2);
    } else {
        const char* s = "?";
        switch (id) {
        case DV_GRAPH_PLAIN: s = "graph:k_graph"; break;
        case DV_GRAPH_Q4: s = "graph:k_graph_q4"; break;
        case DV_GRAPH_Q4_ENCODE: s = "graph:km_graph_q4_encode (+ particle encoder)"; break;
        case DV_GRAPH_STRIPS: s = "graph:k_graph_strips_q<128>"; break;
        case DV_GRAPH_STRIPS256: s = "graph:k_graph_strips_q<256>"; dflt = false; break;   // from 800 particles, where the cells have taken over (DRP_NO_GRAPH_CELLS=1)
        case DV_GRAPH_CELLS: s = "graph:k_graph_cells"; break;
        case DV_GRAPH_REV: s = "graph:k_graph_rev"; break;
        case DV_GRAPH_IN_ROLLOUT: s = "graph:in km_rollout"; break;
        case DV_VALU_STEP: s = "valu:k_node_encode..k_predict"; break;
        case DV_NODE_ENCODE: s = "km_node_encode"; break;
        case DV_NODE_ENCODE_SPLIT: s = "km_node_encode_split"; break;
        case DV_EDGE_ENCODE: s = "km_edge_encode"; break;
        case DV_EDGE_ENCODE_SPLIT: s = "km_edge_encode_split"; break;
        case DV_AGGREGATE: s = "k_aggregate"; break;
        case DV_AGGREGATE_LDS: s = "k_aggregate_lds"; break;
        case DV_AGGREGATE_TAPE: s = "k_aggregate_tape"; break;
        case DV_UPDATE: s = "km_update"; break;
        case DV_REWARD: s = "k_reward"; break;
        case DV_BWD_REWARD: s = "kb_reward"; break;
        case DV_REV_256: s = "kb_reverse_lists<256>"; break;
        case DV_REV_1024: s = "kb_reverse_lists<1024>"; break;
        case DV_BWD_ROWS: s = "bwd:kmb_rows_bwd"; break;
        case DV_BWD_STEP: s = "bwd:kmb_step_bwd"; break;
        case DV_BWD_STAGES_MFMA: s = "bwd:stages kmb_*"; break;
        case DV_BWD_EDGE_MFMA: s = "bwd:kmb_edge_encode"; break;
        case DV_TRAIN_NODE_FUSED: s = "train:kmb_step_bwd<dump>"; dflt = false; break;    // DRP_TRAIN_COOP=0 (by default a workgroup of the one-launch pass has one tile)
        case DV_TRAIN_NODE_FUSED_COOP: s = "train:kmb_step_bwd<dump,coop>"; break;
        case DV_TRAIN_NODE_MFMA: s = "train:stages kmb_*"; break;
        case DV_WGRAD_MFMA: s = "train:kt_wgrad_mfma"; break;
        case DV_WGRAD_VALU: s = "train:kt_wgrad"; dflt = false; break;
        case DV_WGRAD_DEFERRED: s = "train:deferred wgrad lists"; break;
        case DV_MPPI_SOFTMAX: s = "mppi:k_mppi_partials+update"; break;
        case DV_ELITE_SORT: s = "mppi:k_elite_local sort"; break;
        case DV_ELITE_ROUNDS: s = "mppi:k_elite_local rounds"; break;
        case DV_FPS_REG: s = "k_fps_reg"; break;
        case DV_FPS_MEM: s = "k_fps"; break;
        case DV_DT_CV5: s = "k_dt_cv5"; break;
        case DV_DT_EXACT: s = "k_edt"; break;
        case DV_NODE_ENCODE_SPLIT_LITE: s = "km_node_encode_split<lite>"; dflt = false; break;
        case DV_GRAPH_Q4_ENCODE_LITE: s = "graph:km_graph_q4_encode<lite> (+ particle encoder)"; dflt = false; break;
        case DV_TRAIN_BARRIER_RETRY: s = "train:barrier gave up, step re-run with one workgroup per group"; dflt = false; break;   // a shared / masked device
        default: break;
        }
        snprintf(buf, n, "%s", s);
    }
    if (by_default) *by_default = dflt;
}

// ---- the policy ----------------------------------------------------------------------------------------------------
struct DispatchPolicy {
    bool agg_global_only = false;   // always gather sender rows from L2/HBM (timing builds)
    bool rev_global_only = false;   // DRP_REV_GLOBAL=1: reversed neighbour lists built in global memory (the N > 3072 path)
    bool self_const = true;         // DRP_NO_SELF_CONST=1: always run the encoder chain on the self slot too
    bool prop3 = true;              // DRP_NO_PROP3=1: one launch per propagation step even for chip-filling batches
    int prop3_min_b = 0;            // km_prop3 / kmb_step_bwd from this many samples (0: whole_samples() decides)
    int prop3_min_tiles = 1;        // km_prop3 from this many tiles per workgroup and step
    int bwd_fused_min_tiles = 1;    // the same for kmb_step_bwd
    bool graph_cells = true;        // DRP_NO_GRAPH_CELLS=1: x strips only (k_graph_strips) for large samples
    int graph_cells_min_n = 400;    // DRP_GRAPH_CELLS_MIN_N: two-dimensional cells from this many particles up (measured: slower at 300, 8 % faster at 450)
    float graph_cells_halo = 0.0f;  // DRP_GRAPH_CELLS_HALO: first-sweep halo in camera-frame units (default: from the particle count)
    float graph_cells_hb = 0.0f;    // DRP_GRAPH_CELLS_HB: band height in camera-frame units (default: from the particle count)
    bool graph_strips = true;       // DRP_NO_GRAPH_STRIPS=1: plain neighbour sweep for every shape
    bool bwd_fused = true;          // DRP_NO_BWD_FUSED=1: the GD planner's backward pass as one launch per stage
    bool graph_rev = true;          // DRP_NO_GRAPH_REV=1: the GD planner's reversed lists always in a launch of their own (kb_reverse_lists)
    bool graph_encode = true;       // DRP_NO_GRAPH_ENCODE=1: k_graph_q4 and km_node_encode_split as two launches where they could be one (km_graph_q4_encode)
    int train_fused = -1;           // DRP_TRAIN_FUSED=0/1: the trainer's node stages as one launch per rollout step (kmb_step_bwd<dump>) never / for any batch (-1: up to n_cu / 4 tiles)
    int train_coop = -1;            // DRP_TRAIN_COOP=0/1: the workgroup-wide gather of the edge terms off / on whatever the tile count (-1: by tiles per workgroup)
    int train_parts = 0;            // DRP_TRAIN_PARTS=n: workgroups per group of samples in the trainer's kmb_step_bwd (0: as many as there are CUs for)
    bool bwd_rows = true;           // DRP_NO_BWD_ROWS=1: piles of up to 256 particles through kmb_step_bwd (rows through memory) instead of kmb_rows_bwd
    bool prop3_order = true;        // false: km_prop3's tiles in the natural row order instead of by in-degree
    int prop_pair_rows = 128;       // DRP_PROP_PAIR_ROWS: a workgroup of the whole-sample kernels with up to so many rows runs tiles of
                                    // 16 receivers x two slots (0 = never)
    int prop_pair_always = 64;      // DRP_PROP_PAIR_ALWAYS: ... whatever the in-degrees up to so many rows (four tiles of 16: a SIMD each),
    int prop_pair_deg10 = 83;       // DRP_PROP_PAIR_DEG10: above that while the piles' mean in-degree (x 10) is at most this
    bool prop3e = true;             // false: the particle encoder stays its own launch in front of km_prop3
    bool rollout_fused = true;      // DRP_NO_ROLLOUT_FUSED=1: one graph + one km_prop3 launch per rollout step for small piles too
    int rollout_max_n = 64;         // DRP_ROLLOUT_MAX_N: km_rollout (the whole rollout in one launch) up to this many particles ...
    int rollout_mid_n = 256, rollout_mid_rows = 256;  // ... up to 256 particles for workgroups of up to 256 rows (small batches; the
                                    // kernels with the kept rows and the lists beside the encoder: 256 x 80 / 100 / 128 / 150 / 200 / 256
                                    // + 23 / + 14 / + 13 / + 13 / + 5 / + 6 %, 512 x 100 / 128 + 13 / + 16 %, 128 x 150 + 7 %, 341 x 96 + 16 %;
                                    // 64 x 256 - 5 %: above 200 particles only from half a chip of samples; 1024 x 80 / 100 (320 / 400 rows): - 1 %)
    int rollout_max_rows = 704;     // ... and this many rows (samples x particles) per workgroup.  Measured
                                    // against the step-by-step pipeline at 1024 samples: +18 % at 10 particles, +12 % at 20, +2 % at
                                    // 50, +5 % at 64, -1 % at 80, -10 % at 150 (the strip build wins); 50 particles x 4096 samples
                                    // (800 rows per workgroup) -5 %, 20 x 8192 (640 rows) +7 %

    // Edge-chain cache of the whole-sample kernels (prop_tiles, EC): the relation encoder's chain runs in the first propagation
    // step only and its output is read back in the other two, from a workgroup-private buffer of 80 KB per tile of 32 receivers
    // (2.5 KB per receiver).  The cached kernels differ from the recomputing ones in the last place of one sum, so WHICH of the
    // two serves a sample must not depend on how many samples travel with it (a 1 024-sample shard of an 8 192-sample job, a
    // rank's half of the planner's 1 500 rows: the sharded and the unsharded run must agree bit for bit): the choice is a function
    // of the PILE SIZE alone (ec_shape; DRP_ECACHE_MAX_MB=0: never) -- and the buffer stays small by construction instead: a
    // cached launch gives a workgroup at most ec_rows_cap(N) rows, and a batch that needs more than one such launch is run as
    // several, one after the other on the stream, over the same buffer (cut_blocks; 256 workgroups x 9 tiles
    // x 80 KB = 189 MB, inside the 256 MB of last-level cache).
    // Which pile sizes: measured with the blocks in place (tools/ab_env_shapes.sh, DRP_ECACHE_MAX_N=64 against 256, one box):
    // 256 samples x 80 / 100 / 150 / 200 particles + 15 / + 31 / + 35 / + 19 %, 1 024 x 80 / 100 / 128 / 256 + 8 / + 7 / + 7 /
    // + 3 %, but 1 024 x 150 - 12 % and x 200 - 5 %: one sample of 129 ... 224 particles leaves three to one of a workgroup's
    // eight waves without a tile.  So: up to ecache_max_n = 128 particles (two samples of up to 128 fill the eight tiles), and
    // ecache_full_n = 225 ... 256 (one sample, eight tiles).  The TAPE's launches (gradient-descent planner, trainer) write one
    // history buffer over the whole batch and are cut into the same blocks (the kernel takes the buffer's slot stride: hist_rows;
    // tests/test_gpu_tape_blocks.py); the cache pays up to ecache_tape_max_n = 40 particles at the planner's 1 500 rows, one launch
    // (50 particles: 0.398 ms per iteration recomputing, 0.42 cached).
    int ecache_max_mb = 192;
    int ecache_hard_max_mb = 4096;  // DRP_ECACHE_HARD_MAX_MB: a cached batch whose first launch would need more (batch columns no block is a multiple
                                    // of: 1.6 million rows in one launch) recomputes instead, in one launch -- no caller of the reference comes
                                    // near; the one place where the batch decides the kernel
    int ecache_max_n = 128, ecache_full_n = 225, ecache_tape_max_n = 40;
    int graph_q4 = 1;               // DRP_GRAPH_Q4=0 / 1 / 2: four threads per receiver in the plain neighbour sweep -- never / for a handful
                                    // of samples (fewer workgroups than half the CUs) / whenever the plain sweep is chosen
    bool wgrad_mfma = true;         // DRP_NO_WGRAD_MFMA=1: the weight gradients' outer-product sums on the VALU kernel (kt_wgrad_multi)
    bool prop_spread = true;        // DRP_NO_PROP_SPREAD=1: km_prop's tiles eight to a workgroup whatever their number
};

// ---- the environment switches: ONE table ---------------------------------------------------------------------------
struct EnvSwitch {
    enum Kind { OFF_IF_SET, ON_IF_SET, INT, FLOAT };
    const char* name;
    Kind kind;
    bool DispatchPolicy::*b;
    int DispatchPolicy::*i;
    float DispatchPolicy::*f;
    int lo, hi;                                 // INT: the value is clamped to [lo, hi]
    void (*also)(DispatchPolicy&);              // what setting it changes besides its own field (null: nothing)
    const char* what;
};
inline void rollout_max_n_also(DispatchPolicy& p) { p.rollout_mid_n = 0; p.rollout_max_rows = ROLLOUT_MAX_ROWS; }
inline void ecache_max_n_also(DispatchPolicy& p) { p.ecache_full_n = 257; }
#define DRP_SW_B(NAME, KIND, FIELD, WHAT) {NAME, EnvSwitch::KIND, &DispatchPolicy::FIELD, nullptr, nullptr, 0, 0, nullptr, WHAT}
#define DRP_SW_I(NAME, FIELD, LO, HI, ALSO, WHAT) {NAME, EnvSwitch::INT, nullptr, &DispatchPolicy::FIELD, nullptr, LO, HI, ALSO, WHAT}
#define DRP_SW_F(NAME, FIELD, WHAT) {NAME, EnvSwitch::FLOAT, nullptr, nullptr, &DispatchPolicy::FIELD, 0, 0, nullptr, WHAT}
inline const EnvSwitch* env_switches(int* count) {
    static const EnvSwitch table[] = {
        DRP_SW_B("DRP_NO_SELF_CONST", OFF_IF_SET, self_const, "the encoder chain runs on the self slot too"),
        DRP_SW_B("DRP_NO_PROP3", OFF_IF_SET, prop3, "one launch per propagation step even for chip-filling batches"),
        DRP_SW_B("DRP_NO_GRAPH_STRIPS", OFF_IF_SET, graph_strips, "plain neighbour sweep for every shape"),
        DRP_SW_B("DRP_NO_GRAPH_CELLS", OFF_IF_SET, graph_cells, "x strips only for large samples"),
        DRP_SW_I("DRP_GRAPH_CELLS_MIN_N", graph_cells_min_n, INT_MIN, INT_MAX, nullptr, "two-dimensional cells from this many particles up"),
        DRP_SW_F("DRP_GRAPH_CELLS_HB", graph_cells_hb, "band height of the cells in camera-frame units"),
        DRP_SW_F("DRP_GRAPH_CELLS_HALO", graph_cells_halo, "first-sweep halo of the cells in camera-frame units"),
        DRP_SW_B("DRP_NO_ROLLOUT_FUSED", OFF_IF_SET, rollout_fused, "graph + km_prop3 per rollout step for small piles too"),
        DRP_SW_B("DRP_NO_PROP_SPREAD", OFF_IF_SET, prop_spread, "km_prop's tiles eight to a workgroup whatever their number"),
        DRP_SW_B("DRP_NO_WGRAD_MFMA", OFF_IF_SET, wgrad_mfma, "weight gradients on the VALU kernel"),
        DRP_SW_I("DRP_GRAPH_Q4", graph_q4, INT_MIN, INT_MAX, nullptr, "k_graph_q4: 0 never, 1 for a handful of samples, 2 wherever the plain sweep is chosen"),
        DRP_SW_I("DRP_ROLLOUT_MAX_N", rollout_max_n, INT_MIN, INT_MAX, rollout_max_n_also,
                 "km_rollout up to this many particles; also: no mid range (rollout_mid_n = 0), rows per workgroup up to the kernel's limit"),
        // km_rollout<pair> keeps 16 B per row in the 4 KB behind the encoder's matrices
        DRP_SW_I("DRP_PROP_PAIR_ROWS", prop_pair_rows, 0, 256, nullptr, "paired tiles up to so many rows per workgroup (0: never)"),
        DRP_SW_I("DRP_PROP_PAIR_ALWAYS", prop_pair_always, 0, INT_MAX, nullptr, "... whatever the in-degrees up to so many rows"),
        DRP_SW_I("DRP_PROP_PAIR_DEG10", prop_pair_deg10, 0, INT_MAX, nullptr, "... above that while the mean in-degree x 10 is at most this"),
        DRP_SW_B("DRP_NO_BWD_FUSED", OFF_IF_SET, bwd_fused, "the backward pass as one launch per stage"),
        DRP_SW_B("DRP_NO_BWD_ROWS", OFF_IF_SET, bwd_rows, "piles of up to 256 particles through kmb_step_bwd instead of kmb_rows_bwd"),
        DRP_SW_I("DRP_TRAIN_PARTS", train_parts, INT_MIN, INT_MAX, nullptr, "workgroups per group of samples in the trainer's kmb_step_bwd"),
        DRP_SW_I("DRP_TRAIN_COOP", train_coop, INT_MIN, INT_MAX, nullptr, "the workgroup-wide gather of the edge terms: 0 off, 1 on"),
        DRP_SW_B("DRP_NO_GRAPH_ENCODE", OFF_IF_SET, graph_encode, "k_graph_q4 and km_node_encode_split as two launches"),
        DRP_SW_I("DRP_TRAIN_FUSED", train_fused, INT_MIN, INT_MAX, nullptr, "the trainer's node stages in one launch: 0 never, 1 for any batch"),
        DRP_SW_B("DRP_NO_GRAPH_REV", OFF_IF_SET, graph_rev, "the reversed lists always in a launch of their own"),
        DRP_SW_B("DRP_REV_GLOBAL", ON_IF_SET, rev_global_only, "reversed lists built in global memory"),
        DRP_SW_I("DRP_ECACHE_MAX_MB", ecache_max_mb, 0, INT_MAX, nullptr, "0: the edge-chain cache is never used"),
        DRP_SW_I("DRP_ECACHE_HARD_MAX_MB", ecache_hard_max_mb, 0, INT_MAX, nullptr,
                 "a cached batch whose first launch needs a cache buffer above this many MB recomputes instead, in one launch"),
        DRP_SW_I("DRP_ECACHE_MAX_N", ecache_max_n, 0, INT_MAX, ecache_max_n_also, "cached up to this many particles; also: no 225 ... 256 range (ecache_full_n = 257)"),
        DRP_SW_I("DRP_ECACHE_TAPE_MAX_N", ecache_tape_max_n, 0, INT_MAX, nullptr, "the tape's launches cached up to this many particles"),
    };
    *count = (int)(sizeof(table) / sizeof(table[0]));
    return table;
}
#undef DRP_SW_B
#undef DRP_SW_I
#undef DRP_SW_F
inline DispatchPolicy policy_from_env() {
    DispatchPolicy p;
    int n = 0;
    const EnvSwitch* t = env_switches(&n);
    for (int q = 0; q < n; ++q) {
        const char* e = getenv(t[q].name);
        switch (t[q].kind) {
        case EnvSwitch::OFF_IF_SET: p.*(t[q].b) = e == nullptr; break;
        case EnvSwitch::ON_IF_SET: p.*(t[q].b) = e != nullptr; break;
        case EnvSwitch::INT: if (e) p.*(t[q].i) = std::min(t[q].hi, std::max(t[q].lo, atoi(e))); break;
        case EnvSwitch::FLOAT: if (e) p.*(t[q].f) = (float)atof(e); break;
        }
        if (e && t[q].also) t[q].also(p);
    }
    return p;
}

// ---- rules shared by the plans ---------------------------------------------------------------------------------------
// the mean in-degree the last lists of a shape had (k_deg_stat writes it behind a launch, every few launches); only ever a
// question of speed -- paired and unpaired tiles give the same bits
struct DegStat {
    bool have = false;              // false: no word yet
    long sum = 0, rows = 0, n = 0;  // in-degrees summed over `rows` rows of piles of `n` particles
};
inline DegStat decode_deg_stat(unsigned long long v) {
    DegStat d;
    d.have = true; d.sum = (long)(v & 0xffffffull); d.rows = (long)((v >> 24) & 0xffffffull); d.n = (long)(v >> 48);
    return d;
}

namespace detail {
// km_prop3 / kmb_step_bwd (a workgroup owns whole samples and runs all propagation steps in one launch) or the
// per-step kernels (the tiles of all samples dealt over the chip)?  Whole samples whenever (nearly) every CU gets one --
// and for ANY batch of samples of up to 256 particles (one round of tiles per step for the workgroup's eight waves):
// a small batch is latency, and one launch per rollout step instead of five is what counts (B = 32 ... 255 at 50 / 100
// particles: 1.7 - 2.0 -> 1.0 - 1.2 ms per MPPI iteration; 300 particles: 2 - 7 % slower below 200 samples, 27 % faster
// at 255).
inline bool whole_samples(const DispatchPolicy& p, int n_cu, long B, int N) {
    if (p.prop3_min_b > 0) return B >= p.prop3_min_b;
    return B >= n_cu - n_cu / 5 || N <= 256;
}
inline long tiles32(long rows) { return (rows + 31) / 32; }
}  // namespace detail

// paired tiles (16 receivers x two slots) for a workgroup of `spw` samples of N particles, of a batch of B?
struct PairRule {
    int rows, always, deg10;        // DispatchPolicy::prop_pair_*
    bool operator()(const DegStat& d, long spw, long N, long B) const {
        const long r = spw * N;
        if (r > rows) return false;
        if (r <= always || !d.have) return true;
        if (d.n != N || d.rows != std::min(B * N, DEG_STAT_ROWS) || d.rows == 0) return true;   // not known (yet)
        return d.sum * 10 <= d.rows * (long)deg10;
    }
};
inline PairRule pair_rule(const DispatchPolicy& p) { return PairRule{p.prop_pair_rows, p.prop_pair_always, p.prop_pair_deg10}; }
// how many float4 a workgroup of `rows` receivers needs in the edge-chain cache
inline size_t ecache_stride(long rows, bool pair) {
    const long tiles = pair ? (rows + 15) / 16 : (rows + 31) / 32;
    return (size_t)tiles * (pair ? 5 : K) * EC_UNITS_;
}
inline bool ec_shape(const DispatchPolicy& p, int N, bool tape) {
    if (p.ecache_max_mb <= 0) return false;
    if (tape) return N <= p.ecache_tape_max_n;
    return N <= p.ecache_max_n || (N >= p.ecache_full_n && N <= 256);
}
// rows a workgroup of a cached launch may hold: nine tiles of 32 (up to 64 particles: the measured best at 1 024 x 64 is
// four samples = eight tiles), eight -- one per wave, rows kept in registers -- above
inline long ec_rows_cap(int N) { return N <= 64 ? 288 : 256; }
// samples per launch of a cached shape: every CU a workgroup of at most ec_rows_cap rows, in whole multiples of `unit`
// (the batch columns: row b reads column b % unit of the replicated inputs)
inline long ec_chunk(int n_cu, int N, long unit) {
    const long spw = std::max(1L, ec_rows_cap(N) / N);
    long chunk = (long)n_cu * spw;
    if (unit > 1) chunk = chunk / unit * unit;
    return chunk;
}

// One launch of a whole-sample kernel (km_prop3, km_rollout) over a block of consecutive samples
struct Block {
    long b_off; int Bc, spw, grid;
    bool pair;
    int cache;                      // 0 off, 1 on, 2 on with the rows kept: no more tiles than waves in a workgroup -- the cached kernel
                                    // then hands a tile's own rows from one propagation step to the next in registers
    size_t ec_stride, cache_bytes;  // float4 per workgroup; what the launch needs of the cache buffer
};
// A batch as the whole-sample kernels take it: cached or recomputing by the pile size alone (ec_shape); a cached batch too
// large for one launch of at most ec_rows_cap rows per workgroup goes out as several launches over consecutive blocks of
// `chunk` samples, the same cache buffer under each.  The blocks are computed on demand (block(q)): no list, no allocation.
struct Blocks {
    int B = 0, N = 0, n_cu = 1, n = 1;
    long chunk = 0;
    bool cache = false;
    size_t cache_bytes = 0;         // the cache buffer of the first (largest) block with unpaired tiles
    DegStat deg;
    PairRule pair{0, 0, 0};
    Block block(int q) const {
        Block b;
        b.b_off = (long)q * chunk;
        b.Bc = (int)std::min(chunk, (long)B - b.b_off);
        b.spw = (b.Bc + n_cu - 1) / n_cu;
        b.grid = (b.Bc + b.spw - 1) / b.spw;
        b.pair = pair(deg, b.spw, N, B);
        const long rows = (long)b.spw * N;
        b.cache = !cache ? 0 : ((b.pair ? (rows + 15) / 16 : (rows + 31) / 32) <= PROP_WAVES_ ? 2 : 1);
        b.ec_stride = ecache_stride(rows, b.pair);
        b.cache_bytes = cache ? (size_t)b.grid * b.ec_stride * 16 : 0;
        return b;
    }
};
// unit / splittable: the batch columns every block must be a whole multiple of, and whether there is such a multiple
inline Blocks cut_blocks(const DispatchPolicy& p, int n_cu, int B, int N, bool tape, long unit, bool splittable, const DegStat& deg) {
    Blocks k;
    k.B = B; k.N = N; k.n_cu = n_cu; k.deg = deg;
    k.pair = pair_rule(p);
    k.cache = ec_shape(p, N, tape);
    k.chunk = B;
    if (k.cache && splittable) {
        const long cap = ec_chunk(n_cu, N, unit);
        if (cap > 0 && cap < B) k.chunk = cap;
    }
    if (k.cache) {
        // a launch that cannot be split (the tape's; batch columns no block is a multiple of) takes a cache over the whole
        // batch, 2.5 KB per row: beyond ecache_hard_max_mb it recomputes instead of failing for memory
        const long B0 = std::min((long)B, k.chunk), spw0 = (B0 + n_cu - 1) / n_cu;
        k.cache_bytes = (size_t)((B0 + spw0 - 1) / spw0) * ecache_stride(spw0 * N, false) * 16;
        if (k.cache_bytes > ((size_t)p.ecache_hard_max_mb << 20)) { k.cache = false; k.chunk = B; k.cache_bytes = 0; }
    }
    k.n = (int)((B + k.chunk - 1) / k.chunk);
    return k;
}

// ---- neighbour lists ---------------------------------------------------------------------------------------------------
// x-strip variant for samples of at least two workgroups (below that a wave's range is the whole sample anyway), plain
// sweep otherwise and for zero-padded batches (coincident particles tie at the cut); two-dimensional cells for large samples;
// four threads per receiver for a handful of samples (training batches)
struct GraphPlan {
    enum Kind { NONE, CELLS, STRIPS128, STRIPS256, Q4, Q4_ENCODE, REV, PLAIN };
    Kind kind = NONE;
    int chunks = 1;                 // workgroups (CELLS: of 16 quarter waves) per sample
    long grid = 0;                  // of the lists' launch (Q4_ENCODE: its graph part)
    int gy = 0; float inv_hb = 0.0f, halo = 0.0f;   // CELLS: y bands, their inverse height, the first sweep's halo
    bool lite = false;              // Q4_ENCODE: the encoder's part on the reduced products
    int variant() const {
        switch (kind) {
        case CELLS: return DV_GRAPH_CELLS;
        case STRIPS128: return DV_GRAPH_STRIPS;
        case STRIPS256: return DV_GRAPH_STRIPS256;
        case Q4: return DV_GRAPH_Q4;
        case Q4_ENCODE: return lite ? DV_GRAPH_Q4_ENCODE_LITE : DV_GRAPH_Q4_ENCODE;
        case REV: return DV_GRAPH_REV;
        default: return DV_GRAPH_PLAIN;
        }
    }
};
// has_actions: the impulses come from pushes (false: they are data); wants_rev: the caller can take the reversed lists from
// the lists' own launch; no_encoder_launch: the step has no particle encoder launch to share (km_prop3 runs it)
inline GraphPlan plan_graph(const DispatchPolicy& p, int n_cu, int engine, int B, int N, bool padded, bool has_actions, bool wants_rev,
                            bool no_encoder_launch) {
    GraphPlan g;
    g.lite = engine == ENGINE_LITE;
    engine = engine_for_plan(engine);
    if (wants_rev && N <= GRAPH_THREADS_ && p.graph_rev) {
        g.kind = GraphPlan::REV;
        g.grid = spread_grid(B);
    } else if (p.graph_cells && p.graph_strips && !padded && N >= p.graph_cells_min_n) {
        // y bands of height hb ~ sqrt(16 / density) (a 16-receiver block of a band is then about as wide as the band is
        // high; the density of a pile spread over the 0.4 x 0.4 workspace -- any positive hb gives the same lists)
        g.kind = GraphPlan::CELLS;
        float hb = sqrtf(16.0f * 0.16f / (float)N);
        if (p.graph_cells_hb > 0.0f) hb = p.graph_cells_hb;
        g.gy = std::max(1, std::min(GC_MAX_BANDS_, (int)ceilf(0.64f / hb)));
        g.inv_hb = (float)g.gy / 0.64f;
        g.halo = p.graph_cells_halo > 0.0f ? p.graph_cells_halo
                 // expected distance of the 10th neighbour in a pile of this density, with a third to spare
                 : 1.3f * sqrtf(10.0f * 0.16f / (3.14159265f * (float)N));
        // receivers are dealt to quarter waves band by band: at most N / 16 + gy quarters, 16 per workgroup
        g.chunks = ((N + 15) / 16 + g.gy + GC_THREADS_ / 16 - 1) / (GC_THREADS_ / 16);
        g.grid = spread_grid((long)B * g.chunks);
    } else if (p.graph_strips && !padded && N > GRAPH_THREADS_) {
        g.kind = N >= 800 ? GraphPlan::STRIPS256 : GraphPlan::STRIPS128;
        g.chunks = N >= 800 ? (N + 255) / 256 : (N + GRAPH_THREADS_ - 1) / GRAPH_THREADS_;
        g.grid = spread_grid((long)B * g.chunks);
    } else if (p.graph_q4 != 0 && N >= 64 && (p.graph_q4 == 2 || (long)B * ((N + 127) / 128) * 2 <= n_cu)) {
        // with the particle encoder in the same launch where the impulses are data (the trainer's forward pass): the lists
        // and the encoder read nothing of one another
        g.kind = (!has_actions && engine == ENGINE_FUSED && p.graph_encode && !no_encoder_launch) ? GraphPlan::Q4_ENCODE : GraphPlan::Q4;
        g.chunks = (N + 127) / 128;
        g.grid = (long)B * g.chunks;
    } else {
        g.kind = GraphPlan::PLAIN;
        g.chunks = (N + GRAPH_THREADS_ - 1) / GRAPH_THREADS_;
        g.grid = spread_grid((long)B * g.chunks);
    }
    return g;
}

// the aggregate of the engines that materialise the edge constants: a handful of samples (training batches) get several
// workgroups per sample on the global variant
struct AggPlan { int chunks; bool lds; };
inline AggPlan plan_aggregate(const DispatchPolicy& p, int n_cu, int B, int N) {
    AggPlan a{1, false};
    if (B < n_cu / 2) a.chunks = std::max(1, std::min((N + 15) / 16, 2048 / B));
    a.lds = N <= AGG_LDS_MAX_N && !p.agg_global_only && a.chunks == 1;
    return a;
}

// ---- one predict_one_step ------------------------------------------------------------------------------------------------
struct StepShape {
    int engine = ENGINE_FUSED, B = 1, N = 1;
    bool tape = false;              // the backward pass's tape is written
    int prev_mod = 1, attr_mod = 1, dens_mod = 1;   // sample b reads row b % mod of the state / attributes / densities
    bool work = false;              // the counting instantiations (drp_probe_begin("prop+work"))
    bool build_graph = true, padded = false, has_actions = false, wants_rev = false;
    DegStat deg;
};
struct StepPlan {
    int engine = ENGINE_FUSED, N = 1;   // ENGINE_LITE arrives here as ENGINE_FUSED with `lite` set
    bool tape = false, work = false, lite = false;
    GraphPlan graph;
    bool fused = false;             // the relation encoder is recomputed inside the propagation kernels (no edge-encode launch)
    bool split_encoders = false;    // the split-fp16 encoders (split and fused engines)
    bool tape_mfma = false;         // the tape beside the fp32 matrix engine's stage kernels
    bool prop3 = false, phase_e = false;   // the three propagation steps in one launch; the particle encoder as its first phase
    bool node_encode = false;       // a particle encoder launch of its own
    int spw = 1;                    // samples per workgroup of an unsplit whole-sample launch
    Blocks blocks;                  // prop3: its launches
    int spread = 0; bool pair = false; int grid = 1;   // per-step km_prop
    AggPlan agg{1, false};
    // every variant carrying out this plan launches
    void mark(unsigned char* hit) const {
        if (graph.kind != GraphPlan::NONE) hit[graph.variant()] = 1;
        if (engine == ENGINE_VALU) { hit[DV_VALU_STEP] = 1; hit[agg.lds ? DV_AGGREGATE_LDS : DV_AGGREGATE] = 1; return; }
        if (node_encode) hit[fused ? (lite ? DV_NODE_ENCODE_SPLIT_LITE : DV_NODE_ENCODE_SPLIT) : DV_NODE_ENCODE] = 1;
        if (!fused) {
            hit[split_encoders ? DV_EDGE_ENCODE_SPLIT : DV_EDGE_ENCODE] = 1;
            hit[tape_mfma ? DV_AGGREGATE_TAPE : agg.lds ? DV_AGGREGATE_LDS : DV_AGGREGATE] = 1;
            hit[DV_UPDATE] = 1;
        } else if (prop3) {
            for (int q = 0; q < blocks.n; ++q) hit[prop3_flags(blocks.block(q)).variant()] = 1;
        } else {
            hit[prop_flags(false).variant()] = 1;
            hit[prop_flags(true).variant()] = 1;
        }
    }
    PropFlags prop_flags(bool last) const { return PropFlags{last, tape, pair, work, lite}; }
    Prop3Flags prop3_flags(const Block& b) const { return Prop3Flags{tape, b.pair, b.cache, work, lite}; }
};
inline StepPlan plan_step(const DispatchPolicy& p, int n_cu, const StepShape& s) {
    StepPlan k;
    const int B = s.B, N = s.N;
    k.engine = engine_for_plan(s.engine); k.N = N; k.tape = s.tape; k.work = s.work;
    k.lite = s.engine == ENGINE_LITE && !s.tape;         // the tape is written with the full products, whatever is selected
    k.fused = k.engine == ENGINE_FUSED;
    k.split_encoders = k.fused || k.engine == ENGINE_SPLIT;
    k.tape_mfma = s.tape && k.engine == ENGINE_MFMA;
    k.agg = plan_aggregate(p, n_cu, B, N);
    // chip-filling batches on the fused engine: the three propagation steps are one launch (km_prop3: a workgroup owns whole
    // samples and barriers locally between steps), and the particle encoder is its first phase unless switched off;
    // otherwise one launch per step with the tiles of all samples dealt over the chip
    k.spw = (B + n_cu - 1) / n_cu;
    k.prop3 = k.fused && p.prop3 && detail::whole_samples(p, n_cu, B, N) && detail::tiles32((long)k.spw * N) >= p.prop3_min_tiles;
    k.phase_e = k.prop3 && p.prop3e;
    if (s.build_graph) k.graph = plan_graph(p, n_cu, k.lite ? ENGINE_LITE : k.engine, B, N, s.padded, s.has_actions, s.wants_rev, k.phase_e);
    k.node_encode = k.engine != ENGINE_VALU && !k.phase_e && k.graph.kind != GraphPlan::Q4_ENCODE;
    if (k.prop3) {
        long unit = 1;
        bool ok = true;
        for (int mod : {s.prev_mod, s.attr_mod, s.dens_mod})
            if (mod < B) { if (unit % mod != 0 && mod % unit != 0) ok = false; else unit = std::max(unit, (long)mod); }
        k.blocks = cut_blocks(p, n_cu, B, N, s.tape, unit, ok, s.deg);
    } else if (k.fused) {
        const long node_tiles = (long)B * ((N + 31) / 32);
        long pb = (node_tiles + PROP_WAVES_ - 1) / PROP_WAVES_;
        // few tiles (up to four per CU): one per workgroup first, so that a tile has its SIMD to itself
        k.spread = (p.prop_spread && node_tiles <= 4L * n_cu) ? 1 : 0;
        // fewer still (up to two per CU): tiles of 16 receivers x two slots, half the slot iterations each
        k.pair = k.spread && p.prop_pair_rows > 0 && node_tiles <= 2L * n_cu;
        if (k.spread) pb = k.pair ? (long)B * ((N + 15) / 16) : node_tiles;
        k.grid = (int)std::min(pb, (long)n_cu);
    }
    return k;
}

// ---- a rollout of H steps ----------------------------------------------------------------------------------------------
// small piles on the fused engine: the whole rollout is ONE launch per block (km_rollout, k_rollout.h) -- a workgroup owns its
// samples from the first step to the last, builds their neighbour lists itself and keeps the node matrices in LDS
struct RolloutPlan {
    bool one_launch = false;
    int spw = 1;                    // samples per workgroup of the first block
    Blocks blocks;
    bool work = false, lite = false;
    RolloutFlags flags(const Block& b) const { return RolloutFlags{b.pair, b.cache, work, lite}; }
    void mark(unsigned char* hit) const {
        if (!one_launch) return;
        hit[DV_GRAPH_IN_ROLLOUT] = 1;
        for (int q = 0; q < blocks.n; ++q) hit[flags(blocks.block(q)).variant()] = 1;
    }
};
inline RolloutPlan plan_rollout(const DispatchPolicy& p, int n_cu, int engine, int B, int N, int nb, bool work, const DegStat& deg) {
    RolloutPlan r;
    r.work = work;
    r.lite = engine == ENGINE_LITE;
    engine = engine_for_plan(engine);
    r.blocks = cut_blocks(p, n_cu, B, N, false, nb, true, deg);
    if (engine != ENGINE_FUSED) { r.blocks.cache = false; r.blocks.cache_bytes = 0; r.blocks.chunk = B; r.blocks.n = 1; }
    r.spw = (int)((std::min((long)B, r.blocks.chunk) + n_cu - 1) / n_cu);
    const long rows = (long)r.spw * N;
    // up to rollout_max_n particles whatever the batch; up to rollout_mid_n while a workgroup holds no more than rollout_mid_rows
    const bool roll_size = N <= p.rollout_max_n || (N <= p.rollout_mid_n && rows <= p.rollout_mid_rows && (N <= 200 || B >= n_cu / 2));
    r.one_launch = engine == ENGINE_FUSED && p.rollout_fused && p.prop3 && p.prop3e && roll_size && detail::whole_samples(p, n_cu, B, N) &&
                   detail::tiles32(rows) >= p.prop3_min_tiles && rows <= ROLLOUT_MAX_ROWS && rows <= p.rollout_max_rows;
    return r;
}

// ---- the backward pass of a rollout step --------------------------------------------------------------------------------
struct BwdPlan {
    enum Kind { ROWS, STEP, STAGES };
    Kind kind = STAGES;
    int spw = 1, grid = 1;
    int gps = 1;                    // ROWS: samples per group
    int variant() const { return kind == ROWS ? DV_BWD_ROWS : kind == STEP ? DV_BWD_STEP : DV_BWD_STAGES_MFMA; }
};
inline BwdPlan plan_backward(const DispatchPolicy& p, int n_cu, int B, int N) {
    BwdPlan k;
    k.spw = (B + n_cu - 1) / n_cu;
    if (p.bwd_fused && p.bwd_rows && N <= BWD_ROWS_MAX) {
        // piles of up to 256 particles: a workgroup takes groups of whole samples with at most 256 rows, a wave keeps
        // its tile's rows in registers through all phases (kmb_rows_bwd).  Samples per group: the fewest that do not
        // add a round of groups over the CUs (fewer waves at work per CU, more CUs at work)
        k.kind = BwdPlan::ROWS;
        const int g_max = BWD_ROWS_MAX / N;
        auto rounds = [&](int g) { return (((long)B + g - 1) / g + n_cu - 1) / n_cu; };
        k.gps = g_max;
        while (k.gps > 1 && rounds(k.gps - 1) == rounds(g_max)) --k.gps;
        k.grid = (int)std::min(((long)B + k.gps - 1) / k.gps, (long)n_cu);
    } else if (p.bwd_fused && detail::whole_samples(p, n_cu, B, N) && detail::tiles32((long)k.spw * N) >= p.bwd_fused_min_tiles) {
        // chip-filling batches: everything between the reward's gradient and the impulses' in one launch,
        // a workgroup owning whole samples (kmb_step_bwd)
        k.kind = BwdPlan::STEP;
        k.grid = (B + k.spw - 1) / k.spw;
    }
    return k;
}
// The trainer's node stages of a rollout step in ONE launch (kmb_step_bwd<dump>): it needs every dump in a buffer of its own
// (`defer`: the deferred weight gradients' layout).  A group of `spw` samples is shared by `parts` workgroups, the grid at
// most one workgroup per CU (the kernel's barrier in memory).  It pays for a handful of tiles only (the reference's batch of
// 4 x <= 300 particles: 40): every tile is a chain of memory round trips, and the stage kernels spread the same gathers
// over more threads (32 x 300: 2.6 ms per iteration staged, 4.3 in one launch)
struct TrainBwdPlan {
    bool fused = false, coop = false;
    int spw = 1, groups = 1, parts = 1;
    int variant() const { return !fused ? DV_TRAIN_NODE_MFMA : coop ? DV_TRAIN_NODE_FUSED_COOP : DV_TRAIN_NODE_FUSED; }
};
inline TrainBwdPlan plan_train_backward(const DispatchPolicy& p, int n_cu, int B, int N, bool defer) {
    TrainBwdPlan k;
    const long tiles = (long)B * ((N + 31) / 32);
    k.fused = defer && p.bwd_fused && (p.train_fused >= 0 ? p.train_fused != 0 : tiles <= n_cu / 4);
    k.spw = (B + n_cu - 1) / n_cu;
    k.groups = (B + k.spw - 1) / k.spw;
    if (k.fused) {
        const int group_tiles = (int)detail::tiles32((long)k.spw * N);
        k.parts = p.train_parts > 0 ? p.train_parts : n_cu / k.groups;
        k.parts = std::max(1, std::min(k.parts, std::min(n_cu / k.groups, group_tiles)));
        // a handful of tiles per workgroup: all eight waves gather a tile's edge terms (a wave on its own is one long chain of
        // L2 round trips per tile and phase: 27 us against 6); many: a tile per wave, the waves hide each other's latency
        k.coop = p.train_coop >= 0 ? p.train_coop != 0 : (group_tiles + k.parts - 1) / k.parts <= 2 * COOP_SLOTS;
    }
    return k;
}

// ---- the deferred weight gradients of a whole backward pass (capi_pipeline.h: WgradQueue::flush_all) ----------------------
// Job q is `blocks[q]` workgroups adding into target `target[q]` (any identity: the address of its dW).  A slab of partial
// sums per job; jobs of one size through one launch, the larger first (stable: queue order among equals); one reduction
// block per target, targets in first-seen order, each adding its jobs' sums in queue order.
struct WgradListPlan {
    std::vector<size_t> part_off;   // [n]: where job q's slab starts, in floats
    size_t part_floats = 0;
    std::vector<int> order;         // [n]: the jobs in launch order
    int n_targets = 0;
    std::vector<int> idx;           // what the kernels read: order[n] | tgt_off[n_targets + 1] | tgt_jobs[n]
};
inline WgradListPlan plan_wgrad_lists(const std::vector<int>& blocks, const std::vector<const void*>& target) {
    const int n = (int)blocks.size();
    WgradListPlan k;
    k.part_off.resize(n);
    for (int q = 0; q < n; ++q) { k.part_off[q] = k.part_floats; k.part_floats += (size_t)blocks[q] * 66 * 64; }
    k.order.resize(n);
    for (int q = 0; q < n; ++q) k.order[q] = q;
    std::stable_sort(k.order.begin(), k.order.end(), [&](int a, int b) { return blocks[a] > blocks[b]; });
    std::vector<const void*> targets;
    std::vector<std::vector<int>> lists;
    for (int q = 0; q < n; ++q) {
        size_t t = 0;
        while (t < targets.size() && targets[t] != target[q]) ++t;
        if (t == targets.size()) { targets.push_back(target[q]); lists.emplace_back(); }
        lists[t].push_back(q);
    }
    k.n_targets = (int)targets.size();
    k.idx = k.order;
    int off = 0;
    for (const std::vector<int>& l : lists) { k.idx.push_back(off); off += (int)l.size(); }
    k.idx.push_back(off);
    for (const std::vector<int>& l : lists) k.idx.insert(k.idx.end(), l.begin(), l.end());
    return k;
}

}  // namespace dispatch

#endif  // DRP_DISPATCH_H
