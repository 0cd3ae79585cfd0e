// Host-only driver of csrc/dispatch.h for tests/test_dispatch_plan.py: built with the host compiler alone (-Wall -Werror, no HIP
// header in reach), it answers what the library would launch from the plan functions.
//   dispatch_dump table FILE n_cu     every step / rollout / mppi / gd line of FILE (tools/dispatch_table.py's format) with the names
//                                     the plans give, policy from the environment
//   dispatch_dump pair spw N B [sum rows n]      paired tiles?  (no statistic given: unknown)
//   dispatch_dump cache n_cu          N B nb step-cached rollout-cached, for N = 1 ... 300 and a set of batches
//   dispatch_dump blocks n_cu B N nb H tape    how km_prop3's launches of every rollout step t < H of a gd / rollout call are cut
//                                     (plan_step; tape: 0 / 1): per step a line "step t prop3 cache n chunk cache_bytes" and a line
//                                     "block q b_off Bc spw grid pair cache ec_stride cache_bytes" per launch
//   dispatch_dump policy              every policy field, from the environment
//   dispatch_dump env                 the names of the environment table
//   dispatch_dump wgrad b0 t0 b1 t1 ...       the deferred weight gradients' lists (plan_wgrad_lists) for jobs of b_q blocks adding
//                                     into target t_q: the lines part_off, part_floats, order, n_targets, idx
#include <cstdint>
#include <cstring>
#include <set>
#include <string>

#include "../dyn_res_pile_manip_amd/csrc/dispatch.h"

using namespace dispatch;

static void step(const DispatchPolicy& p, int n_cu, unsigned char* hit, int engine, int B, int N, int mod0, int mod, bool tape, bool has_actions,
                 bool wants_rev, bool* rev_built) {
    StepShape s;
    s.engine = engine; s.B = B; s.N = N; s.tape = tape;
    s.prev_mod = mod0; s.attr_mod = mod; s.dens_mod = mod;
    s.has_actions = has_actions; s.wants_rev = wants_rev;
    const StepPlan k = plan_step(p, n_cu, s);
    k.mark(hit);
    if (rev_built) *rev_built = k.graph.kind == GraphPlan::REV;
}

// what an entry point of include/drp.h launches around its steps
static void entry(const DispatchPolicy& p, int n_cu, unsigned char* hit, int engine, const std::string& what, int B, int N, int nb, int H) {
    if (what == "step") {
        step(p, n_cu, hit, engine, B, N, B, B, false, false, false, nullptr);
    } else if (what == "rollout" || what == "mppi") {
        const RolloutPlan r = plan_rollout(p, n_cu, engine, B, N, nb, false, DegStat{});
        r.mark(hit);
        for (int t = 0; t < H && !r.one_launch; ++t) step(p, n_cu, hit, engine, B, N, t == 0 ? nb : B, nb, false, true, false, nullptr);
        hit[DV_REWARD] = 1;
        if (what == "mppi") hit[DV_MPPI_SOFTMAX] = 1;
    } else if (what == "gd") {
        // the tape is written by the fused engine unless an fp32 engine is selected (pick_tape_engine)
        const int tape_engine = (engine == ENGINE_MFMA || engine == ENGINE_VALU) ? ENGINE_MFMA : ENGINE_FUSED;
        bool rev_built = false;
        for (int t = 0; t < H; ++t) step(p, n_cu, hit, tape_engine, B, N, t == 0 ? nb : B, nb, true, true, H == 1, &rev_built);
        hit[DV_BWD_REWARD] = 1;
        if (!rev_built) hit[N <= 512 ? DV_REV_256 : DV_REV_1024] = 1;
        hit[plan_backward(p, n_cu, B, N).variant()] = 1;
        if (H > 1) hit[DV_BWD_EDGE_MFMA] = 1;
    }
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    const DispatchPolicy p = policy_from_env();
    if (mode == "table" && argc == 4) {
        FILE* f = fopen(argv[2], "r");
        if (!f) return 2;
        const int n_cu = atoi(argv[3]);
        char line[4096], eng[16], what[16];
        while (fgets(line, sizeof(line), f)) {
            int B, N, nb, H;
            if (sscanf(line, "%15s %15s B=%d N=%d nb=%d H=%d", eng, what, &B, &N, &nb, &H) != 6 || !strcmp(what, "train")) continue;
            const char* const engines[4] = {"valu", "mfma", "split", "fused"};
            int engine = -1;
            for (int q = 0; q < 4; ++q) if (!strcmp(eng, engines[q])) engine = q;
            unsigned char hit[DV_COUNT] = {};
            entry(p, n_cu, hit, engine, what, B, N, nb, H);
            std::set<std::string> names;
            for (int id = 0; id < DV_COUNT; ++id)
                if (hit[id]) { char name[96]; dv_name(id, name, sizeof(name), nullptr); names.insert(name); }
            printf("%s %s B=%d N=%d nb=%d H=%d ->", eng, what, B, N, nb, H);
            const char* sep = " ";
            for (const std::string& s : names) { printf("%s%s", sep, s.c_str()); sep = " | "; }
            printf("\n");
        }
        fclose(f);
    } else if (mode == "pair" && (argc == 5 || argc == 8)) {
        DegStat d;
        if (argc == 8) { d.have = true; d.sum = atol(argv[5]); d.rows = atol(argv[6]); d.n = atol(argv[7]); }
        printf("%d\n", pair_rule(p)(d, atol(argv[2]), atol(argv[3]), atol(argv[4])) ? 1 : 0);
    } else if (mode == "cache" && argc == 3) {
        const int n_cu = atoi(argv[2]);
        for (int N = 1; N <= 300; ++N)
            for (int B : {8, 64, 240, 1024, 1500, 4096, 8192})
                for (int nb : {1, 2, 8}) {
                    StepShape s;
                    s.B = B; s.N = N; s.prev_mod = B; s.attr_mod = nb; s.dens_mod = nb;
                    const StepPlan k = plan_step(p, n_cu, s);
                    const RolloutPlan r = plan_rollout(p, n_cu, ENGINE_FUSED, B, N, nb, false, DegStat{});
                    printf("%d %d %d %d %d\n", N, B, nb, k.prop3 ? (k.blocks.cache ? 1 : 0) : -1, r.one_launch ? (r.blocks.cache ? 1 : 0) : -1);
                }
    } else if (mode == "blocks" && argc == 8) {
        const int n_cu = atoi(argv[2]), B = atoi(argv[3]), N = atoi(argv[4]), nb = atoi(argv[5]), H = atoi(argv[6]);
        const bool tape = atoi(argv[7]) != 0;
        for (int t = 0; t < H; ++t) {
            StepShape s;
            s.B = B; s.N = N; s.tape = tape; s.has_actions = true; s.wants_rev = tape && H == 1;
            s.prev_mod = t == 0 ? nb : B; s.attr_mod = nb; s.dens_mod = nb;
            const StepPlan k = plan_step(p, n_cu, s);
            printf("step %d %d %d %d %ld %zu\n", t, k.prop3 ? 1 : 0, k.blocks.cache ? 1 : 0, k.blocks.n, k.blocks.chunk, k.blocks.cache_bytes);
            for (int q = 0; k.prop3 && q < k.blocks.n; ++q) {
                const Block b = k.blocks.block(q);
                printf("block %d %ld %d %d %d %d %d %zu %zu\n", q, b.b_off, b.Bc, b.spw, b.grid, b.pair ? 1 : 0, b.cache, b.ec_stride, b.cache_bytes);
            }
        }
    } else if (mode == "policy") {
#define FIELD(NAME) printf(#NAME "=%g\n", (double)p.NAME)
        FIELD(agg_global_only); FIELD(rev_global_only); FIELD(self_const); FIELD(prop3); FIELD(prop3_min_b); FIELD(prop3_min_tiles);
        FIELD(bwd_fused_min_tiles); FIELD(graph_cells); FIELD(graph_cells_min_n); FIELD(graph_cells_halo); FIELD(graph_cells_hb);
        FIELD(graph_strips); FIELD(bwd_fused); FIELD(graph_rev); FIELD(graph_encode); FIELD(train_fused); FIELD(train_coop);
        FIELD(train_parts); FIELD(bwd_rows); FIELD(prop3_order); FIELD(prop_pair_rows); FIELD(prop_pair_always); FIELD(prop_pair_deg10);
        FIELD(prop3e); FIELD(rollout_fused); FIELD(rollout_max_n); FIELD(rollout_mid_n); FIELD(rollout_mid_rows); FIELD(rollout_max_rows);
        FIELD(ecache_max_mb); FIELD(ecache_hard_max_mb); FIELD(ecache_max_n); FIELD(ecache_full_n); FIELD(ecache_tape_max_n);
        FIELD(graph_q4); FIELD(wgrad_mfma); FIELD(prop_spread);
#undef FIELD
    } else if (mode == "env") {
        int n = 0;
        const EnvSwitch* t = env_switches(&n);
        for (int q = 0; q < n; ++q) printf("%s\n", t[q].name);
    } else if (mode == "wgrad" && argc >= 4 && argc % 2 == 0) {
        std::vector<int> blocks;
        std::vector<const void*> target;
        for (int q = 2; q < argc; q += 2) {
            blocks.push_back(atoi(argv[q]));
            target.push_back(reinterpret_cast<const void*>((uintptr_t)atol(argv[q + 1])));
        }
        const WgradListPlan k = plan_wgrad_lists(blocks, target);
        printf("part_off");
        for (size_t v : k.part_off) printf(" %zu", v);
        printf("\npart_floats %zu\norder", k.part_floats);
        for (int v : k.order) printf(" %d", v);
        printf("\nn_targets %d\nidx", k.n_targets);
        for (int v : k.idx) printf(" %d", v);
        printf("\n");
    } else {
        return 2;
    }
    return 0;
}
