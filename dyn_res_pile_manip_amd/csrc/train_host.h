// train_host.h -- the trainer's entry points' host arithmetic that touches no device: the description of a loss (TrLoss), the table
// of the blocks a trainer call stages and brings back (tr_blocks) with the one carve, staging copy, readback and device view over
// it, the one-shots' buffers, and which pushes, seeds, reaches and matchings a call refuses.  Plain C++ (no HIP header), so that
// tools/train_host_check.cpp builds it alone under the host sanitizers; drp_capi.hip includes it ahead of the C ABI's sections.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/drp.h"

// what seeds the reverse pass: the tracked loss (kt_mse_grad against the given next states) or the Chamfer loss against
// untracked target clouds (k_chamfer.h), the one-to-one matching loss against them (k_match.h), or the two mixed; the targets as
// the HOST gave them (the entry point stages them behind the batch).  The kinds beyond the MSE are include/drp.h's DRP_LOSS_*.
// The float64 yardstick (capi_grad_f64.h) reads the same description; it has every kind but the transport loss.
// TR_LOSS_TRANSPORT (k_sinkhorn.h) is internal: drp_train_step_transport's, no loss_kind of drp_train_step_loss; so is
// TR_LOSS_DIVERGENCE (k_sinkhorn.h), drp_train_step_divergence's, and TR_LOSS_GIVEN: no loss at all but the CALLER's d loss / d
// s_pred as the seed (drp_train_step_seeded, drp_train_grad_f64_seeded; kt_seed_given, k64_seed_given)
enum { TR_LOSS_MSE = 0, TR_LOSS_CHAMFER = DRP_LOSS_CHAMFER, TR_LOSS_MATCH = DRP_LOSS_MATCH, TR_LOSS_CHAMFER_MATCH = DRP_LOSS_CHAMFER_MATCH,
       TR_LOSS_TRANSPORT = 4, TR_LOSS_DIVERGENCE = 5, TR_LOSS_GIVEN = 6 };
// the predicates of a loss that decide which blocks a call has (TrLoss::shape; tools/train_host_check.cpp sets them freely)
struct TrShape { bool targeted, chamfer, match, match_in, sinkhorn, divergence, unbalanced, given; int M; };
struct TrLoss {
    int kind = TR_LOSS_MSE;
    const float* targets = nullptr;         // [B][H][M][3]
    const int32_t* target_nums = nullptr;   // [B][H]
    int M = 0;
    double match_weight = 0.0;              // TR_LOSS_CHAMFER_MATCH: (1 - w) Chamfer + w matching
    int32_t* match_out = nullptr;           // the caller's [H][B][N], nullable: every predicted row's partner (kinds with a matching)
    const int32_t* match_in = nullptr;      // float64 only: the caller's [H][B][N], nullable: the pairs of the term and the seed
    double* cost_out = nullptr;             // float64 only: the caller's [H][B][2], nullable (ka64_match's costs)
    double* margin_out = nullptr;           // float64 only: the caller's [H][B], nullable (kc64_chamfer's arg-min margins)
    const double* eps = nullptr;            // TR_LOSS_TRANSPORT, _DIVERGENCE: the caller's [B], the regularisation of every step of a sample
    int iters = 0;                          // TR_LOSS_TRANSPORT, _DIVERGENCE: the sweeps
    double* col_err_out = nullptr;          // TR_LOSS_TRANSPORT, _DIVERGENCE: the caller's [H][B], nullable
    double* self_err_out = nullptr;         // TR_LOSS_DIVERGENCE: the caller's [H][B][2], nullable
    const double* rho = nullptr;            // TR_LOSS_DIVERGENCE, non-null: the unbalanced divergence -- the caller's reaches [B] ...
    const double* mass_q = nullptr;         //   ... and the targets' total masses [H][B] (both or neither)
    double* transported_out = nullptr;      //   ... and the caller's [H][B], nullable
    const float* seed = nullptr;            // TR_LOSS_GIVEN: the caller's d loss / d s_pred [B][H][N][3] ...
    const double* seed64 = nullptr;         //   ... float64: the same in double
    bool given() const { return kind == TR_LOSS_GIVEN; }
    bool targeted() const { return kind != TR_LOSS_MSE && kind != TR_LOSS_GIVEN; }     // a loss against target clouds
    bool unbalanced() const { return kind == TR_LOSS_DIVERGENCE && rho != nullptr; }
    bool transport() const { return kind == TR_LOSS_TRANSPORT; }
    bool divergence() const { return kind == TR_LOSS_DIVERGENCE; }
    bool sinkhorn() const { return transport() || divergence(); }      // eps and iters, the kernels' caps and col_err
    bool chamfer() const { return kind == TR_LOSS_CHAMFER || kind == TR_LOSS_CHAMFER_MATCH; }
    bool match() const { return kind == TR_LOSS_MATCH || kind == TR_LOSS_CHAMFER_MATCH; }
    TrShape shape() const {
        return TrShape{targeted(), chamfer(), match(), match() && match_in != nullptr, sinkhorn(), divergence(), unbalanced(), given(), M};
    }
    static TrLoss against(int kind, const float* targets, const int32_t* target_nums, int M) {
        TrLoss lk;
        lk.kind = kind; lk.targets = targets; lk.target_nums = target_nums; lk.M = M;
        return lk;
    }
    // the transport loss and the divergence: `against` with the sweeps' arguments and the certificates' outputs (nullable)
    static TrLoss sinkhorn(int kind, const float* targets, const int32_t* target_nums, int M, const double* eps, int iters,
                           double* col_err_out, double* self_err_out = nullptr) {
        TrLoss lk = against(kind, targets, target_nums, M);
        lk.eps = eps; lk.iters = iters; lk.col_err_out = col_err_out; lk.self_err_out = self_err_out;
        return lk;
    }
};

// ---- the blocks of a trainer call: ONE table for the fp32 trainer (capi_train.h) and its float64 yardstick (capi_grad_f64.h) ----
// A row is a block: its id, its element size and its count, each count written once, here.  Rows in the order they lie:
//   the fixed five      states [B][H+1][N][3] | impulses [B][H][N][3] (`actions`: the pushes [B][H][4]) | attributes [B][H+1][N]
//                       (float64: a_cur = attrs[:, 0] alone, [B][N]) | densities [B] | particle counts [B] (ints)
//   the loss's inputs   target clouds [B][H][M][3] | their counts [B][H] (targeted) | eps [B] (sinkhorn) | rho [B] | mass_q [H][B]
//                       (sinkhorn and unbalanced: a reach without eps adds nothing) | the caller's partners [H][B][N] (float64 with
//                       a match_in) | the caller's d loss / d s_pred [B][H][N][3] (given; floats, float64: doubles)
//   the results         terms [H][B] | the float64 weight-gradient sums [DRP_N_WEIGHTS] (no result of the loss: they lie between
//                       the terms and the rest) | margin [H][B] (float64 Chamfer) | col_err [H][B] (sinkhorn) | self_err [H][B][2]
//                       (divergence) | transported [H][B] (unbalanced) | cost [H][B][2] (float64 match) | partners [H][B][N] (match)
//   the scratch         the divergence's value sums [3][H][B] | gradient sums [2][H][B][N][3]: behind the fp32 trainer's results;
//                       the float64 yardstick carves them per chunk (Tr64Ws, from the same two rows at B = the chunk's samples)
// Inputs and results are carved apart (tr_carve): every block on a multiple of 16 bytes of its buffer, so every double on one of
// 8 and the fp32 arena, which kt_unpack_inputs copies in float4 units, a multiple of 16 long; a block that is absent (count 0)
// takes no byte, has offset 0 and a null address in the view, and moves nothing ahead of it.
enum { TRB_STATES, TRB_IMPULSES, TRB_ATTRS, TRB_DENS, TRB_NUMS,
       TRB_TARGETS, TRB_TNUMS, TRB_EPS, TRB_RHO, TRB_MASS_Q, TRB_MATCH_IN, TRB_SEED,
       TRB_TERMS, TRB_TOTAL, TRB_MARGIN, TRB_COL_ERR, TRB_SELF_ERR, TRB_TRANSPORTED, TRB_COST, TRB_MATCH,
       TRB_VALS, TRB_GSUM, TRB_COUNT, TRB_IN_END = TRB_TERMS, TRB_SCRATCH = TRB_VALS };
struct TrBlocks {
    size_t elem[TRB_COUNT], count[TRB_COUNT], off[TRB_COUNT];
    size_t bytes, res_bytes;        // the staged inputs; the results (fp32: with the scratch)
    int res_end;                    // the first row behind the carved results
    size_t size(int id) const { return elem[id] * count[id]; }
};
// rows [first, end) laid one behind the other from offset 0 -> the bytes they take
inline size_t tr_carve(TrBlocks& t, int first, int end) {
    size_t at = 0;
    for (int id = first; id < end; ++id) {
        t.off[id] = t.count[id] ? at : 0;
        at = (at + t.size(id) + 15) & ~(size_t)15;
    }
    return at;
}
inline TrBlocks tr_blocks(const TrShape& s, int B, int H, int N, bool actions, bool f64) {
    const size_t F = sizeof(float), I = sizeof(int32_t), D = sizeof(double);
    const size_t b = (size_t)B, hb = (size_t)H * B, hbn = hb * N, m = s.targeted ? (size_t)s.M : 0;
    const bool reach = s.sinkhorn && s.unbalanced, div = s.sinkhorn && s.divergence;
    TrBlocks t{};
    auto row = [&t](int id, size_t elem, size_t count) { t.elem[id] = elem; t.count[id] = count; };
    row(TRB_STATES, F, b * (H + 1) * N * 3);
    row(TRB_IMPULSES, F, actions ? hb * 4 : hbn * 3);
    row(TRB_ATTRS, F, f64 ? b * N : b * (H + 1) * N);
    row(TRB_DENS, F, b);
    row(TRB_NUMS, I, b);
    row(TRB_TARGETS, F, hb * m * 3);
    row(TRB_TNUMS, I, m ? hb : 0);
    row(TRB_EPS, D, s.sinkhorn ? b : 0);
    row(TRB_RHO, D, reach ? b : 0);
    row(TRB_MASS_Q, D, reach ? hb : 0);
    row(TRB_MATCH_IN, I, f64 && s.match_in ? hbn : 0);
    row(TRB_SEED, f64 ? D : F, s.given ? hbn * 3 : 0);
    row(TRB_TERMS, D, hb);
    row(TRB_TOTAL, D, f64 ? DRP_N_WEIGHTS : 0);
    row(TRB_MARGIN, D, f64 && s.chamfer ? hb : 0);
    row(TRB_COL_ERR, D, s.sinkhorn ? hb : 0);
    row(TRB_SELF_ERR, D, div ? 2 * hb : 0);
    row(TRB_TRANSPORTED, D, div && reach ? hb : 0);
    row(TRB_COST, D, f64 && s.match ? 2 * hb : 0);
    row(TRB_MATCH, I, s.match ? hbn : 0);
    row(TRB_VALS, D, div ? 3 * hb : 0);
    row(TRB_GSUM, D, div ? 2 * hbn * 3 : 0);
    t.bytes = tr_carve(t, TRB_STATES, TRB_IN_END);
    t.res_end = f64 ? TRB_SCRATCH : TRB_COUNT;
    t.res_bytes = tr_carve(t, TRB_TERMS, t.res_end);
    return t;
}
// the loss's input rows copied from the caller's arrays to their places in the staged batch at `dst`
inline void tr_stage_loss_inputs(char* dst, const TrBlocks& t, const TrLoss& lk) {
    const void* src[TRB_IN_END] = {};
    src[TRB_TARGETS] = lk.targets; src[TRB_TNUMS] = lk.target_nums; src[TRB_EPS] = lk.eps; src[TRB_RHO] = lk.rho;
    src[TRB_MASS_Q] = lk.mass_q; src[TRB_MATCH_IN] = lk.match_in;
    src[TRB_SEED] = t.elem[TRB_SEED] == sizeof(double) ? static_cast<const void*>(lk.seed64) : lk.seed;
    for (int id = TRB_TARGETS; id < TRB_IN_END; ++id)
        if (t.count[id]) memcpy(dst + t.off[id], src[id], t.size(id));
}
// every result row behind the terms and the sums that the caller gave a pointer for: copy(dst, src, bytes) -> 0 or the error
// that ends the walk (the trainers: a d2h on the stream).  The terms stay with the trainers: they differ in where those land
template <typename Copy>
inline int tr_read_results(const TrBlocks& t, const void* res, const TrLoss& lk, Copy copy) {
    void* dst[TRB_COUNT] = {};
    dst[TRB_MARGIN] = lk.margin_out; dst[TRB_COL_ERR] = lk.col_err_out; dst[TRB_SELF_ERR] = lk.self_err_out;
    dst[TRB_TRANSPORTED] = lk.transported_out; dst[TRB_COST] = lk.cost_out; dst[TRB_MATCH] = lk.match_out;
    for (int id = TRB_MARGIN; id < TRB_SCRATCH; ++id)
        if (t.count[id] && dst[id])
            if (const int rc = copy(dst[id], static_cast<const char*>(res) + t.off[id], t.size(id))) return rc;
    return 0;
}
// the addresses of the loss's blocks: `in` the staged batch, `res` the results; null where a block is absent
struct TrView {
    const float* targets; const int32_t* tnums; const double *eps, *rho, *mass_q; const int32_t* match_in; const void* seed;
    double *terms, *total, *margin, *col_err, *self_err, *transported, *cost; int32_t* match; double *vals, *gsum;
};
inline TrView tr_view(const void* in, void* res, const TrBlocks& t) {
    auto at = [&t](const void* base, int id) -> void* {
        return t.count[id] && id < t.res_end ? const_cast<char*>(static_cast<const char*>(base)) + t.off[id] : nullptr;
    };
    auto f64 = [&](int id) { return static_cast<double*>(at(id < TRB_IN_END ? in : res, id)); };
    auto i32 = [&](int id) { return static_cast<int32_t*>(at(id < TRB_IN_END ? in : res, id)); };
    return TrView{static_cast<const float*>(at(in, TRB_TARGETS)), i32(TRB_TNUMS), f64(TRB_EPS), f64(TRB_RHO), f64(TRB_MASS_Q),
                  i32(TRB_MATCH_IN), at(in, TRB_SEED), f64(TRB_TERMS), f64(TRB_TOTAL), f64(TRB_MARGIN), f64(TRB_COL_ERR),
                  f64(TRB_SELF_ERR), f64(TRB_TRANSPORTED), f64(TRB_COST), i32(TRB_MATCH), f64(TRB_VALS), f64(TRB_GSUM)};
}


// The one buffer of a one-shot on two clouds (capi_pipeline.h: cloud_begin), every block 16-byte aligned.  Up: p [B][N][3]
// (elements of p_elem bytes: floats, or the float64 divergence's doubles) | q [B][M][3] | n_p [B] | n_q [B] (ints); down, behind
// `in_bytes`: the call's n_out output blocks out[k] of out_bytes[k] each
#define CLOUD_MAX_OUT 5
struct CloudLayout { size_t p_elem, pts_p, pts_q, n_p, n_q, in_bytes, out[CLOUD_MAX_OUT], out_bytes[CLOUD_MAX_OUT], bytes; int n_out; };
inline CloudLayout cloud_layout(int B, int N, int M, const size_t (&out_bytes)[CLOUD_MAX_OUT], size_t p_elem = sizeof(float)) {
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    CloudLayout a{};
    a.p_elem = p_elem;
    a.pts_p = 0;
    a.pts_q = up(a.pts_p + (size_t)B * N * 3 * p_elem);
    a.n_p = up(a.pts_q + (size_t)B * M * 3 * sizeof(float));
    a.n_q = up(a.n_p + (size_t)B * sizeof(int32_t));
    a.bytes = a.in_bytes = up(a.n_q + (size_t)B * sizeof(int32_t));
    for (int k = 0; k < CLOUD_MAX_OUT && out_bytes[k] > 0; ++k) {
        a.out[k] = a.bytes;
        a.out_bytes[k] = out_bytes[k];
        a.bytes = up(a.bytes + out_bytes[k]);
        a.n_out = k + 1;
    }
    return a;
}
// the three callers' output blocks, with bn = B N, bm = B M.  drp_cloud_chamfer: terms [B][2] (doubles) | gradient [B][N][3] |
// a(.) [B][N] | c(.) [B][M] (ints)
inline CloudLayout chamfer_layout(int B, int N, int M) {
    const size_t bn = (size_t)B * N, bm = (size_t)B * M;
    return cloud_layout(B, N, M, {(size_t)B * 2 * sizeof(double), bn * 3 * sizeof(float), bn * sizeof(int32_t), bm * sizeof(int32_t), 0});
}
// drp_cloud_chamfer_f64: terms [B][2] | margins [B][2] | gradient [B][N][3] (doubles) | a(.) [B][N] | c(.) [B][M] (ints)
inline CloudLayout chamfer64_layout(int B, int N, int M) {
    const size_t bn = (size_t)B * N, bm = (size_t)B * M;
    return cloud_layout(B, N, M, {(size_t)B * 2 * sizeof(double), (size_t)B * 2 * sizeof(double), bn * 3 * sizeof(double),
                                  bn * sizeof(int32_t), bm * sizeof(int32_t)});
}
// drp_cloud_match: terms [B] (doubles) | gradient [B][N][3] | partner of every row of p [B][N] | of q [B][M] (ints) | duals
// [B][N + M] (doubles)
inline CloudLayout cm_layout(int B, int N, int M) {
    const size_t bn = (size_t)B * N, bm = (size_t)B * M;
    return cloud_layout(B, N, M, {(size_t)B * sizeof(double), bn * 3 * sizeof(float), bn * sizeof(int32_t), bm * sizeof(int32_t),
                                  (bn + bm) * sizeof(double)});
}
// drp_cloud_transport: terms [B] (doubles) | gradient [B][N][3] | duals [B][N + M] | col_err [B] (doubles) | eps [B] (doubles): the
// last block goes UP behind cloud_begin's copy and is never read back
inline CloudLayout transport_layout(int B, int N, int M) {
    const size_t bn = (size_t)B * N, bm = (size_t)B * M;
    return cloud_layout(B, N, M, {(size_t)B * sizeof(double), bn * 3 * sizeof(float), (bn + bm) * sizeof(double),
                                  (size_t)B * sizeof(double), (size_t)B * sizeof(double)});
}
// drp_cloud_divergence: terms [B] (doubles) | gradient [B][N][3] | duals [B][2N + 2M] | col_err [B] | self_err [B][2] (doubles) come
// back; behind them, never read back: eps [B] (doubles, UP behind cloud_begin's copy) | the kernels' scratch: the value sums
// [3][B] | the gradient sums [2][B][N][3] (doubles).  drp_cloud_divergence_unbalanced (`reach`): rho [B] | mass_q [B] (doubles) lie
// side by side with eps -- the three go UP in one copy -- ahead of the scratch, and transported [B] (doubles, comes back by a copy
// of its own: a sixth output) behind it; the five blocks that come back and eps stay where they are without it.
// drp_cloud_divergence_f64 and its unbalanced twin: the same blocks with p and the gradient as doubles (p_elem 8).  Every block
// starts on a multiple of 16 bytes or, within eps | rho | mass_q, of 8: no double is misaligned
struct DivLayout { CloudLayout cloud; size_t eps, rho, mass_q, vals, gsum, transported; };
inline DivLayout divergence_layout(int B, int N, int M, bool reach = false, size_t p_elem = sizeof(float)) {
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t bn = (size_t)B * N, bm = (size_t)B * M, b8 = (size_t)B * sizeof(double);
    DivLayout a{};
    a.cloud = cloud_layout(B, N, M, {b8, bn * 3 * p_elem, 2 * (bn + bm) * sizeof(double), b8, 2 * b8}, p_elem);
    a.eps = a.cloud.bytes;
    size_t end = a.eps + b8;
    if (reach) {
        a.rho = end;
        a.mass_q = a.rho + b8;
        end = a.mass_q + b8;
    }
    a.vals = up(end);
    a.gsum = up(a.vals + 3 * b8);
    a.cloud.bytes = up(a.gsum + 2 * bn * 3 * sizeof(double));
    if (reach) {
        a.transported = a.cloud.bytes;
        a.cloud.bytes = up(a.transported + b8);
    }
    return a;
}
// drp_cloud_match_f64: a buffer of its own (an optional sixth input, six outputs: more than CloudLayout holds).  Up, in one copy: p [B][N][3] (doubles) | q [B][M][3]
// | n_p [B] | n_q [B] | with `match_in` the caller's partners [B][N] (ints); down, behind `in_bytes`: terms [B] | gradient [B][N][3]
// (doubles) | partner of every row of p [B][N] | of q [B][M] (ints) | duals [B][N + M] | costs [B][2] (doubles) (out[0..6)).  Every
// block 16-byte aligned
struct Match64Layout { size_t pts_p, pts_q, n_p, n_q, match_in, in_bytes, out[6], out_bytes[6], bytes; };
inline Match64Layout match64_layout(int B, int N, int M, bool match_in) {
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t bn = (size_t)B * N, bm = (size_t)B * M;
    Match64Layout a{};
    a.pts_p = 0;
    a.pts_q = up(a.pts_p + bn * 3 * sizeof(double));
    a.n_p = up(a.pts_q + bm * 3 * sizeof(float));
    a.n_q = up(a.n_p + (size_t)B * sizeof(int32_t));
    a.match_in = up(a.n_q + (size_t)B * sizeof(int32_t));
    a.bytes = a.in_bytes = match_in ? up(a.match_in + bn * sizeof(int32_t)) : a.match_in;
    const size_t ob[6] = {(size_t)B * sizeof(double), bn * 3 * sizeof(double), bn * sizeof(int32_t), bm * sizeof(int32_t),
                          (bn + bm) * sizeof(double), (size_t)B * 2 * sizeof(double)};
    for (int k = 0; k < 6; ++k) {
        a.out[k] = a.bytes;
        a.out_bytes[k] = ob[k];
        a.bytes = up(a.bytes + ob[k]);
    }
    return a;
}
// A matching given by the caller (drp_cloud_match_f64, drp_train_grad_f64_match): match [N] has the partner in q of every row of p,
// or -1.  It must be a one-to-one matching of exactly r = min(n_p, n_q) of p's n_p real rows into 0..n_q-1 with no partner on a
// padded row -> MATCH_OK, or what is wrong with *row_out, the first row at fault (MATCH_FEW: the first real row without a partner)
enum { MATCH_OK = 0, MATCH_RANGE = 1, MATCH_DUP = 2, MATCH_PAD = 3, MATCH_FEW = 4 };
inline int check_matching(const int32_t* match, int n_p, int n_q, int N, int* row_out) {
    std::vector<char> taken((size_t)(n_q > 0 ? n_q : 0), 0);
    const int r = n_p < n_q ? n_p : n_q;
    int pairs = 0, first_free = -1;
    for (int i = 0; i < N; ++i) {
        const int32_t j = match[i];
        *row_out = i;
        if (j < -1 || j >= n_q) return MATCH_RANGE;
        if (j < 0) {
            if (i < n_p && first_free < 0) first_free = i;
            continue;
        }
        if (i >= n_p) return MATCH_PAD;
        if (taken[(size_t)j]) return MATCH_DUP;
        taken[(size_t)j] = 1;
        ++pairs;
    }
    *row_out = first_free;
    return pairs == r ? MATCH_OK : MATCH_FEW;
}
inline const char* matching_fault(int why) {
    return why == MATCH_RANGE ? "has a partner out of range" : why == MATCH_DUP ? "has a partner another row has"
         : why == MATCH_PAD ? "is padding and has a partner" : "has no partner: too few pairs";
}

// the first of the B regularisation strengths that is zero, negative, infinite or no number, or -1
inline int first_bad_eps(const double* eps, int B) {
    for (int b = 0; b < B; ++b)
        if (!(eps[b] > 0.0) || !std::isfinite(eps[b])) return b;
    return -1;
}
// the first coordinate of a seed [B][H][N][3] (drp_train_step_seeded's d loss / d s_pred, the caller's layout) on a real row -- row
// n < counts[b] of every step -- that is infinite or no number, as (b * H + t) * N + row, or -1 (the padded rows are never read as
// numbers: rubbish there is allowed); T: float, or drp_train_grad_f64_seeded's double
template <typename T>
inline long first_bad_seed(const T* seed, const int32_t* counts, int B, int H, int N) {
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < H; ++t)
            for (int i = 0; i < counts[b] && i < N; ++i)
                for (int d = 0; d < 3; ++d)
                    if (!std::isfinite(seed[(((size_t)b * H + t) * N + i) * 3 + d])) return ((long)b * H + t) * N + i;
    return -1;
}
// the planner's seed [B][H][N][3] (drp_gd_grad_seeded's d loss / d s_pred; no padding: every row is a particle): the first
// coordinate that is infinite or no number, as (b * H + t) * N + row, or -1 -- first_nonfinite_row over the B * H blocks
template <typename T>
inline long first_bad_plan_seed(const T* seed, int B, int H, int N) {
    for (size_t r = 0; r < (size_t)B * H * N; ++r)
        for (int d = 0; d < 3; ++d)
            if (!std::isfinite(seed[r * 3 + d])) return (long)r;
    return -1;
}
// the unbalanced divergence's reach and target mass of one problem (include/drp.h: drp_cloud_divergence_unbalanced): 0 where it
// is served, else what is refused
enum { REACH_OK = 0, REACH_RHO = 1, REACH_MASS = 2, REACH_INF_MASS = 3 };
#define KD_MIN_REACH_PER_EPS (1.0 / 1024.0)
#define KD_MIN_MASS 0.125
#define KD_MAX_MASS 8.0
inline int check_reach(double eps, double rho, double mass_q) {
    const bool inf = rho == INFINITY;
    if (!inf && !(std::isfinite(rho) && rho >= eps * KD_MIN_REACH_PER_EPS)) return REACH_RHO;      // (NaN, <= 0 and -inf too)
    if (!(mass_q >= KD_MIN_MASS && mass_q <= KD_MAX_MASS)) return REACH_MASS;
    if (inf && mass_q != 1.0) return REACH_INF_MASS;
    return REACH_OK;
}
// the first of the real rows' coordinates of a padded cloud batch [B][N][3] that is infinite or no number, as b * N + row, or -1
// (the padding is never read as points: rubbish there is allowed); T: float, or drp_cloud_divergence_f64's double
template <typename T>
inline long first_nonfinite_row(const T* x, const int32_t* counts, int B, int N) {
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < counts[b] && i < N; ++i)
            for (int d = 0; d < 3; ++d)
                if (!std::isfinite(x[((size_t)b * N + i) * 3 + d])) return (long)b * N + i;
    return -1;
}

// the length of a push (sx, sy, ex, ey) in the camera frame, with push_frame's operations (k_graph.h: the same fmaf chain,
// division and sum, no contraction); m: the 3x4 world -> camera map, gs: global_scale
inline float push_len_host(const float* m, float gs, const float* act) {
#pragma clang fp contract(off)
    float p[2][3];
    for (int e = 0; e < 2; ++e)
        for (int r = 0; r < 3; ++r)
            p[e][r] = fmaf(m[r * 4 + 2], -act[e * 2 + 1], fmaf(m[r * 4 + 1], 0.0f, fmaf(m[r * 4 + 0], act[e * 2], m[r * 4 + 3]))) / gs;
    const float vx = p[1][0] - p[0][0], vy = p[1][1] - p[0][1], vz = p[1][2] - p[0][2];
    return sqrtf(vx * vx + vy * vy + vz * vz);
}
// the first of n pushes [n][4] whose length is zero, infinite or no number -- what would put 0 / 0 into every impulse of its step
// (planners.py:240) and from there into every weight -- or -1; *len_out: that length
inline long first_bad_push(const float* m, float gs, const float* actions, size_t n, float* len_out) {
    for (size_t e = 0; e < n; ++e) {
        const float len = push_len_host(m, gs, actions + e * 4);
        if (!(len > 0.0f) || len == INFINITY) {
            *len_out = len;
            return (long)e;
        }
    }
    return -1;
}
