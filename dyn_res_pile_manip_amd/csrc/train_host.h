// train_host.h -- the trainer's entry points' host arithmetic that touches no device: where a staged batch's blocks lie, and which
// pushes a call refuses.  Plain C++ (no HIP header), so that tools/train_host_check.cpp builds it alone under the host
// sanitizers; drp_capi.hip includes it ahead of the C ABI's sections.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

// the batch as uploaded (drp_train_step): states [B][H+1][N][3] | impulses [B][H][N][3] | attributes [B][H+1][N] | densities [B]
// | particle counts [B] (ints), every block 16-byte aligned; drp_train_step_untracked (M > 0): behind them the target clouds
// [B][H][M][3] | their counts [B][H] (ints) -- with M = 0 the layout, and so the one copy, is drp_train_step's;
// drp_train_step_actions (`actions`): the pushes [B][H][4] where the impulses are, everything behind them moving up;
// drp_train_step_transport, drp_train_step_divergence (`eps`): behind everything the regularisation strengths [B] (doubles);
// drp_train_step_divergence_unbalanced (`reach`, with `eps`): behind those the reaches [B] | the targets' masses [H][B] (doubles);
// drp_train_step_seeded (`seed`): behind everything the caller's d loss / d s_pred [B][H][N][3] (floats, the caller's layout) -- a
// call without it takes zero bytes for it, and nothing ahead of it moves
struct TrArena { size_t states, sdelta, attrs, dens, nums, targets, tnums, bytes, eps, rho, mass_q, seed; };
// the impulse block: what train_stage_batch copies to TrArena::sdelta
inline size_t tr_impulse_bytes(int B, int H, int N, bool actions) {
    return (actions ? (size_t)B * H * 4 : (size_t)B * H * N * 3) * sizeof(float);
}
inline TrArena tr_layout(int B, int H, int N, int M = 0, bool actions = false, bool eps = false, bool reach = false,
                         bool seed = false) {
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    TrArena a{};
    a.states = 0;
    a.sdelta = up(a.states + (size_t)B * (H + 1) * N * 3 * sizeof(float));
    a.attrs = up(a.sdelta + tr_impulse_bytes(B, H, N, actions));
    a.dens = up(a.attrs + (size_t)B * (H + 1) * N * sizeof(float));
    a.nums = up(a.dens + (size_t)B * sizeof(float));
    a.bytes = up(a.nums + (size_t)B * sizeof(int));
    if (M > 0) {
        a.targets = a.bytes;
        a.tnums = up(a.targets + (size_t)B * H * M * 3 * sizeof(float));
        a.bytes = up(a.tnums + (size_t)B * H * sizeof(int));
    }
    if (eps) {
        a.eps = a.bytes;
        a.bytes = up(a.eps + (size_t)B * sizeof(double));
    }
    if (eps && reach) {
        a.rho = a.bytes;
        a.mass_q = up(a.rho + (size_t)B * sizeof(double));
        a.bytes = up(a.mass_q + (size_t)H * B * sizeof(double));
    }
    if (seed) {
        a.seed = a.bytes;
        a.bytes = up(a.seed + (size_t)B * H * N * 3 * sizeof(float));
    }
    return a;
}

// the batch as the float64 yardsticks upload it (capi_grad_f64.h: train_grad_f64_body), in 4-byte words, packed: states
// [B][H+1][N][3] | impulses [B][H][N][3] (`actions`: the pushes [B][H][4]) | attrs[:, 0] [B][N] | densities [B] | particle counts
// [B] (ints); drp_train_grad_f64_untracked (M > 0): behind them the target clouds [B][H][M][3] | their counts [B][H] (ints) --
// with M = 0 the layout, and so the one copy, is drp_train_grad_f64's; drp_train_grad_f64_divergence (`eps`): behind everything
// the regularisation strengths [B] (doubles, two words each) on the next even word -- the vector's base is 256-byte aligned on
// the device, so an even word is an 8-byte boundary -- and nothing ahead of them moves; drp_train_grad_f64_divergence_unbalanced
// (`reach`, with `eps`): behind eps the reaches [B] | the targets' masses [H][B] (doubles too); drp_train_grad_f64_match with a matching
// of the caller's (`match_in`): behind everything the partners [H][B][N] (ints), nothing ahead of them moving either;
// drp_train_grad_f64_seeded (`seed`): behind everything the caller's d loss / d s_pred [B][H][N][3] (doubles, two words each) on
// the next multiple of four words -- a 16-byte boundary on the device --, nothing ahead of it moving
struct Tr64Arena { size_t states, sdelta, attr, dens, nums, targets, tnums, words, eps, match_in, rho, mass_q, seed; };
inline Tr64Arena tr64_layout(int B, int H, int N, int M = 0, bool actions = false, bool eps = false, bool match_in = false,
                             bool reach = false, bool seed = false) {
    Tr64Arena a{};
    a.states = 0;
    a.sdelta = a.states + (size_t)B * (H + 1) * N * 3;
    a.attr = a.sdelta + tr_impulse_bytes(B, H, N, actions) / sizeof(float);
    a.dens = a.attr + (size_t)B * N;
    a.nums = a.dens + (size_t)B;
    a.words = a.nums + (size_t)B;
    a.targets = a.tnums = a.words;
    if (M > 0) {
        a.tnums = a.targets + (size_t)B * H * M * 3;
        a.words = a.tnums + (size_t)B * H;
    }
    if (eps) {
        a.eps = (a.words + 1) & ~(size_t)1;
        a.words = a.eps + 2 * (size_t)B;
    }
    if (eps && reach) {
        a.rho = a.words;
        a.mass_q = a.rho + 2 * (size_t)B;
        a.words = a.mass_q + 2 * (size_t)H * B;
    }
    if (match_in) {
        a.match_in = a.words;
        a.words = a.match_in + (size_t)H * B * N;
    }
    if (seed) {
        a.seed = (a.words + 3) & ~(size_t)3;
        a.words = a.seed + 2 * (size_t)B * H * N * 3;
    }
    return a;
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

// drp_train_step_divergence's device doubles (c->tr_loss), in doubles: terms [H][B] | col_err [H][B] | self_err [H][B][2] | the
// value sums [3][H][B] | the gradient sums [2][H][B][N][3]; drp_train_step_divergence_unbalanced (`unbalanced`): behind them
// transported [H][B]
struct TrDivLoss { size_t terms, col_err, self_err, vals, gsum, count, transported; };
inline TrDivLoss tr_div_loss_layout(int B, int H, int N, bool unbalanced = false) {
    const size_t hb = (size_t)H * B;
    TrDivLoss a{};
    a.terms = 0;
    a.col_err = a.terms + hb;
    a.self_err = a.col_err + hb;
    a.vals = a.self_err + 2 * hb;
    a.gsum = a.vals + 3 * hb;
    a.count = a.gsum + 2 * hb * N * 3;
    if (unbalanced) {
        a.transported = a.count;
        a.count = a.transported + hb;
    }
    return a;
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
