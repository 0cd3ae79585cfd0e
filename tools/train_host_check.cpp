// Host-code hygiene of the trainer's entry points (csrc/train_host.h): where the blocks of a staged batch lie, with data impulses,
// with pushes and with target clouds, and which pushes a call refuses.  A stand-alone program for the host sanitizers:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/train_host_check.cpp -o build/train_host_check && build/train_host_check
//   (or any C++17 compiler: c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all ...)
//
// It stages batches as train_stage_batch does -- the same copies, to the offsets tr_layout gives, into a heap block of exactly
// TrArena::bytes -- so a block that overlaps the next one or runs past the end is the sanitizer's finding; the offsets are held
// to the documented layout as well.  The float64 yardsticks' upload (tr64_layout: train_grad_f64_body's one vector, with and
// without target clouds) is staged the same way, and so is the one buffer of the three one-shots on two clouds (cloud_layout with
// cm_layout's, chamfer_layout's and chamfer64_layout's blocks: the inputs staged, every output block written in full; the two
// Chamfer layouts held to offset chains written out by hand here, an independent restatement), with the check
// that refuses a real row that is no number.  The transport loss: transport_layout's blocks staged like the matching's, the
// eps block behind a training batch (tr_layout with `eps`), and the check of the regularisation strengths.  The Sinkhorn divergence:
// divergence_layout's five blocks that come back staged the same way, eps and the kernels' scratch behind them written in full
// inside a block of exactly its `bytes`, and the trainer's doubles (tr_div_loss_layout) likewise.  Its float64 yardstick: eps [B]
// (doubles) behind the float64 upload on an even word (tr64_layout with `eps`), nothing ahead of it moved, and
// drp_cloud_divergence_f64's buffer (divergence_layout with 8-byte elements: p and the gradient as doubles, staged through the same
// cloud_layout as every one-shot), every block written in full; the finiteness check on double rows.  The matching losses' float64 yardstick: the caller's partners [H][B][N] behind the float64 upload
// (tr64_layout with `match_in`), drp_cloud_match_f64's buffer of its own (match64_layout, with and without match_in), and the
// check of a matching given by the caller (check_matching) on arrays of exactly [N].  The unbalanced Sinkhorn divergence:
// divergence_layout with `reach` (eps | rho | mass_q side by side, the scratch, transported, inside a block of exactly its `bytes`,
// the five blocks that come back where they are without it, no rho or mass_q without it), the trainer's rho [B] | mass_q [H][B] behind eps (tr_layout
// with `reach`) and transported behind its doubles (tr_div_loss_layout with `unbalanced`), nothing ahead of them moved, and the
// check of a reach and a target mass (check_reach) at the edges of its ranges.  Its float64 yardstick: rho [B] | mass_q [H][B]
// (doubles) behind eps in the float64 upload (tr64_layout with `reach`), and drp_cloud_divergence_unbalanced_f64's buffer
// (divergence_layout with `reach` and 8-byte elements: the same blocks, every double on a multiple of 8).  The seeded step: the caller's d loss / d s_pred [B][H][N][3] behind a training batch (tr_layout with
// `seed`: floats, 16-byte aligned) and behind the float64 upload (tr64_layout with `seed`: doubles on a multiple of four words),
// staged as train_stage_batch and train_grad_f64_body stage them and read back as kt_seed_given and k64_seed_given address them,
// nothing ahead of either moved and a call without a seed taking no byte for it; and the scan that refuses a real row of a seed
// that is no number (first_bad_seed) on arrays of exactly [B][H][N][3].  No device is touched.
//
//   train_host_check layout64 B H N M actions     prints tr64_layout's eight fields (4-byte words) and exits
//   train_host_check layout B H N M actions eps reach seed     prints tr_layout's twelve fields (bytes) and exits
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../dyn_res_pile_manip_amd/csrc/train_host.h"

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

static void stage(int B, int H, int N, int M, bool actions) {
    const TrArena lay = tr_layout(B, H, N, M, actions);
    const size_t n_st = (size_t)B * (H + 1) * N * 3, n_imp = actions ? (size_t)B * H * 4 : (size_t)B * H * N * 3;
    const size_t n_at = (size_t)B * (H + 1) * N, n_tg = (size_t)B * H * M * 3;
    std::vector<float> states(n_st, 1.0f), imp(n_imp, 2.0f), attrs(n_at, 3.0f), dens(B, 4.0f), targets(n_tg, 6.0f);
    std::vector<int32_t> nums(B, 5), tnums((size_t)B * H, 7);
    // every block starts on 16 bytes, in the documented order, and ends before the next one starts
    const size_t off[] = {lay.states, lay.sdelta, lay.attrs, lay.dens, lay.nums, M > 0 ? lay.targets : lay.bytes,
                          M > 0 ? lay.tnums : lay.bytes, lay.bytes};
    const size_t len[] = {n_st * 4, n_imp * 4, n_at * 4, (size_t)B * 4, (size_t)B * 4, n_tg * 4, M > 0 ? (size_t)B * H * 4 : 0};
    for (int k = 0; k < 7; ++k) {
        EXPECT(off[k] % 16 == 0);
        EXPECT(off[k] + len[k] <= off[k + 1]);
        EXPECT(off[k + 1] - (off[k] + len[k]) < 16);             // no more than the alignment between two blocks
    }
    EXPECT(tr_impulse_bytes(B, H, N, actions) == n_imp * 4);
    if (!actions && M == 0) {                                    // the existing call's layout, restated from its description
        auto up = [](size_t v) { return (v + 15) / 16 * 16; };
        size_t at = up(n_st * 4);
        EXPECT(lay.sdelta == at);
        at = up(at + (size_t)B * H * N * 3 * 4);
        EXPECT(lay.attrs == at);
        at = up(at + n_at * 4);
        EXPECT(lay.dens == at);
        at = up(at + (size_t)B * 4);
        EXPECT(lay.nums == at);
        EXPECT(lay.bytes == up(at + (size_t)B * 4));
    }
    if (actions) {                                               // the pushes shrink the impulse block: nothing else moves ahead of it
        const TrArena data = tr_layout(B, H, N, M, false);
        EXPECT(lay.states == data.states && lay.sdelta == data.sdelta);
        EXPECT(lay.bytes <= data.bytes);
    }
    // train_stage_batch's copies into a block of exactly lay.bytes
    char* pin = static_cast<char*>(std::malloc(lay.bytes));
    std::memset(pin, 0xff, lay.bytes);
    std::memcpy(pin + lay.states, states.data(), n_st * sizeof(float));
    std::memcpy(pin + lay.sdelta, imp.data(), tr_impulse_bytes(B, H, N, actions));
    std::memcpy(pin + lay.attrs, attrs.data(), n_at * sizeof(float));
    std::memcpy(pin + lay.dens, dens.data(), (size_t)B * sizeof(float));
    std::memcpy(pin + lay.nums, nums.data(), (size_t)B * sizeof(int));
    if (M > 0) {
        std::memcpy(pin + lay.targets, targets.data(), n_tg * sizeof(float));
        std::memcpy(pin + lay.tnums, tnums.data(), (size_t)B * H * sizeof(int));
    }
    // read back as the kernels address it: no copy overwrote another block
    auto f = [&](size_t o, size_t i) { float v; std::memcpy(&v, pin + o + i * 4, 4); return v; };
    auto n = [&](size_t o, size_t i) { int32_t v; std::memcpy(&v, pin + o + i * 4, 4); return v; };
    EXPECT(f(lay.states, 0) == 1.0f && f(lay.states, n_st - 1) == 1.0f);
    EXPECT(f(lay.sdelta, 0) == 2.0f && f(lay.sdelta, n_imp - 1) == 2.0f);
    EXPECT(f(lay.attrs, 0) == 3.0f && f(lay.attrs, n_at - 1) == 3.0f);
    EXPECT(f(lay.dens, 0) == 4.0f && f(lay.dens, B - 1) == 4.0f);
    EXPECT(n(lay.nums, 0) == 5 && n(lay.nums, B - 1) == 5);
    if (M > 0) {
        EXPECT(f(lay.targets, 0) == 6.0f && f(lay.targets, n_tg - 1) == 6.0f);
        EXPECT(n(lay.tnums, 0) == 7 && n(lay.tnums, (size_t)B * H - 1) == 7);
    }
    std::free(pin);
}

// the float64 yardsticks' batch as train_grad_f64_body stages it: one vector of exactly Tr64Arena::words 4-byte words
static void stage64(int B, int H, int N, int M, bool actions) {
    const Tr64Arena lay = tr64_layout(B, H, N, M, actions);
    const size_t n_st = (size_t)B * (H + 1) * N * 3, n_imp = actions ? (size_t)B * H * 4 : (size_t)B * H * N * 3;
    const size_t n_at_in = (size_t)B * (H + 1) * N, n_tg = (size_t)B * H * M * 3;
    std::vector<float> states(n_st, 1.0f), imp(n_imp, 2.0f), attrs(n_at_in, 3.0f), dens(B, 4.0f), targets(n_tg, 6.0f);
    std::vector<int32_t> nums(B, 5), tnums((size_t)B * H, 7);
    // packed, in the documented order: every block ends where the next one starts
    const size_t off[] = {lay.states, lay.sdelta, lay.attr, lay.dens, lay.nums, lay.targets, lay.tnums, lay.words};
    const size_t len[] = {n_st, n_imp, (size_t)B * N, (size_t)B, (size_t)B, n_tg, M > 0 ? (size_t)B * H : 0};
    for (int k = 0; k < 7; ++k) EXPECT(off[k] + len[k] == off[k + 1]);
    EXPECT(lay.states == 0);
    if (M == 0) EXPECT(lay.words == n_st + n_imp + (size_t)B * N + 2 * (size_t)B);      // drp_train_grad_f64's vector, restated
    // train_grad_f64_body's copies into a block of exactly lay.words words
    float* host = static_cast<float*>(std::malloc(lay.words * sizeof(float)));
    std::memset(host, 0xff, lay.words * sizeof(float));
    std::memcpy(host + lay.states, states.data(), (lay.sdelta - lay.states) * sizeof(float));
    std::memcpy(host + lay.sdelta, imp.data(), (lay.attr - lay.sdelta) * sizeof(float));
    for (int b = 0; b < B; ++b) std::memcpy(host + lay.attr + (size_t)b * N, attrs.data() + (size_t)b * (H + 1) * N, (size_t)N * sizeof(float));
    std::memcpy(host + lay.dens, dens.data(), (size_t)B * sizeof(float));
    std::memcpy(host + lay.nums, nums.data(), (size_t)B * sizeof(int32_t));
    if (M > 0) {
        std::memcpy(host + lay.targets, targets.data(), n_tg * sizeof(float));
        std::memcpy(host + lay.tnums, tnums.data(), (size_t)B * H * sizeof(int32_t));
    }
    auto n = [&](size_t o, size_t i) { int32_t v; std::memcpy(&v, host + o + i, 4); return v; };
    EXPECT(host[lay.states] == 1.0f && host[lay.sdelta - 1] == 1.0f);
    EXPECT(host[lay.sdelta] == 2.0f && host[lay.attr - 1] == 2.0f);
    EXPECT(host[lay.attr] == 3.0f && host[lay.dens - 1] == 3.0f);
    EXPECT(host[lay.dens] == 4.0f && host[lay.nums - 1] == 4.0f);
    EXPECT(n(lay.nums, 0) == 5 && n(lay.nums, B - 1) == 5);
    if (M > 0) {
        EXPECT(host[lay.targets] == 6.0f && host[lay.tnums - 1] == 6.0f);
        EXPECT(n(lay.tnums, 0) == 7 && n(lay.tnums, (size_t)B * H - 1) == 7 && lay.tnums + (size_t)B * H == lay.words);
    }
    std::free(host);
}

// drp_train_grad_f64_divergence's upload: eps [B] (doubles) behind everything else on an 8-byte boundary of a vector whose base is
// aligned, the other blocks where they were
static void stage64_eps(int B, int H, int N, int M, bool actions) {
    const Tr64Arena lay = tr64_layout(B, H, N, M, actions, true), plain = tr64_layout(B, H, N, M, actions);
    EXPECT(lay.states == plain.states && lay.sdelta == plain.sdelta && lay.attr == plain.attr && lay.dens == plain.dens &&
           lay.nums == plain.nums && lay.targets == plain.targets && lay.tnums == plain.tnums);
    EXPECT(lay.eps % 2 == 0 && lay.eps >= plain.words && lay.eps - plain.words < 2);
    EXPECT(lay.words == lay.eps + 2 * (size_t)B);
    EXPECT(plain.eps == 0);
    std::vector<double> eps(B, 0.5);
    float* host = static_cast<float*>(std::malloc(lay.words * sizeof(float)));      // (malloc aligns to 16: the device buffer to 256)
    std::memset(host, 0xff, lay.words * sizeof(float));
    std::memcpy(host + lay.eps, eps.data(), (size_t)B * sizeof(double));
    EXPECT(reinterpret_cast<uintptr_t>(host + lay.eps) % sizeof(double) == 0);
    const double* as_kernel = reinterpret_cast<const double*>(host + lay.eps);       // as kd64_sweeps addresses it
    EXPECT(as_kernel[0] == 0.5 && as_kernel[B - 1] == 0.5);
    std::free(host);
}

// drp_train_grad_f64_divergence_unbalanced's upload: rho [B] | mass_q [H][B] (doubles) behind eps, 8-byte aligned, everything ahead
// of them where it was; both written and read back as the kernels address them, in a block of exactly `words`
static void stage64_reach(int B, int H, int N, int M, bool actions) {
    const Tr64Arena lay = tr64_layout(B, H, N, M, actions, true, false, true), plain = tr64_layout(B, H, N, M, actions, true);
    EXPECT(lay.states == plain.states && lay.sdelta == plain.sdelta && lay.attr == plain.attr && lay.dens == plain.dens &&
           lay.nums == plain.nums && lay.targets == plain.targets && lay.tnums == plain.tnums && lay.eps == plain.eps);
    EXPECT(lay.rho == plain.words && lay.rho % 2 == 0);
    EXPECT(lay.mass_q == lay.rho + 2 * (size_t)B && lay.words == lay.mass_q + 2 * (size_t)H * B);
    EXPECT(plain.rho == 0 && plain.mass_q == 0);
    EXPECT(tr64_layout(B, H, N, M, actions, false, false, true).words == tr64_layout(B, H, N, M, actions).words);  // (no reach without eps)
    std::vector<double> rho(B, 0.25), w((size_t)H * B, 1.5);
    float* host = static_cast<float*>(std::malloc(lay.words * sizeof(float)));
    std::memset(host, 0xff, lay.words * sizeof(float));
    std::memcpy(host + lay.rho, rho.data(), (size_t)B * sizeof(double));
    std::memcpy(host + lay.mass_q, w.data(), (size_t)H * B * sizeof(double));
    EXPECT(reinterpret_cast<uintptr_t>(host + lay.rho) % sizeof(double) == 0);
    const double* r = reinterpret_cast<const double*>(host + lay.rho);               // as kd64_sweeps_unbalanced addresses them
    const double* m = reinterpret_cast<const double*>(host + lay.mass_q);
    EXPECT(r[0] == 0.25 && r[B - 1] == 0.25 && m[0] == 1.5 && m[(size_t)(H - 1) * B + (B - 1)] == 1.5);
    std::free(host);
}

// drp_train_grad_f64_match's upload: the caller's partners [H][B][N] (ints) behind everything else, the other blocks where they were
static void stage64_match(int B, int H, int N, int M, bool actions) {
    const Tr64Arena lay = tr64_layout(B, H, N, M, actions, false, true), plain = tr64_layout(B, H, N, M, actions);
    EXPECT(lay.states == plain.states && lay.sdelta == plain.sdelta && lay.attr == plain.attr && lay.dens == plain.dens &&
           lay.nums == plain.nums && lay.targets == plain.targets && lay.tnums == plain.tnums);
    EXPECT(lay.match_in == plain.words && lay.words == lay.match_in + (size_t)H * B * N && plain.match_in == 0);
    std::vector<int32_t> match((size_t)H * B * N, 7);
    float* host = static_cast<float*>(std::malloc(lay.words * sizeof(float)));
    std::memset(host, 0xff, lay.words * sizeof(float));
    std::memcpy(host + lay.match_in, match.data(), match.size() * sizeof(int32_t));
    const int* as_kernel = reinterpret_cast<const int*>(host + lay.match_in);          // as ka64_match addresses it
    EXPECT(as_kernel[0] == 7 && as_kernel[((size_t)(H - 1) * B + (B - 1)) * N + (N - 1)] == 7);
    std::free(host);
}

// drp_cloud_match_f64's buffer: the inputs (p as doubles, the caller's partners last and optional) staged into a vector of exactly
// in_bytes, the six blocks that come back written in full inside a block of exactly `bytes`
static void stage_match64(int B, int N, int M, bool match_in) {
    const size_t bn = (size_t)B * N, bm = (size_t)B * M;
    const Match64Layout lay = match64_layout(B, N, M, match_in);
    const size_t off[] = {lay.pts_p, lay.pts_q, lay.n_p, lay.n_q, lay.match_in, lay.out[0], lay.out[1], lay.out[2], lay.out[3],
                          lay.out[4], lay.out[5], lay.bytes};
    const size_t len[] = {bn * 24, bm * 12, (size_t)B * 4, (size_t)B * 4, match_in ? bn * 4 : 0, (size_t)B * 8, bn * 24, bn * 4, bm * 4,
                          (bn + bm) * 8, (size_t)B * 16};
    for (int k = 0; k < 11; ++k) {
        EXPECT(off[k] % 16 == 0);
        EXPECT(off[k] + len[k] <= off[k + 1] && off[k + 1] - (off[k] + len[k]) < 16);
        if (k >= 5) EXPECT(lay.out_bytes[k - 5] == len[k]);
    }
    EXPECT(lay.pts_p == 0 && lay.out[0] == lay.in_bytes);
    std::vector<double> p(bn * 3, 1.0);
    std::vector<float> q(bm * 3, 2.0f);
    std::vector<int32_t> n_p(B, N), n_q(B, M), match(bn, 3);
    std::vector<char> stage(lay.in_bytes);
    std::memcpy(stage.data() + lay.pts_p, p.data(), bn * 3 * sizeof(double));
    std::memcpy(stage.data() + lay.pts_q, q.data(), bm * 3 * sizeof(float));
    std::memcpy(stage.data() + lay.n_p, n_p.data(), (size_t)B * sizeof(int32_t));
    std::memcpy(stage.data() + lay.n_q, n_q.data(), (size_t)B * sizeof(int32_t));
    if (match_in) std::memcpy(stage.data() + lay.match_in, match.data(), bn * sizeof(int32_t));
    char* io = static_cast<char*>(std::malloc(lay.bytes));
    std::memcpy(io, stage.data(), lay.in_bytes);
    for (int k = 5; k < 11; ++k) std::memset(io + off[k], k, len[k]);          // the kernel's stores, block by block
    double d; int32_t n;
    std::memcpy(&d, io + lay.pts_p + (bn * 3 - 1) * 8, 8);
    EXPECT(d == 1.0);
    std::memcpy(&n, io + lay.n_q + (size_t)(B - 1) * 4, 4);
    EXPECT(n == M);
    if (match_in) {
        std::memcpy(&n, io + lay.match_in + (bn - 1) * 4, 4);
        EXPECT(n == 3);
    }
    for (int k = 5; k < 11; ++k) EXPECT(io[off[k]] == k && io[off[k] + len[k] - 1] == k);
    std::free(io);
}

// a matching given by the caller, on a heap array of exactly [N]: what check_matching accepts and what it refuses, with the row
static void check_matchings() {
    const int N = 6;
    int32_t* m = static_cast<int32_t*>(std::malloc(N * sizeof(int32_t)));
    int row = -7;
    auto set = [&](int a, int b, int c, int d, int e, int f) { m[0] = a; m[1] = b; m[2] = c; m[3] = d; m[4] = e; m[5] = f; };
    set(2, 0, 1, 3, -1, -1);                                     // n_p = 4 rows into n_q = 5: every real row matched
    EXPECT(check_matching(m, 4, 5, N, &row) == MATCH_OK);
    set(-1, 0, -1, 1, 2, -1);                                    // n_p = 5 rows, n_q = 3: r = 3 pairs, two real rows left out
    EXPECT(check_matching(m, 5, 3, N, &row) == MATCH_OK);
    set(2, 0, 2, 3, -1, -1);                                     // a partner two rows have
    EXPECT(check_matching(m, 4, 5, N, &row) == MATCH_DUP && row == 2);
    set(2, 0, 5, 3, -1, -1);                                     // out of range: n_q = 5
    EXPECT(check_matching(m, 4, 5, N, &row) == MATCH_RANGE && row == 2);
    set(2, 0, 1, -2, -1, -1);                                    // below -1
    EXPECT(check_matching(m, 4, 5, N, &row) == MATCH_RANGE && row == 3);
    set(2, -1, 1, 3, -1, -1);                                    // too few pairs: row 1 has none
    EXPECT(check_matching(m, 4, 5, N, &row) == MATCH_FEW && row == 1);
    set(2, 0, 1, 3, -1, 4);                                      // a partner on the last padded row
    EXPECT(check_matching(m, 4, 5, N, &row) == MATCH_PAD && row == 5);
    set(0, -1, -1, -1, -1, -1);                                  // one row each
    EXPECT(check_matching(m, 1, 1, N, &row) == MATCH_OK);
    EXPECT(check_matching(m, 1, 1, 1, &row) == MATCH_OK);        // N = 1: one element read
    std::free(m);
}

// a one-shot's buffer as cloud_begin and the kernel use it (capi_pipeline.h): the inputs copied into a vector of exactly
// CloudLayout::in_bytes, every output block written in full inside a block of exactly CloudLayout::bytes; len: the n_out blocks'
// sizes, restated by the caller; p_elem: bytes of one of p's elements (floats, or the float64 divergence's doubles)
static void stage_cloud(const CloudLayout& lay, int B, int N, int M, int n_out, const size_t* out_len, size_t p_elem = 4) {
    const size_t bn = (size_t)B * N, bm = (size_t)B * M;
    EXPECT(lay.n_out == n_out);
    size_t off[4 + CLOUD_MAX_OUT + 1] = {lay.pts_p, lay.pts_q, lay.n_p, lay.n_q};
    size_t len[4 + CLOUD_MAX_OUT] = {bn * 3 * p_elem, bm * 12, (size_t)B * 4, (size_t)B * 4};
    EXPECT(lay.p_elem == p_elem);
    for (int k = 0; k < n_out; ++k) {
        off[4 + k] = lay.out[k];
        len[4 + k] = out_len[k];
        EXPECT(lay.out_bytes[k] == out_len[k]);
    }
    const int nb = 4 + n_out;
    off[nb] = lay.bytes;
    for (int k = 0; k < nb; ++k) {
        EXPECT(off[k] % 16 == 0);
        EXPECT(off[k] + len[k] <= off[k + 1]);                   // no block overlaps the next
        EXPECT(off[k + 1] - (off[k] + len[k]) < 16);
    }
    EXPECT(lay.pts_p == 0 && lay.out[0] == lay.in_bytes);
    std::vector<float> p(bn * 3, 1.0f), q(bm * 3, 2.0f);
    std::vector<double> p64(bn * 3, 1.0);
    std::vector<int32_t> n_p(B, N), n_q(B, M);
    std::vector<char> stage(lay.in_bytes);
    std::memcpy(stage.data() + lay.pts_p, p_elem == 8 ? (const void*)p64.data() : (const void*)p.data(), bn * 3 * p_elem);     // as cloud_begin does
    std::memcpy(stage.data() + lay.pts_q, q.data(), bm * 3 * sizeof(float));
    std::memcpy(stage.data() + lay.n_p, n_p.data(), (size_t)B * sizeof(int32_t));
    std::memcpy(stage.data() + lay.n_q, n_q.data(), (size_t)B * sizeof(int32_t));
    char* io = static_cast<char*>(std::malloc(lay.bytes));
    std::memcpy(io, stage.data(), lay.in_bytes);
    for (int k = 4; k < nb; ++k) std::memset(io + off[k], k, len[k]);      // the kernel's stores, block by block
    float f; double d; int32_t n;
    if (p_elem == 8) {
        std::memcpy(&d, io + lay.pts_p + (bn * 3 - 1) * 8, 8);
        EXPECT(d == 1.0);
    } else {
        std::memcpy(&f, io + lay.pts_p + (bn * 3 - 1) * 4, 4);
        EXPECT(f == 1.0f);
    }
    std::memcpy(&f, io + lay.pts_q + (bm * 3 - 1) * 4, 4);
    EXPECT(f == 2.0f);
    std::memcpy(&n, io + lay.n_q + (size_t)(B - 1) * 4, 4);
    EXPECT(n == M);
    for (int k = 4; k < nb; ++k) EXPECT(io[off[k]] == k && io[off[k] + len[k] - 1] == k);
    std::free(io);
}
static void stage_match(int B, int N, int M) {
    const size_t bn = (size_t)B * N, bm = (size_t)B * M;
    const size_t len[] = {(size_t)B * 8, bn * 12, bn * 4, bm * 4, (bn + bm) * 8};
    stage_cloud(cm_layout(B, N, M), B, N, M, 5, len);
}
// drp_cloud_transport: four output blocks and eps [B] as a fifth, which the entry point copies up behind the inputs
static void stage_transport(int B, int N, int M) {
    const size_t bn = (size_t)B * N, bm = (size_t)B * M;
    const size_t len[] = {(size_t)B * 8, bn * 12, (bn + bm) * 8, (size_t)B * 8, (size_t)B * 8};
    stage_cloud(transport_layout(B, N, M), B, N, M, 5, len);
}
// drp_cloud_divergence: five output blocks as a one-shot's; behind them eps [B], the value sums [3][B] and the gradient sums
// [2][B][N][3], which the kernels write and nothing reads back.  p_elem 8: drp_cloud_divergence_f64, p and the gradient as doubles
static void stage_divergence(int B, int N, int M, size_t p_elem) {
    const size_t bn = (size_t)B * N, bm = (size_t)B * M;
    const DivLayout lay = divergence_layout(B, N, M, false, p_elem);
    const size_t len[] = {(size_t)B * 8, bn * 3 * p_elem, 2 * (bn + bm) * 8, (size_t)B * 8, (size_t)B * 16};
    CloudLayout back = lay.cloud;
    back.bytes = lay.eps;                                            // what comes back ends where eps starts
    stage_cloud(back, B, N, M, 5, len, p_elem);
    const size_t off[] = {lay.eps, lay.vals, lay.gsum, lay.cloud.bytes};
    const size_t xlen[] = {(size_t)B * 8, (size_t)3 * B * 8, 2 * bn * 3 * 8};
    char* io = static_cast<char*>(std::malloc(lay.cloud.bytes));
    for (int k = 0; k < 3; ++k) {
        EXPECT(off[k] % 16 == 0);
        EXPECT(off[k] + xlen[k] <= off[k + 1] && off[k + 1] - (off[k] + xlen[k]) < 16);
        std::memset(io + off[k], k + 1, xlen[k]);
    }
    for (int k = 0; k < 3; ++k) EXPECT(io[off[k]] == k + 1 && io[off[k] + xlen[k] - 1] == k + 1);
    // the last row's last gradient sum of the second problem set, where kd_sweeps' p-p block of the last sample stores it
    double* gsum = reinterpret_cast<double*>(io + lay.gsum);
    gsum[((size_t)B + (B - 1)) * N * 3 + (size_t)(N - 1) * 3 + 2] = 1.0;
    reinterpret_cast<double*>(io + lay.vals)[2 * (size_t)B + (B - 1)] = 1.0;
    std::free(io);
}
// drp_train_step_divergence's doubles on the device: the terms, the certificates and the kernels' scratch, packed, in doubles
static void stage_div_loss(int B, int H, int N) {
    const TrDivLoss dl = tr_div_loss_layout(B, H, N);
    const size_t hb = (size_t)H * B;
    const size_t off[] = {dl.terms, dl.col_err, dl.self_err, dl.vals, dl.gsum, dl.count};
    const size_t len[] = {hb, hb, 2 * hb, 3 * hb, 2 * hb * N * 3};
    EXPECT(dl.terms == 0 && dl.col_err == hb);                       // the transport loss's two blocks where they were
    double* d = static_cast<double*>(std::malloc(dl.count * sizeof(double)));
    for (int k = 0; k < 5; ++k) {
        EXPECT(off[k] + len[k] == off[k + 1]);
        for (size_t e = 0; e < len[k]; ++e) d[off[k] + e] = (double)k;
    }
    for (int k = 0; k < 5; ++k) EXPECT(d[off[k]] == (double)k && d[off[k + 1] - 1] == (double)k);
    std::free(d);
}
// drp_cloud_divergence_unbalanced (divergence_layout with `reach`): the five blocks where they were; behind them eps | rho | mass_q [B] each, side
// by side (one copy up), the same scratch, then transported [B], all inside a block of exactly `bytes`.  p_elem 8:
// drp_cloud_divergence_unbalanced_f64
static void stage_divergence_unbalanced(int B, int N, int M, size_t p_elem) {
    const size_t bn = (size_t)B * N;
    const DivLayout lay = divergence_layout(B, N, M, true, p_elem), plain = divergence_layout(B, N, M, false, p_elem);
    EXPECT(plain.rho == 0 && plain.mass_q == 0 && plain.transported == 0 && plain.vals < lay.vals);
    for (int k = 0; k < CLOUD_MAX_OUT; ++k) EXPECT(lay.cloud.out[k] == plain.cloud.out[k] && lay.cloud.out_bytes[k] == plain.cloud.out_bytes[k]);
    EXPECT(lay.cloud.in_bytes == plain.cloud.in_bytes && lay.cloud.n_out == plain.cloud.n_out && lay.eps == plain.eps);
    EXPECT(lay.rho == lay.eps + (size_t)B * 8 && lay.mass_q == lay.rho + (size_t)B * 8);
    EXPECT(lay.cloud.out[1] % 8 == 0 && lay.rho % 8 == 0 && lay.mass_q % 8 == 0);      // every double on a multiple of 8
    const size_t off[] = {lay.eps, lay.vals, lay.gsum, lay.transported, lay.cloud.bytes};
    const size_t xlen[] = {(size_t)3 * B * 8, (size_t)3 * B * 8, 2 * bn * 3 * 8, (size_t)B * 8};
    char* io = static_cast<char*>(std::malloc(lay.cloud.bytes));
    for (int k = 0; k < 4; ++k) {
        EXPECT(off[k] % 16 == 0);
        EXPECT(off[k] + xlen[k] <= off[k + 1] && off[k + 1] - (off[k] + xlen[k]) < 16);
        std::memset(io + off[k], k + 1, xlen[k]);
    }
    for (int k = 0; k < 4; ++k) EXPECT(io[off[k]] == k + 1 && io[off[k] + xlen[k] - 1] == k + 1);
    reinterpret_cast<double*>(io + lay.transported)[B - 1] = 1.0;
    reinterpret_cast<double*>(io + lay.mass_q)[B - 1] = 1.0;
    std::free(io);
}
// drp_train_step_divergence_unbalanced: the balanced step's doubles where they were, transported [H][B] behind them; and its batch:
// rho [B] | mass_q [H][B] behind eps, nothing ahead of them moved
static void stage_div_unbalanced_train(int B, int H, int N, int M, bool actions) {
    const TrDivLoss dl = tr_div_loss_layout(B, H, N, true), plain = tr_div_loss_layout(B, H, N);
    const size_t hb = (size_t)H * B;
    EXPECT(dl.terms == plain.terms && dl.col_err == plain.col_err && dl.self_err == plain.self_err && dl.vals == plain.vals &&
           dl.gsum == plain.gsum);
    EXPECT(dl.transported == plain.count && dl.count == dl.transported + hb && plain.transported == 0);
    double* d = static_cast<double*>(std::malloc(dl.count * sizeof(double)));
    for (size_t e = 0; e < hb; ++e) d[dl.transported + e] = 1.0;
    EXPECT(d[dl.count - 1] == 1.0);
    std::free(d);
    const TrArena lay = tr_layout(B, H, N, M, actions, true, true), bal = tr_layout(B, H, N, M, actions, true);
    EXPECT(lay.states == bal.states && lay.sdelta == bal.sdelta && lay.attrs == bal.attrs && lay.dens == bal.dens && lay.nums == bal.nums &&
           lay.targets == bal.targets && lay.tnums == bal.tnums && lay.eps == bal.eps);
    EXPECT(lay.rho == bal.bytes && lay.rho % 16 == 0 && lay.mass_q % 16 == 0 && lay.bytes % 16 == 0);
    EXPECT(lay.rho + (size_t)B * 8 <= lay.mass_q && lay.mass_q - (lay.rho + (size_t)B * 8) < 16);
    EXPECT(lay.mass_q + hb * 8 <= lay.bytes && lay.bytes - (lay.mass_q + hb * 8) < 16);
    EXPECT(tr_layout(B, H, N, M, actions, false, true).bytes == tr_layout(B, H, N, M, actions).bytes);     // a reach without eps: nothing
    std::vector<double> rho(B, 0.5), w(hb, 2.0);
    char* pin = static_cast<char*>(std::malloc(lay.bytes));
    std::memset(pin, 0xff, lay.bytes);
    std::memcpy(pin + lay.rho, rho.data(), (size_t)B * sizeof(double));
    std::memcpy(pin + lay.mass_q, w.data(), hb * sizeof(double));
    double last;
    std::memcpy(&last, pin + lay.mass_q + (hb - 1) * 8, 8);
    EXPECT(last == 2.0);
    std::memcpy(&last, pin + lay.rho + (size_t)(B - 1) * 8, 8);
    EXPECT(last == 0.5);
    std::free(pin);
}
// the reach and the target mass a problem of the unbalanced divergence is served with (check_reach)
static void check_reaches() {
    const double inf64 = std::numeric_limits<double>::infinity(), nan64 = std::numeric_limits<double>::quiet_NaN();
    const double eps = 4e-4;
    EXPECT(check_reach(eps, 4 * eps, 1.0) == REACH_OK && check_reach(eps, eps / 1024, 0.125) == REACH_OK);
    EXPECT(check_reach(eps, 4 * eps, 8.0) == REACH_OK && check_reach(eps, inf64, 1.0) == REACH_OK);
    EXPECT(check_reach(eps, 0.0, 1.0) == REACH_RHO && check_reach(eps, -eps, 1.0) == REACH_RHO && check_reach(eps, nan64, 1.0) == REACH_RHO);
    EXPECT(check_reach(eps, -inf64, 1.0) == REACH_RHO && check_reach(eps, eps / 1025, 1.0) == REACH_RHO);
    EXPECT(check_reach(eps, 4 * eps, 0.1249) == REACH_MASS && check_reach(eps, 4 * eps, 8.001) == REACH_MASS);
    EXPECT(check_reach(eps, 4 * eps, nan64) == REACH_MASS && check_reach(eps, 4 * eps, 0.0) == REACH_MASS && check_reach(eps, inf64, nan64) == REACH_MASS);
    EXPECT(check_reach(eps, inf64, 0.6) == REACH_INF_MASS && check_reach(eps, inf64, 8.0) == REACH_INF_MASS);
}
// drp_train_step_transport's batch: eps [B] (doubles) behind everything else, the other blocks where they were
static void stage_eps(int B, int H, int N, int M, bool actions) {
    const TrArena lay = tr_layout(B, H, N, M, actions, true), plain = tr_layout(B, H, N, M, actions);
    EXPECT(lay.states == plain.states && lay.sdelta == plain.sdelta && lay.attrs == plain.attrs && lay.dens == plain.dens &&
           lay.nums == plain.nums && lay.targets == plain.targets && lay.tnums == plain.tnums);
    EXPECT(lay.eps == plain.bytes && lay.eps % 16 == 0);
    EXPECT(lay.eps + (size_t)B * 8 <= lay.bytes && lay.bytes - (lay.eps + (size_t)B * 8) < 16 && lay.bytes % 16 == 0);
    std::vector<double> eps(B, 0.5);
    char* pin = static_cast<char*>(std::malloc(lay.bytes));
    std::memset(pin, 0xff, lay.bytes);
    std::memcpy(pin + lay.eps, eps.data(), (size_t)B * sizeof(double));
    double last;
    std::memcpy(&last, pin + lay.eps + (size_t)(B - 1) * 8, 8);
    EXPECT(last == 0.5);
    std::free(pin);
}

// drp_train_step_seeded's batch: the seed [B][H][N][3] (floats) behind everything else, the other blocks where they were, with every
// combination of the older blocks; drp_train_grad_f64_seeded's upload: the same in doubles behind the float64 batch
static void stage_seed(int B, int H, int N, int M, bool actions) {
    const size_t n_seed = (size_t)B * H * N * 3;
    for (int eps = 0; eps < 2; ++eps)
        for (int reach = 0; reach < 2; ++reach) {
            const TrArena lay = tr_layout(B, H, N, M, actions, eps != 0, reach != 0, true), plain = tr_layout(B, H, N, M, actions, eps != 0, reach != 0);
            EXPECT(lay.states == plain.states && lay.sdelta == plain.sdelta && lay.attrs == plain.attrs && lay.dens == plain.dens &&
                   lay.nums == plain.nums && lay.targets == plain.targets && lay.tnums == plain.tnums && lay.eps == plain.eps &&
                   lay.rho == plain.rho && lay.mass_q == plain.mass_q);
            EXPECT(plain.seed == 0 && lay.seed == plain.bytes && lay.seed % 16 == 0 && lay.bytes % 16 == 0);
            EXPECT(lay.seed + n_seed * 4 <= lay.bytes && lay.bytes - (lay.seed + n_seed * 4) < 16);
        }
    const TrArena lay = tr_layout(B, H, N, M, actions, false, false, true);
    std::vector<float> seed(n_seed);
    for (size_t e = 0; e < n_seed; ++e) seed[e] = (float)(e % 1021);
    char* pin = static_cast<char*>(std::malloc(lay.bytes));
    std::memset(pin, 0xff, lay.bytes);
    std::memcpy(pin + lay.seed, seed.data(), n_seed * sizeof(float));           // train_stage_batch's copy
    // as kt_seed_given addresses it: sample b, step t at ((b H + t) N) 3 floats, the last element of the last slice included
    const float* as_kernel = reinterpret_cast<const float*>(pin + lay.seed);
    const size_t last = ((size_t)(B - 1) * H + (H - 1)) * N * 3 + (size_t)N * 3 - 1;
    EXPECT(last == n_seed - 1 && as_kernel[0] == 0.0f && as_kernel[last] == (float)(last % 1021));
    if ((N * 3) % 4 == 0) EXPECT((lay.seed + ((size_t)(B - 1) * H + (H - 1)) * N * 3 * 4) % 16 == 0);      // its float4 path's premise
    std::free(pin);

    const Tr64Arena l64 = tr64_layout(B, H, N, M, actions, false, false, false, true), p64 = tr64_layout(B, H, N, M, actions);
    EXPECT(l64.states == p64.states && l64.sdelta == p64.sdelta && l64.attr == p64.attr && l64.dens == p64.dens && l64.nums == p64.nums &&
           l64.targets == p64.targets && l64.tnums == p64.tnums);
    EXPECT(p64.seed == 0 && l64.seed % 4 == 0 && l64.seed >= p64.words && l64.seed - p64.words < 4 && l64.words == l64.seed + 2 * n_seed);
    std::vector<double> seed64(n_seed, 0.5);
    seed64[n_seed - 1] = 0.25;
    float* host = static_cast<float*>(std::malloc(l64.words * sizeof(float)));
    std::memset(host, 0xff, l64.words * sizeof(float));
    std::memcpy(host + l64.seed, seed64.data(), n_seed * sizeof(double));       // train_grad_f64_body's copy
    EXPECT(reinterpret_cast<uintptr_t>(host + l64.seed) % 16 == 0);              // (malloc aligns to 16: the device buffer to 256)
    const double* k64 = reinterpret_cast<const double*>(host + l64.seed);        // as k64_seed_given addresses it
    EXPECT(k64[0] == 0.5 && k64[last] == 0.25);
    std::free(host);
}
// the scan of a seed's real rows: every one of them read, in every step, and nothing of the padding
template <typename T>
static void check_seeds() {
    const T inf = std::numeric_limits<T>::infinity(), nan = std::numeric_limits<T>::quiet_NaN();
    const int B = 2, H = 3, N = 4;
    const int32_t counts[2] = {2, 4};
    const size_t n = (size_t)B * H * N * 3;
    T* x = static_cast<T*>(std::malloc(n * sizeof(T)));                           // exactly [B][H][N][3]
    for (size_t e = 0; e < n; ++e) x[e] = (T)0.125 * (T)e;
    EXPECT(first_bad_seed(x, counts, B, H, N) == -1);
    for (int t = 0; t < H; ++t) x[((size_t)(0 * H + t) * N + 2) * 3 + 1] = nan;       // sample 0's padding, every step
    x[((size_t)(0 * H + 2) * N + 3) * 3 + 2] = inf;
    EXPECT(first_bad_seed(x, counts, B, H, N) == -1);
    x[n - 1] = inf;                                                                 // the last coordinate of the last real row
    EXPECT(first_bad_seed(x, counts, B, H, N) == ((long)1 * H + 2) * N + 3);
    x[((size_t)(1 * H + 0) * N + 0) * 3 + 0] = nan;                                 // an earlier one wins
    EXPECT(first_bad_seed(x, counts, B, H, N) == ((long)1 * H + 0) * N + 0);
    x[((size_t)(0 * H + 1) * N + 1) * 3 + 2] = -inf;
    EXPECT(first_bad_seed(x, counts, B, H, N) == ((long)0 * H + 1) * N + 1);
    const int32_t over[2] = {9, 4};                                                 // a count beyond N is read up to N
    EXPECT(first_bad_seed(x, over, B, H, N) == ((long)0 * H + 0) * N + 2);
    std::free(x);
}

// drp_cloud_chamfer's and drp_cloud_chamfer_f64's layouts against their offset chains written out block by block (the yardstick
// of cloud_layout: the offsets a call's kernel and copies have always used), then staged like the matching's
static void stage_chamfer(int B, int N, int M) {
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t bn = (size_t)B * N, bm = (size_t)B * M;
    const size_t o_p = 0, o_q = up(o_p + bn * 3 * sizeof(float)), o_np = up(o_q + bm * 3 * sizeof(float)),
                 o_nq = up(o_np + (size_t)B * sizeof(int)), in_bytes = up(o_nq + (size_t)B * sizeof(int));
    {
        const size_t o_terms = in_bytes, o_grad = up(o_terms + (size_t)B * 2 * sizeof(double)), o_pq = up(o_grad + bn * 3 * sizeof(float)),
                     o_qp = up(o_pq + bn * sizeof(int)), bytes = up(o_qp + bm * sizeof(int));
        const CloudLayout lay = chamfer_layout(B, N, M);
        EXPECT(lay.pts_p == o_p && lay.pts_q == o_q && lay.n_p == o_np && lay.n_q == o_nq && lay.in_bytes == in_bytes);
        EXPECT(lay.out[0] == o_terms && lay.out[1] == o_grad && lay.out[2] == o_pq && lay.out[3] == o_qp && lay.bytes == bytes);
        const size_t len[] = {(size_t)B * 16, bn * 12, bn * 4, bm * 4};
        stage_cloud(lay, B, N, M, 4, len);
    }
    {
        const size_t o_terms = in_bytes, o_mar = up(o_terms + (size_t)B * 2 * sizeof(double)), o_grad = up(o_mar + (size_t)B * 2 * sizeof(double)),
                     o_pq = up(o_grad + bn * 3 * sizeof(double)), o_qp = up(o_pq + bn * sizeof(int)), bytes = up(o_qp + bm * sizeof(int));
        const CloudLayout lay = chamfer64_layout(B, N, M);
        EXPECT(lay.pts_p == o_p && lay.pts_q == o_q && lay.n_p == o_np && lay.n_q == o_nq && lay.in_bytes == in_bytes);
        EXPECT(lay.out[0] == o_terms && lay.out[1] == o_mar && lay.out[2] == o_grad && lay.out[3] == o_pq && lay.out[4] == o_qp &&
               lay.bytes == bytes);
        const size_t len[] = {(size_t)B * 16, (size_t)B * 16, bn * 24, bn * 4, bm * 4};
        stage_cloud(lay, B, N, M, 5, len);
    }
}

int main(int argc, char** argv) {
    if (argc == 7 && std::strcmp(argv[1], "layout64") == 0) {
        const Tr64Arena a = tr64_layout(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]) != 0);
        std::printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", a.states, a.sdelta, a.attr, a.dens, a.nums, a.targets, a.tnums, a.words);
        return 0;
    }
    if (argc == 10 && std::strcmp(argv[1], "layout") == 0) {
        const TrArena a = tr_layout(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]) != 0,
                                    std::atoi(argv[7]) != 0, std::atoi(argv[8]) != 0, std::atoi(argv[9]) != 0);
        std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", a.states, a.sdelta, a.attrs, a.dens, a.nums, a.targets, a.tnums,
                    a.bytes, a.eps, a.rho, a.mass_q, a.seed);
        return 0;
    }
    // odd sizes (no block a multiple of 16 bytes), one sample, the reference's batch, a large one
    const int shapes[][4] = {{1, 1, 1, 0}, {1, 1, 5, 3}, {3, 3, 24, 0}, {3, 3, 23, 17}, {2, 5, 11, 0}, {4, 5, 300, 0}, {4, 5, 300, 300},
                             {7, 2, 301, 299}, {32, 5, 300, 0}, {2, 64, 9, 1}};
    for (const auto& s : shapes)
        for (int actions = 0; actions < 2; ++actions) {
            stage(s[0], s[1], s[2], s[3], actions != 0);
            stage64(s[0], s[1], s[2], s[3], actions != 0);
            stage_seed(s[0], s[1], s[2], s[3], actions != 0);
            if (s[3] > 0) stage64_eps(s[0], s[1], s[2], s[3], actions != 0);
            if (s[3] > 0) stage64_match(s[0], s[1], s[2], s[3], actions != 0);
            if (s[3] > 0) stage64_reach(s[0], s[1], s[2], s[3], actions != 0);
        }
    stage64(1, 1, 4096, 4096, false);                            // the largest clouds of one (sample, step)
    const int mshapes[][3] = {{1, 1, 1}, {1, 5, 3}, {3, 7, 9}, {2, 65, 64}, {1, 1024, 1024}, {5, 1024, 1}, {4, 300, 257}};
    for (const auto& s : mshapes) {
        stage_match(s[0], s[1], s[2]);
        stage_transport(s[0], s[1], s[2]);
        for (size_t p_elem : {sizeof(float), sizeof(double)}) {
            stage_divergence(s[0], s[1], s[2], p_elem);
            stage_divergence_unbalanced(s[0], s[1], s[2], p_elem);
        }
        stage_match64(s[0], s[1], s[2], false);
        stage_match64(s[0], s[1], s[2], true);
    }
    check_matchings();
    const int dshapes[][3] = {{1, 1, 1}, {2, 2, 9}, {4, 5, 100}, {3, 1, 1024}};
    for (const auto& s : dshapes) stage_div_loss(s[0], s[1], s[2]);
    for (const auto& s : shapes)
        for (int actions = 0; actions < 2; ++actions)
            if (s[3] > 0) {
                stage_eps(s[0], s[1], s[2], s[3], actions != 0);
                stage_div_unbalanced_train(s[0], s[1], s[2], s[3], actions != 0);
            }
    check_reaches();
    check_seeds<float>();
    check_seeds<double>();
    {
        // the regularisation strengths: every one read, none beyond the B-th
        const double inf64 = std::numeric_limits<double>::infinity(), nan64 = std::numeric_limits<double>::quiet_NaN();
        double* eps = static_cast<double*>(std::malloc(3 * sizeof(double)));                 // exactly [B]
        eps[0] = 4e-4; eps[1] = 1e-300; eps[2] = 7.0;
        EXPECT(first_bad_eps(eps, 3) == -1);
        eps[2] = 0.0;
        EXPECT(first_bad_eps(eps, 3) == 2 && first_bad_eps(eps, 2) == -1);
        eps[2] = -4e-4;
        EXPECT(first_bad_eps(eps, 3) == 2);
        eps[2] = inf64;
        EXPECT(first_bad_eps(eps, 3) == 2);
        eps[2] = 1.0; eps[0] = nan64;
        EXPECT(first_bad_eps(eps, 3) == 0);
        std::free(eps);
    }
    const int cshapes[][3] = {{1, 1, 1}, {2, 5, 3}, {3, 70, 130}, {1, 4096, 4096}};
    for (const auto& s : cshapes) stage_chamfer(s[0], s[1], s[2]);
    {
        // the finiteness check reads the real rows only, every one of them, and no further
        const float inf32 = std::numeric_limits<float>::infinity(), nan32 = std::numeric_limits<float>::quiet_NaN();
        const int B = 2, N = 3;
        const int32_t counts[2] = {2, 3};
        float* x = static_cast<float*>(std::malloc((size_t)B * N * 3 * sizeof(float)));     // exactly [B][N][3]
        for (int e = 0; e < B * N * 3; ++e) x[e] = 0.25f * e;
        EXPECT(first_nonfinite_row(x, counts, B, N) == -1);
        x[2 * 3 + 1] = nan32;                                    // sample 0's padding row
        EXPECT(first_nonfinite_row(x, counts, B, N) == -1);
        x[(1 * N + 2) * 3 + 2] = inf32;                          // the last coordinate of the last real row
        EXPECT(first_nonfinite_row(x, counts, B, N) == 1 * N + 2);
        x[1 * 3 + 0] = nan32;
        EXPECT(first_nonfinite_row(x, counts, B, N) == 1);
        const int32_t over[2] = {7, 3};                          // a count beyond N is read up to N (the entry point refuses it first)
        EXPECT(first_nonfinite_row(x, over, B, N) == 1);
        std::free(x);
        // the same on double rows (drp_cloud_divergence_f64's p)
        const double inf64 = std::numeric_limits<double>::infinity(), nan64 = std::numeric_limits<double>::quiet_NaN();
        double* y = static_cast<double*>(std::malloc((size_t)B * N * 3 * sizeof(double)));
        for (int e = 0; e < B * N * 3; ++e) y[e] = 0.25 * e + 1e-12;
        EXPECT(first_nonfinite_row(y, counts, B, N) == -1);
        y[2 * 3 + 1] = nan64;                                    // sample 0's padding row
        EXPECT(first_nonfinite_row(y, counts, B, N) == -1);
        y[(1 * N + 2) * 3 + 2] = inf64;
        EXPECT(first_nonfinite_row(y, counts, B, N) == 1 * N + 2);
        std::free(y);
    }

    // the push check, with the demo camera's map (x, z, -y + 18 scaled by 1 / 24: a camera that looks straight down)
    const float m[12] = {1, 0, 0, 0, 0, 0, 1, 0, 0, -1, 0, 18};
    const float gs = 24.0f;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    float len = -1.0f;
    {
        const int B = 3, H = 4;
        std::vector<float> acts((size_t)B * H * 4);
        for (int e = 0; e < B * H; ++e) {
            acts[e * 4 + 0] = -3.0f + 0.1f * e; acts[e * 4 + 1] = 0.5f; acts[e * 4 + 2] = 3.0f; acts[e * 4 + 3] = -0.25f * e;
        }
        EXPECT(first_bad_push(m, gs, acts.data(), acts.size() / 4, &len) == -1 && len == -1.0f);
        EXPECT(std::fabs(push_len_host(m, gs, acts.data()) - std::sqrt(36.0f + 0.25f) / 24.0f) < 1e-6f);
        std::vector<float> bad = acts;                           // a zero-length push in the middle of the batch
        bad[(1 * H + 1) * 4 + 2] = bad[(1 * H + 1) * 4 + 0];
        bad[(1 * H + 1) * 4 + 3] = bad[(1 * H + 1) * 4 + 1];
        EXPECT(first_bad_push(m, gs, bad.data(), bad.size() / 4, &len) == 1 * H + 1 && len == 0.0f);
        bad = acts;                                              // the last one: the loop reads every push and no further
        bad[bad.size() - 1] = nan;
        EXPECT(first_bad_push(m, gs, bad.data(), bad.size() / 4, &len) == B * H - 1 && len != len);
        bad = acts;
        bad[0] = inf;
        EXPECT(first_bad_push(m, gs, bad.data(), bad.size() / 4, &len) == 0);
        bad = acts;
        bad[2] = 3e38f; bad[0] = -3e38f;                         // a finite push whose length overflows
        EXPECT(first_bad_push(m, gs, bad.data(), bad.size() / 4, &len) == 0 && len == inf);
        EXPECT(first_bad_push(m, gs, acts.data(), 0, &len) == -1);
    }
    {
        const float denormal[4] = {0.0f, 0.0f, 1e-30f, 0.0f};   // its square underflows: the length is zero as push_frame computes it
        EXPECT(first_bad_push(m, gs, denormal, 1, &len) == 0 && len == 0.0f);
    }
    std::printf(failures ? "%d checks FAILED\n" : "train_host_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
