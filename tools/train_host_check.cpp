// Host-code hygiene of the trainer's entry points (csrc/train_host.h): the table of the blocks a trainer call stages and brings
// back, the one-shots' buffers, and what a call refuses.  A stand-alone program for the host sanitizers:
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/train_host_check.cpp -o build/train_host_check && build/train_host_check
//   (or any C++17 compiler: c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all ...)
//
// The block table (tr_blocks; both trainers, every combination of the loss shape's predicates, odd and large sizes, data impulses
// and pushes): every count against a restatement written out here; the input rows and the result rows each disjoint, in order,
// inside `bytes` / `res_bytes`, every block on 16 bytes and every double on 8, no more than the alignment between two blocks; an
// absent block takes no byte and has a null address in the view; adding a block moves nothing ahead of it and everything behind it
// by its own rounded size; a reach without eps adds nothing; the fp32 arena against its offset chain written out by hand.  Then
// the copies themselves: a batch staged as train_stage_batch and train_grad_f64_body stage it (the fixed five, then
// tr_stage_loss_inputs) from arrays of exactly the caller's sizes into a heap block of exactly `bytes`, read back through tr_view as
// the kernels address it; every result row written in full inside a block of exactly `res_bytes` and brought back by
// tr_read_results into arrays of exactly the caller's sizes, a null caller pointer copying nothing -- so a block that overlaps the
// next one or runs past an end is the sanitizer's finding.  The seed block once more as kt_seed_given and k64_seed_given address it.
// The one buffer of the one-shots on two clouds (cloud_layout with cm_layout's, chamfer_layout's and chamfer64_layout's blocks: the
// inputs staged, every output block written in full; the two Chamfer layouts held to offset chains written out by hand here, an
// independent restatement), transport_layout, divergence_layout (balanced and with `reach`, 4- and 8-byte elements),
// drp_cloud_match_f64's buffer of its own (match64_layout, with and without match_in).  The checks: a real row that is no number
// (first_nonfinite_row), the regularisation strengths (first_bad_eps), a matching given by the caller (check_matching), a reach and
// a target mass (check_reach), a seed's real rows (first_bad_seed), the planner's seed (first_bad_plan_seed), a push of no length (first_bad_push).  No device is touched.
//
//   train_host_check layout B H N M actions eps reach seed [f64 match_in]
//       prints the offsets of states, impulses, attributes, densities, counts, targets, their counts, then `bytes`, then the offsets
//       of eps, rho, mass_q, seed (bytes; 0 for an absent block) of the fp32 trainer's staged batch and exits; with the two further
//       flags: of the float64 yardstick's upload (f64 = 1), and the offset of the caller's partners behind them
#include <array>
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

// the loss shape of a bit pattern: every combination of the predicates, meaningful or not -- the table must hold for all
static TrShape shape_of(unsigned bits, int M) {
    return TrShape{(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0, (bits & 32) != 0, (bits & 64) != 0,
                   (bits & 128) != 0, M};
}
static size_t up16(size_t v) { return (v + 15) / 16 * 16; }

// rows [first, end) of a carved range: in order, disjoint, aligned, inside `total`, an absent one at offset 0 and costing nothing
static void check_carved(const TrBlocks& t, int first, int end, size_t total) {
    size_t prev_end = 0;
    for (int id = first; id < end; ++id) {
        if (t.count[id] == 0) {
            EXPECT(t.off[id] == 0);
            continue;
        }
        EXPECT(t.off[id] % 16 == 0 && t.off[id] % t.elem[id] == 0);            // every block on 16 bytes: every double on 8
        EXPECT(t.off[id] >= prev_end && t.off[id] - prev_end < 16);            // no more than the alignment between two blocks
        prev_end = t.off[id] + t.size(id);
    }
    EXPECT(total % 16 == 0 && total >= prev_end && total - prev_end < 16);
}
// `more` is `less` with blocks added: nothing ahead of the first added block moves, everything behind by the added rounded sizes
static void check_added(const TrBlocks& more, const TrBlocks& less, int first, int end, size_t total_more, size_t total_less) {
    size_t shift = 0;
    for (int id = first; id < end; ++id) {
        EXPECT(more.count[id] >= less.count[id]);
        if (less.count[id]) EXPECT(more.off[id] == less.off[id] + shift);
        shift += up16(more.size(id)) - up16(less.size(id));
    }
    EXPECT(total_more == total_less + shift);
}
// the layout of one call: the counts restated, both carved ranges, and what adding each predicate's blocks moves
static void check_layout(unsigned bits, int B, int H, int N, int M, bool actions, bool f64) {
    const TrShape s = shape_of(bits, M);
    const TrBlocks t = tr_blocks(s, B, H, N, actions, f64);
    const size_t b = (size_t)B, hb = (size_t)H * B, hbn = hb * N, m = s.targeted ? (size_t)M : 0;
    const bool reach = s.sinkhorn && s.unbalanced, div = s.sinkhorn && s.divergence;
    const size_t count[TRB_COUNT] = {b * (H + 1) * N * 3, actions ? hb * 4 : hbn * 3, f64 ? b * N : b * (H + 1) * N, b, b,
                                     hb * m * 3, m ? hb : 0, s.sinkhorn ? b : 0, reach ? b : 0, reach ? hb : 0,
                                     f64 && s.match_in ? hbn : 0, s.given ? hbn * 3 : 0,
                                     hb, f64 ? (size_t)DRP_N_WEIGHTS : 0, f64 && s.chamfer ? hb : 0, s.sinkhorn ? hb : 0, div ? 2 * hb : 0,
                                     div && reach ? hb : 0, f64 && s.match ? 2 * hb : 0, s.match ? hbn : 0, div ? 3 * hb : 0,
                                     div ? 2 * hbn * 3 : 0};
    const size_t elem[TRB_COUNT] = {4, 4, 4, 4, 4, 4, 4, 8, 8, 8, 4, f64 ? (size_t)8 : 4, 8, 8, 8, 8, 8, 8, 8, 4, 8, 8};
    for (int id = 0; id < TRB_COUNT; ++id) EXPECT(t.count[id] == count[id] && t.elem[id] == elem[id]);
    EXPECT(t.res_end == (f64 ? (int)TRB_SCRATCH : (int)TRB_COUNT));     // the float64 scratch is the chunk's, not the batch's
    check_carved(t, TRB_STATES, TRB_IN_END, t.bytes);
    check_carved(t, TRB_TERMS, t.res_end, t.res_bytes);
    EXPECT(t.off[TRB_STATES] == 0 && t.off[TRB_TERMS] == 0);
    for (unsigned bit = 1; bit < 256; bit <<= 1)
        if (bits & bit) {               // without this predicate (a reach without eps: nothing differs, nothing moves)
            const TrBlocks less = tr_blocks(shape_of(bits & ~bit, M), B, H, N, actions, f64);
            check_added(t, less, TRB_STATES, TRB_IN_END, t.bytes, less.bytes);
            check_added(t, less, TRB_TERMS, t.res_end, t.res_bytes, less.res_bytes);
        }
    if (!s.sinkhorn) EXPECT(t.count[TRB_RHO] == 0 && t.count[TRB_MASS_Q] == 0 && t.count[TRB_TRANSPORTED] == 0);
    if (actions) {                      // the pushes shrink the impulse block: nothing else moves ahead of it
        const TrBlocks data = tr_blocks(s, B, H, N, false, f64);
        EXPECT(t.off[TRB_STATES] == data.off[TRB_STATES] && t.off[TRB_IMPULSES] == data.off[TRB_IMPULSES] && t.bytes <= data.bytes);
    }
    if (!f64) {                         // the fp32 arena, restated from its description: kt_unpack_inputs copies it in float4 units
        size_t at = up16(count[0] * 4);
        EXPECT(t.off[TRB_IMPULSES] == at);
        at = up16(at + count[1] * 4);
        EXPECT(t.off[TRB_ATTRS] == at);
        at = up16(at + count[2] * 4);
        EXPECT(t.off[TRB_DENS] == at);
        at = up16(at + b * 4);
        EXPECT(t.off[TRB_NUMS] == at);
        at = up16(at + b * 4);
        if (m) EXPECT(t.off[TRB_TARGETS] == at && t.off[TRB_TNUMS] == up16(at + count[5] * 4));
        EXPECT(t.bytes % 16 == 0 && t.count[TRB_MATCH_IN] == 0 && t.count[TRB_TOTAL] == 0);
    }
}

// One call's copies.  Up: arrays of exactly the caller's sizes staged into a block of exactly `bytes` as train_stage_batch and
// train_grad_f64_body do, read back through tr_view as the kernels address them.  Down: every result row written in full inside a
// block of exactly `res_bytes`, brought back by tr_read_results into arrays of exactly the caller's sizes
static void stage(unsigned bits, int B, int H, int N, int M, bool actions, bool f64) {
    const TrShape s = shape_of(bits, M);
    const TrBlocks t = tr_blocks(s, B, H, N, actions, f64);
    std::vector<std::vector<char>> arr(TRB_COUNT);
    for (int id = 0; id < TRB_COUNT; ++id) arr[id].assign(t.size(id), (char)(id + 1));
    arr[TRB_ATTRS].assign((size_t)B * (H + 1) * N * 4, (char)(TRB_ATTRS + 1));          // the caller's attributes are [B][H+1][N] either way
    auto in = [&](int id) { return arr[id].empty() ? nullptr : arr[id].data(); };
    TrLoss lk;
    lk.targets = reinterpret_cast<const float*>(in(TRB_TARGETS)); lk.target_nums = reinterpret_cast<const int32_t*>(in(TRB_TNUMS));
    lk.eps = reinterpret_cast<const double*>(in(TRB_EPS)); lk.rho = reinterpret_cast<const double*>(in(TRB_RHO));
    lk.mass_q = reinterpret_cast<const double*>(in(TRB_MASS_Q)); lk.match_in = reinterpret_cast<const int32_t*>(in(TRB_MATCH_IN));
    if (f64) lk.seed64 = reinterpret_cast<const double*>(in(TRB_SEED));
    else lk.seed = reinterpret_cast<const float*>(in(TRB_SEED));
    char* pin = static_cast<char*>(std::malloc(t.bytes));
    std::memset(pin, 0xff, t.bytes);
    for (int id = TRB_STATES; id <= TRB_NUMS; ++id)
        if (id == TRB_ATTRS && f64)
            for (int b = 0; b < B; ++b) std::memcpy(pin + t.off[id] + (size_t)b * N * 4, arr[id].data() + (size_t)b * (H + 1) * N * 4, (size_t)N * 4);
        else
            std::memcpy(pin + t.off[id], arr[id].data(), t.size(id));
    tr_stage_loss_inputs(pin, t, lk);
    char* res = static_cast<char*>(std::malloc(t.res_bytes));
    const TrView v = tr_view(pin, res, t);
    const void* seen[TRB_COUNT] = {pin, pin + t.off[TRB_IMPULSES], pin + t.off[TRB_ATTRS], pin + t.off[TRB_DENS], pin + t.off[TRB_NUMS],
                                   v.targets, v.tnums, v.eps, v.rho, v.mass_q, v.match_in, v.seed,
                                   v.terms, v.total, v.margin, v.col_err, v.self_err, v.transported, v.cost, v.match, v.vals, v.gsum};
    for (int id = 0; id < TRB_IN_END; ++id) {           // the staged bytes are the caller's: no copy overwrote another block
        EXPECT((seen[id] != nullptr) == (t.count[id] != 0));
        if (seen[id]) EXPECT(std::memcmp(seen[id], arr[id].data(), t.size(id)) == 0 && reinterpret_cast<uintptr_t>(seen[id]) % t.elem[id] == 0);
    }
    for (int id = TRB_TERMS; id < TRB_COUNT; ++id) {
        EXPECT((seen[id] != nullptr) == (t.count[id] != 0 && id < t.res_end));
        if (seen[id]) {
            EXPECT(seen[id] == res + t.off[id] && t.off[id] + t.size(id) <= t.res_bytes);
            std::memset(res + t.off[id], id + 1, t.size(id));                          // as the kernels write it: in full
        }
    }
    auto out = [&](int id) { arr[id].assign(t.size(id), 0); return arr[id].empty() ? nullptr : arr[id].data(); };
    lk.margin_out = reinterpret_cast<double*>(out(TRB_MARGIN)); lk.col_err_out = reinterpret_cast<double*>(out(TRB_COL_ERR));
    lk.self_err_out = reinterpret_cast<double*>(out(TRB_SELF_ERR)); lk.transported_out = reinterpret_cast<double*>(out(TRB_TRANSPORTED));
    lk.cost_out = reinterpret_cast<double*>(out(TRB_COST)); lk.match_out = reinterpret_cast<int32_t*>(out(TRB_MATCH));
    int copies = 0;
    auto copy = [&copies](void* dst, const void* src, size_t n) { std::memcpy(dst, src, n); ++copies; return 0; };
    EXPECT(tr_read_results(t, res, lk, copy) == 0);
    int present = 0;
    for (int id = TRB_MARGIN; id < TRB_SCRATCH; ++id) {
        present += t.count[id] != 0;
        if (t.count[id]) EXPECT(arr[id].front() == (char)(id + 1) && arr[id].back() == (char)(id + 1));
    }
    EXPECT(copies == present);
    EXPECT(tr_read_results(t, res, TrLoss{}, copy) == 0 && copies == present);          // no caller pointer: nothing is copied
    EXPECT(tr_read_results(t, res, lk, [](void*, const void*, size_t) { return 7; }) == (present ? 7 : 0));    // a copy's error ends the walk
    std::free(res);
    std::free(pin);
}

// the seed block [B][H][N][3] as kt_seed_given (floats) and k64_seed_given (doubles) address it behind a batch of every kind
static void stage_seed(int B, int H, int N, int M, bool actions) {
    const size_t n_seed = (size_t)B * H * N * 3, last = ((size_t)(B - 1) * H + (H - 1)) * N * 3 + (size_t)N * 3 - 1;
    EXPECT(last == n_seed - 1);
    for (unsigned bits : {128u, 128u | 1u, 128u | 1u | 16u, 128u | 1u | 16u | 64u})
        for (int f64 = 0; f64 < 2; ++f64) {
            const TrBlocks t = tr_blocks(shape_of(bits, M), B, H, N, actions, f64 != 0), plain = tr_blocks(shape_of(bits & ~128u, M), B, H, N, actions, f64 != 0);
            EXPECT(plain.count[TRB_SEED] == 0 && plain.off[TRB_SEED] == 0 && t.off[TRB_SEED] == plain.bytes);
            EXPECT(t.bytes == up16(plain.bytes + n_seed * (f64 ? 8 : 4)));
            if (!f64 && (N * 3) % 4 == 0) EXPECT((t.off[TRB_SEED] + ((size_t)(B - 1) * H + (H - 1)) * N * 3 * 4) % 16 == 0);  // its float4 path's premise
        }
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
    if ((argc == 10 || argc == 12) && std::strcmp(argv[1], "layout") == 0) {
        int x[10] = {};
        for (int k = 2; k < argc; ++k) x[k - 2] = std::atoi(argv[k]);
        TrShape s{};
        s.targeted = x[3] > 0; s.M = x[3]; s.sinkhorn = x[5] != 0; s.unbalanced = x[6] != 0; s.given = x[7] != 0; s.match = s.match_in = x[9] != 0;
        const TrBlocks t = tr_blocks(s, x[0], x[1], x[2], x[4] != 0, x[8] != 0);
        const int ids[] = {TRB_STATES, TRB_IMPULSES, TRB_ATTRS, TRB_DENS, TRB_NUMS, TRB_TARGETS, TRB_TNUMS, -1, TRB_EPS, TRB_RHO, TRB_MASS_Q,
                           TRB_SEED, TRB_MATCH_IN};
        for (int k = 0; k < (argc == 10 ? 12 : 13); ++k) std::printf(k ? " %zu" : "%zu", ids[k] < 0 ? t.bytes : t.off[ids[k]]);
        std::printf("\n");
        return 0;
    }
    // odd sizes (no block a multiple of 16 bytes), one sample, the reference's batch, a large one
    const int shapes[][4] = {{1, 1, 1, 0}, {1, 1, 5, 3}, {3, 3, 24, 0}, {3, 3, 23, 17}, {2, 5, 11, 0}, {4, 5, 300, 0}, {4, 5, 300, 300},
                             {7, 2, 301, 299}, {32, 5, 300, 0}, {2, 64, 9, 1}, {3, 3, 5, 3}};
    // the loss shapes the entry points form (targeted 1, chamfer 2, match 4, match_in 8, sinkhorn 16, divergence 32, unbalanced 64,
    // given 128): MSE, Chamfer, match (with a match_in too), the mix (likewise), transport, divergence, with a reach, a given seed
    const unsigned kinds[] = {0, 1 | 2, 1 | 4, 1 | 4 | 8, 1 | 2 | 4, 1 | 2 | 4 | 8, 1 | 16, 1 | 16 | 32, 1 | 16 | 32 | 64, 128};
    for (const auto& s : shapes)
        for (int actions = 0; actions < 2; ++actions) {
            for (int f64 = 0; f64 < 2; ++f64) {
                for (unsigned bits = 0; bits < 256; ++bits) check_layout(bits, s[0], s[1], s[2], s[3], actions != 0, f64 != 0);
                for (unsigned bits : kinds)
                    if (s[3] > 0 || !(bits & 1)) stage(bits, s[0], s[1], s[2], s[3], actions != 0, f64 != 0);
            }
            stage_seed(s[0], s[1], s[2], s[3], actions != 0);
        }
    for (int f64 = 0; f64 < 2; ++f64) stage(1 | 2, 1, 1, 4096, 4096, false, f64 != 0);      // the largest clouds of one (sample, step)
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
    for (unsigned bits : {1u | 16u | 32u, 1u | 16u | 32u | 64u})                               // the divergence's results at its caps
        for (const auto& s : {std::array<int, 3>{4, 5, 100}, std::array<int, 3>{3, 1, 1024}}) stage(bits, s[0], s[1], s[2], s[2], false, false);
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
    {
        // the planner's seed [B][H][N][3] (drp_gd_grad_seeded, drp_gd_grad_f64_seeded): no padding, every coordinate read once and
        // none beyond the block; the index names row, step and particle as the entry points' message splits it
        const int B = 3, H = 2, N = 5;
        const size_t n = (size_t)B * H * N * 3;
        float* s = static_cast<float*>(std::malloc(n * sizeof(float)));                     // exactly [B][H][N][3]
        for (size_t e = 0; e < n; ++e) s[e] = 0.5f - 0.125f * (float)e;
        EXPECT(first_bad_plan_seed(s, B, H, N) == -1);
        s[n - 1] = std::numeric_limits<float>::infinity();                                  // the last coordinate of the block
        EXPECT(first_bad_plan_seed(s, B, H, N) == (long)(B * H * N - 1));
        const long at = ((long)1 * H + 1) * N + 3;                                          // row 1, step 1, particle 3
        s[at * 3 + 1] = std::numeric_limits<float>::quiet_NaN();
        const long bad = first_bad_plan_seed(s, B, H, N);
        EXPECT(bad == at && bad / ((long)H * N) == 1 && (bad / N) % H == 1 && bad % N == 3);
        s[0] = -std::numeric_limits<float>::infinity();
        EXPECT(first_bad_plan_seed(s, B, H, N) == 0);
        std::free(s);
        double* d = static_cast<double*>(std::malloc(n * sizeof(double)));
        for (size_t e = 0; e < n; ++e) d[e] = 1e-300 * (double)(e + 1);                     // tiny is finite
        EXPECT(first_bad_plan_seed(d, B, H, N) == -1);
        d[(size_t)at * 3] = std::numeric_limits<double>::quiet_NaN();
        EXPECT(first_bad_plan_seed(d, B, H, N) == at);
        EXPECT(first_bad_plan_seed(d, 1, 1, 1) == -1);                                      // a smaller view reads no further
        std::free(d);
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
