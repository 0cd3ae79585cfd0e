// k_match_f64.h -- k_match.h's one-to-one matching distance and its gradient with NOTHING in fp32: the yardstick of
// the 'match' and 'chamfer+match' losses, stand-alone (drp_cloud_match_f64) and as the seed of the float64 reverse pass
// (drp_train_grad_f64_match, launched where kc64_chamfer is, or behind it for the mix).  A yardstick like k_chamfer_f64.h, not an
// engine: correctness and one fixed order come before speed.  With r = min(n_p, n_q):
//   C[i][j] = dx*dx + dy*dy + dz*dz in double, in that order, on the double differences of p_i (double: the float64 tape's
//             predicted state, or the caller's doubles) and q_j (the caller's floats, widened where they are loaded);
//             -ffp-contract=off: no fused multiply-add
//   sigma   = the one-to-one matching of the SMALLER cloud's rows into the larger one's that minimises sum C (n_p == n_q: the rows
//             are p's), by k_match.h's shortest augmenting paths: rows inserted in ascending index, among equal shortest reduced
//             costs the lowest column index wins; u, v, shortest distances and reduced costs double
//   term    = scale / (3 r) sum_pairs C, the pairs' costs summed in ascending row index of p
//   d/dp_i  = scale 2 (p_i - q_sigma(i)) / (3 r) for a matched row, +0.0 for an unmatched row and for padding
// A MATCHING GIVEN BY THE CALLER (match_in non-null: every row of p's partner or -1; the entry points have verified it).  The
// term and the gradient are taken on the caller's pairs; the solver runs all the same and its own optimum goes to match_pq,
// match_qp, dual and cost[1].  cost[0] is sum C over the pairs the term used: with the fp32 trainer's partners as match_in the
// gradient's difference from the fp32 one is arithmetic on the SAME pairs, and cost[0] - cost[1] says how far from the double
// optimum those pairs are -- a flipped partner is reported, not mistaken for error.
// One wavefront per problem (sample, rollout step), one problem per workgroup, as ka_match.  Column j belongs to lane j & 63
// whatever the sizes, so the bits do not depend on N, M, B, the padding or the batch around a sample.  Double coordinates of
// 1024 columns do not fit the register file beside v and the distances (ka_match's 16-slot form already fills it), so both
// clouds, u, v, the distances and the three index arrays are in dynamic LDS, sized by the padded size L = max(N, M) rounded up to
// 64: p as three double arrays 24 L, u / v / distances 24 L, q as float4 16 L, three index arrays 12 L = 76 bytes per point,
// 76 KB at the cap (above the static limit: the context sets the function's attribute once, at first use).  Only the scanned
// bits (16 per lane) stay in a register.  A lane reads and writes its own columns' v, distance and predecessor only; what lanes
// read of each other (the row of a column, u) is written between the two barriers of the augmentation.  The arg-min is the
// six-step xor-shuffle of (double, index).  No atomics.
// NO INPUT PROLONGS A LOOP, as in ka_match: row i's search is a `for` over i + 1 iterations, the flip walks at most i + 1
// columns, no loop waits on a floating-point condition.  A non-finite prediction makes comparisons false, the search takes the
// lowest unscanned columns, the matching stays one-to-one and the term comes out NaN or inf after the same number of steps.
#pragma once
#include "k_cloud_pair.h"
#include "k_match.h"            // KA_MAX_POINTS: the cap is the fp32 kernel's

#define KA64_THREADS 64
#define KA64_PAD(n) ((((n) < KA_MAX_POINTS ? (n) : KA_MAX_POINTS) + 63) & ~63)
#define KA64_LDS(L) ((size_t)(L) * 76)

struct Ka64Args {
    const double* pred;         // p's rows (cp's strides); the trainer: the chunk's
    CloudPair cp;               // q and the counts are the batch's: sample b_off + b
    int b_off;                  // the chunk's first sample (p and grad are the chunk's, everything else the batch's); one-shot: 0
    int B;                      // samples of the batch: slot (t, b_off + b) of everything but grad is t * B + b_off + b
    double scale;
    double keep;                // the mix: kc64_chamfer<true> ran before with the whole Chamfer term -- grad and terms become
                                // keep * (what is there) + this kernel's share; 0: they are written
    const int* match_in;        // [H][B][N], nullable: the pairs of the term and the gradient
    double* grad;               // [H][gridDim.x][N][3], every row written (or combined), nullable
    double* terms;              // [H][B]
    int* match_pq;              // [H][B][N] the optimum's partner of every row of p (-1: unmatched, padding), nullable
    int* match_qp;              // [H][B][M], nullable
    double* dual;               // [H][B][N + M]: the optimum's duals of p's rows, then of q's (0 on padding), nullable
    double* cost;               // [H][B][2]: sum C over the pairs the term used, over the optimum's; nullable
};

// grid (samples, steps), KA64_LDS(KA64_PAD(max(N, M))) bytes of dynamic LDS
__global__ void __launch_bounds__(KA64_THREADS) ka64_match(Ka64Args A) {
    extern __shared__ __align__(16) unsigned char ka64_lds[];
    const int b = blockIdx.x, t = blockIdx.y, nb = gridDim.x;
    const int lane = threadIdx.x;
    const int N = A.cp.N, M = A.cp.M;
    const int L = KA64_PAD(N > M ? N : M);
    double* s_px = reinterpret_cast<double*>(ka64_lds);
    double* s_py = s_px + L;
    double* s_pz = s_py + L;
    double* s_u = s_pz + L;                                 // the rows' duals
    double* s_v = s_u + L;                                  // the columns'
    double* s_sh = s_v + L;                                 // the columns' shortest distances
    float4* s_q = reinterpret_cast<float4*>(s_sh + L);
    int* s_colof = reinterpret_cast<int*>(s_q + L);         // row -> its column, -1
    int* s_rowof = s_colof + L;                             // column -> its row, -1
    int* s_pred = s_rowof + L;                              // column -> the row its shortest path comes through
    const int bb = A.b_off + b;                             // the sample in the batch's arrays
    const int np = A.cp.count_p(bb, KA_MAX_POINTS), nq = A.cp.count_q(bb, t, KA_MAX_POINTS);
    const double* p = A.cp.p_rows(A.pred, b, t);
    const float* q = A.cp.q_rows(bb, t);
    const size_t slot = (size_t)t * A.B + bb;
    double* g = A.grad != nullptr ? A.grad + ((size_t)t * nb + b) * N * 3 : nullptr;
    const int* m_in = A.match_in != nullptr ? A.match_in + slot * N : nullptr;
    int* m_pq = A.match_pq != nullptr ? A.match_pq + slot * N : nullptr;
    int* m_qp = A.match_qp != nullptr ? A.match_qp + slot * M : nullptr;
    double* dual = A.dual != nullptr ? A.dual + slot * ((size_t)N + M) : nullptr;
    const bool rows_q = np > nq;                            // the rows are the smaller cloud's; p's where the counts are equal
    const int nr = rows_q ? nq : np, nc = rows_q ? np : nq;
    const int cpl = (nc + 63) >> 6;
    const double inf = __builtin_inf();

    for (int e = lane; e < L; e += KA64_THREADS) {
        double x = 0.0, y = 0.0, z = 0.0;
        if (e < np) { x = p[(size_t)e * 3]; y = p[(size_t)e * 3 + 1]; z = p[(size_t)e * 3 + 2]; }
        s_px[e] = x; s_py[e] = y; s_pz[e] = z;
        float4 q4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (e < nq) q4 = make_float4(q[(size_t)e * 3], q[(size_t)e * 3 + 1], q[(size_t)e * 3 + 2], 0.0f);
        s_q[e] = q4;
        s_u[e] = 0.0; s_v[e] = 0.0;
        s_colof[e] = -1; s_rowof[e] = -1;
    }
    __syncthreads();
    // |p_pi - q_qi|^2
    auto cost_of = [&](int pi, int qi) {
        const float4 q4 = s_q[qi];
        const double dx = s_px[pi] - (double)q4.x, dy = s_py[pi] - (double)q4.y, dz = s_pz[pi] - (double)q4.z;
        return dx * dx + dy * dy + dz * dz;
    };

    for (int i = 0; i < nr; ++i) {
        // ---- the shortest paths from row i over reduced costs, until a free column is scanned ----
        unsigned scanned = 0;
        for (int k = 0; k < cpl; ++k) {
            const int j = k * 64 + lane;
            if (j < nc) { s_sh[j] = inf; s_pred[j] = i; }   // a column no finite cost ever reaches hangs on the inserted row
        }
        int cur = i, sink = -1;
        double minval = 0.0;
        for (int it = 0; it <= i; ++it) {
            const double ucur = s_u[cur];
            double best = inf;
            int bj = 0x7fffffff;
            for (int k = 0; k < cpl; ++k) {
                const int j = k * 64 + lane;
                if (j < nc && !((scanned >> k) & 1u)) {
                    const double cost = rows_q ? cost_of(j, cur) : cost_of(cur, j);
                    const double d = minval + cost - ucur - s_v[j];
                    double sh = s_sh[j];
                    if (d < sh) { sh = d; s_sh[j] = d; s_pred[j] = cur; }
                    if (bj == 0x7fffffff || sh < best) { best = sh; bj = j; }   // ascending j: the lowest on a tie
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ob = __shfl_xor(best, off, 64);
                const int oj = __shfl_xor(bj, off, 64);
                if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
            }
            if (bj == 0x7fffffff) break;                    // (no unscanned column: cannot happen while it <= i < nc)
            minval = best;
            if (lane == (bj & 63)) scanned |= 1u << (bj >> 6);
            const int rj = s_rowof[bj];
            if (rj < 0) { sink = bj; break; }
            cur = rj;
        }
        // ---- duals: the scanned columns and their rows, then the inserted row ----
        for (int k = 0; k < cpl; ++k)
            if ((scanned >> k) & 1u) {
                const int j = k * 64 + lane;
                const double delta = minval - s_sh[j];
                s_v[j] -= delta;
                const int rj = s_rowof[j];
                if (rj >= 0) s_u[rj] += delta;              // one column per row: one writer
            }
        if (lane == 0) s_u[i] += minval;                    // (row i has no column yet: nobody else wrote it)
        __syncthreads();
        // ---- augment along the predecessors: at most i + 1 columns ----
        if (lane == 0 && sink >= 0) {
            int j = sink;
            for (int s = 0; s <= i; ++s) {
                const int i2 = s_pred[j];
                s_rowof[j] = i2;
                const int jp = s_colof[i2];
                s_colof[i2] = j;
                j = jp;
                if (i2 == i || j < 0) break;
            }
        }
        __syncthreads();
    }

    // ---- the optimum's duals and q's partners ----
    if (dual != nullptr) {
        for (int e = lane; e < N; e += KA64_THREADS) dual[e] = e < np ? (rows_q ? s_v[e] : s_u[e]) : 0.0;
        for (int e = lane; e < M; e += KA64_THREADS) dual[(size_t)N + e] = e < nq ? (rows_q ? s_u[e] : s_v[e]) : 0.0;
    }
    if (m_qp != nullptr)
        for (int e = lane; e < M; e += KA64_THREADS) m_qp[e] = e < nq ? (rows_q ? s_colof[e] : s_rowof[e]) : -1;
    __syncthreads();                                        // v and the distances are done with: they take the rows' costs
    // ---- every row of p: its partners (the optimum's, the term's), its cost under each, its gradient ----
    const double inv = nr > 0 ? A.scale / (3.0 * (double)nr) : 0.0;
    const bool add = A.keep != 0.0;
    const double keep = A.keep;
    for (int e = lane; e < np; e += KA64_THREADS) {
        const int jo = rows_q ? s_rowof[e] : s_colof[e];
        int ju = jo;
        if (m_in != nullptr) { ju = m_in[e]; if (ju < 0 || ju >= nq) ju = -1; }
        const double c_opt = jo >= 0 ? cost_of(e, jo) : 0.0;
        double c_use = c_opt, gx = 0.0, gy = 0.0, gz = 0.0;     // an unmatched row's share is +0.0
        if (ju >= 0) {
            const float4 q4 = s_q[ju];
            const double dx = s_px[e] - (double)q4.x, dy = s_py[e] - (double)q4.y, dz = s_pz[e] - (double)q4.z;
            c_use = dx * dx + dy * dy + dz * dz;
            gx = 2.0 * dx * inv; gy = 2.0 * dy * inv; gz = 2.0 * dz * inv;
        } else {
            c_use = 0.0;
        }
        s_sh[e] = c_use; s_v[e] = c_opt;
        if (g != nullptr) {
            double* gp = g + (size_t)e * 3;
            if (add) { gp[0] = keep * gp[0] + gx; gp[1] = keep * gp[1] + gy; gp[2] = keep * gp[2] + gz; }
            else { gp[0] = gx; gp[1] = gy; gp[2] = gz; }
        }
        if (m_pq != nullptr) m_pq[e] = jo;
    }
    // padding: gradient exactly +0.0 (the mix: the Chamfer kernel's zeros stay), no partner
    if (g != nullptr && !add)
        for (int e = np * 3 + lane; e < N * 3; e += KA64_THREADS) g[e] = 0.0;
    if (m_pq != nullptr)
        for (int e = np + lane; e < N; e += KA64_THREADS) m_pq[e] = -1;
    __syncthreads();
    if (lane == 0) {                                        // one fixed order: ascending row of p
        double used = 0.0, opt = 0.0;
        for (int e = 0; e < np; ++e) { used += s_sh[e]; opt += s_v[e]; }
        const double term = used * inv;
        A.terms[slot] = add ? keep * A.terms[slot] + term : term;
        if (A.cost != nullptr) { A.cost[slot * 2] = used; A.cost[slot * 2 + 1] = opt; }
    }
}

// one wavefront per problem on grid (samples, steps); the entry points hold N, M <= KA_MAX_POINTS.  The dynamic LDS at the cap is
// above the 64 KB a function may use unasked: the caller has set the function's attribute (capi_match_f64.h: ka64_run)
inline void ka64_launch(dim3 grid, hipStream_t st, const Ka64Args& a) {
    const int L = KA64_PAD(a.cp.N > a.cp.M ? a.cp.N : a.cp.M);
    hipLaunchKernelGGL(ka64_match, grid, dim3(KA64_THREADS), KA64_LDS(L), st, a);
}
