// One-to-one matching (earth mover's) distance of two padded cloud batches and its gradient: the loss that sees
// density, which the Chamfer distance of k_chamfer.h does not.  With r = min(n_p, n_q):
//   C[i][j] = |p_i - q_j|^2 in fp32, formed as kc_chamfer forms it (fp32 differences, dx*dx + dy*dy + dz*dz, no fused multiply-add)
//   sigma   = the one-to-one matching of the SMALLER cloud's rows into the larger one's that minimises sum C (rectangular
//             linear assignment; n_p == n_q: the rows are p's)
//   match   = scale / (3 r) sum_pairs |p_i - q_j|^2      (each pair's squared fp32 differences summed in double)
//   d/dp_i  = scale 2 (p_i - q_sigma(i)) / (3 r) for a matched row, +0.0 for an unmatched row (n_p > n_q) and for padding
//             (sigma is a constant of the derivative, as the Chamfer arg-mins are)
// Exact shortest augmenting paths (Jonker-Volgenant / Crouse's rectangular form): rows of the smaller cloud are inserted in
// ascending index, a Dijkstra search over reduced costs finds the nearest free column, duals u (rows), v (columns), the running
// shortest distances and the reduced costs are DOUBLE (the fp32 costs widen exactly); no epsilon, the result is the optimum.
// Among equal shortest reduced costs the lowest column index wins.
// One wavefront per problem (sample, rollout step), one problem per workgroup.  The columns (the larger cloud) are striped
// over the 64 lanes, column j on lane j & 63 in slot j >> 6, at most KA_CPL = 16 per lane (the kernel is instantiated for 1, 2,
// 4, 8 and 16 slots and launched by the padded size): a lane keeps its columns' coordinates,
// v, the shortest distances and the scanned bits in registers.  The rows' coordinates and u, and what the augmentation walks
// (predecessor row of a column, row of a column, column of a row) are in LDS: 16 + 8 + 3 x 4 = 36 KB.  The cost matrix is
// never stored.  The search's arg-min is a (value, index) xor-shuffle over the wave: no barrier in the inner loop.  No atomics:
// the same bits from run to run and for a sample alone or inside any batch.
// NO INPUT PROLONGS A LOOP.  Every trip count is fixed by r and c: row i's search scans one new column per iteration and at most
// i columns are taken, so its `for` over i + 1 iterations always meets a free column -- whatever the values; the augmentation
// walks at most i + 1 columns.  No loop waits on a floating-point condition.  A non-finite coordinate (a diverged model) makes
// comparisons false, the search then takes the lowest unscanned columns with the inserted row as predecessor, the matching stays
// one-to-one and the term comes out NaN or inf -- after the same number of steps.
#pragma once
#include "k_cloud_pair.h"

#define KA_THREADS 64
#define KA_MAX_POINTS 1024      // per cloud: the work is O(r^2) dependent steps of O(c / 64) each
#define KA_CPL (KA_MAX_POINTS / 64)

struct KaArgs {
    const float* pred;          // p's rows (cp's strides)
    CloudPair cp;
    double scale;
    double keep;                // TRAIN, the mix: kc_chamfer<true> ran before with the whole Chamfer term -- grad and terms become
                                // keep * (what is there) + this kernel's share, one rounding per element; 0: they are written
    float* grad;                // TRAIN: [H][B][N][3], every row written (or combined); else [B][N][3], nullable
    double* terms;              // TRAIN: [H][B], scale * match (or keep * Chamfer + that); else [B]
    int* match_pq;              // [slot][N] partner of every predicted row (-1: unmatched, padding), nullable
    int* match_qp;              // [B][M], nullable; not TRAIN only
    double* dual;               // [B][N + M]: the duals of p's rows, then of q's (0 on padding), nullable; not TRAIN only
    float* zero; size_t n_zero; // TRAIN, nullable: filled with 0 (the gradient blob and kmb_step_bwd's counters, as kt_mse_grad does)
};

// CPL: the column slots a lane holds, 64 * CPL >= max(N, M) (ka_launch picks 1, 2, 4, 8 or 16: a 100-point problem does not carry
// the registers of a 1024-point one).  Column j is slot j >> 6 of lane j & 63 whatever CPL is: the bits do not depend on it.
template <bool TRAIN, int CPL>
__global__ void __launch_bounds__(KA_THREADS) ka_match(KaArgs A) {
    __shared__ float4 s_row[KA_MAX_POINTS];     // the smaller cloud
    __shared__ double s_u[KA_MAX_POINTS];       // its duals
    __shared__ int s_colof[KA_MAX_POINTS];      // row -> its column, -1
    __shared__ int s_rowof[KA_MAX_POINTS];      // column -> its row, -1
    __shared__ int s_pred[KA_MAX_POINTS];       // column -> the row its shortest path comes through
    const int b = blockIdx.x, t = blockIdx.y, B = gridDim.x;
    const int lane = threadIdx.x;
    const int N = A.cp.N, M = A.cp.M;
    if (TRAIN) train_zero_fill(A.zero, A.n_zero, KA_THREADS);
    const int np = A.cp.count_p(b, 64 * CPL), nq = A.cp.count_q(b, t, 64 * CPL);
    const float* p = A.cp.p_rows(A.pred, b, t);
    const float* q = A.cp.q_rows(b, t);
    const size_t slot = (size_t)t * B + b;
    float* g = A.grad != nullptr ? A.grad + slot * N * 3 : nullptr;
    int* m_pq = A.match_pq != nullptr ? A.match_pq + slot * N : nullptr;
    int* m_qp = (!TRAIN && A.match_qp != nullptr) ? A.match_qp + slot * M : nullptr;
    double* dual = (!TRAIN && A.dual != nullptr) ? A.dual + slot * ((size_t)N + M) : nullptr;
    const bool rows_q = np > nq;                            // the rows are the smaller cloud's; p's where the counts are equal
    const int nr = rows_q ? nq : np, nc = rows_q ? np : nq;
    const float* rowp = rows_q ? q : p;
    const float* colp = rows_q ? p : q;
    const int cpl = (nc + 63) >> 6;
    const double inf = (double)__builtin_inff();

    float cx[CPL], cy[CPL], cz[CPL];
    double v[CPL], sh[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int j = k * 64 + lane;
        cx[k] = cy[k] = cz[k] = 0.0f;
        v[k] = 0.0; sh[k] = inf;
        if (j < nc) { cx[k] = colp[(size_t)j * 3]; cy[k] = colp[(size_t)j * 3 + 1]; cz[k] = colp[(size_t)j * 3 + 2]; }
    }
    for (int e = lane; e < KA_MAX_POINTS; e += KA_THREADS) {
        float4 r4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (e < nr) r4 = make_float4(rowp[(size_t)e * 3], rowp[(size_t)e * 3 + 1], rowp[(size_t)e * 3 + 2], 0.0f);
        s_row[e] = r4;
        s_u[e] = 0.0;
        s_colof[e] = -1;
        s_rowof[e] = -1;
    }
    __syncthreads();

    for (int i = 0; i < nr; ++i) {
        // ---- the shortest paths from row i over reduced costs, until a free column is scanned ----
        unsigned scanned = 0;
#pragma unroll
        for (int k = 0; k < CPL; ++k)
            if (k < cpl) {
                sh[k] = inf;
                const int j = k * 64 + lane;
                if (j < nc) s_pred[j] = i;          // a column no finite cost ever reaches hangs on the inserted row
            }
        int cur = i, sink = -1;
        double minval = 0.0;
        for (int it = 0; it <= i; ++it) {
            const float4 rp = s_row[cur];
            const double ucur = s_u[cur];
            double best = inf;
            int bj = 0x7fffffff;
#pragma unroll
            for (int k = 0; k < CPL; ++k)
                if (k < cpl) {
                    const int j = k * 64 + lane;
                    if (j < nc && !((scanned >> k) & 1u)) {
                        const float dx = rp.x - cx[k], dy = rp.y - cy[k], dz = rp.z - cz[k];
                        const float cost = dx * dx + dy * dy + dz * dz;
                        const double d = minval + (double)cost - ucur - v[k];
                        if (d < sh[k]) { sh[k] = d; s_pred[j] = cur; }
                        if (bj == 0x7fffffff || sh[k] < best) { best = sh[k]; bj = j; }     // ascending j: the lowest on a tie
                    }
                }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ob = __shfl_xor(best, off, 64);
                const int oj = __shfl_xor(bj, off, 64);
                if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
            }
            if (bj == 0x7fffffff) break;            // (no unscanned column: cannot happen while it <= i < nc)
            minval = best;
            if (lane == (bj & 63)) scanned |= 1u << (bj >> 6);
            const int rj = s_rowof[bj];
            if (rj < 0) { sink = bj; break; }
            cur = rj;
        }
        // ---- duals: the scanned columns and their rows, then the inserted row ----
#pragma unroll
        for (int k = 0; k < CPL; ++k)
            if (k < cpl && ((scanned >> k) & 1u)) {
                const int j = k * 64 + lane;
                const double delta = minval - sh[k];
                v[k] -= delta;
                const int rj = s_rowof[j];
                if (rj >= 0) s_u[rj] += delta;      // one column per row: one writer
            }
        if (lane == 0) s_u[i] += minval;            // (row i has no column yet: nobody else wrote it)
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

    // ---- the pairs: term, gradient, partners, duals; every column's lane writes its pair ----
    const double inv = nr > 0 ? A.scale / (3.0 * (double)nr) : 0.0;
    const bool add = TRAIN && A.keep != 0.0;
    const double keep = A.keep;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < CPL; ++k)
        if (k < cpl) {
            const int j = k * 64 + lane;
            if (j < nc) {
                const int i = s_rowof[j];
                double gx = 0.0, gy = 0.0, gz = 0.0;               // an unmatched row's share is +0.0
                if (i >= 0) {
                    const float4 rp = s_row[i];
                    // p - q, whichever of them the rows are
                    const float dx = rows_q ? cx[k] - rp.x : rp.x - cx[k], dy = rows_q ? cy[k] - rp.y : rp.y - cy[k],
                                dz = rows_q ? cz[k] - rp.z : rp.z - cz[k];
                    acc += (double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz;
                    gx = 2.0 * (double)dx * inv; gy = 2.0 * (double)dy * inv; gz = 2.0 * (double)dz * inv;
                }
                const int pi = rows_q ? j : i, qi = rows_q ? i : j;     // this pair's rows of p and of q (one of them may be -1)
                if (pi >= 0) {
                    if (g != nullptr) {
                        float* gp = g + (size_t)pi * 3;
                        if (add) {              // rounded once
                            gp[0] = (float)(keep * (double)gp[0] + gx); gp[1] = (float)(keep * (double)gp[1] + gy);
                            gp[2] = (float)(keep * (double)gp[2] + gz);
                        } else {
                            gp[0] = (float)gx; gp[1] = (float)gy; gp[2] = (float)gz;
                        }
                    }
                    if (m_pq != nullptr) m_pq[pi] = qi;
                }
                if (qi >= 0 && m_qp != nullptr) m_qp[qi] = pi;
                if (dual != nullptr) dual[rows_q ? (size_t)j : (size_t)N + j] = v[k];
            }
        }
    if (dual != nullptr) {
        for (int e = lane; e < nr; e += KA_THREADS) dual[rows_q ? (size_t)N + e : (size_t)e] = s_u[e];
        for (int e = np + lane; e < N; e += KA_THREADS) dual[e] = 0.0;
        for (int e = nq + lane; e < M; e += KA_THREADS) dual[(size_t)N + e] = 0.0;
    }
    // padding: gradient exactly 0 (the mix: the Chamfer kernel's zeros stay), no partner
    if (g != nullptr && !add)
        for (int e = np * 3 + lane; e < N * 3; e += KA_THREADS) g[e] = 0.0f;
    if (m_pq != nullptr)
        for (int e = np + lane; e < N; e += KA_THREADS) m_pq[e] = -1;
    if (m_qp != nullptr)
        for (int e = nq + lane; e < M; e += KA_THREADS) m_qp[e] = -1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);     // one fixed order: slots in a lane, then lanes
    if (lane == 0) {
        const double term = acc * inv;
        A.terms[slot] = add ? keep * A.terms[slot] + term : term;
    }
}

// one wavefront per problem on grid (B, H); the instantiation by the larger padded size (the entry points hold N, M <= KA_MAX_POINTS)
template <bool TRAIN>
inline void ka_launch(dim3 grid, hipStream_t st, const KaArgs& a) {
    const int c = a.cp.N > a.cp.M ? a.cp.N : a.cp.M;
    if (c <= 64) hipLaunchKernelGGL((ka_match<TRAIN, 1>), grid, dim3(KA_THREADS), 0, st, a);
    else if (c <= 128) hipLaunchKernelGGL((ka_match<TRAIN, 2>), grid, dim3(KA_THREADS), 0, st, a);
    else if (c <= 256) hipLaunchKernelGGL((ka_match<TRAIN, 4>), grid, dim3(KA_THREADS), 0, st, a);
    else if (c <= 512) hipLaunchKernelGGL((ka_match<TRAIN, 8>), grid, dim3(KA_THREADS), 0, st, a);
    else hipLaunchKernelGGL((ka_match<TRAIN, KA_CPL>), grid, dim3(KA_THREADS), 0, st, a);
}
