// k_cloud_goal.h -- the planners' reward against ONE target cloud shared by every row (capi_cloud_goal.h): the
// symmetric Chamfer distance or the Sinkhorn divergence of each row's final predicted state to the installed cloud, written
// as reward = (float)(-(weight * value)) straight into the slot the update kernels read, and with GRAD the gradient
// weight * d value / d state_{H-1} where the reverse pass starts.
//   kg_chamfer<GRAD>          grid (rows), KC_THREADS.  kc_chamfer<false>'s arithmetic on (row's state, target): kc_nearest and
//                             kc_block_sum, the same fp32 distance expression, the same strict `<` over ascending j, the same
//                             order of every sum -- fwd and bwd are drp_cloud_chamfer's bits on the same pair.  Without GRAD the
//                             c(.) table, its walk and every gradient store are compiled out (the sampling planners).
//   kg_target_self            grid (columns), KT_THREADS.  The target's self problem depends on the target and eps alone: once
//                             per session (and per one-shot), one value sum per start column.
//   kg_sinkhorn<GRAD>         grid (rows, 2), KT_THREADS: y = 0 the cross problem, y = 1 the prediction's self problem
//                             (sk_cross_problem, sk_self_problem: k_sinkhorn.h's bodies, so every sum is ordered by the counts
//                             alone and the values are drp_cloud_divergence's bits with scale 1).  Without GRAD no pass over a
//                             plan's rows runs: sweeps and the value sums only.
//   kg_sinkhorn_combine<GRAD> grid (rows), KD_COMBINE_THREADS: cross - self_p - table[row % n_batch], the reward, the gradient.
// A row's cloud is read at states + row * row_stride (a session: the final step of [rows][H][N][3]); the target with batch
// stride 0.  eps and the target's table are per start column: column = cloud_goal::column_of_row(row, n_batch).
// NO VALUE PROLONGS A LOOP (k_sinkhorn.h): every trip count is fixed by N, M, the counts and K.  A row with a non-finite
// coordinate ends in a NaN reward after the same number of steps; no block reads another row, so the other rows' bits stay.
// No atomics.  LDS (static): kg_chamfer<true> 16 KB tile + 16 KB c(.), kg_chamfer<false> the tile alone; kg_sinkhorn and
// kg_target_self 48 KB as kd_sweeps (three problems, 24 wavefronts, a CU).
#pragma once
#include "k_chamfer.h"
#include "k_sinkhorn.h"
#include "cloud_goal_host.h"        // cloud_goal::column_of_row: rows to start columns, the host's definition

struct KgArgs {
    const float* states;        // row b's cloud [N][3] at states + b * row_stride
    size_t row_stride;
    const int* n_p;             // [rows] real rows of each cloud, nullable: all N (the sessions)
    const float* q;             // the target [M][3], shared by every row
    int N, M;
    double weight;
    float* rewards;             // rewards[b * reward_stride] = (float)(-(weight * value)); nullable
    size_t reward_stride;
    float* host_rewards;        // [rows], nullable: the same rewards, dense (pinned host memory of drp_gd_step_async)
    double* values;             // [rows], nullable: weight * value before the sign and the rounding (the one-shot)
    float* grad;                // GRAD: row b's [N][3] at grad + b * grad_stride, every row written (padding +0.0)
    size_t grad_stride;
    // the Sinkhorn kind
    const double* eps;          // [n_batch]
    const double* self_q;       // [n_batch]: the target's self problem's value sum (kg_target_self)
    int n_batch, iters;
    double* vals;               // scratch [2][rows]: the cross problem's value sum | the prediction's self problem's
    double* gsum;               // scratch [2][rows][N][3]: sum_j P_ij (p_i - q_j) | sum_j S^p_ij (p_i - p_j); GRAD only
};

__device__ __forceinline__ int kg_count(const KgArgs& A, int b, int cap) {
    return A.n_p != nullptr ? min(max(A.n_p[b], 0), min(A.N, cap)) : min(A.N, cap);
}
__device__ __forceinline__ void kg_store_value(const KgArgs& A, int b, double value) {
    const float r = (float)(-value);
    if (A.rewards != nullptr) A.rewards[(size_t)b * A.reward_stride] = r;
    if (A.host_rewards != nullptr) A.host_rewards[b] = r;
    if (A.values != nullptr) A.values[b] = value;
}

template <bool GRAD>
__global__ void __launch_bounds__(KC_THREADS) kg_chamfer(KgArgs A) {
    __shared__ float4 s_tile[KC_TILE];
    __shared__ int s_c[GRAD ? KC_MAX_POINTS : 1];
    __shared__ double s_w[4];
    const int b = blockIdx.x;
    const int N = A.N;
    const int np = kg_count(A, b, KC_MAX_POINTS), nq = min(A.M, KC_MAX_POINTS);
    const float* p = A.states + (size_t)b * A.row_stride;
    const float* q = A.q;
    float* g = GRAD ? A.grad + (size_t)b * A.grad_stride : nullptr;
    const bool empty = np == 0 || nq == 0;
    // (kc_chamfer's scale is the float 1: x 1.0 is exact)
    const double inv_p = empty ? 0.0 : 1.0 / (3.0 * (double)np), inv_q = empty ? 0.0 : 1.0 / (3.0 * (double)nq);

    // c(j) of every target row (GRAD: into LDS); the backward sum
    double acc_b = 0.0;
    for (int j0 = 0; j0 < (empty ? 0 : nq); j0 += KC_THREADS) {
        const int j = j0 + threadIdx.x;
        const bool live = j < nq;
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (live) { x = q[(size_t)j * 3]; y = q[(size_t)j * 3 + 1]; z = q[(size_t)j * 3 + 2]; }
        const int c = kc_nearest(x, y, z, live, p, np, s_tile);
        if (live) {
            const float dx = x - p[(size_t)c * 3], dy = y - p[(size_t)c * 3 + 1], dz = z - p[(size_t)c * 3 + 2];
            acc_b += (double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz;
            if (GRAD) s_c[j] = c;
        }
    }
    __syncthreads();                                        // s_c is complete

    // a(i) of every predicted row, the forward sum, and with GRAD the row's gradient: its own term, then its entries of c(.)
    double acc_f = 0.0;
    for (int i0 = 0; i0 < (empty ? 0 : np); i0 += KC_THREADS) {
        const int i = i0 + threadIdx.x;
        const bool live = i < np;
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (live) { x = p[(size_t)i * 3]; y = p[(size_t)i * 3 + 1]; z = p[(size_t)i * 3 + 2]; }
        const int a = kc_nearest(x, y, z, live, q, nq, s_tile);
        if (live) {
            const float dx = x - q[(size_t)a * 3], dy = y - q[(size_t)a * 3 + 1], dz = z - q[(size_t)a * 3 + 2];
            acc_f += (double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz;
            if (GRAD) {
                double sx = 0.0, sy = 0.0, sz = 0.0;
                for (int j = 0; j < nq; ++j)
                    if (s_c[j] == i) {
                        sx += (double)(x - q[(size_t)j * 3]); sy += (double)(y - q[(size_t)j * 3 + 1]); sz += (double)(z - q[(size_t)j * 3 + 2]);
                    }
                // kc_chamfer's double, times the weight, rounded once
                g[(size_t)i * 3] = (float)(A.weight * (2.0 * (double)dx * inv_p + 2.0 * sx * inv_q));
                g[(size_t)i * 3 + 1] = (float)(A.weight * (2.0 * (double)dy * inv_p + 2.0 * sy * inv_q));
                g[(size_t)i * 3 + 2] = (float)(A.weight * (2.0 * (double)dz * inv_p + 2.0 * sz * inv_q));
            }
        }
    }
    if (GRAD)                                               // padding: gradient exactly 0
        for (int e = (empty ? 0 : np) * 3 + threadIdx.x; e < N * 3; e += KC_THREADS) g[e] = 0.0f;

    const double sum_f = kc_block_sum(acc_f, s_w);
    const double sum_b = kc_block_sum(acc_b, s_w);
    if (threadIdx.x == 0) {
        const double fwd = sum_f * inv_p, bwd = sum_b * inv_q;
        kg_store_value(A, b, A.weight * (fwd + bwd));
    }
}

// what sk_cross_problem and sk_self_problem read of a problem: the counts, eps and the sweeps (balanced: no reach, mass 1)
__device__ __forceinline__ SkProblem<float> kg_problem(const KgArgs& A, int b, int col) {
    SkProblem<float> pr;
    pr.np = kg_count(A, b, KT_MAX_POINTS); pr.nq = min(A.M, KT_MAX_POINTS);
    pr.rows_p = A.states + (size_t)b * A.row_stride;
    pr.rows_q = A.q;
    pr.slot = pr.oslot = (size_t)b; pr.slots = gridDim.x;
    pr.empty = pr.np == 0 || pr.nq == 0;
    pr.iters = pr.empty ? 0 : min(max(A.iters, 0), KT_MAX_ITERS);
    pr.eps = A.eps[col];
    pr.R = KdReach{};
    pr.w = 1.0;
    return pr;
}

// the target's self problem per start column: out[col] = sum_j b h^q_j at eps[col]
__global__ void __launch_bounds__(KT_THREADS) kg_target_self(KgArgs A, double* out) {
    __shared__ float4 s_q[KT_MAX_POINTS];
    __shared__ double s_f[KT_MAX_POINTS];
    __shared__ double s_g[KT_MAX_POINTS];
    __shared__ double s_w[KT_WAVES];
    const int col = blockIdx.x;
    const int nq = min(A.M, KT_MAX_POINTS);
    const int iters = nq == 0 ? 0 : min(max(A.iters, 0), KT_MAX_ITERS);
    sk_load(s_q, A.q, nq);
    sk_self_problem<false>(SkPts32{s_q}, nq, A.M, nq == 0, iters, A.eps[col], s_f, s_g, s_w, out + col, (double*)nullptr,
                           (double*)nullptr, (double*)nullptr, KdReach{}, 1.0);
}

template <bool GRAD>
__global__ void __launch_bounds__(KT_THREADS) kg_sinkhorn(KgArgs A) {
    __shared__ float4 s_p[KT_MAX_POINTS];       // the row's state (cross and self)
    __shared__ float4 s_q[KT_MAX_POINTS];       // the target (cross)
    __shared__ double s_f[KT_MAX_POINTS];       // cross: f; self: h of the even sweeps
    __shared__ double s_g[KT_MAX_POINTS];       // cross: g; self: h of the odd sweeps
    __shared__ double s_w[KT_WAVES];
    const int b = blockIdx.x, rows = gridDim.x;
    const size_t n3 = (size_t)A.N * 3;
    const SkProblem<float> pr = kg_problem(A, b, cloud_goal::column_of_row(b, A.n_batch));
    sk_load(s_p, pr.rows_p, pr.np);
    if (blockIdx.y == 0) {
        sk_load(s_q, pr.rows_q, pr.nq);
        (void)sk_cross_problem<false, false>(pr, A.N, A.M, SkPts32{s_p}, SkPts32{s_q}, s_f, s_g, s_w, A.vals + b, (double*)nullptr,
                                             GRAD ? A.gsum + (size_t)b * n3 : (double*)nullptr, 0.0, (double*)nullptr, (double*)nullptr);
    } else {
        sk_self_problem<false>(SkPts32{s_p}, pr.np, A.N, pr.empty, pr.iters, pr.eps, s_f, s_g, s_w, A.vals + rows + b, (double*)nullptr,
                               GRAD ? A.gsum + ((size_t)rows + b) * n3 : (double*)nullptr, (double*)nullptr, pr.R, 1.0);
    }
}

template <bool GRAD>
__global__ void __launch_bounds__(KD_COMBINE_THREADS) kg_sinkhorn_combine(KgArgs A) {
    const int b = blockIdx.x, rows = gridDim.x;
    const int tid = threadIdx.x;
    const int N = A.N;
    const int np = kg_count(A, b, KT_MAX_POINTS);
    const bool empty = np == 0 || A.M <= 0;
    if (GRAD) {
        const double gscale = 2.0 * 1.0 / 3.0;             // sk_combine's, scale 1
        const double* cross = A.gsum + (size_t)b * N * 3;
        const double* self = A.gsum + ((size_t)rows + b) * N * 3;
        float* g = A.grad + (size_t)b * A.grad_stride;
        const int real = (empty ? 0 : np) * 3;
        // sk_combine's double, times the weight, rounded once
        for (int e = tid; e < N * 3; e += KD_COMBINE_THREADS) g[e] = e < real ? (float)(A.weight * (gscale * (cross[e] - self[e]))) : 0.0f;
    }
    if (tid == 0) {
        const double sum = A.vals[b] - A.vals[rows + b] - A.self_q[cloud_goal::column_of_row(b, A.n_batch)];
        kg_store_value(A, b, A.weight * (1.0 * (sum / 3.0)));
    }
}
