// Symmetric squared Chamfer distance of two padded cloud batches and its gradient: the loss of a cloud whose rows
// are NOT the prediction's particles -- a re-sampled pile, a depth camera's cloud.
//   a(i) = argmin_j |p_i - q_j|^2   j < n_q (lowest j on a tie)        c(j) = argmin_i |q_j - p_i|^2   i < n_p (lowest i)
//   fwd = 1/(3 n_p) sum_i |p_i - q_a(i)|^2                            bwd = 1/(3 n_q) sum_j |q_j - p_c(j)|^2
//   d/dp_i = scale [ 2/(3 n_p) (p_i - q_a(i)) + 2/(3 n_q) sum_{j: c(j) = i} (p_i - q_j) ]       (the arg-mins are constants)
// One workgroup per (sample, rollout step), ONE path for every N, M <= 4096: the other cloud passes through LDS in tiles of
// KC_TILE points (a tile entry is read by all 64 lanes at once: a broadcast, no bank conflict), every thread keeps the running
// minimum of the points it owns (i = thread, thread + 256, ...).  Squared distances are fp32 sums of squares of fp32
// differences (-ffp-contract=off: no fused multiply-add); a strict `<` over ascending j is the tie rule.  The loss sums take
// each winner's squared fp32 differences in double, per thread in ascending i, then lanes, then waves: one fixed order.
// No atomics: c(.) stays in LDS and every i walks it in ascending j, adding (p_i - q_j) for its own entries -- the same bits
// from run to run, and for a sample alone or inside any batch (nothing depends on B, on the padding or on another sample).
#pragma once
#include "k_cloud_pair.h"

#define KC_THREADS 256
#define KC_TILE 1024            // points of the other cloud per LDS tile (float4 each: 16 KB)
#define KC_MAX_POINTS 4096      // check_bn's limit: c(.) of a whole cloud stays in LDS (16 KB)

struct KcArgs {
    const float* pred;          // p's rows (cp's strides)
    CloudPair cp;
    float scale;
    float* grad;                // TRAIN: [H][B][N][3], every row written (padded rows 0); else [B][N][3], nullable
    double* terms;              // TRAIN: [H][B], scale (fwd + bwd); else [B][2]: fwd, bwd
    int* nn_pq;                 // [B][N] a(.), nullable (padded rows -1); not TRAIN only
    int* nn_qp;                 // [B][M] c(.), nullable (padded rows -1); not TRAIN only
    float* zero; size_t n_zero; // TRAIN, nullable: filled with 0 (the gradient blob and kmb_step_bwd's counters, as kt_mse_grad does)
};

// the nearest of other[0 .. n_other) to (ox, oy, oz) for a thread with `live`; every thread of the workgroup calls it (the tiles
// are loaded together).  arg stays 0 where nothing compares below +inf (NaN coordinates): always a valid row.
__device__ __forceinline__ int kc_nearest(float ox, float oy, float oz, bool live, const float* __restrict__ other, int n_other,
                                          float4* tile) {
    float best = __builtin_inff();
    int arg = 0;
    for (int j0 = 0; j0 < n_other; j0 += KC_TILE) {
        const int cnt = min(KC_TILE, n_other - j0);
        __syncthreads();                                    // the previous tile (or whatever used the LDS before) is done with
        for (int e = threadIdx.x; e < cnt; e += KC_THREADS) {
            const float* o = other + (size_t)(j0 + e) * 3;
            tile[e] = make_float4(o[0], o[1], o[2], 0.0f);
        }
        __syncthreads();
        if (live)
            for (int j = 0; j < cnt; ++j) {
                const float4 o = tile[j];
                const float dx = ox - o.x, dy = oy - o.y, dz = oz - o.z;
                const float d = dx * dx + dy * dy + dz * dz;
                if (d < best) { best = d; arg = j0 + j; }
            }
    }
    return arg;
}

// sum over the workgroup in one fixed order (lanes by xor-shuffle, then the four waves); valid in thread 0
__device__ __forceinline__ double kc_block_sum(double v, double* s_w) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

template <bool TRAIN>
__global__ void __launch_bounds__(KC_THREADS) kc_chamfer(KcArgs A) {
    __shared__ float4 s_tile[KC_TILE];
    __shared__ int s_c[KC_MAX_POINTS];
    __shared__ double s_w[4];
    const int b = blockIdx.x, t = blockIdx.y, B = gridDim.x;
    const int N = A.cp.N, M = A.cp.M;
    if (TRAIN) train_zero_fill(A.zero, A.n_zero, KC_THREADS);
    const int np = A.cp.count_p(b, KC_MAX_POINTS), nq = A.cp.count_q(b, t, KC_MAX_POINTS);
    const float* p = A.cp.p_rows(A.pred, b, t);
    const float* q = A.cp.q_rows(b, t);
    const size_t slot = (size_t)t * B + b;
    float* g = A.grad != nullptr ? A.grad + slot * N * 3 : nullptr;
    int* nn_pq = (!TRAIN && A.nn_pq != nullptr) ? A.nn_pq + slot * N : nullptr;
    int* nn_qp = (!TRAIN && A.nn_qp != nullptr) ? A.nn_qp + slot * M : nullptr;
    const bool empty = np == 0 || nq == 0;
    const double inv_p = empty ? 0.0 : (double)A.scale / (3.0 * (double)np), inv_q = empty ? 0.0 : (double)A.scale / (3.0 * (double)nq);

    // c(j) of every target row, into LDS; the backward sum
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
            s_c[j] = c;
        }
    }
    if (nn_qp != nullptr)
        for (int j = threadIdx.x; j < M; j += KC_THREADS) nn_qp[j] = -1;       // (the real rows follow after the barrier below)
    __syncthreads();                                        // s_c is complete
    if (nn_qp != nullptr && !empty)
        for (int j = threadIdx.x; j < nq; j += KC_THREADS) nn_qp[j] = s_c[j];

    // a(i) of every predicted row, the forward sum, and the row's gradient: its own term, then its entries of c(.) in ascending j
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
            if (nn_pq != nullptr) nn_pq[i] = a;
            if (g != nullptr) {
                double sx = 0.0, sy = 0.0, sz = 0.0;       // fp32 differences added in double: a row may own hundreds of targets
                for (int j = 0; j < nq; ++j)
                    if (s_c[j] == i) {
                        sx += (double)(x - q[(size_t)j * 3]); sy += (double)(y - q[(size_t)j * 3 + 1]); sz += (double)(z - q[(size_t)j * 3 + 2]);
                    }
                g[(size_t)i * 3] = (float)(2.0 * (double)dx * inv_p + 2.0 * sx * inv_q);          // rounded once
                g[(size_t)i * 3 + 1] = (float)(2.0 * (double)dy * inv_p + 2.0 * sy * inv_q);
                g[(size_t)i * 3 + 2] = (float)(2.0 * (double)dz * inv_p + 2.0 * sz * inv_q);
            }
        }
    }
    // padding: gradient exactly 0, no neighbour
    const int first_pad = empty ? 0 : np;
    if (g != nullptr)
        for (int e = first_pad * 3 + threadIdx.x; e < N * 3; e += KC_THREADS) g[e] = 0.0f;
    if (nn_pq != nullptr)
        for (int i = first_pad + threadIdx.x; i < N; i += KC_THREADS) nn_pq[i] = -1;

    const double sum_f = kc_block_sum(acc_f, s_w);
    const double sum_b = kc_block_sum(acc_b, s_w);
    if (threadIdx.x == 0) {
        const double fwd = sum_f * inv_p, bwd = sum_b * inv_q;
        if (TRAIN) A.terms[slot] = fwd + bwd;       // one slot per (step, sample)
        else { A.terms[(size_t)b * 2] = fwd; A.terms[(size_t)b * 2 + 1] = bwd; }
    }
}
