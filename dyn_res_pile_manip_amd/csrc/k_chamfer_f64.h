// k_chamfer_f64.h -- k_chamfer.h's symmetric squared Chamfer distance and its gradient in float64: the yardstick of
// the untracked loss, stand-alone (drp_cloud_chamfer_f64) and as the seed of the float64 reverse pass (drp_train_grad_f64_untracked,
// launched where kt64_mse is).  A yardstick like k_train_f64.h, not an engine.
//   a(i) = argmin_j |p_i - q_j|^2   j < n_q (lowest j on a tie)        c(j) = argmin_i |q_j - p_i|^2   i < n_p (lowest i)
//   fwd = 1/(3 n_p) sum_i |p_i - q_a(i)|^2                            bwd = 1/(3 n_q) sum_j |q_j - p_c(j)|^2
//   d/dp_i = scale [ 2/(3 n_p) (p_i - q_a(i)) + 2/(3 n_q) sum_{j: c(j) = i} (p_i - q_j) ]       (the arg-mins are constants)
// Arithmetic: p is double (TRAIN: the tape's predicted state; else the caller's floats widened exactly), q the caller's floats
// widened where they are loaded; a squared distance is dx*dx + dy*dy + dz*dz in double in that order (-ffp-contract=off: no fused
// multiply-add); a strict `<` over ascending indices is the tie rule.  The arg-mins are taken HERE, in double on the double
// prediction: the fp32 kernel's are no input.
// Margins (no fp32 counterpart): beside its best distance every row keeps the best distance over all OTHER indices; the row's
// margin is second - best -- a duplicate of the winner gives 0 exactly, an other cloud of one row +inf -- and the workgroup
// reduces the margins of its real rows to one minimum per direction (a minimum is order-free).  A probe reads it to tell an
// arithmetic finding from a partner that a near-tie flipped between fp32 and float64.
// Structure: kc_chamfer's.  One workgroup of 256 threads per (sample, step), ONE path for every N, M <= 4096; the other cloud
// passes through LDS in tiles of KC64_TILE points (four doubles each, 32 KB; a tile entry is read by all 64 lanes at once: a
// broadcast), c(.) stays in LDS (16 KB) and every row walks it in ascending j for its gather sum.  Loss sums per thread in
// ascending row, then lanes by xor-shuffle, then the four waves in order.  No atomics: the same bits from run to run, for a
// sample alone or in any batch, and in any chunk of a batch.
#pragma once
#include "k_cloud_pair.h"

#define KC64_THREADS 256
#define KC64_TILE 1024          // points of the other cloud per LDS tile (four doubles each: 32 KB)
#define KC64_MAX_POINTS 4096    // check_bn's limit: c(.) of a whole cloud stays in LDS (16 KB)

struct Kc64Pt { double x, y, z, w; };

struct Kc64Args {
    const double* p64; const float* p32;                // p's rows (cp's strides): TRAIN: p64, the chunk's; else p32
    CloudPair cp;               // q and the counts are the batch's: sample b_off + b
    int b_off;                  // TRAIN: the chunk's first sample (p and grad are the chunk's, everything else the batch's)
    int B;                      // TRAIN: samples of the batch (the stride of terms and margin)
    double scale;
    double* grad;               // TRAIN: [H][gridDim.x][N][3], every row written (padded rows +0.0); else [B][N][3], nullable
    double* terms;              // TRAIN: [H][B], scale (fwd + bwd); else [B][2]: fwd, bwd
    double* margin;             // TRAIN: [H][B], the smaller of both directions; else [B][2]: p -> q, q -> p; nullable
    int* nn_pq;                 // [B][N] a(.), nullable (padded rows -1); not TRAIN only
    int* nn_qp;                 // [B][M] c(.), nullable (padded rows -1); not TRAIN only
};

// the nearest of other[0 .. n_other) to (ox, oy, oz) for a thread with `live`, with the best distance and the best over all
// other indices; every thread of the workgroup calls it (the tiles are loaded together).  arg stays 0 where nothing compares
// below +inf (NaN coordinates): always a valid row.
template <typename T>
__device__ __forceinline__ int kc64_nearest(double ox, double oy, double oz, bool live, const T* __restrict__ other, int n_other,
                                            Kc64Pt* tile, double* best_out, double* second_out) {
    double best = __builtin_inf(), second = __builtin_inf();
    int arg = 0;
    for (int j0 = 0; j0 < n_other; j0 += KC64_TILE) {
        const int cnt = min(KC64_TILE, n_other - j0);
        __syncthreads();                                    // the previous tile (or whatever used the LDS before) is done with
        for (int e = threadIdx.x; e < cnt; e += KC64_THREADS) {
            const T* o = other + (size_t)(j0 + e) * 3;
            tile[e] = Kc64Pt{(double)o[0], (double)o[1], (double)o[2], 0.0};
        }
        __syncthreads();
        if (live)
            for (int j = 0; j < cnt; ++j) {
                const Kc64Pt o = tile[j];
                const double dx = ox - o.x, dy = oy - o.y, dz = oz - o.z;
                const double d = dx * dx + dy * dy + dz * dz;
                if (d < best) { second = best; best = d; arg = j0 + j; }
                else if (d < second) second = d;
            }
    }
    *best_out = best;
    *second_out = second;
    return arg;
}

// sum over the workgroup in one fixed order (lanes by xor-shuffle, then the four waves); valid in thread 0
__device__ __forceinline__ double kc64_block_sum(double v, double* s_w) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
// the minimum over the workgroup (order-free); valid in thread 0
__device__ __forceinline__ double kc64_block_min(double v, double* s_w) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmin(fmin(s_w[0], s_w[1]), fmin(s_w[2], s_w[3]));
}

template <bool TRAIN, typename P>
__device__ __forceinline__ void kc64_body(const Kc64Args& A, const P* __restrict__ p_all, Kc64Pt* s_tile, int* s_c, double* s_w) {
    const int b = blockIdx.x, t = blockIdx.y, nb = gridDim.x;
    const int N = A.cp.N, M = A.cp.M;
    const int bb = A.b_off + b;                             // the sample in the batch's arrays
    const int np = A.cp.count_p(bb, KC64_MAX_POINTS), nq = A.cp.count_q(bb, t, KC64_MAX_POINTS);
    const P* p = A.cp.p_rows(p_all, b, t);
    const float* q = A.cp.q_rows(bb, t);
    const size_t slot = (size_t)t * nb + b;                 // of the launch's own outputs
    double* g = A.grad != nullptr ? A.grad + slot * N * 3 : nullptr;
    int* nn_pq = (!TRAIN && A.nn_pq != nullptr) ? A.nn_pq + slot * N : nullptr;
    int* nn_qp = (!TRAIN && A.nn_qp != nullptr) ? A.nn_qp + slot * M : nullptr;
    const bool empty = np == 0 || nq == 0;
    const double inv_p = empty ? 0.0 : A.scale / (3.0 * (double)np), inv_q = empty ? 0.0 : A.scale / (3.0 * (double)nq);

    // c(j) of every target row, into LDS; the backward sum and the margins of q -> p
    double acc_b = 0.0, mar_b = __builtin_inf();
    for (int j0 = 0; j0 < (empty ? 0 : nq); j0 += KC64_THREADS) {
        const int j = j0 + threadIdx.x;
        const bool live = j < nq;
        double x = 0.0, y = 0.0, z = 0.0;
        if (live) { x = (double)q[(size_t)j * 3]; y = (double)q[(size_t)j * 3 + 1]; z = (double)q[(size_t)j * 3 + 2]; }
        double best, second;
        const int c = kc64_nearest<P>(x, y, z, live, p, np, s_tile, &best, &second);
        if (live) {
            acc_b += best;
            mar_b = fmin(mar_b, second - best);
            s_c[j] = c;
        }
    }
    if (nn_qp != nullptr)
        for (int j = threadIdx.x; j < M; j += KC64_THREADS) nn_qp[j] = -1;     // (the real rows follow after the barrier below)
    __syncthreads();                                        // s_c is complete
    if (nn_qp != nullptr && !empty)
        for (int j = threadIdx.x; j < nq; j += KC64_THREADS) nn_qp[j] = s_c[j];

    // a(i) of every predicted row, the forward sum, the margins of p -> q, and the row's gradient: its own term, then its
    // entries of c(.) in ascending j
    double acc_f = 0.0, mar_f = __builtin_inf();
    for (int i0 = 0; i0 < (empty ? 0 : np); i0 += KC64_THREADS) {
        const int i = i0 + threadIdx.x;
        const bool live = i < np;
        double x = 0.0, y = 0.0, z = 0.0;
        if (live) { x = (double)p[(size_t)i * 3]; y = (double)p[(size_t)i * 3 + 1]; z = (double)p[(size_t)i * 3 + 2]; }
        double best, second;
        const int a = kc64_nearest<float>(x, y, z, live, q, nq, s_tile, &best, &second);
        if (live) {
            acc_f += best;
            mar_f = fmin(mar_f, second - best);
            if (nn_pq != nullptr) nn_pq[i] = a;
            if (g != nullptr) {
                const double dx = x - (double)q[(size_t)a * 3], dy = y - (double)q[(size_t)a * 3 + 1], dz = z - (double)q[(size_t)a * 3 + 2];
                double sx = 0.0, sy = 0.0, sz = 0.0;
                for (int j = 0; j < nq; ++j)
                    if (s_c[j] == i) {
                        sx += x - (double)q[(size_t)j * 3]; sy += y - (double)q[(size_t)j * 3 + 1]; sz += z - (double)q[(size_t)j * 3 + 2];
                    }
                g[(size_t)i * 3] = 2.0 * dx * inv_p + 2.0 * sx * inv_q;
                g[(size_t)i * 3 + 1] = 2.0 * dy * inv_p + 2.0 * sy * inv_q;
                g[(size_t)i * 3 + 2] = 2.0 * dz * inv_p + 2.0 * sz * inv_q;
            }
        }
    }
    // padding: gradient exactly +0.0, no neighbour
    const int first_pad = empty ? 0 : np;
    if (g != nullptr)
        for (int e = first_pad * 3 + threadIdx.x; e < N * 3; e += KC64_THREADS) g[e] = 0.0;
    if (nn_pq != nullptr)
        for (int i = first_pad + threadIdx.x; i < N; i += KC64_THREADS) nn_pq[i] = -1;

    const double sum_f = kc64_block_sum(acc_f, s_w);
    const double sum_b = kc64_block_sum(acc_b, s_w);
    const double min_f = kc64_block_min(mar_f, s_w);
    const double min_b = kc64_block_min(mar_b, s_w);
    if (threadIdx.x == 0) {
        const double fwd = sum_f * inv_p, bwd = sum_b * inv_q;
        if (TRAIN) {                                        // one slot per (step, sample of the batch)
            const size_t o = (size_t)t * A.B + bb;
            A.terms[o] = fwd + bwd;
            if (A.margin != nullptr) A.margin[o] = fmin(min_f, min_b);
        } else {
            A.terms[(size_t)b * 2] = fwd; A.terms[(size_t)b * 2 + 1] = bwd;
            if (A.margin != nullptr) { A.margin[(size_t)b * 2] = min_f; A.margin[(size_t)b * 2 + 1] = min_b; }
        }
    }
}

// grid (samples, steps): TRAIN (bc, H) on a chunk of the float64 tape; else (B, 1)
template <bool TRAIN>
__global__ void __launch_bounds__(KC64_THREADS) kc64_chamfer(Kc64Args A) {
    __shared__ Kc64Pt s_tile[KC64_TILE];
    __shared__ int s_c[KC64_MAX_POINTS];
    __shared__ double s_w[4];
    if (TRAIN) kc64_body<TRAIN, double>(A, A.p64, s_tile, s_c, s_w);
    else kc64_body<TRAIN, float>(A, A.p32, s_tile, s_c, s_w);
}
