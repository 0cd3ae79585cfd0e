// k_cloud_pair.h -- what the three cloud losses read (k_chamfer.h, k_match.h, k_chamfer_f64.h): a padded pair of cloud batches,
// p the prediction, q the target, and the prologue a training launch shares with kt_mse_grad (k_train.h).  The one definition of
// the fields, of where (sample, step) lies and of how a count is clamped.
#pragma once
#include "drp_common.h"

// p's rows are the kernel's own pointer (float, or the float64 tape's double): only its strides are here
struct CloudPair {
    size_t p_bstride, p_tstride;                    // p [.][.][N][3]: sample b, step t at p + b * p_bstride + t * p_tstride
    const float* q; size_t q_bstride, q_tstride;    // [.][.][M][3]
    const int* n_p;                                 // [B]
    const int* n_q; int nq_bstride, nq_tstride;     // n_q[b * nq_bstride + t * nq_tstride]
    int N, M;

    // b: the sample in p's batch; bb: the sample in q's and the counts' (the float64 kernel's chunk: bb = b_off + b; else bb = b)
    template <typename P>
    __device__ __forceinline__ const P* p_rows(const P* p, int b, int t) const { return p + (size_t)b * p_bstride + (size_t)t * p_tstride; }
    __device__ __forceinline__ const float* q_rows(int bb, int t) const { return q + (size_t)bb * q_bstride + (size_t)t * q_tstride; }
    // the real rows, held to the padding and to `cap` (what the kernel has room for): the entry points refuse counts outside
    // 1..N, 1..M and sizes beyond the cap
    __device__ __forceinline__ int count_p(int bb, int cap) const { return min(max(n_p[bb], 0), min(N, cap)); }
    __device__ __forceinline__ int count_q(int bb, int t, int cap) const {
        return min(max(n_q[(size_t)bb * nq_bstride + (size_t)t * nq_tstride], 0), min(M, cap));
    }
};

// with a backward pass to follow: the gradient blob (and kmb_step_bwd's barrier counters behind it) start at zero -- in the loss
// launch on grid (B, H) instead of a memset of their own (two fill launches); `threads`: the launch's workgroup size
__device__ __forceinline__ void train_zero_fill(float* zero /* nullable */, size_t n_zero, int threads) {
    const int b = blockIdx.x, t = blockIdx.y, B = gridDim.x;
    if (zero != nullptr)
        for (size_t e = ((size_t)t * B + b) * threads + threadIdx.x; e < n_zero; e += (size_t)gridDim.x * gridDim.y * threads) zero[e] = 0.0f;
}
