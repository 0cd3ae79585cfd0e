// k_optim.h -- the trainer's optimiser seam (capi_optim.h: drp_train_accumulate, drp_train_apply): a float64 accumulator of
// gradient blobs, its scaled 2-norm in a fixed order, torch's clip_grad_norm_ factor, and one Adam step on the scaled sum.
// Small, bandwidth-trivial kernels over W_TOTAL = 38 403 = 150 * 256 + 3 elements: plain HIP, no atomics.
#pragma once

#define KO_THREADS 256
#define KO_BLOCKS(n) (((n) + KO_THREADS - 1) / KO_THREADS)
#define KO_CLIP_EPS 1e-6        // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6)

// what ko_norm_final leaves for ko_adam_scaled on the device, and once more in pinned host memory for the caller
struct KoStep {
    double norm;        // || s0 acc ||_2
    double clip;        // min(1, max_norm / (norm + 1e-6))
    double s;           // s0 * clip: what the accumulator is multiplied by
    unsigned skip;      // 1: the norm is not finite, nothing moves
    unsigned pad;
};

// acc[i] += weight * (double)grad[i].  An integer weight up to 2^29 times an fp32 value is exact in double (24 + 29 = 53
// bits), so the sum is rounded once per addition, in call order
__global__ void __launch_bounds__(KO_THREADS)
ko_accumulate(double* __restrict__ acc, const float* __restrict__ grad, int n, double weight) {
    const int i = blockIdx.x * KO_THREADS + threadIdx.x;
    if (i >= n) return;
    acc[i] += weight * (double)grad[i];
}

// the block's tree sum of `x` in a fixed order (LDS, halving strides); the result is valid in thread 0
__device__ __forceinline__ double ko_block_sum(double x, double* sh) {
    const int t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
    for (int w = KO_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) sh[t] += sh[t + w];
        __syncthreads();
    }
    return sh[0];
}

// stage 1: part[block] = sum over the block's elements of (s0 acc[i])^2; elements past n count +0.0
__global__ void __launch_bounds__(KO_THREADS)
ko_norm_partial(const double* __restrict__ acc, int n, double s0, double* __restrict__ part) {
    __shared__ double sh[KO_THREADS];
    const int i = blockIdx.x * KO_THREADS + threadIdx.x;
    const double x = i < n ? s0 * acc[i] : 0.0;
    const double sum = ko_block_sum(x * x, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// stage 2, one block: the partials in thread order (thread t: part[t], part[t + 256], ...), the same tree, then the norm, the
// clip factor and the scale -- on the device for ko_adam_scaled, and in pinned host memory for the caller
__global__ void __launch_bounds__(KO_THREADS)
ko_norm_final(const double* __restrict__ part, int n_part, double s0, double max_norm, KoStep* __restrict__ dev,
              KoStep* __restrict__ host) {
    __shared__ double sh[KO_THREADS];
    double x = 0.0;
    for (int p = threadIdx.x; p < n_part; p += KO_THREADS) x += part[p];
    const double sum = ko_block_sum(x, sh);
    if (threadIdx.x != 0) return;
    KoStep k;
    k.norm = sqrt(sum);
    k.clip = fmin(1.0, max_norm / (k.norm + KO_CLIP_EPS));
    k.s = s0 * k.clip;
    k.skip = isfinite(k.norm) ? 0u : 1u;
    k.pad = 0u;
    *dev = k;
    *host = k;
}

// g = (float)(acc[i] * s), the accumulator cleared, then k_adam's step on g (adam_update; lo / hi: k_adam's box, -inf / +inf
// for the weights).  A norm that was not finite (k->skip): the accumulator is still cleared and g still stored, nothing else moves
__global__ void __launch_bounds__(KO_THREADS)
ko_adam_scaled(float* __restrict__ w, double* __restrict__ acc, float* __restrict__ m, float* __restrict__ v, int n,
               float step_size, float bc2_sqrt, float b1, float lo, float hi, const KoStep* __restrict__ k,
               float* __restrict__ g32, float* __restrict__ w_copy /* nullable: pinned host memory, the updated values once more */) {
    const int i = blockIdx.x * KO_THREADS + threadIdx.x;
    if (i >= n) return;
    const float g = (float)(acc[i] * k->s);
    acc[i] = 0.0;
    g32[i] = g;
    if (k->skip != 0u) return;
    float mi = m[i], vi = v[i];
    const float a = adam_update(w[i], g, mi, vi, step_size, bc2_sqrt, b1, lo, hi);
    m[i] = mi;
    v[i] = vi;
    w[i] = a;
    if (w_copy != nullptr) w_copy[i] = a;
}
