// k_train_f64.h -- the training loop body (train/train_gnn_dyn.py:167-203) in float64: the MSE of every rollout step with its
// seed of the reverse pass, the step's d loss / d input state, and the weight-gradient reductions.  A yardstick like
// k_prop_f64.h / k_gd_f64.h (whose forward and backward kernels it runs on), not an engine: every product and sum in double.
//
// Weight gradients: dW[o, i] = sum_rows G[row, o] X[row, i], db[o] = sum_rows G[row, o], G the ReLU-masked pre-activation
// gradient of the layer.  The 64-wide input blocks run on v_mfma_f64_16x16x4_f64 (fragment layout: top of k_prop_f64.h) with the
// ROWS as the k dimension: one wave owns a 16 x 16 tile of dW for one sample and walks that sample's rows in ascending k-steps
// of four.  The narrow inputs (the encoders' first layers, the density columns, the predictor's 3-row output layer, the biases)
// are one ascending fma / add chain per entry.  Masks and gathers (the receiver's and the sender's effect of a relation slot,
// through the lists) happen inside the loads; a slot past its receiver's count has G == 0 exactly and contributes exactly zero.
//
// ONE order per value: the contribution of (sample b, step t) to an entry in ascending row order (rows of relation slots:
// receiver-major, slot ascending), added to acc[b][W_TOTAL] in the order the reverse pass visits the steps (t descending; within
// a step the fixed launch order); kt64_total then takes acc[b] for b ascending in one chain per entry.  No atomics: every entry
// of acc[b] is written by one wave (or one thread) of one launch at a time, and launches are ordered by the stream.
#pragma once
#include "k_gd_f64.h"

// the chunk's start state: states[b0 + b, 0] widened.  n = bc * N * 3
__global__ __launch_bounds__(256) void kt64_init_state(const float* __restrict__ given, int b0, int N, int H, long n, double* __restrict__ s) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long b = i / (N * 3), k = i - b * (N * 3);
    s[i] = (double)given[((size_t)(b0 + b) * (H + 1)) * N * 3 + k];
}

// step t's impulse is data: states_delta[b0 + b, t] widened into the tape, and the fp32 values the graph build reads (the
// rounding of the double state, the impulse as given)
__global__ __launch_bounds__(256) void kt64_stage_step(const double* __restrict__ s_t, const float* __restrict__ sdelta_in, int b0, int N,
                                                       int H, int t, long n, double* __restrict__ sd_t, float* __restrict__ s32,
                                                       float* __restrict__ sd32) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long b = i / (N * 3), k = i - b * (N * 3);
    const float d = sdelta_in[((size_t)(b0 + b) * H + t) * N * 3 + k];
    sd_t[i] = (double)d;
    sd32[i] = d;
    s32[i] = (float)s_t[i];
}

// step t's impulse from the batch's pushes (drp_train_grad_f64_actions): kg_sdelta on the chunk's state with the padding mask --
// row n < nums[b0 + b] gets gen_s_delta(s_t[b], act[b0 + b, t])[n] in double, the padded rows zero -- and the fp32 roundings the
// graph build reads.  grid = samples of the chunk; act: the batch's pushes [B][H][4]
__global__ __launch_bounds__(256) void kt64_sdelta_actions(const double* __restrict__ s_t, const float* __restrict__ act,
                                                           const int* __restrict__ nums, int b0, int N, int H, int t, DrpCam cam,
                                                           double* __restrict__ sd_t, float* __restrict__ s32, float* __restrict__ sd32) {
    const int b = blockIdx.x;
    const float* ab = act + ((size_t)(b0 + b) * H + t) * 4;
    const double a[4] = {(double)ab[0], (double)ab[1], (double)ab[2], (double)ab[3]};
    const KgFrame<double> f = kg_frame<double>(cam, a);
    const int nb = min(max(nums[b0 + b], 0), N);
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const size_t o = ((size_t)b * N + n) * 3;
        const double p[3] = {s_t[o], s_t[o + 1], s_t[o + 2]};
        double out[3] = {0.0, 0.0, 0.0};
        if (n < nb) kg_push<double>(f, p, out);
#pragma unroll
        for (int k = 0; k < 3; ++k) { sd_t[o + k] = out[k]; s32[o + k] = (float)p[k]; sd32[o + k] = (float)out[k]; }
    }
}

// the loss term of (sample b, step t) = mse(s_pred[b, :n_b], s_nxt[b, :n_b]) / (H B) and its seed of the reverse pass,
// 2 (s_pred - s_nxt) / (3 n_b H B) on real rows, 0 on padded rows.  grid (bc, H); s_pred: the tape's states [H+1][bc*N,3]
// (slice t + 1), s_nxt: the caller's states [B][H+1][N][3] (fp32, widened exactly), loss [H][B], seed [H][bc*N,3].
__global__ __launch_bounds__(256) void kt64_mse(const double* __restrict__ states, const float* __restrict__ given,
                                                const int* __restrict__ nums, int b0, int bc, int B, int N, int H,
                                                double* __restrict__ loss, double* __restrict__ seed) {
    __shared__ double part[256];
    const int b = blockIdx.x, t = blockIdx.y;
    const int nb = nums[b0 + b];
    const size_t pn = (size_t)bc * N;
    const double* p = states + (size_t)(t + 1) * pn * 3 + (size_t)b * N * 3;
    const float* q = given + ((size_t)(b0 + b) * (H + 1) + (t + 1)) * N * 3;
    double* g = seed + (size_t)t * pn * 3 + (size_t)b * N * 3;
    const double denom = 3.0 * (double)nb * (double)H * (double)B;
    double acc = 0.0;
    for (int i = threadIdx.x; i < N * 3; i += 256) {        // a thread's elements ascending
        double gv = 0.0;
        if (i < nb * 3) {
            const double d = p[i] - (double)q[i];
            gv = 2.0 * d / denom;
            acc += d * d;
        }
        g[i] = gv;
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < 256; ++k) s += part[k];         // the threads' partial sums ascending
        loss[(size_t)t * B + b0 + b] = s / denom;
    }
}

// the seed of the reverse pass as the CALLER gives it (drp_train_grad_f64_seeded), in kt64_mse's slot and on its grid (bc, H): the
// batch's seed [B][H][N][3] (doubles, the caller's layout) at the chunk's sample offset b0 to seed_out [H][bc*N,3], real rows bit
// for bit, +0.0 on rows n >= nums[b0 + b] whatever lies there.  No loss term.  Where N * 3 is even both slices start on 16 bytes
// and the copy is double2s.
__global__ __launch_bounds__(256) void k64_seed_given(const double* __restrict__ seed_in, const int* __restrict__ nums, int b0, int bc,
                                                      int N, int H, double* __restrict__ seed_out) {
    const int b = blockIdx.x, t = blockIdx.y;
    const int n3 = N * 3, real = min(max(nums[b0 + b], 0), N) * 3;
    const double* s = seed_in + ((size_t)(b0 + b) * H + t) * n3;
    double* g = seed_out + ((size_t)t * bc + b) * n3;
    if ((n3 & 1) == 0) {
        const double2* s2 = reinterpret_cast<const double2*>(s);
        double2* g2 = reinterpret_cast<double2*>(g);
        for (int i = threadIdx.x; i < n3 / 2; i += 256) {
            double2 v = s2[i];
            v.x = i * 2 + 0 < real ? v.x : 0.0;
            v.y = i * 2 + 1 < real ? v.y : 0.0;
            g2[i] = v;
        }
    } else {
        for (int i = threadIdx.x; i < n3; i += 256) g[i] = i < real ? s[i] : 0.0;
    }
}

// d loss / d s_pred_{t-1} += the step's share: the + s_cur of the output, then the relation encoder's (kg_state_share).
// g_prev holds the MSE's seed of step t - 1 when this runs.
__global__ __launch_bounds__(256) void kt64_state_bwd(const double* __restrict__ g_out, const double* __restrict__ g_diff,
                                                      const uint8_t* __restrict__ cnt, const int* __restrict__ rev_off,
                                                      const int* __restrict__ rev, int N, int rows, double* __restrict__ g_prev) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const long b = i / N;
    const int n = (int)(i - b * N);
#pragma unroll
    for (int k = 0; k < 3; ++k)
        g_prev[i * 3 + k] = kg_state_share(g_prev[i * 3 + k] + g_out[i * 3 + k], g_diff, cnt, rev_off, rev, N, (size_t)b, n, k);
}

// the push's share on top of kt64_state_bwd's sum (drp_train_grad_f64_actions; kg_sdelta_bwd's position part with the padding
// mask): g_prev[b, n] += J_pos^T g_sd[b, n] on rows n < nums[b0 + b]; the hard mask a constant of the derivative, the soft mask
// and both projections differentiated (directions 4..6 of KgDual); padded rows receive nothing
__global__ __launch_bounds__(256) void kt64_push_bwd(const double* __restrict__ s_t, const float* __restrict__ act,
                                                     const int* __restrict__ nums, int b0, int N, int H, int t, DrpCam cam,
                                                     const double* __restrict__ g_sd, double* __restrict__ g_prev) {
    const int b = blockIdx.x;
    const float* ab = act + ((size_t)(b0 + b) * H + t) * 4;
    KgDual a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = KgDual((double)ab[k]);
    const KgFrame<KgDual> f = kg_frame<KgDual>(cam, a);
    const int nb = min(max(nums[b0 + b], 0), N);
    for (int n = threadIdx.x; n < nb; n += blockDim.x) {
        const size_t i = (size_t)b * N + n;
        KgDual p[3], out[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { p[k] = KgDual(s_t[i * 3 + k]); p[k].d[4 + k] = 1.0; }
        if (!kg_push<KgDual>(f, p, out)) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            g_prev[i * 3 + k] += g_sd[i * 3] * out[0].d[4 + k] + g_sd[i * 3 + 1] * out[1].d[4 + k] + g_sd[i * 3 + 2] * out[2].d[4 + k];
    }
}

// ---- the operands of a 64-wide layer's weight gradient ------------------------------------------------------------------
// G[row, o] = g[(row / g_div) * 64 + o], under the mask m[row * 64 + o] > 0 when m is given (the layer's own output: its ReLU).
// g_div = DRP_K: rows are relation slots and g is per receiver.  X[row, i] by x_mode: the row itself, the slot's receiver, or
// the slot's sender through the lists (a slot past the count reads its receiver, as the forward pass; its G is zero).
enum { KT64_X_ROW = 0, KT64_X_RECV = 1, KT64_X_SEND = 2 };
struct Kt64Job {
    const double* g; const double* m; int g_div;
    const double* x; int x_mode;
    const int16_t* idx; const uint8_t* cnt;
    int N;                      // particles per sample (the sender's sample base)
    int R;                      // rows per sample: N, or N * DRP_K
    int w_off, ld;              // dW[o, i] at acc[w_off + o * ld + i]
    int b_off, d_off;           // kt64_wgrad_bias: the bias at acc[b_off + o]; the density column at acc[d_off + o * ld] (-1: none)
};
__device__ __forceinline__ double kt64_g(const Kt64Job& j, size_t row, int o) {
    const double v = j.g[(row / (size_t)j.g_div) * 64 + o];
    return (j.m == nullptr || j.m[row * 64 + o] > 0.0) ? v : 0.0;
}
__device__ __forceinline__ size_t kt64_xrow(const Kt64Job& j, size_t row) {
    if (j.x_mode == KT64_X_ROW) return row;
    const size_t p = row / DRP_K;
    if (j.x_mode == KT64_X_RECV) return p;
    const int k = (int)(row - p * DRP_K);
    return k < (int)j.cnt[p] ? (p / (size_t)j.N) * (size_t)j.N + (size_t)j.idx[row] : p;
}

// dW of one 64 x 64 block for every sample of the chunk: grid (4 strips of 16 outputs, bc), 4 waves = the 4 tiles of 16 inputs.
// A[i = output][k = row], B[k = row][j = input]; C: col = input, row = output.
__global__ __launch_bounds__(256) void kt64_wgrad64(Kt64Job j, double* __restrict__ acc_all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int o0 = blockIdx.x * 16, i0 = wave * 16;
    const size_t base = (size_t)blockIdx.y * (size_t)j.R;
    kf_d4 acc = kf_d4{0.0, 0.0, 0.0, 0.0};
    for (int r0 = 0; r0 < j.R; r0 += 4) {
        const int lr = r0 + q;
        const bool ok = lr < j.R;
        const size_t row = base + (size_t)(ok ? lr : j.R - 1);
        double a = kt64_g(j, row, o0 + r);
        double b = j.x[kt64_xrow(j, row) * 64 + i0 + r];
        if (!ok) { a = 0.0; b = 0.0; }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    double* dst = acc_all + (size_t)blockIdx.y * W_TOTAL + j.w_off;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int o = o0 + q + 4 * g;
        dst[o * j.ld + i0 + r] += acc[g];
    }
}

// bias (threads 0..63) and density column (threads 64..127, dens / 5000 per sample) of the same layer: grid bc
__global__ __launch_bounds__(128) void kt64_wgrad_bias(Kt64Job j, const float* __restrict__ dens, double* __restrict__ acc_all) {
    const int o = threadIdx.x & 63, which = threadIdx.x >> 6;
    if (which == 1 && j.d_off < 0) return;
    const size_t base = (size_t)blockIdx.x * (size_t)j.R;
    const double d = (double)dens[blockIdx.x] / 5000.0;
    double a = 0.0;
    if (which == 0)
        for (int lr = 0; lr < j.R; ++lr) a += kt64_g(j, base + lr, o);
    else
        for (int lr = 0; lr < j.R; ++lr) a = fma(kt64_g(j, base + lr, o), d, a);
    double* dst = acc_all + (size_t)blockIdx.x * W_TOTAL;
    if (which == 0) dst[j.b_off + o] += a;
    else dst[j.d_off + o * j.ld] += a;
}

// a narrow layer: G [rows, gw], X [rows, xw] plain arrays -> dW[o, i] at acc[w_off + o * xw + i] (i < xw), db[o] at
// acc[b_off + o]; one thread per entry, rows ascending.  grid (ceil(gw * (xw + 1) / 256), bc).
__global__ __launch_bounds__(256) void kt64_wgrad_narrow(const double* __restrict__ G, int gw, const double* __restrict__ X, int xw,
                                                         int R, int w_off, int b_off, double* __restrict__ acc_all) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= gw * (xw + 1)) return;
    const int o = e / (xw + 1), i = e - o * (xw + 1);
    const size_t base = (size_t)blockIdx.y * (size_t)R;
    double a = 0.0;
    if (i < xw)
        for (int lr = 0; lr < R; ++lr) a = fma(G[(base + lr) * gw + o], X[(base + lr) * xw + i], a);
    else
        for (int lr = 0; lr < R; ++lr) a += G[(base + lr) * gw + o];
    double* dst = acc_all + (size_t)blockIdx.y * W_TOTAL;
    if (i < xw) dst[w_off + o * xw + i] += a;
    else dst[b_off + o] += a;
}

// total[e] += acc[b][e], b ascending over the chunk's samples: with the chunks in order, one chain over the whole batch
__global__ __launch_bounds__(256) void kt64_total(const double* __restrict__ acc_all, int bc, double* __restrict__ total) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= (int)W_TOTAL) return;
    double v = total[e];
    for (int b = 0; b < bc; ++b) v += acc_all[(size_t)b * W_TOTAL + e];
    total[e] = v;
}
