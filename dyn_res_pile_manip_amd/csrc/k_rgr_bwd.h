// The resolution regressor's training step (train/train_res_rgr.py:150-183): loss, backward pass and Adam, on the forward's
// layouts (k_rgr.h: activations NHWC, conv weights [Cout][kh][kw][Cin], FC1's columns in NHWC order).
// Numerics: fp32 (fp32-input MFMA for the convolutions, fmaf chains elsewhere), loss terms in float64.  Every value has ONE
// reduction order, fixed by the layer and the batch: the k order inside an MFMA tile, a fixed split count per layer whose
// partials are summed slab 0 first, sample-ascending chains for K = B.  No float atomics: two runs of the same step
// sequence give bit-identical weights.
// LeakyReLU(0.2)'s derivative is read off the stored post-activation: it has the sign of the pre-activation.
#pragma once
#include "k_rgr.h"
#include "k_backward.h"

__device__ __forceinline__ float rgr_dleaky(float g, float act) { return act > 0.0f ? g : g * RGR_SLOPE; }
__device__ __forceinline__ float rgr_sign(float w) { return w > 0.0f ? 1.0f : (w < 0.0f ? -1.0f : 0.0f); }  // norm(1)'s backward

// the sum of a workgroup's 256 doubles, one fixed tree; the result is valid in thread 0
__device__ __forceinline__ double rgr_block_sum(double s, double* red) {
    const int tid = threadIdx.x;
    red[tid] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    return red[0];
}

// part[block] = sum |w| over the elements this workgroup strides over (a fixed grid: a fixed order)
__global__ void __launch_bounds__(256) k_rgr_l1(const float* __restrict__ w, size_t n, double* __restrict__ part) {
    __shared__ double red[256];
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) s += fabs((double)w[i]);
    s = rgr_block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ---- loss and head (one workgroup) -----------------------------------------------------------------------------------
// regressor (n_out 1): loss_part[b] = conf[b] (out[b] - y[b])^2, dOut[b] = 2 conf[b] (out[b] - y[b]) / B   (MSE * conf, .mean())
// classifier (n_out 6): loss_part[b] = logsumexp(out[b]) - out[b][label[b]], dOut[b] = (softmax(out[b]) - onehot) / B
// then (backward): dz4[b][k] = leaky'(f4[b][k]) sum_o dOut[b][o] Wh[o][k];  gW[o][k] = sum_b dOut[b][o] f4[b][k] + coef sign(Wh);
// gb[o] = sum_b dOut[b][o]
__global__ void __launch_bounds__(256)
k_rgr_loss_head(const float* __restrict__ out, int B, int n_out, const float* __restrict__ y, const float* __restrict__ conf,
                const int* __restrict__ label, const float* __restrict__ Wh, const float* __restrict__ f4,
                double* __restrict__ loss_part, int backward, float coef, float* __restrict__ gW, float* __restrict__ gb,
                float* __restrict__ dz4) {
    __shared__ float s_d[RGR_BMAX * 6];
    const int tid = threadIdx.x;
    if (tid < B) {
        const int b = tid;
        if (n_out == 1) {
            const double d = (double)out[b] - (double)y[b];
            loss_part[b] = (double)conf[b] * d * d;
            s_d[b] = (float)(2.0 * (double)conf[b] * d / (double)B);
        } else {
            const float* l = out + b * 6;
            double mx = l[0];
            for (int o = 1; o < 6; ++o) mx = fmax(mx, (double)l[o]);
            double se = 0.0;
            for (int o = 0; o < 6; ++o) se += exp((double)l[o] - mx);
            const double lse = mx + log(se);
            const int t = label[b];
            loss_part[b] = lse - (double)l[t];
            for (int o = 0; o < 6; ++o) s_d[b * 6 + o] = (float)((exp((double)l[o] - lse) - (o == t ? 1.0 : 0.0)) / (double)B);
        }
    }
    if (!backward) return;                  // (uniform over the workgroup)
    __syncthreads();
    for (int i = tid; i < B * 64; i += 256) {
        const int b = i >> 6, k = i & 63;
        float a = 0.0f;
        for (int o = 0; o < n_out; ++o) a = fmaf(s_d[b * n_out + o], Wh[o * 64 + k], a);
        dz4[i] = rgr_dleaky(a, f4[i]);
    }
    for (int i = tid; i < n_out * 64; i += 256) {
        const int o = i >> 6, k = i & 63;
        float a = 0.0f;
        for (int b = 0; b < B; ++b) a = fmaf(s_d[b * n_out + o], f4[b * 64 + k], a);
        gW[i] = a + coef * rgr_sign(Wh[i]);
    }
    if (tid < n_out) {
        float a = 0.0f;
        for (int b = 0; b < B; ++b) a += s_d[b * n_out + tid];
        gb[tid] = a;
    }
}

// ---- column sums (bias gradients) -------------------------------------------------------------------------------------
// part[c][n] = sum of dz[r][n] over rows r of chunk c (RGR_CS_CHUNK rows, ascending); then g[n] = sum_c part[c][n] (ascending)
#define RGR_CS_CHUNK 1024
__global__ void __launch_bounds__(256)
k_rgr_colsum_part(const float* __restrict__ dz, int rows, int N, float* __restrict__ part) {
    const int n = blockIdx.y * 256 + threadIdx.x;
    if (n >= N) return;
    const int c = blockIdx.x, r1 = min(rows, (c + 1) * RGR_CS_CHUNK);
    float a = 0.0f;
#pragma unroll 8
    for (int r = c * RGR_CS_CHUNK; r < r1; ++r) a += dz[(size_t)r * N + n];
    part[(size_t)c * N + n] = a;
}
__global__ void __launch_bounds__(256)
k_rgr_colsum_fin(const float* __restrict__ part, int nchunk, int N, float* __restrict__ g) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float a = 0.0f;
    for (int c = 0; c < nchunk; ++c) a += part[(size_t)c * N + n];
    g[n] = a;
}

// ---- fully connected layers ------------------------------------------------------------------------------------------
// dX, transposed GEMV: part[s][b][k] = sum over rows o of slice s (R rows, ascending) of dz[b][o] W[o][k].  Workgroup: 1024
// columns (4 per lane), samples g*16 .. +16 (grid z), slice s (grid y); the slice's dz block sits in LDS.
__global__ void __launch_bounds__(256)
k_rgr_fct(const float* __restrict__ W, const float* __restrict__ dz, int B, int N, int K, int R, float* __restrict__ part) {
    extern __shared__ float zs[];                       // [R][16]
    const int tid = threadIdx.x, s = blockIdx.y, g = blockIdx.z;
    for (int i = tid; i < R * 16; i += 256) {
        const int r = i >> 4, b = g * 16 + (i & 15);
        zs[i] = b < B ? dz[(size_t)b * N + (size_t)s * R + r] : 0.0f;
    }
    __syncthreads();
    const int k = (blockIdx.x * 256 + tid) * 4;
    if (k >= K) return;
    float acc[16][4];
#pragma unroll
    for (int b = 0; b < 16; ++b) acc[b][0] = acc[b][1] = acc[b][2] = acc[b][3] = 0.0f;
    const float* wp = W + (size_t)s * R * K + k;
#pragma unroll 4
    for (int r = 0; r < R; ++r) {
        const rgr_f32x4 w = __builtin_nontemporal_load(reinterpret_cast<const rgr_f32x4*>(wp + (size_t)r * K));
        const float4* z4 = reinterpret_cast<const float4*>(zs + r * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 z = z4[q];
            const float zz[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float* a = acc[4 * q + e];
                a[0] = fmaf(zz[e], w.x, a[0]);
                a[1] = fmaf(zz[e], w.y, a[1]);
                a[2] = fmaf(zz[e], w.z, a[2]);
                a[3] = fmaf(zz[e], w.w, a[3]);
            }
        }
    }
#pragma unroll
    for (int bb = 0; bb < 16; ++bb) {
        const int b = g * 16 + bb;
        if (b < B)
            *reinterpret_cast<float4*>(part + ((size_t)s * B + b) * K + k) = make_float4(acc[bb][0], acc[bb][1], acc[bb][2], acc[bb][3]);
    }
}

// out[i] = leaky'(act[i]) (((part[0][i] + part[1][i]) + ...) + part[S-1][i]);  n % 4 == 0
__global__ void __launch_bounds__(256)
k_rgr_dreduce(const float* __restrict__ part, int S, size_t n, const float* __restrict__ act, float* __restrict__ out) {
    const size_t i4 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 >= n) return;
    float4 v = *reinterpret_cast<const float4*>(part + i4);
    for (int s = 1; s < S; ++s) {
        const float4 u = *reinterpret_cast<const float4*>(part + (size_t)s * n + i4);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    const float4 a = *reinterpret_cast<const float4*>(act + i4);
    *reinterpret_cast<float4*>(out + i4) =
        make_float4(rgr_dleaky(v.x, a.x), rgr_dleaky(v.y, a.y), rgr_dleaky(v.z, a.z), rgr_dleaky(v.w, a.w));
}

// dW[o][k] = (sum over b = 0..B-1 of dz[b][o] x[b][k], one fmaf chain) + coef sign(W[o][k]).  Workgroup: 64 rows x 256
// columns (wave w: rows r0 + 16 w .. +16; lane: 4 columns), samples staged through LDS 16 at a time.  ADAM: the Adam step on
// W, m, v in place -- the weights are read once and written once, the gradient never leaves the registers; otherwise g
// (nullable) receives dW.  Every workgroup writes the float64 sum of |W| over its tile (before the step) to
// l1[blockIdx.y * gridDim.x + blockIdx.x].  K % 256 == 0, N % 64 == 0.
template <bool ADAM>
__global__ void __launch_bounds__(256)
k_rgr_fc_wgrad(float* W, const float* __restrict__ x, const float* __restrict__ dz, int B, int N, int K, float coef,
               float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, float step_size, float bc2_sqrt, float b1,
               double* __restrict__ l1) {
    __shared__ float xs[16][256];
    __shared__ float zs[64][17];
    __shared__ double red[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * 256, r0 = blockIdx.y * 64;
    float acc[16][4];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0.0f;
    for (int b0 = 0; b0 < B; b0 += 16) {
        const int nb = min(16, B - b0);
        __syncthreads();
        for (int i = tid; i < 16 * 64; i += 256) {
            const int bb = i >> 6, c4 = (i & 63) * 4;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (bb < nb) val = *reinterpret_cast<const float4*>(x + (size_t)(b0 + bb) * K + c0 + c4);
            *reinterpret_cast<float4*>(&xs[bb][c4]) = val;
        }
        for (int i = tid; i < 64 * 16; i += 256) {
            const int r = i >> 4, bb = i & 15;
            zs[r][bb] = bb < nb ? dz[(size_t)(b0 + bb) * N + r0 + r] : 0.0f;
        }
        __syncthreads();
        for (int bb = 0; bb < nb; ++bb) {
            const float4 xv = *reinterpret_cast<const float4*>(&xs[bb][lane * 4]);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float z = zs[wave * 16 + r][bb];
                acc[r][0] = fmaf(z, xv.x, acc[r][0]);
                acc[r][1] = fmaf(z, xv.y, acc[r][1]);
                acc[r][2] = fmaf(z, xv.z, acc[r][2]);
                acc[r][3] = fmaf(z, xv.w, acc[r][3]);
            }
        }
    }
    const float inf = __builtin_inff();
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const size_t idx = (size_t)(r0 + wave * 16 + r) * K + c0 + lane * 4;
        rgr_f32x4 w = __builtin_nontemporal_load(reinterpret_cast<const rgr_f32x4*>(W + idx));
        float gg[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s += fabs((double)w[e]);
            gg[e] = acc[r][e] + coef * rgr_sign(w[e]);
        }
        if (ADAM) {
            rgr_f32x4 mm = __builtin_nontemporal_load(reinterpret_cast<const rgr_f32x4*>(m + idx));
            rgr_f32x4 vv = __builtin_nontemporal_load(reinterpret_cast<const rgr_f32x4*>(v + idx));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float me = mm[e], ve = vv[e];
                w[e] = adam_update(w[e], gg[e], me, ve, step_size, bc2_sqrt, b1, -inf, inf);
                mm[e] = me;
                vv[e] = ve;
            }
            __builtin_nontemporal_store(w, reinterpret_cast<rgr_f32x4*>(W + idx));
            __builtin_nontemporal_store(mm, reinterpret_cast<rgr_f32x4*>(m + idx));
            __builtin_nontemporal_store(vv, reinterpret_cast<rgr_f32x4*>(v + idx));
        } else if (g != nullptr) {
            *reinterpret_cast<float4*>(g + idx) = make_float4(gg[0], gg[1], gg[2], gg[3]);
        }
    }
    s = rgr_block_sum(s, red);
    if (tid == 0) l1[blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// ---- convolutions: implicit GEMMs on v_mfma_f32_16x16x4_f32 ----------------------------------------------------------
// Both passes share the forward's tile: C[m][n] = sum_k A[m][k] B[n][k], workgroup 64 (m) x 64 (n), k in steps of 32 through
// LDS (next step prefetched in registers), 4 waves of 2 x 2 MFMA blocks.  Loads come in two patterns: "row" (thread: one row,
// 8 consecutive k) and "k" (thread: one k, 8 consecutive rows), whichever keeps the global reads contiguous.
struct RgrTile {
    float a[RGR_CT][RGR_CK + 1];
    float b[RGR_CT][RGR_CK + 1];
};
__device__ __forceinline__ void rgr_tile_mma(const RgrTile& t, int wm, int wn, int li, int lq, rgr_f32x4 (&acc)[2][2]) {
#pragma unroll
    for (int kk = 0; kk < RGR_CK; kk += 4) {
        float a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = t.a[wm + i * 16 + li][kk + lq];
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = t.b[wn + j * 16 + li][kk + lq];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
}
__device__ __forceinline__ void rgr_ld8(const float* p, float (&r)[8]) {
    const float4 u = reinterpret_cast<const float4*>(p)[0], v = reinterpret_cast<const float4*>(p)[1];
    r[0] = u.x; r[1] = u.y; r[2] = u.z; r[3] = u.w; r[4] = v.x; r[5] = v.y; r[6] = v.z; r[7] = v.w;
}

// wgrad of a conv layer: C[co][n] = sum_k dz[k][co] X(k, n), n = (kh, kw, ci) (the device's weight layout), k = (b, oh, ow)
// over [0, B OH OW).  Split s of gridDim.z takes k in [s kc, (s+1) kc), kc = the per-split share rounded up to 32; the raw
// partial goes to slab[s][co][n] (k_rgr_wreduce sums the slabs).  dz: NHWC [B][OH][OH][cout]; X: the layer's input (NCHW
// [B][6][IH][IH] for conv1, NHWC otherwise).  grid (cout / 64, ceil(16 CIN / 64), S).
template <int CIN, bool NCHW>
__global__ void __launch_bounds__(256)
k_rgr_conv_wgrad(const float* __restrict__ dz, const float* __restrict__ X, int B, int IH, int cout, float* __restrict__ slab) {
    constexpr int N = 16 * CIN;
    __shared__ RgrTile t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int OH = IH >> 1, P = OH * OH, K = B * P;
    const int S = gridDim.z, s = blockIdx.z;
    const int kc = ((K + S - 1) / S + RGR_CK - 1) / RGR_CK * RGR_CK;
    const int kbeg = min(K, s * kc), kend = min(K, kbeg + kc);
    const int nsteps = (kend - kbeg + RGR_CK - 1) / RGR_CK;
    const int m0 = blockIdx.x * RGR_CT, n0 = blockIdx.y * RGR_CT;
    const int kk = tid >> 3, r8 = (tid & 7) * 8;          // "k" pattern for both operands

    float ra[8], rb[8];
    auto load = [&](int step) {
        const int k = kbeg + step * RGR_CK + kk;
        if (k >= kend) {
#pragma unroll
            for (int e = 0; e < 8; ++e) ra[e] = rb[e] = 0.0f;
            return;
        }
        rgr_ld8(dz + (size_t)k * cout + m0 + r8, ra);
        const int b = k / P, rr = k - b * P, oh = rr / OH, ow = rr - oh * OH;
        if (NCHW) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int n = n0 + r8 + e;
                const int khw = n / CIN, ci = n - khw * CIN;
                const int ih = 2 * oh - 1 + (khw >> 2), iw = 2 * ow - 1 + (khw & 3);
                rb[e] = (n < N && ih >= 0 && ih < IH && iw >= 0 && iw < IH) ? X[(((size_t)b * CIN + ci) * IH + ih) * IH + iw] : 0.0f;
            }
        } else {
            const int n = n0 + r8;                            // CIN % 8 == 0: the 8 share (kh, kw)
            const int khw = n / CIN, ci = n - khw * CIN;
            const int ih = 2 * oh - 1 + (khw >> 2), iw = 2 * ow - 1 + (khw & 3);
            if (ih >= 0 && ih < IH && iw >= 0 && iw < IH) {
                rgr_ld8(X + (((size_t)b * IH + ih) * IH + iw) * CIN + ci, rb);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) rb[e] = 0.0f;
            }
        }
    };

    rgr_f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = rgr_f32x4{0.f, 0.f, 0.f, 0.f};
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    const int li = lane & 15, lq = lane >> 4;

    if (nsteps > 0) load(0);
    for (int step = 0; step < nsteps; ++step) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { t.a[r8 + e][kk] = ra[e]; t.b[r8 + e][kk] = rb[e]; }
        __syncthreads();
        if (step + 1 < nsteps) load(step + 1);
        rgr_tile_mma(t, wm, wn, li, lq, acc);
        __syncthreads();
    }
    // C/D map of 16x16x4: col = lane & 15 (n), row = 4 * (lane >> 4) + r (m)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn + j * 16 + li;
            if (n >= N) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int mm = m0 + wm + i * 16 + 4 * lq + r;
                slab[((size_t)s * cout + mm) * N + n] = acc[i][j][r];
            }
        }
}

// g[i] = (((slab[0][i] + slab[1][i]) + ...) + slab[S-1][i]) + coef sign(w[i]);  n % 4 == 0
__global__ void __launch_bounds__(256)
k_rgr_wreduce(const float* __restrict__ slab, int S, size_t n, const float* __restrict__ w, float coef, float* __restrict__ g) {
    const size_t i4 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 >= n) return;
    float4 v = *reinterpret_cast<const float4*>(slab + i4);
    for (int s = 1; s < S; ++s) {
        const float4 u = *reinterpret_cast<const float4*>(slab + (size_t)s * n + i4);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    const float4 ww = *reinterpret_cast<const float4*>(w + i4);
    *reinterpret_cast<float4*>(g + i4) = make_float4(v.x + coef * rgr_sign(ww.x), v.y + coef * rgr_sign(ww.y),
                                                     v.z + coef * rgr_sign(ww.z), v.w + coef * rgr_sign(ww.w));
}

// dgrad of a conv layer (stride 2, k 4, pad 1: a transposed convolution), split into the 4 output-parity classes (grid z:
// py = z >> 1, px = z & 1).  Input pixel (ih, iw) = (2i + py, 2j + px) receives taps kh = (1 - py) + 2 ty from output row
// oh = i + py - ty (ty = 0, 1), the same along w: a 2 x 2-tap implicit GEMM, m = (b, i, j) over B OH OH, n = ci, k = (ty, tx, co)
// over 4 COUT.  The epilogue applies the derivative of the LeakyReLU that produced the layer's input:
// out[b][ih][iw][ci] = leaky'(act[...]) C[m][ci].  grid (ceil(B OH OH / 64), CIN / 64, 4); every input pixel is written once.
template <int CIN, int COUT>
__global__ void __launch_bounds__(256)
k_rgr_conv_dgrad(const float* __restrict__ dz, const float* __restrict__ wt, const float* __restrict__ act, int B, int IH,
                 float* __restrict__ out) {
    constexpr int K = 4 * COUT, nsteps = K / RGR_CK;
    static_assert(COUT % RGR_CK == 0 && CIN % RGR_CT == 0, "tile");
    __shared__ RgrTile t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int OH = IH >> 1, P = OH * OH, M = B * P;
    const int py = blockIdx.z >> 1, px = blockIdx.z & 1;
    const int m0 = blockIdx.x * RGR_CT, n0 = blockIdx.y * RGR_CT;

    // A ("row"): row lrow, k = lk .. lk + 8 (one tap, 8 consecutive co)
    const int lrow = tid >> 2, lk = (tid & 3) * 8;
    const int m = m0 + lrow;
    const bool mvalid = m < M;
    int pb = 0, pi = 0, pj = 0;
    if (mvalid) { pb = m / P; const int r = m - pb * P; pi = r / OH; pj = r - pi * OH; }
    // B ("k"): k = kk, rows n0 + r8 .. + 8 (8 consecutive ci)
    const int kk = tid >> 3, r8 = (tid & 7) * 8;

    float ra[8], rb[8];
    auto load = [&](int step) {
        {
            const int k = step * RGR_CK + lk;
            const int tap = k / COUT, co = k - tap * COUT;
            const int oh = pi + py - (tap >> 1), ow = pj + px - (tap & 1);
            if (mvalid && oh >= 0 && oh < OH && ow >= 0 && ow < OH) {
                rgr_ld8(dz + (((size_t)pb * OH + oh) * OH + ow) * COUT + co, ra);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) ra[e] = 0.0f;
            }
        }
        {
            const int k = step * RGR_CK + kk;
            const int tap = k / COUT, co = k - tap * COUT;
            const int kh = (1 - py) + 2 * (tap >> 1), kw = (1 - px) + 2 * (tap & 1);
            rgr_ld8(wt + (((size_t)co * 4 + kh) * 4 + kw) * CIN + n0 + r8, rb);
        }
    };

    rgr_f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = rgr_f32x4{0.f, 0.f, 0.f, 0.f};
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    const int li = lane & 15, lq = lane >> 4;

    load(0);
    for (int step = 0; step < nsteps; ++step) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { t.a[lrow][lk + e] = ra[e]; t.b[r8 + e][kk] = rb[e]; }
        __syncthreads();
        if (step + 1 < nsteps) load(step + 1);
        rgr_tile_mma(t, wm, wn, li, lq, acc);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn + j * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int mm = m0 + wm + i * 16 + 4 * lq + r;
                if (mm >= M) continue;
                const int b = mm / P, rr = mm - b * P, ii = rr / OH, jj = rr - ii * OH;
                const size_t p = (((size_t)b * IH + 2 * ii + py) * IH + 2 * jj + px) * CIN + n;
                out[p] = rgr_dleaky(acc[i][j][r], act[p]);
            }
        }
}

// ---- back to torch's layouts (gradients and weights leaving the device) ----------------------------------------------
// conv: [cout][kh][kw][cin] -> [cout][cin][kh][kw]
__global__ void k_rgr_unpack_conv(const float* __restrict__ src, int cout, int cin, float* __restrict__ dst) {
    const size_t n = (size_t)cout * cin * 16;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int khw = (int)(i % 16);
        const size_t r = i / 16;
        const int ci = (int)(r % cin);
        const size_t co = r / cin;
        dst[i] = src[(co * 16 + khw) * cin + ci];
    }
}
// FC1: NHWC column order ((h*7 + w)*512 + c) -> torch's NCHW flatten (c*49 + h*7 + w)
__global__ void k_rgr_unpack_fc1(const float* __restrict__ src, float* __restrict__ dst) {
    const size_t n = (size_t)4096 * 25088;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int k = (int)(i % 25088);
        const size_t o = i / 25088;
        const int c = k / 49, hw = k % 49;
        dst[i] = src[o * 25088 + (size_t)hw * 512 + c];
    }
}
