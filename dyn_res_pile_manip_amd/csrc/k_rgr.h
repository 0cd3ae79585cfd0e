// The resolution regressor (model/res_regressor.py:106-177, MPCResRgrNoPool; MPCResCls :15-104 differs in its head only):
// the CNN that picks the particle count at every MPC step (env/flex_env.py:981-998, :1083-1086).
//   input  [B,6,224,224] NCHW fp32 (the stack: init, goal, their distance images / h, the two exclusions)
//   conv   5 x Conv2d(k=4, s=2, p=1) + LeakyReLU(0.2), 6 -> 64 -> 128 -> 256 -> 512 -> 512, 224 -> 112 -> 56 -> 28 -> 14 -> 7
//   fc     25088 -> 4096 -> 1024 -> 256 -> 64, each + LeakyReLU(0.2); head 64 -> 1 (regressor) or 6 (classifier)
// Numerics: fp32 everywhere (fp32-input MFMA, exact products).  Every output element has ONE reduction tree, fixed by the
// layer and independent of the batch: the k order inside a tile, the split count of each layer (constants below) and the
// order in which the split partials are summed (k_rgr_splitk_reduce, slab 0 first).  A sample's outputs are therefore
// bit-identical whatever batch it travels in.  No float atomics.
// Internal layouts: activations NHWC [B][H][W][C]; conv weights [Cout][kh][kw][Cin]; FC1's columns permuted to the NHWC
// flatten order (k_rgr_repack_conv / k_rgr_repack_fc1); FC2..head as torch stores them ([out][in]).
#pragma once
#include "drp_common.h"
#include "k_goal.h"

#define RGR_S 224                 // state_h = state_w (config train_res_cls)
#define RGR_BMAX 64               // batch bound of the device buffers
#define RGR_SLOPE 0.2f            // LeakyReLU negative_slope

typedef float rgr_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float rgr_leaky(float v) { return v > 0.0f ? v : v * RGR_SLOPE; }

// ---- the stack (model/res_regressor.py:146-175) ---------------------------------------------------------------------
// Both distance transforms of (1 - mask) in ONE launch: workgroup z transforms mask z ([2][h][w] u8, nonzero = 1).
__global__ void __launch_bounds__(DT_THREADS)
k_rgr_dt_cv5_pair(const uint8_t* __restrict__ masks, int h, int w, int* __restrict__ tmp, float* __restrict__ dist) {
    extern __shared__ int s_rows[];
    __shared__ int s_w[16];
    __shared__ int s_carry;
    const size_t off = (size_t)blockIdx.x * h * w;
    dt_cv5_body<true>(masks + off, h, w, tmp + off, dist + off, s_rows, s_w, s_carry);
}

__global__ void __launch_bounds__(256)
k_rgr_edt_cols_pair(const uint8_t* __restrict__ masks, int h, int w, int* __restrict__ g) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    const size_t off = (size_t)blockIdx.y * h * w;
    edt_cols_body<true>(masks + off, h, w, g + off, x);
}

__global__ void __launch_bounds__(256)
k_rgr_edt_rows_pair(const int* __restrict__ g, int h, int w, float* __restrict__ dist) {
    extern __shared__ int s_g[];
    const size_t off = (size_t)blockIdx.y * h * w;
    edt_rows_body(g + off, w, dist + off, s_g, blockIdx.x);
}

// The six channels at one source pixel.  The distance images are divided by h (a float32 true division, :146-147).
struct RgrPix { float v[6]; };
__device__ __forceinline__ RgrPix rgr_pix(const uint8_t* __restrict__ masks, const float* __restrict__ dist, size_t npix,
                                          size_t i, float fh) {
    const bool a = masks[i] != 0, b = masks[npix + i] != 0;
    RgrPix p;
    p.v[0] = a ? 1.0f : 0.0f;
    p.v[1] = b ? 1.0f : 0.0f;
    p.v[2] = dist[i] / fh;
    p.v[3] = dist[npix + i] / fh;
    p.v[4] = (a && !b) ? 1.0f : 0.0f;        // init AND NOT goal (:149)
    p.v[5] = (b && !a) ? 1.0f : 0.0f;        // goal AND NOT init (:150)
    return p;
}

// INTER_AREA downscale of all six channels to 224 x 224 (:152-157), one workgroup per destination row, x [6][224][224].
// General scale: tables per axis (host, computed in double, stored as float): destination d takes the source indices
// si[off[d] .. off[d+1]) with weights a[...].  Horizontal weighted sums per source row first (float32, in table order),
// then the vertical weighted accumulation (float32, in table order).  Integer scale on both axes (fast = 1): the block
// mean, the block summed in row-major order times the float 1 / (fx * fy).
struct RgrTabs {
    const int* xoff; const int* xsi; const float* xa;
    const int* yoff; const int* ysi; const float* ya;
};
__global__ void __launch_bounds__(256)
k_rgr_stack(const uint8_t* __restrict__ masks, const float* __restrict__ dist, int h, int w, RgrTabs t, int fast, int fx,
            int fy, float inv_area, float* __restrict__ x) {
    const int dy = blockIdx.x, dx = threadIdx.x;
    if (dx >= RGR_S) return;
    const size_t npix = (size_t)h * w;
    const float fh = (float)h;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (fast) {
        for (int r = 0; r < fy; ++r) {
            const size_t row = (size_t)(dy * fy + r) * w;
            for (int q = 0; q < fx; ++q) {
                const RgrPix p = rgr_pix(masks, dist, npix, row + (size_t)dx * fx + q, fh);
#pragma unroll
                for (int c = 0; c < 6; ++c) acc[c] = acc[c] + p.v[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[c] = acc[c] * inv_area;
    } else {
        const int x0 = t.xoff[dx], x1 = t.xoff[dx + 1];
        for (int j = t.yoff[dy]; j < t.yoff[dy + 1]; ++j) {
            const size_t row = (size_t)t.ysi[j] * w;
            const float beta = t.ya[j];
            float hs[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int k = x0; k < x1; ++k) {
                const RgrPix p = rgr_pix(masks, dist, npix, row + t.xsi[k], fh);
                const float alpha = t.xa[k];
#pragma unroll
                for (int c = 0; c < 6; ++c) hs[c] = hs[c] + p.v[c] * alpha;
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) acc[c] = acc[c] + beta * hs[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) x[((size_t)c * RGR_S + dy) * RGR_S + dx] = acc[c];
}

// ---- weight repack (once per drp_rgr_load) ----------------------------------------------------------------------------
// conv: torch [cout][cin][4][4] -> [cout][kh][kw][cin]
__global__ void k_rgr_repack_conv(const float* __restrict__ src, int cout, int cin, float* __restrict__ dst) {
    const size_t n = (size_t)cout * cin * 16;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int ci = (int)(i % cin);
        const size_t r = i / cin;
        const int khw = (int)(r % 16);
        const size_t co = r / 16;
        dst[i] = src[(co * cin + ci) * 16 + khw];
    }
}
// FC1: torch flattens NCHW (feature c*49 + h*7 + w); the device's conv5 output is NHWC ((h*7 + w)*512 + c)
__global__ void k_rgr_repack_fc1(const float* __restrict__ src, float* __restrict__ dst) {
    const size_t n = (size_t)4096 * 25088;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int k = (int)(i % 25088);
        const size_t o = i / 25088;
        const int c = k % 512, hw = k / 512;
        dst[i] = src[o * 25088 + (size_t)c * 49 + hw];
    }
}

// ---- convolutions: implicit GEMM on v_mfma_f32_16x16x4_f32 ----------------------------------------------------------
// C[m][n] = sum_k A[m][k] W[n][k]: m = (b, oh, ow) output position, n = output channel, k = (kh, kw, ci).
// A is gathered on the fly (zero padding inside the gather).  Workgroup tile 64 (m) x 64 (n), k in steps of 32 staged through
// LDS (next step prefetched in registers); 4 waves, each 32 x 32 = 2 x 2 MFMA blocks.  Split-K over gridDim.z (split s takes
// k in [s*K/S, (s+1)*K/S)): with S = 1 the epilogue adds the bias and applies LeakyReLU, otherwise the raw partial goes to
// slab [S][M][Cout] for k_rgr_splitk_reduce.
#define RGR_CT 64
#define RGR_CK 32
template <int CIN, bool NCHW>
__global__ void __launch_bounds__(256)
k_rgr_conv(const float* __restrict__ in, int B, int IH, const float* __restrict__ wt, const float* __restrict__ bias, int cout,
           float* __restrict__ out, float* __restrict__ slab) {
    constexpr int K = 16 * CIN;
    __shared__ float sA[RGR_CT][RGR_CK + 1];
    __shared__ float sB[RGR_CT][RGR_CK + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int OH = IH >> 1, P = OH * OH;
    const int M = B * P;
    const int S = gridDim.z, s = blockIdx.z;
    const int ks = K / S, k_begin = s * ks, nsteps = ks / RGR_CK;
    const int m0 = blockIdx.x * RGR_CT, n0 = blockIdx.y * RGR_CT;

    // this thread's loads: row (m or n) = tid / 4, k = (tid % 4) * 8 .. + 8 within the step
    const int lrow = tid >> 2, lk = (tid & 3) * 8;
    const int m = m0 + lrow;
    int pb = 0, poh = 0, pow_ = 0;
    const bool mvalid = m < M;
    if (mvalid) { pb = m / P; const int r = m - pb * P; poh = r / OH; pow_ = r - poh * OH; }
    const float* wrow = wt + (size_t)(n0 + lrow) * K + k_begin + lk;

    float ra[8], rb[8];
    auto load = [&](int step) {
        const int kg = k_begin + step * RGR_CK + lk;      // first of 8 consecutive k
        if (NCHW) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int kk = kg + e;
                const int khw = kk / CIN, ci = kk - khw * CIN;
                const int ih = 2 * poh - 1 + (khw >> 2), iw = 2 * pow_ - 1 + (khw & 3);
                ra[e] = (mvalid && ih >= 0 && ih < IH && iw >= 0 && iw < IH)
                            ? in[(((size_t)pb * CIN + ci) * IH + ih) * IH + iw] : 0.0f;
            }
        } else {
            const int khw = kg / CIN, ci = kg - khw * CIN;  // CIN % 8 == 0: the 8 share (kh, kw)
            const int ih = 2 * poh - 1 + (khw >> 2), iw = 2 * pow_ - 1 + (khw & 3);
            if (mvalid && ih >= 0 && ih < IH && iw >= 0 && iw < IH) {
                const float4* p = reinterpret_cast<const float4*>(in + (((size_t)pb * IH + ih) * IH + iw) * CIN + ci);
                const float4 u = p[0], v = p[1];
                ra[0] = u.x; ra[1] = u.y; ra[2] = u.z; ra[3] = u.w; ra[4] = v.x; ra[5] = v.y; ra[6] = v.z; ra[7] = v.w;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) ra[e] = 0.0f;
            }
        }
        const float4* q = reinterpret_cast<const float4*>(wrow + step * RGR_CK);
        const float4 u = q[0], v = q[1];
        rb[0] = u.x; rb[1] = u.y; rb[2] = u.z; rb[3] = u.w; rb[4] = v.x; rb[5] = v.y; rb[6] = v.z; rb[7] = v.w;
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
        for (int e = 0; e < 8; ++e) { sA[lrow][lk + e] = ra[e]; sB[lrow][lk + e] = rb[e]; }
        __syncthreads();
        if (step + 1 < nsteps) load(step + 1);
#pragma unroll
        for (int kk = 0; kk < RGR_CK; kk += 4) {
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = sA[wm + i * 16 + li][kk + lq];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = sB[wn + j * 16 + li][kk + lq];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map of 16x16x4: col = lane & 15 (n), row = 4 * (lane >> 4) + r (m)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn + j * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int mm = m0 + wm + i * 16 + 4 * lq + r;
                if (mm >= M) continue;
                if (S == 1) out[(size_t)mm * cout + n] = rgr_leaky(acc[i][j][r] + bias[n]);
                else slab[((size_t)s * M + mm) * cout + n] = acc[i][j][r];
            }
        }
}

// out[i] = leaky((((slab[0][i] + slab[1][i]) + ...) + slab[S-1][i]) + bias[i % n]); mn = rows * n, n % 4 == 0
__global__ void __launch_bounds__(256)
k_rgr_splitk_reduce(const float* __restrict__ slab, int S, size_t mn, int n, const float* __restrict__ bias,
                    float* __restrict__ out) {
    const size_t i4 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 >= mn) return;
    float4 v = *reinterpret_cast<const float4*>(slab + i4);
    for (int s = 1; s < S; ++s) {
        const float4 u = *reinterpret_cast<const float4*>(slab + (size_t)s * mn + i4);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    const int c = (int)(i4 % n);
    const float4 bb = *reinterpret_cast<const float4*>(bias + c);
    float4 o;
    o.x = rgr_leaky(v.x + bb.x); o.y = rgr_leaky(v.y + bb.y); o.z = rgr_leaky(v.z + bb.z); o.w = rgr_leaky(v.w + bb.w);
    *reinterpret_cast<float4*>(out + i4) = o;
}

// ---- fully connected layers: weight-streaming GEMV on v_mfma_f32_16x16x4_f32 ----------------------------------------
// out[b][o] = sum_k W[o][k] x[b][k].  A = 16 weight rows per wave, B = 16 samples (grid z: sample group of 16; missing
// samples are zero columns).  Workgroup: WAVES x 16 rows, one K slice of KS = K / S (grid y); the slice of x for its 16
// samples sits in LDS for the whole launch, the weights go straight from HBM to VGPRs, DEPTH chunks of 32 k in flight per
// lane (lane: row lane & 15, k = 32c + 16t + 4 (lane >> 4) + q, the same k order for every row and every sample).
// S = 1: bias + LeakyReLU in the epilogue; otherwise partials to part [S][B][N] (k_rgr_splitk_reduce).
template <int K, int S, int WAVES, int DEPTH>
__global__ void __launch_bounds__(WAVES * 64)
k_rgr_fc(const float* __restrict__ W, const float* __restrict__ x, int B, int N, const float* __restrict__ bias,
         float* __restrict__ out, float* __restrict__ part) {
    constexpr int KS = K / S, NCH = KS / 32, LDX = KS + 4;
    static_assert(KS % 32 == 0, "K slice");
    extern __shared__ float xs[];                  // [16][LDX]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lq = lane >> 4;
    const int s = blockIdx.y, g = blockIdx.z;
    const int row0 = (blockIdx.x * WAVES + wave) * 16;
    const float* wp = W + (size_t)(row0 + li) * K + (size_t)s * KS + 4 * lq;

    rgr_f32x4 wr[DEPTH][2];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
        if (d < NCH) {
            wr[d][0] = __builtin_nontemporal_load(reinterpret_cast<const rgr_f32x4*>(wp + 32 * d));
            wr[d][1] = __builtin_nontemporal_load(reinterpret_cast<const rgr_f32x4*>(wp + 32 * d + 16));
        }
    // the x slice of samples g*16 .. g*16+15 (zeros past B)
    for (int i = tid; i < 16 * (KS / 4); i += WAVES * 64) {
        const int b = i / (KS / 4), k4 = (i - b * (KS / 4)) * 4;
        const int bb = g * 16 + b;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bb < B) v = *reinterpret_cast<const float4*>(x + (size_t)bb * K + (size_t)s * KS + k4);
        *reinterpret_cast<float4*>(xs + b * LDX + k4) = v;
    }
    __syncthreads();

    rgr_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* xr = xs + li * LDX + 4 * lq;
    for (int c0 = 0; c0 < NCH; c0 += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            const int c = c0 + d;
            if (c < NCH) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const float4 xv = *reinterpret_cast<const float4*>(xr + 32 * c + 16 * t);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[d][t].x, xv.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[d][t].y, xv.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[d][t].z, xv.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[d][t].w, xv.w, acc, 0, 0, 0);
                }
                if (c + DEPTH < NCH) {
                    wr[d][0] = __builtin_nontemporal_load(reinterpret_cast<const rgr_f32x4*>(wp + 32 * (c + DEPTH)));
                    wr[d][1] = __builtin_nontemporal_load(reinterpret_cast<const rgr_f32x4*>(wp + 32 * (c + DEPTH) + 16));
                }
            }
        }
    }
    // C/D: col = lane & 15 (sample), row = 4 * (lane >> 4) + r (output)
    const int b = g * 16 + li;
    if (b >= B) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = row0 + 4 * lq + r;
        if (S == 1) out[(size_t)b * N + o] = rgr_leaky(acc[r] + bias[o]);
        else part[((size_t)s * B + b) * N + o] = acc[r];
    }
}

// head: out[b][o] = bias[o] + sum_k W[o][k] x[b][k] (sequential fmaf chain over k = 0..63, no activation)
__global__ void k_rgr_head(const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ x, int B,
                           int n_out, float* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= B * n_out) return;
    const int b = i / n_out, o = i - b * n_out;
    float acc = 0.0f;
    for (int k = 0; k < 64; ++k) acc = fmaf(W[o * 64 + k], x[b * 64 + k], acc);
    out[i] = acc + bias[o];
}
