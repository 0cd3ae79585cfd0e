// k_prop_f64.h -- PropModuleDiffDen.forward (model/gnn_dyn.py:147-198) evaluated in float64, and the reduction of the
// accuracy probe.  A yardstick, not an engine: it is the reference's own formulation (relation propagator over
// cat[relation_encode, effect_r, effect_s, dens], particle propagator over cat[particle_encode, agg, dens] with the residual
// inside the ReLU), not the factored one the fp32 / split-fp16 kernels compute, so it shares no rounding with them.
//
// Arithmetic: every product and sum in double.  The 64-in blocks run on v_mfma_f64_16x16x4_f64, one wave per tile of 16
// rows (particles or relation slots); the 5- and 6-input first layers and the 3-output head are fma chains; the density
// column of the 193- and 129-wide layers is one fma after the k-loop, then the bias.  Every output has ONE reduction order:
// ascending k within a layer, ascending slot in the aggregation, no atomics; a row's result depends on nothing but the row,
// so it is the same bits in whichever tile, batch or chunk the row lands.
//
// MFMA operands (one double per lane): A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15];
// C/D (four doubles per lane): col = lane & 15, row = (lane >> 4) + 4 * reg.
#pragma once
#include "drp_common.h"

typedef double kf_d4 __attribute__((ext_vector_type(4)));

#define KF_WAVES 4                  // tiles per workgroup
#define KF_LD 66                    // doubles per row of a wave's LDS tile (64 + 2: the 16 rows of an A read fall into distinct banks)

// the 64x64 blocks of the blob, kept a second time in B-fragment order: [block][k-step 16][column tile 4][lane 64]
enum { KF_PE2 = 0, KF_RE2, KF_RE4, KF_PP_PE, KF_PP_AGG, KF_RP_E, KF_RP_R, KF_RP_S, KF_PR0, KF_BLOCKS };
#define KF_W_TOTAL ((int)W_TOTAL + KF_BLOCKS * 4096)    // doubles: the blob widened, then the fragments
// ... and the blocks a third time, in the B-fragment order of the transposed product dX = dY W (k_gd_f64.h): same layout, k = output
#define KF_W_ALL (KF_W_TOTAL + KF_BLOCKS * 4096)
// workspace per particle of a chunk, in bytes: particle_encode, 3 effects, 3 aggregates, prediction (64, 3 x 64, 3 x 64, 3 doubles)
// and per relation slot the encoding and 3 effects (10 x 4 x 64 doubles)
#define KF_BYTES_PER_PARTICLE ((size_t)(7 * 64 + 3 + DRP_K * 4 * 64) * sizeof(double))

__device__ __forceinline__ void kf_block_src(int blk, int& base, int& ld) {
    switch (blk) {
    case KF_PE2: base = W_PE2_W; ld = 64; break;
    case KF_RE2: base = W_RE2_W; ld = 64; break;
    case KF_RE4: base = W_RE4_W; ld = 64; break;
    case KF_PP_PE: base = W_PP_W; ld = 129; break;
    case KF_PP_AGG: base = W_PP_W + 64; ld = 129; break;
    case KF_RP_E: base = W_RP_W; ld = 193; break;
    case KF_RP_R: base = W_RP_W + 64; ld = 193; break;
    case KF_RP_S: base = W_RP_W + 128; ld = 193; break;
    default: base = W_PR0_W; ld = 64; break;
    }
}

// the fp32 blob (torch Linear layout [out][in]) widened exactly, and its 64x64 blocks as the B operand reads them
__global__ __launch_bounds__(256) void kf_widen_weights(const float* __restrict__ w, double* __restrict__ w64) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < (int)W_TOTAL) { w64[t] = (double)w[t]; return; }
    if (t >= KF_W_ALL) return;
    const bool tr = t >= KF_W_TOTAL;
    const int q = t - (tr ? KF_W_TOTAL : (int)W_TOTAL), blk = q >> 12, r = q & 4095;
    const int ks = r >> 8, jt = (r >> 6) & 3, lane = r & 63;
    int base, ld;
    kf_block_src(blk, base, ld);
    w64[t] = tr ? (double)w[base + (ks * 4 + (lane >> 4)) * ld + jt * 16 + (lane & 15)]
                : (double)w[base + (jt * 16 + (lane & 15)) * ld + ks * 4 + (lane >> 4)];
}

__device__ __forceinline__ const double* kf_frag(const double* w64, int blk) { return w64 + W_TOTAL + blk * 4096; }
__device__ __forceinline__ const double* kf_frag_t(const double* w64, int blk) { return w64 + KF_W_TOTAL + blk * 4096; }
__device__ __forceinline__ double kf_relu(double x) { return x > 0.0 ? x : 0.0; }

// acc[jt] += X W^T for one 64x64 block: a_row is this lane's row of X (64 doubles), k ascending
__device__ __forceinline__ void kf_mma64(kf_d4 acc[4], const double* a_row, const double* __restrict__ frag, int lane) {
    const int kq = lane >> 4;
#pragma unroll 4
    for (int ks = 0; ks < 16; ++ks) {
        const double a = a_row[ks * 4 + kq];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
            acc[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, frag[(ks * 4 + jt) * 64 + lane], acc[jt], 0, 0, 0);
    }
}

__device__ __forceinline__ void kf_zero(kf_d4 acc[4]) {
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) acc[jt] = kf_d4{0.0, 0.0, 0.0, 0.0};
}

// particle encoder on [s_delta, a, dens / 5000] (:174-175); rows = particles of the chunk, dens per sample.  TS: the type the
// impulses (below: the positions) come in -- float widened exactly, or double (a rollout that stays in double, k_gd_f64.h)
template <typename TS>
__global__ __launch_bounds__(64 * KF_WAVES) void kf_particle_encode(const double* __restrict__ w, const TS* __restrict__ s_delta,
                                                                    const float* __restrict__ attr, const float* __restrict__ dens,
                                                                    int N, int rows, double* __restrict__ pe) {
    __shared__ double X[KF_WAVES][16 * KF_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int row0 = (blockIdx.x * KF_WAVES + wave) * 16;
    const int row = min(row0 + r, rows - 1);
    double* x = X[wave];
    {
        const double in[5] = {(double)s_delta[(size_t)row * 3], (double)s_delta[(size_t)row * 3 + 1], (double)s_delta[(size_t)row * 3 + 2],
                              (double)attr[row], (double)dens[row / N] / 5000.0};
        for (int o = q * 16; o < q * 16 + 16; ++o) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 5; ++k) acc = fma(in[k], w[W_PE0_W + o * 5 + k], acc);
            x[r * KF_LD + o] = kf_relu(acc + w[W_PE0_B + o]);
        }
    }
    __syncthreads();
    kf_d4 acc[4];
    kf_zero(acc);
    kf_mma64(acc, x + r * KF_LD, kf_frag(w, KF_PE2), lane);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int col = jt * 16 + r, orow = row0 + q + 4 * g;
            if (orow < rows) pe[(size_t)orow * 64 + col] = kf_relu(acc[jt][g] + w[W_PE2_B + col]);
        }
}

// relation encoder on [a_r, a_s, s_r - s_s, dens / 5000] per list entry (:166-171,:179-180); rows = relation slots
// (receiver-major, DRP_K per particle); a slot past the receiver's count is written as zeros
template <typename TS>
__global__ __launch_bounds__(64 * KF_WAVES) void kf_relation_encode(const double* __restrict__ w, const TS* __restrict__ s_cur,
                                                                    const float* __restrict__ attr, const float* __restrict__ dens,
                                                                    const int16_t* __restrict__ idx, const uint8_t* __restrict__ cnt,
                                                                    int N, int rows, double* __restrict__ re) {
    __shared__ double X[KF_WAVES][16 * KF_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int row0 = (blockIdx.x * KF_WAVES + wave) * 16;
    const int e = min(row0 + r, rows - 1);
    double* x = X[wave];
    {
        const int p = e / DRP_K, k = e - p * DRP_K, b = p / N;
        const int s = (k < (int)cnt[p]) ? b * N + (int)idx[e] : p;
        const double in[6] = {(double)attr[p], (double)attr[s],
                              (double)s_cur[(size_t)p * 3] - (double)s_cur[(size_t)s * 3],
                              (double)s_cur[(size_t)p * 3 + 1] - (double)s_cur[(size_t)s * 3 + 1],
                              (double)s_cur[(size_t)p * 3 + 2] - (double)s_cur[(size_t)s * 3 + 2], (double)dens[b] / 5000.0};
        for (int o = q * 16; o < q * 16 + 16; ++o) {
            double acc = 0.0;
#pragma unroll
            for (int kk = 0; kk < 6; ++kk) acc = fma(in[kk], w[W_RE0_W + o * 6 + kk], acc);
            x[r * KF_LD + o] = kf_relu(acc + w[W_RE0_B + o]);
        }
    }
    __syncthreads();
    kf_d4 acc[4];
    kf_zero(acc);
    kf_mma64(acc, x + r * KF_LD, kf_frag(w, KF_RE2), lane);
    __syncthreads();
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int col = jt * 16 + r;
            x[(q + 4 * g) * KF_LD + col] = kf_relu(acc[jt][g] + w[W_RE2_B + col]);
        }
    __syncthreads();
    kf_zero(acc);
    kf_mma64(acc, x + r * KF_LD, kf_frag(w, KF_RE4), lane);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int oe = row0 + q + 4 * g;
        if (oe >= rows) continue;
        const bool valid = (oe % DRP_K) < (int)cnt[oe / DRP_K];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const int col = jt * 16 + r;
            re[(size_t)oe * 64 + col] = valid ? kf_relu(acc[jt][g] + w[W_RE4_B + col]) : 0.0;
        }
    }
}

// relation propagator on [relation_encode | effect_r | effect_s | dens], 193 -> 64 (:183-187)
__global__ __launch_bounds__(64 * KF_WAVES) void kf_relation_prop(const double* __restrict__ w, const double* __restrict__ re,
                                                                  const double* __restrict__ eff, const float* __restrict__ dens,
                                                                  const int16_t* __restrict__ idx, const uint8_t* __restrict__ cnt,
                                                                  int N, int rows, double* __restrict__ erel) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int row0 = (blockIdx.x * KF_WAVES + wave) * 16;
    const int e = min(row0 + r, rows - 1);
    const int p = e / DRP_K, k = e - p * DRP_K;
    const int s = (k < (int)cnt[p]) ? (p / N) * N + (int)idx[e] : p;
    kf_d4 acc[4];
    kf_zero(acc);
    kf_mma64(acc, re + (size_t)e * 64, kf_frag(w, KF_RP_E), lane);
    kf_mma64(acc, eff + (size_t)p * 64, kf_frag(w, KF_RP_R), lane);
    kf_mma64(acc, eff + (size_t)s * 64, kf_frag(w, KF_RP_S), lane);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int oe = row0 + q + 4 * g;
        if (oe >= rows) continue;
        const int op = oe / DRP_K;
        const bool valid = (oe - op * DRP_K) < (int)cnt[op];
        const double d = (double)dens[op / N] / 5000.0;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const int col = jt * 16 + r;
            const double v = fma(d, w[W_RP_W + col * 193 + 192], acc[jt][g]) + w[W_RP_B + col];
            erel[(size_t)oe * 64 + col] = valid ? kf_relu(v) : 0.0;
        }
    }
}

// sum over the receiver's entries in slot order (:189), then the particle propagator on [particle_encode | agg | dens],
// 129 -> 64, with the residual added before the ReLU (:191-193, :82-85); rows = particles
__global__ __launch_bounds__(64 * KF_WAVES) void kf_particle_prop(const double* __restrict__ w, const double* __restrict__ pe,
                                                                  const double* __restrict__ erel, const double* __restrict__ eff_prev,
                                                                  const float* __restrict__ dens, const uint8_t* __restrict__ cnt, int N,
                                                                  int rows, double* __restrict__ agg, double* __restrict__ eff_next) {
    __shared__ double X[KF_WAVES][16 * KF_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int row0 = (blockIdx.x * KF_WAVES + wave) * 16;
    const int row = min(row0 + r, rows - 1);
    double* x = X[wave];
    {
        const int n = (int)cnt[row];
        for (int f = q * 16; f < q * 16 + 16; ++f) {
            double a = 0.0;
            for (int k = 0; k < n; ++k) a += erel[((size_t)row * DRP_K + k) * 64 + f];
            x[r * KF_LD + f] = a;
            if (row0 + r < rows) agg[(size_t)row * 64 + f] = a;
        }
    }
    __syncthreads();
    kf_d4 acc[4];
    kf_zero(acc);
    kf_mma64(acc, pe + (size_t)row * 64, kf_frag(w, KF_PP_PE), lane);
    kf_mma64(acc, x + r * KF_LD, kf_frag(w, KF_PP_AGG), lane);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int orow = row0 + q + 4 * g;
        if (orow >= rows) continue;
        const double d = (double)dens[orow / N] / 5000.0;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const int col = jt * 16 + r;
            const double v = fma(d, w[W_PP_W + col * 129 + 128], acc[jt][g]) + w[W_PP_B + col];
            eff_next[(size_t)orow * 64 + col] = kf_relu(v + eff_prev[(size_t)orow * 64 + col]);
        }
    }
}

// predictor (:196, :110) and + s_cur (:198)
template <typename TS>
__global__ __launch_bounds__(64 * KF_WAVES) void kf_predict(const double* __restrict__ w, const double* __restrict__ eff,
                                                            const TS* __restrict__ s_cur, int rows, double* __restrict__ pred,
                                                            double* __restrict__ s_pred) {
    __shared__ double X[KF_WAVES][16 * KF_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int row0 = (blockIdx.x * KF_WAVES + wave) * 16;
    const int row = min(row0 + r, rows - 1);
    double* x = X[wave];
    kf_d4 acc[4];
    kf_zero(acc);
    kf_mma64(acc, eff + (size_t)row * 64, kf_frag(w, KF_PR0), lane);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int col = jt * 16 + r;
            x[(q + 4 * g) * KF_LD + col] = kf_relu(acc[jt][g] + w[W_PR0_B + col]);
        }
    __syncthreads();
    if (q < 3 && row0 + r < rows) {
        double a = 0.0;
        for (int k = 0; k < 64; ++k) a = fma(x[r * KF_LD + k], w[W_PR1_W + q * 64 + k], a);
        a += w[W_PR1_B + q];
        pred[(size_t)row * 3 + q] = a;
        s_pred[(size_t)row * 3 + q] = a + (double)s_cur[(size_t)row * 3 + q];
    }
}

// ---- the accuracy probe's reduction ---------------------------------------------------------------------------
// phase 0 (grid = parts): workgroup g takes the particles [g * per, (g + 1) * per) and leaves part[g] = {largest
// |s32 - s64| over its particles' coordinates, the lowest particle that has it, largest |s64 - s_cur|};
// phase 1 (one workgroup): the parts in index order -> out[0..3] (include/drp.h: drp_accuracy_probe).  A later part
// replaces an earlier one only when strictly larger, so ties go to the lowest index; a NaN counts as +inf.
#define KF_RED_THREADS 256
#define KF_RED_PARTS_MAX 256
__global__ __launch_bounds__(KF_RED_THREADS) void kf_probe_reduce(const float* __restrict__ s32, const double* __restrict__ s64,
                                                                  const float* __restrict__ s_cur, long n_part, long per,
                                                                  double* __restrict__ part, int parts, double* __restrict__ out, int phase) {
    if (phase == 1) {
        if (threadIdx.x != 0 || blockIdx.x != 0) return;
        double e = -1.0, ei = 0.0, dm = 0.0;
        for (int g = 0; g < parts; ++g) {
            if (part[g * 3] > e) { e = part[g * 3]; ei = part[g * 3 + 1]; }
            if (part[g * 3 + 2] > dm) dm = part[g * 3 + 2];
        }
        out[0] = e; out[1] = dm; out[2] = e / (dm > 1e-12 ? dm : 1e-12); out[3] = ei;
        return;
    }
    __shared__ double se[KF_RED_THREADS], sd[KF_RED_THREADS];
    __shared__ long si[KF_RED_THREADS];
    const long lo = (long)blockIdx.x * per, hi = min(lo + per, n_part);
    double e = -1.0, dm = 0.0;
    long ei = lo;
    for (long p = lo + threadIdx.x; p < hi; p += KF_RED_THREADS) {      // ascending: a thread keeps its first largest
        for (int k = 0; k < 3; ++k) {
            const double v64 = s64[p * 3 + k];
            double a = fabs((double)s32[p * 3 + k] - v64), d = fabs(v64 - (double)s_cur[p * 3 + k]);
            if (a != a) a = __builtin_inf();
            if (d != d) d = __builtin_inf();
            if (a > e) { e = a; ei = p; }
            if (d > dm) dm = d;
        }
    }
    se[threadIdx.x] = e; si[threadIdx.x] = ei; sd[threadIdx.x] = dm;
    __syncthreads();
    for (int off = KF_RED_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const double oe = se[threadIdx.x + off];
            const long oi = si[threadIdx.x + off];
            if (oe > se[threadIdx.x] || (oe == se[threadIdx.x] && oi < si[threadIdx.x])) { se[threadIdx.x] = oe; si[threadIdx.x] = oi; }
            if (sd[threadIdx.x + off] > sd[threadIdx.x]) sd[threadIdx.x] = sd[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[blockIdx.x * 3] = se[0]; part[blockIdx.x * 3 + 1] = (double)si[0]; part[blockIdx.x * 3 + 2] = sd[0]; }
}
