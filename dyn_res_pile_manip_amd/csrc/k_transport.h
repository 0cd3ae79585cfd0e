// Entropy-regularised optimal-transport distance of two padded cloud batches and its gradient: the loss that sees
// density AND gives every real row a gradient whatever the two counts are -- the matching of k_match.h leaves the larger cloud's
// surplus rows out.  Both clouds carry total mass 1.  With n_p, n_q real rows:
//   C[i][j] = |p_i - q_j|^2 in fp32, formed as kc_chamfer forms it (fp32 differences, dx*dx + dy*dy + dz*dz, no fused
//             multiply-add), widened to double exactly; everything behind it is double
//   a_i = 1 / n_p, b_j = 1 / n_q;  eps > 0 in squared-distance units, per sample;  K = iters sweeps
//   f = 0; for k = 1 .. K:   g_j = -eps LSE_i((f_i - C_ij) / eps + log a_i),  then  f_i = -eps LSE_j((g_j - C_ij) / eps + log b_j)
//             (LSE max-shifted: m = max x, m + log sum exp(x - m))
//   P_ij = a_i b_j exp((f_i + g_j - C_ij) / eps): the last update is f's, so its row sums are a_i to rounding -- every predicted
//             particle's whole mass is placed
//   transport = scale sum_ij P_ij C_ij / 3
//   d/dp_i  = scale sum_j P_ij 2 (p_i - q_j) / 3  (P a constant of the derivative; fp32 differences, the sum in double, rounded
//             once to fp32), +0.0 on padding
//   col_err = sum_j |sum_i P_ij - b_j|: the column-marginal violation K sweeps leave -- an output, not a stopping rule
// One workgroup of 512 threads per problem (sample, rollout step).  Both clouds lie in LDS as float4 and f, g as double:
// 16 + 16 + 8 + 8 KB, three problems (24 wavefronts) a CU.  The cost matrix is never stored: each half-sweep forms it again from LDS.
// THE MAPPING.  A half-sweep has one log-sum-exp per row of the cloud it updates (an "output"), over the rows of the other cloud
// (the "terms").  Each output is shared by PARTS = 2^lp adjacent lanes of one wavefront (kt_parts: the smallest power of two
// that gives the workgroup at least KT_MIN_ITEMS (output, part) items, at most 64 and no more than the terms can occupy): part
// s takes the terms s, s + PARTS, ... in ascending index, first for the maximum of f_i - C_ij (division by eps > 0 and the
// added constant are monotonic: the maximum of x is x at that term), then for the sum of exp(x - m); the parts are combined by
// an xor butterfly over the lane offsets PARTS/2 .. 1 (a + b is b + a bit for bit: every lane of the group ends with the same
// value).  Items are dealt to threads in ascending order, 512 at a time.  So a 20 x 20 problem runs 20 x 64 = 1 280 items in
// 3 rounds (83 % of the thread slots busy), not 20 threads for the whole sweep.  PARTS and with it the order of every sum is a function of the two
// COUNTS alone: the bits do not depend on the padded N, M, on B or on another sample.  No atomics.
// One barrier separates the half-sweeps (g's reads f and writes g; f's reads g and writes f).
// NO VALUE PROLONGS A LOOP: every trip count is fixed by K, n_p and n_q.  A non-finite coordinate (a diverged model) ends in
// a NaN term after the same number of steps.
#pragma once
#include "k_cloud_pair.h"

#define KT_THREADS 512          // two waves a SIMD: the exponentials' dependent chains overlap (DESIGN.md 9 has the sizes tried)
#define KT_WAVES (KT_THREADS / 64)
#define KT_UNROLL 4             // the sum's loop: four independent exponentials in flight, added in the same ascending order
#define KT_MAX_POINTS 1024      // per cloud: the work is K n_p n_q exponentials
#define KT_MAX_ITERS 1000
#define KT_MIN_ITEMS 1024       // (output, part) items a pass aims for: two rounds of the workgroup

struct KtArgs {
    const float* pred;          // p's rows (cp's strides)
    CloudPair cp;
    const double* eps;          // [B]
    int iters;
    double scale;
    float* grad;                // TRAIN: [H][B][N][3], every row written (padded rows 0); else [B][N][3], nullable
    double* terms;              // TRAIN: [H][B], scale * transport; else [B]
    double* dual;               // [B][N + M]: f then g (0 on padding), nullable; not TRAIN only
    double* col_err;            // [H][B] (TRAIN) or [B], nullable: the pass over the columns runs only where it is asked for
    float* zero; size_t n_zero; // TRAIN, nullable: filled with 0 (the gradient blob and kmb_step_bwd's counters, as kt_mse_grad does)
};

// log2 of the lanes that share one output's sum: by the counts alone
__device__ __forceinline__ int kt_parts(int n_out, int n_terms) {
    int lp = 0;
    while (lp < 6 && (n_out << lp) < KT_MIN_ITEMS && (1 << lp) < n_terms) ++lp;
    return lp;
}

__device__ __forceinline__ float kt_cost(const float4 a, const float4 b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;     // (a - b)^2 is (b - a)^2 bit for bit
    return dx * dx + dy * dy + dz * dz;
}

// the combination of the PARTS = 2^lp lanes of a group, in one fixed order; every lane of the wave calls them
__device__ __forceinline__ double kt_group_max(double v, int lp) {
    for (int off = (1 << lp) >> 1; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ double kt_group_sum(double v, int lp) {
    for (int off = (1 << lp) >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// out_dual[j] = -eps LSE_i((in_dual[i] - C_ij) / eps + log_mass) for every j < n_out; the caller's barrier is behind it.
// AVERAGE (k_divergence.h's self problems, both clouds the same one): out_dual[j] = (in_dual[j] + that) / 2
// DAMPED (k_divergence.h's unbalanced problems): `that` is lambda x the soft minimum -- one multiply per output, nothing per term
template <bool AVERAGE = false, bool DAMPED = false>
__device__ __forceinline__ void kt_half_sweep(const float4* out_pts, int n_out, const float4* in_pts, int n_in, const double* in_dual,
                                              double* out_dual, double eps, double log_mass, double lambda = 1.0) {
    const int lp = kt_parts(n_out, n_in), parts = 1 << lp, items = n_out << lp;
    const double ninf = -(double)__builtin_inff();
    for (int e0 = 0; e0 < items; e0 += KT_THREADS) {
        const int e = e0 + (int)threadIdx.x;
        const int j = e >> lp, s = e & (parts - 1);
        const bool live = j < n_out;
        const float4 o = out_pts[live ? j : 0];
        double top = ninf;
        for (int i = s; i < n_in; i += parts) {
            const double d = in_dual[i] - (double)kt_cost(in_pts[i], o);
            top = d > top ? d : top;
        }
        top = kt_group_max(top, lp);
        const double m = top / eps + log_mass;
        double sum = 0.0;
#pragma unroll KT_UNROLL
        for (int i = s; i < n_in; i += parts) {
            const double x = (in_dual[i] - (double)kt_cost(in_pts[i], o)) / eps + log_mass;
            sum += exp(x - m);
        }
        sum = kt_group_sum(sum, lp);
        if (live && s == 0) {
            const double u = -eps * (m + log(sum));
            const double v = DAMPED ? lambda * u : u;
            out_dual[j] = AVERAGE ? 0.5 * (in_dual[j] + v) : v;
        }
    }
}

// sum over the workgroup in one fixed order (lanes by xor-shuffle, then the waves in ascending order); valid in every thread
__device__ __forceinline__ double kt_block_sum(double v, double* s_w) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    double total = s_w[0];
#pragma unroll
    for (int w = 1; w < KT_WAVES; ++w) total += s_w[w];
    return total;
}

template <bool TRAIN>
__global__ void __launch_bounds__(KT_THREADS) kt_transport(KtArgs A) {
    __shared__ float4 s_p[KT_MAX_POINTS];
    __shared__ float4 s_q[KT_MAX_POINTS];
    __shared__ double s_f[KT_MAX_POINTS];
    __shared__ double s_g[KT_MAX_POINTS];
    __shared__ double s_w[KT_WAVES];
    const int b = blockIdx.x, t = blockIdx.y, B = gridDim.x;
    const int tid = threadIdx.x;
    const int N = A.cp.N, M = A.cp.M;
    if (TRAIN) train_zero_fill(A.zero, A.n_zero, KT_THREADS);
    const int np = A.cp.count_p(b, KT_MAX_POINTS), nq = A.cp.count_q(b, t, KT_MAX_POINTS);
    const float* p = A.cp.p_rows(A.pred, b, t);
    const float* q = A.cp.q_rows(b, t);
    const size_t slot = (size_t)t * B + b;
    float* g_out = A.grad != nullptr ? A.grad + slot * N * 3 : nullptr;
    double* dual = (!TRAIN && A.dual != nullptr) ? A.dual + slot * ((size_t)N + M) : nullptr;
    const bool empty = np == 0 || nq == 0;              // (the entry points refuse it)
    const int iters = empty ? 0 : min(max(A.iters, 0), KT_MAX_ITERS);
    const double eps = A.eps[b];

    for (int e = tid; e < np; e += KT_THREADS) {
        s_p[e] = make_float4(p[(size_t)e * 3], p[(size_t)e * 3 + 1], p[(size_t)e * 3 + 2], 0.0f);
        s_f[e] = 0.0;
    }
    for (int e = tid; e < nq; e += KT_THREADS) {
        s_q[e] = make_float4(q[(size_t)e * 3], q[(size_t)e * 3 + 1], q[(size_t)e * 3 + 2], 0.0f);
        s_g[e] = 0.0;
    }
    __syncthreads();

    const double mass_p = empty ? 0.0 : 1.0 / (double)np, mass_q = empty ? 0.0 : 1.0 / (double)nq;
    const double log_a = log(mass_p), log_b = log(mass_q);
    for (int k = 0; k < iters; ++k) {
        kt_half_sweep(s_q, nq, s_p, np, s_f, s_g, eps, log_a);
        __syncthreads();
        kt_half_sweep(s_p, np, s_q, nq, s_g, s_f, eps, log_b);
        __syncthreads();
    }

    // ---- the plan's rows: the term and the gradient ----
    const double ab = mass_p * mass_q;
    const double gscale = 2.0 * A.scale / 3.0;
    double acc = 0.0;
    {
        const int lp = kt_parts(np, nq), parts = 1 << lp, items = empty ? 0 : np << lp;
        for (int e0 = 0; e0 < items; e0 += KT_THREADS) {
            const int e = e0 + tid;
            const int i = e >> lp, s = e & (parts - 1);
            const bool live = i < np;
            const float4 o = s_p[live ? i : 0];
            const double fi = s_f[live ? i : 0];
            double sc = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
            for (int j = s; j < nq; j += parts) {
                const float4 r = s_q[j];
                const float dx = o.x - r.x, dy = o.y - r.y, dz = o.z - r.z;
                const double c = (double)(dx * dx + dy * dy + dz * dz);
                const double pij = ab * exp((fi + s_g[j] - c) / eps);
                sc += pij * c;
                sx += pij * (double)dx; sy += pij * (double)dy; sz += pij * (double)dz;
            }
            sc = kt_group_sum(sc, lp);
            if (g_out != nullptr) { sx = kt_group_sum(sx, lp); sy = kt_group_sum(sy, lp); sz = kt_group_sum(sz, lp); }
            if (live && s == 0) {
                acc += sc;
                if (g_out != nullptr) {             // rounded once
                    g_out[(size_t)i * 3] = (float)(gscale * sx); g_out[(size_t)i * 3 + 1] = (float)(gscale * sy);
                    g_out[(size_t)i * 3 + 2] = (float)(gscale * sz);
                }
            }
        }
    }
    // padding: gradient exactly 0
    if (g_out != nullptr)
        for (int e = (empty ? 0 : np) * 3 + tid; e < N * 3; e += KT_THREADS) g_out[e] = 0.0f;
    if (dual != nullptr) {
        for (int e = tid; e < N; e += KT_THREADS) dual[e] = (!empty && e < np) ? s_f[e] : 0.0;
        for (int e = tid; e < M; e += KT_THREADS) dual[(size_t)N + e] = (!empty && e < nq) ? s_g[e] : 0.0;
    }
    const double total = kt_block_sum(acc, s_w);
    if (tid == 0) A.terms[slot] = A.scale * (total / 3.0);

    // ---- the plan's columns: what the sweeps left of the column marginals ----
    if (A.col_err != nullptr) {
        double err = 0.0;
        const int lp = kt_parts(nq, np), parts = 1 << lp, items = empty ? 0 : nq << lp;
        for (int e0 = 0; e0 < items; e0 += KT_THREADS) {
            const int e = e0 + tid;
            const int j = e >> lp, s = e & (parts - 1);
            const bool live = j < nq;
            const float4 o = s_q[live ? j : 0];
            const double gj = s_g[live ? j : 0];
            double col = 0.0;
            for (int i = s; i < np; i += parts) col += ab * exp((s_f[i] + gj - (double)kt_cost(s_p[i], o)) / eps);
            col = kt_group_sum(col, lp);
            if (live && s == 0) err += fabs(col - mass_q);
        }
        const double sum = kt_block_sum(err, s_w);
        if (tid == 0) A.col_err[slot] = sum;
    }
}
