// Sinkhorn divergence of two padded cloud batches and its gradient: the transport loss of k_transport.h with its
// entropic bias taken out.  The cloud that minimises the entropy-regularised cost T_eps(p, q) over p is a shrunken copy of q;
//   S(p, q) = OT(p, q) - OT(p, p) / 2 - OT(q, q) / 2   (on the dual values)
// is non-negative, zero only for equal clouds, and still gives every real row a gradient whatever the two counts are.  With n_p,
// n_q real rows, a = 1 / n_p, b = 1 / n_q, eps > 0, K = iters and kt_transport's fp32 cost C:
//   cross problem   exactly kt_transport's sweeps: f = 0, K times g's update then f's; P_ij = a b exp((f_i + g_j - C_ij) / eps)
//   self problem of a cloud x with n rows, m = 1 / n:  h = 0; K times, for every j from the PREVIOUS sweep's h (Jacobi, two arrays):
//                   h_j <- (h_j + (-eps LSE_i((h_i - C^xx_ij) / eps + log m))) / 2;   S_ij = m^2 exp((h_i + h_j - C^xx_ij) / eps)
//                   -- symmetric by construction, one half-sweep a sweep
//   divergence = scale (sum_i a f_i + sum_j b g_j - sum_i a h^p_i - sum_j b h^q_j) / 3      (not clamped)
//   d/dp_i     = (2 scale / 3) (sum_j P_ij (p_i - q_j) - sum_j S^p_ij (p_i - p_j)): P, S constants of the derivative; fp32
//                differences widened, both sums in double, their difference rounded once to fp32; +0.0 on padding
//   col_err    = sum_j |sum_i P_ij - b| as kt_transport's;  self_err = [sum_i |sum_j S^p_ij - a|, sum_j |sum_i S^q_ij - b|]
// THE GRID.  The three sub-problems are independent chains of K dependent sweeps: kd_sweeps runs them as grid (B, H, 3), one
// 512-thread workgroup each (z = 0 cross, 1 p-p, 2 q-q), with kt_half_sweep's mapping of (output, part) items -- PARTS by the
// counts alone.  A self block keeps its one cloud in s_p and the two h arrays where the cross block keeps f and g.  What the
// blocks of one problem must share goes through a double scratch buffer: the three value sums, and the two gradient sums per
// row [2][H][B][N][3].  kd_combine, grid (B, H), follows in the stream: the fp32 gradient from the double difference, the zero
// padding, the term, and in the trainer the zero-fill of the gradient blob (train_zero_fill: this launch alone does it, on the
// grid the other loss kernels do it on).  The duals and the certificates are each written by the one block that owns them.
// No atomics, one summation order fixed by the counts, no value prolongs a loop (k_transport.h).
// UNBALANCED (kd_sweeps_unbalanced, kd_combine<., true>; include/drp.h: drp_cloud_divergence_unbalanced).  Each marginal is held
// by a KL penalty of weight rho (the reach, in eps's unit) in place of the hard constraint, and the target cloud carries total
// mass w: a = 1 / n_p, b = w / n_q, lambda = rho / (rho + eps).  Every sweep's soft minimum is multiplied by lambda (kt_half_sweep's
// DAMPED: one multiply per output), the self problems' mass is the cloud's own, and
//   divergence = scale (rho + eps / 2) (sum_i a (expm1(-h^p_i / rho) - expm1(-f_i / rho)) + sum_j b (expm1(-h^q_j / rho) - expm1(-g_j / rho))) / 3
//   col_err    = sum_j |sum_i P_ij - b exp(-g_j / rho)|;  self_err likewise against m exp(-h / rho);  the gradient's expression is the same
//   transported = sum_i a exp(-f_i / rho): the plan's total mass (its rows sum to a exp(-f_i / rho) exactly behind f's update)
// rho = +inf (with w = 1): lambda = 1 and the balanced value -- x 1.0 and exp(-0) are exact, so every output has the balanced
// kernel's bits.  Same LDS, same grid, same loops: the sums of the value are kt_block_sum's as the duals' are.
#pragma once
#include "k_transport.h"

#define KD_COMBINE_THREADS 256

struct KdArgs {
    const float* pred;          // p's rows (cp's strides)
    CloudPair cp;
    const double* eps;          // [B]
    int iters;
    double scale;
    double* vals;               // scratch [3][H][B]: sum a f + sum b g | sum a h^p | sum b h^q  (unbalanced: of -expm1(-. / rho))
    double* gsum;               // scratch [2][H][B][N][3]: sum_j P_ij (p_i - q_j) | sum_j S^p_ij (p_i - p_j), real rows; null: no gradient
    float* grad;                // [H][B][N][3], every row written (padded rows 0); null with gsum
    double* terms;              // [H][B]
    double* dual;               // [B][2N + 2M]: f, g, h^p, h^q (0 on padding), nullable; the one-shot only
    double* col_err;            // [H][B], nullable: the pass over the columns runs only where it is asked for
    double* self_err;           // [H][B][2], nullable
    float* zero; size_t n_zero; // the trainer, nullable: filled with 0 by kd_combine<true>
    const double* rho;          // unbalanced: [B], the reach (+inf: balanced); else null
    const double* mass_q;       // unbalanced: [H][B], the target cloud's total mass w; else null
    double* transported;        // unbalanced: [H][B], nullable
};

// what the relaxation adds to a block: the reach, its damping factor and whether it is the balanced limit
struct KdReach {
    double rho, lambda;
    bool balanced;
};
__device__ __forceinline__ KdReach kd_reach(double rho, double eps) {
    KdReach r;
    r.rho = rho;
    r.balanced = rho == (double)__builtin_inff();
    r.lambda = r.balanced ? 1.0 : rho / (rho + eps);
    return r;
}
// a dual's share of the value: the dual itself, or with a finite reach -expm1(-dual / rho) (kd_combine multiplies by rho + eps / 2)
template <bool UNBAL>
__device__ __forceinline__ double kd_value_term(double dual, const KdReach& r) {
    if (UNBAL && !r.balanced) return -expm1(-dual / r.rho);
    return dual;
}
// what a row (column) of a plan sums to at the fixed point: the mass, or with a finite reach what the penalty leaves of it
template <bool UNBAL>
__device__ __forceinline__ double kd_marginal(double mass, double dual, const KdReach& r) {
    if (UNBAL) return mass * exp(-dual / r.rho);
    return mass;
}

// z = 0: the cross problem -- kt_transport's sweeps; behind them the duals' sum, the plan's rows against q, col_err
template <bool UNBAL>
__device__ __forceinline__ void kd_cross(const KdArgs& A, float4* s_p, float4* s_q, double* s_f, double* s_g, double* s_w, const float* p,
                                         const float* q, int np, int nq, bool empty, int iters, double eps, size_t slot, const KdReach& R,
                                         double w) {
    const int tid = threadIdx.x;
    const int N = A.cp.N, M = A.cp.M;
    for (int e = tid; e < np; e += KT_THREADS) {
        s_p[e] = make_float4(p[(size_t)e * 3], p[(size_t)e * 3 + 1], p[(size_t)e * 3 + 2], 0.0f);
        s_f[e] = 0.0;
    }
    for (int e = tid; e < nq; e += KT_THREADS) {
        s_q[e] = make_float4(q[(size_t)e * 3], q[(size_t)e * 3 + 1], q[(size_t)e * 3 + 2], 0.0f);
        s_g[e] = 0.0;
    }
    __syncthreads();
    const double mass_p = empty ? 0.0 : 1.0 / (double)np, mass_q = empty ? 0.0 : (UNBAL ? w : 1.0) / (double)nq;
    const double log_a = log(mass_p), log_b = log(mass_q);
    for (int k = 0; k < iters; ++k) {
        kt_half_sweep<false, UNBAL>(s_q, nq, s_p, np, s_f, s_g, eps, log_a, R.lambda);
        __syncthreads();
        kt_half_sweep<false, UNBAL>(s_p, np, s_q, nq, s_g, s_f, eps, log_b, R.lambda);
        __syncthreads();
    }
    double acc = 0.0;
    if (!empty) {
        for (int e = tid; e < np; e += KT_THREADS) acc += mass_p * kd_value_term<UNBAL>(s_f[e], R);
        for (int e = tid; e < nq; e += KT_THREADS) acc += mass_q * kd_value_term<UNBAL>(s_g[e], R);
    }
    const double total = kt_block_sum(acc, s_w);
    if (tid == 0) A.vals[slot] = total;
    if (UNBAL && A.transported != nullptr) {
        double moved = 0.0;
        if (!empty)
            for (int e = tid; e < np; e += KT_THREADS) moved += kd_marginal<UNBAL>(mass_p, s_f[e], R);
        const double sum = kt_block_sum(moved, s_w);
        if (tid == 0) A.transported[slot] = sum;
    }
    if (A.dual != nullptr) {
        double* dual = A.dual + slot * (2 * ((size_t)N + M));
        for (int e = tid; e < N; e += KT_THREADS) dual[e] = (!empty && e < np) ? s_f[e] : 0.0;
        for (int e = tid; e < M; e += KT_THREADS) dual[(size_t)N + e] = (!empty && e < nq) ? s_g[e] : 0.0;
    }
    const double ab = mass_p * mass_q;
    if (A.gsum != nullptr) {
        double* gs = A.gsum + slot * N * 3;
        const int lp = kt_parts(np, nq), parts = 1 << lp, items = empty ? 0 : np << lp;
        for (int e0 = 0; e0 < items; e0 += KT_THREADS) {
            const int e = e0 + tid;
            const int i = e >> lp, s = e & (parts - 1);
            const bool live = i < np;
            const float4 o = s_p[live ? i : 0];
            const double fi = s_f[live ? i : 0];
            double sx = 0.0, sy = 0.0, sz = 0.0;
            for (int j = s; j < nq; j += parts) {
                const float4 r = s_q[j];
                const float dx = o.x - r.x, dy = o.y - r.y, dz = o.z - r.z;
                const double c = (double)(dx * dx + dy * dy + dz * dz);
                const double pij = ab * exp((fi + s_g[j] - c) / eps);
                sx += pij * (double)dx; sy += pij * (double)dy; sz += pij * (double)dz;
            }
            sx = kt_group_sum(sx, lp); sy = kt_group_sum(sy, lp); sz = kt_group_sum(sz, lp);
            if (live && s == 0) { gs[(size_t)i * 3] = sx; gs[(size_t)i * 3 + 1] = sy; gs[(size_t)i * 3 + 2] = sz; }
        }
    }
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
            if (live && s == 0) err += fabs(col - kd_marginal<UNBAL>(mass_q, gj, R));
        }
        const double sum = kt_block_sum(err, s_w);
        if (tid == 0) A.col_err[slot] = sum;
    }
}

// z = 1 (x = p) and 2 (x = q): the self problem of one cloud of n rows (row length `len` in the padded batch) -- the averaged
// Jacobi sweeps between h0 and h1; behind them h's sum, the symmetric plan's rows against x itself (the gradient's second sum:
// p's only) and self_err.  total_mass: the cloud's (1, or the unbalanced target's w)
template <bool UNBAL>
__device__ __forceinline__ void kd_self(const KdArgs& A, float4* s_x, double* h0, double* h1, double* s_w, const float* x, int n, int len,
                                        bool empty, int iters, double eps, size_t slot, size_t slots, int which, double* dual,
                                        const KdReach& R, double total_mass) {
    const int tid = threadIdx.x;
    for (int e = tid; e < n; e += KT_THREADS) {
        s_x[e] = make_float4(x[(size_t)e * 3], x[(size_t)e * 3 + 1], x[(size_t)e * 3 + 2], 0.0f);
        h0[e] = 0.0;
    }
    __syncthreads();
    const double mass = empty ? 0.0 : (UNBAL ? total_mass : 1.0) / (double)n;
    const double log_m = log(mass);
    double* cur = h0;
    double* nxt = h1;
    for (int k = 0; k < iters; ++k) {
        kt_half_sweep<true, UNBAL>(s_x, n, s_x, n, cur, nxt, eps, log_m, R.lambda);
        __syncthreads();
        double* const sw = cur; cur = nxt; nxt = sw;
    }
    double acc = 0.0;
    if (!empty)
        for (int e = tid; e < n; e += KT_THREADS) acc += mass * kd_value_term<UNBAL>(cur[e], R);
    const double total = kt_block_sum(acc, s_w);
    if (tid == 0) A.vals[(size_t)(1 + which) * slots + slot] = total;
    if (dual != nullptr)
        for (int e = tid; e < len; e += KT_THREADS) dual[e] = (!empty && e < n) ? cur[e] : 0.0;
    double* gs = (which == 0 && A.gsum != nullptr) ? A.gsum + (slots + slot) * A.cp.N * 3 : nullptr;
    if (gs == nullptr && A.self_err == nullptr) return;
    const double mm = mass * mass;
    double err = 0.0;
    const int lp = kt_parts(n, n), parts = 1 << lp, items = empty ? 0 : n << lp;
    for (int e0 = 0; e0 < items; e0 += KT_THREADS) {
        const int e = e0 + tid;
        const int i = e >> lp, s = e & (parts - 1);
        const bool live = i < n;
        const float4 o = s_x[live ? i : 0];
        const double hi = cur[live ? i : 0];
        double row = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
        for (int j = s; j < n; j += parts) {
            const float4 r = s_x[j];
            const float dx = o.x - r.x, dy = o.y - r.y, dz = o.z - r.z;
            const double c = (double)(dx * dx + dy * dy + dz * dz);
            const double sij = mm * exp((hi + cur[j] - c) / eps);
            row += sij;
            sx += sij * (double)dx; sy += sij * (double)dy; sz += sij * (double)dz;
        }
        row = kt_group_sum(row, lp);
        if (gs != nullptr) { sx = kt_group_sum(sx, lp); sy = kt_group_sum(sy, lp); sz = kt_group_sum(sz, lp); }
        if (live && s == 0) {
            err += fabs(row - kd_marginal<UNBAL>(mass, hi, R));
            if (gs != nullptr) { gs[(size_t)i * 3] = sx; gs[(size_t)i * 3 + 1] = sy; gs[(size_t)i * 3 + 2] = sz; }
        }
    }
    if (A.self_err != nullptr) {
        const double sum = kt_block_sum(err, s_w);
        if (tid == 0) A.self_err[slot * 2 + which] = sum;
    }
}

template <bool UNBAL>
__device__ __forceinline__ void kd_sweeps_body(const KdArgs& A) {
    __shared__ float4 s_p[KT_MAX_POINTS];       // cross: p; self: the cloud
    __shared__ float4 s_q[KT_MAX_POINTS];       // cross: q
    __shared__ double s_f[KT_MAX_POINTS];       // cross: f; self: h of the even sweeps
    __shared__ double s_g[KT_MAX_POINTS];       // cross: g; self: h of the odd sweeps
    __shared__ double s_w[KT_WAVES];
    const int b = blockIdx.x, t = blockIdx.y, z = blockIdx.z, B = gridDim.x;
    const int N = A.cp.N, M = A.cp.M;
    const int np = A.cp.count_p(b, KT_MAX_POINTS), nq = A.cp.count_q(b, t, KT_MAX_POINTS);
    const float* p = A.cp.p_rows(A.pred, b, t);
    const float* q = A.cp.q_rows(b, t);
    const size_t slot = (size_t)t * B + b, slots = (size_t)gridDim.y * B;
    const bool empty = np == 0 || nq == 0;              // (the entry points refuse it)
    const int iters = empty ? 0 : min(max(A.iters, 0), KT_MAX_ITERS);
    const double eps = A.eps[b];
    KdReach R{};
    double w = 1.0;
    if (UNBAL) {
        R = kd_reach(A.rho[b], eps);
        w = A.mass_q[slot];
    }
    double* dual = A.dual != nullptr ? A.dual + slot * (2 * ((size_t)N + M)) : nullptr;
    if (z == 0) kd_cross<UNBAL>(A, s_p, s_q, s_f, s_g, s_w, p, q, np, nq, empty, iters, eps, slot, R, w);
    else if (z == 1) kd_self<UNBAL>(A, s_p, s_f, s_g, s_w, p, np, N, empty, iters, eps, slot, slots, 0, dual != nullptr ? dual + N + M : nullptr, R, 1.0);
    else kd_self<UNBAL>(A, s_p, s_f, s_g, s_w, q, nq, M, empty, iters, eps, slot, slots, 1, dual != nullptr ? dual + 2 * (size_t)N + M : nullptr, R, w);
}

__global__ void __launch_bounds__(KT_THREADS) kd_sweeps(KdArgs A) { kd_sweeps_body<false>(A); }
__global__ void __launch_bounds__(KT_THREADS) kd_sweeps_unbalanced(KdArgs A) { kd_sweeps_body<true>(A); }

// behind kd_sweeps in the stream: what needs more than one block's results
template <bool TRAIN, bool UNBAL = false>
__global__ void __launch_bounds__(KD_COMBINE_THREADS) kd_combine(KdArgs A) {
    const int b = blockIdx.x, t = blockIdx.y, B = gridDim.x;
    const int tid = threadIdx.x;
    const int N = A.cp.N;
    if (TRAIN) train_zero_fill(A.zero, A.n_zero, KD_COMBINE_THREADS);
    const int np = A.cp.count_p(b, KT_MAX_POINTS), nq = A.cp.count_q(b, t, KT_MAX_POINTS);
    const bool empty = np == 0 || nq == 0;
    const size_t slot = (size_t)t * B + b, slots = (size_t)gridDim.y * B;
    if (A.grad != nullptr && A.gsum != nullptr) {
        const double gscale = 2.0 * A.scale / 3.0;
        const double* cross = A.gsum + slot * N * 3;
        const double* self = A.gsum + (slots + slot) * N * 3;
        float* g = A.grad + slot * N * 3;
        const int real = (empty ? 0 : np) * 3;
        for (int e = tid; e < N * 3; e += KD_COMBINE_THREADS) g[e] = e < real ? (float)(gscale * (cross[e] - self[e])) : 0.0f;     // rounded once
    }
    if (tid == 0) {
        const double sum = A.vals[slot] - A.vals[slots + slot] - A.vals[2 * slots + slot];
        const KdReach R = UNBAL ? kd_reach(A.rho[b], A.eps[b]) : KdReach{};
        if (UNBAL && !R.balanced) A.terms[slot] = A.scale * (((R.rho + 0.5 * A.eps[b]) * sum) / 3.0);
        else A.terms[slot] = A.scale * (sum / 3.0);
    }
}
