// k_divergence_f64.h -- k_divergence.h's Sinkhorn divergence and its gradient with NOTHING in fp32: the yardstick of
// the 'sinkhorn' loss, stand-alone (drp_cloud_divergence_f64) and as the seed of the float64 reverse pass
// (drp_train_grad_f64_divergence, launched where kt64_mse and kc64_chamfer are).  A yardstick like k_chamfer_f64.h, not an engine.
// The definition is k_divergence.h's, sweep for sweep; what differs is the arithmetic in front of the exponentials:
//   p          double: the caller's doubles, or in the trainer the float64 tape's predicted state
//   q          the caller's floats, widened where they are loaded
//   C_ij       dx*dx + dy*dy + dz*dz in double in that order on double differences (-ffp-contract=off: no fused multiply-add) --
//              of p - q, p - p and q - q alike
//   d/dp_i     (2 scale / 3) (sum_j P_ij (p_i - q_j) - sum_j S^p_ij (p_i - p_j)) written as double, never rounded to fp32; +0.0 on
//              padding
//   value      scale (sum_i a f_i + sum_j b g_j - sum_i a h^p_i - sum_j b h^q_j) / 3, the dual form, not clamped
// The plans are therefore exp(. / eps) of a cost that carries every bit of the float64 prediction: the fp32 kernel's plans are no
// input, as kc64_chamfer takes its own arg-mins.
// Structure: kd_sweeps' and kd_combine's.  Grid (samples, H, 3), one 512-thread workgroup per sub-problem (z = 0 cross, 1 p-p,
// 2 q-q), kt_parts' (output, part) mapping, ascending-index sums, then the xor butterfly, then the waves in order; Jacobi
// ping-pong for the self problems; no atomics, no trip count that depends on a value; PARTS and every summation order a function
// of the two counts alone.  LDS (static, 56 KB of the 64 KB limit): p as three double arrays 24 KB, q as float4 16 KB, the two
// dual arrays 16 KB.  The cross block uses all of it; the p-p block p's doubles, the q-q block q's floats.  At most 1024 points a
// cloud, the fp32 call's limit.
// CHUNKS.  The trainer runs samples [b_off, b_off + gridDim.x) of a batch of B: p, the gradient and the two scratch buffers are
// the chunk's; q, the counts, eps, the terms and the certificates are the batch's (as Kc64Args).
// UNBALANCED (kd64_sweeps_unbalanced, kd64_combine_unbalanced; include/drp.h: drp_cloud_divergence_unbalanced_f64).  k_divergence.h's
// relaxation, by its method: the same bodies instantiated a second time with UNBAL.  lambda = rho / (rho + eps) multiplies every
// sweep's soft minimum (kd64_half_sweep's DAMPED), the self problems use the cloud's own mass (a = 1 / n_p, b = w / n_q), the value
// sums are of -expm1(-dual / rho) and kd64_combine_unbalanced multiplies by rho + eps / 2, the certificates compare against
// mass exp(-dual / rho), and transported = sum_i a exp(-f_i / rho) is one more output.  kd_reach, kd_value_term and kd_marginal are
// k_divergence.h's: double already.  rho, mass_q and transported are the BATCH's ([B], [H][B], [H][B]: bb and oslot below, never
// the chunk's slot).  rho = +inf with w = 1: x 1.0 and exp(-0) are exact, so every output has the balanced kernels' bits.
#pragma once
#include "k_divergence.h"

// a cloud in LDS: p's doubles, or q's floats widened at the read
struct Kd64PtsD {
    const double *x, *y, *z;
    __device__ __forceinline__ void get(int i, double& X, double& Y, double& Z) const { X = x[i]; Y = y[i]; Z = z[i]; }
};
struct Kd64PtsF {
    const float4* v;
    __device__ __forceinline__ void get(int i, double& X, double& Y, double& Z) const {
        const float4 r = v[i];
        X = (double)r.x; Y = (double)r.y; Z = (double)r.z;
    }
};

struct Kd64Args {
    const double* pred;         // p's rows (cp's strides): the chunk's
    CloudPair cp;               // q and the counts are the batch's: sample b_off + b
    int b_off;                  // the chunk's first sample (the one-shot: 0)
    int B;                      // samples of the batch: the stride of terms, col_err and self_err
    const double* eps;          // [B], the batch's
    int iters;
    double scale;
    double* vals;               // scratch [3][H][gridDim.x]: sum a f + sum b g | sum a h^p | sum b h^q
    double* gsum;               // scratch [2][H][gridDim.x][N][3]: sum_j P_ij (p_i - q_j) | sum_j S^p_ij (p_i - p_j); null: no gradient
    double* grad;               // [H][gridDim.x][N][3], every row written (padded rows +0.0); null with gsum
    double* terms;              // [H][B]
    double* dual;               // [gridDim.x][2N + 2M]: f, g, h^p, h^q (0 on padding), nullable; the one-shot only
    double* col_err;            // [H][B], nullable
    double* self_err;           // [H][B][2], nullable
    const double* rho;          // unbalanced: [B], the reach (+inf: balanced), the batch's; else null
    const double* mass_q;       // unbalanced: [H][B], the target cloud's total mass w, the batch's; else null
    double* transported;        // unbalanced: [H][B], the batch's, nullable
};

// kt_half_sweep on double costs: out_dual[j] = -eps LSE_i((in_dual[i] - C_ij) / eps + log_mass) for every j < n_out; AVERAGE and
// DAMPED (lambda x the soft minimum: one multiply per output) as there
template <bool AVERAGE, bool DAMPED, typename OV, typename IV>
__device__ __forceinline__ void kd64_half_sweep(const OV out_pts, int n_out, const IV in_pts, int n_in, const double* in_dual,
                                                double* out_dual, double eps, double log_mass, double lambda) {
    const int lp = kt_parts(n_out, n_in), parts = 1 << lp, items = n_out << lp;
    const double ninf = -(double)__builtin_inff();
    for (int e0 = 0; e0 < items; e0 += KT_THREADS) {
        const int e = e0 + (int)threadIdx.x;
        const int j = e >> lp, s = e & (parts - 1);
        const bool live = j < n_out;
        double ox, oy, oz;
        out_pts.get(live ? j : 0, ox, oy, oz);
        double top = ninf;
        for (int i = s; i < n_in; i += parts) {
            double x, y, z;
            in_pts.get(i, x, y, z);
            const double dx = x - ox, dy = y - oy, dz = z - oz;
            const double d = in_dual[i] - (dx * dx + dy * dy + dz * dz);
            top = d > top ? d : top;
        }
        top = kt_group_max(top, lp);
        const double m = top / eps + log_mass;
        double sum = 0.0;
#pragma unroll KT_UNROLL
        for (int i = s; i < n_in; i += parts) {
            double x, y, z;
            in_pts.get(i, x, y, z);
            const double dx = x - ox, dy = y - oy, dz = z - oz;
            const double v = (in_dual[i] - (dx * dx + dy * dy + dz * dz)) / eps + log_mass;
            sum += exp(v - m);
        }
        sum = kt_group_sum(sum, lp);
        if (live && s == 0) {
            const double u = -eps * (m + log(sum));
            const double v = DAMPED ? lambda * u : u;
            out_dual[j] = AVERAGE ? 0.5 * (in_dual[j] + v) : v;
        }
    }
}

// The plan w exp((d_out_i + d_in_j - C_ij) / eps) row by row of the `out` cloud: with gs the row's sum_j plan_ij (out_i - in_j)
// into gs[i][3]; returns this thread's share of sum_i |sum_j plan_ij - target| (the rows it owns), the target the row's mass or
// with UNBAL what the penalty leaves of it (kd_marginal).  n_out = 0: nothing runs.
template <bool UNBAL, typename OV, typename IV>
__device__ __forceinline__ double kd64_plan_rows(const OV out_pts, int n_out, const IV in_pts, int n_in, const double* d_out,
                                                 const double* d_in, double w, double eps, double target, const KdReach& R,
                                                 double* gs) {
    double err = 0.0;
    const int lp = kt_parts(n_out, n_in), parts = 1 << lp, items = n_out << lp;
    for (int e0 = 0; e0 < items; e0 += KT_THREADS) {
        const int e = e0 + (int)threadIdx.x;
        const int i = e >> lp, s = e & (parts - 1);
        const bool live = i < n_out;
        double ox, oy, oz;
        out_pts.get(live ? i : 0, ox, oy, oz);
        const double di = d_out[live ? i : 0];
        double row = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
        for (int j = s; j < n_in; j += parts) {
            double x, y, z;
            in_pts.get(j, x, y, z);
            const double dx = ox - x, dy = oy - y, dz = oz - z;
            const double c = dx * dx + dy * dy + dz * dz;
            const double pij = w * exp((di + d_in[j] - c) / eps);
            row += pij;
            sx += pij * dx; sy += pij * dy; sz += pij * dz;
        }
        row = kt_group_sum(row, lp);
        if (gs != nullptr) { sx = kt_group_sum(sx, lp); sy = kt_group_sum(sy, lp); sz = kt_group_sum(sz, lp); }
        if (live && s == 0) {
            err += fabs(row - kd_marginal<UNBAL>(target, di, R));
            if (gs != nullptr) { gs[(size_t)i * 3] = sx; gs[(size_t)i * 3 + 1] = sy; gs[(size_t)i * 3 + 2] = sz; }
        }
    }
    return err;
}

// the self problem of one cloud already in LDS: the averaged Jacobi sweeps between h0 and h1, h's sum, the symmetric plan's rows
// against the cloud itself (gs: p's only) and self_err.  total_mass: the cloud's (1, or the unbalanced target's w)
template <bool UNBAL, typename V>
__device__ __forceinline__ void kd64_self(const V pts, int n, int len, bool empty, int iters, double eps, double* h0, double* h1,
                                          double* s_w, double* val_out, double* dual /* nullable */, double* gs /* nullable */,
                                          double* err_out /* nullable */, const KdReach& R, double total_mass) {
    const int tid = threadIdx.x;
    for (int e = tid; e < n; e += KT_THREADS) h0[e] = 0.0;
    __syncthreads();
    const double mass = empty ? 0.0 : (UNBAL ? total_mass : 1.0) / (double)n;
    const double log_m = log(mass);
    double* cur = h0;
    double* nxt = h1;
    for (int k = 0; k < iters; ++k) {
        kd64_half_sweep<true, UNBAL>(pts, n, pts, n, cur, nxt, eps, log_m, R.lambda);
        __syncthreads();
        double* const sw = cur; cur = nxt; nxt = sw;
    }
    double acc = 0.0;
    if (!empty)
        for (int e = tid; e < n; e += KT_THREADS) acc += mass * kd_value_term<UNBAL>(cur[e], R);
    const double total = kt_block_sum(acc, s_w);
    if (tid == 0) *val_out = total;
    if (dual != nullptr)
        for (int e = tid; e < len; e += KT_THREADS) dual[e] = (!empty && e < n) ? cur[e] : 0.0;
    if (gs == nullptr && err_out == nullptr) return;
    const double err = kd64_plan_rows<UNBAL>(pts, empty ? 0 : n, pts, n, cur, cur, mass * mass, eps, mass, R, gs);
    if (err_out != nullptr) {
        const double sum = kt_block_sum(err, s_w);
        if (tid == 0) *err_out = sum;
    }
}

template <bool UNBAL>
__device__ __forceinline__ void kd64_sweeps_body(const Kd64Args& A) {
    __shared__ double s_px[KT_MAX_POINTS];      // p, by coordinate (cross and p-p)
    __shared__ double s_py[KT_MAX_POINTS];
    __shared__ double s_pz[KT_MAX_POINTS];
    __shared__ float4 s_q[KT_MAX_POINTS];       // q (cross and q-q)
    __shared__ double s_f[KT_MAX_POINTS];       // cross: f; self: h of the even sweeps
    __shared__ double s_g[KT_MAX_POINTS];       // cross: g; self: h of the odd sweeps
    __shared__ double s_w[KT_WAVES];
    const int b = blockIdx.x, t = blockIdx.y, z = blockIdx.z, nb = gridDim.x;
    const int tid = threadIdx.x;
    const int N = A.cp.N, M = A.cp.M;
    const int bb = A.b_off + b;                             // the sample in the batch's arrays
    const int np = A.cp.count_p(bb, KT_MAX_POINTS), nq = A.cp.count_q(bb, t, KT_MAX_POINTS);
    const double* p = A.cp.p_rows(A.pred, b, t);
    const float* q = A.cp.q_rows(bb, t);
    const size_t slot = (size_t)t * nb + b, slots = (size_t)gridDim.y * nb;     // of the launch's own buffers
    const size_t oslot = (size_t)t * A.B + bb;                                  // of the batch's outputs
    const bool empty = np == 0 || nq == 0;                  // (the entry points refuse it)
    const int iters = empty ? 0 : min(max(A.iters, 0), KT_MAX_ITERS);
    const double eps = A.eps[bb];
    KdReach R{};
    double w = 1.0;
    if (UNBAL) {
        R = kd_reach(A.rho[bb], eps);
        w = A.mass_q[oslot];
    }
    double* dual = A.dual != nullptr ? A.dual + slot * (2 * ((size_t)N + M)) : nullptr;
    const Kd64PtsD P{s_px, s_py, s_pz};
    const Kd64PtsF Q{s_q};
    if (z != 2)
        for (int e = tid; e < np; e += KT_THREADS) { s_px[e] = p[(size_t)e * 3]; s_py[e] = p[(size_t)e * 3 + 1]; s_pz[e] = p[(size_t)e * 3 + 2]; }
    if (z != 1)
        for (int e = tid; e < nq; e += KT_THREADS) s_q[e] = make_float4(q[(size_t)e * 3], q[(size_t)e * 3 + 1], q[(size_t)e * 3 + 2], 0.0f);
    if (z == 1) {
        kd64_self<UNBAL>(P, np, N, empty, iters, eps, s_f, s_g, s_w, A.vals + slots + slot, dual != nullptr ? dual + N + M : nullptr,
                         A.gsum != nullptr ? A.gsum + (slots + slot) * N * 3 : nullptr, A.self_err != nullptr ? A.self_err + oslot * 2 : nullptr,
                         R, 1.0);
        return;
    }
    if (z == 2) {
        kd64_self<UNBAL>(Q, nq, M, empty, iters, eps, s_f, s_g, s_w, A.vals + 2 * slots + slot,
                         dual != nullptr ? dual + 2 * (size_t)N + M : nullptr, (double*)nullptr,
                         A.self_err != nullptr ? A.self_err + oslot * 2 + 1 : nullptr, R, w);
        return;
    }
    // z = 0: the cross problem -- kt_transport's sweeps; behind them the duals' sum, the plan's rows against q, col_err
    for (int e = tid; e < np; e += KT_THREADS) s_f[e] = 0.0;
    for (int e = tid; e < nq; e += KT_THREADS) s_g[e] = 0.0;
    __syncthreads();
    const double mass_p = empty ? 0.0 : 1.0 / (double)np, mass_q = empty ? 0.0 : (UNBAL ? w : 1.0) / (double)nq;
    const double log_a = log(mass_p), log_b = log(mass_q);
    for (int k = 0; k < iters; ++k) {
        kd64_half_sweep<false, UNBAL>(Q, nq, P, np, s_f, s_g, eps, log_a, R.lambda);
        __syncthreads();
        kd64_half_sweep<false, UNBAL>(P, np, Q, nq, s_g, s_f, eps, log_b, R.lambda);
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
        if (tid == 0) A.transported[oslot] = sum;
    }
    if (dual != nullptr) {
        for (int e = tid; e < N; e += KT_THREADS) dual[e] = (!empty && e < np) ? s_f[e] : 0.0;
        for (int e = tid; e < M; e += KT_THREADS) dual[(size_t)N + e] = (!empty && e < nq) ? s_g[e] : 0.0;
    }
    const double ab = mass_p * mass_q;
    if (A.gsum != nullptr) (void)kd64_plan_rows<UNBAL>(P, empty ? 0 : np, Q, nq, s_f, s_g, ab, eps, mass_p, R, A.gsum + slot * N * 3);
    if (A.col_err != nullptr) {
        const double err = kd64_plan_rows<UNBAL>(Q, empty ? 0 : nq, P, np, s_g, s_f, ab, eps, mass_q, R, (double*)nullptr);
        const double sum = kt_block_sum(err, s_w);
        if (tid == 0) A.col_err[oslot] = sum;
    }
}

__global__ void __launch_bounds__(KT_THREADS) kd64_sweeps(Kd64Args A) { kd64_sweeps_body<false>(A); }
__global__ void __launch_bounds__(KT_THREADS) kd64_sweeps_unbalanced(Kd64Args A) { kd64_sweeps_body<true>(A); }

// behind kd64_sweeps in the stream, grid (samples, H): the gradient from the two sums, the zero padding, the term
template <bool UNBAL>
__device__ __forceinline__ void kd64_combine_body(const Kd64Args& A) {
    const int b = blockIdx.x, t = blockIdx.y, nb = gridDim.x;
    const int tid = threadIdx.x;
    const int N = A.cp.N;
    const int bb = A.b_off + b;
    const int np = A.cp.count_p(bb, KT_MAX_POINTS), nq = A.cp.count_q(bb, t, KT_MAX_POINTS);
    const bool empty = np == 0 || nq == 0;
    const size_t slot = (size_t)t * nb + b, slots = (size_t)gridDim.y * nb;
    if (A.grad != nullptr && A.gsum != nullptr) {
        const double gscale = 2.0 * A.scale / 3.0;
        const double* cross = A.gsum + slot * N * 3;
        const double* self = A.gsum + (slots + slot) * N * 3;
        double* g = A.grad + slot * N * 3;
        const int real = (empty ? 0 : np) * 3;
        for (int e = tid; e < N * 3; e += KD_COMBINE_THREADS) g[e] = e < real ? gscale * (cross[e] - self[e]) : 0.0;
    }
    if (tid == 0) {
        const double sum = A.vals[slot] - A.vals[slots + slot] - A.vals[2 * slots + slot];
        const KdReach R = UNBAL ? kd_reach(A.rho[bb], A.eps[bb]) : KdReach{};
        if (UNBAL && !R.balanced) A.terms[(size_t)t * A.B + bb] = A.scale * (((R.rho + 0.5 * A.eps[bb]) * sum) / 3.0);
        else A.terms[(size_t)t * A.B + bb] = A.scale * (sum / 3.0);
    }
}
__global__ void __launch_bounds__(KD_COMBINE_THREADS) kd64_combine(Kd64Args A) { kd64_combine_body<false>(A); }
__global__ void __launch_bounds__(KD_COMBINE_THREADS) kd64_combine_unbalanced(Kd64Args A) { kd64_combine_body<true>(A); }
