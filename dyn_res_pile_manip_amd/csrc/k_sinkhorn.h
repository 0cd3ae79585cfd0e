// k_sinkhorn.h -- the Sinkhorn losses of two padded cloud batches and their gradients: the entropy-regularised
// transport distance, the Sinkhorn divergence, its unbalanced relaxation, and the float64 yardsticks of the last two.  ONE body
// each for the half-sweep, the plan's rows, the cross problem, the self problem and the combine; what differs between the
// kernels is a points view (how C_ij is formed), three compile-time flags and which outputs a caller asks for.
//
// THE DEFINITIONS.  n_p, n_q real rows; eps > 0 in squared-distance units, per sample; K = iters sweeps; a = 1 / n_p, b = 1 / n_q.
//   C[i][j] = |p_i - q_j|^2     fp32 kernels: fp32 differences, dx*dx + dy*dy + dz*dz in fp32 as kc_chamfer forms it (no fused
//             multiply-add), widened to double exactly; everything behind it is double.  float64 kernels: p the caller's doubles
//             (in the trainer the float64 tape's predicted state), q the caller's floats widened where they are read, the
//             differences and the same expression in double -- of p - q, p - p and q - q alike, so the plans carry every bit of
//             the float64 prediction and the fp32 kernel's plans are no input (as kc64_chamfer takes its own arg-mins)
//   cross problem   f = 0; K times   g_j = -eps LSE_i((f_i - C_ij) / eps + log a),  then  f_i = -eps LSE_j((g_j - C_ij) / eps + log b)
//             (LSE max-shifted: m = max x, m + log sum exp(x - m));  P_ij = a b exp((f_i + g_j - C_ij) / eps): the last update is
//             f's, so its row sums are a to rounding -- every predicted particle's whole mass is placed
//   self problem of a cloud x with n rows, m = 1 / n:  h = 0; K times, for every j from the PREVIOUS sweep's h (Jacobi, two arrays):
//             h_j <- (h_j + (-eps LSE_i((h_i - C^xx_ij) / eps + log m))) / 2;   S_ij = m^2 exp((h_i + h_j - C^xx_ij) / eps)
//             -- symmetric by construction, one half-sweep a sweep
//   TRANSPORT (kt_transport; the loss that sees density AND gives every real row a gradient whatever the two counts are -- the
//             matching of k_match.h leaves the larger cloud's surplus rows out):
//             transport = scale sum_ij P_ij C_ij / 3;   d/dp_i = scale sum_j P_ij 2 (p_i - q_j) / 3
//   DIVERGENCE (kd_sweeps + kd_combine; the transport loss with its entropic bias taken out: the cloud that minimises the
//             entropy-regularised cost over p is a shrunken copy of q;  S(p, q) = OT(p, q) - OT(p, p) / 2 - OT(q, q) / 2 on the dual
//             values is non-negative and zero only for equal clouds):
//             divergence = scale (sum_i a f_i + sum_j b g_j - sum_i a h^p_i - sum_j b h^q_j) / 3      (the dual form, not clamped)
//             d/dp_i     = (2 scale / 3) (sum_j P_ij (p_i - q_j) - sum_j S^p_ij (p_i - p_j))
//   the gradients: P, S constants of the derivative; the differences widened (fp32) or double, the sums in double; fp32 kernels
//             round the result once to fp32, the float64 ones never; +0.0 on padding
//   col_err  = sum_j |sum_i P_ij - b|: the column-marginal violation K sweeps leave -- an output, not a stopping rule;
//   self_err = [sum_i |sum_j S^p_ij - a|, sum_j |sum_i S^q_ij - b|]
//   UNBALANCED (kd_sweeps_unbalanced, kd_combine<., true>, kd64_*_unbalanced; include/drp.h: drp_cloud_divergence_unbalanced).  Each
//             marginal is held by a KL penalty of weight rho (the reach, in eps's unit) in place of the hard constraint, and the
//             target cloud carries total mass w: a = 1 / n_p, b = w / n_q, lambda = rho / (rho + eps).  Every sweep's soft minimum
//             is multiplied by lambda (DAMPED: one multiply per output), the self problems' mass is the cloud's own, and
//             divergence = scale (rho + eps / 2) (sum_i a (expm1(-h^p_i / rho) - expm1(-f_i / rho)) + sum_j b (expm1(-h^q_j / rho) - expm1(-g_j / rho))) / 3
//             col_err    = sum_j |sum_i P_ij - b exp(-g_j / rho)|;  self_err likewise against m exp(-h / rho);  the gradient's expression is the same
//             transported = sum_i a exp(-f_i / rho): the plan's total mass (its rows sum to a exp(-f_i / rho) exactly behind f's update)
//             rho = +inf (with w = 1): lambda = 1 and the balanced value -- x 1.0 and exp(-0) are exact, so every output has the
//             balanced kernel's bits.
//
// THE MAPPING.  One workgroup of 512 threads per problem.  A half-sweep has one log-sum-exp per row of the cloud it updates (an
// "output"), over the rows of the other cloud (the "terms").  Each output is shared by PARTS = 2^lp adjacent lanes of one
// wavefront (kt_parts: the smallest power of two that gives the workgroup at least KT_MIN_ITEMS (output, part) items, at most 64
// and no more than the terms can occupy): part s takes the terms s, s + PARTS, ... in ascending index, first for the maximum of
// f_i - C_ij (division by eps > 0 and the added constant are monotonic: the maximum of x is x at that term), then for the sum of
// exp(x - m); the parts are combined by an xor butterfly over the lane offsets PARTS/2 .. 1 (a + b is b + a bit for bit: every
// lane of the group ends with the same value).  Items are dealt to threads in ascending order, 512 at a time.  So a 20 x 20
// problem runs 20 x 64 = 1 280 items in 3 rounds (83 % of the thread slots busy), not 20 threads for the whole sweep.  PARTS and
// with it the order of every sum is a function of the two COUNTS alone: the bits do not depend on the padded N, M, on B or on
// another sample.  No atomics.  The cost matrix is never stored: each half-sweep forms it again from LDS.  One barrier separates
// the half-sweeps.  NO VALUE PROLONGS A LOOP: every trip count is fixed by K, n_p and n_q.  A non-finite coordinate (a diverged
// model) ends in a NaN term after the same number of steps.
// THE GRIDS.  kt_transport: (B, H), the cross problem alone.  The divergence's three sub-problems are independent chains of K
// dependent sweeps: k*_sweeps run them as grid (samples, H, 3) (z = 0 cross, 1 p-p, 2 q-q).  What the blocks of one problem must
// share goes through a double scratch buffer: the three value sums, and the two gradient sums per row [2][H][samples][N][3].
// k*_combine, grid (samples, H), follows in the stream: the gradient from the double difference, the zero padding, the term, and
// in the fp32 trainer the zero-fill of the gradient blob (train_zero_fill: this launch alone does it, on the grid the other loss
// kernels do it on).  The duals and the certificates are each written by the one block that owns them.
// LDS (static).  fp32: both clouds as float4 and the two dual arrays as double, 16 + 16 + 8 + 8 KB, three problems (24
// wavefronts) a CU.  float64 (56 KB of the 64 KB limit): p as three double arrays 24 KB, q as float4 16 KB, the duals 16 KB; the
// cross block uses all of it, the p-p block p's doubles, the q-q block q's floats.  At most 1024 points a cloud.
// CHUNKS.  The float64 trainer runs samples [b_off, b_off + gridDim.x) of a batch of B: p, the gradient, the duals and the two
// scratch buffers are the launch's (slot); q, the counts, eps, rho, mass_q, the terms, the certificates and transported are the
// batch's (sample bb = b_off + b, oslot).  Every other caller passes b_off = 0 and B = gridDim.x: the two slots are one.
#pragma once
#include "k_cloud_pair.h"

#define KT_THREADS 512          // two waves a SIMD: the exponentials' dependent chains overlap (DESIGN.md 9 has the sizes tried)
#define KT_WAVES (KT_THREADS / 64)
#define KT_UNROLL 4             // the sum's loop: four independent exponentials in flight, added in the same ascending order
#define KT_MAX_POINTS 1024      // per cloud: the work is K n_p n_q exponentials
#define KT_MAX_ITERS 1000
#define KT_MIN_ITEMS 1024       // (output, part) items a pass aims for: two rounds of the workgroup
#define KD_COMBINE_THREADS 256

// P: p's scalar; G: the gradient's.  (float, float): kt_transport and the kd_* kernels; (double, double): the kd64_* kernels
template <typename P, typename G>
struct SkArgs {
    const P* pred;              // p's rows (cp's strides): the launch's
    CloudPair cp;               // q and the counts are the batch's: sample b_off + b
    int b_off;                  // the launch's first sample in the batch (all but the float64 trainer: 0)
    int B;                      // samples of the batch: the stride of terms, the certificates, mass_q and transported
    const double* eps;          // [B]
    int iters;
    double scale;
    double* vals;               // divergence: scratch [3][H][gridDim.x]: sum a f + sum b g | sum a h^p | sum b h^q  (unbalanced: of -expm1(-. / rho))
    double* gsum;               // divergence: scratch [2][H][gridDim.x][N][3]: sum_j P_ij (p_i - q_j) | sum_j S^p_ij (p_i - p_j), real rows; null: no gradient
    G* grad;                    // [H][gridDim.x][N][3], every row written (padded rows +0.0); nullable (divergence: null with gsum)
    double* terms;              // [H][B]
    double* dual;               // the one-shots only, nullable (0 on padding).  transport: [gridDim.x][N + M]: f, g; divergence: [gridDim.x][2N + 2M]: f, g, h^p, h^q
    double* col_err;            // [H][B], nullable: the pass over the columns runs only where it is asked for
    double* self_err;           // divergence: [H][B][2], nullable
    float* zero; size_t n_zero; // the fp32 trainer, nullable: filled with 0 by kt_transport<true> / kd_combine<true> (the gradient blob and
                                // kmb_step_bwd's counters, as kt_mse_grad does)
    const double* rho;          // unbalanced: [B], the reach (+inf: balanced); else null
    const double* mass_q;       // unbalanced: [H][B], the target cloud's total mass w; else null
    double* transported;        // unbalanced: [H][B], nullable
};
using SkArgs32 = SkArgs<float, float>;
using SkArgs64 = SkArgs<double, double>;

// log2 of the lanes that share one output's sum: by the counts alone
__device__ __forceinline__ int kt_parts(int n_out, int n_terms) {
    int lp = 0;
    while (lp < 6 && (n_out << lp) < KT_MIN_ITEMS && (1 << lp) < n_terms) ++lp;
    return lp;
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

// ---- a cloud in LDS and the cost between two of its points: the one place where the fp32 and the float64 kernels differ ----
// sk_diff(a, b, ...): the differences a - b by coordinate as doubles, and |a - b|^2 ((a - b)^2 is (b - a)^2 bit for bit)
struct SkD3 { double x, y, z; };
struct SkPts32 {                    // fp32 kernels: either cloud
    const float4* v;
    __device__ __forceinline__ float4 get(int i) const { return v[i]; }
};
struct SkPts64D {                   // float64 kernels: p's doubles, by coordinate
    const double *x, *y, *z;
    __device__ __forceinline__ SkD3 get(int i) const { return SkD3{x[i], y[i], z[i]}; }
};
struct SkPts64F {                   // float64 kernels: q's floats, widened at the read
    const float4* v;
    __device__ __forceinline__ SkD3 get(int i) const {
        const float4 r = v[i];
        return SkD3{(double)r.x, (double)r.y, (double)r.z};
    }
};
__device__ __forceinline__ double sk_diff(const float4 a, const float4 b, double& dx, double& dy, double& dz) {
    const float fx = a.x - b.x, fy = a.y - b.y, fz = a.z - b.z;     // in fp32, then widened exactly
    dx = (double)fx; dy = (double)fy; dz = (double)fz;
    return (double)(fx * fx + fy * fy + fz * fz);
}
__device__ __forceinline__ double sk_diff(const SkD3 a, const SkD3 b, double& dx, double& dy, double& dz) {
    dx = a.x - b.x; dy = a.y - b.y; dz = a.z - b.z;
    return dx * dx + dy * dy + dz * dz;
}
__device__ __forceinline__ void sk_load(float4* dst, const float* rows, int n) {
    for (int e = threadIdx.x; e < n; e += KT_THREADS) dst[e] = make_float4(rows[(size_t)e * 3], rows[(size_t)e * 3 + 1], rows[(size_t)e * 3 + 2], 0.0f);
}

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
// a dual's share of the value: the dual itself, or with a finite reach -expm1(-dual / rho) (sk_combine multiplies by rho + eps / 2)
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

// out_dual[j] = -eps LSE_i((in_dual[i] - C_ij) / eps + log_mass) for every j < n_out; the caller's barrier is behind it.
// AVERAGE (the self problems, both clouds the same one): out_dual[j] = (in_dual[j] + that) / 2
// DAMPED (the unbalanced problems): `that` is lambda x the soft minimum -- one multiply per output, nothing per term
template <bool AVERAGE, bool DAMPED, typename OV, typename IV>
__device__ __forceinline__ void sk_half_sweep(const OV out_pts, int n_out, const IV in_pts, int n_in, const double* in_dual,
                                              double* out_dual, double eps, double log_mass, double lambda) {
    const int lp = kt_parts(n_out, n_in), parts = 1 << lp, items = n_out << lp;
    const double ninf = -(double)__builtin_inff();
    double dx, dy, dz;                                      // (unused here: in - out)
    for (int e0 = 0; e0 < items; e0 += KT_THREADS) {
        const int e = e0 + (int)threadIdx.x;
        const int j = e >> lp, s = e & (parts - 1);
        const bool live = j < n_out;
        const auto o = out_pts.get(live ? j : 0);
        double top = ninf;
        for (int i = s; i < n_in; i += parts) {
            const double d = in_dual[i] - sk_diff(in_pts.get(i), o, dx, dy, dz);
            top = d > top ? d : top;
        }
        top = kt_group_max(top, lp);
        const double m = top / eps + log_mass;
        double sum = 0.0;
#pragma unroll KT_UNROLL
        for (int i = s; i < n_in; i += parts) {
            const double x = (in_dual[i] - sk_diff(in_pts.get(i), o, dx, dy, dz)) / eps + log_mass;
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

// what a pass over the plan's rows sums per row besides the gradient: nothing, the row itself (for |row - marginal|), or plan x cost
enum SkRow { SK_ROW_NONE, SK_ROW_ERR, SK_ROW_COST };
// a row's three gradient sums out: the divergence keeps the doubles (sk_combine scales their difference); kt_transport rounds
// gscale x the sum once to fp32
__device__ __forceinline__ void sk_store_row(double* g, double, double sx, double sy, double sz) { g[0] = sx; g[1] = sy; g[2] = sz; }
__device__ __forceinline__ void sk_store_row(float* g, double gscale, double sx, double sy, double sz) {
    g[0] = (float)(gscale * sx); g[1] = (float)(gscale * sy); g[2] = (float)(gscale * sz);
}

// The plan w exp((d_out_i + d_in_j - C_ij) / eps) row by row of the `out` cloud: with gs the row's sum_j plan_ij (out_i - in_j)
// into gs[i][3]; returns this thread's share (the rows it owns) of sum_i |sum_j plan_ij - target| (SK_ROW_ERR: the target the
// row's mass or with UNBAL what the penalty leaves of it, kd_marginal), of sum_ij plan_ij C_ij (SK_ROW_COST), or 0.
// n_out = 0: nothing runs.
template <bool UNBAL, SkRow ROW, typename OV, typename IV, typename GS>
__device__ __forceinline__ double sk_plan_rows(const OV out_pts, int n_out, const IV in_pts, int n_in, const double* d_out,
                                               const double* d_in, double w, double eps, double target, const KdReach& R,
                                               GS* gs /* nullable */, double gscale) {
    double ret = 0.0;
    const int lp = kt_parts(n_out, n_in), parts = 1 << lp, items = n_out << lp;
    for (int e0 = 0; e0 < items; e0 += KT_THREADS) {
        const int e = e0 + (int)threadIdx.x;
        const int i = e >> lp, s = e & (parts - 1);
        const bool live = i < n_out;
        const auto o = out_pts.get(live ? i : 0);
        const double di = d_out[live ? i : 0];
        double row = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
        for (int j = s; j < n_in; j += parts) {
            double dx, dy, dz;
            const double c = sk_diff(o, in_pts.get(j), dx, dy, dz);     // out - in: the gradient's sign
            const double pij = w * exp((di + d_in[j] - c) / eps);
            if (ROW == SK_ROW_ERR) row += pij;
            if (ROW == SK_ROW_COST) row += pij * c;
            sx += pij * dx; sy += pij * dy; sz += pij * dz;
        }
        if (ROW != SK_ROW_NONE) row = kt_group_sum(row, lp);
        if (gs != nullptr) { sx = kt_group_sum(sx, lp); sy = kt_group_sum(sy, lp); sz = kt_group_sum(sz, lp); }
        if (live && s == 0) {
            if (ROW == SK_ROW_ERR) ret += fabs(row - kd_marginal<UNBAL>(target, di, R));
            if (ROW == SK_ROW_COST) ret += row;
            if (gs != nullptr) sk_store_row(gs + (size_t)i * 3, gscale, sx, sy, sz);
        }
    }
    return ret;
}

// what every block of a launch works out first: its sample, the two counts, the rows, its slots and the sample's parameters
template <typename P>
struct SkProblem {
    int np, nq;
    const P* rows_p;
    const float* rows_q;
    size_t slot, slots;         // (step, sample) in the launch's own buffers, and their number
    size_t oslot;               // in the batch's outputs
    bool empty;                 // (the entry points refuse it)
    int iters;
    double eps, w;
    KdReach R;
};
template <bool UNBAL, typename P, typename G>
__device__ __forceinline__ SkProblem<P> sk_problem(const SkArgs<P, G>& A) {
    const int b = blockIdx.x, t = blockIdx.y, nb = gridDim.x;
    const int bb = A.b_off + b;                             // the sample in the batch's arrays
    SkProblem<P> pr;
    pr.np = A.cp.count_p(bb, KT_MAX_POINTS); pr.nq = A.cp.count_q(bb, t, KT_MAX_POINTS);
    pr.rows_p = A.cp.p_rows(A.pred, b, t);
    pr.rows_q = A.cp.q_rows(bb, t);
    pr.slot = (size_t)t * nb + b; pr.slots = (size_t)gridDim.y * nb;
    pr.oslot = (size_t)t * A.B + bb;
    pr.empty = pr.np == 0 || pr.nq == 0;
    pr.iters = pr.empty ? 0 : min(max(A.iters, 0), KT_MAX_ITERS);
    pr.eps = A.eps[bb];
    pr.R = KdReach{};
    pr.w = 1.0;
    if (UNBAL) {
        pr.R = kd_reach(A.rho[bb], pr.eps);
        pr.w = A.mass_q[pr.oslot];
    }
    return pr;
}

// The cross problem of two clouds already in LDS: f = g = 0, the K sweeps, then the plan's rows and what hangs on them.
// The problem's value sum: sum_i a v(f_i) + sum_j b v(g_j) (kd_value_term) written to *val_out at once (the passes behind it
// need every register), or with PRIMAL (kt_transport) sum_ij P_ij C_ij returned, valid in every thread.  gs: the rows'
// gradient sums against q (sk_store_row), dual: f [N] then g [M], col_err, transported: each nullable, each pass run only where
// it is asked for
template <bool UNBAL, bool PRIMAL, typename P, typename PV, typename QV, typename GS>
__device__ __forceinline__ double sk_cross_problem(const SkProblem<P>& pr, int N, int M, const PV p_pts, const QV q_pts, double* s_f,
                                                   double* s_g, double* s_w, double* val_out, double* dual, GS* gs, double gscale,
                                                   double* col_err, double* transported) {
    const int tid = threadIdx.x;
    const int np = pr.np, nq = pr.nq;
    const bool empty = pr.empty;
    const double eps = pr.eps;
    for (int e = tid; e < np; e += KT_THREADS) s_f[e] = 0.0;
    for (int e = tid; e < nq; e += KT_THREADS) s_g[e] = 0.0;
    __syncthreads();
    const double mass_p = empty ? 0.0 : 1.0 / (double)np, mass_q = empty ? 0.0 : (UNBAL ? pr.w : 1.0) / (double)nq;
    const double log_a = log(mass_p), log_b = log(mass_q);
    for (int k = 0; k < pr.iters; ++k) {
        sk_half_sweep<false, UNBAL>(q_pts, nq, p_pts, np, s_f, s_g, eps, log_a, pr.R.lambda);
        __syncthreads();
        sk_half_sweep<false, UNBAL>(p_pts, np, q_pts, nq, s_g, s_f, eps, log_b, pr.R.lambda);
        __syncthreads();
    }
    const double ab = mass_p * mass_q;
    double acc = 0.0;
    if (PRIMAL) {
        acc = sk_plan_rows<UNBAL, SK_ROW_COST>(p_pts, empty ? 0 : np, q_pts, nq, s_f, s_g, ab, eps, mass_p, pr.R, gs, gscale);
    } else if (!empty) {
        for (int e = tid; e < np; e += KT_THREADS) acc += mass_p * kd_value_term<UNBAL>(s_f[e], pr.R);
        for (int e = tid; e < nq; e += KT_THREADS) acc += mass_q * kd_value_term<UNBAL>(s_g[e], pr.R);
    }
    const double total = kt_block_sum(acc, s_w);
    if (!PRIMAL && tid == 0) *val_out = total;
    if (UNBAL && transported != nullptr) {
        double moved = 0.0;
        if (!empty)
            for (int e = tid; e < np; e += KT_THREADS) moved += kd_marginal<UNBAL>(mass_p, s_f[e], pr.R);
        const double sum = kt_block_sum(moved, s_w);
        if (tid == 0) *transported = sum;
    }
    if (dual != nullptr) {
        for (int e = tid; e < N; e += KT_THREADS) dual[e] = (!empty && e < np) ? s_f[e] : 0.0;
        for (int e = tid; e < M; e += KT_THREADS) dual[(size_t)N + e] = (!empty && e < nq) ? s_g[e] : 0.0;
    }
    if (!PRIMAL && gs != nullptr)
        (void)sk_plan_rows<UNBAL, SK_ROW_NONE>(p_pts, empty ? 0 : np, q_pts, nq, s_f, s_g, ab, eps, mass_p, pr.R, gs, gscale);
    if (col_err != nullptr) {       // the plan's columns: what the sweeps left of the column marginals
        const double err = sk_plan_rows<UNBAL, SK_ROW_ERR>(q_pts, empty ? 0 : nq, p_pts, np, s_g, s_f, ab, eps, mass_q, pr.R, (double*)nullptr, 0.0);
        const double sum = kt_block_sum(err, s_w);
        if (tid == 0) *col_err = sum;
    }
    return total;
}

// The self problem of one cloud of n rows already in LDS (row length `len` in the padded batch): the averaged Jacobi sweeps
// between h0 and h1, h's sum, the symmetric plan's rows against the cloud itself (gs, the gradient's second sum: p's only) and
// self_err.  total_mass: the cloud's (1, or the unbalanced target's w)
template <bool UNBAL, typename V>
__device__ __forceinline__ void sk_self_problem(const V pts, int n, int len, bool empty, int iters, double eps, double* h0, double* h1,
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
        sk_half_sweep<true, UNBAL>(pts, n, pts, n, cur, nxt, eps, log_m, R.lambda);
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
    const double err = sk_plan_rows<UNBAL, SK_ROW_ERR>(pts, empty ? 0 : n, pts, n, cur, cur, mass * mass, eps, mass, R, gs, 0.0);
    if (err_out != nullptr) {
        const double sum = kt_block_sum(err, s_w);
        if (tid == 0) *err_out = sum;
    }
}

// a block of the divergence's grid (samples, H, 3) on its clouds in LDS: z = 0 the cross problem, 1 p's self problem, 2 q's
template <bool UNBAL, typename P, typename G, typename PV, typename QV>
__device__ __forceinline__ void sk_divergence_block(const SkArgs<P, G>& A, const SkProblem<P>& pr, const PV p_pts, const QV q_pts,
                                                    double* s_f, double* s_g, double* s_w) {
    const int z = blockIdx.z;
    const int N = A.cp.N, M = A.cp.M;
    const size_t slot = pr.slot, slots = pr.slots;
    double* dual = A.dual != nullptr ? A.dual + slot * (2 * ((size_t)N + M)) : nullptr;
    if (z == 1) {
        sk_self_problem<UNBAL>(p_pts, pr.np, N, pr.empty, pr.iters, pr.eps, s_f, s_g, s_w, A.vals + slots + slot,
                               dual != nullptr ? dual + N + M : nullptr, A.gsum != nullptr ? A.gsum + (slots + slot) * N * 3 : nullptr,
                               A.self_err != nullptr ? A.self_err + pr.oslot * 2 : nullptr, pr.R, 1.0);
    } else if (z == 2) {
        sk_self_problem<UNBAL>(q_pts, pr.nq, M, pr.empty, pr.iters, pr.eps, s_f, s_g, s_w, A.vals + 2 * slots + slot,
                               dual != nullptr ? dual + 2 * (size_t)N + M : nullptr, (double*)nullptr,
                               A.self_err != nullptr ? A.self_err + pr.oslot * 2 + 1 : nullptr, pr.R, pr.w);
    } else {
        (void)sk_cross_problem<UNBAL, false>(pr, N, M, p_pts, q_pts, s_f, s_g, s_w, A.vals + slot, dual,
                                             A.gsum != nullptr ? A.gsum + slot * N * 3 : (double*)nullptr, 0.0,
                                             A.col_err != nullptr ? A.col_err + pr.oslot : nullptr,
                                             A.transported != nullptr ? A.transported + pr.oslot : nullptr);
    }
}

// behind the sweeps in the stream, grid (samples, H): what needs more than one block's results -- the gradient from the two
// sums (T = float: rounded once), the zero padding, the term
template <typename T, bool TRAIN, bool UNBAL>
__device__ __forceinline__ void sk_combine(const SkArgs<T, T>& A) {
    const int b = blockIdx.x, t = blockIdx.y, nb = gridDim.x;
    const int tid = threadIdx.x;
    const int N = A.cp.N;
    if (TRAIN) train_zero_fill(A.zero, A.n_zero, KD_COMBINE_THREADS);
    const int bb = A.b_off + b;
    const int np = A.cp.count_p(bb, KT_MAX_POINTS), nq = A.cp.count_q(bb, t, KT_MAX_POINTS);
    const bool empty = np == 0 || nq == 0;
    const size_t slot = (size_t)t * nb + b, slots = (size_t)gridDim.y * nb;
    if (A.grad != nullptr && A.gsum != nullptr) {
        const double gscale = 2.0 * A.scale / 3.0;
        const double* cross = A.gsum + slot * N * 3;
        const double* self = A.gsum + (slots + slot) * N * 3;
        T* g = A.grad + slot * N * 3;
        const int real = (empty ? 0 : np) * 3;
        for (int e = tid; e < N * 3; e += KD_COMBINE_THREADS) g[e] = e < real ? (T)(gscale * (cross[e] - self[e])) : (T)0;
    }
    if (tid == 0) {
        const double sum = A.vals[slot] - A.vals[slots + slot] - A.vals[2 * slots + slot];
        const KdReach R = UNBAL ? kd_reach(A.rho[bb], A.eps[bb]) : KdReach{};
        double* const term = A.terms + (size_t)t * A.B + bb;
        if (UNBAL && !R.balanced) *term = A.scale * (((R.rho + 0.5 * A.eps[bb]) * sum) / 3.0);
        else *term = A.scale * (sum / 3.0);
    }
}

// ---- the entry points: the LDS of each and its instantiations ----
template <bool TRAIN>
__global__ void __launch_bounds__(KT_THREADS) kt_transport(SkArgs32 A) {
    __shared__ float4 s_p[KT_MAX_POINTS];
    __shared__ float4 s_q[KT_MAX_POINTS];
    __shared__ double s_f[KT_MAX_POINTS];
    __shared__ double s_g[KT_MAX_POINTS];
    __shared__ double s_w[KT_WAVES];
    const int N = A.cp.N, M = A.cp.M;
    if (TRAIN) train_zero_fill(A.zero, A.n_zero, KT_THREADS);
    const SkProblem<float> pr = sk_problem<false>(A);
    sk_load(s_p, pr.rows_p, pr.np);
    sk_load(s_q, pr.rows_q, pr.nq);
    float* g_out = A.grad != nullptr ? A.grad + pr.slot * N * 3 : nullptr;
    double* dual = (!TRAIN && A.dual != nullptr) ? A.dual + pr.slot * ((size_t)N + M) : nullptr;
    const double total = sk_cross_problem<false, true>(pr, N, M, SkPts32{s_p}, SkPts32{s_q}, s_f, s_g, s_w, (double*)nullptr, dual, g_out,
                                                       2.0 * A.scale / 3.0,
                                                       A.col_err != nullptr ? A.col_err + pr.oslot : nullptr, (double*)nullptr);
    if (g_out != nullptr)           // padding: gradient exactly 0
        for (int e = (pr.empty ? 0 : pr.np) * 3 + (int)threadIdx.x; e < N * 3; e += KT_THREADS) g_out[e] = 0.0f;
    if (threadIdx.x == 0) A.terms[pr.oslot] = A.scale * (total / 3.0);
}

template <bool UNBAL>
__device__ __forceinline__ void kd_sweeps_body(const SkArgs32& A) {
    __shared__ float4 s_p[KT_MAX_POINTS];       // p (cross and p-p)
    __shared__ float4 s_q[KT_MAX_POINTS];       // q (cross and q-q)
    __shared__ double s_f[KT_MAX_POINTS];       // cross: f; self: h of the even sweeps
    __shared__ double s_g[KT_MAX_POINTS];       // cross: g; self: h of the odd sweeps
    __shared__ double s_w[KT_WAVES];
    const SkProblem<float> pr = sk_problem<UNBAL>(A);
    if (blockIdx.z != 2) sk_load(s_p, pr.rows_p, pr.np);
    if (blockIdx.z != 1) sk_load(s_q, pr.rows_q, pr.nq);
    sk_divergence_block<UNBAL>(A, pr, SkPts32{s_p}, SkPts32{s_q}, s_f, s_g, s_w);
}
__global__ void __launch_bounds__(KT_THREADS) kd_sweeps(SkArgs32 A) { kd_sweeps_body<false>(A); }
__global__ void __launch_bounds__(KT_THREADS) kd_sweeps_unbalanced(SkArgs32 A) { kd_sweeps_body<true>(A); }
template <bool TRAIN, bool UNBAL = false>
__global__ void __launch_bounds__(KD_COMBINE_THREADS) kd_combine(SkArgs32 A) { sk_combine<float, TRAIN, UNBAL>(A); }

template <bool UNBAL>
__device__ __forceinline__ void kd64_sweeps_body(const SkArgs64& A) {
    __shared__ double s_px[KT_MAX_POINTS];      // p, by coordinate (cross and p-p)
    __shared__ double s_py[KT_MAX_POINTS];
    __shared__ double s_pz[KT_MAX_POINTS];
    __shared__ float4 s_q[KT_MAX_POINTS];       // q (cross and q-q)
    __shared__ double s_f[KT_MAX_POINTS];       // cross: f; self: h of the even sweeps
    __shared__ double s_g[KT_MAX_POINTS];       // cross: g; self: h of the odd sweeps
    __shared__ double s_w[KT_WAVES];
    const SkProblem<double> pr = sk_problem<UNBAL>(A);
    if (blockIdx.z != 2)
        for (int e = threadIdx.x; e < pr.np; e += KT_THREADS) { s_px[e] = pr.rows_p[(size_t)e * 3]; s_py[e] = pr.rows_p[(size_t)e * 3 + 1]; s_pz[e] = pr.rows_p[(size_t)e * 3 + 2]; }
    if (blockIdx.z != 1) sk_load(s_q, pr.rows_q, pr.nq);
    sk_divergence_block<UNBAL>(A, pr, SkPts64D{s_px, s_py, s_pz}, SkPts64F{s_q}, s_f, s_g, s_w);
}
__global__ void __launch_bounds__(KT_THREADS) kd64_sweeps(SkArgs64 A) { kd64_sweeps_body<false>(A); }
__global__ void __launch_bounds__(KT_THREADS) kd64_sweeps_unbalanced(SkArgs64 A) { kd64_sweeps_body<true>(A); }
__global__ void __launch_bounds__(KD_COMBINE_THREADS) kd64_combine(SkArgs64 A) { sk_combine<double, false, false>(A); }
__global__ void __launch_bounds__(KD_COMBINE_THREADS) kd64_combine_unbalanced(SkArgs64 A) { sk_combine<double, false, true>(A); }
