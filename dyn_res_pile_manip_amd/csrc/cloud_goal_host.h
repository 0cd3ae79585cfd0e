// cloud_goal_host.h -- host-side arithmetic of the cloud goal (capi_cloud_goal.h): the parameter checks, the eps
// table of the Sinkhorn kind and the mapping of a session's rows to its start columns (column_of_row: the ONE definition, which
// the kernels of k_cloud_goal.h call too).  No HIP, no context: plain C++ that tools/cloud_goal_host_check.cpp compiles alone
// (under the host sanitizers); under hipcc column_of_row is also a device function.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdio>

#ifdef __HIPCC__
#define CLOUD_GOAL_HD __host__ __device__
#else
#define CLOUD_GOAL_HD
#endif

namespace cloud_goal {

enum Kind { CHAMFER = 0, SINKHORN = 1 };        // DRP_CLOUD_CHAMFER, DRP_CLOUD_SINKHORN (include/drp.h)

// the kernels' limits, handed in by the caller (k_chamfer.h: KC_MAX_POINTS; k_sinkhorn.h: KT_MAX_POINTS, KT_MAX_ITERS)
struct Limits { int chamfer_points, sinkhorn_points, sinkhorn_iters; };

inline bool kind_ok(int kind) { return kind == CHAMFER || kind == SINKHORN; }
// the most points either cloud of a problem may have; 0 for a kind that does not exist
inline int point_cap(int kind, const Limits& lim) {
    return kind == CHAMFER ? lim.chamfer_points : kind == SINKHORN ? lim.sinkhorn_points : 0;
}

// index of the first coordinate of x[0 .. n) that is infinite or not a number, or -1
inline long first_nonfinite(const float* x, size_t n) {
    for (size_t e = 0; e < n; ++e)
        if (!std::isfinite(x[e])) return (long)e;
    return -1;
}

// what drp_set_goal_cloud refuses beside null pointers and non-finite points: true if all is well, else `msg` says what is not
inline bool check_params(int kind, double weight, double eps_scale, int iters, int M, const Limits& lim, char* msg, size_t n_msg) {
    if (!kind_ok(kind)) { snprintf(msg, n_msg, "bad cloud goal kind %d", kind); return false; }
    if (!(weight > 0.0) || !std::isfinite(weight)) { snprintf(msg, n_msg, "weight=%g is not a positive finite number", weight); return false; }
    const int cap = point_cap(kind, lim);
    if (M < 1 || M > cap) { snprintf(msg, n_msg, "bad shape M=%d (1..%d for this kind of cloud goal)", M, cap); return false; }
    if (kind == SINKHORN) {
        if (!(eps_scale > 0.0) || !std::isfinite(eps_scale)) { snprintf(msg, n_msg, "eps_scale=%g is not a positive finite number", eps_scale); return false; }
        if (iters < 1 || iters > lim.sinkhorn_iters) { snprintf(msg, n_msg, "iters=%d outside 1..%d", iters, lim.sinkhorn_iters); return false; }
    }
    return true;
}

// the predicted cloud's size against the kind's limit (the sessions' begin, the one-shot)
inline bool check_pred_points(int kind, int N, const Limits& lim, char* msg, size_t n_msg) {
    const int cap = point_cap(kind, lim);
    if (N < 1 || N > cap) { snprintf(msg, n_msg, "bad shape N=%d (1..%d for this kind of cloud goal)", N, cap); return false; }
    return true;
}

// row = trajectory * n_batch + column (planners.py's layout): the start column whose density, eps and target self problem a row
// reads.  kg_sinkhorn and kg_sinkhorn_combine index their tables with it; the one-shot has a column per row (n_batch = B)
CLOUD_GOAL_HD inline int column_of_row(long row, int n_batch) { return (int)(row % (long)n_batch); }

// eps[col] = (double)eps_scale / (double)dens[col], as costs.cloud_divergence_cost forms it (1 / dens is the squared sampling
// spacing); returns the first column whose eps is not a positive finite number (a density that is zero, negative, infinite
// or no number), or -1
inline int eps_table(double eps_scale, const float* dens, int n_batch, double* eps) {
    int bad = -1;
    for (int col = 0; col < n_batch; ++col) {
        eps[col] = eps_scale / (double)dens[col];
        if (bad < 0 && (!(eps[col] > 0.0) || !std::isfinite(eps[col]))) bad = col;
    }
    return bad;
}

// counts of the one-shot's clouds: the first row whose count lies outside 1..N, or -1 (a null array: every row has N)
inline int first_bad_count(const int* n_p, int B, int N) {
    if (n_p == nullptr) return -1;
    for (int b = 0; b < B; ++b)
        if (n_p[b] < 1 || n_p[b] > N) return b;
    return -1;
}

}  // namespace cloud_goal
