// k_gd_f64.h -- one iteration of the gradient-descent planner (planners.py:685-745) in float64: gen_s_delta and the reward
// forward, and the reverse pass through the reward, the steps of k_prop_f64.h (whose stored intermediates are the tape) and
// gen_s_delta.  A yardstick like k_prop_f64.h, not an engine: the reference's own formulation, every product and sum in double.
//
// The graph, gen_s_delta's hard mask, the bilinear cell and the chamfer arg-min are constants of the reverse pass, as autograd
// treats them.  The hidden layers of the encoders and of the predictor are not on the tape: the backward kernels evaluate them
// again with the forward kernels' own expressions (the same bits), for their ReLU masks.  Those three kernels can also write the
// hidden layers, their masked gradients and the narrow inputs out (null here): the operands of the weight gradients of
// k_train_f64.h.
//
// The 64-wide blocks run on v_mfma_f64_16x16x4_f64 with the fragment layout at the top of k_prop_f64.h; dX = dY W reads the
// blocks in the transposed fragment order (kf_frag_t).  The 5-, 6- and 3-wide layers and the reductions are fma / add chains.
// ONE order per value: ascending k in a layer; residual, then receiver slots ascending, then the edges a particle sends to in
// ascending (receiver, slot) order (the reversed lists of k_graph.h) in a gather; ascending particle / goal point in the
// reward's and the push gradient's sums.  No atomics: a row's outputs are the same bits in any batch, chunk or run.
#pragma once
#include "k_prop_f64.h"

#define KG_WAVES 2                  // tiles per workgroup (the relation encoder's backward keeps two LDS tiles per wave)
// the constants of gen_s_delta as the reference's expressions give them in double (planners.py:228, :251)
#define KG_PUSHER_W (0.8 / 24.0)
#define KG_SOFT_SCALE 0.01

// acc[jt] += (M > 0 ? G : 0) B for one 64x64 block: g_row / m_row are this lane's rows of the gradient and of the forward value
// whose ReLU it passed
__device__ __forceinline__ void kg_mma64_masked(kf_d4 acc[4], const double* __restrict__ g_row, const double* __restrict__ m_row,
                                                const double* __restrict__ frag, int lane) {
    const int kq = lane >> 4;
#pragma unroll 4
    for (int ks = 0; ks < 16; ++ks) {
        const double a = m_row[ks * 4 + kq] > 0.0 ? g_row[ks * 4 + kq] : 0.0;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
            acc[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, frag[(ks * 4 + jt) * 64 + lane], acc[jt], 0, 0, 0);
    }
}

// ---- gen_s_delta (planners.py:211-257) on doubles or on duals ---------------------------------------------------------
// directions 0..3: the push (sx, sy, ex, ey); 4..6: the particle's own position
struct KgDual {
    double v, d[7];
    __device__ KgDual() {}
    __device__ KgDual(double c) : v(c) {
#pragma unroll
        for (int i = 0; i < 7; ++i) d[i] = 0.0;
    }
};
__device__ __forceinline__ KgDual operator+(const KgDual& a, const KgDual& b) {
    KgDual r; r.v = a.v + b.v;
#pragma unroll
    for (int i = 0; i < 7; ++i) r.d[i] = a.d[i] + b.d[i];
    return r;
}
__device__ __forceinline__ KgDual operator-(const KgDual& a, const KgDual& b) {
    KgDual r; r.v = a.v - b.v;
#pragma unroll
    for (int i = 0; i < 7; ++i) r.d[i] = a.d[i] - b.d[i];
    return r;
}
__device__ __forceinline__ KgDual operator*(const KgDual& a, const KgDual& b) {
    KgDual r; r.v = a.v * b.v;
#pragma unroll
    for (int i = 0; i < 7; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
    return r;
}
__device__ __forceinline__ KgDual operator/(const KgDual& a, const KgDual& b) {
    KgDual r; r.v = a.v / b.v;
#pragma unroll
    for (int i = 0; i < 7; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) / b.v;
    return r;
}
__device__ __forceinline__ double kg_val(double a) { return a; }
__device__ __forceinline__ double kg_val(const KgDual& a) { return a.v; }
__device__ __forceinline__ double kg_sqrt(double a) { return sqrt(a); }
__device__ __forceinline__ KgDual kg_sqrt(const KgDual& a) {
    KgDual r; r.v = sqrt(a.v);
#pragma unroll
    for (int i = 0; i < 7; ++i) r.d[i] = a.d[i] * 0.5 / r.v;
    return r;
}
__device__ __forceinline__ double kg_exp(double a) { return exp(a); }
__device__ __forceinline__ KgDual kg_exp(const KgDual& a) {
    KgDual r; r.v = exp(a.v);
#pragma unroll
    for (int i = 0; i < 7; ++i) r.d[i] = a.d[i] * r.v;
    return r;
}

template <typename T> struct KgFrame { T sc[3], ec[3], dir[3], len; };
// camera-frame start / end of the push: s3 = (sx, 0, -sy), e3 = (ex, 0, -ey) through (M [p;1])[:3] / gs (planners.py:231-240);
// a zero-length push gives 0 / 0 = NaN, as the reference
template <typename T> __device__ __forceinline__ KgFrame<T> kg_frame(const DrpCam& cam, const T a[4]) {
    KgFrame<T> f;
    const T gs((double)cam.gs);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const T m0((double)cam.m[r * 4 + 0]), m2((double)cam.m[r * 4 + 2]), m3((double)cam.m[r * 4 + 3]);
        f.sc[r] = (a[0] * m0 - a[1] * m2 + m3) / gs;
        f.ec[r] = (a[2] * m0 - a[3] * m2 + m3) / gs;
    }
    const T vx = f.ec[0] - f.sc[0], vy = f.ec[1] - f.sc[1], vz = f.ec[2] - f.sc[2];
    f.len = kg_sqrt(vx * vx + vy * vy + vz * vz);
    f.dir[0] = vx / f.len; f.dir[1] = vy / f.len; f.dir[2] = vz / f.len;
    return f;
}
// the impulse of one particle (:242-254); false (and zeros) where the hard mask is off
template <typename T> __device__ __forceinline__ bool kg_push(const KgFrame<T>& f, const T p[3], T out[3]) {
    const T rx = p[0] - f.sc[0], ry = p[1] - f.sc[1], rz = p[2] - f.sc[2];
    const T v = ry * f.dir[0] - rx * f.dir[1];                   // (p - s) . ortho, ortho = (-dir_y, dir_x, 0)
    const T u = rx * f.dir[0] + ry * f.dir[1] + rz * f.dir[2];
    out[0] = out[1] = out[2] = T(0.0);
    if (!(kg_val(u) < kg_val(f.len) && kg_val(u) > 0.0)) {
        // the reference multiplies by a zero mask: a zero-length push (dir = 0 / 0) leaves NaN there, not zero
        if (kg_val(f.dir[0]) != kg_val(f.dir[0])) out[0] = out[1] = out[2] = T(__builtin_nan(""));
        return false;
    }
    // soft = exp(-max(relu(-w - v), relu(v - w)) / 0.01): at most one of the two is above zero
    const double lo = -KG_PUSHER_W - kg_val(v), hi = kg_val(v) - KG_PUSHER_W;
    T pen(0.0);
    if (lo > 0.0 && lo >= hi) pen = T(-KG_PUSHER_W) - v;
    else if (hi > 0.0) pen = v - T(KG_PUSHER_W);
    const T soft = kg_exp((T(0.0) - pen) / T(KG_SOFT_SCALE));
    const T te = (f.ec[0] - p[0]) * f.dir[0] + (f.ec[1] - p[1]) * f.dir[1] + (f.ec[2] - p[2]) * f.dir[2];
    const T base = te * soft;
    out[0] = base * f.dir[0]; out[1] = base * f.dir[1]; out[2] = base * f.dir[2];
    return true;
}

// the chunk's start state: row b of the batch starts from s0[b % nb], widened
__global__ __launch_bounds__(256) void kg_init_state(const float* __restrict__ s0, int nb, int b0, int N, long n, double* __restrict__ s) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const long row = t / (N * 3), k = t - row * (N * 3);
    s[t] = (double)s0[(size_t)((b0 + row) % nb) * N * 3 + k];
}

// impulses of a rollout step in double, and the fp32 roundings of state and impulse the graph build reads; grid = rows of the chunk
__global__ __launch_bounds__(256) void kg_sdelta(const double* __restrict__ s, const float* __restrict__ act, size_t act_stride, int N,
                                                 DrpCam cam, double* __restrict__ sd, float* __restrict__ s32, float* __restrict__ sd32) {
    const int b = blockIdx.x;
    const double a[4] = {(double)act[b * act_stride], (double)act[b * act_stride + 1], (double)act[b * act_stride + 2],
                         (double)act[b * act_stride + 3]};
    const KgFrame<double> f = kg_frame<double>(cam, a);
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const size_t o = ((size_t)b * N + n) * 3;
        const double p[3] = {s[o], s[o + 1], s[o + 2]};
        double out[3];
        kg_push<double>(f, p, out);
#pragma unroll
        for (int k = 0; k < 3; ++k) { sd[o + k] = out[k]; s32[o + k] = (float)p[k]; sd32[o + k] = (float)out[k]; }
    }
}

// ---- reward of the final state (env/flex_rewards.py:189-214) and d loss / d state, loss = -sum_b reward_b ---------------
// reward_b = -(r1 + r2) / N: r1 = sum_n bilinear(G, pix_n) under grid_sample's border clamp (align_corners = False), r2 =
// sum_m min_n |g_m - pix_n| (the lowest n wins a tie), pix = (x fx / z + cx, y fy / z + cy).  One workgroup per row; its
// scratch: px, py, gx, gy, r1t [N] doubles, dist [M] doubles, arg [M] ints.
__global__ __launch_bounds__(256) void kg_reward(const double* __restrict__ state, int N, const float* __restrict__ G, int Hh, int Ww,
                                                 const float* __restrict__ goal, int M, DrpCam cam, double* __restrict__ px_,
                                                 double* __restrict__ py_, double* __restrict__ gx_, double* __restrict__ gy_,
                                                 double* __restrict__ r1t_, double* __restrict__ dist_, int* __restrict__ arg_,
                                                 double* __restrict__ reward, double* __restrict__ g_state) {
    const int b = blockIdx.x;
    const double* s = state + (size_t)b * N * 3;
    double* px = px_ + (size_t)b * N; double* py = py_ + (size_t)b * N;
    double* gx = gx_ + (size_t)b * N; double* gy = gy_ + (size_t)b * N;
    double* r1t = r1t_ + (size_t)b * N;
    double* dist = dist_ + (size_t)b * M;
    int* arg = arg_ + (size_t)b * M;
    const double fx = (double)cam.fx, fy = (double)cam.fy, cx = (double)cam.cx, cy = (double)cam.cy;
    const double scale = 1.0 / (double)N, dW = (double)Ww, dH = (double)Hh;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const double x = s[n * 3], y = s[n * 3 + 1], z = s[n * 3 + 2];
        const double u = x * fx / z + cx, v = y * fy / z + cy;
        px[n] = u; py[n] = v;
        double ix = ((u / dH * 2.0 - 1.0) + 1.0) * dW / 2.0 - 0.5, iy = ((v / dH * 2.0 - 1.0) + 1.0) * dH / 2.0 - 0.5;
        double mx = dW / dH, my = 1.0;                       // d ix / d u, d iy / d v; zero where the clamp is active
        if (!(ix > 0.0)) { ix = 0.0; mx = 0.0; } else if (ix >= dW - 1.0) { ix = dW - 1.0; mx = 0.0; }
        if (!(iy > 0.0)) { iy = 0.0; my = 0.0; } else if (iy >= dH - 1.0) { iy = dH - 1.0; my = 0.0; }
        const double x0f = floor(ix), y0f = floor(iy);
        const double tx = ix - x0f, ty = iy - y0f;
        const int x0 = (int)x0f, y0 = (int)y0f;
        const int x1 = min(x0 + 1, Ww - 1), y1 = min(y0 + 1, Hh - 1);
        const double g00 = (double)G[(size_t)y0 * Ww + x0], g01 = (double)G[(size_t)y0 * Ww + x1];
        const double g10 = (double)G[(size_t)y1 * Ww + x0], g11 = (double)G[(size_t)y1 * Ww + x1];
        r1t[n] = g00 * (1.0 - tx) * (1.0 - ty) + g01 * tx * (1.0 - ty) + g10 * (1.0 - tx) * ty + g11 * tx * ty;
        gx[n] = scale * ((g01 - g00) * (1.0 - ty) + (g11 - g10) * ty) * mx;
        gy[n] = scale * ((g10 - g00) * (1.0 - tx) + (g11 - g01) * tx) * my;
    }
    __syncthreads();
    for (int m = threadIdx.x; m < M; m += blockDim.x) {
        const double qx = (double)goal[m * 2], qy = (double)goal[m * 2 + 1];
        double best = __builtin_inf();
        int a = 0;
        for (int n = 0; n < N; ++n) {
            const double dx = qx - px[n], dy = qy - py[n];
            const double d2 = dx * dx + dy * dy;
            if (d2 < best) { best = d2; a = n; }
        }
        dist[m] = sqrt(best);
        arg[m] = a;
    }
    __syncthreads();
    double* g = g_state + (size_t)b * N * 3;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        double ax = gx[n], ay = gy[n];
        for (int m = 0; m < M; ++m) {                        // d |q - p| / d p = -(q - p) / dist, goal points ascending
            if (arg[m] != n || !(dist[m] > 0.0)) continue;   // at distance 0: nothing, as torch.norm's backward (not 0 / 0)
            ax += -scale * ((double)goal[m * 2] - px[n]) / dist[m];
            ay += -scale * ((double)goal[m * 2 + 1] - py[n]) / dist[m];
        }
        const double x = s[n * 3], y = s[n * 3 + 1], z = s[n * 3 + 2];
        g[n * 3] = ax * fx / z;
        g[n * 3 + 1] = ay * fy / z;
        g[n * 3 + 2] = -(ax * x * fx + ay * y * fy) / (z * z);
    }
    if (threadIdx.x == 0) {
        double r1 = 0.0, r2 = 0.0;
        for (int n = 0; n < N; ++n) r1 += r1t[n];
        for (int m = 0; m < M; ++m) r2 += dist[m];
        reward[b] = -((r1 + r2) / (double)N);
    }
}

// ---- predictor backward (model/gnn_dyn.py:196, :110): g_out [rows,3] -> g_eff [rows,64] --------------------------------
__global__ __launch_bounds__(64 * KG_WAVES) void kg_predict_bwd(const double* __restrict__ w, const double* __restrict__ eff,
                                                                const double* __restrict__ g_out, int rows, double* __restrict__ g_eff,
                                                                double* __restrict__ h_out = nullptr /* [rows,64] the hidden layer ... */,
                                                                double* __restrict__ gh_out = nullptr /* ... and its masked gradient */) {
    __shared__ double X[KG_WAVES][16 * KF_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int row0 = (blockIdx.x * KG_WAVES + wave) * 16;
    const int row = min(row0 + r, rows - 1);
    double* x = X[wave];
    kf_d4 acc[4];
    kf_zero(acc);
    kf_mma64(acc, eff + (size_t)row * 64, kf_frag(w, KF_PR0), lane);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int col = jt * 16 + r, lrow = q + 4 * g;
            const size_t grow = (size_t)min(row0 + lrow, rows - 1);
            double gh = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) gh = fma(g_out[grow * 3 + k], w[W_PR1_W + k * 64 + col], gh);
            const double hv = acc[jt][g] + w[W_PR0_B + col];
            x[lrow * KF_LD + col] = hv > 0.0 ? gh : 0.0;
            if (h_out != nullptr && row0 + lrow < rows) {
                h_out[grow * 64 + col] = kf_relu(hv);
                gh_out[grow * 64 + col] = hv > 0.0 ? gh : 0.0;
            }
        }
    __syncthreads();
    kf_zero(acc);
    kf_mma64(acc, x + r * KF_LD, kf_frag_t(w, KF_PR0), lane);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int orow = row0 + q + 4 * g;
            if (orow < rows) g_eff[(size_t)orow * 64 + jt * 16 + r] = acc[jt][g];
        }
}

// ---- particle propagator backward (:191-193): g_next = d / d effect_{p+1} -> the pre-activation gradient g_pre (also the
// residual's share of d / d effect_p), g_agg = g_pre W[:, 64:128], g_pe (+)= g_pre W[:, 0:64] ----------------------------
__global__ __launch_bounds__(64 * KG_WAVES) void kg_pprop_bwd(const double* __restrict__ w, const double* __restrict__ eff_next,
                                                              const double* __restrict__ g_next, int rows, double* __restrict__ g_pre,
                                                              double* __restrict__ g_agg, double* __restrict__ g_pe, int first) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int row0 = (blockIdx.x * KG_WAVES + wave) * 16;
    const size_t row = (size_t)min(row0 + r, rows - 1);
    if (row0 + r < rows)
        for (int f = q * 16; f < q * 16 + 16; ++f) g_pre[row * 64 + f] = eff_next[row * 64 + f] > 0.0 ? g_next[row * 64 + f] : 0.0;
    kf_d4 acc[4];
    kf_zero(acc);
    kg_mma64_masked(acc, g_next + row * 64, eff_next + row * 64, kf_frag_t(w, KF_PP_AGG), lane);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int orow = row0 + q + 4 * g;
            if (orow < rows) g_agg[(size_t)orow * 64 + jt * 16 + r] = acc[jt][g];
        }
    kf_zero(acc);
    kg_mma64_masked(acc, g_next + row * 64, eff_next + row * 64, kf_frag_t(w, KF_PP_PE), lane);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int orow = row0 + q + 4 * g;
            if (orow >= rows) continue;
            const size_t o = (size_t)orow * 64 + jt * 16 + r;
            g_pe[o] = first ? acc[jt][g] : g_pe[o] + acc[jt][g];
        }
}

// ---- relation propagator backward (:183-189): the receiver's g_agg under the slot's ReLU -> g_re (+)= . W[:, 0:64], and per
// slot the receiver's and the sender's terms gr = . W[:, 64:128], gs = . W[:, 128:192] (kg_gather_bwd sums them) ---------
__global__ __launch_bounds__(64 * KG_WAVES) void kg_rprop_bwd(const double* __restrict__ w, const double* __restrict__ erel,
                                                              const double* __restrict__ g_agg, int erows, double* __restrict__ g_re,
                                                              double* __restrict__ gr, double* __restrict__ gs, int first) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int row0 = (blockIdx.x * KG_WAVES + wave) * 16;
    const size_t e = (size_t)min(row0 + r, erows - 1), p = e / DRP_K;
    kf_d4 acc[4];
    for (int part = 0; part < 3; ++part) {
        kf_zero(acc);
        kg_mma64_masked(acc, g_agg + p * 64, erel + e * 64, kf_frag_t(w, part == 0 ? KF_RP_E : part == 1 ? KF_RP_R : KF_RP_S), lane);
        double* dst = part == 0 ? g_re : part == 1 ? gr : gs;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int oe = row0 + q + 4 * g;
                if (oe >= erows) continue;
                const size_t o = (size_t)oe * 64 + jt * 16 + r;
                dst[o] = (part == 0 && !first) ? dst[o] + acc[jt][g] : acc[jt][g];
            }
    }
}

// d / d effect_p of a particle: the residual's share, its slots' receiver terms in slot order, the sender terms of the edges
// it feeds in the order of the reversed lists (ascending receiver, then slot); `add` (nullable) last.  One thread per value.
__global__ __launch_bounds__(256) void kg_gather_bwd(const double* __restrict__ g_pre, const double* __restrict__ gr,
                                                     const double* __restrict__ gs, const uint8_t* __restrict__ cnt,
                                                     const int* __restrict__ rev_off, const int* __restrict__ rev, int N, int rows,
                                                     const double* __restrict__ add, double* __restrict__ out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long i = t >> 6;
    const int f = (int)(t & 63);
    if (i >= rows) return;
    const long b = i / N, n = i - b * N;
    double a = g_pre[i * 64 + f];
    const int c = (int)cnt[i];
    for (int k = 0; k < c; ++k) a += gr[((size_t)i * DRP_K + k) * 64 + f];
    const int* ro = rev_off + b * (N + 1);
    const int* rv = rev + b * N * DRP_K;
    for (int p = ro[n]; p < ro[n + 1]; ++p) a += gs[((size_t)b * N * DRP_K + rv[p]) * 64 + f];
    if (add) a += add[i * 64 + f];
    out[i * 64 + f] = a;
}

// ---- particle encoder backward (:174-175): d / d particle_encode -> d / d s_delta [rows,3] ------------------------------
__global__ __launch_bounds__(64 * KG_WAVES) void kg_pencode_bwd(const double* __restrict__ w, const double* __restrict__ s_delta,
                                                                const float* __restrict__ attr, const float* __restrict__ dens,
                                                                const double* __restrict__ pe, const double* __restrict__ g_pe, int N,
                                                                int rows, double* __restrict__ g_sd,
                                                                double* __restrict__ in_out = nullptr /* [rows,5] the inputs, ... */,
                                                                double* __restrict__ h_out = nullptr /* [rows,64] the hidden layer ... */,
                                                                double* __restrict__ gh_out = nullptr /* ... and its masked gradient */) {
    __shared__ double X[KG_WAVES][16 * KF_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int row0 = (blockIdx.x * KG_WAVES + wave) * 16;
    const size_t row = (size_t)min(row0 + r, rows - 1);
    double* x = X[wave];
    {
        const double in[5] = {s_delta[row * 3], s_delta[row * 3 + 1], s_delta[row * 3 + 2], (double)attr[row],
                              (double)dens[row / N] / 5000.0};
        for (int o = q * 16; o < q * 16 + 16; ++o) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 5; ++k) acc = fma(in[k], w[W_PE0_W + o * 5 + k], acc);
            x[r * KF_LD + o] = kf_relu(acc + w[W_PE0_B + o]);
            if (h_out != nullptr && row0 + r < rows) h_out[row * 64 + o] = x[r * KF_LD + o];
        }
        if (in_out != nullptr && q == 0 && row0 + r < rows)
            for (int k = 0; k < 5; ++k) in_out[row * 5 + k] = in[k];
    }
    __syncthreads();
    kf_d4 acc[4];
    kf_zero(acc);
    kg_mma64_masked(acc, g_pe + row * 64, pe + row * 64, kf_frag_t(w, KF_PE2), lane);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int o = (q + 4 * g) * KF_LD + jt * 16 + r;
            x[o] = x[o] > 0.0 ? acc[jt][g] : 0.0;
            if (gh_out != nullptr && row0 + q + 4 * g < rows) gh_out[(size_t)(row0 + q + 4 * g) * 64 + jt * 16 + r] = x[o];
        }
    __syncthreads();
    if (q < 3 && row0 + r < rows) {
        double a = 0.0;
        for (int o = 0; o < 64; ++o) a = fma(x[r * KF_LD + o], w[W_PE0_W + o * 5 + q], a);
        g_sd[row * 3 + q] = a;
    }
}

// ---- relation encoder backward (:166-171, :179-180): d / d relation_encode -> d / d (s_r - s_s) per slot [erows,3] ------
__global__ __launch_bounds__(64 * KG_WAVES) void kg_rencode_bwd(const double* __restrict__ w, const double* __restrict__ s_cur,
                                                                const float* __restrict__ attr, const float* __restrict__ dens,
                                                                const int16_t* __restrict__ idx, const uint8_t* __restrict__ cnt,
                                                                const double* __restrict__ re, const double* __restrict__ g_re, int N,
                                                                int erows, double* __restrict__ g_diff,
                                                                double* __restrict__ in_out = nullptr /* [erows,6] the inputs, ... */,
                                                                double* __restrict__ h1_out = nullptr, double* __restrict__ h2_out = nullptr
                                                                /* [erows,64] the two hidden layers ... */,
                                                                double* __restrict__ g1_out = nullptr, double* __restrict__ g2_out = nullptr
                                                                /* ... and their masked gradients */) {
    __shared__ double X[KG_WAVES][16 * KF_LD], Y[KG_WAVES][16 * KF_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int row0 = (blockIdx.x * KG_WAVES + wave) * 16;
    const size_t e = (size_t)min(row0 + r, erows - 1);
    double* x = X[wave];
    double* y = Y[wave];
    {
        const size_t p = e / DRP_K, b = p / N;
        const int k = (int)(e - p * DRP_K);
        const size_t s = (k < (int)cnt[p]) ? b * N + (size_t)idx[e] : p;
        const double in[6] = {(double)attr[p], (double)attr[s], s_cur[p * 3] - s_cur[s * 3], s_cur[p * 3 + 1] - s_cur[s * 3 + 1],
                              s_cur[p * 3 + 2] - s_cur[s * 3 + 2], (double)dens[b] / 5000.0};
        for (int o = q * 16; o < q * 16 + 16; ++o) {
            double acc = 0.0;
#pragma unroll
            for (int kk = 0; kk < 6; ++kk) acc = fma(in[kk], w[W_RE0_W + o * 6 + kk], acc);
            x[r * KF_LD + o] = kf_relu(acc + w[W_RE0_B + o]);
            if (h1_out != nullptr && row0 + r < erows) h1_out[e * 64 + o] = x[r * KF_LD + o];
        }
        if (in_out != nullptr && q == 0 && row0 + r < erows)
            for (int kk = 0; kk < 6; ++kk) in_out[e * 6 + kk] = in[kk];
    }
    __syncthreads();
    kf_d4 acc[4];
    kf_zero(acc);
    kf_mma64(acc, x + r * KF_LD, kf_frag(w, KF_RE2), lane);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int col = jt * 16 + r;
            y[(q + 4 * g) * KF_LD + col] = kf_relu(acc[jt][g] + w[W_RE2_B + col]);
            if (h2_out != nullptr && row0 + q + 4 * g < erows) h2_out[(size_t)(row0 + q + 4 * g) * 64 + col] = y[(q + 4 * g) * KF_LD + col];
        }
    kf_zero(acc);
    kg_mma64_masked(acc, g_re + e * 64, re + e * 64, kf_frag_t(w, KF_RE4), lane);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int o = (q + 4 * g) * KF_LD + jt * 16 + r;
            y[o] = y[o] > 0.0 ? acc[jt][g] : 0.0;
            if (g2_out != nullptr && row0 + q + 4 * g < erows) g2_out[(size_t)(row0 + q + 4 * g) * 64 + jt * 16 + r] = y[o];
        }
    __syncthreads();
    kf_zero(acc);
    kf_mma64(acc, y + r * KF_LD, kf_frag_t(w, KF_RE2), lane);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int o = (q + 4 * g) * KF_LD + jt * 16 + r;
            x[o] = x[o] > 0.0 ? acc[jt][g] : 0.0;
            if (g1_out != nullptr && row0 + q + 4 * g < erows) g1_out[(size_t)(row0 + q + 4 * g) * 64 + jt * 16 + r] = x[o];
        }
    __syncthreads();
    if (q < 3 && row0 + r < erows) {
        double a = 0.0;
        for (int o = 0; o < 64; ++o) a = fma(x[r * KF_LD + o], w[W_RE0_W + o * 6 + 2 + q], a);
        g_diff[e * 3 + q] = a;
    }
}

// ---- the step's d loss / d input state ------------------------------------------------------------------------------------
// The relation encoder's share of component k of particle n of sample b, continuing the chain from v: plus g_diff [erows,3] of
// the particle's own slots ascending, minus g_diff of the slots it is the sender of in the reversed lists' order.
__device__ __forceinline__ double kg_state_share(double v, const double* __restrict__ g_diff, const uint8_t* __restrict__ cnt,
                                                 const int* __restrict__ rev_off, const int* __restrict__ rev, int N, size_t b, int n,
                                                 int k) {
    const size_t i = b * N + n, e0 = b * N * DRP_K;
    const int c = (int)cnt[i];
    const int* ro = rev_off + b * (N + 1);
    const int* rv = rev + e0;
    for (int j = 0; j < c; ++j) v += g_diff[(i * DRP_K + j) * 3 + k];
    for (int j = ro[n]; j < ro[n + 1]; ++j) v -= g_diff[(e0 + rv[j]) * 3 + k];
    return v;
}

// ---- the caller's seed in kg_reward's place (drp_gd_grad_f64_seeded) ---------------------------------------------------------
// the batch's seed [B][H][N][3] (doubles, the caller's layout) at the chunk's row offset b0, on grid (bc, H): step H-1's slice to
// g_last [bc*N,3] (g_state's slice H-1, where kg_reward writes), the steps before it to g_mid [H-1][bc*N,3] (kg_sdelta_bwd's
// g_add), bit for bit -- kb_seed_stage in double
__global__ __launch_bounds__(256) void kg_seed_in(const double* __restrict__ seed_in, int b0, int N, double* __restrict__ g_mid,
                                                  double* __restrict__ g_last) {
    const int b = blockIdx.x, t = blockIdx.y, bc = gridDim.x, H = gridDim.y;
    const int n3 = N * 3;
    const double* s = seed_in + ((size_t)(b0 + b) * H + t) * n3;
    double* g = (t == H - 1) ? g_last + (size_t)b * n3 : g_mid + ((size_t)t * bc + b) * n3;
    for (int i = threadIdx.x; i < n3; i += 256) g[i] = s[i];
}

// ---- gen_s_delta backward and the step's d loss / d input state ---------------------------------------------------------
// g_act[b, 0:4] = sum_n J_n^T g_sd[n] (particles ascending); g_prev[n] (nullable) = g_out[n] (the + s_cur of the output) [+ the
// caller's seed of that step, g_add] + the relation encoder's share (kg_state_share) + gen_s_delta's dependence on the position.  One workgroup per row; part
// [rows*N,4]: scratch.
__global__ __launch_bounds__(256) void kg_sdelta_bwd(const double* __restrict__ s, const float* __restrict__ act, size_t act_stride,
                                                     const double* __restrict__ g_sd, const double* __restrict__ g_out,
                                                     const double* __restrict__ g_diff, const uint8_t* __restrict__ cnt,
                                                     const int* __restrict__ rev_off, const int* __restrict__ rev, int N, DrpCam cam,
                                                     double* __restrict__ part, double* __restrict__ g_act, size_t gact_stride,
                                                     double* __restrict__ g_prev,
                                                     const double* __restrict__ g_add = nullptr /* nullable, laid out as g_prev: the
                                                        caller's seed of the step before (drp_gd_grad_f64_seeded), added to g_out
                                                        first -- the point where kb_gather_pos adds it in fp32 */) {
    const int b = blockIdx.x;
    KgDual a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { a[k] = KgDual((double)act[b * act_stride + k]); a[k].d[k] = 1.0; }
    const KgFrame<KgDual> f = kg_frame<KgDual>(cam, a);
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const size_t i = (size_t)b * N + n;
        KgDual p[3], out[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { p[k] = KgDual(s[i * 3 + k]); p[k].d[4 + k] = 1.0; }
        double g7[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (kg_push<KgDual>(f, p, out)) {
#pragma unroll
            for (int k = 0; k < 7; ++k) g7[k] = g_sd[i * 3] * out[0].d[k] + g_sd[i * 3 + 1] * out[1].d[k] + g_sd[i * 3 + 2] * out[2].d[k];
        } else if (out[0].v != out[0].v) {
#pragma unroll
            for (int k = 0; k < 7; ++k) g7[k] = out[0].v;           // a zero-length push: NaN, as the reference's autograd
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) part[i * 4 + k] = g7[k];
        if (g_prev != nullptr) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double v = g_add != nullptr ? g_out[i * 3 + k] + g_add[i * 3 + k] : g_out[i * 3 + k];
                g_prev[i * 3 + k] = kg_state_share(v, g_diff, cnt, rev_off, rev, N, (size_t)b, n, k) + g7[4 + k];
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double v = 0.0;
        for (int n = 0; n < N; ++n) v += part[((size_t)b * N + n) * 4 + threadIdx.x];
        g_act[b * gact_stride + threadIdx.x] = v;
    }
}
