// Reverse mode of the path for the gradient-descent planner:
//   loss = -sum_b reward_b    planners.py:743   ->   d loss / d pushes
// through config_reward_ptcl (env/flex_rewards.py:189-214), PropModuleDiffDen.forward
// (model/gnn_dyn.py:147-198; the graph masks are constants: autograd gives zero through
// topk / the radius test) and gen_s_delta (planners.py:211-257; the hard mask is constant,
// the soft mask and the projections are differentiated, the direction depends on the push).
//
// Any horizon: the reward is taken at the final step only (planners.py:436-438); going back
// through a step, the gradient w.r.t. its input positions is the residual's share, plus the
// relation encoder's (its inputs are position differences), plus gen_s_delta's dependence
// on the particle position.  Here the fp32 VALU kernels of the pass (the node-level stages and the relation
// encoder's backward run on the matrix cores, k_backward_mfma.h) over what the fused forward pass
// (km_prop<., TAPE>) left in HBM: the effect after the encoder and after every propagation step, and the
// edges' ReLU masks.  The one scatter of the backward pass
// (gradient of the gathered sender rows) is turned into a gather over reversed neighbour lists
// (kb_reverse_lists, kb_edge_terms, kb_gather_pos): no atomics, reproducible sums.
#pragma once
#include "drp_common.h"
#include "k_reward.h"
#include "k_graph.h"
#include "k_mlp_valu.h"

#define KB_R 4

// kb_edge_terms runs one workgroup per (sample, chunk of rows): `chunks` = 1 when the batch
// alone fills the chip (the planner's thousands of samples), more for the trainer's handful.
struct KbRange { int b, lo, hi; };
__device__ __forceinline__ KbRange kb_range(int N, int chunks) {
    KbRange r;
    r.b = blockIdx.x / chunks;
    const int ch = blockIdx.x - r.b * chunks;
    const int len = (((N + chunks - 1) / chunks) + KB_R - 1) & ~(KB_R - 1);
    r.lo = ch * len;
    r.hi = min(N, r.lo + len);
    return r;
}

// ---- reward backward: g_state[b,n,:] = d(-reward_b... ) see below ------------------------------
// loss = -sum_b reward_b, reward_b = -(r1 + r2)/N  =>  d loss / d r1 = d loss / d r2 = 1/N.
//   r1 = sum_n bilinear(G, pix_n)      -> grid_sample's gradient w.r.t. the grid (zero where the
//                                          border clamp is active, as torch does)
//   r2 = sum_m min_n |g_m - pix_n|     -> -(g_m - pix_n*) / dist to the arg-min particle n*
//   pix = (x fx / z + cx, y fy / z + cy)
// one workgroup per state row; gradient accumulated in LDS, then written.  dynamic LDS = KB_REWARD_LDS(N).
// reward_out (nullable): the reward itself too, in k_reward's arithmetic and reduction order (the same bits) --
// the planner's iteration then needs one launch for the reward and its gradient instead of two.
#define KB_REWARD_LDS(N) ((size_t)(2 * (N) + 8) * sizeof(float) + (size_t)(2 * (N)) * sizeof(long long))
// one state row `s` against one goal, gradient to `g`: the workgroup's whole work (kb_reward and kb_reward_scenes differ in
// where G, goal_coor and M come from, in nothing else)
__device__ __forceinline__ void kb_reward_row(const float* __restrict__ s, int N, const float* __restrict__ G, int Hh, int Ww,
                                              const float* __restrict__ goal_coor, int M, const DrpCam& cam, int normalize,
                                              float* __restrict__ g, float* __restrict__ reward_out,
                                              float* __restrict__ reward_copy) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* px = lds;
    float* py = lds + N;
    float* red = lds + 2 * N + 4 * N;                 // behind the two long long arrays
    float r1 = 0.0f, r2 = 0.0f;
    // d loss / d pixel, accumulated as 2^-40 fixed point: integer adds commute, so the many goal
    // points whose nearest particle is the same one can add in any order and the sum is the same
    // bits every run (fp32 LDS atomics were the last source of run-to-run differences)
    long long* gx = reinterpret_cast<long long*>(lds + 2 * N);
    long long* gy = gx + N;
    const float FIX = 1099511627776.0f, UNFIX = 1.0f / 1099511627776.0f;
    const float scale = normalize ? 1.0f / (float)N : 1.0f;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const float x = s[n * 3 + 0], y = s[n * 3 + 1], z = s[n * 3 + 2];
        const float u = x * cam.fx / z + cam.cx, v = y * cam.fy / z + cam.cy;
        px[n] = u;
        py[n] = v;
        // bilinear sample gradient (align_corners = False, padding 'border')
        const float nx = u / (float)Hh * 2.0f - 1.0f, ny = v / (float)Hh * 2.0f - 1.0f;
        float ix = ((nx + 1.0f) * (float)Ww - 1.0f) / 2.0f, iy = ((ny + 1.0f) * (float)Hh - 1.0f) / 2.0f;
        // clip_coordinates_set_grad: gradient multiplier 0 outside [0, size-1]
        float mx = (float)Ww / (float)Hh, my = 1.0f;     // d ix / d u, d iy / d v
        if (ix <= 0.0f) { ix = 0.0f; mx = 0.0f; } else if (ix >= (float)(Ww - 1)) { ix = (float)(Ww - 1); mx = 0.0f; }
        if (iy <= 0.0f) { iy = 0.0f; my = 0.0f; } else if (iy >= (float)(Hh - 1)) { iy = (float)(Hh - 1); my = 0.0f; }
        const float x0f = floorf(ix), y0f = floorf(iy);
        const float tx = ix - x0f, ty = iy - y0f;
        const int x0 = (int)x0f, y0 = (int)y0f;
        const int x1 = x0 + 1, y1 = y0 + 1;
        const float g00 = G[(size_t)y0 * Ww + x0];
        const float g01 = (x1 < Ww) ? G[(size_t)y0 * Ww + x1] : 0.0f;
        const float g10 = (y1 < Hh) ? G[(size_t)y1 * Ww + x0] : 0.0f;
        const float g11 = (x1 < Ww && y1 < Hh) ? G[(size_t)y1 * Ww + x1] : 0.0f;
        const float dgx = (g01 - g00) * (1.0f - ty) + (g11 - g10) * ty;
        const float dgy = (g10 - g00) * (1.0f - tx) + (g11 - g01) * tx;
        gx[n] = __float2ll_rn(scale * dgx * mx * FIX);
        gy[n] = __float2ll_rn(scale * dgy * my * FIX);
        if (reward_out != nullptr) {
            // k_reward's forward value: border clamp of the coordinates and of the upper taps
            const float fx_ = fminf(fmaxf(((nx + 1.0f) * (float)Ww - 1.0f) / 2.0f, 0.0f), (float)(Ww - 1));
            const float fy_ = fminf(fmaxf(((ny + 1.0f) * (float)Hh - 1.0f) / 2.0f, 0.0f), (float)(Hh - 1));
            const float fx0 = floorf(fx_), fy0 = floorf(fy_);
            const float ftx = fx_ - fx0, fty = fy_ - fy0;
            const int ax0 = (int)fx0, ay0 = (int)fy0;
            const int ax1 = min(ax0 + 1, Ww - 1), ay1 = min(ay0 + 1, Hh - 1);
            const float f00 = G[(size_t)ay0 * Ww + ax0], f01 = G[(size_t)ay0 * Ww + ax1];
            const float f10 = G[(size_t)ay1 * Ww + ax0], f11 = G[(size_t)ay1 * Ww + ax1];
            r1 += f00 * ((1.0f - ftx) * (1.0f - fty)) + f01 * (ftx * (1.0f - fty)) +
                  f10 * ((1.0f - ftx) * fty) + f11 * (ftx * fty);
        }
    }
    __syncthreads();
    for (int m = threadIdx.x; m < M; m += blockDim.x) {
        const float qx = goal_coor[m * 2 + 0], qy = goal_coor[m * 2 + 1];
        float best = __builtin_inff();
        int arg = 0;
        for (int n = 0; n < N; ++n) {
            const float dx = qx - px[n], dy = qy - py[n];
            const float d2 = dx * dx + dy * dy;
            if (d2 < best) { best = d2; arg = n; }       // first minimum, as torch.min
        }
        const float dist = drp_sqrt_rn(best);
        r2 += dist;
        // d |q - p| / d p = -(q - p) / dist; a goal pixel that IS the particle's pixel contributes nothing (torch.norm's
        // backward gives 0 at 0, not 0 / 0 -- and a NaN has no defined conversion to the fixed point)
        if (dist > 0.0f) {
            atomicAdd(reinterpret_cast<unsigned long long*>(&gx[arg]), (unsigned long long)__float2ll_rn(-scale * (qx - px[arg]) / dist * FIX));
            atomicAdd(reinterpret_cast<unsigned long long*>(&gy[arg]), (unsigned long long)__float2ll_rn(-scale * (qy - py[arg]) / dist * FIX));
        }
    }
    __syncthreads();
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const float x = s[n * 3 + 0], y = s[n * 3 + 1], z = s[n * 3 + 2];
        const float gxn = (float)((double)gx[n] * (double)UNFIX), gyn = (float)((double)gy[n] * (double)UNFIX);
        g[n * 3 + 0] = gxn * cam.fx / z;
        g[n * 3 + 1] = gyn * cam.fy / z;
        g[n * 3 + 2] = -(gxn * x * cam.fx + gyn * y * cam.fy) / (z * z);
    }
    if (reward_out != nullptr) {
        const float t1 = block_sum_256(r1, red);
        const float t2 = block_sum_256(r2, red);
        if (threadIdx.x == 0) {
            float r = t1 + t2;
            if (normalize) r = __fdiv_rn(r, (float)N);
            reward_out[blockIdx.x] = -r;
            if (reward_copy != nullptr) reward_copy[blockIdx.x] = -r;
        }
    }
}

__global__ void __launch_bounds__(256)
kb_reward(const float* __restrict__ state, size_t row_stride, int N, const float* __restrict__ G, int Hh, int Ww,
          const float* __restrict__ goal_coor, int M, DrpCam cam, int normalize, float* __restrict__ g_state,
          size_t g_stride, float* __restrict__ reward_out, float* __restrict__ reward_copy = nullptr /* pinned host memory */) {
    kb_reward_row(state + (size_t)blockIdx.x * row_stride, N, G, Hh, Ww, goal_coor, M, cam, normalize,
                  g_state + (size_t)blockIdx.x * g_stride, reward_out, reward_copy);
}

// the same with a goal per row (k_reward.h: GoalTable): row r reads the field, the pixels and the pixel count of scene(r)
__global__ void __launch_bounds__(256)
kb_reward_scenes(const float* __restrict__ state, size_t row_stride, int N, GoalTable gt, int Hh, int Ww, DrpCam cam,
                 int normalize, float* __restrict__ g_state, size_t g_stride, float* __restrict__ reward_out,
                 float* __restrict__ reward_copy /* pinned host memory, nullable */) {
    const int sc = goal_scene(gt, (int)blockIdx.x);
    kb_reward_row(state + (size_t)blockIdx.x * row_stride, N, gt.fields + (size_t)sc * gt.field_stride, Hh, Ww,
                  gt.coor + (size_t)sc * gt.m_max * 2, gt.m[sc], cam, normalize, g_state + (size_t)blockIdx.x * g_stride,
                  reward_out, reward_copy);
}

// ---- reversed neighbour lists: for every sender j the edge slots (i*10 + k) it feeds, ascending --
// The backward pass of the sender gather is a scatter; with the lists reversed it becomes a
// gather again -- no atomics, a fixed summation order (the first version scattered with fp32 global
// atomics: 64 per edge, 61 % of a planner iteration, and not reproducible run to run).
// One workgroup per sample; out-degrees counted and scanned in LDS; the lists are filled and put
// in order in LDS too when they fit (dynamic LDS = 2*N ints, + 10*N ints with `in_lds`).
#define KB_REV_THREADS 1024
#define KB_REV_LDS(N, in_lds) ((size_t)((in_lds) ? 12 : 2) * (N) * sizeof(int))
#define KB_REV_LDS_MAX_N 3072
// T threads per sample: 1024, or 256 for samples of up to 512 particles (four times as many samples in flight per CU:
// the kernel is a chain of short LDS phases, 45 -> 15 us at 1500 x 100)
template <int T>
__global__ void __launch_bounds__(T)
kb_reverse_lists(const int16_t* __restrict__ nbr_idx, const uint8_t* __restrict__ nbr_cnt, int N,
                 int* __restrict__ rev_off /* [B][N+1] */, int* __restrict__ rev /* [B][N*10] */, int in_lds,
                 const int* __restrict__ n_real /* nullable [B]: receivers >= n_real[b] are padding whose
                                                   gradient is identically zero (training batches) */,
                 int n_real_mod = 0 /* > 0: the grid runs over several rollout steps' lists, sample = block % n_real_mod */) {
    extern __shared__ int s_rev[];
    const int b = blockIdx.x;
    const int n_recv = n_real ? n_real[n_real_mod > 0 ? b % n_real_mod : b] : N;
    reverse_lists<T>(nbr_idx + (size_t)b * N * DRP_K, nbr_cnt + (size_t)b * N, N, rev_off + (size_t)b * (N + 1),
                     rev + (size_t)b * N * DRP_K, in_lds, n_recv, s_rev);
}

// ---- aggregate backward.  The gradient of an edge's pre-activation is the receiver's g_agg row
//      under the edge's ReLU mask: g_u[i,k,:] = g_agg[i,:] . [relation effect of (i,k) > 0].  The
//      forward pass (km_prop<., TAPE>) leaves the 64 mask bits of every edge slot and propagation
//      step (8 B instead of a 256-B row); nothing else of the edge stage is kept.  Here: the
//      receiver term g_proj[i][0:64] = sum_k g_u and, over the reversed lists, the sender term
//      g_proj[j][64:128] (kb_edge_terms); kmb_edge_encode and the weight gradients rebuild g_u the same way.
// Mask layout (k_mlp_split.h frag_positive_bits): two words per slot; feature f lives in word
// (f>>2)&1 at bit 31 - (16*(f>>5) + (f&3) + 4*((f&31)>>3)).  The four features 4q..4q+3 of a float4
// lane q are one nibble of word q&1.
__device__ __forceinline__ int kb_mask_word(int f) { return (f >> 2) & 1; }
__device__ __forceinline__ int kb_mask_bit(int f) { return 31 - (16 * (f >> 5) + (f & 3) + 4 * ((f & 31) >> 3)); }
__device__ __forceinline__ unsigned kb_mask_nibble(const unsigned* __restrict__ m2, int q) {
    return (m2[q & 1] >> (28 - 16 * (q >> 3) - 4 * ((q >> 1) & 3))) & 0xfu;      // bit 3 = component x ... bit 0 = w
}

// both edge terms of a node in one launch: g_proj[n][0:64] from the node's own slots (the same value
// g_agg[n] under 0/1 masks, added one by one as an edge loop would), g_proj[n][64:128] from the edges it
// feeds, in the order of the reversed lists (ascending receiver, then slot).
// Same 16-lanes-per-node layout as k_aggregate.
__global__ void __launch_bounds__(256)
kb_edge_terms(const float* __restrict__ g_agg, const unsigned* __restrict__ mask, const uint8_t* __restrict__ nbr_cnt,
              const int* __restrict__ rev_off, const int* __restrict__ rev, int N, float* __restrict__ g_proj, int chunks) {
    const KbRange rg = kb_range(N, chunks);
    const int b = rg.b;
    const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
    const float4* ga = reinterpret_cast<const float4*>(g_agg) + (size_t)b * N * 16;
    const unsigned* mk = mask + (size_t)b * N * DRP_K * 2;
    const int* ro = rev_off + (size_t)b * (N + 1);
    const int* rv = rev + (size_t)b * N * DRP_K;
    float* gp = g_proj + (size_t)b * N * 128;
    const uint8_t* nc = nbr_cnt + (size_t)b * N;
    for (int i = rg.lo + g; i < rg.hi; i += 16) {
        const int cnt = nc[i];
        const float4 gi = ga[(size_t)i * 16 + q];
        int nx = 0, ny = 0, nz = 0, nw = 0;
        for (int k = 0; k < cnt; ++k) {
            const unsigned nib = kb_mask_nibble(mk + ((size_t)i * DRP_K + k) * 2, q);
            nx += (nib >> 3) & 1; ny += (nib >> 2) & 1; nz += (nib >> 1) & 1; nw += nib & 1;
        }
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t = 0; t < nx; ++t) acc.x += gi.x;
        for (int t = 0; t < ny; ++t) acc.y += gi.y;
        for (int t = 0; t < nz; ++t) acc.z += gi.z;
        for (int t = 0; t < nw; ++t) acc.w += gi.w;
        *reinterpret_cast<float4*>(gp + (size_t)i * 128 + q * 4) = acc;
        const int p0 = ro[i], p1 = ro[i + 1];
        acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int p = p0; p < p1; ++p) {
            const int e = rv[p];
            const unsigned nib = kb_mask_nibble(mk + (size_t)e * 2, q);
            const float4 v = ga[(size_t)(e / DRP_K) * 16 + q];
            acc.x += (nib & 8u) ? v.x : 0.0f;
            acc.y += (nib & 4u) ? v.y : 0.0f;
            acc.z += (nib & 2u) ? v.z : 0.0f;
            acc.w += (nib & 1u) ? v.w : 0.0f;
        }
        *reinterpret_cast<float4*>(gp + (size_t)i * 128 + 64 + q * 4) = acc;
    }
}

// ---- gen_s_delta backward: g_action[b, 0:4] = sum_n J_n^T g_s_delta[n], forward-mode over the four
//      push parameters (sx, sy, ex, ey); the hard mask is a constant (planners.py:248)
template <int ND>
struct Dual {
    float v, d[ND];
};
template <int ND> __device__ __forceinline__ Dual<ND> dconst(float v) {
    Dual<ND> r; r.v = v;
#pragma unroll
    for (int c = 0; c < ND; ++c) r.d[c] = 0.0f;
    return r;
}
template <int ND> __device__ __forceinline__ Dual<ND> operator+(const Dual<ND>& a, const Dual<ND>& b) {
    Dual<ND> r; r.v = a.v + b.v;
#pragma unroll
    for (int c = 0; c < ND; ++c) r.d[c] = a.d[c] + b.d[c];
    return r;
}
template <int ND> __device__ __forceinline__ Dual<ND> operator-(const Dual<ND>& a, const Dual<ND>& b) {
    Dual<ND> r; r.v = a.v - b.v;
#pragma unroll
    for (int c = 0; c < ND; ++c) r.d[c] = a.d[c] - b.d[c];
    return r;
}
template <int ND> __device__ __forceinline__ Dual<ND> operator*(const Dual<ND>& a, const Dual<ND>& b) {
    Dual<ND> r; r.v = a.v * b.v;
#pragma unroll
    for (int c = 0; c < ND; ++c) r.d[c] = a.d[c] * b.v + a.v * b.d[c];
    return r;
}
template <int ND> __device__ __forceinline__ Dual<ND> operator/(const Dual<ND>& a, const Dual<ND>& b) {
    Dual<ND> r; r.v = a.v / b.v;
    const float ib = 1.0f / b.v;
#pragma unroll
    for (int c = 0; c < ND; ++c) r.d[c] = (a.d[c] - r.v * b.d[c]) * ib;
    return r;
}
template <int ND> __device__ __forceinline__ Dual<ND> dsqrt(const Dual<ND>& a) {
    Dual<ND> r; r.v = sqrtf(a.v);
    const float k = 0.5f / r.v;
#pragma unroll
    for (int c = 0; c < ND; ++c) r.d[c] = a.d[c] * k;
    return r;
}

// ---- Adam (torch.optim.Adam defaults: betas (0.9, 0.999), eps 1e-8) + the clip box ------------
//      planners.py:674, :743-746, :756-764
struct KbAdam {                 // the optimiser step of a row's pushes at the end of kb_sdelta (act == null: not in this launch)
    float* act; float* m; float* v; float* act_copy /* nullable: pinned host memory */;
    int n_row;                  // values per row: H * 4
    float step_size, bc2_sqrt, b1;
    float4 lo, hi;
};
__device__ __forceinline__ float adam_update(float a0, float g, float& m, float& v, float step_size, float bc2_sqrt, float b1,
                                             float l, float h) {
    const float b2 = 0.999f, eps = 1e-8f;
    const float mi = m + (g - m) * (1.0f - b1);          // exp_avg.lerp_(grad, 1 - beta1)
    const float vi = v * b2 + (1.0f - b2) * g * g;
    m = mi;
    v = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    const float a = a0 - step_size * (mi / denom);
    return fminf(fmaxf(a, l), h);
}

// directions 0..3: the push (sx, sy, ex, ey); 4..6: the particle's own position (x, y, z).
// g_action[b, 0:4] = sum_n J_n^T g_s_delta[n];  g_pos[b, n, 0:3] += J_pos^T g_s_delta[n] (nullable)
__global__ void __launch_bounds__(256)
kb_sdelta(const float* __restrict__ s_cur, int s_mod, size_t s_stride, const float* actions /* may be adam.act: no restrict */,
          size_t act_stride, const float* __restrict__ g_sdelta, int N, DrpCam cam, float* g_action /* read back below */,
          size_t gact_stride, float* __restrict__ g_pos, size_t gpos_stride, KbAdam adam = KbAdam{}) {
    typedef Dual<7> D;
    __shared__ float red[4][4];
    const int b = blockIdx.x;
    // the push of this row and step, by value: with rollout step 0 the optimiser step at the end of this kernel overwrites
    // the very elements (adam.act is the actions buffer)
    const float act[4] = {actions[(size_t)b * act_stride + 0], actions[(size_t)b * act_stride + 1],
                          actions[(size_t)b * act_stride + 2], actions[(size_t)b * act_stride + 3]};
    const float* s = s_cur + (size_t)(b % s_mod) * s_stride;
    const float* gs = g_sdelta + (size_t)b * N * 3;
    // camera-frame start / end as duals of (sx, sy, ex, ey): s3 = (sx, 0, -sy), e3 = (ex, 0, -ey)
    D sc[3], ec[3];
    const float igs = 1.0f / cam.gs;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float m0 = cam.m[r * 4 + 0], m2 = cam.m[r * 4 + 2], m3 = cam.m[r * 4 + 3];
        sc[r] = dconst<7>((m0 * act[0] - m2 * act[1] + m3) * igs);
        sc[r].d[0] = m0 * igs; sc[r].d[1] = -m2 * igs;
        ec[r] = dconst<7>((m0 * act[2] - m2 * act[3] + m3) * igs);
        ec[r].d[2] = m0 * igs; ec[r].d[3] = -m2 * igs;
    }
    const D vx = ec[0] - sc[0], vy = ec[1] - sc[1], vz = ec[2] - sc[2];
    const D len = dsqrt(vx * vx + vy * vy + vz * vz);
    const D dx = vx / len, dy = vy / len, dz = vz / len;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        D px = dconst<7>(s[n * 3 + 0]), py = dconst<7>(s[n * 3 + 1]), pz = dconst<7>(s[n * 3 + 2]);
        px.d[4] = 1.0f; py.d[5] = 1.0f; pz.d[6] = 1.0f;
        const D rx = px - sc[0], ry = py - sc[1], rz = pz - sc[2];
        const D v = ry * dx - rx * dy;                                  // (p - s) . ortho, ortho = (-dy, dx, 0)
        const D u = rx * dx + ry * dy + rz * dz;
        float g7[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (u.v < len.v && u.v > 0.0f) {                                 // hard mask (constant)
            // soft = exp(-max(relu(-w - v), relu(v - w)) / 0.01)
            D pen = dconst<7>(0.0f);
            const float lo = -DRP_PUSHER_W - v.v, hi = v.v - DRP_PUSHER_W;
            if (lo > 0.0f && lo >= hi) pen = dconst<7>(-DRP_PUSHER_W) - v;
            else if (hi > 0.0f) pen = v - dconst<7>(DRP_PUSHER_W);
            const float e = expf(-pen.v / DRP_SOFT_SCALE);
            D soft = dconst<7>(e);
#pragma unroll
            for (int c = 0; c < 7; ++c) soft.d[c] = -e * pen.d[c] / DRP_SOFT_SCALE;
            const D te = (ec[0] - px) * dx + (ec[1] - py) * dy + (ec[2] - pz) * dz;
            const D base = te * soft;
            const D ox = base * dx, oy = base * dy, oz = base * dz;
            const float g0 = gs[n * 3 + 0], g1 = gs[n * 3 + 1], g2 = gs[n * 3 + 2];
#pragma unroll
            for (int c = 0; c < 7; ++c) g7[c] = g0 * ox.d[c] + g1 * oy.d[c] + g2 * oz.d[c];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] += g7[c];
        if (g_pos != nullptr) {
            float* gp = g_pos + (size_t)b * gpos_stride + (size_t)n * 3;
            gp[0] += g7[4]; gp[1] += g7[5]; gp[2] += g7[6];
        }
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float t = wave_sum(acc[c]);
        if ((threadIdx.x & 63) == 0) red[wave][c] = t;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        float t = 0.0f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w][threadIdx.x];
        g_action[(size_t)b * gact_stride + threadIdx.x] = t;
    }
    // The row's optimiser step, in the launch that completes its gradient (rollout step 0's: the later steps' launches ran
    // before it, and with step 0 `g_action + b * gact_stride` is the start of the row's H * 4 gradients): thread x owns
    // value x of the row -- for this step's four values the sum it has just stored itself.
    if (adam.act != nullptr) {
        // (value x < 4 is the sum thread x has just stored itself; the others come from the later steps' launches)
        for (int x = threadIdx.x; x < adam.n_row; x += blockDim.x) {         // any horizon: a row's H * 4 values over the block
            const size_t i = (size_t)b * adam.n_row + x;
            const int c = x & 3;
            const float l = (c == 0) ? adam.lo.x : (c == 1) ? adam.lo.y : (c == 2) ? adam.lo.z : adam.lo.w;
            const float h = (c == 0) ? adam.hi.x : (c == 1) ? adam.hi.y : (c == 2) ? adam.hi.z : adam.hi.w;
            float mi = adam.m[i], vi = adam.v[i];
            const float a = adam_update(adam.act[i], g_action[(size_t)b * gact_stride + x], mi, vi, adam.step_size,
                                        adam.bc2_sqrt, adam.b1, l, h);
            adam.m[i] = mi;
            adam.v[i] = vi;
            adam.act[i] = a;
            if (adam.act_copy != nullptr) adam.act_copy[i] = a;
        }
    }
}

// kb_sdelta's position share alone, for the trainer's pushes (drp_train_step_actions: the pushes are data, d / d actions is no
// output): g_pos[b, n, 0:3] += J_pos^T g_s_delta[n] on the real rows n < nums[b]; padded rows (collate_fn's zero rows, whose
// impulse kt_sdelta_actions sets to zero) receive nothing.  The same expressions as kb_sdelta's directions 4..6: the push's
// frame is a constant here, the hard mask a constant of the derivative (push_hard on push_frame's values: the forward's decision
// on every row, also within an ulp of u = 0 or u = L), the soft mask and both projections differentiated.
// One thread per element, no atomics.
__global__ void __launch_bounds__(256)
kb_sdelta_pos(const float* __restrict__ s_cur, size_t s_stride, const float* __restrict__ actions, size_t act_stride,
              const float* __restrict__ g_sdelta, const int* __restrict__ nums, int N, DrpCam cam, float* __restrict__ g_pos,
              size_t gpos_stride) {
    typedef Dual<3> D;
    const int b = blockIdx.x;
    const int nb = min(max(nums[b], 0), N);
    const float* act = actions + (size_t)b * act_stride;
    const float* s = s_cur + (size_t)b * s_stride;
    const float* gs = g_sdelta + (size_t)b * N * 3;
    float sc[3], ec[3];
    const float igs = 1.0f / cam.gs;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float m0 = cam.m[r * 4 + 0], m2 = cam.m[r * 4 + 2], m3 = cam.m[r * 4 + 3];
        sc[r] = (m0 * act[0] - m2 * act[1] + m3) * igs;
        ec[r] = (m0 * act[2] - m2 * act[3] + m3) * igs;
    }
    const float vx = ec[0] - sc[0], vy = ec[1] - sc[1], vz = ec[2] - sc[2];
    const float len = sqrtf(vx * vx + vy * vy + vz * vz);
    const D dx = dconst<3>(vx / len), dy = dconst<3>(vy / len), dz = dconst<3>(vz / len);
    const PushFrame fwd = push_frame(cam, act);       // kt_sdelta_actions' frame: the hard mask is decided on its values
    for (int n = threadIdx.x; n < nb; n += blockDim.x) {
        D px = dconst<3>(s[n * 3 + 0]), py = dconst<3>(s[n * 3 + 1]), pz = dconst<3>(s[n * 3 + 2]);
        px.d[0] = 1.0f; py.d[1] = 1.0f; pz.d[2] = 1.0f;
        const D rx = px - dconst<3>(sc[0]), ry = py - dconst<3>(sc[1]);
        if (!push_hard(fwd, s[n * 3 + 0], s[n * 3 + 1], s[n * 3 + 2])) continue;    // hard mask (constant), as the forward took it
        const D v = ry * dx - rx * dy;
        D pen = dconst<3>(0.0f);
        const float lo = -DRP_PUSHER_W - v.v, hi = v.v - DRP_PUSHER_W;
        if (lo > 0.0f && lo >= hi) pen = dconst<3>(-DRP_PUSHER_W) - v;
        else if (hi > 0.0f) pen = v - dconst<3>(DRP_PUSHER_W);
        const float e = expf(-pen.v / DRP_SOFT_SCALE);
        D soft = dconst<3>(e);
#pragma unroll
        for (int c = 0; c < 3; ++c) soft.d[c] = -e * pen.d[c] / DRP_SOFT_SCALE;
        const D te = (dconst<3>(ec[0]) - px) * dx + (dconst<3>(ec[1]) - py) * dy + (dconst<3>(ec[2]) - pz) * dz;
        const D base = te * soft;
        const D ox = base * dx, oy = base * dy, oz = base * dz;
        const float g0 = gs[n * 3 + 0], g1 = gs[n * 3 + 1], g2 = gs[n * 3 + 2];
        float* gp = g_pos + (size_t)b * gpos_stride + (size_t)n * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) gp[c] += g0 * ox.d[c] + g1 * oy.d[c] + g2 * oz.d[c];
    }
}

// what the weight-gradient pass of the training path needs from kmb_edge_encode, per edge slot
// (row = (b*N + i)*10 + k; every slot is written, padded ones with zero gradients)
struct KbEdgeDump {
    float* re;    // [rows,64] relation encoding relu(h3)
    float* a2;    // [rows,64] relu(h2)
    float* a1;    // [rows,64] relu(h1)
    float* x0;    // [rows,8]  the 6 encoder inputs
    float* gce;   // [rows,64] gradient at c_edge (= W_e . re + ...), rebuilt from the masks
    float* g3;    // [rows,64] gradients at the three pre-activations
    float* g2;
    float* g1;
};

// the relation encoder's position gradient from its per-slot parts (kmb_edge_encode): g_pos[j] += the sum over node j's own
// slots, in slot order, -= the sum over the edges j feeds, in the order of the reversed lists (no atomics)
__global__ void __launch_bounds__(256)
kb_gather_pos(const float* __restrict__ gpos_edge, const int* __restrict__ rev_off, const int* __restrict__ rev, int N,
              float* __restrict__ g_pos, size_t gpos_stride, const uint8_t* __restrict__ nbr_cnt,
              const float* __restrict__ g_add = nullptr /* nullable, laid out as g_pos: added first (the residual's share of the
                                                           next step's gradient) */) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const int* ro = rev_off + (size_t)b * (N + 1);
    const int* rv = rev + (size_t)b * N * DRP_K;
    const float4* ge = reinterpret_cast<const float4*>(gpos_edge) + (size_t)b * N * DRP_K;
    float* gp = g_pos + (size_t)b * gpos_stride + (size_t)j * 3;
    float g0 = gp[0], g1 = gp[1], g2 = gp[2];
    if (g_add != nullptr) {
        const float* ga = g_add + (size_t)b * gpos_stride + (size_t)j * 3;
        g0 += ga[0]; g1 += ga[1]; g2 += ga[2];
    }
    const int cnt = nbr_cnt[(size_t)b * N + j];
    float rx = 0.0f, ry = 0.0f, rz = 0.0f;
    for (int k = 0; k < cnt; ++k) {
        const float4 v = ge[(size_t)j * DRP_K + k];
        rx += v.x; ry += v.y; rz += v.z;
    }
    g0 += rx; g1 += ry; g2 += rz;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    for (int p = ro[j]; p < ro[j + 1]; ++p) {
        const float4 v = ge[rv[p]];
        ax += v.x; ay += v.y; az += v.z;
    }
    gp[0] = g0 - ax; gp[1] = g1 - ay; gp[2] = g2 - az;
}

// d loss / d s_pred as the CALLER gives it (drp_gd_grad_seeded, drp_gd_step_seeded), in kb_reward's slot of the stream: the staged
// seed [B][H][N][3] (the caller's layout) to the backward pass's step-major layout, bit for bit, on grid B x H.  The last step's
// slice goes where kb_reward writes its gradient (g_last [B,N,3]: g_state's slice H-1), the slices of the steps before it to
// g_mid [H-1][B,N,3], from where kb_gather_pos adds them (its g_add).  Where N * 3 is a multiple of four every slice starts on
// 16 bytes (the buffers do) and the copy is float4s.
__global__ void __launch_bounds__(256)
kb_seed_stage(const float* __restrict__ seed /* [B][H][N][3] */, int N, float* __restrict__ g_mid, float* __restrict__ g_last) {
    const int b = blockIdx.x, t = blockIdx.y, B = gridDim.x, H = gridDim.y;
    const int n3 = N * 3;
    const float* s = seed + ((size_t)b * H + t) * n3;
    float* g = (t == H - 1) ? g_last + (size_t)b * n3 : g_mid + ((size_t)t * B + b) * n3;
    if ((n3 & 3) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(s);
        float4* g4 = reinterpret_cast<float4*>(g);
        for (int i = threadIdx.x; i < n3 / 4; i += 256) g4[i] = s4[i];
    } else {
        for (int i = threadIdx.x; i < n3; i += 256) g[i] = s[i];
    }
}

// the same step as a launch of its own (the trainer's weights; a planner row whose gradient needs no kb_sdelta launch)
__global__ void k_adam(float* __restrict__ act, const float* __restrict__ grad, float* __restrict__ m,
                       float* __restrict__ v, int n, float step_size, float bc2_sqrt, float4 lo, float4 hi,
                       float b1 = 0.9f, float* __restrict__ act_copy = nullptr /* pinned host memory: the updated values once more */,
                       const unsigned* __restrict__ skip = nullptr /* not null and set: the gradient is not to be trusted, nothing moves */,
                       unsigned* __restrict__ skip_copy = nullptr /* pinned host memory: what `skip` held */) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && skip != nullptr && skip_copy != nullptr) *skip_copy = *skip;
    if (i >= n) return;
    if (skip != nullptr && *skip != 0u) return;
    const int c = i & 3;
    const float l = (c == 0) ? lo.x : (c == 1) ? lo.y : (c == 2) ? lo.z : lo.w;
    const float h = (c == 0) ? hi.x : (c == 1) ? hi.y : (c == 2) ? hi.z : hi.w;
    float mi = m[i], vi = v[i];
    const float a = adam_update(act[i], grad[i], mi, vi, step_size, bc2_sqrt, b1, l, h);
    m[i] = mi;
    v[i] = vi;
    act[i] = a;
    if (act_copy != nullptr) act_copy[i] = a;
}
