// GNN training samples from recorded episodes (row x4): dataset/dataset_gnn_dyn.py:86-201 (ParticleDataset.__getitem__)
// for a batch of B samples, each its own episode, frame window, radius and sampler start.
//   depth PNG (uint16) -> foreground cloud (utils.py:491-506, the float64 rule of :97-98)
//   -> fps_rad (utils.py:438-449) -> recenter in float64 (utils.py:468-477, :101)
//   -> nearest frame-0 particle (KDTree.query(k=1), :108-109) -> states / states_delta (:114-194)
//   -> the zero-padded float32 layout of collate_fn (train/train_gnn_dyn.py:20-45).
// Untracked samples straight from the depth frames (drp_ptcl_dataset_frames): the same chain on every frame of a window.  The
// count / scan / compact / meta / fps_rad / recenter kernels below index images, not samples, so that call launches them on
// the B * T images in (b, t) order with radius[b][t] and init_idx[b][t]; only the pack (k_pd_pack_frames) is its own.
// Everything the reference computes in float64 stays float64, in its evaluation order; no FMA contraction
// (-ffp-contract=off).  No atomics: every output has one order of evaluation, the same in any batch.
#pragma once
#include "drp_common.h"
#include "k_particles.h"

#define PD_CAP 4096              // the trainer's check_bn limit: a sample with more particles is an error
#define PD_PUSH 10               // per push: s_3d_cam[3], e_3d_cam[3], push_dir_cam[3], push_l

struct PdCam {
    double M[16];                // inv(opencv_T_world), row-major (dataset_gnn_dyn.py:69-78, formed on the host)
    double gs;                   // global_scale: the particles' divisor, and x 1000.0 the depth PNG's
    double fx, fy, cx, cy;
};

__device__ __forceinline__ bool pd_fg(const uint16_t* __restrict__ depth, double scale, size_t i, double& d) {
    d = (double)depth[i] / scale;                      // :97 imread(...) / (global_scale * 1000.0), float64
    return d < 0.599 / 0.8 && d > 0.0;                 // :98 first_depth < 0.599/0.8, utils.py:496 depth > 0
}

// foreground pixels per PX_TILE tile of every image: grid (tiles, B)
__global__ void __launch_bounds__(PX_BLOCK)
k_pd_count(const uint16_t* __restrict__ depth, size_t npix, double scale, unsigned long long* __restrict__ blk_cnt) {
    const int b = blockIdx.y, nblk = gridDim.x;
    const uint16_t* img = depth + (size_t)b * npix;
    const size_t base = (size_t)blockIdx.x * PX_TILE + (size_t)threadIdx.x * PX_PER_THREAD;
    int c = 0;
#pragma unroll
    for (int q = 0; q < PX_PER_THREAD; ++q) {
        double d;
        if (base + q < npix && pd_fg(img, scale, base + q, d)) ++c;
    }
    int total;
    (void)px_block_scan(c, total);
    if (threadIdx.x == 0) blk_cnt[(size_t)b * nblk + blockIdx.x] = (unsigned long long)total;
}

// row-major compaction of every image's foreground into camera-frame float64 points (utils.py:498-505), at the
// offsets of one exclusive scan over all images' tiles in order: image b's cloud is pcd[off[b*nblk] ...)
__global__ void __launch_bounds__(PX_BLOCK)
k_pd_compact(const uint16_t* __restrict__ depth, size_t npix, int w, PdCam cam,
             const unsigned long long* __restrict__ blk_off, long long cap, double* __restrict__ pcd) {
    const int b = blockIdx.y, nblk = gridDim.x;
    const uint16_t* img = depth + (size_t)b * npix;
    const double scale = cam.gs * 1000.0;
    const size_t base = (size_t)blockIdx.x * PX_TILE + (size_t)threadIdx.x * PX_PER_THREAD;
    double dv[PX_PER_THREAD];
    bool fg[PX_PER_THREAD];
    int c = 0;
#pragma unroll
    for (int q = 0; q < PX_PER_THREAD; ++q) {
        fg[q] = base + q < npix && pd_fg(img, scale, base + q, dv[q]);
        c += fg[q] ? 1 : 0;
    }
    int total;
    size_t pos = (size_t)blk_off[(size_t)b * nblk + blockIdx.x] + (size_t)px_block_scan(c, total);
#pragma unroll
    for (int q = 0; q < PX_PER_THREAD; ++q) {
        if (!fg[q] || pos >= (size_t)cap) continue;      // cap: the host's count (a disagreement is reported)
        const size_t i = base + q;
        const int py = (int)(i / (size_t)w), px = (int)(i - (size_t)py * w);
        const double d = dv[q];
        pcd[pos * 3] = (((double)px - cam.cx) * d) / cam.fx;
        pcd[pos * 3 + 1] = (((double)py - cam.cy) * d) / cam.fy;
        pcd[pos * 3 + 2] = d;
        ++pos;
    }
}

// per-image count and offset from the scan: meta[b] = n_fg, pcd_off[b]
__global__ void k_pd_meta(const unsigned long long* __restrict__ blk_off, int nblk, int B, int* __restrict__ nfg,
                          long long* __restrict__ pcd_off) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const unsigned long long lo = blk_off[(size_t)b * nblk], hi = blk_off[(size_t)(b + 1) * nblk];
    nfg[b] = (int)(hi - lo);
    pcd_off[b] = (long long)lo;
}

// fps_rad, one workgroup per sample (its own cloud, radius = 1/sqrt(den) and start).  A start outside the cloud (an empty
// foreground, a cloud beyond the host-sized buffer) samples nothing: count 0, which the host reports.  cap = PD_CAP + 1 slots, so a
// count above PD_CAP means the cap was reached.
__global__ void __launch_bounds__(1024)
k_pd_fps_rad(const double* __restrict__ pcd, long long pcd_cap, const long long* __restrict__ pcd_off, const int* __restrict__ nfg,
             const int* __restrict__ init_idx, const double* __restrict__ radius, int cap, double* __restrict__ dist,
             int* __restrict__ chosen, int* __restrict__ counts) {
    __shared__ double sval[16];
    __shared__ int sidx[16];
    __shared__ int s_last;
    const int b = blockIdx.x;
    const int n = nfg[b], init = init_idx[b];
    if (init < 0 || init >= n || pcd_off[b] + n > pcd_cap) {
        if (threadIdx.x == 0) counts[b] = 0;
        return;
    }
    const size_t off = (size_t)pcd_off[b];
    px_fps_rad_body(pcd + off * 3, n, radius[b], init, cap, dist + off, chosen + (size_t)b * cap, counts + b,
                    sval, sidx, &s_last);
}

__device__ __forceinline__ double pd_sq(const double* __restrict__ p, const double* __restrict__ q) {
    const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    return (dx * dx + dy * dy) + dz * dz;              // np.linalg.norm: sequential sum of 3 squares
}

// recenter (utils.py:468-477) in float64, r = min(0.02, 0.5 * particle_r) (:101): one wavefront per (sample, particle);
// cloud points with |p - sample| < r summed in ascending index order (numpy's axis-0 mean), divided by their count.
// out [B][n_max][3]
__global__ void __launch_bounds__(256)
k_pd_recenter(const double* __restrict__ pcd, const long long* __restrict__ pcd_off, const int* __restrict__ nfg,
              const int* __restrict__ chosen, int cap, const int* __restrict__ counts, const double* __restrict__ radius,
              int n_max, int B, double* __restrict__ out) {
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wid >= B * n_max) return;
    const int b = wid / n_max, j = wid - b * n_max;
    if (j >= counts[b]) return;
    const double* cloud = pcd + (size_t)pcd_off[b] * 3;
    const int m = nfg[b];
    const double* q = cloud + (size_t)chosen[(size_t)b * cap + j] * 3;
    const double r = fmin(0.02, 0.5 * radius[b]);
    double acc[3] = {0.0, 0.0, 0.0};
    int cnt = 0;
    for (int base = 0; base < m; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < m) in = sqrt(pd_sq(cloud + (size_t)i * 3, q)) < r;
        unsigned long long mask = __ballot(in);
        while (mask) {
            const int l = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const double* p = cloud + (size_t)(base + l) * 3;
            acc[0] += p[0]; acc[1] += p[1]; acc[2] += p[2];
            ++cnt;
        }
    }
    if (lane < 3) out[(size_t)wid * 3 + lane] = (lane == 0 ? acc[0] : (lane == 1 ? acc[1] : acc[2])) / (double)cnt;
}

// read_particles (:69-78): rows (x, y, z, 1) through inv(opencv_T_world), the first three divided by global_scale
__device__ __forceinline__ void pd_to_cam(const float* __restrict__ p4, const PdCam& cam, double* out) {
    const double x = (double)p4[0], y = (double)p4[1], z = (double)p4[2];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        out[a] = (((cam.M[a * 4] * x + cam.M[a * 4 + 1] * y) + cam.M[a * 4 + 2] * z) + cam.M[a * 4 + 3]) / cam.gs;
}

// nearest frame-0 particle of every recentered point (KDTree.query(k=1), :108-109): brute force over the sample's
// particles in float64, the lowest index on an exact tie.  grid (ceil(n_max/256), B)
__global__ void __launch_bounds__(256)
k_pd_nearest(const double* __restrict__ rec, const int* __restrict__ counts, int n_max, const float* __restrict__ ptcl,
             const long long* __restrict__ ptcl_off, const int* __restrict__ n_ptcl, PdCam cam, int* __restrict__ nearest) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_max) return;
    if (j >= counts[b]) { nearest[(size_t)b * n_max + j] = -1; return; }
    const double* q = rec + ((size_t)b * n_max + j) * 3;
    const float* P = ptcl + (size_t)ptcl_off[b];          // frame 0 of the sample: [n_ptcl][4]
    const int np = n_ptcl[b];
    double best = INFINITY;
    int arg = 0;
    for (int k = 0; k < np; ++k) {
        double p[3];
        pd_to_cam(P + (size_t)k * 4, cam, p);
        const double d = pd_sq(p, q);
        if (d < best) { best = d; arg = k; }
    }
    nearest[(size_t)b * n_max + j] = arg;
}

// states [B][T][n_max][3] = the nearest particles in every frame (:114-118), states_delta [B][T-1][n_max][3] by the push
// formula (:130-194), float32 (torch.FloatTensor), zero beyond the sample's count.  grid (ceil(n_max/256), T, B)
__global__ void __launch_bounds__(256)
k_pd_pack(const int* __restrict__ nearest, const int* __restrict__ counts, int n_max, int T, const float* __restrict__ ptcl,
          const long long* __restrict__ ptcl_off, const int* __restrict__ n_ptcl, const double* __restrict__ push, PdCam cam,
          float* __restrict__ states, float* __restrict__ sdelta) {
    const int b = blockIdx.z, t = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_max) return;
    float* so = states + (((size_t)b * T + t) * n_max + j) * 3;
    float* dout = t < T - 1 ? sdelta + (((size_t)b * (T - 1) + t) * n_max + j) * 3 : nullptr;
    if (j >= counts[b]) {
        so[0] = so[1] = so[2] = 0.0f;
        if (dout) dout[0] = dout[1] = dout[2] = 0.0f;
        return;
    }
    const int np = n_ptcl[b];
    double P[3];
    pd_to_cam(ptcl + (size_t)ptcl_off[b] + ((size_t)t * np + nearest[(size_t)b * n_max + j]) * 4, cam, P);
    so[0] = (float)P[0]; so[1] = (float)P[1]; so[2] = (float)P[2];
    if (!dout) return;
    const double* pu = push + ((size_t)b * (T - 1) + t) * PD_PUSH;
    const double* s = pu;
    const double* e = pu + 3;
    const double* dir = pu + 6;
    const double len = pu[9];
    const double pusher_w = 0.8 / 24.0;
    const double o[3] = {-dir[1], dir[0], 0.0};                              // push_dir_ortho_cam
    const double pd[3] = {P[0] - s[0], P[1] - s[1], P[2] - s[2]};           // pos_diff_cam
    const double ortho = (pd[0] * o[0] + pd[1] * o[1]) + pd[2] * o[2];     // (.. * tile(..)).sum(axis=1)
    const double proj = (pd[0] * dir[0] + pd[1] * dir[1]) + pd[2] * dir[2];
    const double lm = (proj < len && proj > 0.0) ? 1.0 : 0.0;              // hard mask
    double wm = fmax(fmax(-pusher_w - ortho, 0.0), fmax(ortho - pusher_w, 0.0));
    wm = exp(-wm / 0.01);                                                   // soft mask
    const double te = ((e[0] - P[0]) * dir[0] + (e[1] - P[1]) * dir[1]) + (e[2] - P[2]) * dir[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) dout[a] = (float)(((te * dir[a]) * lm) * wm);
}

// clouds [B * T][n_max][3] = the recentered points of every (sample, frame) image rounded once to float32
// (torch.FloatTensor), +0.0f beyond the image's count.  grid (ceil(n_max/256), B * T)
__global__ void __launch_bounds__(256)
k_pd_pack_frames(const double* __restrict__ rec, const int* __restrict__ counts, int n_max, float* __restrict__ clouds) {
    const int img = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_max) return;
    const size_t o = ((size_t)img * n_max + j) * 3;
    if (j >= counts[img]) { clouds[o] = clouds[o + 1] = clouds[o + 2] = 0.0f; return; }
    clouds[o] = (float)rec[o]; clouds[o + 1] = (float)rec[o + 1]; clouds[o + 2] = (float)rec[o + 2];
}
