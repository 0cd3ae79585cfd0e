// ptcl_dataset_host.h -- the dataset calls' host arithmetic that touches no device (capi_ptcl_dataset.h): where the blocks of the
// upload arena lie, and which image of a call is refused for what.  Plain C++ (no HIP header), so that
// tools/ptcl_dataset_host_check.cpp builds it alone under the host sanitizers; drp_capi.hip includes it ahead of the C ABI's sections.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#define PD_PUSH 10               // as k_ptcl_dataset.h has it: s_3d_cam[3], e_3d_cam[3], push_dir_cam[3], push_l

inline size_t pd_align(size_t x) { return (x + 255) & ~(size_t)255; }

// The upload arena (pinned staging and its device copy) of a call over n_img images of npix pixels, every block 256-byte aligned:
// depth [n_img][npix] (uint16) | particle files, ptcl_floats floats | radius [n_img] (doubles) | pushes [n_img][T-1][PD_PUSH]
// (doubles) | init_idx [n_img] | n_ptcl [n_img] (ints) | ptcl_off [n_img] (long longs).  drp_ptcl_dataset_frames has no particle
// file (ptcl_floats = 0, T = 0): those four blocks take no byte, and its upload is depth | radius | init_idx
struct PdLayout { size_t depth, ptcl, radius, push, init, nptcl, ptcl_off, bytes; };
inline PdLayout pd_layout(int n_img, size_t npix, size_t ptcl_floats = 0, int T = 0) {
    const size_t n = (size_t)n_img, per = T > 0 ? n : 0, n_push = T > 0 ? n * (T - 1) : 0;
    PdLayout L;
    size_t o = 0;
    L.depth = o; o = pd_align(o + n * npix * sizeof(uint16_t));
    L.ptcl = o; o = pd_align(o + ptcl_floats * sizeof(float));
    L.radius = o; o = pd_align(o + n * sizeof(double));
    L.push = o; o = pd_align(o + n_push * PD_PUSH * sizeof(double));
    L.init = o; o = pd_align(o + n * sizeof(int));
    L.nptcl = o; o = pd_align(o + per * sizeof(int));
    L.ptcl_off = o; o = pd_align(o + per * sizeof(long long));
    L.bytes = o;
    return L;
}

// what a call refuses an image for; the caller words the message
enum PdFault {
    PD_FINE, PD_NO_PTCL, PD_BAD_INIT, PD_BAD_RADIUS, PD_PUSH_LEN, PD_PUSH_PLANE, PD_BAD_NFG,     // before anything is launched
    PD_NO_FG, PD_NFG_DIFFERS, PD_INIT_OUTSIDE, PD_CAPPED                                         // once the device's counts are known
};
struct PdBad { int img; PdFault fault; int push; };       // push: which of the image's T - 1 pushes, for the two push faults

// The first image, in index order, that a call refuses before it launches anything, and its first fault in the fixed order n_ptcl
// -> init_idx -> radius -> each push (length, then plane: dataset_gnn_dyn.py:148-153, a zero-length push divides by zero, a push
// off the table plane exits) -> the host's foreground count.  n_ptcl and push may be null (drp_ptcl_dataset_frames: no particle
// file); push is [n_img][T-1][PD_PUSH]
inline PdBad pd_first_bad(int n_img, size_t npix, const double* radius, const int32_t* init_idx, const int32_t* n_fg_host,
                          const int32_t* n_ptcl = nullptr, const double* push = nullptr, int T = 0) {
    for (int i = 0; i < n_img; ++i) {
        if (n_ptcl && n_ptcl[i] <= 0) return {i, PD_NO_PTCL, 0};
        if (init_idx[i] < 0) return {i, PD_BAD_INIT, 0};
        if (!(radius[i] > 0.0) || !std::isfinite(radius[i])) return {i, PD_BAD_RADIUS, 0};
        for (int t = 0; push && t + 1 < T; ++t) {
            const double* pu = push + ((size_t)i * (T - 1) + t) * PD_PUSH;
            if (!(pu[9] > 0.0) || !std::isfinite(pu[9])) return {i, PD_PUSH_LEN, t};
            if (!(std::fabs(pu[8]) < 1e-6)) return {i, PD_PUSH_PLANE, t};
        }
        if (n_fg_host[i] < 0 || (size_t)n_fg_host[i] > npix) return {i, PD_BAD_NFG, 0};
    }
    return {-1, PD_FINE, 0};
}

// The same once the device's foreground counts nfg and particle counts have come back: no foreground -> the host's count
// disagrees -> the sampler's start outside the cloud -> fps_rad reached the cap of `cap` particles
inline PdBad pd_first_bad_counts(int n_img, const int* nfg, const int* counts, const int32_t* n_fg_host, const int32_t* init_idx,
                                 int cap) {
    for (int i = 0; i < n_img; ++i) {
        if (nfg[i] == 0) return {i, PD_NO_FG, 0};
        if (n_fg_host[i] != nfg[i]) return {i, PD_NFG_DIFFERS, 0};
        if (init_idx[i] >= nfg[i]) return {i, PD_INIT_OUTSIDE, 0};
        if (counts[i] > cap) return {i, PD_CAPPED, 0};
    }
    return {-1, PD_FINE, 0};
}
