// C ABI of the engine (include/drp.h): context, device workspaces, kernel pipelines -- ONE translation unit whose text lives in
// the capi_*.h sections included below (context; pipelines; then the entry points by surface: core, planner, pre-processing,
// gradient descent, training, RCCL, resolution regressor, float64 yardstick, measurement).  The propagation kernels' instantiations are translation units of their own.
// Built with: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c (this file and csrc/inst_*.hip, in parallel), then -shared
// (__graft_entry__.build)
#include "../../include/drp.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>          // types and enums only: the library itself is bound at run time (RcclApi below)

#include <dlfcn.h>
#include <link.h>
#include <sched.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "drp_common.h"
#include "k_aggregate.h"
#include "k_graph.h"
#include "k_mlp_valu.h"
#include "k_mppi.h"
#include "k_reward.h"
#include "k_backward.h"
#include "k_fps.h"
#include "k_particles.h"
#include "k_goal.h"
#include "k_train.h"
#include "k_optim.h"
#include "k_mlp_mfma.h"
#include "k_mlp_split.h"
#include "k_backward_mfma.h"
#include "k_rollout.h"
#include "k_rgr.h"
#include "k_rgr_bwd.h"
#include "k_ptcl_dataset.h"
#include "k_prop_f64.h"
#include "k_gd_f64.h"
#include "k_train_f64.h"
#include "k_chamfer.h"
#include "k_chamfer_f64.h"
#include "k_match.h"
#include "k_match_f64.h"
#include "k_sinkhorn.h"
#include "k_cloud_goal.h"
#include "k_prop_inst.h"       // km_prop / km_prop3 / km_rollout: declared here, instantiated in inst_*.hip

#include "dispatch.h"          // host-only: policy, variant flags, plan functions
#include "train_host.h"        // host-only: the trainer's staged-batch layout and push check
#include "cloud_goal_host.h"   // host-only: the cloud goal's parameter checks, eps table and row-to-column mapping
#include "ptcl_dataset_host.h" // host-only: the dataset calls' upload arena and per-image checks
#include "capi_ctx.h"
#include "capi_pipeline.h"

extern "C" {

#include "capi_core.h"
#include "capi_cloud_goal.h"
#include "capi_mpc.h"
#include "capi_prep.h"
#include "capi_gd.h"
#include "capi_train.h"
#include "capi_optim.h"
#include "capi_chamfer.h"
#include "capi_match.h"
#include "capi_transport.h"
#include "capi_divergence.h"
#include "capi_comm.h"
#include "capi_rgr.h"
#include "capi_rgr_train.h"
#include "capi_ptcl_dataset.h"
#include "capi_f64.h"
#include "capi_grad_f64.h"
#include "capi_divergence_f64.h"
#include "capi_match_f64.h"
#include "capi_debug.h"

}  // extern "C"

#ifdef ROLLOUT_STAMPS
extern "C" int drp_debug_roll_stamps(unsigned long long* out16, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out16 && hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_roll_stamps), 16 * 8) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[16] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_roll_stamps), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

#ifdef ROLLOUT_STAMPS
extern "C" int drp_debug_bwd_stamps(unsigned long long* out16, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out16 && hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_bwd_stamps), 16 * 8) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[16] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_bwd_stamps), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

#ifdef GC_STATS
extern "C" int drp_gc_stats(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(gc_stats), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[16] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(gc_stats), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
