// Explicit instantiations (k_prop_inst.h): this translation unit holds the device code of these kernels; csrc/drp_capi.hip launches them.
#define DRP_PROP_INSTANTIATE
#include "k_prop_inst.h"
#ifndef DRP_UNITY
KM_ROLLOUT_LIST(KM_INST_ROLLOUT_LITE)
#endif
