"""ctypes binding of the C ABI in include/drp.h.

The shared library `libdrp.so` is built in-tree by `__graft_entry__.build()` (hipcc,
gfx950).  There is no CPU fallback: if the library is missing or no GPU is present,
creating an engine raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DRP_LIB: alternative build of the same library (kernel A/B experiments)
LIB_PATH = os.environ.get('DRP_LIB') or os.path.join(_HERE, 'libdrp.so')

DRP_K = 10
DRP_F = 64
DRP_N_WEIGHTS = 38403
ENGINE_VALU = 0
ENGINE_MFMA = 1
ENGINE_SPLIT = 2
ENGINE_FUSED = 3
ENGINE_LITE = 4             # opt-in reduced products on the fused engine's kernels (include/drp.h: DRP_ENGINE_LITE)
TRAIN_MODES = {'eval': 0, 'grad': 1, 'update': 2}
LOSS_KINDS = {'chamfer': 1, 'match': 2, 'chamfer+match': 3}     # DRP_LOSS_*: drp_train_step_loss
MATCH_LOSSES = ('match', 'chamfer+match')   # the kinds with a matching: drp_train_grad_f64_match's
MATCH_MAX_POINTS = 1024     # KA_MAX_POINTS: the largest cloud of a matching
TRANSPORT_MAX_ITERS = 1000  # DRP_TRANSPORT_MAX_ITERS: the most sweeps of drp_cloud_transport / drp_train_step_transport
DIST_TRANSFORMS = {'cv5': 0, 'exact': 1}
RGR_REGRESSOR = 1           # DRP_RGR_REGRESSOR: n_out of the MPCResRgrNoPool head
RGR_CLASSIFIER = 6          # DRP_RGR_CLASSIFIER: n_out of the MPCResCls head
RGR_BMAX = 64
PD_BMAX = 1024              # drp_ptcl_dataset_batch: samples per call; drp_ptcl_dataset_frames: images (B * T) per call
PD_CAP = 4096               # particles per sample
NOISE_TYPES = {'normal': 0, 'uniform': 1, 'total_rand': 2}
ENGINES = {'valu': ENGINE_VALU, 'mfma': ENGINE_MFMA, 'split': ENGINE_SPLIT, 'fused': ENGINE_FUSED, 'lite': ENGINE_LITE}

c_float_p = ctypes.POINTER(ctypes.c_float)
c_double_p = ctypes.POINTER(ctypes.c_double)
c_int32_p = ctypes.POINTER(ctypes.c_int32)
c_int16_p = ctypes.POINTER(ctypes.c_int16)
c_uint8_p = ctypes.POINTER(ctypes.c_uint8)


class MpcParams(ctypes.Structure):
    """struct drp_mpc_params (include/drp.h)."""
    _fields_ = [('n_batch', ctypes.c_int), ('n_particles', ctypes.c_int),
                ('n_sample', ctypes.c_int), ('n_look_ahead', ctypes.c_int),
                ('sigma', ctypes.c_double), ('beta_filter', ctypes.c_double),
                ('reward_weight', ctypes.c_double),
                ('act_lo', ctypes.c_float * 4), ('act_hi', ctypes.c_float * 4),
                ('seed', ctypes.c_uint64), ('sample_offset', ctypes.c_uint64),
                ('noise_type', ctypes.c_int), ('reserved', ctypes.c_int)]


class CloudGoalParams(ctypes.Structure):
    """struct drp_cloud_goal_params (include/drp.h)."""
    _fields_ = [('kind', ctypes.c_int), ('iters', ctypes.c_int), ('weight', ctypes.c_double), ('eps_scale', ctypes.c_double)]


CLOUD_GOAL_KINDS = {'chamfer': 0, 'sinkhorn': 1}    # DRP_CLOUD_CHAMFER, DRP_CLOUD_SINKHORN
CLOUD_GOAL_MAX_POINTS = {'chamfer': 4096, 'sinkhorn': 1024}     # KC_MAX_POINTS, KT_MAX_POINTS: either cloud of a cloud goal

# name -> (restype, argtypes); exactly the symbols include/drp.h declares
SIGNATURES = {
    'drp_create': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    'drp_destroy': (None, [ctypes.c_void_p]),
    'drp_last_error': (ctypes.c_char_p, [ctypes.c_void_p]),
    'drp_sync': (ctypes.c_int, [ctypes.c_void_p]),
    'drp_set_engine': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'drp_device_info': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t,
                                       ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_size_t)]),
    'drp_load_weights': (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_size_t, ctypes.c_double]),
    'drp_set_camera': (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_float, c_float_p]),
    'drp_set_goal': (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_int, ctypes.c_int,
                                    c_float_p, ctypes.c_int]),
    'drp_distance_transform': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, c_float_p]),
    'drp_set_goal_image': (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, c_float_p, c_float_p,
                                          ctypes.POINTER(ctypes.c_int)]),
    'drp_set_goal_scenes': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_float_p, ctypes.c_int, ctypes.c_int, c_float_p,
                                           ctypes.POINTER(ctypes.c_int32), ctypes.c_int]),
    'drp_set_goal_image_scenes': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_int, c_float_p, c_float_p,
                                                 ctypes.POINTER(ctypes.c_int32)]),
    'drp_gen_s_delta': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, ctypes.c_int,
                                       ctypes.c_int, c_float_p]),
    'drp_build_graph': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, ctypes.c_int,
                                       ctypes.c_int, c_int16_p, c_uint8_p]),
    'drp_step': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p,
                                ctypes.c_int, ctypes.c_int, c_float_p]),
    'drp_forward': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p,
                                   c_int16_p, c_uint8_p, ctypes.c_int, ctypes.c_int, c_float_p]),
    'drp_rollout': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, ctypes.c_int,
                                   ctypes.c_int, c_float_p, ctypes.c_int, ctypes.c_int, c_float_p,
                                   c_float_p]),
    'drp_reward': (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_int, c_float_p]),
    'drp_reward_scenes': (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, c_float_p]),
    'drp_mpc_begin_scenes': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(MpcParams), ctypes.c_int, c_float_p,
                                            c_float_p, c_float_p, c_double_p, ctypes.POINTER(ctypes.c_uint64)]),
    'drp_mpc_stats_scenes': (ctypes.c_int, [ctypes.c_void_p, c_double_p]),
    'drp_mpc_begin': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(MpcParams), c_float_p,
                                     c_float_p, c_float_p, c_double_p]),
    'drp_mpc_sample': (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_uint64]),
    'drp_mpc_set_actions': (ctypes.c_int, [ctypes.c_void_p, c_float_p]),
    'drp_mpc_rollout': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'drp_mpc_partials': (ctypes.c_int, [ctypes.c_void_p, c_double_p]),
    'drp_mpc_update': (ctypes.c_int, [ctypes.c_void_p, c_double_p, ctypes.c_int, c_double_p]),
    'drp_mpc_update_device': (ctypes.c_int, [ctypes.c_void_p]),
    'drp_mpc_elite': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_double_p]),
    'drp_mpc_update_elite': (ctypes.c_int, [ctypes.c_void_p, c_double_p, ctypes.c_int, ctypes.c_int, c_double_p]),
    'drp_mpc_update_elite_device': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'drp_mpc_get': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p,
                                   c_double_p]),
    'drp_mpc_fetch_async': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'drp_mpc_wait': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_float_p, c_float_p]),
    'drp_fps': (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                               ctypes.POINTER(ctypes.c_int32), c_float_p]),
    'drp_train_begin': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double]),
    'drp_train_step': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_int32_p, c_float_p, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_int, c_double_p, c_float_p]),
    'drp_train_step_untracked': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_int32_p, c_float_p,
                                                ctypes.c_int, ctypes.c_int, c_float_p, c_int32_p, ctypes.c_int, ctypes.c_int,
                                                c_double_p, c_float_p]),
    'drp_train_step_actions': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_int32_p, c_float_p, ctypes.c_int,
                                              ctypes.c_int, c_float_p, c_int32_p, ctypes.c_int, ctypes.c_int, c_double_p, c_float_p]),
    'drp_train_set_lr': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double]),
    'drp_get_weights': (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_size_t]),
    'drp_depth2fgpcd': (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int,
                                       ctypes.c_int, c_double_p, c_double_p, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_int)]),
    'drp_downsample_pcd': (ctypes.c_int, [ctypes.c_void_p, c_double_p, ctypes.c_int, ctypes.c_double, c_double_p,
                                          ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    'drp_fps_pcd': (ctypes.c_int, [ctypes.c_void_p, c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_int32), ctypes.c_uint64, c_float_p, c_double_p]),
    'drp_fps_rad': (ctypes.c_int, [ctypes.c_void_p, c_double_p, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int)]),
    'drp_recenter': (ctypes.c_int, [ctypes.c_void_p, c_double_p, ctypes.c_int, c_float_p, ctypes.c_int, ctypes.c_int,
                                    c_double_p, c_float_p]),
    'drp_obs2ptcl': (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                    c_double_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int32),
                                    ctypes.c_uint64, c_double_p, c_double_p, ctypes.POINTER(ctypes.c_int),
                                    ctypes.POINTER(ctypes.c_int)]),
    'drp_gd_begin': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int,
                                    c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_float_p, c_float_p]),
    'drp_gd_begin_scenes': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_float_p, c_float_p, c_float_p, ctypes.c_int,
                                           ctypes.c_int, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_float_p,
                                           c_float_p]),
    'drp_gd_grad': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p]),
    'drp_gd_step': (ctypes.c_int, [ctypes.c_void_p, c_float_p]),
    'drp_gd_get': (ctypes.c_int, [ctypes.c_void_p, c_float_p]),
    'drp_gd_step_async': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'drp_gd_wait': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_float_p, c_float_p]),
    'drp_gd_begin_cost': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int,
                                         c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_float_p, c_float_p]),
    'drp_gd_predict': (ctypes.c_int, [ctypes.c_void_p, c_float_p]),
    'drp_gd_grad_seeded': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p]),
    'drp_gd_step_seeded': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p]),
    'drp_gd_predict_f64': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int, c_float_p,
                                          ctypes.c_int, ctypes.c_int, c_double_p]),
    'drp_gd_grad_f64_seeded': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int,
                                              c_float_p, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p]),
    'drp_mpc_begin_cost': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(MpcParams), c_float_p, c_float_p, c_float_p,
                                          c_double_p]),
    'drp_mpc_set_rewards': (ctypes.c_int, [ctypes.c_void_p, c_float_p]),
    'drp_set_goal_cloud': (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_int, ctypes.POINTER(CloudGoalParams)]),
    'drp_mpc_begin_cloud': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(MpcParams), c_float_p, c_float_p, c_float_p,
                                           c_double_p]),
    'drp_gd_begin_cloud': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int,
                                          c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_float_p, c_float_p]),
    'drp_cloud_goal_eval': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_int32_p, c_float_p, ctypes.c_int, ctypes.c_int,
                                           c_float_p, c_double_p, c_float_p]),
    'drp_comm_unique_id': (ctypes.c_int, [ctypes.c_char_p]),
    'drp_comm_init': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]),
    'drp_comm_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'drp_comm_info': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                     ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_size_t]),
    'drp_debug_stall': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'drp_comm_allgather': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    'drp_probe_begin': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    'drp_probe_read': (ctypes.c_int, [ctypes.c_void_p, c_double_p, ctypes.POINTER(ctypes.c_long)]),
    'drp_probe_prop_launches': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_long)]),
    'drp_probe_work': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong)]),
    'drp_dispatch_reset': (ctypes.c_int, [ctypes.c_void_p]),
    'drp_last_dispatch': (ctypes.c_long, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]),
    'drp_dispatch_variants': (ctypes.c_long, [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]),
    'drp_range_info': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), c_double_p, c_double_p,
                                      ctypes.POINTER(ctypes.c_int)]),
    'drp_debug_fetch': (ctypes.c_long, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p,
                                        ctypes.c_size_t]),
    'drp_rgr_load': (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_size_t, ctypes.c_int]),
    'drp_rgr_forward': (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_int, c_float_p]),
    'drp_rgr_stack': (ctypes.c_int, [ctypes.c_void_p, c_uint8_p, c_uint8_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     c_float_p]),
    'drp_rgr_infer': (ctypes.c_int, [ctypes.c_void_p, c_uint8_p, c_uint8_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     c_float_p]),
    'drp_rgr_time': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_float_p]),
    'drp_rgr_train_begin': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double]),
    'drp_rgr_train_step': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, ctypes.POINTER(ctypes.c_int32),
                                          ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double), c_float_p]),
    'drp_rgr_train_set_lr': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double]),
    'drp_rgr_get_weights': (ctypes.c_int, [ctypes.c_void_p, c_float_p, ctypes.c_size_t]),
    'drp_rgr_train_time': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_float_p]),
    'drp_ptcl_dataset_batch': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_uint16), ctypes.c_int,
                                              ctypes.c_int, ctypes.c_double, c_double_p, c_double_p, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_int32), c_float_p, c_double_p,
                                              ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), c_double_p,
                                              ctypes.POINTER(ctypes.c_int32), ctypes.c_int, c_float_p, c_float_p,
                                              ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int)]),
    'drp_ptcl_dataset_frames': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint16),
                                               ctypes.c_int, ctypes.c_int, ctypes.c_double, c_double_p, c_double_p,
                                               ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                               ctypes.POINTER(ctypes.c_int32), ctypes.c_int, c_float_p,
                                               ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int)]),
    'drp_ptcl_dataset_time': (ctypes.c_int, [ctypes.c_void_p, c_float_p]),
    'drp_forward_f64': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p,
                                       c_int16_p, c_uint8_p, ctypes.c_int, ctypes.c_int, c_double_p]),
    'drp_step_f64': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p,
                                    ctypes.c_int, ctypes.c_int, c_double_p]),
    'drp_f64_tap': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, c_double_p, ctypes.c_size_t]),
    'drp_debug_set_f64_cap': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t]),
    'drp_accuracy_probe': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_float_p, c_float_p, c_float_p, c_float_p,
                                          ctypes.c_int, ctypes.c_int, c_double_p]),
    'drp_gd_grad_f64': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int, c_float_p,
                                       ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p]),
    'drp_train_grad_f64': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_int32_p, c_float_p, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p]),
    'drp_train_grad_f64_actions': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_int32_p, c_float_p,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p,
                                                  c_double_p]),
    'drp_cloud_chamfer': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_int32_p, c_float_p, c_int32_p, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, c_double_p, c_float_p, c_int32_p, c_int32_p]),
    'drp_train_grad_f64_untracked': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_int32_p,
                                                    c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_float_p, c_int32_p,
                                                    ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    'drp_cloud_chamfer_f64': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_int32_p, c_float_p, c_int32_p, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_int32_p, c_int32_p, c_double_p]),
    'drp_cloud_match': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_int32_p, c_float_p, c_int32_p, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, c_double_p, c_float_p, c_int32_p, c_int32_p, c_double_p]),
    'drp_train_step_loss': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_int32_p, c_float_p,
                                           ctypes.c_int, ctypes.c_int, c_float_p, c_int32_p, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_double, ctypes.c_int, c_double_p, c_float_p, c_int32_p]),
    'drp_train_predict': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_int32_p, c_float_p,
                                         ctypes.c_int, ctypes.c_int, c_float_p]),
    'drp_train_step_seeded': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_int32_p, c_float_p,
                                             ctypes.c_int, ctypes.c_int, c_float_p, ctypes.c_int, c_float_p]),
    'drp_train_predict_f64': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_int32_p, c_float_p,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p]),
    'drp_train_grad_f64_seeded': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_int32_p, c_float_p,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p]),
    'drp_cloud_transport': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_int32_p, c_float_p, c_int32_p, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, c_float_p, c_double_p, c_double_p]),
    'drp_train_step_transport': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_int32_p, c_float_p,
                                                ctypes.c_int, ctypes.c_int, c_float_p, c_int32_p, ctypes.c_int, c_double_p,
                                                ctypes.c_int, ctypes.c_int, c_double_p, c_float_p, c_double_p]),
    'drp_cloud_divergence': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_int32_p, c_float_p, c_int32_p, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, c_float_p, c_double_p, c_double_p,
                                            c_double_p]),
    'drp_train_step_divergence': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_int32_p, c_float_p,
                                                 ctypes.c_int, ctypes.c_int, c_float_p, c_int32_p, ctypes.c_int, c_double_p,
                                                 ctypes.c_int, ctypes.c_int, c_double_p, c_float_p, c_double_p, c_double_p]),
    'drp_cloud_divergence_unbalanced': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_int32_p, c_float_p, c_int32_p, ctypes.c_int,
                                                       ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p, ctypes.c_int,
                                                       c_double_p, c_float_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    'drp_train_step_divergence_unbalanced': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_int32_p,
                                                            c_float_p, ctypes.c_int, ctypes.c_int, c_float_p, c_int32_p, ctypes.c_int,
                                                            c_double_p, c_double_p, c_double_p, ctypes.c_int, ctypes.c_int, c_double_p,
                                                            c_float_p, c_double_p, c_double_p, c_double_p]),
    'drp_cloud_divergence_f64': (ctypes.c_int, [ctypes.c_void_p, c_double_p, c_int32_p, c_float_p, c_int32_p, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, c_double_p,
                                                c_double_p, c_double_p, c_double_p]),
    'drp_cloud_divergence_unbalanced_f64': (ctypes.c_int, [ctypes.c_void_p, c_double_p, c_int32_p, c_float_p, c_int32_p, ctypes.c_int,
                                                           ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p, ctypes.c_int,
                                                           c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    'drp_train_grad_f64_divergence_unbalanced': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_int32_p,
                                                                c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_float_p,
                                                                c_int32_p, ctypes.c_int, c_double_p, c_double_p, c_double_p,
                                                                ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p,
                                                                c_double_p, c_double_p, c_double_p]),
    'drp_train_grad_f64_divergence': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_int32_p,
                                                     c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_float_p, c_int32_p,
                                                     ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, c_double_p, c_double_p,
                                                     c_double_p, c_double_p, c_double_p]),
    'drp_cloud_match_f64': (ctypes.c_int, [ctypes.c_void_p, c_double_p, c_int32_p, c_float_p, c_int32_p, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, c_int32_p, c_double_p, c_double_p, c_int32_p, c_int32_p, c_double_p,
                                           c_double_p]),
    'drp_train_grad_f64_match': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, c_float_p, c_float_p, c_int32_p, c_float_p,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_int, c_float_p, c_int32_p, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_double, c_int32_p, c_double_p, c_double_p, c_double_p,
                                                c_double_p, c_int32_p, c_double_p, c_double_p]),
    'drp_train_accumulate': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double]),
    'drp_train_apply': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, c_double_p, c_double_p,
                                       ctypes.POINTER(ctypes.c_int), c_float_p]),
    'drp_train_get_state': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, ctypes.POINTER(ctypes.c_int64)]),
    'drp_train_set_state': (ctypes.c_int, [ctypes.c_void_p, c_float_p, c_float_p, ctypes.c_int64]),
}

_lib = None


DRP_ERANGE = -6
MAX_SCENES = 64             # DRP_MAX_SCENES


class DrpError(RuntimeError):
    pass


class DrpRangeError(DrpError):
    """DRP_ERANGE: weights or inputs outside the range the split-fp16 relation encoder is scaled for (include/drp.h)."""


def load():
    """Load libdrp.so and bind every declared symbol.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DrpError('HIP extension %s is missing: run `python -c "import __graft_entry__ as g; '
                       'g.build()"` (there is no CPU fallback)' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)        # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
