"""numpy-facing wrapper of one C-ABI context (one GPU, one HIP stream)."""
import ctypes
import types

import numpy as np

from . import _lib as L


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def _f64(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def _fp(a):
    return a.ctypes.data_as(L.c_float_p)


def _dp(a):
    return a.ctypes.data_as(L.c_double_p)


def _i32(x):
    return np.ascontiguousarray(x, dtype=np.int32)


def _ip(a):
    return a.ctypes.data_as(L.c_int32_p)


def _opt(f, a):
    """f(a), or None for an argument that is not given"""
    return None if a is None else f(a)


_POINTERS = {np.dtype(np.float32): _fp, np.dtype(np.float64): _dp, np.dtype(np.int32): _ip}


def _ptr(a):
    """an array's ctypes pointer by its dtype; None and plain numbers pass through"""
    return _POINTERS[a.dtype](a) if isinstance(a, np.ndarray) else a


def _per_sample(x, B):
    """a number or [B] -> float64 [B] (eps, reach)"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float64).reshape(-1), (B,)))


def _per_step(x, H, B):
    """a number, [B] or [H, B] -> float64 [H, B] (mass_q)"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(x, np.float64), (H, B)))


def _impulses(states_delta, actions, exactly_one=True):
    """a trainer call's impulse source -> (by_actions, the array _train_batch takes for it); exactly_one: giving both or neither
    is refused (the float64 calls ignore states_delta beside actions instead)"""
    if exactly_one and (states_delta is None) == (actions is None):
        raise ValueError('exactly one of states_delta and actions must be given')
    by_actions = actions is not None
    return by_actions, _f32(actions) if by_actions else states_delta


def _source_args(by_actions, impulses):
    """the C ABI's (states_delta, actions) argument pair"""
    return (None, impulses) if by_actions else (impulses, None)


def _compare_blobs(g32, g64):
    """an fp32 gradient blob against its float64 yardstick, per tensor -> ({state_dict key: {'max_abs_err', 'max_abs_ref', 'rel' =
    err / max(ref, 1e-300)}}, the key of the largest rel); NaN counts as +inf"""
    from .weights import STATE_DICT_KEYS
    tensors, off, worst = {}, 0, None
    for key, shape in STATE_DICT_KEYS:
        n = int(np.prod(shape))
        err = np.abs(g32[off:off + n].astype(np.float64) - g64[off:off + n])
        err = float(np.where(np.isnan(err), np.inf, err).max())
        ref = float(np.abs(g64[off:off + n]).max())
        tensors[key] = {'max_abs_err': err, 'max_abs_ref': ref, 'rel': err / max(ref, 1e-300)}
        if worst is None or tensors[key]['rel'] > tensors[worst]['rel']:
            worst = key
        off += n
    return tensors, worst


# ---- the row layout of a multi-scene session (include/drp.h: drp_mpc_begin_scenes; pure numpy, no device, no library) --------
def scene_rows(S, n_units, nb):
    """Rows of every scene in a session of S scenes x n_units samples (or trajectories) x nb columns -> int64 [S, n_units * nb]:
    scene s's rows in the order a single-scene session numbers them (unit * nb + column).  The layout is planners.py:661-662
    with S * nb columns: row = (unit * S + scene) * nb + column, so scene(row) = (row // nb) % S and row % (S * nb) is the
    start column."""
    S, n_units, nb = int(S), int(n_units), int(nb)
    if S < 1 or n_units < 1 or nb < 1:
        raise ValueError('scene_rows needs S, n_units, nb >= 1, got %d, %d, %d' % (S, n_units, nb))
    u = np.arange(n_units, dtype=np.int64)[None, :, None]
    k = np.arange(S, dtype=np.int64)[:, None, None]
    c = np.arange(nb, dtype=np.int64)[None, None, :]
    return ((u * S + k) * nb + c).reshape(S, n_units * nb)


def interleave_scenes(per_scene, nb):
    """S per-scene arrays [n_units * nb, ...] (a sequence, or an array [S, n_units * nb, ...]) -> the session's array
    [n_units * S * nb, ...] (scene_rows' layout)."""
    a = np.asarray(per_scene)
    if a.ndim < 2 or a.shape[1] % int(nb) != 0:
        raise ValueError('interleave_scenes needs [S, n_units * nb, ...] with nb = %d, got %s' % (int(nb), a.shape))
    S, rows = a.shape[0], a.shape[1]
    out = np.empty((S * rows,) + a.shape[2:], a.dtype)
    out[scene_rows(S, rows // int(nb), nb).reshape(-1)] = a.reshape((S * rows,) + a.shape[2:])
    return out


def split_scenes(session, S, nb):
    """The inverse of interleave_scenes: a session array [n_units * S * nb, ...] -> [S, n_units * nb, ...]."""
    a = np.asarray(session)
    if a.ndim < 1 or a.shape[0] % (int(S) * int(nb)) != 0:
        raise ValueError('split_scenes needs [n_units * S * nb, ...] with S = %d, nb = %d, got %s' % (int(S), int(nb), a.shape))
    return a[scene_rows(S, a.shape[0] // (int(S) * int(nb)), nb)]


_DEFAULT = {}


def default_engine(device=0):
    """The process's ONE context of a device, created on first use: what the reference-named mirrors (the model of
    gnn_dyn.py, the helpers of utils.py, config_reward_ptcl of flex_rewards.py) run on unless they are handed an Engine --
    one stream, one set of workspaces, one installed camera, as the reference's modules share one CUDA device.  It
    serves what its fused engine refuses (DRP_ERANGE) on the fp32 matrix engine by itself (`auto_engine`)."""
    device = int(device)
    eng = _DEFAULT.get(device)
    if eng is None or getattr(eng, 'h', None) is None:
        eng = _DEFAULT[device] = Engine(device, auto_engine=True)
    return eng


def set_default_engine(engine):
    """Make `engine` the context default_engine(engine.device) returns (None: forget it)."""
    if engine is None:
        _DEFAULT.clear()
    else:
        _DEFAULT[int(engine.device)] = engine


class Engine(object):
    """Owns a `drp_ctx`.  Every method takes/returns numpy arrays (fp32).

    auto_engine: a call the fused (or split) engine refuses with DRP_ERANGE -- weights with an entry beyond fp16, inputs
    whose proven activation bound leaves it: include/drp.h -- is repeated on the fp32 matrix engine (`mfma`), which has no
    such limit; the engine stays switched until other weights are loaded, and a warning is issued.  (The gradient-descent
    planner and the trainer choose their tape's engine by themselves -- include/drp.h, drp_gd_begin -- and never raise it.)"""

    def __init__(self, device=0, engine=None, auto_engine=False):
        self.lib = L.load()
        h = ctypes.c_void_p()
        rc = self.lib.drp_create(int(device), ctypes.byref(h))
        if rc != 0:
            raise L.DrpError('drp_create(device=%d) failed (%d): %s' %
                             (device, rc, self.lib.drp_last_error(None).decode()))
        self.h = h
        self.device = int(device)
        self.H = 0
        self.auto_engine = bool(auto_engine)
        self.engine_id = self.chosen_engine = L.ENGINE_FUSED     # drp_create's choice
        if engine is not None:
            self.set_engine(engine)

    def close(self):
        if getattr(self, 'h', None):
            self.lib.drp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc < 0:
            msg = 'drp error %d: %s' % (rc, self.lib.drp_last_error(self.h).decode())
            raise (L.DrpRangeError if rc == L.DRP_ERANGE else L.DrpError)(msg)
        return rc

    def _ranged(self, call):
        """`call()` -> return code of an entry point that checks the split engine's range."""
        try:
            return self._ck(call())
        except L.DrpRangeError as e:
            if not self.auto_engine or self.engine_id not in (L.ENGINE_FUSED, L.ENGINE_SPLIT, L.ENGINE_LITE):
                raise
            import warnings
            warnings.warn('the split-fp16 engine refused the call (%s): continuing on the fp32 matrix engine' % e,
                          RuntimeWarning, stacklevel=3)
            self._give_way(L.ENGINE_MFMA)               # undone by the next load_weights: the refusal belongs to these weights / inputs
            return self._ck(call())

    # ---- constants ----------------------------------------------------------------
    def set_engine(self, engine):
        """engine: an id or a name of _lib.ENGINES.  'lite' (reduced products on the fused engine's kernels, forward calls only:
        include/drp.h) is never chosen for the caller; load_weights(probe=..., max_disp_rel=...) is its guard."""
        if isinstance(engine, str):
            engine = L.ENGINES[engine]
        self._give_way(engine)
        self.chosen_engine = int(engine)              # the caller's choice: written here and nowhere else

    def _give_way(self, engine):
        """run on `engine` without touching the caller's choice (a range refusal, a probe finding): load_weights returns to it"""
        self._ck(self.lib.drp_set_engine(self.h, int(engine)))
        self.engine_id = int(engine)

    def device_info(self):
        name = ctypes.create_string_buffer(256)
        ncu = ctypes.c_int()
        mem = ctypes.c_size_t()
        self._ck(self.lib.drp_device_info(self.h, name, 256, ctypes.byref(ncu), ctypes.byref(mem)))
        return {'name': name.value.decode(), 'n_cu': ncu.value, 'hbm_bytes': mem.value}

    def load_weights(self, blob, adj_thresh=0.08, probe=None, max_disp_rel=None, max_grad_rel=None):
        """probe: None (nothing measured), True (the fixed batch of `probe_batch`; the camera must be set) or a batch
        (a_cur, s_cur, s_delta, dens): after loading, the selected engine's one-step error against the float64 evaluation is
        measured on it (`accuracy_probe`) and kept for `range_info()['probe']`.  max_disp_rel: the largest error, as a share
        of the largest displacement, the caller accepts -- beyond it the fused / split engine gives way to the fp32 matrix
        engine exactly as after DRP_ERANGE (one RuntimeWarning; the next load_weights restores the choice), whatever
        `auto_engine` says, and on the fp32 engines, which have nowhere to fall back to, DrpError is raised.  The lite engine
        gives way to the fused one first (one RuntimeWarning), which is then probed and held to the same threshold in turn;
        `range_info()['probe']` names the engine whose figures it holds.
        max_grad_rel: the same guard for the quantity the gradient-descent planner consumes.  After the forward probe (if one
        was asked for) `gradient_probe` runs on `probe_batch`'s pile under its eight pushes (nb = 1, B = 8, H = 1) with the
        context's camera and goal -- both must be set: ValueError otherwise, the probe invents no goal -- and is kept as
        `range_info()['grad_probe']`.  Beyond max_grad_rel on a split-fp16 tape the engine gives way to the fp32 matrix engine
        (one RuntimeWarning, the next load_weights restores the choice), so the tape is fp32; that tape is probed in turn, and
        beyond the threshold there too DrpError is raised.  The gradient probe ends a running planner session."""
        blob = _f32(blob).ravel()
        if max_disp_rel is not None and probe is None:
            raise ValueError('max_disp_rel needs a probe (probe=True or a batch)')
        if max_grad_rel is not None and not (hasattr(self, '_cam') and getattr(self, '_have_goal', False)):
            raise ValueError('max_grad_rel needs the camera and a goal (set_camera, set_goal / set_goal_image): the gradient '
                             'probe differentiates the reward of the context\'s own goal')
        self._weights_owner = None                    # whoever believed its weights were resident no longer is right
        self._ck(self.lib.drp_load_weights(self.h, _fp(blob), blob.size, float(adj_thresh)))
        if self.engine_id != self.chosen_engine:
            # the fallback was for the OTHER weights: these get the chance of the engine the caller had chosen again
            self._give_way(self.chosen_engine)
        self._probe = self._grad_probe = None
        if probe is not None:
            self._forward_guard(self.probe_batch() if probe is True else tuple(probe), max_disp_rel)
        if max_grad_rel is not None:
            self._gradient_guard(max_grad_rel)

    def _gradient_guard(self, max_grad_rel):
        import warnings
        from . import synthetic as syn
        s0, dens, attr = syn.make_pile(64, 1, seed=0)
        acts = syn.sample_pushes(8, 1, seed=0)
        lo, hi = syn.action_limits()
        while True:
            res = self.gradient_probe(s0, attr, dens, acts, lo, hi)
            self._grad_probe = dict(res)
            if res['rel'] <= max_grad_rel:
                return
            msg = ('the %s tape\'s gradient is %.3e of its largest component away from the float64 evaluation on these weights '
                   '(component %d), beyond the %.3e asked for' % (res['tape'], res['rel'], res['worst'], max_grad_rel))
            if res['tape'] != 'fused':
                raise L.DrpError(msg + ': the fp32 tape has nowhere to fall back to')
            warnings.warn(msg + ': continuing on the fp32 matrix engine', RuntimeWarning, stacklevel=3)
            self._give_way(L.ENGINE_MFMA)             # undone by the next load_weights: the finding belongs to these weights

    def _forward_guard(self, batch, max_disp_rel):
        import warnings
        names = dict((v, k) for k, v in L.ENGINES.items())
        while True:
            res = self.accuracy_probe(*batch)         # (a refusal of the range check is handled as every ranged call's)
            self._probe = dict(res, engine=names[self.engine_id])
            if max_disp_rel is None or res['disp_rel'] <= max_disp_rel:
                return
            msg = ('the %s engine is %.3e of the largest displacement away from the float64 evaluation on these weights '
                   '(particle %d), beyond the %.3e asked for' % (names[self.engine_id], res['disp_rel'], res['worst'], max_disp_rel))
            if self.engine_id not in (L.ENGINE_FUSED, L.ENGINE_SPLIT, L.ENGINE_LITE):
                raise L.DrpError(msg + ': the fp32 engines have nowhere to fall back to')
            # lite gives way to the full products of the same kernels, and those, like the split engine, to fp32
            nxt = L.ENGINE_FUSED if self.engine_id == L.ENGINE_LITE else L.ENGINE_MFMA
            warnings.warn(msg + ': continuing on the %s engine' % ('fused' if nxt == L.ENGINE_FUSED else 'fp32 matrix'),
                          RuntimeWarning, stacklevel=3)
            self._give_way(nxt)                       # undone by the next load_weights: the finding belongs to these weights
            if nxt == L.ENGINE_MFMA:
                return

    def probe_batch(self):
        """The fixed batch of load_weights(probe=True): 8 samples x 64 particles, one pile and eight pushes of the synthetic
        scene, seed 0, through gen_s_delta (so the camera must be set) -> (a_cur, s_cur, s_delta, dens)."""
        from . import synthetic as syn
        s0, dens, attr = syn.make_pile(64, 1, seed=0)
        acts = syn.sample_pushes(8, 1, seed=0)[:, 0]
        s = np.repeat(s0, 8, axis=0)
        return np.repeat(attr, 8, axis=0), s, self.gen_s_delta(s, acts), np.repeat(dens, 8)

    def set_camera(self, m34, global_scale, intr):
        m34 = _f32(m34).ravel()
        intr = _f32(intr).ravel()
        assert m34.size == 12 and intr.size == 4
        self._cam = (m34.copy(), float(global_scale))
        self._ck(self.lib.drp_set_camera(self.h, _fp(m34), float(global_scale), _fp(intr)))

    def set_camera_intrinsics(self, intr):
        """Change [fx,fy,cx,cy] only (the reward's projection), keeping the extrinsic map."""
        m34, gs = getattr(self, '_cam', (np.eye(3, 4, dtype=np.float32).ravel(), 1.0))
        self.set_camera(m34, gs, intr)

    def set_goal(self, field, goal_coor):
        field = _f32(field)
        goal_coor = _f32(goal_coor)
        assert field.ndim == 2 and goal_coor.ndim == 2 and goal_coor.shape[1] == 2
        self._ck(self.lib.drp_set_goal(self.h, _fp(field), field.shape[0], field.shape[1],
                                       _fp(goal_coor), goal_coor.shape[0]))
        self._have_goal = True

    def distance_transform(self, src, mode='cv5'):
        """cv2.distanceTransform(src, cv2.DIST_L2, 5) on the device ('cv5': OpenCV's 5x5 chamfer;
        'exact': Euclidean) -> [h,w] float32."""
        src = np.ascontiguousarray(np.asarray(src) != 0, dtype=np.uint8)
        out = np.empty(src.shape, np.float32)
        self._ck(self.lib.drp_distance_transform(self.h, src.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                                 src.shape[0], src.shape[1], L.DIST_TRANSFORMS[mode], _fp(out)))
        return out

    # ---- resolution regressor (model/res_regressor.py; include/drp.h drp_rgr_*) -----------------------------------
    rgr_n_out = 0
    rgr_owner = None

    def rgr_load(self, blob, n_out):
        """state_dict blob (res_regressor.blob_from_state_dict) of the regressor (n_out 1) or the classifier (n_out 6)."""
        b = _f32(blob).reshape(-1)
        self.rgr_owner = None         # the res_regressor model whose weights the context holds (set by that model)
        self._ck(self.lib.drp_rgr_load(self.h, _fp(b), b.size, int(n_out)))
        self.rgr_n_out = int(n_out)
        self._rgr_lastB = 0

    def rgr_forward(self, x):
        """x [B,6,224,224], 1 <= B <= 64 -> [B,n_out]"""
        a = _f32(x)
        B = a.shape[0] if a.ndim == 4 else 0
        out = np.empty((max(B, 1), max(self.rgr_n_out, 1)), np.float32)
        self._ck(self.lib.drp_rgr_forward(self.h, _fp(a), int(B), _fp(out)))
        self._rgr_lastB = B
        return out

    def _rgr_masks(self, init, goal):
        a = np.ascontiguousarray(init, dtype=np.uint8)
        g = np.ascontiguousarray(goal, dtype=np.uint8)
        assert a.shape == g.shape and a.ndim == 2, (a.shape, g.shape)
        return a, g, a.ctypes.data_as(L.c_uint8_p), g.ctypes.data_as(L.c_uint8_p)

    def rgr_stack(self, init, goal, mode='cv5'):
        """the [6,224,224] input stack of infer_param from two 0/1 masks [h,w] (h, w >= 224)"""
        a, g, pa, pg = self._rgr_masks(init, goal)
        out = np.empty((6, 224, 224), np.float32)
        self._ck(self.lib.drp_rgr_stack(self.h, pa, pg, a.shape[0], a.shape[1], L.DIST_TRANSFORMS[mode], _fp(out)))
        return out

    def rgr_infer(self, init, goal, mode='cv5'):
        """stack + forward of one mask pair -> the head's outputs [n_out]"""
        a, g, pa, pg = self._rgr_masks(init, goal)
        out = np.empty(max(self.rgr_n_out, 1), np.float32)
        self._ck(self.lib.drp_rgr_infer(self.h, pa, pg, a.shape[0], a.shape[1], L.DIST_TRANSFORMS[mode], _fp(out)))
        self._rgr_lastB = 1
        return out

    def rgr_time(self, B, iters=20, parts=7):
        """device ms of each of `iters` forward passes at batch B (parts: 1 convolutions, 2 FC1, 4 FC2..head, summed)"""
        ms = np.empty(int(iters), np.float32)
        self._ck(self.lib.drp_rgr_time(self.h, int(parts), int(B), int(iters), _fp(ms)))
        return ms

    def rgr_train_begin(self, lr, beta1=0.9, lam_reg=0.0):
        """Adam state for the loaded regressor (zeroed, t = 0): torch.optim.Adam(lr, betas=(beta1, 0.999)) and the L1 weight
        lam_reg of train/train_res_rgr.py:170-183"""
        self._ck(self.lib.drp_rgr_train_begin(self.h, float(lr), float(beta1), float(lam_reg)))

    def rgr_train_step(self, x, y=None, conf=None, label=None, mode='update', want_grad=False):
        """x [B,6,224,224]; y [B] and conf [B] (regressor) or label [B] in 0..5 (classifier); mode 'eval' | 'grad' | 'update'
        -> ((loss, mse|ce, reg) before any update, gradient blob in state_dict order or None; want_grad needs mode 'grad')"""
        a = _f32(x)
        B = a.shape[0] if a.ndim == 4 else 0
        yp = cp = lp = None
        if y is not None:
            y = _f32(y).reshape(-1)
            yp = _fp(y)
        if conf is not None:
            conf = _f32(conf).reshape(-1)
            cp = _fp(conf)
        if label is not None:
            label = np.ascontiguousarray(label, dtype=np.int32).reshape(-1)
            lp = label.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        for v in (y, conf, label):
            if v is not None and v.size != B:
                raise ValueError('target of %d values for a batch of %d' % (v.size, B))
        loss = np.zeros(3, np.float64)
        grad = None
        if want_grad:
            from .res_regressor import n_floats
            grad = np.empty(n_floats(max(self.rgr_n_out, 1)), np.float32)
        self._ck(self.lib.drp_rgr_train_step(self.h, _fp(a), yp, cp, lp, int(B), L.TRAIN_MODES[mode], _dp(loss),
                                             _fp(grad) if grad is not None else None))
        self._rgr_lastB = B
        return (float(loss[0]), float(loss[1]), float(loss[2])), grad

    def rgr_train_set_lr(self, lr):
        self._ck(self.lib.drp_rgr_train_set_lr(self.h, float(lr)))

    def rgr_get_weights(self):
        """the regressor's device weights as a blob in state_dict order, torch layouts"""
        from .res_regressor import n_floats
        out = np.empty(n_floats(max(self.rgr_n_out, 1)), np.float32)
        self._ck(self.lib.drp_rgr_get_weights(self.h, _fp(out), out.size))
        return out

    def rgr_train_time(self, B, iters=10):
        """device ms [iters, 3] of back-to-back UPDATE steps on the last training step's inputs (batch B): forward | loss + FC
        backward with FC1's Adam step | conv backward + the other parameters' Adam step.  The steps move the weights."""
        ms = np.empty((int(iters), 3), np.float32)
        self._ck(self.lib.drp_rgr_train_time(self.h, int(B), int(iters), _fp(ms)))
        return ms

    def rgr_tap(self, name):
        """post-activation tap of the last regressor forward: 'c1'..'c5' -> [B,C,H,W] (torch's layout), 'f1'..'f4' -> [B,F]"""
        B = getattr(self, '_rgr_lastB', 0)
        if name[0] == 'c':
            l = int(name[1]) - 1
            hw, ch = 112 >> l, (64, 128, 256, 512, 512)[l]
            return self.debug_fetch('rgr_' + name, (B, hw, hw, ch)).transpose(0, 3, 1, 2).copy()
        return self.debug_fetch('rgr_' + name, (B, (4096, 1024, 256, 64)[int(name[1]) - 1]))

    def set_goal_image(self, obs_goal, max_goal_pts, fps_init=0, mode='cv5', want=False):
        """Goal field (env/flex_rewards.py:172-177) and goal pixel subsample (planners.py:620-624) from
        the goal distance image, computed and kept on the device.  want=True also returns
        (field [h,w], goal_coor [m,2])."""
        g = _f32(obs_goal)
        assert g.ndim == 2
        m = ctypes.c_int()
        if not want:
            self._ck(self.lib.drp_set_goal_image(self.h, _fp(g), g.shape[0], g.shape[1], L.DIST_TRANSFORMS[mode],
                                                 int(max_goal_pts), int(fps_init), None, None, ctypes.byref(m)))
            self._have_goal = True
            return m.value
        field = np.empty(g.shape, np.float32)
        coor = np.empty((int(max_goal_pts), 2), np.float32)
        self._ck(self.lib.drp_set_goal_image(self.h, _fp(g), g.shape[0], g.shape[1], L.DIST_TRANSFORMS[mode],
                                             int(max_goal_pts), int(fps_init), _fp(field), _fp(coor),
                                             ctypes.byref(m)))
        self._have_goal = True
        return field, coor[:m.value].copy()

    # ---- the goal table of multi-scene sessions (include/drp.h: drp_set_goal_scenes) ------------------------------------
    scene_rows = staticmethod(scene_rows)
    interleave_scenes = staticmethod(interleave_scenes)
    split_scenes = staticmethod(split_scenes)

    def set_goal_scenes(self, fields, goal_coor, m=None):
        """S goals of one image size beside the single goal: fields [S,h,w]; goal_coor either a sequence of S arrays [m_s,2]
        (padded here to the longest) or an array [S,m_max,2] with the counts m [S]."""
        fields = _f32(fields)
        assert fields.ndim == 3
        S = fields.shape[0]
        if m is None:
            parts = [_f32(g) for g in goal_coor]
            assert len(parts) == S and all(g.ndim == 2 and g.shape[1] == 2 for g in parts)
            m = np.array([g.shape[0] for g in parts], np.int32)
            coor = np.zeros((S, max(int(m.max()) if S else 0, 1), 2), np.float32)
            for k, g in enumerate(parts):
                coor[k, :g.shape[0]] = g
        else:
            coor = _f32(goal_coor)
            m = np.ascontiguousarray(m, dtype=np.int32).reshape(-1)
            assert coor.ndim == 3 and coor.shape[0] == S and coor.shape[2] == 2 and m.shape == (S,)
        self._ck(self.lib.drp_set_goal_scenes(self.h, int(S), _fp(fields), fields.shape[1], fields.shape[2], _fp(coor),
                                              m.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), coor.shape[1]))
        self._goal_scenes = int(S)

    def set_goal_image_scenes(self, obs_goals, max_goal_pts, fps_init=0, mode='cv5', want=False):
        """set_goal_image for S goal distance images [S,h,w] into the goal table: slot s gets the bits set_goal_image gives for
        obs_goals[s].  -> the counts m [S]; want=True: (fields [S,h,w], [goal_coor_s [m_s,2] for every scene])."""
        g = _f32(obs_goals)
        assert g.ndim == 3
        S = g.shape[0]
        m = np.zeros(max(S, 1), np.int32)
        field = np.empty(g.shape, np.float32) if want else None
        coor = np.empty((S, int(max_goal_pts), 2), np.float32) if want else None
        self._ck(self.lib.drp_set_goal_image_scenes(self.h, int(S), _fp(g), g.shape[1], g.shape[2], L.DIST_TRANSFORMS[mode],
                                                    int(max_goal_pts), int(fps_init), _fp(field) if want else None,
                                                    _fp(coor) if want else None, m.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        self._goal_scenes = int(S)
        if not want:
            return m[:S].copy()
        return field, [coor[k, :m[k]].copy() for k in range(S)]

    def reward_scenes(self, state, scene, normalize=True):
        """reward() with a goal per row: state [Bp,N,3], scene [Bp] indices into the goal table -> [Bp]"""
        state = _f32(state)
        Bp, N, _ = state.shape
        scene = np.ascontiguousarray(scene, dtype=np.int32).reshape(-1)
        assert scene.shape == (Bp,)
        out = np.empty((Bp,), dtype=np.float32)
        self._ck(self.lib.drp_reward_scenes(self.h, _fp(state), scene.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), Bp, N,
                                            int(bool(normalize)), _fp(out)))
        return out

    # ---- single operations --------------------------------------------------------
    def gen_s_delta(self, s_cur, action):
        s_cur, action = _f32(s_cur), _f32(action)
        B, N, _ = s_cur.shape
        assert action.shape == (B, 4)
        out = np.empty((B, N, 3), dtype=np.float32)
        self._ck(self.lib.drp_gen_s_delta(self.h, _fp(s_cur), _fp(action), B, N, _fp(out)))
        return out

    def build_graph(self, s_cur, s_delta):
        s_cur, s_delta = _f32(s_cur), _f32(s_delta)
        B, N, _ = s_cur.shape
        idx = np.empty((B, N, L.DRP_K), dtype=np.int16)
        cnt = np.empty((B, N), dtype=np.uint8)
        self._ck(self.lib.drp_build_graph(self.h, _fp(s_cur), _fp(s_delta), B, N,
                                          idx.ctypes.data_as(L.c_int16_p),
                                          cnt.ctypes.data_as(L.c_uint8_p)))
        return idx, cnt

    def step(self, a_cur, s_cur, s_delta, dens):
        a_cur, s_cur, s_delta, dens = _f32(a_cur), _f32(s_cur), _f32(s_delta), _f32(dens)
        B, N, _ = s_cur.shape
        assert a_cur.shape == (B, N) and s_delta.shape == (B, N, 3) and dens.shape == (B,)
        out = np.empty((B, N, 3), dtype=np.float32)
        self._ranged(lambda: self.lib.drp_step(self.h, _fp(a_cur), _fp(s_cur), _fp(s_delta), _fp(dens), B, N, _fp(out)))
        return out

    def forward(self, a_cur, s_cur, s_delta, dens, nbr_idx, nbr_cnt):
        a_cur, s_cur, s_delta, dens = _f32(a_cur), _f32(s_cur), _f32(s_delta), _f32(dens)
        nbr_idx = np.ascontiguousarray(nbr_idx, dtype=np.int16)
        nbr_cnt = np.ascontiguousarray(nbr_cnt, dtype=np.uint8)
        B, N, _ = s_cur.shape
        assert nbr_idx.shape == (B, N, L.DRP_K) and nbr_cnt.shape == (B, N)
        out = np.empty((B, N, 3), dtype=np.float32)
        self._ranged(lambda: self.lib.drp_forward(self.h, _fp(a_cur), _fp(s_cur), _fp(s_delta), _fp(dens),
                                                  nbr_idx.ctypes.data_as(L.c_int16_p),
                                                  nbr_cnt.ctypes.data_as(L.c_uint8_p), B, N, _fp(out)))
        return out

    # ---- the float64 yardstick (include/drp.h: drp_forward_f64 ... drp_accuracy_probe) ---------------------------
    def step_f64(self, a_cur, s_cur, s_delta, dens):
        """predict_one_step evaluated in float64 on the device (fp32 inputs and weights widened exactly) -> [B,N,3] float64"""
        a_cur, s_cur, s_delta, dens = _f32(a_cur), _f32(s_cur), _f32(s_delta), _f32(dens)
        B, N, _ = s_cur.shape
        assert a_cur.shape == (B, N) and s_delta.shape == (B, N, 3) and dens.shape == (B,)
        out = np.empty((B, N, 3), dtype=np.float64)
        self._ck(self.lib.drp_step_f64(self.h, _fp(a_cur), _fp(s_cur), _fp(s_delta), _fp(dens), B, N, _dp(out)))
        self._f64_shape = (B, N)
        return out

    def forward_f64(self, a_cur, s_cur, s_delta, dens, nbr_idx, nbr_cnt):
        """forward() with explicit relations, in float64 -> [B,N,3] float64"""
        a_cur, s_cur, s_delta, dens = _f32(a_cur), _f32(s_cur), _f32(s_delta), _f32(dens)
        nbr_idx = np.ascontiguousarray(nbr_idx, dtype=np.int16)
        nbr_cnt = np.ascontiguousarray(nbr_cnt, dtype=np.uint8)
        B, N, _ = s_cur.shape
        assert a_cur.shape == (B, N) and s_delta.shape == (B, N, 3) and dens.shape == (B,)
        assert nbr_idx.shape == (B, N, L.DRP_K) and nbr_cnt.shape == (B, N)
        out = np.empty((B, N, 3), dtype=np.float64)
        self._ck(self.lib.drp_forward_f64(self.h, _fp(a_cur), _fp(s_cur), _fp(s_delta), _fp(dens),
                                          nbr_idx.ctypes.data_as(L.c_int16_p), nbr_cnt.ctypes.data_as(L.c_uint8_p), B, N, _dp(out)))
        self._f64_shape = (B, N)
        return out

    def f64_tap(self, name):
        """float64 intermediate of the last step_f64 / forward_f64 / accuracy_probe: 'particle_encode' [B,N,64],
        'relation_encode' [B,N,10,64], 'effect_rel_p' [B,N,10,64], 'agg_p' and 'effect_p' [B,N,64] (p = 0..2),
        'particle_pred' [B,N,3]"""
        B, N = getattr(self, '_f64_shape', (0, 0))
        if name.startswith(('relation_encode', 'c_edge', 'effect_rel_')):
            shape = (B, N, L.DRP_K, L.DRP_F)
        else:
            shape = (B, N, 3 if name == 'particle_pred' else L.DRP_F)
        out = np.empty(shape, np.float64)
        self._ck(self.lib.drp_f64_tap(self.h, name.encode(), _dp(out), out.size))
        return out

    def set_f64_cap(self, n_bytes=0):
        """bytes of float64 workspace a *_f64 call may hold (0: the default, 256 MB); the batch is walked in chunks under it"""
        self._ck(self.lib.drp_debug_set_f64_cap(self.h, int(n_bytes)))

    def accuracy_probe(self, a_cur, s_cur, s_delta, dens, engine=None):
        """One step on `engine` (default: the selected one) against the float64 evaluation of the same step, reduced on the
        device -> {'abs': max |s_pred - s_pred_f64|, 'disp': max |s_pred_f64 - s_cur|, 'disp_rel': abs / max(disp, 1e-12),
        'worst': index b * N + n of the worst particle}.  The selected engine stays selected."""
        a_cur, s_cur, s_delta, dens = _f32(a_cur), _f32(s_cur), _f32(s_delta), _f32(dens)
        B, N, _ = s_cur.shape
        assert a_cur.shape == (B, N) and s_delta.shape == (B, N, 3) and dens.shape == (B,)
        out = np.zeros(4, np.float64)

        def call(e):
            return self.lib.drp_accuracy_probe(self.h, int(e), _fp(a_cur), _fp(s_cur), _fp(s_delta), _fp(dens), B, N, _dp(out))
        if engine is None:
            self._ranged(lambda: call(self.engine_id))        # of the selected engine: a refusal is handled as its calls' are
        else:
            self._ck(call(engine))
        self._f64_shape = (B, N)
        return {'abs': float(out[0]), 'disp': float(out[1]), 'disp_rel': float(out[2]), 'worst': int(out[3])}

    # ---- the float64 yardstick of the gradient (include/drp.h: drp_gd_grad_f64) ------------------------------------
    def gd_grad_f64(self, s0, attr, dens, actions, want_state_grad=False):
        """One iteration of the GD planner (what gd_begin + gd_grad compute) in float64 on the device: s0 [nb,N,3], attr [nb,N],
        dens [nb], actions [B,H,4] (row = traj * nb + batch) -> (rewards [B], d loss / d actions [B,H,4][, d loss / d every step's
        predicted state [B,H,N,3]]) as float64.  A one-shot call in buffers of its own: it ends no session and leaves the
        selected engine, last_dispatch() and the float64 taps as they were."""
        s0, attr, dens, actions = _f32(s0), _f32(attr), _f32(dens), _f32(actions)
        nb, N = (s0.shape[0], s0.shape[1]) if s0.ndim == 3 else (0, 0)
        B, H = (actions.shape[0], actions.shape[1]) if actions.ndim == 3 else (0, 0)
        r = np.empty((max(B, 0),), np.float64)
        g = np.empty((max(B, 0), max(H, 0), 4), np.float64)
        gs = np.empty((max(B, 0), max(H, 0), max(N, 0), 3), np.float64) if want_state_grad else None
        self._ck(self.lib.drp_gd_grad_f64(self.h, _fp(s0), _fp(attr), _fp(dens), int(nb), int(N), _fp(actions), int(B), int(H),
                                          _dp(r), _dp(g), _dp(gs) if want_state_grad else None))
        return (r, g, gs) if want_state_grad else (r, g)

    def gradient_probe(self, s0, attr, dens, actions, act_lo, act_hi):
        """The gradient the planner consumes, held against float64: gd_begin + gd_grad on whatever tape the selection gives,
        then gd_grad_f64 on the same inputs -> {'abs': max |g32 - g64|, 'scale': max |g64|, 'rel': abs / max(scale, 1e-300),
        'worst': flat index of the worst component (the lowest on a tie; NaN counts as +inf), 'reward_rel': max |r32 - r64| /
        max |r64|, 'tape': 'fused' | 'mfma'}.  A one-shot like gd_begin: it ENDS a running planner session (mpc_* or gd_*), and
        it resets the dispatch marks: last_dispatch() afterwards names this call's kernels (the tape's engine is read from them)."""
        self.dispatch_reset()
        self.gd_begin(s0, attr, dens, actions, 0.05, act_lo, act_hi)
        r32, g32, _ = self.gd_grad()
        # the fp32 matrix engine's tape is the only user of k_aggregate_tape (pick_tape_engine: selected, or after a range refusal)
        tape = 'mfma' if 'k_aggregate_tape' in self.last_dispatch() else 'fused'
        r64, g64 = self.gd_grad_f64(s0, attr, dens, actions)
        err = np.abs(g32.astype(np.float64) - g64).ravel()
        err = np.where(np.isnan(err), np.inf, err)
        scale = float(np.abs(g64).max())
        a = float(err.max())
        rscale = float(np.abs(r64).max())
        return {'abs': a, 'scale': scale, 'rel': a / max(scale, 1e-300), 'worst': int(np.argmax(err)),
                'reward_rel': float(np.abs(r32.astype(np.float64) - r64).max()) / max(rscale, 1e-300), 'tape': tape}

    def rollout(self, s0, attr, dens, actions, want_states=True, want_reward=False):
        s0, attr, dens, actions = _f32(s0), _f32(attr), _f32(dens), _f32(actions)
        nb, N, _ = s0.shape
        B, H, _ = actions.shape
        states = np.empty((B, H, N, 3), dtype=np.float32) if want_states else None
        rew = np.empty((B, H), dtype=np.float32) if want_reward else None
        self._ranged(lambda: self.lib.drp_rollout(self.h, _fp(s0), _fp(attr), _fp(dens), nb, N, _fp(actions), B, H,
                                                  _fp(states) if want_states else None,
                                                  _fp(rew) if want_reward else None))
        return states, rew

    def reward(self, state, normalize=True):
        state = _f32(state)
        Bp, N, _ = state.shape
        out = np.empty((Bp,), dtype=np.float32)
        self._ck(self.lib.drp_reward(self.h, _fp(state), Bp, N, int(bool(normalize)), _fp(out)))
        return out

    # ---- device-resident MPPI -----------------------------------------------------
    def mpc_begin(self, s0, attr, dens, nominal, n_sample, sigma, beta_filter, reward_weight,
                  act_lo, act_hi, seed=0, sample_offset=0, noise_type='normal'):
        s0, attr, dens = _f32(s0), _f32(attr), _f32(dens)
        nominal = np.ascontiguousarray(nominal, dtype=np.float64)
        nb, N, _ = s0.shape
        H = nominal.shape[0]
        p = L.MpcParams()
        p.n_batch, p.n_particles, p.n_sample, p.n_look_ahead = nb, N, int(n_sample), H
        p.sigma, p.beta_filter, p.reward_weight = float(sigma), float(beta_filter), float(reward_weight)
        for i in range(4):
            p.act_lo[i] = float(act_lo[i])
            p.act_hi[i] = float(act_hi[i])
        p.seed, p.sample_offset = int(seed), int(sample_offset)
        p.noise_type, p.reserved = L.NOISE_TYPES[noise_type], 0
        self._ranged(lambda: self.lib.drp_mpc_begin(self.h, ctypes.byref(p), _fp(s0), _fp(attr), _fp(dens), _dp(nominal)))
        self.H, self.nb, self.N, self.ns = H, nb, N, int(n_sample)
        self.S = 0

    S = 0       # scenes of the running sampling session (mpc_begin_scenes); 0: a single-scene session

    def mpc_begin_scenes(self, s0, attr, dens, nominal, n_sample, sigma, beta_filter, reward_weight,
                         act_lo, act_hi, seeds, sample_offset=0, noise_type='normal'):
        """mpc_begin over S scenes on the installed goal table (include/drp.h: drp_mpc_begin_scenes): s0 [S,nb,N,3], attr
        [S,nb,N], dens [S,nb], nominal [S,H,4], seeds [S]; n_sample is per scene.  The session calls then move
        n_sample * S * nb rows in scene_rows' layout, nominals [S,H,4], host noise [S,n_sample,H,4].  The range check is taken
        over all scenes: one scene out of range refuses the whole session (auto_engine: moves all of it to the fp32 engine)."""
        s0, attr, dens = _f32(s0), _f32(attr), _f32(dens)
        nominal = np.ascontiguousarray(nominal, dtype=np.float64)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1)
        assert s0.ndim == 4 and nominal.ndim == 3
        S, nb, N, _ = s0.shape
        H = nominal.shape[1]
        assert attr.shape == (S, nb, N) and dens.shape == (S, nb) and nominal.shape == (S, H, 4) and seeds.shape == (S,)
        p = L.MpcParams()
        p.n_batch, p.n_particles, p.n_sample, p.n_look_ahead = nb, N, int(n_sample), H
        p.sigma, p.beta_filter, p.reward_weight = float(sigma), float(beta_filter), float(reward_weight)
        for i in range(4):
            p.act_lo[i] = float(act_lo[i])
            p.act_hi[i] = float(act_hi[i])
        p.seed, p.sample_offset = 0, int(sample_offset)
        p.noise_type, p.reserved = L.NOISE_TYPES[noise_type], 0
        self._ranged(lambda: self.lib.drp_mpc_begin_scenes(self.h, ctypes.byref(p), int(S), _fp(s0), _fp(attr), _fp(dens),
                                                           _dp(nominal), seeds.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        self.H, self.nb, self.N, self.ns = H, nb, N, int(n_sample)
        self.S = int(S)

    def _mpc_rows(self):
        return self.ns * max(self.S, 1) * self.nb

    def mpc_stats_scenes(self):
        """the last update's statistics of every scene (one entry for a single-scene session), each as mpc_stats() gives them"""
        out = np.empty((max(self.S, 1), 6), dtype=np.float64)
        self._ck(self.lib.drp_mpc_stats_scenes(self.h, _dp(out)))
        return [{'mean': o[0], 'std': o[1], 'max': o[2], 'argmax': int(o[3]), 'Z': o[4], 'm': o[5]} for o in out]

    def mpc_sample(self, iteration, noise=None):
        if noise is not None:
            noise = _f32(noise)
            assert noise.shape == ((self.S, self.ns, self.H, 4) if self.S else (self.ns, self.H, 4))
        self._ranged(lambda: self.lib.drp_mpc_sample(self.h, _fp(noise) if noise is not None else None, int(iteration)))

    def mpc_set_actions(self, actions):
        actions = _f32(actions)
        assert actions.shape == (self._mpc_rows(), self.H, 4)
        self._ranged(lambda: self.lib.drp_mpc_set_actions(self.h, _fp(actions)))

    def mpc_rollout(self, reward_all_steps=False):
        self._ck(self.lib.drp_mpc_rollout(self.h, int(bool(reward_all_steps))))

    def mpc_partials(self, fetch=True):
        out = np.empty((6 + 4 * self.H,), dtype=np.float64) if fetch else None
        self._ck(self.lib.drp_mpc_partials(self.h, _dp(out) if fetch else None))
        return out

    def mpc_update(self, partials):
        partials = np.ascontiguousarray(partials, dtype=np.float64).reshape(-1, 6 + 4 * self.H)
        nominal = np.empty((self.H, 4), dtype=np.float64)
        self._ck(self.lib.drp_mpc_update(self.h, _dp(partials), partials.shape[0], _dp(nominal)))
        return nominal

    def mpc_update_device(self):
        self._ck(self.lib.drp_mpc_update_device(self.h))

    # elite (CEM-style) update: nominal = mean of the k best sequences (not in the reference; include/drp.h)
    def mpc_elite(self, k, fetch=True):
        out = np.empty((int(k), 2 + 4 * self.H), dtype=np.float64) if fetch else None
        self._ck(self.lib.drp_mpc_elite(self.h, int(k), _dp(out) if fetch else None))
        return out

    def mpc_update_elite(self, records, k):
        records = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, int(k), 2 + 4 * self.H)
        nominal = np.empty((self.H, 4), dtype=np.float64)
        self._ck(self.lib.drp_mpc_update_elite(self.h, _dp(records), records.shape[0], int(k), _dp(nominal)))
        return nominal

    def mpc_update_elite_device(self, k):
        self._ck(self.lib.drp_mpc_update_elite_device(self.h, int(k)))

    def mpc_get(self, actions=False, rewards=False, rewards_all=False, states=False, nominal=False):
        B = self._mpc_rows()
        a = np.empty((B, self.H, 4), np.float32) if actions else None
        r = np.empty((B,), np.float32) if rewards else None
        ra = np.empty((B, self.H), np.float32) if rewards_all else None
        s = np.empty((B, self.H, self.N, 3), np.float32) if states else None
        n = np.empty(((self.S, self.H, 4) if self.S else (self.H, 4)), np.float64) if nominal else None
        self._ck(self.lib.drp_mpc_get(self.h, _fp(a) if actions else None, _fp(r) if rewards else None,
                                      _fp(ra) if rewards_all else None, _fp(s) if states else None,
                                      _dp(n) if nominal else None))
        return {'actions': a, 'rewards': r, 'rewards_all': ra, 'states': s, 'nominal': n}

    def mpc_fetch_async(self, slot):
        """The enqueued iteration's pushes and final rewards go to pinned memory behind its kernels (mpc_wait)."""
        self._ck(self.lib.drp_mpc_fetch_async(self.h, int(slot)))

    def mpc_wait(self, slot):
        B = self._mpc_rows()
        a = np.empty((B, self.H, 4), np.float32)
        r = np.empty((B,), np.float32)
        self._ck(self.lib.drp_mpc_wait(self.h, int(slot), _fp(a), _fp(r)))
        return {'actions': a, 'rewards': r}

    def mpc_stats(self):
        out = np.empty((8,), dtype=np.float64)
        self._ck(self.lib.drp_debug_fetch(self.h, b'stats', out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
        return {'mean': out[0], 'std': out[1], 'max': out[2], 'argmax': int(out[3]), 'Z': out[4], 'm': out[5]}

    def fps(self, pts, k, init_idx=0):
        """utils.fps_np on the device: returns (pts[chosen], max distance, chosen indices)."""
        pts = _f32(pts)
        n, dim = pts.shape
        idx = np.empty((k,), np.int32)
        md = ctypes.c_float()
        self._ck(self.lib.drp_fps(self.h, _fp(pts), n, dim, int(k), int(init_idx),
                                  idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(md)))
        return pts[idx], md.value, idx

    # ---- training (row f4) -------------------------------------------------
    def train_begin(self, n_rollout, lr=1e-3, beta1=0.9):
        self._ck(self.lib.drp_train_begin(self.h, int(n_rollout), float(lr), float(beta1)))
        self._n_rollout = int(n_rollout)

    def _train_batch(self, states, impulses, attrs, particle_nums, particle_dens, targets, target_nums, by_actions, need_begin):
        """A training batch as every trainer entry point takes it: contiguous float32 / int32 arrays, their shapes held to one
        another.  impulses: states_delta [B, H, N, 3], or with by_actions the pushes [B, H, 4]; targets / target_nums: None, or
        [B, H, M, 3] / [B, H].  need_begin: H is train_begin's n_rollout; else it is read from `states`, and a batch with an empty
        axis goes on for the C ABI to refuse -> (the arrays, (B, N, H, M), their ctypes pointers), arrays and pointers in the order
        of the arguments; M = 0 and None for targets that are not there."""
        arrays = (_f32(states), _f32(impulses), _f32(attrs), _i32(particle_nums), _f32(particle_dens),
                  _opt(_f32, targets), _opt(_i32, target_nums))
        states, imp, attrs, nums, dens, targets, tnums = arrays
        B, T1, N = states.shape[:3] if states.ndim == 4 else (0, 1, 0)
        H, M = T1 - 1, 0
        assert not need_begin or (states.ndim == 4 and T1 == self._n_rollout + 1)
        if need_begin or (B > 0 and N > 0 and H > 0):
            assert states.shape == (B, T1, N, 3) and imp.shape == ((B, H, 4) if by_actions else (B, H, N, 3))
            assert attrs.shape == (B, T1, N) and nums.shape == (B,) and dens.shape == (B,)
        assert (targets is None) == (tnums is None)
        if targets is not None:
            assert targets.ndim == 4 and targets.shape[:2] == (B, H) and targets.shape[3] == 3 and tnums.shape == (B, H)
            M = targets.shape[2]
        ptrs = (_fp(states), _fp(imp), _fp(attrs), _ip(nums), _fp(dens), _opt(_fp, targets), _opt(_ip, tnums))
        return arrays, (int(B), int(N), int(H), int(M)), ptrs

    def _train_step32(self, states, states_delta, actions, attrs, particle_nums, particle_dens, targets, target_nums, mode,
                      want_grad, loss=None, match_weight=0.5, want_match=False):
        """One fp32 trainer call -> (loss, gradient blob or None, match or None).  The C function by what is given: `loss` (a key
        of L.LOSS_KINDS): drp_train_step_loss; else `actions`: drp_train_step_actions; else `targets`: drp_train_step_untracked;
        else drp_train_step."""
        by_actions = actions is not None
        keep, (B, N, H, M), (ps, pi, pa, pn, pd, pt, ptn) = self._train_batch(
            states, actions if by_actions else states_delta, attrs, particle_nums, particle_dens, targets, target_nums, by_actions, True)
        out = ctypes.c_double()
        grad = np.empty((L.DRP_N_WEIGHTS,), np.float32) if (want_grad and mode != 'eval') else None
        match = np.full((H, B, N), -1, np.int32) if (want_match and loss != 'chamfer') else None
        tail = (L.TRAIN_MODES[mode], ctypes.byref(out), _opt(_fp, grad))
        if loss is not None:
            rc = self.lib.drp_train_step_loss(self.h, ps, *_source_args(by_actions, pi), pa, pn, pd, B, N, pt, ptn, M,
                                              L.LOSS_KINDS[loss], float(match_weight), *tail, _opt(_ip, match))
        elif by_actions:
            rc = self.lib.drp_train_step_actions(self.h, ps, pi, pa, pn, pd, B, N, pt, ptn, M, *tail)
        elif targets is not None:
            rc = self.lib.drp_train_step_untracked(self.h, ps, pi, pa, pn, pd, B, N, pt, ptn, M, *tail)
        else:
            rc = self.lib.drp_train_step(self.h, ps, pi, pa, pn, pd, B, N, *tail)
        self._ck(rc)
        return out.value, grad, match

    def train_step(self, states, states_delta, attrs, particle_nums, particle_dens, mode='update', want_grad=False):
        """One body of the loop at train/train_gnn_dyn.py:159-210 -> (loss, gradient blob or None)."""
        return self._train_step32(states, states_delta, None, attrs, particle_nums, particle_dens, None, None, mode, want_grad)[:2]

    def train_step_untracked(self, states, states_delta, attrs, particle_nums, particle_dens, targets, target_nums,
                             mode='update', want_grad=False):
        """train_step with each step's loss taken against an untracked cloud (include/drp.h: drp_train_step_untracked): targets
        [B, n_rollout, M, 3] with target_nums [B, n_rollout] real rows; of `states` only step 0 is read -> (loss, gradient blob
        or None)."""
        assert targets is not None and target_nums is not None
        return self._train_step32(states, states_delta, None, attrs, particle_nums, particle_dens, targets, target_nums, mode,
                                  want_grad)[:2]

    def train_step_actions(self, states, actions, attrs, particle_nums, particle_dens, targets=None, target_nums=None,
                           mode='update', want_grad=False):
        """train_step (targets None: the tracked MSE) or train_step_untracked (targets [B, n_rollout, M, 3], target_nums
        [B, n_rollout]: the Chamfer loss) with every step's impulse computed from `actions` [B, n_rollout, 4] = (sx, sy, ex, ey) on
        the state the step reads -- states[:, 0], then the model's own predictions -- zero on padded rows, and the push's
        position share in the backward pass (include/drp.h: drp_train_step_actions).  Needs set_camera -> (loss, gradient blob or
        None)."""
        return self._train_step32(states, None, _f32(actions), attrs, particle_nums, particle_dens, targets, target_nums, mode,
                                  want_grad)[:2]

    def train_step_loss(self, states, attrs, particle_nums, particle_dens, targets, target_nums, states_delta=None, actions=None,
                        loss='match', match_weight=0.5, mode='update', want_grad=False, want_match=False):
        """train_step_untracked (states_delta [B, n_rollout, N, 3]) or train_step_actions (actions [B, n_rollout, 4]) -- exactly
        one of the two -- with the loss chosen by name (include/drp.h: drp_train_step_loss): 'chamfer', 'match' (the one-to-one
        matching term of cloud_match) or 'chamfer+match' = (1 - match_weight) chamfer + match_weight match -> (loss, gradient blob
        or None[, match [n_rollout, B, N]: every predicted row's partner in its target, -1 for unmatched rows and padding])."""
        if loss not in L.LOSS_KINDS:
            raise ValueError('loss must be one of %s' % (tuple(L.LOSS_KINDS),))
        _impulses(states_delta, actions)
        assert targets is not None and target_nums is not None
        out = self._train_step32(states, states_delta, actions, attrs, particle_nums, particle_dens, targets, target_nums, mode,
                                 want_grad, loss, match_weight, want_match)
        return out if want_match else out[:2]

    # ---- training on a loss of the caller's (include/drp.h: drp_train_predict, drp_train_step_seeded) ----------------------
    def _seeded_batch(self, states, states_delta, actions, attrs, particle_nums, particle_dens, need_begin):
        """the batch of the four seeded calls: exactly one impulse source -> (_train_batch's arrays, (B, N, H), the C arguments up
        to N)"""
        by_actions, imp = _impulses(states_delta, actions)
        keep, (B, N, H, _), (ps, pi, pa, pn, pd, _, _) = self._train_batch(
            states, imp, attrs, particle_nums, particle_dens, None, None, by_actions, need_begin)
        return keep, (B, N, H), (self.h, ps, *_source_args(by_actions, pi), pa, pn, pd, B, N)

    def train_predict(self, states, attrs, particle_nums, particle_dens, states_delta=None, actions=None):
        """What the training forward predicts: every step's state [B, n_rollout, N, 3] float32, from the forward exactly as
        train_step_seeded (and train_step(mode='grad')) runs it -- on real rows the bits of that call's own forward (include/drp.h:
        drp_train_predict).  states_delta [B, n_rollout, N, 3] or actions [B, n_rollout, 4] -- exactly one of the two.  Rows
        n >= particle_nums[b] come back as the forward leaves them.  Needs train_begin; changes no weight, Adam moment or
        iteration count."""
        keep, (B, N, H), args = self._seeded_batch(states, states_delta, actions, attrs, particle_nums, particle_dens, True)
        pred = np.empty((B, H, N, 3), np.float32)
        self._ck(self.lib.drp_train_predict(*args, _fp(pred)))
        return pred

    def train_step_seeded(self, states, attrs, particle_nums, particle_dens, seed, states_delta=None, actions=None, mode='update',
                          want_grad=False):
        """train_step with the reverse pass seeded by the caller: seed [B, n_rollout, N, 3], seed[b, t, n] = d loss / d
        s_pred_t[b, n], complete (no 1 / (n_rollout B), no 1 / (3 n_b) is applied); rows n >= particle_nums[b] are ignored
        (include/drp.h: drp_train_step_seeded).  mode 'grad' or 'update' -> the gradient blob, or None."""
        keep, (B, N, H), args = self._seeded_batch(states, states_delta, actions, attrs, particle_nums, particle_dens, True)
        seed = _f32(seed)
        assert seed.shape == (B, H, N, 3)
        grad = np.empty((L.DRP_N_WEIGHTS,), np.float32) if want_grad else None
        self._ck(self.lib.drp_train_step_seeded(*args, _fp(seed), L.TRAIN_MODES[mode], _opt(_fp, grad)))
        return grad

    def train_step_custom(self, loss_fn, states, attrs, particle_nums, particle_dens, states_delta=None, actions=None,
                          mode='update', want_grad=False, context=None):
        """One training step on a loss that is a Python function: loss_fn(pred, context) -> (value, grad), a pure function of
        pred [B, n_rollout, N, 3] (train_predict's; it must work on float32 and float64 arrays alike), grad = d value / d pred in
        pred's shape; context: whatever the caller passes through.  mode='eval': train_predict and loss_fn, the gradient dropped;
        else train_predict, loss_fn, train_step_seeded -- the forward runs twice, and being deterministic gives the same bits
        both times, so the gradient is taken at the right point -> (loss, gradient blob or None).  (losses.py: worked examples,
        and torch_loss for a loss written in torch.)"""
        if mode not in L.TRAIN_MODES:
            raise ValueError('mode must be one of %s' % (tuple(L.TRAIN_MODES),))
        pred = self.train_predict(states, attrs, particle_nums, particle_dens, states_delta=states_delta, actions=actions)
        value, seed = loss_fn(pred, context)
        if mode == 'eval':
            return float(value), None
        seed = np.asarray(seed)
        if seed.shape != pred.shape:
            raise ValueError('loss_fn must return a gradient of pred\'s shape %s, got %s' % (pred.shape, seed.shape))
        grad = self.train_step_seeded(states, attrs, particle_nums, particle_dens, seed, states_delta=states_delta, actions=actions,
                                      mode=mode, want_grad=want_grad)
        return float(value), grad

    # ---- one-shots on two cloud batches (include/drp.h: drp_cloud_chamfer, drp_cloud_match, drp_cloud_divergence and their _f64) ----
    @staticmethod
    def _cloud_pair(p, q, n_p, n_q, dtype=np.float32):
        """p [B, N, 3] and q [B, M, 3] (or one pair as [N, 3], [M, 3]) with their real rows n_p, n_q [B] (None: all) as the one-shots
        take them -> (p, q, n_p, n_q, B, N, M); dtype: p's -- float64 for the yardsticks that take p as doubles."""
        p, q = np.ascontiguousarray(p, dtype=dtype), _f32(q)
        if p.ndim == 2 and q.ndim == 2:
            p, q = p[None], q[None]
        assert p.ndim == 3 and q.ndim == 3 and p.shape[2] == 3 and q.shape[2] == 3 and p.shape[0] == q.shape[0]
        B, N, M = p.shape[0], p.shape[1], q.shape[1]
        n_p = np.full((B,), N, np.int32) if n_p is None else _i32(n_p).reshape(-1)
        n_q = np.full((B,), M, np.int32) if n_q is None else _i32(n_q).reshape(-1)
        assert n_p.shape == (B,) and n_q.shape == (B,)
        return p, q, n_p, n_q, int(B), int(N), int(M)

    def _cloud_call(self, fn, pair, middle, outs):
        """A one-shot's C call on _cloud_pair's tuple: `middle` goes between M and the outputs, `outs` are the output arrays, None
        for one that is not wanted; the pointers by each array's dtype"""
        p, q, n_p, n_q, B, N, M = pair
        self._ck(fn(self.h, _ptr(p), _ip(n_p), _fp(q), _ip(n_q), B, N, M, *map(_ptr, middle), *map(_ptr, outs)))

    def _cloud_chamfer(self, dtype, p, q, n_p, n_q, want_grad, want_nn):
        """cloud_chamfer (dtype float32) and cloud_chamfer_f64 (float64: the gradient's type, and the margins; p stays float32)"""
        f64 = dtype is np.float64
        pair = self._cloud_pair(p, q, n_p, n_q)
        B, N, M = pair[4:]
        terms = np.empty((B, 2), np.float64)
        grad = np.empty((B, N, 3), dtype) if want_grad else None
        nn_pq = np.empty((B, N), np.int32) if want_nn else None
        nn_qp = np.empty((B, M), np.int32) if want_nn else None
        margin = np.empty((B, 2), np.float64) if f64 else None
        self._cloud_call(self.lib.drp_cloud_chamfer_f64 if f64 else self.lib.drp_cloud_chamfer, pair, (),
                         (terms, grad, nn_pq, nn_qp) + ((margin,) if f64 else ()))
        out = {'fwd': terms[:, 0].copy(), 'bwd': terms[:, 1].copy(), 'total': terms[:, 0] + terms[:, 1]}
        if f64:
            out['margin'] = margin
        if want_grad:
            out['grad'] = grad
        if want_nn:
            out['nn_pq'], out['nn_qp'] = nn_pq, nn_qp
        return out

    def cloud_chamfer(self, p, q, n_p=None, n_q=None, want_grad=False, want_nn=False):
        """Symmetric squared Chamfer distance of p [B, N, 3] (n_p [B] real rows, default all) and q [B, M, 3] (n_q) ->
        {'fwd', 'bwd', 'total' [B] float64[, 'grad' [B, N, 3] = d total / d p][, 'nn_pq' [B, N], 'nn_qp' [B, M]: each row's nearest
        row of the other cloud, -1 on padding]}.  A single cloud pair may be given as [N, 3], [M, 3].  A one-shot: it needs no
        weights and ends no session."""
        return self._cloud_chamfer(np.float32, p, q, n_p, n_q, want_grad, want_nn)

    def _cloud_match(self, dtype, p, q, n_p, n_q, match_in, want_grad, want_match, want_dual):
        """cloud_match (dtype float32) and cloud_match_f64 (float64: p's and the gradient's type, match_in and the two costs)"""
        f64 = dtype is np.float64
        pair = self._cloud_pair(p, q, n_p, n_q, dtype)
        n_p, n_q, B, N, M = pair[2:]
        if match_in is not None:
            match_in = _i32(match_in).reshape(B, N)
        terms = np.empty((B,), np.float64)
        grad = np.empty((B, N, 3), dtype) if want_grad else None
        m_pq = np.empty((B, N), np.int32) if want_match else None
        m_qp = np.empty((B, M), np.int32) if want_match else None
        dual = np.empty((B, N + M), np.float64) if want_dual else None
        cost = np.empty((B, 2), np.float64) if f64 else None
        self._cloud_call(self.lib.drp_cloud_match_f64 if f64 else self.lib.drp_cloud_match, pair, (match_in,) if f64 else (),
                         (terms, grad, m_pq, m_qp, dual) + ((cost,) if f64 else ()))
        out = {'match': terms, 'r': np.minimum(n_p, n_q)}
        if f64:
            out['cost'], out['opt_cost'] = cost[:, 0].copy(), cost[:, 1].copy()
        if want_grad:
            out['grad'] = grad
        if want_match:
            out['match_pq'], out['match_qp'] = m_pq, m_qp
        if want_dual:
            out['u'], out['v'] = dual[:, :N].copy(), dual[:, N:].copy()
        return out

    def cloud_match(self, p, q, n_p=None, n_q=None, want_grad=False, want_match=False, want_dual=False):
        """Matching (earth mover's) distance of p [B, N, 3] (n_p [B] real rows, default all) and q [B, M, 3] (n_q): every row of
        the smaller cloud paired with a distinct row of the larger one at the least total squared distance ->
        {'match' [B] float64 = sum over the pairs / (3 r), 'r' [B] = min(n_p, n_q)[, 'grad' [B, N, 3] = d match / d p][, 'match_pq'
        [B, N], 'match_qp' [B, M]: each row's partner, -1 for unmatched rows and padding][, 'u' [B, N], 'v' [B, M]: the duals of
        p's and q's rows, float64]}.  A single cloud pair may be given as [N, 3], [M, 3].  At most 1024 points per cloud.  A
        one-shot: it needs no weights and ends no session."""
        return self._cloud_match(np.float32, p, q, n_p, n_q, None, want_grad, want_match, want_dual)

    def cloud_transport(self, p, q, n_p=None, n_q=None, eps=None, iters=None, want_grad=False, want_dual=False, want_col_err=False):
        """Entropy-regularised optimal-transport distance of p [B, N, 3] (n_p [B] real rows, default all; mass 1 / n_p each) and
        q [B, M, 3] (n_q; mass 1 / n_q each) after `iters` log-domain Sinkhorn sweeps with eps (a number or [B], in
        squared-distance units; both are required) -> {'transport' [B] float64 = sum_ij P_ij |p_i - q_j|^2 / 3[, 'grad' [B, N, 3] =
        d transport / d p with the plan P held fixed: non-zero on every real row whatever the counts][, 'f' [B, N], 'g' [B, M]: the
        duals, float64, 0 on padding][, 'col_err' [B]: sum_j |sum_i P_ij - 1 / n_q|, what the sweeps left of the column
        marginals]} (include/drp.h: drp_cloud_transport).  A single cloud pair may be given as [N, 3], [M, 3].  At most 1024
        points per cloud.  A one-shot: it needs no weights and ends no session."""
        if eps is None or iters is None:
            raise ValueError('cloud_transport needs eps (squared-distance units) and iters')
        pair = self._cloud_pair(p, q, n_p, n_q)
        B, N, M = pair[4:]
        terms = np.empty((B,), np.float64)
        grad = np.empty((B, N, 3), np.float32) if want_grad else None
        dual = np.empty((B, N + M), np.float64) if want_dual else None
        col_err = np.empty((B,), np.float64) if want_col_err else None
        self._cloud_call(self.lib.drp_cloud_transport, pair, (_per_sample(eps, B), int(iters)), (terms, grad, dual, col_err))
        out = {'transport': terms}
        if want_grad:
            out['grad'] = grad
        if want_dual:
            out['f'], out['g'] = dual[:, :N].copy(), dual[:, N:].copy()
        if want_col_err:
            out['col_err'] = col_err
        return out

    def _train_targeted32(self, fn, by_actions, impulses, states, attrs, particle_nums, particle_dens, targets, target_nums, mode,
                          want_grad, extra):
        """An fp32 trainer call whose loss takes arguments of its own (drp_train_step_transport, drp_train_step_divergence,
        drp_train_step_divergence_unbalanced).  by_actions, impulses: _impulses'.  extra(H, B) -> (the C arguments between M and
        mode, the outputs behind grad_out -- None for one that is not wanted), arrays as numpy arrays -> (loss, gradient blob or
        None) + the outputs."""
        assert targets is not None and target_nums is not None
        keep, (B, N, H, M), (ps, pi, pa, pn, pd, pt, ptn) = self._train_batch(
            states, impulses, attrs, particle_nums, particle_dens, targets, target_nums, by_actions, True)
        args, outs = extra(H, B)
        loss = ctypes.c_double()
        grad = np.empty((L.DRP_N_WEIGHTS,), np.float32) if (want_grad and mode != 'eval') else None
        self._ck(fn(self.h, ps, *_source_args(by_actions, pi), pa, pn, pd, B, N, pt, ptn, M, *map(_ptr, args), L.TRAIN_MODES[mode],
                    ctypes.byref(loss), _ptr(grad), *map(_ptr, outs)))
        return (loss.value, grad) + tuple(outs)

    def train_step_transport(self, states, attrs, particle_nums, particle_dens, targets, target_nums, eps, iters, states_delta=None,
                             actions=None, mode='update', want_grad=False, want_col_err=False):
        """train_step_loss with each step's term the transport distance of cloud_transport between the predicted state and its
        target cloud (include/drp.h: drp_train_step_transport): eps [B] (or a number) per sample, iters sweeps; states_delta
        [B, n_rollout, N, 3] or actions [B, n_rollout, 4] -- exactly one of the two -> (loss, gradient blob or None[, col_err
        [n_rollout, B]: every problem's column-marginal violation])."""
        by_actions, imp = _impulses(states_delta, actions)
        out = self._train_targeted32(
            self.lib.drp_train_step_transport, by_actions, imp, states, attrs, particle_nums, particle_dens, targets, target_nums,
            mode, want_grad, lambda H, B: ((_per_sample(eps, B), int(iters)), (np.empty((H, B)) if want_col_err else None,)))
        return out if want_col_err else out[:2]

    def _cloud_divergence(self, name, dtype, p, q, n_p, n_q, eps, iters, want_grad, want_dual, want_col_err, want_self_err, reach,
                          mass_q, want_transported):
        """cloud_divergence (dtype float32) and cloud_divergence_f64 (float64: p's and the gradient's type); the balanced and the
        unbalanced call differ in their trailing arguments alone"""
        if eps is None or iters is None:
            raise ValueError('%s needs eps (squared-distance units) and iters' % name)
        if reach is None and (mass_q is not None or want_transported):
            raise ValueError('mass_q and want_transported belong to the unbalanced divergence: give reach')
        pair = self._cloud_pair(p, q, n_p, n_q, dtype)
        B, N, M = pair[4:]
        middle = (_per_sample(eps, B),)
        terms = np.empty((B,), np.float64)
        grad = np.empty((B, N, 3), dtype) if want_grad else None
        dual = np.empty((B, 2 * (N + M)), np.float64) if want_dual else None
        col_err = np.empty((B,), np.float64) if want_col_err else None
        self_err = np.empty((B, 2), np.float64) if want_self_err else None
        outs = (terms, grad, dual, col_err, self_err)
        if reach is not None:
            middle += (_per_sample(reach, B), _per_sample(1.0 if mass_q is None else mass_q, B))
            moved = np.empty((B,), np.float64) if want_transported else None
            outs += (moved,)
        fn = 'drp_cloud_divergence' + ('' if reach is None else '_unbalanced') + ('_f64' if dtype is np.float64 else '')
        self._cloud_call(getattr(self.lib, fn), pair, middle + (int(iters),), outs)
        out = {'divergence': terms}
        if want_transported:
            out['transported'] = moved
        if want_grad:
            out['grad'] = grad
        if want_dual:
            out['f'], out['g'] = dual[:, :N].copy(), dual[:, N:N + M].copy()
            out['h_p'], out['h_q'] = dual[:, N + M:2 * N + M].copy(), dual[:, 2 * N + M:].copy()
        if want_col_err:
            out['col_err'] = col_err
        if want_self_err:
            out['self_err'] = self_err
        return out

    def cloud_divergence(self, p, q, n_p=None, n_q=None, eps=None, iters=None, want_grad=False, want_dual=False, want_col_err=False,
                         want_self_err=False, reach=None, mass_q=None, want_transported=False):
        """Sinkhorn divergence of p [B, N, 3] and q [B, M, 3] (arguments as cloud_transport's; eps and iters are required):
        cloud_transport's loss with its entropic bias taken out, OT(p, q) - OT(p, p) / 2 - OT(q, q) / 2 on the dual values, zero
        only for equal clouds -> {'divergence' [B] float64 (not clamped: rounding can leave it a hair below zero at p ~ q)[, 'grad'
        [B, N, 3] = d divergence / d p with the cross plan and p's self plan held fixed: non-zero on every real row whatever the
        counts, and zero where transport's is not, at p == q][, 'f' [B, N], 'g' [B, M], 'h_p' [B, N], 'h_q' [B, M]: the duals of
        the cross problem and of the two self problems, float64, 0 on padding][, 'col_err' [B] as cloud_transport's][, 'self_err'
        [B, 2]: sum_i |sum_j S_ij - mass| of p's and of q's self plan]} (include/drp.h: drp_cloud_divergence).  At most 1024
        points per cloud.  A one-shot: it needs no weights and ends no session.
        reach (a number or [B], in eps's unit; np.inf: balanced) makes it the UNBALANCED divergence for a pile seen partly
        (include/drp.h: drp_cloud_divergence_unbalanced): mass further than about sqrt(reach) from the other cloud is given up
        instead of moved.  mass_q (a number or [B], default 1, within [1/8, 8]): q's total mass against p's 1 -- n_q / n_p is
        equal mass per point.  want_transported: + 'transported' [B], the plan's total mass.  reach=None is the call above."""
        return self._cloud_divergence('cloud_divergence', np.float32, p, q, n_p, n_q, eps, iters, want_grad, want_dual, want_col_err,
                                      want_self_err, reach, mass_q, want_transported)

    @staticmethod
    def _divergence_extra(eps, iters, reach, mass_q, want_err, floor=0):
        """_train_targeted32's / _train_targeted64's `extra` of the divergence: eps [B][, reach [B], mass_q [H, B]], iters, and
        col_err [H, B], self_err [H, B, 2][, transported [H, B]] where wanted; floor: the least length the inputs are broadcast to
        (the float64 calls hand an empty batch on for the C ABI to refuse)"""
        def extra(H, B):
            Hi, Bi = max(H, floor), max(B, floor)
            args = (_per_sample(eps, Bi),)
            shapes = ((H, B), (H, B, 2))
            if reach is not None:
                args += (_per_sample(reach, Bi), _per_step(1.0 if mass_q is None else mass_q, Hi, Bi))
                shapes += ((H, B),)
            return args + (int(iters),), tuple(np.empty(s, np.float64) if want_err else None for s in shapes)
        return extra

    def train_step_divergence(self, states, attrs, particle_nums, particle_dens, targets, target_nums, eps, iters, states_delta=None,
                              actions=None, mode='update', want_grad=False, want_err=False, reach=None, mass_q=None):
        """train_step_transport with each step's term the Sinkhorn divergence of cloud_divergence (include/drp.h:
        drp_train_step_divergence): the same arguments -> (loss, gradient blob or None[, col_err [n_rollout, B], self_err
        [n_rollout, B, 2]: every problem's certificates]).  reach (a number or [B]) and mass_q (a number, [B] or [n_rollout, B];
        default 1): cloud_divergence's unbalanced divergence as each step's term (drp_train_step_divergence_unbalanced); want_err
        then also returns transported [n_rollout, B].  reach=None is the call above."""
        by_actions, imp = _impulses(states_delta, actions)
        if reach is None and mass_q is not None:
            raise ValueError('mass_q belongs to the unbalanced divergence: give reach')
        fn = self.lib.drp_train_step_divergence if reach is None else self.lib.drp_train_step_divergence_unbalanced
        out = self._train_targeted32(fn, by_actions, imp, states, attrs, particle_nums, particle_dens, targets, target_nums, mode,
                                     want_grad, self._divergence_extra(eps, iters, reach, mass_q, want_err))
        return out if want_err else out[:2]

    def cloud_chamfer_f64(self, p, q, n_p=None, n_q=None, want_grad=False, want_nn=False):
        """cloud_chamfer in float64 on the device (include/drp.h: drp_cloud_chamfer_f64): the same dict with 'grad' as float64,
        plus 'margin' [B, 2] -- per sample the smallest (second-best - best) squared distance over its arg-mins, p -> q then
        q -> p: 0 for a duplicate of a winner, inf where the other cloud has one row."""
        return self._cloud_chamfer(np.float64, p, q, n_p, n_q, want_grad, want_nn)

    def cloud_divergence_f64(self, p, q, n_p=None, n_q=None, eps=None, iters=None, want_grad=False, want_dual=False,
                             want_col_err=False, want_self_err=False, reach=None, mass_q=None, want_transported=False):
        """cloud_divergence with nothing in fp32, on the device (include/drp.h: drp_cloud_divergence_f64): p is taken as float64
        [B, N, 3] -- every bit of it enters the costs, as the float64 tape's predicted state does in train_grad_f64_divergence --
        q as float32 widened exactly; costs and differences are double, and 'grad' is float64, never rounded to fp32.  The same
        arguments, dict, limits (1024 points per cloud) and one-shot contract.  reach, mass_q and want_transported as
        cloud_divergence's: the unbalanced divergence's yardstick (include/drp.h: drp_cloud_divergence_unbalanced_f64)."""
        return self._cloud_divergence('cloud_divergence_f64', np.float64, p, q, n_p, n_q, eps, iters, want_grad, want_dual,
                                      want_col_err, want_self_err, reach, mass_q, want_transported)

    def cloud_match_f64(self, p, q, n_p=None, n_q=None, match_in=None, want_grad=False, want_match=False, want_dual=False):
        """cloud_match with nothing in fp32, on the device (include/drp.h: drp_cloud_match_f64): p is taken as float64 [B, N, 3]
        -- every bit of it enters the costs, as the float64 tape's predicted state does in train_grad_f64_match -- q as float32
        widened exactly; the assignment is solved on double costs -> cloud_match's dict with 'grad' as float64, plus 'cost' [B]
        (sum of the squared distances over the pairs the term used) and 'opt_cost' [B] (over the optimum's pairs).  match_in
        [B, N] (every row of p's partner, -1 for none): 'match' and 'grad' are taken on these pairs; 'match_pq', 'match_qp', 'u',
        'v' and 'opt_cost' are the solver's own optimum all the same, and cost >= opt_cost says how far from it the given pairs
        are.  The same limits (1024 points per cloud) and one-shot contract."""
        return self._cloud_match(np.float64, p, q, n_p, n_q, match_in, want_grad, want_match, want_dual)

    # ---- the float64 yardstick of the trainer's gradients (include/drp.h: drp_train_grad_f64) ------------------------
    def _train_grad64(self, states, states_delta, actions, attrs, particle_nums, particle_dens, targets, target_nums, want_state):
        """One float64 trainer call -> (loss, terms [H, B], gradient blob, margin [H, B] or None, state gradient or None).  The C
        function by what is given: `targets`: drp_train_grad_f64_untracked; else `actions`: drp_train_grad_f64_actions; else
        drp_train_grad_f64."""
        by_actions = actions is not None
        keep, (B, N, H, M), (ps, pi, pa, pn, pd, pt, ptn) = self._train_batch(
            states, actions if by_actions else states_delta, attrs, particle_nums, particle_dens, targets, target_nums, by_actions, False)
        loss = ctypes.c_double()
        terms = np.empty((max(H, 0), B), np.float64)
        margin = np.empty((H, B), np.float64) if targets is not None else None
        grad = np.empty((L.DRP_N_WEIGHTS,), np.float64)
        gs = np.empty((B, max(H, 0), N, 3), np.float64) if want_state else None
        tail = (ctypes.byref(loss), _dp(terms), _dp(grad), _opt(_dp, gs))
        if targets is not None:
            rc = self.lib.drp_train_grad_f64_untracked(self.h, ps, *_source_args(by_actions, pi), pa, pn, pd, B, N, H, pt, ptn, M,
                                                       *tail, _dp(margin))
        else:
            fn = self.lib.drp_train_grad_f64_actions if by_actions else self.lib.drp_train_grad_f64
            rc = fn(self.h, ps, pi, pa, pn, pd, B, N, H, *tail)
        self._ck(rc)
        return loss.value, terms, grad, margin, gs

    def train_grad_f64(self, states, states_delta, attrs, particle_nums, particle_dens, want_state=False):
        """What train_step(mode='grad') computes, in float64 on the device -> (loss, loss_terms [n_rollout, B], gradient blob
        [38403] in state_dict order[, d loss / d every step's predicted state [B, n_rollout, N, 3]]) as float64.  n_rollout is
        read from the arrays.  A one-shot call in buffers of its own: no train_begin needed; it ends no session and leaves the
        trainer's Adam state, the selected engine, last_dispatch() and the float64 taps as they were."""
        loss, terms, grad, _, gs = self._train_grad64(states, states_delta, None, attrs, particle_nums, particle_dens, None, None,
                                                      want_state)
        return (loss, terms, grad, gs) if want_state else (loss, terms, grad)

    def train_grad_f64_actions(self, states, actions, attrs, particle_nums, particle_dens, want_state=False):
        """train_grad_f64 with the pushes `actions` [B, n_rollout, 4] in place of states_delta: what
        train_step_actions(mode='grad') computes with the MSE loss, in float64 on the device (include/drp.h:
        drp_train_grad_f64_actions).  Needs set_camera; the same returns and the same one-shot contract."""
        loss, terms, grad, _, gs = self._train_grad64(states, None, _f32(actions), attrs, particle_nums, particle_dens, None, None,
                                                      want_state)
        return (loss, terms, grad, gs) if want_state else (loss, terms, grad)

    def train_grad_f64_untracked(self, states, states_delta, attrs, particle_nums, particle_dens, targets, target_nums,
                                 actions=None, want_state=False):
        """train_grad_f64 (actions None) or train_grad_f64_actions (actions [B, n_rollout, 4]; states_delta is then ignored and
        may be None) with the Chamfer loss against targets [B, n_rollout, M, 3] / target_nums [B, n_rollout]: what
        train_step_untracked / train_step_actions(targets=...) compute with mode='grad', in float64 on the device (include/drp.h:
        drp_train_grad_f64_untracked) -> (loss, loss_terms [n_rollout, B], gradient blob [38403], margin [n_rollout, B][, d loss /
        d every step's predicted state [B, n_rollout, N, 3]]).  margin: per (step, sample) the smallest (second-best - best)
        squared distance over its float64 arg-mins -- how close the nearest partner flip is.  The same one-shot contract."""
        assert targets is not None and target_nums is not None
        loss, terms, grad, margin, gs = self._train_grad64(states, states_delta, actions, attrs, particle_nums, particle_dens,
                                                           targets, target_nums, want_state)
        return (loss, terms, grad, margin, gs) if want_state else (loss, terms, grad, margin)

    def _train_targeted64(self, fn, states, states_delta, actions, attrs, particle_nums, particle_dens, targets, target_nums,
                          want_state, extra):
        """_train_targeted32's float64 counterpart (drp_train_grad_f64_divergence, drp_train_grad_f64_divergence_unbalanced,
        drp_train_grad_f64_match): n_rollout is read from the arrays, states_delta is ignored beside actions, and extra(H, B, N)'s
        outputs go behind grad_state_out -> ((loss, loss_terms [H, B], gradient blob[, state gradient]), the outputs)."""
        assert targets is not None and target_nums is not None
        by_actions, imp = _impulses(states_delta, actions, exactly_one=False)
        keep, (B, N, H, M), (ps, pi, pa, pn, pd, pt, ptn) = self._train_batch(
            states, imp, attrs, particle_nums, particle_dens, targets, target_nums, by_actions, False)
        args, outs = extra(max(H, 0), B, N)
        loss = ctypes.c_double()
        terms = np.empty((max(H, 0), B), np.float64)
        grad = np.empty((L.DRP_N_WEIGHTS,), np.float64)
        gs = np.empty((B, max(H, 0), N, 3), np.float64) if want_state else None
        self._ck(fn(self.h, ps, *_source_args(by_actions, pi), pa, pn, pd, B, N, H, pt, ptn, M, *map(_ptr, args), ctypes.byref(loss),
                    _dp(terms), _dp(grad), _ptr(gs), *map(_ptr, outs)))
        return (loss.value, terms, grad) + ((gs,) if want_state else ()), tuple(outs)

    def train_grad_f64_divergence(self, states, states_delta, attrs, particle_nums, particle_dens, targets, target_nums, eps, iters,
                                  actions=None, want_state=False, want_err=False, reach=None, mass_q=None):
        """train_grad_f64_untracked with the Sinkhorn divergence in place of the Chamfer loss: what
        train_step_divergence(mode='grad') computes, in float64 on the device (include/drp.h: drp_train_grad_f64_divergence).
        eps [B] (or a number) and iters as train_step_divergence's; actions [B, n_rollout, 4] in place of states_delta (then
        ignored, may be None).  The plans of every step are formed from the float64 prediction itself -> (loss, loss_terms
        [n_rollout, B], gradient blob [38403][, d loss / d every step's predicted state [B, n_rollout, N, 3]][, col_err
        [n_rollout, B], self_err [n_rollout, B, 2]: every problem's certificates]).  The same one-shot contract.  reach (a number
        or [B]) and mass_q (a number, [B] or [n_rollout, B]; default 1) as train_step_divergence's: the unbalanced divergence as
        each step's term (drp_train_grad_f64_divergence_unbalanced); want_err then also returns transported [n_rollout, B].
        reach=None is the call above."""
        if reach is None and mass_q is not None:
            raise ValueError('mass_q belongs to the unbalanced divergence: give reach')
        fn = self.lib.drp_train_grad_f64_divergence if reach is None else self.lib.drp_train_grad_f64_divergence_unbalanced
        extra = self._divergence_extra(eps, iters, reach, mass_q, want_err, floor=1)
        out, errs = self._train_targeted64(fn, states, states_delta, actions, attrs, particle_nums, particle_dens, targets, target_nums,
                                           want_state, lambda H, B, N: extra(H, B))
        return out + (errs if want_err else ())

    def train_grad_f64_match(self, states, states_delta, attrs, particle_nums, particle_dens, targets, target_nums, loss='match',
                             match_weight=0.5, actions=None, match_in=None, want_state=False, want_info=False):
        """train_grad_f64_untracked with a matching loss in place of the Chamfer loss: what train_step_loss(mode='grad') computes
        for loss 'match' or 'chamfer+match' (match_weight: the mix's), in float64 on the device (include/drp.h:
        drp_train_grad_f64_match).  actions [B, n_rollout, 4] in place of states_delta (then ignored, may be None).  match_in
        [n_rollout, B, N] (train_step_loss's match): every term and the seed of the reverse pass are taken on these pairs, so that
        the difference from the fp32 gradient is arithmetic on the same pairs; None: on the float64 side's own optimum, solved on
        its double prediction -> (loss, loss_terms [n_rollout, B], gradient blob [38403][, d loss / d every step's predicted state
        [B, n_rollout, N, 3]][, info = {'match' [n_rollout, B, N]: the float64 optimum's partners, 'cost', 'opt_cost'
        [n_rollout, B]: the sum of squared distances over the pairs used and over the optimum's, 'chamfer_margin' [n_rollout, B]:
        the mix's Chamfer arg-min margins, None for 'match'}]).  The same one-shot contract."""
        if loss not in L.MATCH_LOSSES:
            raise ValueError('loss must be one of %s' % (L.MATCH_LOSSES,))

        def extra(H, B, N):
            given = None if match_in is None else _i32(match_in).reshape(H, B, N)
            match = np.full((H, B, N), -1, np.int32) if want_info else None
            cost = np.empty((H, B, 2), np.float64) if want_info else None
            margin = np.empty((H, B), np.float64) if (want_info and loss != 'match') else None
            return (L.LOSS_KINDS[loss], float(match_weight), given), (match, cost, margin)
        out, (match, cost, margin) = self._train_targeted64(self.lib.drp_train_grad_f64_match, states, states_delta, actions, attrs,
                                                            particle_nums, particle_dens, targets, target_nums, want_state, extra)
        info = {'match': match, 'cost': cost[..., 0].copy(), 'opt_cost': cost[..., 1].copy(),
                'chamfer_margin': margin} if want_info else None
        return out + ((info,) if want_info else ())

    def train_predict_f64(self, states, attrs, particle_nums, particle_dens, states_delta=None, actions=None):
        """train_predict in float64 on the device: every step's predicted state [B, n_rollout, N, 3] float64 of train_grad_f64's
        forward (include/drp.h: drp_train_predict_f64).  n_rollout is read from the arrays; train_grad_f64's one-shot contract."""
        keep, (B, N, H), args = self._seeded_batch(states, states_delta, actions, attrs, particle_nums, particle_dens, False)
        pred = np.empty((B, max(H, 0), N, 3), np.float64)
        self._ck(self.lib.drp_train_predict_f64(*args, H, _dp(pred)))
        return pred

    def train_grad_f64_seeded(self, states, attrs, particle_nums, particle_dens, seed, states_delta=None, actions=None,
                              want_state=False):
        """What train_step_seeded(mode='grad') computes, in float64 on the device: seed [B, n_rollout, N, 3] float64 = d loss / d
        every step's predicted state, complete; padded rows ignored (include/drp.h: drp_train_grad_f64_seeded) -> (gradient blob
        [38403][, d loss / d every step's predicted state with the later steps' shares, [B, n_rollout, N, 3]]) as float64.
        train_grad_f64's one-shot contract."""
        keep, (B, N, H), args = self._seeded_batch(states, states_delta, actions, attrs, particle_nums, particle_dens, False)
        seed = _f64(seed)
        assert seed.shape == (B, H, N, 3)
        grad = np.empty((L.DRP_N_WEIGHTS,), np.float64)
        gs = np.empty((B, max(H, 0), N, 3), np.float64) if want_state else None
        self._ck(self.lib.drp_train_grad_f64_seeded(*args, H, _dp(seed), _dp(grad), _opt(_dp, gs)))
        return (grad, gs) if want_state else (grad,)

    def train_gradient_probe_custom(self, loss_fn, states, attrs, particle_nums, particle_dens, states_delta=None, actions=None,
                                    context=None):
        """train_gradient_probe for a loss of the caller's (train_step_custom's loss_fn): the fp32 pair -- train_predict, loss_fn,
        train_step_seeded(mode='grad') -- held against the float64 pair -- train_predict_f64, loss_fn, train_grad_f64_seeded -- on
        the same batch -> train_gradient_probe's dict ('tensors', 'worst', 'rel', 'loss32', 'loss64', 'loss_diff', 'tape') with
        'loss_kind': 'custom' and 'seed_rel' = max |seed32 - seed64| / max |seed64|: how far the loss's own gradient moves under
        the fp32 drift of the prediction -- the loss's conditioning, as opposed to the tape's arithmetic.  Needs train_begin; it
        changes no weight, Adam moment or iteration count; like train_gradient_probe it ends a running planner session and
        resets the dispatch marks."""
        kw = {'states_delta': states_delta, 'actions': actions}
        self.dispatch_reset()
        pred32 = self.train_predict(states, attrs, particle_nums, particle_dens, **kw)
        loss32, seed32 = loss_fn(pred32, context)
        g32 = self.train_step_seeded(states, attrs, particle_nums, particle_dens, seed32, mode='grad', want_grad=True, **kw)
        tape = 'mfma' if 'k_aggregate_tape' in self.last_dispatch() else 'fused'
        pred64 = self.train_predict_f64(states, attrs, particle_nums, particle_dens, **kw)
        loss64, seed64 = loss_fn(pred64, context)
        g64, = self.train_grad_f64_seeded(states, attrs, particle_nums, particle_dens, seed64, **kw)
        loss32, loss64 = float(loss32), float(loss64)
        tensors, worst = _compare_blobs(g32, g64)
        real = np.arange(pred32.shape[2])[None, :] < _i32(particle_nums).reshape(-1, 1)          # [B, N]
        s32 = np.where(real[:, None, :, None], np.asarray(seed32, np.float64), 0.0)
        s64 = np.where(real[:, None, :, None], np.asarray(seed64, np.float64), 0.0)
        return {'tensors': tensors, 'worst': worst, 'rel': tensors[worst]['rel'], 'loss32': loss32, 'loss64': loss64,
                'loss_diff': abs(loss32 - loss64), 'tape': tape, 'loss_kind': 'custom',
                'seed_rel': float(np.abs(s32 - s64).max() / max(np.abs(s64).max(), 1e-300))}

    def train_gradient_probe(self, states, states_delta, attrs, particle_nums, particle_dens, actions=None, targets=None,
                             target_nums=None, eps=None, iters=None, loss=None, match_weight=0.5, reach=None, mass_q=None):
        """The gradients the trainer consumes, held against float64: train_step(mode='grad', want_grad=True) on whatever tape the
        selection gives, then train_grad_f64 on the same batch -> {'tensors': {state_dict key: {'max_abs_err', 'max_abs_ref',
        'rel' = err / max(ref, 1e-300)}}, 'worst': the key of the largest rel, 'rel': that rel, 'loss32', 'loss64', 'loss_diff',
        'tape': 'fused' | 'mfma'}.  Needs train_begin, like train_step; it changes no weight, Adam moment or iteration count, so a
        following train_step(mode='update') is what it would have been.  Like train_step it ends a running planner session, and
        it resets the dispatch marks: last_dispatch() afterwards names this call's kernels.  With `actions` [B, n_rollout, 4]
        (states_delta is then ignored and may be None) the pair is train_step_actions and train_grad_f64_actions: the impulses
        from the pushes on the predicted state, the MSE loss.  With `targets` [B, n_rollout, M, 3] and `target_nums`
        [B, n_rollout] the loss is the Chamfer distance to the untracked clouds: the pair is train_step_untracked (or
        train_step_actions with targets) and train_grad_f64_untracked, and the dict also has 'loss_kind': 'chamfer' and
        'min_margin', the smallest arg-min margin of the float64 evaluation over the batch (squared distance).  The float64 side
        takes its own arg-mins: where min_margin is as small as the fp32 drift of a predicted state allows a nearest partner to
        flip, a finding may be that flip -- a discrete change of the gradient -- and no arithmetic error.  With `eps` [B] (or a
        number) and `iters` given beside the targets the loss is the Sinkhorn divergence to them: the pair is
        train_step_divergence(mode='grad') and train_grad_f64_divergence, and the dict has 'loss_kind': 'sinkhorn', 'col_err' and
        'self_err' -- the float64 side's largest certificates over the batch -- in place of 'min_margin'.  The float64 side forms
        its own plans from its own predicted states.  With `loss` 'match' or 'chamfer+match' (match_weight: the mix's) beside
        the targets the pair is train_step_loss(mode='grad', want_match=True) and train_grad_f64_match(match_in=the fp32 side's
        partners): 'rel' and 'tensors' are then ARITHMETIC error on the same pairs, whatever the fp32 tape's drift did to the
        assignment.  What it did is reported beside them, from the same float64 call, which solves the assignment on its own
        double prediction all the same: 'loss_kind'; 'flipped', the number of (step, sample) problems whose float64 optimum
        differs from the fp32 side's partners, and 'rows_flipped', the rows that differ; 'cost_gap', the largest (cost - opt_cost)
        / opt_cost -- how far from optimal, in double, the fp32 side's matching is; for the mix 'min_margin' as for Chamfer.  Only
        where flipped > 0, a second float64 call on its own matching gives 'rel_own': what the disagreement costs in the
        gradient.  loss=None is the call without these two keywords.  With `reach` (a number or [B]) and `mass_q` (a number,
        [B] or [n_rollout, B]; default 1) beside eps and iters the loss is the UNBALANCED divergence: the pair is
        train_step_divergence(reach=, mass_q=, mode='grad', want_err=True) and train_grad_f64_divergence(reach=, mass_q=), and the
        'sinkhorn' dict also has 'reach': True, 'transported' -- the float64 side's smallest transported share over the batch --
        and 'transported_diff', the largest |fp32 side - float64 side| of a problem's share: whether the tape's drift changed what
        the loss gives up.  reach=None is the call without these two keywords."""
        if reach is not None and (eps is None or loss is not None):
            raise ValueError('reach= belongs to the Sinkhorn divergence: give eps and iters, and no loss=')
        if reach is None and mass_q is not None:
            raise ValueError('mass_q belongs to the unbalanced divergence: give reach')
        assert (targets is None) == (target_nums is None)
        assert (eps is None) == (iters is None) and (eps is None or targets is not None)
        if loss is not None and (loss not in L.MATCH_LOSSES or targets is None or eps is not None):
            raise ValueError('loss= takes one of %s, with targets and without eps' % (L.MATCH_LOSSES,))
        # the batch as the fp32 calls take it (one impulse source) and as the float64 calls do (states_delta ignored beside actions)
        five32 = (states, None if actions is not None else states_delta, actions, attrs, particle_nums, particle_dens)
        six = (states, attrs, particle_nums, particle_dens, targets, target_nums)
        seven64 = (states, states_delta, attrs, particle_nums, particle_dens, targets, target_nums)
        self.dispatch_reset()
        # each loss: the fp32 call -> (loss32, g32, the rest); the float64 call on the rest -> (loss64, terms, g64, the rest)
        if loss is not None:
            run32 = lambda: self._train_step32(*five32, targets, target_nums, 'grad', True, loss, match_weight, True)
            run64 = lambda match32: self.train_grad_f64_match(*seven64, loss, match_weight, actions=actions, match_in=match32,
                                                              want_info=True)
        elif eps is not None:
            more = {} if reach is None else {'reach': reach, 'mass_q': mass_q}
            run32 = lambda: self.train_step_divergence(*six, eps, iters, states_delta=five32[1], actions=actions, mode='grad',
                                                       want_grad=True, want_err=reach is not None, **more)
            run64 = lambda *_: self.train_grad_f64_divergence(*seven64, eps, iters, actions=actions, want_err=True, **more)
        else:
            run32 = lambda: self._train_step32(states, states_delta, actions, *five32[3:], targets, target_nums, 'grad', True)
            run64 = lambda _: self._train_grad64(states, states_delta, actions, *five32[3:], targets, target_nums, False)[:4]
        loss32, g32, *rest32 = run32()
        # the fp32 matrix engine's tape is the only user of k_aggregate_tape (pick_tape_engine: selected, or after a range refusal)
        tape = 'mfma' if 'k_aggregate_tape' in self.last_dispatch() else 'fused'
        loss64, _, g64, *rest64 = run64(*rest32)
        tensors, worst = _compare_blobs(g32, g64)
        out = {'tensors': tensors, 'worst': worst, 'rel': tensors[worst]['rel'], 'loss32': loss32, 'loss64': loss64,
               'loss_diff': abs(loss32 - loss64), 'tape': tape}
        if loss is not None:
            match32, info = rest32[0], rest64[0]
            differ = info['match'] != match32
            out['loss_kind'] = loss
            out['flipped'], out['rows_flipped'] = int(differ.any(axis=2).sum()), int(differ.sum())
            out['cost_gap'] = float(((info['cost'] - info['opt_cost']) / np.maximum(info['opt_cost'], 1e-300)).max())
            if info['chamfer_margin'] is not None:
                out['min_margin'] = float(info['chamfer_margin'].min())
            if out['flipped'] > 0:
                own = self.train_grad_f64_match(*seven64, loss, match_weight, actions=actions)
                t_own, w_own = _compare_blobs(g32, own[2])
                out['rel_own'] = t_own[w_own]['rel']
        elif eps is not None:
            out['loss_kind'], out['col_err'], out['self_err'] = 'sinkhorn', float(rest64[0].max()), float(rest64[1].max())
            if reach is not None:
                out['reach'], out['transported'] = True, float(rest64[2].min())
                out['transported_diff'] = float(np.abs(rest32[2] - rest64[2]).max())
        elif targets is not None:
            out['loss_kind'], out['min_margin'] = 'chamfer', float(rest64[0].min())
        return out

    def train_set_lr(self, lr):
        self._ck(self.lib.drp_train_set_lr(self.h, float(lr)))

    # ---- the optimiser seam behind mode='grad' (include/drp.h: drp_train_accumulate, drp_train_apply) -----------------------
    def train_accumulate(self, weight=1.0):
        """Add weight x the gradient of the last trainer pass -- a mode='grad' call of any train_step* method that succeeded -- to
        the float64 accumulator on the device.  A pass is accumulated once; an integer weight (a sample count) is exact."""
        self._ck(self.lib.drp_train_accumulate(self.h, float(weight)))

    def train_apply(self, scale=1.0, max_norm=None, want_grad=False):
        """One Adam step on scale x the accumulated gradient, clipped to the global norm max_norm as torch's clip_grad_norm_ does
        (None: no clipping); the accumulator is cleared -> {'norm': || scale x accumulator ||_2 before clipping, 'clip': the
        factor applied (1.0: none), 'applied': False when the norm was not finite and nothing moved, 'grad': the float32 gradient
        the step was taken on [38403], or None}."""
        norm, clip, applied = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        grad = np.empty((L.DRP_N_WEIGHTS,), np.float32) if want_grad else None
        self._ck(self.lib.drp_train_apply(self.h, float(scale), float('inf') if max_norm is None else float(max_norm),
                                          ctypes.byref(norm), ctypes.byref(clip), ctypes.byref(applied), _opt(_fp, grad)))
        return {'norm': norm.value, 'clip': clip.value, 'applied': bool(applied.value), 'grad': grad}

    def train_get_state(self):
        """Adam's state -> (m [38403] float32, v [38403] float32, the steps taken), in get_weights' layout."""
        m, v = np.empty((L.DRP_N_WEIGHTS,), np.float32), np.empty((L.DRP_N_WEIGHTS,), np.float32)
        it = ctypes.c_int64()
        self._ck(self.lib.drp_train_get_state(self.h, _fp(m), _fp(v), ctypes.byref(it)))
        return m, v, int(it.value)

    def train_set_state(self, m, v, iter):
        """train_get_state's triple back in (after train_begin): the next update continues where that run stood."""
        m, v = _f32(m).reshape(-1), _f32(v).reshape(-1)
        if m.size != L.DRP_N_WEIGHTS or v.size != L.DRP_N_WEIGHTS:
            raise ValueError('m and v must hold %d floats each' % L.DRP_N_WEIGHTS)
        self._ck(self.lib.drp_train_set_state(self.h, _fp(m), _fp(v), int(iter)))

    def get_weights(self):
        blob = np.empty((L.DRP_N_WEIGHTS,), np.float32)
        self._ck(self.lib.drp_get_weights(self.h, _fp(blob), blob.size))
        return blob

    # ---- particle extraction (row f2) -------------------------------------
    def depth2fgpcd(self, depth, mask, cam_params):
        """utils.depth2fgpcd on the device -> [n,3] float64."""
        depth = _f32(depth)
        h, w = depth.shape
        cam = _f64(cam_params)
        m8 = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        mp = None if m8 is None else m8.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        n = ctypes.c_int()
        self._ck(self.lib.drp_depth2fgpcd(self.h, _fp(depth), mp, h, w, _dp(cam), None, 0, ctypes.byref(n)))
        out = np.empty((n.value, 3), np.float64)
        if n.value:
            self._ck(self.lib.drp_depth2fgpcd(self.h, _fp(depth), mp, h, w, _dp(cam), _dp(out), n.value,
                                              ctypes.byref(n)))
        return out

    def downsample_pcd(self, pcd, voxel_size):
        """utils.downsample_pcd (open3d voxel_down_sample) on the device -> [m,3] float64."""
        pcd = _f64(pcd)
        n = pcd.shape[0]
        out = np.empty((n, 3), np.float64)
        m = ctypes.c_int()
        self._ck(self.lib.drp_downsample_pcd(self.h, _dp(pcd), n, float(voxel_size), _dp(out), n, ctypes.byref(m)))
        return out[:m.value].copy()

    def fps_pcd(self, pcd, particle_num, init_idx=None, batch=None, seed=0):
        """utils.fps for a batch of starts -> (pts [batch,N,3] float32, particle_r [batch] float64)."""
        pcd = _f64(pcd)
        if init_idx is not None:
            init = np.ascontiguousarray(np.atleast_1d(init_idx), dtype=np.int32)
            batch = init.shape[0]
            ip = init.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        else:
            batch = int(batch or 1)
            ip = None
        pts = np.empty((batch, int(particle_num), 3), np.float32)
        r = np.empty((batch,), np.float64)
        self._ck(self.lib.drp_fps_pcd(self.h, _dp(pcd), pcd.shape[0], int(particle_num), batch, ip, int(seed),
                                      _fp(pts), _dp(r)))
        return pts, r

    def fps_rad(self, pcd, radius, init_idx, cap=None):
        """utils.fps_rad on the device -> (pcd[chosen] float64, chosen indices)."""
        pcd = _f64(pcd)
        n = pcd.shape[0]
        cap = int(cap or n)
        idx = np.empty((cap,), np.int32)
        cnt = ctypes.c_int()
        self._ck(self.lib.drp_fps_rad(self.h, _dp(pcd), n, float(radius), int(init_idx), cap,
                                      idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(cnt)))
        idx = idx[:cnt.value].copy()
        return pcd[idx], idx

    def recenter(self, pcd, sampled, r):
        """utils.recenter for a batch: sampled [batch,N,3] float32, r [batch] -> [batch,N,3] float32."""
        pcd, sampled = _f64(pcd), _f32(sampled)
        batch, npts, _ = sampled.shape
        rr = _f64(np.broadcast_to(np.asarray(r, dtype=np.float64), (batch,)))
        out = np.empty_like(sampled)
        self._ck(self.lib.drp_recenter(self.h, _dp(pcd), pcd.shape[0], _fp(sampled), npts, batch, _dp(rr), _fp(out)))
        return out

    def obs2ptcl(self, depth_raw, global_scale, cam_params, particle_num, batch, init_idx=None, seed=0):
        """FlexEnv.obs2ptcl_fixed_num_batch on the device -> (ptcl [batch,N,3] f64, particle_r [batch],
        (#foreground points, #voxels))."""
        depth_raw = _f32(depth_raw)
        h, w = depth_raw.shape
        cam = _f64(cam_params)
        ip = None
        if init_idx is not None:
            init = np.ascontiguousarray(init_idx, dtype=np.int32)
            assert init.shape == (batch,)
            ip = init.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        out = np.empty((int(batch), int(particle_num), 3), np.float64)
        r = np.empty((int(batch),), np.float64)
        nfg, nd = ctypes.c_int(), ctypes.c_int()
        self._ck(self.lib.drp_obs2ptcl(self.h, _fp(depth_raw), h, w, float(global_scale), _dp(cam), int(particle_num),
                                       int(batch), ip, int(seed), _dp(out), _dp(r), ctypes.byref(nfg),
                                       ctypes.byref(nd)))
        return out, r, (nfg.value, nd.value)

    # ---- GNN training batches from recorded episodes (row x4) ------------
    def _pd_args(self, depth, names, radius, init_idx, n_fg, episode, cam_params, n_cap, rows):
        """what the two dataset calls marshal alike: depth [*lead, h, w] uint16 with lead = (B,) or (B, T) as `names` says; radius,
        init_idx, n_fg per image, [*lead]; episode [B] or None; cam [4]; per entry r of rows an output of prod(lead) * r * n_cap
        * 3 floats (np.empty: only the pages the call writes are ever touched); counts [*lead]; n_max"""
        a = types.SimpleNamespace()
        a.depth = np.ascontiguousarray(depth, dtype=np.uint16)
        if a.depth.ndim != len(names) + 2:
            raise ValueError('depth must be [%s, h, w], got %s' % (', '.join(names), a.depth.shape))
        a.lead, (a.h, a.w) = a.depth.shape[:-2], a.depth.shape[-2:]
        a.radius, a.init, a.nfg = _f64(radius), _i32(init_idx), _i32(n_fg)
        if len(a.lead) == 1:                # one image per sample: [B], [B, 1], ... alike
            a.radius, a.init, a.nfg = a.radius.reshape(a.lead), a.init.reshape(a.lead), a.nfg.reshape(a.lead)
        for name, x in (('radius', a.radius), ('init_idx', a.init), ('n_fg', a.nfg)):
            if x.shape != a.lead:
                raise ValueError('%s must be [%s] = %s, got %s' % (name, ', '.join(names), a.lead, x.shape))
        a.ep = None if episode is None else _i32(episode).reshape(a.lead[0])
        a.cam = _f64(cam_params).reshape(4)
        n_cap, n_img = int(n_cap), int(np.prod(a.lead))
        a.outs = [np.empty((n_img * r * max(n_cap, 0) * 3,), np.float32) for r in rows]
        a.counts = np.empty(a.lead, np.int32)
        a.n_max = ctypes.c_int()
        # the three argument runs the two C calls share
        a.image = (a.depth.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), a.h, a.w)
        a.per_image = (_dp(a.radius), _ip(a.init), _ip(a.nfg))
        a.tail = (None if a.ep is None else _ip(a.ep), n_cap) + tuple(_fp(o) for o in a.outs) + (_ip(a.counts), ctypes.byref(a.n_max))
        return a

    def ptcl_dataset_batch(self, depth, global_scale, cam_params, T_cam, particles, radius, init_idx, n_fg, push,
                           episode=None, n_cap=L.PD_CAP):
        """ParticleDataset.__getitem__ for B samples on the device, collated (drp_ptcl_dataset_batch).
        depth [B,h,w] uint16; T_cam [4,4] = inv(opencv_T_world); particles: B arrays [T,n_ptcl_b,4] float32; radius [B]
        = 1/sqrt(den); init_idx [B]; n_fg [B] host foreground counts; push [B,T-1,10] float64.
        -> (states [B,T,n_max,3] f32, states_delta [B,T-1,n_max,3] f32, counts [B] int32)"""
        parts = [np.ascontiguousarray(p, dtype=np.float32) for p in particles]
        T = parts[0].shape[0]
        a = self._pd_args(depth, ('B',), radius, init_idx, n_fg, episode, cam_params, n_cap, (T, T - 1))
        B, = a.lead
        if len(parts) != B:
            raise ValueError('%d particle arrays for %d depth images' % (len(parts), B))
        for p in parts:
            if p.ndim != 3 or p.shape[0] != T or p.shape[2] != 4:
                raise ValueError('particles must be [T, n, 4] with one T for the batch, got %s' % (p.shape,))
        n_ptcl = np.array([p.shape[1] for p in parts], np.int32)
        flat = np.concatenate([p.ravel() for p in parts]) if B > 1 else parts[0].ravel()
        push = _f64(push)
        if push.shape != (B, T - 1, 10):
            raise ValueError('push must be [B, T-1, 10] = %s, got %s' % ((B, T - 1, 10), push.shape))
        Tm = _f64(T_cam).reshape(16)
        self._ck(self.lib.drp_ptcl_dataset_batch(
            self.h, B, *a.image, float(global_scale), _dp(a.cam), _dp(Tm), T, _ip(n_ptcl), _fp(flat), *a.per_image, _dp(push),
            *a.tail))
        nm = a.n_max.value
        self._pd_shape = (B, nm)
        states, sdelta = a.outs
        return (states[:B * T * nm * 3].reshape(B, T, nm, 3), sdelta[:B * (T - 1) * nm * 3].reshape(B, T - 1, nm, 3),
                a.counts)

    def ptcl_dataset_frames(self, depth, global_scale, cam_params, radius, init_idx, n_fg, episode=None, n_cap=L.PD_CAP):
        """depth2fgpcd -> fps_rad -> recenter on every frame of B windows of T depth frames (drp_ptcl_dataset_frames): untracked
        training samples without a particle file.  depth [B,T,h,w] uint16; radius, init_idx, n_fg [B,T] (fps_rad's radius, the
        sampler's start and the host's foreground count of every frame); B * T <= 1024.
        -> (clouds [B,T,n_max,3] f32, +0.0 beyond each count; counts [B,T] int32)"""
        a = self._pd_args(depth, ('B', 'T'), radius, init_idx, n_fg, episode, cam_params, n_cap, (1,))
        B, T = a.lead
        self._pdf_shape = (0, 0, 0)
        self._ck(self.lib.drp_ptcl_dataset_frames(self.h, B, T, *a.image, float(global_scale), _dp(a.cam), *a.per_image, *a.tail))
        nm = a.n_max.value
        self._pdf_shape = (B, T, nm)
        return a.outs[0][:B * T * nm * 3].reshape(B, T, nm, 3), a.counts

    def _pd_tap(self, prefix, names, lead, nm, name):
        """one of the intermediates `names` of the last dataset call over images [*lead]: the debug tap prefix + name"""
        if name not in names:
            raise KeyError(name)
        shape, dt = {'nfg': ((), np.int32), 'chosen': ((L.PD_CAP + 1,), np.int32), 'recenter': ((nm, 3), np.float64),
                     'nearest': ((nm,), np.int32)}[name]
        return self.debug_fetch(prefix + name, tuple(lead) + shape, dt)

    def ptcl_dataset_frames_tap(self, name):
        """intermediates of the last ptcl_dataset_frames: 'nfg' [B,T], 'chosen' [B,T,4097], 'recenter' [B,T,n_max,3] float64.
        Refused (DrpError) when a ptcl_dataset_batch has run since: the two calls share their buffers"""
        B, T, nm = getattr(self, '_pdf_shape', (0, 0, 0))
        return self._pd_tap('pdf_', ('nfg', 'chosen', 'recenter'), (B, T), nm, name)

    def ptcl_dataset_time(self):
        """device ms of the last ptcl_dataset_batch / ptcl_dataset_frames by stage: {'upload', 'compaction', 'fps_rad', 'recenter',
        'track_pack', 'download'}; after a ptcl_dataset_frames 'track_pack' is the pack alone"""
        ms = np.empty((6,), np.float32)
        self._ck(self.lib.drp_ptcl_dataset_time(self.h, _fp(ms)))
        return dict(zip(('upload', 'compaction', 'fps_rad', 'recenter', 'track_pack', 'download'), ms.tolist()))

    def ptcl_dataset_tap(self, name):
        """intermediates of the last ptcl_dataset_batch: 'nfg' [B], 'chosen' [B,4097], 'recenter' [B,n_max,3] float64,
        'nearest' [B,n_max]"""
        B, nm = getattr(self, '_pd_shape', (0, 0))
        return self._pd_tap('pd_', ('nfg', 'chosen', 'recenter', 'nearest'), (B,), nm, name)

    # ---- gradient-descent planner ---------------------------------------
    def gd_begin(self, s0, attr, dens, actions, lr, act_lo, act_hi):
        s0, attr, dens, actions = _f32(s0), _f32(attr), _f32(dens), _f32(actions)
        nb, N, _ = s0.shape
        B, H, _ = actions.shape
        lo, hi = _f32(act_lo), _f32(act_hi)
        self._ck(self.lib.drp_gd_begin(self.h, _fp(s0), _fp(attr), _fp(dens), nb, N, _fp(actions), B, H,
                                       float(lr), _fp(lo), _fp(hi)))
        self._gd = (B, H, N)

    def gd_begin_scenes(self, s0, attr, dens, actions, lr, act_lo, act_hi):
        """gd_begin over S scenes on the installed goal table (include/drp.h: drp_gd_begin_scenes): s0 [S,nb,N,3], attr [S,nb,N],
        dens [S,nb], actions [B,H,4] in scene_rows' layout (B a multiple of S * nb).  gd_grad, gd_step, gd_step_async / gd_wait
        and gd_actions then run as in a single-scene session."""
        s0, attr, dens, actions = _f32(s0), _f32(attr), _f32(dens), _f32(actions)
        assert s0.ndim == 4
        S, nb, N, _ = s0.shape
        B, H, _ = actions.shape
        assert attr.shape == (S, nb, N) and dens.shape == (S, nb)
        lo, hi = _f32(act_lo), _f32(act_hi)
        self._ck(self.lib.drp_gd_begin_scenes(self.h, int(S), _fp(s0), _fp(attr), _fp(dens), nb, N, _fp(actions), B, H,
                                              float(lr), _fp(lo), _fp(hi)))
        self._gd = (B, H, N)

    def gd_grad(self, want_state_grad=False):
        B, H, N = self._gd
        r = np.empty((B,), np.float32)
        g = np.empty((B, H, 4), np.float32)
        gs = np.empty((B, H, N, 3), np.float32) if want_state_grad else None
        self._ck(self.lib.drp_gd_grad(self.h, _fp(r), _fp(g), _fp(gs) if want_state_grad else None))
        return r, g, gs

    def gd_step(self):
        B, H, N = self._gd
        r = np.empty((B,), np.float32)
        self._ck(self.lib.drp_gd_step(self.h, _fp(r)))
        return r

    def gd_step_async(self, slot):
        """Enqueue one iteration; its rewards and updated pushes go to pinned memory behind it (gd_wait)."""
        self._ck(self.lib.drp_gd_step_async(self.h, int(slot)))

    def gd_wait(self, slot):
        """(rewards [B] of the iterate before the update, pushes [B,H,4] after it) of the iteration in `slot`."""
        B, H, N = self._gd
        r = np.empty((B,), np.float32)
        a = np.empty((B, H, 4), np.float32)
        self._ck(self.lib.drp_gd_wait(self.h, int(slot), _fp(r), _fp(a)))
        return r, a

    def gd_actions(self):
        B, H, N = self._gd
        a = np.empty((B, H, 4), np.float32)
        self._ck(self.lib.drp_gd_get(self.h, _fp(a)))
        return a

    # ---- planning on a caller's cost (include/drp.h: drp_gd_begin_cost, drp_gd_predict, drp_gd_*_seeded) --------------------
    def gd_begin_cost(self, s0, attr, dens, actions, lr, act_lo, act_hi):
        """gd_begin without a goal: a session on a cost of the caller's.  gd_predict, gd_grad_seeded, gd_step_seeded and
        gd_actions run in it; gd_grad, gd_step and gd_step_async are refused."""
        s0, attr, dens, actions = _f32(s0), _f32(attr), _f32(dens), _f32(actions)
        nb, N, _ = s0.shape
        B, H, _ = actions.shape
        lo, hi = _f32(act_lo), _f32(act_hi)
        self._ck(self.lib.drp_gd_begin_cost(self.h, _fp(s0), _fp(attr), _fp(dens), nb, N, _fp(actions), B, H,
                                            float(lr), _fp(lo), _fp(hi)))
        self._gd = (B, H, N)

    def _gd_seed(self, seed):
        B, H, N = self._gd
        seed = _f32(seed)
        if seed.shape != (B, H, N, 3):
            raise ValueError('seed %s, the session wants %s' % (seed.shape, (B, H, N, 3)))
        return seed

    def gd_predict(self):
        """Every step's predicted state [B,H,N,3] on the session's current pushes: the forward as gd_grad runs it, no reward;
        the session is left as it was."""
        B, H, N = self._gd
        out = np.empty((B, H, N, 3), np.float32)
        self._ck(self.lib.drp_gd_predict(self.h, _fp(out)))
        return out

    def gd_grad_seeded(self, seed, want_state_grad=False):
        """The reverse pass from the caller's complete d loss / d s_pred [B,H,N,3] (the library minimises) -> (d loss / d pushes
        [B,H,4], d loss / d state [B,H,N,3] with the seed included, or None)."""
        B, H, N = self._gd
        seed = self._gd_seed(seed)
        g = np.empty((B, H, 4), np.float32)
        gs = np.empty((B, H, N, 3), np.float32) if want_state_grad else None
        self._ck(self.lib.drp_gd_grad_seeded(self.h, _fp(seed), _fp(g), _fp(gs) if want_state_grad else None))
        return g, gs

    def gd_step_seeded(self, seed):
        """gd_grad_seeded plus gd_step's Adam step and clip -> the updated pushes [B,H,4]."""
        B, H, N = self._gd
        seed = self._gd_seed(seed)
        a = np.empty((B, H, 4), np.float32)
        self._ck(self.lib.drp_gd_step_seeded(self.h, _fp(seed), _fp(a)))
        return a

    def gd_predict_f64(self, s0, attr, dens, actions):
        """The float64 forward of one GD iteration -> every step's predicted state [B,H,N,3] float64; gd_grad_f64's one-shot
        contract, no goal needed."""
        s0, attr, dens, actions = _f32(s0), _f32(attr), _f32(dens), _f32(actions)
        nb, N, _ = s0.shape
        B, H, _ = actions.shape
        out = np.empty((B, H, N, 3), np.float64)
        self._ck(self.lib.drp_gd_predict_f64(self.h, _fp(s0), _fp(attr), _fp(dens), int(nb), int(N), _fp(actions), int(B), int(H),
                                             _dp(out)))
        return out

    def gd_grad_f64_seeded(self, s0, attr, dens, actions, seed, want_state_grad=False):
        """The float64 reverse pass from the caller's seed [B,H,N,3] (float64) -> d loss / d pushes [B,H,4][, d loss / d state
        [B,H,N,3]] as float64: the yardstick of gd_grad_seeded."""
        s0, attr, dens, actions = _f32(s0), _f32(attr), _f32(dens), _f32(actions)
        nb, N, _ = s0.shape
        B, H, _ = actions.shape
        seed = np.ascontiguousarray(seed, dtype=np.float64)
        if seed.shape != (B, H, N, 3):
            raise ValueError('seed %s, the inputs want %s' % (seed.shape, (B, H, N, 3)))
        g = np.empty((B, H, 4), np.float64)
        gs = np.empty((B, H, N, 3), np.float64) if want_state_grad else None
        self._ck(self.lib.drp_gd_grad_f64_seeded(self.h, _fp(s0), _fp(attr), _fp(dens), int(nb), int(N), _fp(actions), int(B),
                                                 int(H), _dp(seed), _dp(g), _dp(gs) if want_state_grad else None))
        return (g, gs) if want_state_grad else g

    def gradient_probe_cost(self, cost, s0, attr, dens, actions, act_lo, act_hi, context=None):
        """gradient_probe for a cost of the caller's (costs.py: cost(pred, context, want_grad) -> (values [B], grad [B,H,N,3])):
        gd_begin_cost + gd_predict + cost + gd_grad_seeded on whatever tape the selection gives, against gd_predict_f64 + the
        cost on the float64 prediction + gd_grad_f64_seeded on the same inputs -> gradient_probe's dict ('reward_rel' compares
        -values) plus 'seed_rel': max |seed(pred32) - seed(pred64)| / max |seed(pred64)|, how far the cost's own gradient moves
        under the fp32 drift of the prediction.  It ENDS a running planner session and resets the dispatch marks."""
        self.dispatch_reset()
        self.gd_begin_cost(s0, attr, dens, actions, 0.05, act_lo, act_hi)
        pred32 = self.gd_predict()
        v32, seed32 = cost(pred32, context, True)
        g32, _ = self.gd_grad_seeded(seed32)
        tape = 'mfma' if 'k_aggregate_tape' in self.last_dispatch() else 'fused'
        pred64 = self.gd_predict_f64(s0, attr, dens, actions)
        v64, seed64 = cost(pred64, context, True)
        seed64 = np.asarray(seed64, np.float64)
        g64 = self.gd_grad_f64_seeded(s0, attr, dens, actions, seed64)
        err = np.abs(g32.astype(np.float64) - g64).ravel()
        err = np.where(np.isnan(err), np.inf, err)
        scale = float(np.abs(g64).max())
        a = float(err.max())
        v64 = np.asarray(v64, np.float64)
        rscale = float(np.abs(v64).max())
        sscale = float(np.abs(seed64).max())
        return {'abs': a, 'scale': scale, 'rel': a / max(scale, 1e-300), 'worst': int(np.argmax(err)),
                'reward_rel': float(np.abs(np.asarray(v32, np.float64) - v64).max()) / max(rscale, 1e-300), 'tape': tape,
                'seed_rel': float(np.abs(np.asarray(seed32, np.float64) - seed64).max()) / max(sscale, 1e-300)}

    def mpc_begin_cost(self, s0, attr, dens, nominal, n_sample, sigma, beta_filter, reward_weight,
                       act_lo, act_hi, seed=0, sample_offset=0, noise_type='normal'):
        """mpc_begin without a goal: mpc_rollout then runs no reward kernel; read the states (mpc_get), compute a reward per
        row and hand them in (mpc_set_rewards) before the update."""
        s0, attr, dens = _f32(s0), _f32(attr), _f32(dens)
        nominal = np.ascontiguousarray(nominal, dtype=np.float64)
        nb, N, _ = s0.shape
        H = nominal.shape[0]
        p = L.MpcParams()
        p.n_batch, p.n_particles, p.n_sample, p.n_look_ahead = nb, N, int(n_sample), H
        p.sigma, p.beta_filter, p.reward_weight = float(sigma), float(beta_filter), float(reward_weight)
        for i in range(4):
            p.act_lo[i] = float(act_lo[i])
            p.act_hi[i] = float(act_hi[i])
        p.seed, p.sample_offset = int(seed), int(sample_offset)
        p.noise_type, p.reserved = L.NOISE_TYPES[noise_type], 0
        self._ranged(lambda: self.lib.drp_mpc_begin_cost(self.h, ctypes.byref(p), _fp(s0), _fp(attr), _fp(dens), _dp(nominal)))
        self.H, self.nb, self.N, self.ns = H, nb, N, int(n_sample)
        self.S = 0

    def mpc_set_rewards(self, rewards):
        """The final-step reward of every row [n_sample * nb] of the last rollout, in the slot the update kernels read."""
        rewards = _f32(rewards)
        if rewards.shape != (self.ns * self.nb,):
            raise ValueError('rewards %s, the session has %d rows' % (rewards.shape, self.ns * self.nb))
        self._ck(self.lib.drp_mpc_set_rewards(self.h, _fp(rewards)))

    # ---- planning to a target cloud on the device (include/drp.h: drp_set_goal_cloud, drp_mpc_begin_cloud, drp_gd_begin_cloud) ----
    cloud_goal = None       # the installed cloud goal: {'kind', 'weight', 'eps_scale', 'iters', 'M'}

    def set_goal_cloud(self, target, kind='chamfer', weight=1.0, eps_scale=1.0, iters=50):
        """Install one target cloud [M, 3] (camera frame, as the predicted states) beside the image goal: the goal of
        mpc_begin_cloud / gd_begin_cloud sessions and of cloud_goal_eval.  kind 'chamfer': reward = -weight * (fwd + bwd) of
        cloud_chamfer(final state, target); 'sinkhorn': -weight * cloud_divergence(final state, target) with eps = eps_scale /
        dens[column] and `iters` sweeps.  One cloud for every row: a cloud per scene ([S, M, 3]) and a reach (unbalanced
        masses) are not supported."""
        if kind not in L.CLOUD_GOAL_KINDS:
            raise ValueError('unknown cloud goal kind %r (one of %s)' % (kind, sorted(L.CLOUD_GOAL_KINDS)))
        target = _f32(target)
        if target.ndim == 3:
            raise ValueError('a cloud goal is ONE target [M, 3] shared by every row, got %s: a goal cloud per scene '
                             '(multi-scene sessions) is not supported' % (target.shape,))
        if target.ndim != 2 or target.shape[1] != 3:
            raise ValueError('target must be [M, 3], got %s' % (target.shape,))
        p = L.CloudGoalParams()
        p.kind, p.iters, p.weight, p.eps_scale = L.CLOUD_GOAL_KINDS[kind], int(iters), float(weight), float(eps_scale)
        self._ck(self.lib.drp_set_goal_cloud(self.h, _fp(target), int(target.shape[0]), ctypes.byref(p)))
        self.cloud_goal = {'kind': kind, 'weight': float(weight), 'eps_scale': float(eps_scale), 'iters': int(iters),
                           'M': int(target.shape[0])}

    def mpc_begin_cloud(self, s0, attr, dens, nominal, n_sample, sigma, beta_filter, reward_weight,
                        act_lo, act_hi, seed=0, sample_offset=0, noise_type='normal'):
        """mpc_begin with the installed cloud goal in the image's place: mpc_rollout then ends in the cloud reward kernel on every
        row's final state; every later session call works as after mpc_begin.  Single-scene (s0 [nb, N, 3])."""
        s0, attr, dens = _f32(s0), _f32(attr), _f32(dens)
        if s0.ndim != 3:
            raise ValueError('a cloud session plans one scene: s0 must be [n_batch, N, 3], got %s (multi-scene cloud sessions '
                             'are not supported)' % (s0.shape,))
        nominal = np.ascontiguousarray(nominal, dtype=np.float64)
        nb, N, _ = s0.shape
        H = nominal.shape[0]
        p = L.MpcParams()
        p.n_batch, p.n_particles, p.n_sample, p.n_look_ahead = nb, N, int(n_sample), H
        p.sigma, p.beta_filter, p.reward_weight = float(sigma), float(beta_filter), float(reward_weight)
        for i in range(4):
            p.act_lo[i] = float(act_lo[i])
            p.act_hi[i] = float(act_hi[i])
        p.seed, p.sample_offset = int(seed), int(sample_offset)
        p.noise_type, p.reserved = L.NOISE_TYPES[noise_type], 0
        self._ranged(lambda: self.lib.drp_mpc_begin_cloud(self.h, ctypes.byref(p), _fp(s0), _fp(attr), _fp(dens), _dp(nominal)))
        self.H, self.nb, self.N, self.ns = H, nb, N, int(n_sample)
        self.S = 0

    def gd_begin_cloud(self, s0, attr, dens, actions, lr, act_lo, act_hi):
        """gd_begin with the installed cloud goal in the image's place: gd_grad, gd_step, gd_step_async / gd_wait and gd_actions
        run as in a goal session, one forward per iteration and no seed on the bus.  Single-scene (s0 [nb, N, 3])."""
        s0, attr, dens, actions = _f32(s0), _f32(attr), _f32(dens), _f32(actions)
        if s0.ndim != 3:
            raise ValueError('a cloud session plans one scene: s0 must be [n_batch, N, 3], got %s (multi-scene cloud sessions '
                             'are not supported)' % (s0.shape,))
        nb, N, _ = s0.shape
        B, H, _ = actions.shape
        lo, hi = _f32(act_lo), _f32(act_hi)
        self._ck(self.lib.drp_gd_begin_cloud(self.h, _fp(s0), _fp(attr), _fp(dens), nb, N, _fp(actions), B, H,
                                             float(lr), _fp(lo), _fp(hi)))
        self._gd = (B, H, N)

    def cloud_goal_eval(self, p, n_p=None, dens=None, want_grad=False):
        """The installed cloud goal on the caller's clouds p [B, N, 3] (or one cloud [N, 3]; n_p [B]: real rows, default all;
        dens [B] or a number: the sinkhorn kind's eps = eps_scale / dens) -> {'rewards' [B] float32, 'values' [B] float64 =
        weight * value[, 'grad' [B, N, 3] float32 = d values / d p, +0.0 on padding]}.  A one-shot: it needs no weights and ends
        no session.  A row with a non-finite coordinate gets a NaN reward; the other rows are untouched by it."""
        p = _f32(p)
        if p.ndim == 2:
            p = p[None]
        assert p.ndim == 3 and p.shape[2] == 3
        B, N = int(p.shape[0]), int(p.shape[1])
        n_p = None if n_p is None else np.ascontiguousarray(np.broadcast_to(_i32(n_p).reshape(-1), (B,)))
        dens = None if dens is None else np.ascontiguousarray(np.broadcast_to(_f32(dens).reshape(-1), (B,)))
        rewards = np.empty((B,), np.float32)
        values = np.empty((B,), np.float64)
        grad = np.empty((B, N, 3), np.float32) if want_grad else None
        self._ck(self.lib.drp_cloud_goal_eval(self.h, _fp(p), _ip(n_p) if n_p is not None else None,
                                              _fp(dens) if dens is not None else None, B, N, _fp(rewards), _dp(values),
                                              _fp(grad) if want_grad else None))
        out = {'rewards': rewards, 'values': values}
        if want_grad:
            out['grad'] = grad
        return out

    # ---- multi-GPU ------------------------------------------------------------------
    def comm_unique_id(self):
        buf = ctypes.create_string_buffer(128)
        rc = self.lib.drp_comm_unique_id(buf)
        if rc != 0:
            raise L.DrpError('drp_comm_unique_id failed: %s' % self.lib.drp_last_error(None).decode())
        return buf.raw

    def comm_init(self, uid, rank, n_ranks):
        self._ck(self.lib.drp_comm_init(self.h, uid, int(rank), int(n_ranks)))
        self._n_ranks = int(n_ranks)

    def comm_destroy(self):
        self._ck(self.lib.drp_comm_destroy(self.h))
        self._n_ranks = 1

    def comm_info(self):
        """{'n_ranks': ncclCommCount (0 without a communicator), 'rank', 'version', 'path'} of the RCCL this process bound."""
        n, r, v = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        path = ctypes.create_string_buffer(1024)
        self._ck(self.lib.drp_comm_info(self.h, ctypes.byref(n), ctypes.byref(r), ctypes.byref(v), path, 1024))
        ver = v.value
        return {'n_ranks': n.value, 'rank': r.value, 'version': ver, 'path': path.value.decode(),
                'version_str': '%d.%d.%d' % (ver // 10000, (ver // 100) % 100, ver % 100) if ver >= 10000 else str(ver)}

    def debug_stall(self, ms):
        self._ck(self.lib.drp_debug_stall(self.h, int(ms)))

    def comm_allgather(self, arr):
        """All-gather one host array per rank over the context's communicator -> [n_ranks, *arr.shape]."""
        arr = np.ascontiguousarray(arr)
        # the communicator's own count, not a cached one: an aborted communicator is gone (and the call below says so)
        out = np.empty((max(1, self.comm_info()['n_ranks']),) + arr.shape, arr.dtype)
        self._ck(self.lib.drp_comm_allgather(self.h, arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes,
                                             out.ctypes.data_as(ctypes.c_void_p)))
        return out

    # ---- measurement ------------------------------------------------------------------
    def sync(self):
        self._ck(self.lib.drp_sync(self.h))

    def probe_begin(self, kernel_class):
        self._ck(self.lib.drp_probe_begin(self.h, kernel_class.encode() if kernel_class else None))

    def probe_read(self):
        ms = ctypes.c_double()
        n = ctypes.c_long()
        self._ck(self.lib.drp_probe_read(self.h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def probe_prop_launches(self):
        """Kernel launches inside the regions of the 'prop' probe since probe_begin: probe_read counts regions, and a region
        covers one launch per block of a batch that is cut (include/drp.h: drp_probe_prop_launches)."""
        n = ctypes.c_long()
        self._ck(self.lib.drp_probe_prop_launches(self.h, ctypes.byref(n)))
        return n.value

    def probe_work(self):
        """What the propagation kernels executed since probe_begin('prop'), counted by the kernels (include/drp.h)."""
        out = (ctypes.c_ulonglong * 8)()
        self._ck(self.lib.drp_probe_work(self.h, out))
        keys = ('chain_slots', 'cached_slots', 'tiles', 'tiles_last', 'encoder_tiles', 'mfmas', 'clk_cycles', 'clk_ticks')
        return {k: int(out[i]) for i, k in enumerate(keys)}

    def dispatch_reset(self):
        self._ck(self.lib.drp_dispatch_reset(self.h))

    def last_dispatch(self):
        """Names of the kernel variants launched since dispatch_reset() (include/drp.h drp_last_dispatch)."""
        buf = ctypes.create_string_buffer(8192)
        self._ck(self.lib.drp_last_dispatch(self.h, buf, len(buf)))
        return [s for s in buf.value.decode().split(';') if s]

    def dispatch_variants(self, default_only=True):
        buf = ctypes.create_string_buffer(8192)
        self.lib.drp_dispatch_variants(int(bool(default_only)), buf, len(buf))
        return [s for s in buf.value.decode().split(';') if s]

    def range_info(self):
        """{'shift', 'bound', 'wmax', 'ok'} of the split-fp16 relation encoder for the loaded weights (drp_range_info); after
        load_weights(probe=...) also 'probe': {'abs', 'disp', 'disp_rel', 'worst', 'engine'}, after load_weights(max_grad_rel=...)
        'grad_probe': what gradient_probe returned."""
        k, ok = ctypes.c_int(), ctypes.c_int()
        bound, wmax = ctypes.c_double(), ctypes.c_double()
        self._ck(self.lib.drp_range_info(self.h, ctypes.byref(k), ctypes.byref(bound), ctypes.byref(wmax), ctypes.byref(ok)))
        info = {'shift': k.value, 'bound': bound.value, 'wmax': wmax.value, 'ok': bool(ok.value)}
        if getattr(self, '_probe', None) is not None:
            info['probe'] = dict(self._probe)         # what load_weights(probe=...) measured, and on which engine
        if getattr(self, '_grad_probe', None) is not None:
            info['grad_probe'] = dict(self._grad_probe)       # what load_weights(max_grad_rel=...) measured, and on which tape
        return info

    def debug_fetch(self, name, shape, dtype=np.float32):
        out = np.empty(shape, dtype=dtype)
        self._ck(self.lib.drp_debug_fetch(self.h, name.encode(), out.ctypes.data_as(ctypes.c_void_p),
                                          out.nbytes))
        return out

    WGRAD_JOB_FIELDS = ('M', 'in', 'rows_per_sample', 'dens_mod', 'blocks', 'lane_stride', 'k_stride', 'dW', 'db', 'dwd', 'dens')

    def train_wgrad_jobs(self):
        """The weight-gradient sums of the last trainer pass that ran a reverse pass with deferred weight gradients (the debug
        taps "train_wgrad_*" of include/drp.h): a list of dicts over WGRAD_JOB_FIELDS, the jobs in queue order and the column sums
        of the predictor's last bias behind them ('dW', 'db', 'dwd': offsets in floats inside the gradient blob, -1 for none;
        'dens': whether the job reads the densities).  Refused (DrpError) when the last pass did not defer, ran no reverse pass,
        or a later call has reused its buffers."""
        nf = len(self.WGRAD_JOB_FIELDS)
        buf = np.empty((18 * 64 + 1, nf), np.int64)             # the most a pass queues: 18 jobs a rollout step, 64 steps
        n = self.lib.drp_debug_fetch(self.h, b'train_wgrad_jobs', buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes)
        self._ck(n)
        return [dict(zip(self.WGRAD_JOB_FIELDS, (int(v) for v in rec))) for rec in buf[:n // (8 * nf)]]

    def train_wgrad_tap(self):
        """train_wgrad_jobs() with the rows the sums were taken over -> (jobs, [(g [M,64], x [M,in]) per job, then (g [M,3], None)
        of the column sums], the densities [dens_mod] the jobs read): everything tests/_wgrad_ref.py reconstructs the gradient
        blob from, as float32 copies of what lay in device memory."""
        jobs = self.train_wgrad_jobs()
        ops = []
        for q, j in enumerate(jobs[:-1]):
            ops.append((self.debug_fetch('train_wgrad_g:%d' % q, (j['M'], 64)), self.debug_fetch('train_wgrad_x:%d' % q, (j['M'], j['in']))))
        ops.append((self.debug_fetch('train_wgrad_g:%d' % (len(jobs) - 1), (jobs[-1]['M'], 3)), None))
        n_dens = max([j['dens_mod'] for j in jobs[:-1] if j['dens']] or [0])
        dens = self.debug_fetch('train_wgrad_dens', (n_dens,)) if n_dens else np.zeros((0,), np.float32)
        return jobs, ops, dens
