"""GPU: planning to a target cloud on the device -- drp_set_goal_cloud, drp_mpc_begin_cloud, drp_gd_begin_cloud,
drp_cloud_goal_eval (csrc/k_cloud_goal.h, csrc/capi_cloud_goal.h).

The cloud kernels restate the one-shots' arithmetic (kc_chamfer, the Sinkhorn bodies) for one target shared by every row, so
they are held to the one-shots' BITS: rewards are np.float32(-(np.float64(w) * value)) of Engine.cloud_chamfer /
Engine.cloud_divergence on (final state of the row, target), gradients the one-shot's.  The gradient's product with the weight
is formed in double before the one rounding; the weights of the gradient tests are powers of two (2.0, 0.5), for which that is
w x the one-shot's fp32 gradient exactly, so a seed formed on the host as w x the one-shot's fp32 gradient (scaled in float64,
rounded once) is the kernel's number; the
reward tests use a weight that is no power of two (1.7).  Against float64 every row's Chamfer reward is held to REL = 1e-6 of
tests/test_gpu_chamfer.py (four fp32 roundings of a squared distance, a margin of 4x) plus the one rounding of the reward to fp32.

Shapes: 6 samples x n_batch 2 (two densities) x H 2 = 12 rows: H = 2 exercises the strided reward slot and the final-step
offset of the states, two columns row % n_batch.  Chamfer pairs (N, M): (17, 12), (40, 257) one past KC_THREADS on the target
side, (300, 40) past it on the prediction side, (9, 1030) one LDS tile and a remainder.  Sinkhorn pairs: (12, 20), (20, 12),
(33, 33), iters 10."""
import ctypes

import numpy as np
import pytest

import _divergence_ref as D
import _gd_seeded_ref as S
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd import _lib as L
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.planners import world2cam_affine

pytestmark = pytest.mark.gpu
M34 = world2cam_affine(syn.demo_cam_extrinsics())
CAM = syn.demo_cam_params()
LO, HI = syn.action_limits()
NS, NB, H = 6, 2, 2
ROWS = NS * NB
REL = 1e-6                      # tests/test_gpu_chamfer.py's bound on fwd and bwd
DIV_VALUE_BOUND = 5 * 1.2e-14   # tests/test_gpu_divergence.py's BOUND['value']
CHAMFER_PAIRS = [(17, 12), (40, 257), (300, 40), (9, 1030)]
SINKHORN_PAIRS = [(12, 20), (20, 12), (33, 33)]
ITERS = 10
FP = ctypes.POINTER(ctypes.c_float)


def new_engine(w):
    e = Engine(0)
    e.load_weights(weights.blob_from_state_dict(w), 0.08)
    e.set_camera(M34, 24.0, CAM)
    return e


@pytest.fixture(scope='module')
def engines(golden):
    """a context for the cloud sessions and one for the cost sessions they are held against; neither ever sees an image goal"""
    es = (new_engine(golden.weights_seed0), new_engine(golden.weights_seed0))
    yield es
    for e in es:
        e.close()


_cases = {}


def case(N, M):
    """12 rows of pushes on two start columns of different density, and a target of M points: another pile, a little aside"""
    if (N, M) not in _cases:
        c = S.make_case(N, H, nb=NB, B=ROWS)
        c['dens'] = (c['dens'] * np.array([1.0, 1.5], np.float32)).astype(np.float32)
        c['target'] = (syn.make_pile(M, 1, seed=1000 + M)[0][0] + np.array([0.02, -0.01, 0.0], np.float32)).astype(np.float32)
        for v in c.values():
            v.setflags(write=False)
        _cases[(N, M)] = c
    return _cases[(N, M)]


def install(e, c, kind, w):
    e.set_goal_cloud(c['target'], kind=kind, weight=w, eps_scale=1.0, iters=ITERS)


def mpc_begin(e, c, how, ns=NS, seed=1234):
    nominal = syn.nominal_pushes(H, 0).astype(np.float64)
    getattr(e, how)(c['s_cur'], c['attr'], c['dens'], nominal, ns, 0.6, 0.7, 10.0, LO, HI, seed=seed)


def one_shot(e, c, kind, final, want_grad=False, dens=None):
    """the one-shot of the kind on (final [rows, N, 3], the target broadcast) -> (values float64 [rows], grad or None)"""
    rows = final.shape[0]
    q = np.ascontiguousarray(np.broadcast_to(c['target'][None], (rows,) + c['target'].shape))
    if kind == 'chamfer':
        out = e.cloud_chamfer(np.ascontiguousarray(final), q, want_grad=want_grad)
        return out['fwd'] + out['bwd'], out.get('grad')
    dens = c['dens'] if dens is None else dens
    eps = 1.0 / np.resize(np.asarray(dens, np.float64), rows)           # eps_scale / dens[row % n_batch]
    out = e.cloud_divergence(np.ascontiguousarray(final), q, eps=eps, iters=ITERS, want_grad=want_grad)
    return out['divergence'], out.get('grad')


def rewards_of(values, w):
    return np.float32(-(np.float64(w) * values))


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def rolled(e, c, kind, w):
    """a cloud session, the case's pushes, one rollout -> mpc_get's rewards and states"""
    install(e, c, kind, w)
    mpc_begin(e, c, 'mpc_begin_cloud')
    e.mpc_set_actions(c['act_seqs'])
    e.mpc_rollout()
    return e.mpc_get(rewards=True, rewards_all=True, states=True)


# ---- 1. the rewards of a sampling session ------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,M', CHAMFER_PAIRS)
def test_chamfer_rewards_are_the_one_shots_bits(engines, N, M):
    e, c, w = engines[0], case(N, M), 1.7
    got = rolled(e, c, 'chamfer', w)
    final = got['states'][:, H - 1]
    assert np.all(np.isfinite(final)) and not np.array_equal(final[0], final[NB])      # the rows differ: another push
    values, _ = one_shot(e, c, 'chamfer', final)
    assert same_bits(got['rewards'], rewards_of(values, w))
    assert same_bits(got['rewards_all'][:, H - 1], got['rewards'])                      # the strided slot
    n_p, n_q = np.full(ROWS, N), np.full(ROWS, M)
    ref = U.chamfer64(final, np.broadcast_to(c['target'][None], (ROWS, M, 3)), n_p, n_q)
    want = -(w * (ref['fwd'] + ref['bwd']))
    rel = float((np.abs(got['rewards'].astype(np.float64) - want) / np.abs(want)).max())       # per row, as tests/test_gpu_chamfer.py
    print('[cloud-goal] chamfer %d x %d: rewards against float64, worst row %.2e of its own value (bound %.1e + one fp32 rounding)' % (N, M, rel, REL))
    assert rel <= REL + 2.0 ** -24


@pytest.mark.parametrize('N,M', SINKHORN_PAIRS)
def test_sinkhorn_rewards_are_the_one_shots_bits_per_column(engines, N, M):
    e, c, w = engines[0], case(N, M), 1.7
    got = rolled(e, c, 'sinkhorn', w)
    final = got['states'][:, H - 1]
    values, _ = one_shot(e, c, 'sinkhorn', final)
    assert np.all(values > 0)
    assert same_bits(got['rewards'], rewards_of(values, w))
    # the two columns' densities swapped: the states move (the model reads the density), the rewards move exactly as the
    # one-shot's with the swapped eps -- the per-column table
    sw = dict(c)
    sw['dens'] = np.ascontiguousarray(c['dens'][::-1])
    got2 = rolled(e, sw, 'sinkhorn', w)
    final2 = got2['states'][:, H - 1]
    values2, _ = one_shot(e, c, 'sinkhorn', final2, dens=sw['dens'])
    assert same_bits(got2['rewards'], rewards_of(values2, w))
    assert not same_bits(got2['rewards'], got['rewards'])
    # and on the SAME clouds the table alone: eval with each column's density
    a = e.cloud_goal_eval(final, dens=np.resize(c['dens'], ROWS))
    b = e.cloud_goal_eval(final, dens=np.resize(sw['dens'], ROWS))
    assert same_bits(a['rewards'], got['rewards']) and not same_bits(a['rewards'], b['rewards'])
    assert same_bits(b['rewards'], rewards_of(one_shot(e, c, 'sinkhorn', final, dens=sw['dens'])[0], w))


# ---- 2. the updates --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,N,M', [('chamfer', 17, 12)] + [('sinkhorn',) + nm for nm in SINKHORN_PAIRS])
@pytest.mark.parametrize('update', ['softmax', 'elite'])
def test_the_update_is_the_cost_sessions(engines, kind, N, M, update):
    g, k = engines
    c = case(N, M)
    install(g, c, kind, 1.7)
    mpc_begin(g, c, 'mpc_begin_cloud', ns=8)
    mpc_begin(k, c, 'mpc_begin_cost', ns=8)
    for it in range(2):
        for e in (g, k):
            e.mpc_sample(it)
            e.mpc_rollout()
        a, b = g.mpc_get(actions=True, rewards=True, states=True), k.mpc_get(actions=True, states=True)
        assert same_bits(a['actions'], b['actions']) and same_bits(a['states'], b['states'])
        k.mpc_set_rewards(a['rewards'])
        for e in (g, k):
            e.mpc_update_elite_device(3) if update == 'elite' else e.mpc_update_device()
        assert same_bits(g.mpc_get(nominal=True)['nominal'], k.mpc_get(nominal=True)['nominal']), it
        # the asynchronous fetch reads the same slot
        g.mpc_fetch_async(it & 1)
        got = g.mpc_wait(it & 1)
        assert same_bits(got['rewards'], a['rewards']) and same_bits(got['actions'], a['actions'])
    assert not np.array_equal(g.mpc_get(nominal=True)['nominal'], syn.nominal_pushes(H, 0))
    # rewards handed in replace the cloud's
    mine = -np.arange(8 * NB, dtype=np.float32)
    g.mpc_set_rewards(mine)
    assert same_bits(g.mpc_get(rewards=True)['rewards'], mine)


# ---- 3. the GD pass --------------------------------------------------------------------------------------------------------------
def gd_seed(e, c, kind, w, pred):
    """the seed of the seeded pass: zero but seed[:, H-1] = w x the one-shot's fp32 gradient, scaled in float64 and rounded once"""
    values, grad = one_shot(e, c, kind, pred[:, H - 1], want_grad=True)
    seed = np.zeros_like(pred)
    seed[:, H - 1] = (np.float64(w) * grad.astype(np.float64)).astype(np.float32)
    return values, seed


@pytest.mark.parametrize('tape', ['fused', 'mfma'])
@pytest.mark.parametrize('kind,N,M,w', [('chamfer', 17, 12, 2.0), ('chamfer', 300, 40, 0.5), ('sinkhorn', 12, 20, 2.0),
                                        ('sinkhorn', 20, 12, 2.0), ('sinkhorn', 33, 33, 0.5)])
def test_the_gd_pass_is_the_seeded_pass(engines, tape, kind, N, M, w):
    g, k = engines
    c = case(N, M)
    for e in (g, k):
        e.set_engine(tape)
    try:
        install(g, c, kind, w)
        g.gd_begin_cloud(c['s_cur'], c['attr'], c['dens'], c['act_seqs'], 0.05, LO, HI)
        k.gd_begin_cost(c['s_cur'], c['attr'], c['dens'], c['act_seqs'], 0.05, LO, HI)
        pred = k.gd_predict()
        assert same_bits(g.gd_predict(), pred)
        values, seed = gd_seed(k, c, kind, w, pred)
        r, ga, gs = g.gd_grad(want_state_grad=True)
        assert same_bits(r, rewards_of(values, w))
        assert same_bits(gs[:, H - 1], seed[:, H - 1])          # the kernel's gradient is the one-shot's, scaled
        ga2, gs2 = k.gd_grad_seeded(seed, want_state_grad=True)
        assert np.abs(ga).max() > 0 and np.array_equal(ga, ga2) and np.array_equal(gs, gs2)
        # one forward per iteration: every forward step builds its neighbour lists once (the 'graph' class, on either tape) --
        # the launch census of a cloud iteration against the seam's predict + seeded pass
        g.probe_begin('graph')
        g.gd_grad()
        cloud_regions = g.probe_read()[1]
        g.probe_begin(None)
        k.probe_begin('graph')
        k.gd_predict()
        one_forward = k.probe_read()[1]
        k.probe_begin('graph')
        k.gd_predict()
        k.gd_grad_seeded(seed)
        seam_regions = k.probe_read()[1]
        k.probe_begin(None)
        print('[cloud-goal] %s %s %dx%d: neighbour-list launches per iteration %d (cloud) against %d (seam); one forward %d'
              % (kind, tape, N, M, cloud_regions, seam_regions, one_forward))
        assert one_forward == H and cloud_regions == one_forward and seam_regions == 2 * one_forward
        # five steps
        for it in range(5):
            _, seed = gd_seed(k, c, kind, w, k.gd_predict())
            pushes = k.gd_step_seeded(seed)
            r = g.gd_step()
            assert np.array_equal(g.gd_actions(), pushes), it
        assert not np.array_equal(pushes, c['act_seqs'])
        # the asynchronous form writes the same rewards and pushes
        g.gd_begin_cloud(c['s_cur'], c['attr'], c['dens'], c['act_seqs'], 0.05, LO, HI)
        g.gd_step_async(0)
        r_async, a_async = g.gd_wait(0)
        assert same_bits(r_async, rewards_of(values, w)) and same_bits(a_async, g.gd_actions())
    finally:
        for e in (g, k):
            e.set_engine('fused')


# ---- 5. the one-shot on crafted clouds ---------------------------------------------------------------------------------------
def tie_grids():
    """integer coordinates x 2^-4, and the same grid shifted by half a cell: every point of one has equidistant neighbours in the other"""
    ij = np.stack(np.meshgrid(np.arange(5), np.arange(4), indexing='ij'), -1).reshape(-1, 2)
    p = np.concatenate([ij, np.full((len(ij), 1), 12)], 1).astype(np.float32) / 16.0
    q = (p + np.array([1.0 / 32, 1.0 / 32, 0.0], np.float32)).astype(np.float32)
    return p, q


def test_eval_on_an_exact_tie_grid_has_cloud_chamfers_bits(engines):
    e = engines[0]
    p, q = tie_grids()
    P = np.stack([p, p[::-1].copy(), q])
    for w in (1.0, 2.0):
        e.set_goal_cloud(q, kind='chamfer', weight=w)
        got = e.cloud_goal_eval(P, want_grad=True)
        ref = e.cloud_chamfer(P, np.broadcast_to(q[None], P.shape).copy(), want_grad=True, want_nn=True)
        host = U.chamfer64(P, np.broadcast_to(q[None], P.shape), [len(p)] * 3, [len(q)] * 3)
        assert (host['margin_pq'][:2] == 0).any() and (host['margin_qp'][:2] == 0).any()      # exact ties, both directions
        np.testing.assert_array_equal(ref['nn_pq'], host['nn_pq'])          # the lowest index on every tie
        assert same_bits(got['rewards'], rewards_of(ref['fwd'] + ref['bwd'], w))
        assert same_bits(got['values'], np.float64(w) * (ref['fwd'] + ref['bwd']))
        assert same_bits(got['grad'], (np.float64(w) * ref['grad'].astype(np.float64)).astype(np.float32))
        # p == target: exactly zero, of either sign
        assert got['rewards'][2] == 0.0 and got['values'][2] == 0.0 and not got['grad'][2].any()


def test_eval_sinkhorn_of_the_target_itself_is_zero_to_the_divergence_bound(engines):
    e = engines[0]
    q = D.grid_cloud(40, 3)
    eps = D.GRID_SPACING ** 2
    e.set_goal_cloud(q, kind='sinkhorn', weight=1.0, eps_scale=eps, iters=50)
    got = e.cloud_goal_eval(q[None], dens=1.0, want_grad=True)
    one = e.cloud_divergence(q[None], q[None].copy(), eps=eps, iters=50, want_grad=True)
    assert same_bits(got['values'], one['divergence']) and same_bits(got['grad'], one['grad'])
    # the value is a difference of three sums of the size of the cross problem's: zero to the bound of tests/test_gpu_divergence.py
    # on that size (the bound there is relative to a value that does not cancel)
    ref = D.divergence64(q[None], q[None], [40], [40], np.array([eps]), 50)
    size = abs(float(ref['f'][0].mean() + ref['g'][0].mean())) / 3.0
    print('[cloud-goal] sinkhorn of the target itself: value %.3e, float64 reference %.3e, size of its sums %.3e'
          % (got['values'][0], ref['divergence'][0], size))
    assert abs(got['values'][0] - ref['divergence'][0]) <= DIV_VALUE_BOUND * size
    assert abs(got['values'][0]) <= DIV_VALUE_BOUND * size + abs(ref['divergence'][0])


@pytest.mark.parametrize('M', [12, 33])           # fewer and more target points than the clouds' 20, 13, 1 and 17 real rows
@pytest.mark.parametrize('kind', ['chamfer', 'sinkhorn'])
def test_eval_counts_padding_and_a_nan_row(engines, kind, M):
    e, c = engines[0], case(20, M)
    e.set_goal_cloud(c['target'], kind=kind, weight=2.0, eps_scale=1.0, iters=ITERS)
    rng = np.random.default_rng(3)
    P = (syn.make_pile(20, 4, seed=8)[0] + 0.01 * rng.standard_normal((4, 20, 3))).astype(np.float32)
    n_p = np.array([20, 13, 1, 17], np.int32)
    dens = np.array([125.0, 200.0, 125.0, 300.0], np.float32)
    got = e.cloud_goal_eval(P, n_p=n_p, dens=dens, want_grad=True)
    q = np.ascontiguousarray(np.broadcast_to(c['target'][None], (4, M, 3)))
    if kind == 'chamfer':
        ref = e.cloud_chamfer(P, q, n_p=n_p, want_grad=True)
        values = ref['fwd'] + ref['bwd']
    else:
        ref = e.cloud_divergence(P, q, n_p=n_p, eps=1.0 / dens.astype(np.float64), iters=ITERS, want_grad=True)
        values = ref['divergence']
    assert same_bits(got['rewards'], rewards_of(values, 2.0))
    assert same_bits(got['grad'], (2.0 * ref['grad'].astype(np.float64)).astype(np.float32))
    for b in range(4):
        pad = got['grad'][b, n_p[b]:]
        assert (pad == 0).all() and not np.signbit(pad).any()           # exactly +0.0
        assert np.abs(got['grad'][b, :n_p[b]]).max() > 0
    # rubbish in the padding changes nothing
    P2 = P.copy()
    P2[1, 13:] = 7.0
    again = e.cloud_goal_eval(P2, n_p=n_p, dens=dens, want_grad=True)
    assert all(same_bits(again[k], got[k]) for k in got)
    # one NaN coordinate: that row's reward is NaN, the call returns, the other rows keep their bits
    P3 = P.copy()
    P3[3, 5, 1] = np.nan
    bad = e.cloud_goal_eval(P3, n_p=n_p, dens=dens, want_grad=True)
    assert np.isnan(bad['rewards'][3]) and np.isnan(bad['values'][3])
    for k in got:
        assert same_bits(bad[k][:3], got[k][:3]), k
    # without the gradient the rewards are the same bits (the sampling planners' instantiation)
    assert same_bits(e.cloud_goal_eval(P, n_p=n_p, dens=dens)['rewards'], got['rewards'])


def test_eval_counts_under_the_loss_class_and_ends_no_session(engines):
    e, c = engines[0], case(17, 12)
    got = rolled(e, c, 'chamfer', 1.0)
    e.dispatch_reset()
    marks = e.last_dispatch()
    e.probe_begin('loss')
    e.cloud_goal_eval(got['states'][:, H - 1])
    ms, regions = e.probe_read()
    e.probe_begin(None)
    assert regions == 1 and ms > 0 and e.last_dispatch() == marks
    e.mpc_rollout()                                                     # the session is still there
    assert same_bits(e.mpc_get(rewards=True)['rewards'], got['rewards'])


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_carry_messages(golden):
    e = new_engine(golden.weights_seed0)
    try:
        c = case(17, 12)
        nominal = syn.nominal_pushes(H, 0).astype(np.float64)
        # no cloud goal: DRP_ESTATE
        with pytest.raises(DrpError, match=r'drp error -2: .*drp_set_goal_cloud'):
            mpc_begin(e, c, 'mpc_begin_cloud')
        with pytest.raises(DrpError, match=r'drp error -2: .*drp_set_goal_cloud'):
            e.gd_begin_cloud(c['s_cur'], c['attr'], c['dens'], c['act_seqs'], 0.05, LO, HI)
        with pytest.raises(DrpError, match=r'drp error -2: .*drp_set_goal_cloud'):
            e.cloud_goal_eval(c['s_cur'])
        # the goal's own arguments: DRP_EINVAL
        big = lambda n: np.zeros((n, 3), np.float32)
        for kw, word in ((dict(target=big(L.CLOUD_GOAL_MAX_POINTS['chamfer'] + 1), kind='chamfer'), 'M=4097'),
                         (dict(target=big(L.CLOUD_GOAL_MAX_POINTS['sinkhorn'] + 1), kind='sinkhorn'), 'M=1025'),
                         (dict(target=c['target'], kind='sinkhorn', iters=0), 'iters=0'),
                         (dict(target=c['target'], kind='sinkhorn', iters=L.TRANSPORT_MAX_ITERS + 1), 'iters='),
                         (dict(target=c['target'], kind='sinkhorn', eps_scale=0.0), 'eps_scale'),
                         (dict(target=c['target'], kind='chamfer', weight=0.0), 'weight'),
                         (dict(target=c['target'], kind='chamfer', weight=-1.0), 'weight'),
                         (dict(target=c['target'], kind='chamfer', weight=np.inf), 'weight')):
            with pytest.raises(DrpError, match=r'drp error -1: .*' + word):
                e.set_goal_cloud(**kw)
        for bad in (np.nan, np.inf):
            t = c['target'].copy()
            t[7, 2] = bad
            with pytest.raises(DrpError, match=r'drp error -1: .*q\[7\]\[2\] is not finite'):
                e.set_goal_cloud(t)
        assert e.lib.drp_set_goal_cloud(e.h, None, 3, None) == -1
        with pytest.raises(ValueError, match='unknown cloud goal kind'):
            e.set_goal_cloud(c['target'], kind='emd')
        assert e.cloud_goal is None                                    # nothing of the above installed anything
        with pytest.raises(DrpError, match='drp_set_goal_cloud'):
            e.cloud_goal_eval(c['s_cur'])
        # the multi-scene forms
        with pytest.raises(ValueError, match='per scene'):
            e.set_goal_cloud(np.zeros((2, 12, 3), np.float32))
        e.set_goal_cloud(c['target'], kind='sinkhorn', iters=ITERS)
        with pytest.raises(ValueError, match='multi-scene'):
            e.mpc_begin_cloud(c['s_cur'][None], c['attr'][None], c['dens'][None], nominal, NS, 0.6, 0.7, 10.0, LO, HI)
        with pytest.raises(ValueError, match='multi-scene'):
            e.gd_begin_cloud(c['s_cur'][None], c['attr'][None], c['dens'][None], c['act_seqs'], 0.05, LO, HI)
        # N over the kind's limit, at begin and in the one-shot; a density that gives no eps
        wide = syn.make_pile(L.CLOUD_GOAL_MAX_POINTS['sinkhorn'] + 1, NB, seed=1)
        with pytest.raises(DrpError, match=r'drp error -1: .*N=1025'):
            e.mpc_begin_cloud(wide[0], wide[2], wide[1], nominal, NS, 0.6, 0.7, 10.0, LO, HI)
        with pytest.raises(DrpError, match=r'drp error -1: .*N=1025'):
            e.gd_begin_cloud(wide[0], wide[2], wide[1], np.zeros((ROWS, H, 4), np.float32), 0.05, LO, HI)
        with pytest.raises(DrpError, match=r'drp error -1: .*N=1025'):
            e.cloud_goal_eval(wide[0], dens=wide[1])
        with pytest.raises(DrpError, match=r'drp error -1: .*dens'):
            e.cloud_goal_eval(c['s_cur'])
        with pytest.raises(DrpError, match=r'drp error -1: .*dens\[1\]'):
            e.cloud_goal_eval(c['s_cur'], dens=np.array([100.0, 0.0], np.float32))
        with pytest.raises(DrpError, match=r'drp error -1: .*n_p\[1\]=18'):
            e.cloud_goal_eval(c['s_cur'], n_p=[17, 18], dens=c['dens'])
        # reward_all_steps in a cloud session
        mpc_begin(e, c, 'mpc_begin_cloud')
        e.mpc_set_actions(c['act_seqs'])
        with pytest.raises(DrpError, match=r'drp error -1: .*reward_all_steps'):
            e.mpc_rollout(reward_all_steps=True)
        e.mpc_rollout()
        assert np.all(np.isfinite(e.mpc_get(rewards=True)['rewards']))
        # a new goal ends the cloud session it was begun on
        e.set_goal_cloud(c['target'], kind='chamfer')
        with pytest.raises(DrpError, match=r'drp error -2'):
            e.mpc_rollout()
    finally:
        e.close()


def test_an_image_goal_session_is_untouched_by_the_cloud(golden):
    """installing a cloud and running a cloud session changes no bit of drp_mpc_begin's and drp_gd_begin's rewards"""
    e = new_engine(golden.weights_seed0)
    try:
        c = case(17, 12)
        G = syn.goal_field(syn.goal_distance_image(syn.goal_mask('I')))
        e.set_goal(G, c['goal_coor'])

        def image_rewards():
            mpc_begin(e, c, 'mpc_begin')
            e.mpc_set_actions(c['act_seqs'])
            e.mpc_rollout()
            r = e.mpc_get(rewards=True)['rewards'].copy()
            e.gd_begin(c['s_cur'], c['attr'], c['dens'], c['act_seqs'], 0.05, LO, HI)
            return r, e.gd_grad()[0].copy()
        before = image_rewards()
        for kind in ('chamfer', 'sinkhorn'):
            got = rolled(e, c, kind, 1.7)
            e.gd_begin_cloud(c['s_cur'], c['attr'], c['dens'], c['act_seqs'], 0.05, LO, HI)
            assert np.all(np.isfinite(e.gd_grad()[0]))
            after = image_rewards()
            assert same_bits(after[0], before[0]) and same_bits(after[1], before[1])
            assert not same_bits(got['rewards'], before[0])
    finally:
        e.close()
