"""GPU: the float64 evaluation of one step on the device (Engine.step_f64 / forward_f64 / f64_tap: csrc/k_prop_f64.h) against
its numpy restatement (tests/_f64_ref.py), and the accuracy probe that holds the four engines against it.

TOL: 1e-10 x max|tap|.  Derived, not measured: a K <= 193 dot product in double is within 193 x 2^-53 = 2.1e-14 of
sum |a b|; fourteen dependent layers keep the total below 1e-12 of the largest activation; 1e-10 leaves 100 x for numpy's
own summation order and is four orders below what any fp32 engine reaches."""
import warnings

import numpy as np
import pytest

from dyn_res_pile_manip_amd import synthetic as syn, weights, _lib
from dyn_res_pile_manip_amd._lib import DrpError, DrpRangeError
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel, mask_lists
from oracle import propnet_sparse as osp

import _f64_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-10
ENGINES = ['valu', 'mfma', 'split', 'fused']
TRAINED_SIZES = ['n20', 'n50', 'n100', 'n300']


def new_engine(blob, **kw):
    e = Engine(0, **kw)
    if blob is not None:
        e.load_weights(blob, 0.08)
    e.set_camera(osp.world2cam_affine(syn.demo_cam_extrinsics(), 24), 24.0, syn.demo_cam_params())
    return e


@pytest.fixture(scope='module')
def blob0(golden):
    return weights.blob_from_state_dict(golden.weights_seed0)


@pytest.fixture(scope='module')
def W0(golden):
    return R.weights64(golden.weights_seed0)


@pytest.fixture(scope='module')
def eng(blob0):
    e = new_engine(blob0)
    yield e
    e.close()


def case_inputs(g, case):
    return [g[case + '/' + k] for k in ('attr', 's_cur', 's_delta', 'dens')]


def pushed(eng, N, B, seed, clump=False):
    """B piles of N particles, each under a push of its own -> (a, s, sd, dens); clump: sample 0's particles drawn together
    until every one of them has all the entries a list can hold"""
    s, dens, attr = syn.make_pile(N, B, seed=seed)
    if clump:
        s[0, :, :2] = s[0, :1, :2] + 1e-3 * (s[0, :, :2] - s[0, :1, :2])
    return attr, s, eng.gen_s_delta(s, syn.sample_pushes(B, 1, seed=seed)[:, 0]), dens


def check_against_ref(eng, W, inp, idx, cnt, out, label):
    """the device's s_pred and every tap of its last call against _f64_ref on the same lists, each within TOL x max|tap|"""
    taps = {}
    ref = R.forward64(W, *inp, idx, cnt, taps)
    taps['s_pred'] = ref
    worst = 0.0
    for name in R.TAPS + ['s_pred']:
        got = out if name == 's_pred' else eng.f64_tap(name)
        assert got.dtype == np.float64 and got.shape == taps[name].shape, name
        scale = max(np.abs(taps[name]).max(), 1e-300)
        err = np.abs(got - taps[name]).max() / scale
        worst = max(worst, err)
        assert err <= TOL, (label, name, err)
    print('[f64] %s: worst tap error %.2e of the tap\'s largest value' % (label, worst))


# ---- correctness of the evaluation ------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['n8', 'n64', 'n50'])
def test_step_and_forward_against_the_float64_reference(eng, golden, W0, case):
    g = golden.one_step
    inp = case_inputs(g, case)
    idx, cnt = eng.build_graph(inp[1], inp[2])
    np.testing.assert_array_equal(idx, g[case + '/nbr_idx'])
    out = eng.step_f64(*inp)
    check_against_ref(eng, W0, inp, idx, cnt, out, case + ' step_f64')
    assert np.abs(out - g[case + '/s_pred']).max() < 2e-6            # and the reference's own fp32 output
    out2 = eng.forward_f64(*inp, idx, cnt)
    check_against_ref(eng, W0, inp, idx, cnt, out2, case + ' forward_f64')
    np.testing.assert_array_equal(out, out2)
    # the taps' other names
    np.testing.assert_array_equal(eng.f64_tap('c_node'), eng.f64_tap('particle_encode'))
    np.testing.assert_array_equal(eng.f64_tap('c_edge'), eng.f64_tap('relation_encode'))
    np.testing.assert_array_equal(eng.f64_tap('particle_effect_2'), eng.f64_tap('effect_2'))


@pytest.mark.parametrize('N', [1, 5, 17, 33])
def test_shapes_that_exercise_the_tiling(eng, W0, N):
    """B = 3 at sizes below, one past and two past a 16-row tile, lists from the device's graph build (max_rel = min(10, N));
    then explicit lists with what the graph build never yields, a particle's own entry being always there: a particle
    with no entry, a sample without any edge, beside a clump whose particles all have ten"""
    inp = pushed(eng, N, 3, seed=N, clump=True)
    idx, cnt = eng.build_graph(inp[1], inp[2])
    assert cnt.max() == min(10, N) and cnt.min() >= 1
    out = eng.step_f64(*inp)
    check_against_ref(eng, W0, inp, idx, cnt, out, 'N=%d step_f64' % N)
    idx2, cnt2 = idx.copy(), cnt.copy()
    cnt2[2] = 0                                         # a sample with no edges at all
    cnt2[1, N // 2] = 0                                 # a particle with no entry
    idx2[np.arange(10)[None, None, :] >= cnt2[:, :, None]] = -1
    out2 = eng.forward_f64(*inp, idx2, cnt2)
    check_against_ref(eng, W0, inp, idx2, cnt2, out2, 'N=%d forward_f64, edited lists' % N)
    assert np.all(eng.f64_tap('agg_2')[2] == 0)


def test_batch_independence_chunking_and_repeatability(eng, W0):
    inp = pushed(eng, 50, 5, seed=3)
    eng.set_f64_cap(0)
    full = eng.step_f64(*inp)
    tap = eng.f64_tap('effect_1')
    np.testing.assert_array_equal(eng.step_f64(*inp), full)                          # two runs
    alone = eng.step_f64(*[v[2:3] for v in inp])
    np.testing.assert_array_equal(alone[0], full[2])                                 # sample 2 alone
    np.testing.assert_array_equal(eng.f64_tap('effect_1')[0], tap[2])
    per_sample = 50 * (7 * 64 + 3 + 10 * 4 * 64) * 8
    try:
        eng.set_f64_cap(2 * per_sample + 100)                                        # two samples per chunk: 3 chunks
        np.testing.assert_array_equal(eng.step_f64(*inp), full)
        with pytest.raises(DrpError, match='3 chunks'):
            eng.f64_tap('effect_1')
        eng.set_f64_cap(1)                                                           # below one sample: one sample per chunk
        np.testing.assert_array_equal(eng.step_f64(*inp), full)
        with pytest.raises(DrpError, match='5 chunks'):
            eng.f64_tap('effect_1')
    finally:
        eng.set_f64_cap(0)
    np.testing.assert_array_equal(eng.step_f64(*inp), full)
    np.testing.assert_array_equal(eng.f64_tap('effect_1'), tap)


def test_forward_on_masked_lists(eng, W0):
    """model/gnn_dyn.py:238-241 through gnn_dyn.mask_lists: the float64 forward on the masked lists"""
    inp = pushed(eng, 33, 3, seed=5)
    idx, cnt = eng.build_graph(inp[1], inp[2])
    midx, mcnt = mask_lists(idx, [33, 20, 7])
    assert mcnt[1, 20:].max() == 0 and mcnt.sum() < cnt.sum()
    out = eng.forward_f64(*inp, midx, mcnt)
    check_against_ref(eng, W0, inp, midx, mcnt, out, 'masked lists')


# ---- isolation -------------------------------------------------------------------------------------------------
def disturb(e, inp):
    e.step_f64(*inp)
    for name in ('fused', 'valu'):
        e.accuracy_probe(*inp, engine=_lib.ENGINES[name])


def run_sessions(blob, inp, disturbed):
    """three GD steps and two MPPI iterations, with float64 calls and probes in between or without"""
    e = new_engine(blob)
    out = []
    try:
        e.set_goal_image(syn.goal_distance_image(syn.goal_mask('I')), 200, 0, 'exact')
        s0, dens, attr = syn.make_pile(40, 1, seed=0)
        lo, hi = syn.action_limits()
        e.gd_begin(s0, attr, dens, syn.sample_pushes(4, 2, seed=0), 0.05, lo, hi)
        for _ in range(3):
            out.append(e.gd_step())
            if disturbed:
                disturb(e, inp)
        out.append(e.gd_actions())
        e.mpc_begin(s0, attr, dens, syn.nominal_pushes(2, seed=0), n_sample=8, sigma=0.6, beta_filter=0.7, reward_weight=0.1,
                    act_lo=lo, act_hi=hi, seed=1)
        for it in range(2):
            e.mpc_sample(it)
            if disturbed:
                disturb(e, inp)
            e.mpc_rollout()
            if disturbed:
                disturb(e, inp)
            out.append(e.mpc_update(e.mpc_partials()))
        out.append(e.mpc_get(rewards=True, states=True)['rewards'])
        assert e.engine_id == _lib.ENGINE_FUSED
    finally:
        e.close()
    return out


def test_sessions_go_on_undisturbed(eng, blob0, golden):
    inp = case_inputs(golden.one_step, 'n50')
    plain = run_sessions(blob0, inp, False)
    mixed = run_sessions(blob0, inp, True)
    assert len(plain) == len(mixed)
    for a, b in zip(plain, mixed):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


def test_training_is_undisturbed_and_its_update_reaches_the_float64_weights(blob0, golden):
    g = golden.train
    batch = [g['b4_r3/' + k] for k in ('states', 'states_delta', 'attrs', 'particle_nums', 'particle_dens')]
    inp = case_inputs(golden.one_step, 'n64')
    e = new_engine(blob0)
    try:
        e.train_begin(batch[0].shape[1] - 1, 1e-3, 0.9)
        before = e.train_step(*batch, mode='eval')[0]
        out0 = e.step_f64(*inp)
        disturb(e, inp)
        assert e.train_step(*batch, mode='eval')[0] == before
        e.train_step(*batch, mode='update')
        blob = e.get_weights()
        assert np.abs(blob - blob0).max() > 0
        out1 = e.step_f64(*inp)
        assert np.abs(out1 - out0).max() > 0
        idx, cnt = e.build_graph(inp[1], inp[2])
        check_against_ref(e, R.weights64(weights.state_dict_from_blob(blob)), inp, idx, cnt, out1, 'after an optimiser step')
        e.load_weights(blob0, 0.08)                                                 # and a load refreshes them
        np.testing.assert_array_equal(e.step_f64(*inp), out0)
    finally:
        e.close()


def test_refusals_leave_the_context_usable(blob0, golden):
    inp = case_inputs(golden.one_step, 'n8')
    e = new_engine(None)
    try:
        with pytest.raises(DrpError, match='weights not loaded'):
            e.step_f64(*inp)
        with pytest.raises(DrpError, match='weights not loaded'):
            e.accuracy_probe(*inp)
        e.load_weights(blob0, 0.08)
        idx, cnt = e.build_graph(inp[1], inp[2])
        good = e.forward_f64(*inp, idx, cnt)
        bad = idx.copy()
        bad[1, 3, 0] = 8                                                            # N = 8: entries are 0..7
        with pytest.raises(DrpError, match='outside 0..7'):
            e.forward_f64(*inp, bad, cnt)
        big = np.zeros((1, 5000, 3), np.float32)
        with pytest.raises(DrpError, match='N <= 4096'):
            e.step_f64(np.zeros((1, 5000), np.float32), big, big, np.ones(1, np.float32))
        with pytest.raises(DrpError, match='engine 17'):
            e.accuracy_probe(*inp, engine=17)
        np.testing.assert_array_equal(e.forward_f64(*inp, idx, cnt), good)
        np.testing.assert_array_equal(e.step_f64(*inp), good)
    finally:
        e.close()


# ---- the probe ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('engine', ENGINES)
def test_probe_is_what_numpy_computes(eng, golden, engine):
    inp = case_inputs(golden.one_step, 'n64')
    selected = _lib.ENGINES['split' if engine != 'split' else 'mfma']
    eng.set_engine(selected)
    mine = eng.step(*inp)
    p = eng.accuracy_probe(*inp, engine=_lib.ENGINES[engine])
    assert eng.engine_id == selected
    np.testing.assert_array_equal(eng.step(*inp), mine)            # the library still runs the selected engine
    eng.set_engine(_lib.ENGINES[engine])
    s32 = eng.step(*inp)
    eng.set_engine(_lib.ENGINE_FUSED)
    s64 = eng.step_f64(*inp)
    err = np.abs(s32.astype(np.float64) - s64)
    disp = np.abs(s64 - inp[1].astype(np.float64)).max()
    print('[probe] seed-0 n64 %s: abs %.3e disp %.3e disp_rel %.3e worst %d' % (engine, p['abs'], p['disp'], p['disp_rel'], p['worst']))
    assert p['abs'] == err.max() and p['disp'] == disp
    assert p['worst'] == int(np.argmax(err.reshape(-1, 3).max(1)))            # argmax: the lowest index among ties
    q = err.max() / max(disp, 1e-12)
    assert abs(p['disp_rel'] - q) <= np.spacing(q)


def test_probe_ties_go_to_the_lowest_particle(eng, golden):
    """a batch of one sample four times over: four particles share the largest error, the first of them is reported"""
    inp = [np.concatenate([v[:1]] * 4) for v in case_inputs(golden.one_step, 'n64')]
    p = eng.accuracy_probe(*inp, engine=_lib.ENGINE_MFMA)
    assert 0 <= p['worst'] < 64 and p['abs'] > 0


@pytest.mark.parametrize('which', ['seed0', 'trained'])
def test_every_engine_is_inside_the_parity_tolerance(golden, which):
    """the project's 1e-4-of-displacement tolerance, measured against float64 for the first time"""
    if which == 'seed0':
        blob, cases = weights.blob_from_state_dict(golden.weights_seed0), [(golden.one_step, c + '/') for c in ('n8', 'n64')]
    else:
        blob, cases = weights.blob_from_state_dict(golden.weights_trained), [(golden.trained, 'one_step/%s/' % c) for c in TRAINED_SIZES]
    e = new_engine(blob)
    try:
        for g, p in cases:
            inp = [g[p + k] for k in ('attr', 's_cur', 's_delta', 'dens')]
            for name in ENGINES:
                r = e.accuracy_probe(*inp, engine=_lib.ENGINES[name])
                print('[probe] %s %s %s: abs %.3e disp %.3e disp_rel %.3e' % (which, p, name, r['abs'], r['disp'], r['disp_rel']))
                assert r['disp_rel'] < 1e-4, (which, p, name, r)
    finally:
        e.close()


def test_the_guard(blob0, golden):
    inp = case_inputs(golden.one_step, 'n64')
    e = new_engine(blob0)
    ref = new_engine(blob0)
    try:
        assert 'probe' not in e.range_info()
        plain = e.step(*inp)
        np.testing.assert_array_equal(plain, ref.step(*inp))
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            e.load_weights(blob0, 0.08, probe=True, max_disp_rel=0.0)
        assert [x.category for x in w] == [RuntimeWarning] and 'float64' in str(w[0].message)
        assert e.engine_id == _lib.ENGINE_MFMA
        pr = e.range_info()['probe']
        assert pr['engine'] == 'fused' and pr['disp_rel'] > 0 and set(pr) == {'abs', 'disp', 'disp_rel', 'worst', 'engine'}
        assert pr['disp_rel'] == e.accuracy_probe(*e.probe_batch(), engine=_lib.ENGINE_FUSED)['disp_rel']
        ref.set_engine(_lib.ENGINE_MFMA)
        np.testing.assert_array_equal(e.step(*inp), ref.step(*inp))                 # it does run the fp32 matrix engine now
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            e.load_weights(blob0, 0.08)                                             # no threshold: the choice comes back
            assert e.engine_id == _lib.ENGINE_FUSED and 'probe' not in e.range_info()
            np.testing.assert_array_equal(e.step(*inp), plain)
            e.load_weights(blob0, 0.08, probe=True, max_disp_rel=1.0)
            assert e.engine_id == _lib.ENGINE_FUSED and e.range_info()['probe']['engine'] == 'fused'
            e.load_weights(blob0, 0.08, probe=tuple(inp))                           # a batch of the caller's, nothing asked of it
            assert e.range_info()['probe']['disp_rel'] == e.accuracy_probe(*inp)['disp_rel']
        assert not w
        e.set_engine(_lib.ENGINE_MFMA)
        with pytest.raises(DrpError, match='nowhere to fall back'):
            e.load_weights(blob0, 0.08, probe=True, max_disp_rel=0.0)
        assert e.engine_id == _lib.ENGINE_MFMA
        # probe=None: the parent's call sequence, bit for bit
        e.set_engine(_lib.ENGINE_FUSED)
        e.load_weights(blob0, 0.08)
        assert 'probe' not in e.range_info() and sorted(e.range_info()) == ['bound', 'ok', 'shift', 'wmax']
        np.testing.assert_array_equal(e.step(*inp), plain)
        no_cam = Engine(0)
        try:
            with pytest.raises(DrpError, match='camera not set'):
                no_cam.load_weights(blob0, 0.08, probe=True)
        finally:
            no_cam.close()
    finally:
        e.close()
        ref.close()


def test_weights_the_range_check_refuses(blob0, golden):
    """a relation-encoder entry beyond fp16 (as tests/test_gpu_errors.py spoils one): under probe=True the refusal is what
    DRP_ERANGE is everywhere else -- an error without auto_engine, the fp32 fallback with it -- not an accuracy finding"""
    blob = blob0.copy()
    off = 0
    for k, shape in weights.STATE_DICT_KEYS:
        if k == 'model.relation_encoder.model.2.weight':
            break
        off += int(np.prod(shape))
    blob[off + 17] = 7e4
    e = new_engine(None)
    try:
        with pytest.raises(DrpRangeError, match='outside the range'):
            e.load_weights(blob, 0.08, probe=True, max_disp_rel=1e-4)
        assert e.engine_id == _lib.ENGINE_FUSED and not e.range_info()['ok'] and 'probe' not in e.range_info()
    finally:
        e.close()
    e = new_engine(None, auto_engine=True)
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            e.load_weights(blob, 0.08, probe=True, max_disp_rel=1.0)
        assert [x.category for x in w] == [RuntimeWarning] and 'refused' in str(w[0].message)
        assert e.engine_id == _lib.ENGINE_MFMA and e.range_info()['probe']['engine'] == 'mfma'
        e.load_weights(blob0, 0.08)
        assert e.engine_id == _lib.ENGINE_FUSED
    finally:
        e.close()


def test_the_model_mirror(eng, golden):
    import torch
    inp = case_inputs(golden.one_step, 'n8')
    eng.set_engine(_lib.ENGINE_FUSED)
    model = PropNetDiffDenModel(syn.default_config(), engine=eng)
    model.load_state_dict({k[2:]: torch.from_numpy(golden.weights_seed0[k]) for k in golden.weights_seed0.files
                           if k.startswith('w/')}, strict=False)
    want = eng.step_f64(*inp)
    got = model.predict_one_step(*inp, dtype=np.float64)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    np.testing.assert_array_equal(got, want)
    t = model.predict_one_step(*[torch.from_numpy(v) for v in inp], dtype=torch.float64)
    assert t.dtype == torch.float64 and t.device == torch.device('cpu')
    np.testing.assert_array_equal(t.numpy(), want)
    assert model.predict_one_step(*inp).dtype == np.float32
    nums = [8, 5]
    idx, cnt = mask_lists(eng.build_graph(inp[1], inp[2])[0], nums)
    np.testing.assert_array_equal(model.predict_one_step(*inp, particle_nums=nums, dtype='float64'), eng.forward_f64(*inp, idx, cnt))
    model.load_state_dict(model.state_dict(), probe=True, max_disp_rel=1.0)
    assert eng.range_info()['probe']['engine'] == 'fused'
    model.load_state_dict(model.state_dict())
    assert 'probe' not in eng.range_info()
