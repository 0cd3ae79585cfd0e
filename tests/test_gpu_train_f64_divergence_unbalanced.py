"""GPU: the training loop body with the UNBALANCED Sinkhorn divergence in float64 on the device
(drp_train_grad_f64_divergence_unbalanced: kd64_sweeps_unbalanced and kd64_combine_unbalanced of csrc/k_sinkhorn.h where
drp_train_grad_f64_divergence launches the balanced pair, everything behind the seed unchanged), the probe that holds the fp32
tapes against it, and the trainer's hook.

The batch is tests/_transport_ref.py's train_batch: B = 2, H = 2, N = 9 (counts 9 and 6), M = 12 with target counts 12,7 / 5,10;
K = 50 sweeps, eps = 1 / density, rho = TG.sinkhorn_reach(dens, 4) -- two DIFFERENT reaches -- and the masses of
TG.sinkhorn_mass_q for 'unit' and 'count' (12/9, 5/6, 7/9, 10/6: four different ones).  rho is [B], mass_q and transported are
[H][B] of the BATCH: the one-sample-cap test is the one that catches any of them indexed by the chunk.

Tolerances are the project's own.  The device against the float64 host reference (train_sinkhorn64_unbalanced of
tests/_divergence_unbalanced_f64_ref.py, pinned on the CPU by tests/test_divergence_unbalanced_f64_host.py): 1e-10 x the largest
magnitude of the compared tensor, the comparison of tests/test_gpu_train_f64.py; the certificates and transported within 1e-10
absolute.  The fp32 tapes against float64: GRAD_REL = 2e-4 of each tensor's largest gradient and LOSS_REL = 1e-4
(tests/_train_actions_ref.py), the bounds the balanced probe is held to.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import _divergence_f64_ref as R
import _divergence_unbalanced_f64_ref as RU
import _train_actions_ref as A
import _untracked_ref as U
import test_gpu_train_f64_divergence as TF
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG
from dyn_res_pile_manip_amd import weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine

pytestmark = pytest.mark.gpu
TOL = 1e-10
GRAD_REL = A.GRAD_REL
LOSS_REL = A.LOSS_REL
FP, IP, DP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
WSETS = ('seed0', 'trained')
IMPULSES = ('data', 'actions')
MASSES = RU.MASSES
new_engine = TF.new_engine


@pytest.fixture(scope='module')
def engines(golden):
    es = {'seed0': new_engine(golden.weights_seed0), 'trained': new_engine(golden.weights_trained)}
    yield es
    for e in es.values():
        e.close()


def call64(e, kw, **more):
    return e.train_grad_f64_divergence(kw['states'], kw['states_delta'], kw['attrs'], kw['particle_nums'], kw['particle_dens'],
                                       kw['targets'], kw['target_nums'], kw['eps'], kw['iters'], actions=kw.get('actions'),
                                       reach=kw['reach'], mass_q=kw['mass_q'], **more)


def step32_kw(kw):
    """the keyword arguments of Engine.train_step_divergence(reach=, mass_q=) for the same batch"""
    return dict(TF.step32_kw(kw), reach=kw['reach'], mass_q=kw['mass_q'])


def assert_close(got, want, nums, label):
    """got: train_grad_f64_divergence(reach=, ..., want_state=True, want_err=True); want: host_reference's"""
    loss, terms, grad, gs, col_err, self_err, moved = got
    rl, rt, rg, rgs, rce, rse, rmv = want
    figures = [('loss', abs(loss - rl) / abs(rl))]
    assert terms.dtype == np.float64 and terms.shape == rt.shape
    assert col_err.shape == rt.shape and self_err.shape == rt.shape + (2,) and moved.shape == rt.shape
    figures.append(('loss_terms', float(np.abs(terms - rt).max() / np.abs(rt).max())))
    assert grad.dtype == np.float64 and grad.shape == (38403,)
    off = 0
    for key, shape in weights.STATE_DICT_KEYS:
        n = int(np.prod(shape))
        a, b = grad[off:off + n], rg[off:off + n]
        figures.append((key, float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))))
        np.testing.assert_array_equal(a[b == 0], 0.0)       # identically zero inputs (the attribute columns): exactly zero
        off += n
    assert len(figures) == 2 + 18
    figures.append(('grad_state', float(np.abs(gs - rgs).max() / np.abs(rgs).max())))
    figures.append(('col_err', float(np.abs(col_err - rce).max())))           # absolute: of the total mass 1
    figures.append(('self_err', float(np.abs(self_err - rse).max())))
    figures.append(('transported', float(np.abs(moved - rmv).max())))
    for k, v in figures:
        print('[train-f64-unbalanced] %s %-45s %.3e' % (label, k, v))
    print('[train-f64-unbalanced] %s certificates: col_err up to %.3e, self_err up to %.3e; transported %s'
          % (label, col_err.max(), self_err.max(), np.round(moved.ravel(), 4)))
    for k, v in figures:
        assert v <= TOL, (label, k, v)
    np.testing.assert_array_equal(gs[rgs == 0], 0.0)
    for b, n in enumerate(nums):                            # padded rows of the state gradient: exactly +0.0
        assert (gs[b, :, n:] == 0).all() and not np.signbit(gs[b, :, n:]).any()
        assert (np.abs(gs[b, :, :n]).max(axis=-1) > 0).all()


# ---- 1. the reference's batch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mass', MASSES)
@pytest.mark.parametrize('impulses', IMPULSES)
@pytest.mark.parametrize('wset', WSETS)
def test_against_the_float64_reference(engines, golden, wset, impulses, mass):
    kw = RU.train_case(impulses, mass)
    assert kw['states'].shape == (2, 3, 9, 3) and kw['targets'].shape == (2, 2, 12, 3)
    assert kw['reach'][0] != kw['reach'][1] and kw['mass_q'].shape == (2, 2)
    e = engines[wset]
    got = call64(e, kw, want_state=True, want_err=True)
    assert_close(got, RU.reference(golden, wset, impulses, mass), kw['particle_nums'], '%s %s %s' % (wset, impulses, mass))
    short = call64(e, kw)                                    # the state gradient and the certificates are optional
    assert len(short) == 3 and short[0] == got[0]
    np.testing.assert_array_equal(short[1], got[1])
    np.testing.assert_array_equal(short[2], got[2])


# ---- 2. degenerate batches ------------------------------------------------------------------------------------------------------
def test_tiny_unpadded_batch(engines, golden):
    kw = RU.tiny_case()
    assert kw['states'].shape == (1, 2, 5, 3) and kw['targets'].shape == (1, 1, 3, 3) and kw['mass_q'][0, 0] == 3.0 / 5
    got = call64(engines['seed0'], kw, want_state=True, want_err=True)
    assert_close(got, RU.host_reference(golden.weights_seed0, kw), kw['particle_nums'], 'tiny')


def test_one_target_point_and_a_sample_of_one_particle(engines, golden):
    kw = RU.single_case()
    assert kw['particle_nums'][1] == 1 and kw['target_nums'][0, 0] == 1
    got = call64(engines['seed0'], kw, want_state=True, want_err=True)
    assert_close(got, RU.host_reference(golden.weights_seed0, kw), kw['particle_nums'], 'single')


# ---- 3. one value, one order ----------------------------------------------------------------------------------------------------
def test_same_bits_from_run_to_run_and_under_a_one_sample_cap(engines):
    """count masses and two reaches: under the cap every chunk is one sample, so rho, mass_q or transported indexed by the chunk's
    slot instead of the batch's would read (or write) sample 0's entries for sample 1"""
    e = engines['seed0']
    for impulses in IMPULSES:
        kw = RU.train_case(impulses, 'count')
        assert kw['reach'][0] != kw['reach'][1] and len(set(kw['mass_q'].ravel())) == 4
        whole, again = call64(e, kw, want_state=True, want_err=True), call64(e, kw, want_state=True, want_err=True)
        try:
            e.set_f64_cap(1)                                    # one sample is the smallest chunk: B chunks
            single = call64(e, kw, want_state=True, want_err=True)
        finally:
            e.set_f64_cap(0)
        assert len(whole) == 7
        for a, b, c in zip(whole, again, single):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
            np.testing.assert_array_equal(np.asarray(a), np.asarray(c))


def test_the_seed_is_the_one_shot_on_the_float64_prediction(engines, golden):
    kw = RU.train_case('data', 'count')
    e = engines['seed0']
    loss, terms, _, col_err, self_err, moved = call64(e, kw, want_err=True)
    B, H = 2, 2
    from _f64_grad_ref import _d, step, weights64
    from oracle.propnet_dense import adjacency
    W = weights64(golden.weights_seed0)
    st, sd, at, dens = _d(kw['states']), _d(kw['states_delta']), _d(kw['attrs']), _d(kw['particle_dens'])
    adj, _ = adjacency(st[:, 0].float(), sd[:, 0].float(), 0.08)
    p0 = step(W, at[:, 0], st[:, 0], sd[:, 0], dens, adj.double()).detach().numpy()
    one = e.cloud_divergence_f64(p0, kw['targets'][:, 0], kw['particle_nums'], kw['target_nums'][:, 0], eps=kw['eps'],
                                 iters=kw['iters'], reach=kw['reach'], mass_q=kw['mass_q'][0], want_col_err=True, want_self_err=True,
                                 want_transported=True)
    rel = float(np.abs(one['divergence'] / (H * B) - terms[0]).max() / np.abs(terms[0]).max())
    print('[train-f64-unbalanced] step 0: one-shot on the reference\'s prediction against the call\'s terms: %.3e; col_err apart '
          '%.3e, transported apart %.3e' % (rel, np.abs(one['col_err'] - col_err[0]).max(), np.abs(one['transported'] - moved[0]).max()))
    assert rel <= TOL
    assert np.abs(one['col_err'] - col_err[0]).max() <= TOL and np.abs(one['self_err'] - self_err[0]).max() <= TOL
    assert np.abs(one['transported'] - moved[0]).max() <= TOL


def test_an_infinite_reach_has_the_balanced_calls_bits(engines):
    e = engines['seed0']
    for impulses in IMPULSES:
        kw = R.train_case(impulses)
        want = TF.call64(e, kw, want_state=True, want_err=True)
        got = call64(e, dict(kw, reach=np.inf, mass_q=1.0), want_state=True, want_err=True)
        assert len(got) == len(want) + 1
        for a, b in zip(want, got):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
        assert np.abs(got[6] - 1.0).max() <= 4e-16


# ---- 4. the other yardsticks and the fp32 step are untouched ---------------------------------------------------------------------
def test_the_other_yardsticks_and_the_fp32_step_keep_their_bits(golden):
    kw = RU.train_case('data', 'count')
    kwa = RU.train_case('actions', 'count')
    st, sd, at, nums, dens, tg, tn = (kw[k] for k in ('states', 'states_delta', 'attrs', 'particle_nums', 'particle_dens', 'targets',
                                                      'target_nums'))

    def others(e):
        out = list(e.train_grad_f64(st, sd, at, nums, dens, want_state=True))
        out += list(e.train_grad_f64_actions(st, kwa['actions'], at, nums, dens, want_state=True))
        out += list(e.train_grad_f64_untracked(st, sd, at, nums, dens, tg, tn, want_state=True))
        out += list(TF.call64(e, kw, want_state=True, want_err=True))
        out += list(e.train_step_divergence(mode='grad', want_grad=True, want_err=True, **TF.step32_kw(kw)))
        out += list(e.train_step_divergence(mode='grad', want_grad=True, want_err=True, **step32_kw(kw)))
        return out
    fresh = new_engine(golden.weights_seed0)
    try:
        fresh.train_begin(2, 1e-3, 0.9)
        want = others(fresh)
    finally:
        fresh.close()
    e = new_engine(golden.weights_seed0)
    try:
        e.train_begin(2, 1e-3, 0.9)
        before = others(e)
        s, d, attr = syn.make_pile(20, 2, seed=1)
        imp = 0.004 * np.random.default_rng(1).standard_normal(s.shape).astype(np.float32)
        e.dispatch_reset()
        e.step(attr, s, imp, d)
        e.step_f64(attr, s, imp, d)
        marks, tap = e.last_dispatch(), e.f64_tap('effect_1')
        w0 = e.get_weights().copy()
        call64(e, kw, want_state=True, want_err=True)
        call64(e, kwa)
        assert e.last_dispatch() == marks
        np.testing.assert_array_equal(e.f64_tap('effect_1'), tap)      # taps of the earlier call are still answered
        np.testing.assert_array_equal(e.get_weights(), w0)
        after = others(e)
    finally:
        e.close()
    assert len(want) == len(before) == len(after) == 4 + 4 + 5 + 6 + 4 + 5
    for a, b, c in zip(want, before, after):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
        np.testing.assert_array_equal(np.asarray(a), np.asarray(c))


# ---- 5. the probe ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mass', MASSES)
@pytest.mark.parametrize('impulses', IMPULSES)
@pytest.mark.parametrize('wset', WSETS)
@pytest.mark.parametrize('tape', ['fused', 'mfma'])
def test_probe(golden, tape, wset, impulses, mass):
    """MEASURED on one MI355X, the worst tensor's rel against the bound GRAD_REL = 2e-4 (the float64 side's col_err at most
    1.3e-10, self_err 2.4e-16, transported_diff at most 3.0e-9), masses unit / count:
         fused  seed-0  data 9.7e-7 / 1.2e-6  pushes 1.1e-6 / 1.6e-6     trained  data 4.4e-7 / 5.9e-7  pushes 8.0e-7 / 5.7e-7
         mfma   seed-0  data 4.1e-7 / 4.1e-7  pushes 1.1e-6 / 1.0e-6     trained  data 3.5e-7 / 4.4e-7  pushes 2.5e-7 / 3.1e-7
    and the loss within 1.4e-7 relative (LOSS_REL = 1e-4)"""
    kw = RU.train_case(impulses, mass)
    k32 = step32_kw(kw)
    label = '%s %s %s %s' % (tape, wset, impulses, mass)
    plain = new_engine(U.weights_of(golden, wset), tape)
    try:
        plain.train_begin(2, 1e-3, 0.9)
        plain.train_step(kw['states'], R.train_case('data')['states_delta'], kw['attrs'], kw['particle_nums'], kw['particle_dens'],
                         mode='update')
        want = plain.get_weights().copy()
    finally:
        plain.close()
    e = new_engine(U.weights_of(golden, wset), tape)
    try:
        e.train_begin(2, 1e-3, 0.9)
        w0 = e.get_weights().copy()
        p = e.train_gradient_probe(kw['states'], kw['states_delta'], kw['attrs'], kw['particle_nums'], kw['particle_dens'],
                                   actions=kw.get('actions'), targets=kw['targets'], target_nums=kw['target_nums'], eps=kw['eps'],
                                   iters=kw['iters'], reach=kw['reach'], mass_q=kw['mass_q'])
        np.testing.assert_array_equal(e.get_weights(), w0)
        # the probe is what its two halves give
        loss32, g32, _, _, moved32 = e.train_step_divergence(mode='grad', want_grad=True, want_err=True, **k32)
        loss64, _, g64, col_err, self_err, moved64 = call64(e, kw, want_err=True)
        assert p['loss32'] == loss32 and p['loss64'] == loss64
        assert p['col_err'] == col_err.max() and p['self_err'] == self_err.max()
        assert p['transported'] == moved64.min() and p['transported_diff'] == np.abs(moved32 - moved64).max()
        off = 0
        for key, shape in weights.STATE_DICT_KEYS:
            n = int(np.prod(shape))
            assert p['tensors'][key]['max_abs_err'] == np.abs(g32[off:off + n].astype(np.float64) - g64[off:off + n]).max()
            assert p['tensors'][key]['max_abs_ref'] == np.abs(g64[off:off + n]).max()
            off += n
        # a train_step(mode='update') after the probe gives the bits it gives without the probe
        e.train_step(kw['states'], R.train_case('data')['states_delta'], kw['attrs'], kw['particle_nums'], kw['particle_dens'],
                     mode='update')
        np.testing.assert_array_equal(e.get_weights(), want)
    finally:
        e.close()
    assert sorted(p) == ['col_err', 'loss32', 'loss64', 'loss_diff', 'loss_kind', 'reach', 'rel', 'self_err', 'tape', 'tensors',
                         'transported', 'transported_diff', 'worst']
    assert p['tape'] == tape and p['loss_kind'] == 'sinkhorn' and p['reach'] is True and len(p['tensors']) == 18
    assert 0.0 < p['transported'] <= 1.0 and np.isfinite(p['transported_diff'])
    rel_loss = p['loss_diff'] / abs(p['loss64'])
    print('[sinkhorn-reach-probe] %s: worst %s rel %.3e, loss rel %.3e, col_err %.3e, self_err %.3e, transported %.4f, '
          'transported_diff %.3e' % (label, p['worst'], p['rel'], rel_loss, p['col_err'], p['self_err'], p['transported'],
                                     p['transported_diff']))
    for key, t in p['tensors'].items():
        print('[sinkhorn-reach-probe]     %-45s %.3e' % (key, t['rel']))
    for key, t in p['tensors'].items():
        assert t['max_abs_err'] <= GRAD_REL * t['max_abs_ref'], (label, key, t['rel'], p['col_err'], p['self_err'], p['transported_diff'])
    assert p['rel'] == max(t['rel'] for t in p['tensors'].values())
    assert rel_loss <= LOSS_REL, (label, rel_loss, p['col_err'], p['self_err'], p['transported_diff'])


def test_probe_refuses_a_reach_without_eps_or_beside_a_matching_loss(engines):
    kw = RU.train_case('data', 'unit')
    e = engines['seed0']
    e.train_begin(2, 1e-3, 0.9)
    args = [kw[k] for k in ('states', 'states_delta', 'attrs', 'particle_nums', 'particle_dens')]
    with pytest.raises(ValueError, match='reach='):
        e.train_gradient_probe(*args, targets=kw['targets'], target_nums=kw['target_nums'], reach=kw['reach'])
    with pytest.raises(ValueError, match='reach='):
        e.train_gradient_probe(*args, targets=kw['targets'], target_nums=kw['target_nums'], loss='match', reach=kw['reach'])
    with pytest.raises(ValueError, match='give reach'):
        e.train_gradient_probe(*args, targets=kw['targets'], target_nums=kw['target_nums'], eps=kw['eps'], iters=kw['iters'],
                               mass_q=kw['mass_q'])
    p = e.train_gradient_probe(*args, targets=kw['targets'], target_nums=kw['target_nums'], eps=kw['eps'], iters=kw['iters'])
    assert 'reach' not in p and 'transported' not in p          # without a reach: today's dict


# ---- 6. the trainer's hook -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('impulses', IMPULSES)
def test_the_trainers_hook_changes_no_weight(golden, impulses):
    config = syn.default_config()
    config['train'].update({'n_rollout': 2, 'n_history': 1, 'lr': 2e-4, 'adam_beta1': 0.9, 'log_per_iter': 1, 'n_epoch': 1})
    batches = TF.hook_batches(impulses)
    res, lines = {}, {}
    for every in (0, 2):
        model = TF._model(golden)
        lines[every] = []
        r = TG.train(config, model, {'train': batches, 'valid': batches[:1]}, log=lines[every].append, loss='sinkhorn',
                     impulses=impulses, sinkhorn_reach_scale=4, sinkhorn_mass='count', sinkhorn_reach_probe_every=every,
                     transport_iters=20)
        res[every] = (r, model.engine.get_weights().copy())
        model.engine.close()
    np.testing.assert_array_equal(res[0][1], res[2][1])
    probes = [h for h in res[2][0]['history'] if h[1] == 'grad_probe']
    probe_lines = [ln for ln in lines[2] if ln.startswith('grad_probe')]
    for ln in probe_lines:
        print('[sinkhorn-reach-probe] hook %s: %s' % (impulses, ln))
    assert len(probes) == 2 and all(np.isfinite(h[2]) and h[2] > 0 for h in probes)      # batches 0 and 2 of 4
    assert [h for h in res[2][0]['history'] if h[1] != 'grad_probe'] == res[0][0]['history']
    assert [ln for ln in lines[2] if not ln.startswith('grad_probe')] == lines[0]
    assert len(probe_lines) == 2 and all('col_err' in ln and 'transported_diff' in ln for ln in probe_lines)
    model = TF._model(golden)
    try:
        model.engine.train_begin(2, 2e-4, 0.9)
        pr = TG.probe_batch_sinkhorn(model, batches[0], impulses, transport_iters=20, sinkhorn_reach_scale=4, sinkhorn_mass='count')
        assert pr['loss_kind'] == 'sinkhorn' and pr['reach'] is True
        assert float(pr['rel']) == probes[0][2]                     # the hook's first probe: the same batch, seed-0 weights
    finally:
        model.engine.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(golden):
    kw = RU.train_case('data', 'count')
    st, sd, at, nums, dens, tg, tn, eps, rho, w = (np.ascontiguousarray(kw[k]) for k in (
        'states', 'states_delta', 'attrs', 'particle_nums', 'particle_dens', 'targets', 'target_nums', 'eps', 'reach', 'mass_q'))
    ac = np.ascontiguousarray(R.train_case('actions')['actions'])
    B, T1, N, _ = st.shape
    H, M = T1 - 1, tg.shape[2]

    def call(e, sd_=sd, ac_=None, tg_=tg, tn_=tn, M_=M, N_=N, nums_=nums, H_=H, eps_=eps, rho_=rho, w_=w, iters_=R.K):
        f = lambda a, T_: None if a is None else a.ctypes.data_as(T_)
        return e.lib.drp_train_grad_f64_divergence_unbalanced(e.h, f(st, FP), f(sd_, FP), f(ac_, FP), f(at, FP), f(nums_, IP), f(dens, FP),
                                                              B, N_, H_, f(tg_, FP), f(tn_, IP), M_, f(eps_, DP), f(rho_, DP), f(w_, DP),
                                                              iters_, None, None, None, None, None, None, None)
    e = Engine(0)
    try:
        assert call(e) == -2 and 'weights not loaded' in e.lib.drp_last_error(e.h).decode()        # DRP_ESTATE
        e.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
        good = call64(e, kw, want_state=True, want_err=True)                                       # no train_begin needed

        def still_works():
            for a, b in zip(call64(e, kw, want_state=True, want_err=True), good):
                np.testing.assert_array_equal(np.asarray(a), np.asarray(b))

        def rho_with(v):
            out = rho.copy()
            out[1] = v
            return out

        def w_with(v):
            out = w.copy()
            out[1, 0] = v                                            # (step 1, sample 0): the check walks all of [H][B]
            return out
        zero_t, big_t = tn.copy(), tn.copy()
        zero_t[1, 1], big_t[0, 0] = 0, M + 1
        bad_eps = eps.copy()
        bad_eps[1] = 0.0
        refused = [('null rho', dict(rho_=None), -1, 'null'), ('null mass_q', dict(w_=None), -1, 'null'),
                   ('rho = 0', dict(rho_=rho_with(0.0)), -1, 'rho[1]'), ('rho < 0', dict(rho_=rho_with(-1e-3)), -1, 'rho[1]'),
                   ('rho below eps / 1024', dict(rho_=rho_with(eps[1] / 1025)), -1, 'rho[1]'),
                   ('rho = nan', dict(rho_=rho_with(np.nan)), -1, 'rho[1]'), ('rho = -inf', dict(rho_=rho_with(-np.inf)), -1, 'rho[1]'),
                   ('mass_q below 1/8', dict(w_=w_with(0.1249)), -1, 'mass_q[1][0]'),
                   ('mass_q above 8', dict(w_=w_with(8.001)), -1, 'mass_q[1][0]'), ('mass_q = nan', dict(w_=w_with(np.nan)), -1, 'mass_q[1][0]'),
                   ('mass_q != 1 with rho = inf', dict(rho_=rho_with(np.inf)), -1, 'balanced'),
                   # ... and what the balanced call refuses
                   ('both impulse sources', dict(ac_=ac), -1, 'exactly one'), ('neither impulse source', dict(sd_=None), -1, 'exactly one'),
                   ('pushes without a camera', dict(sd_=None, ac_=ac), -2, ''),
                   ('null targets', dict(tg_=None), -1, ''), ('null target_nums', dict(tn_=None), -1, ''),
                   ('M = 0', dict(M_=0), -1, ''), ('M = 1025', dict(M_=1025), -1, ''), ('N = 1025', dict(N_=1025), -1, ''),
                   ('a target count of 0', dict(tn_=zero_t), -1, ''), ('a target count above M', dict(tn_=big_t), -1, ''),
                   ('a particle count of 0', dict(nums_=np.array([nums[0], 0], np.int32)), -1, ''),
                   ('n_rollout = 0', dict(H_=0), -1, ''), ('n_rollout = 65', dict(H_=65), -1, ''),
                   ('null eps', dict(eps_=None), -1, ''), ('eps = 0', dict(eps_=bad_eps), -1, 'eps'),
                   ('iters = 0', dict(iters_=0), -1, 'iters'), ('iters = 1001', dict(iters_=1001), -1, 'iters')]
        for label, k, rc, word in refused:
            got = call(e, **k)
            msg = e.lib.drp_last_error(e.h).decode()
            print('[train-f64-unbalanced] refusal, %s: %d (%s)' % (label, got, msg))
            assert got == rc and word in msg, label
            still_works()
        e.set_camera(*A.camera_args())
        assert call(e, sd_=None, ac_=ac) == 0
        assert call(e, rho_=rho_with(np.inf), w_=np.ones((H, B))) == 0         # the edges are served
        assert call(e, w_=w_with(8.0)) == 0 and call(e, w_=w_with(0.125)) == 0
        with pytest.raises(DrpError, match='mass_q'):
            call64(e, dict(kw, mass_q=9.0))
        with pytest.raises(DrpError, match='rho'):
            call64(e, dict(kw, reach=-1.0))
        still_works()
    finally:
        e.close()
