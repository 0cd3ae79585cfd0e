"""GPU, row u2: the training loop body with a matching loss in float64 on the device (drp_train_grad_f64_match: ka64_match of
csrc/k_match_f64.h where drp_train_grad_f64 launches kt64_mse, alone or behind kc64_chamfer<true> for the mix; everything behind
the seed unchanged), the probe that holds the fp32 tapes against it ON THE SAME PAIRS, and the trainer's hook.

The batches: the fixtures b4_r3 and b2_r5 against _match_ref.dense_targets (every predicted row matched; seeded per case in
tests/_match_f64_ref.py) and against their own untracked targets (predicted rows left over), U.tiny_batch(), U.single_point_batch;
both kinds; both impulse sources; the seed-0 and the trained weights.

Tolerances are the project's own.  The device against train_match64 of tests/_match_ref.py: TOL = 1e-10 x the largest magnitude
of the compared tensor, the comparison of tests/test_gpu_train_f64_divergence.py -- both sides solve the assignment in double on
the double prediction (tests/test_match_f64_host.py holds every case's uniqueness margin above 1e-7), or take the same given
pairs.  The fp32 tapes against float64 on the fp32 side's own pairs: GRAD_REL = 2e-4 of each tensor's largest gradient and
LOSS_REL = 1e-4 (tests/_train_actions_ref.py).  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import _match_f64_ref as F
import _match_ref as R
import _train_actions_ref as A
import _untracked_ref as U
from dyn_res_pile_manip_amd import synthetic as syn
from dyn_res_pile_manip_amd import train_gnn_dyn as TG
from dyn_res_pile_manip_amd import weights
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.gnn_dyn import PropNetDiffDenModel

pytestmark = pytest.mark.gpu
TOL = 1e-10
GRAD_REL = A.GRAD_REL
LOSS_REL = A.LOSS_REL
WSETS = ('seed0', 'trained')
IMPULSES = ('data', 'actions')
W = 0.25                                # the mix's weight where a test does not vary it


def new_engine(w, engine=None):
    e = Engine(0)
    e.load_weights(weights.blob_from_state_dict(w), 0.08)
    e.set_camera(*A.camera_args())
    if engine is not None:
        e.set_engine(engine)
    return e


@pytest.fixture(scope='module')
def engines(golden):
    es = {'seed0': new_engine(golden.weights_seed0), 'trained': new_engine(golden.weights_trained)}
    yield es
    for e in es.values():
        e.close()


def call64(e, kw, kind='match', weight=W, **more):
    return e.train_grad_f64_match(kw['states'], kw.get('states_delta'), kw['attrs'], kw['particle_nums'], kw['particle_dens'],
                                  kw['targets'], kw['target_nums'], kind, weight, actions=kw.get('actions'), **more)


def flat(got):
    """a call's results as a list of arrays (the info dict spread out)"""
    out = []
    for v in got:
        out += [v[k] for k in sorted(v) if v[k] is not None] if isinstance(v, dict) else [np.asarray(v)]
    return out


def assert_close(got, want, kw, kind, label):
    """got: train_grad_f64_match(..., want_state=True, want_info=True); want: train_match64's"""
    loss, terms, grad, gs, info = got
    rl, rt, rgrads, rgs, rinfo = want
    rg = R.blob64(rgrads)
    nums = kw['particle_nums']
    figures = [('loss', abs(loss - rl) / abs(rl))]
    assert terms.dtype == np.float64 and terms.shape == rt.shape
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
    figures.append(('cost', float(np.abs(info['cost'] - rinfo['cost']).max() / rinfo['cost'].max())))
    figures.append(('opt_cost', float(np.abs(info['opt_cost'] - rinfo['opt_cost']).max() / rinfo['opt_cost'].max())))
    for k, v in figures:
        print('[train-f64-match] %s %-45s %.3e' % (label, k, v))
    for k, v in figures:
        assert v <= TOL, (label, k, v)
    assert info['cost'].shape == rt.shape and info['match'].shape == rt.shape + (kw['states'].shape[2],)
    assert (info['cost'] >= info['opt_cost']).all()
    if kind == 'match':
        assert info['chamfer_margin'] is None
        np.testing.assert_array_equal(gs[rgs == 0], 0.0)    # unmatched rows and padding: exactly zero
    else:
        assert abs(info['chamfer_margin'].min() - rinfo['chamfer_margin']) <= TOL * rinfo['chamfer_margin']
    for b, n in enumerate(nums):                            # padded rows of the state gradient: exactly +0.0
        assert (gs[b, :, n:] == 0).all() and not np.signbit(gs[b, :, n:]).any()
    return info


def own_optimum(info, rinfo, kw):
    """the float64 side's own partners are the reference's optimum, -1 on padding"""
    H, B, N = info['match'].shape
    for t in range(H):
        for b in range(B):
            n = int(kw['particle_nums'][b])
            np.testing.assert_array_equal(info['match'][t, b, :n], rinfo['match'][t, b, :n])
            assert (info['match'][t, b, n:] == -1).all()


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', R.LOSSES)
@pytest.mark.parametrize('impulses', IMPULSES)
@pytest.mark.parametrize('name,wset', U.TRAIN_CASES)
def test_against_the_float64_reference(engines, golden, name, wset, impulses, kind):
    e = engines[wset]
    kw = F.train_kw(golden, name, impulses, 'dense', wset)
    label = '%s %s %s %s' % (name, wset, impulses, kind)
    # the matching solved on its own prediction
    want = F.train_reference(golden, name, wset, impulses, 'dense', kind, W)
    got = call64(e, kw, kind, want_state=True, want_info=True)
    info = assert_close(got, want, kw, kind, label + ' own')
    own_optimum(info, want[4], kw)
    np.testing.assert_array_equal(info['cost'], info['opt_cost'])
    short = call64(e, kw, kind)                              # the state gradient and the info are optional
    assert len(short) == 3 and short[0] == got[0]
    np.testing.assert_array_equal(short[2], got[2])
    # a matching given by the caller: valid, not the optimum (dense targets: rows 0 and 1 are matched in every problem)
    given = info['match'].copy()
    given[:, :, [0, 1]] = given[:, :, [1, 0]]
    want2 = F.reference(kw, U.weights_of(golden, wset), given, kind, W)
    got2 = call64(e, kw, kind, match_in=given, want_state=True, want_info=True)
    info2 = assert_close(got2, want2, kw, kind, label + ' given')
    np.testing.assert_array_equal(info2['match'], info['match'])       # the solver's own optimum all the same
    np.testing.assert_array_equal(info2['opt_cost'], info['opt_cost'])
    assert (info2['cost'] > info2['opt_cost']).all() and got2[0] > got[0]
    fed = call64(e, kw, kind, match_in=info['match'], want_state=True, want_info=True)      # the optimum fed back: the same bits
    for a, b in zip(flat(got), flat(fed)):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('kind', R.LOSSES)
@pytest.mark.parametrize('impulses', IMPULSES)
@pytest.mark.parametrize('name', F.TRAIN_BATCHES)
def test_more_predicted_rows_than_target_rows(engines, golden, name, impulses, kind):
    """the other orientation: the rows of the solver are the target's, predicted rows are left without a partner and a gradient"""
    kw = F.train_kw(golden, name, impulses, 'sparse')
    want = F.train_reference(golden, name, 'seed0', impulses, 'sparse', kind, W)
    got = call64(engines['seed0'], kw, kind, want_state=True, want_info=True)
    info = assert_close(got, want, kw, kind, '%s %s %s sparse' % (name, impulses, kind))
    own_optimum(info, want[4], kw)
    assert ((info['match'] >= 0).sum(axis=2) == np.minimum(np.asarray(kw['particle_nums'])[None, :], kw['target_nums'].T)).all()


@pytest.mark.parametrize('kind', R.LOSSES)
def test_tiny_and_single_point_batches(engines, golden, kind):
    for label, batch in (('tiny', U.tiny_batch()), ('single point', U.single_point_batch(golden))):
        kw = F.batch_kw(batch)
        want = F.reference(kw, golden.weights_seed0, None, kind, 0.5)
        got = call64(engines['seed0'], kw, kind, 0.5, want_state=True, want_info=True)
        info = assert_close(got, want, kw, kind, '%s %s' % (label, kind))
        own_optimum(info, want[4], kw)


# ---- 2. the seed -------------------------------------------------------------------------------------------------------------------
def test_the_seed_is_the_one_shot_on_the_float64_prediction(engines, golden):
    """the last step's state gradient is nothing but the seed: cloud_match_f64's gradient / (H B) on the float64 prediction of that
    step, which the host reference's forward pass reproduces within 1e-10; its terms likewise"""
    from _f64_grad_ref import _d, step, weights64
    from oracle.propnet_dense import adjacency
    kw = F.train_kw(golden, 'b2_r5', 'data', 'dense', 'seed0')
    e = engines['seed0']
    loss, terms, _, gs, info = call64(e, kw, 'match', want_state=True, want_info=True)
    Wt = weights64(golden.weights_seed0)
    st, sd, at, dens = _d(kw['states']), _d(kw['states_delta']), _d(kw['attrs']), _d(kw['particle_dens'])
    B, H = st.shape[0], st.shape[1] - 1
    cur = st[:, 0]
    for t in range(H):
        adj, _ = adjacency(cur.detach().float(), sd[:, t].float(), 0.08)
        cur = step(Wt, at[:, 0], cur, sd[:, t], dens, adj.double()).detach()
    one = e.cloud_match_f64(cur.numpy(), kw['targets'][:, H - 1], kw['particle_nums'], kw['target_nums'][:, H - 1], want_grad=True,
                            want_match=True)
    rel_t = float(np.abs(one['match'] / (H * B) - terms[H - 1]).max() / np.abs(terms[H - 1]).max())
    rel_g = float(np.abs(one['grad'] / (H * B) - gs[:, H - 1]).max() / np.abs(gs[:, H - 1]).max())
    print('[train-f64-match] last step: one-shot on the reference\'s prediction against the call: terms %.3e, seed %.3e' % (rel_t, rel_g))
    assert rel_t <= TOL and rel_g <= TOL
    np.testing.assert_array_equal(one['match_pq'], info['match'][H - 1])
    np.testing.assert_allclose(one['opt_cost'], info['opt_cost'][H - 1], rtol=TOL)


# ---- 3. the mix ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('impulses', IMPULSES)
def test_the_mix_is_the_weighted_sum_of_the_two_yardsticks(engines, golden, impulses):
    """(1 - w) chamfer + w match of drp_train_grad_f64_untracked's and the 'match' kind's terms, to double rounding, down to the
    bookends w -> 0 and w -> 1; the gradients are linear in the seed, so they combine the same way"""
    kw = F.train_kw(golden, 'b2_r5', impulses, 'dense', 'seed0')
    e = engines['seed0']
    lc, tc, gc, mc, gsc = e.train_grad_f64_untracked(kw['states'], kw.get('states_delta'), kw['attrs'], kw['particle_nums'],
                                                     kw['particle_dens'], kw['targets'], kw['target_nums'], actions=kw.get('actions'),
                                                     want_state=True)
    lm, tm, gm, gsm, im = call64(e, kw, 'match', want_state=True, want_info=True)
    for w in (1e-9, 0.25, 0.5, 0.3, 1.0 - 1e-9):
        lx, tx, gx, gsx, ix = call64(e, kw, 'chamfer+match', w, want_state=True, want_info=True)
        want_t = (1.0 - w) * tc + w * tm
        rel_t = float(np.abs(tx - want_t).max() / np.abs(want_t).max())
        rel_gs = float(np.abs(gsx - ((1.0 - w) * gsc + w * gsm)).max() / np.abs(gsx).max())
        rel_g = float(np.abs(gx - ((1.0 - w) * gc + w * gm)).max() / np.abs(gx).max())
        print('[train-f64-match] mix %s w=%.9g: terms %.3e, seed and state gradient %.3e, weight gradients %.3e' % (impulses, w, rel_t, rel_gs,
                                                                                                                    rel_g))
        # the terms: a handful of roundings apart; the gradients: a linear map of the seed, summed over up to 64 x 10 x 5 edges
        assert rel_t <= 4 * 2.0 ** -52 and rel_gs <= 1e-12 and rel_g <= 1e-12
        np.testing.assert_array_equal(ix['match'], im['match'])            # the same forward pass, the same matching
        np.testing.assert_array_equal(ix['cost'], im['cost'])
        np.testing.assert_array_equal(ix['chamfer_margin'], mc)


# ---- 4. one value, one order -----------------------------------------------------------------------------------------------------
def test_same_bits_from_run_to_run_and_under_a_one_sample_cap(engines, golden):
    e = engines['seed0']
    for impulses in IMPULSES:
        for kind in R.LOSSES:
            kw = F.train_kw(golden, 'b4_r3', impulses, 'dense', 'seed0')
            given = call64(e, kw, kind, want_info=True)[3]['match'].copy()
            given[:, :, [0, 1]] = given[:, :, [1, 0]]
            for match_in in (None, given):
                whole = call64(e, kw, kind, match_in=match_in, want_state=True, want_info=True)
                again = call64(e, kw, kind, match_in=match_in, want_state=True, want_info=True)
                try:
                    e.set_f64_cap(1)                                # one sample is the smallest chunk: B chunks
                    single = call64(e, kw, kind, match_in=match_in, want_state=True, want_info=True)
                finally:
                    e.set_f64_cap(0)
                assert len(flat(whole)) == (7 if kind == 'match' else 8)
                for a, b, c in zip(flat(whole), flat(again), flat(single)):
                    np.testing.assert_array_equal(a, b)
                    np.testing.assert_array_equal(a, c)


# ---- 5. the other yardsticks and the fp32 step are untouched ---------------------------------------------------------------------
def step32_kw(kw, kind, weight=W):
    out = dict((k, kw[k]) for k in ('states', 'attrs', 'particle_nums', 'particle_dens', 'targets', 'target_nums'))
    out.update(dict(actions=kw['actions']) if kw.get('actions') is not None else dict(states_delta=kw['states_delta']))
    out.update(loss=kind, match_weight=weight)
    return out


def test_the_other_yardsticks_and_the_fp32_step_keep_their_bits(golden):
    kw = F.train_kw(golden, 'b2_r5', 'data', 'dense', 'seed0')
    kwa = F.train_kw(golden, 'b2_r5', 'actions', 'dense', 'seed0')
    st, sd, at, nums, dens, tg, tn = (kw[k] for k in ('states', 'states_delta', 'attrs', 'particle_nums', 'particle_dens', 'targets',
                                                      'target_nums'))
    H = st.shape[1] - 1
    eps = TG.transport_eps(dens)

    def others(e):
        out = list(e.train_grad_f64(st, sd, at, nums, dens, want_state=True))
        out += list(e.train_grad_f64_untracked(st, sd, at, nums, dens, tg, tn, want_state=True))
        out += list(e.train_grad_f64_divergence(st, sd, at, nums, dens, tg, tn, eps, 20, want_state=True, want_err=True))
        for kind in R.LOSSES:
            out += list(e.train_step_loss(mode='grad', want_grad=True, want_match=True, **step32_kw(kw, kind)))
        return out
    fresh = new_engine(golden.weights_seed0)
    try:
        fresh.train_begin(H, 1e-3, 0.9)
        want = others(fresh)
    finally:
        fresh.close()
    e = new_engine(golden.weights_seed0)
    try:
        e.train_begin(H, 1e-3, 0.9)
        before = others(e)
        s, d, attr = syn.make_pile(20, 2, seed=1)
        imp = 0.004 * np.random.default_rng(1).standard_normal(s.shape).astype(np.float32)
        e.dispatch_reset()
        e.step(attr, s, imp, d)
        e.step_f64(attr, s, imp, d)
        marks, tap = e.last_dispatch(), e.f64_tap('effect_1')
        w0 = e.get_weights().copy()
        for kind in R.LOSSES:
            call64(e, kw, kind, want_state=True, want_info=True)
            call64(e, kwa, kind)
        p = np.random.default_rng(2).random((2, 9, 3))
        e.cloud_match_f64(p, p[:, :7].astype(np.float32), want_grad=True)
        assert e.last_dispatch() == marks
        np.testing.assert_array_equal(e.f64_tap('effect_1'), tap)      # taps of the earlier call are still answered
        np.testing.assert_array_equal(e.get_weights(), w0)
        after = others(e)
    finally:
        e.close()
    assert len(want) == len(before) == len(after) == 4 + 5 + 6 + 3 + 3
    for a, b, c in zip(want, before, after):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
        np.testing.assert_array_equal(np.asarray(a), np.asarray(c))


def test_probe_without_loss_is_todays(engines, golden):
    kw = F.train_kw(golden, 'b2_r5', 'data', 'dense', 'seed0')
    e = engines['seed0']
    e.train_begin(kw['states'].shape[1] - 1, 1e-3, 0.9)
    args = [kw[k] for k in ('states', 'states_delta', 'attrs', 'particle_nums', 'particle_dens')]
    a, b = e.train_gradient_probe(*args), e.train_gradient_probe(*args, loss=None, match_weight=0.7)
    assert sorted(a) == ['loss32', 'loss64', 'loss_diff', 'rel', 'tape', 'tensors', 'worst'] and a == b
    a = e.train_gradient_probe(*args, targets=kw['targets'], target_nums=kw['target_nums'])
    b = e.train_gradient_probe(*args, targets=kw['targets'], target_nums=kw['target_nums'], loss=None)
    assert sorted(a) == ['loss32', 'loss64', 'loss_diff', 'loss_kind', 'min_margin', 'rel', 'tape', 'tensors', 'worst'] and a == b
    assert a['loss_kind'] == 'chamfer'
    eps = TG.transport_eps(kw['particle_dens'])
    a = e.train_gradient_probe(*args, targets=kw['targets'], target_nums=kw['target_nums'], eps=eps, iters=20)
    assert sorted(a) == ['col_err', 'loss32', 'loss64', 'loss_diff', 'loss_kind', 'rel', 'self_err', 'tape', 'tensors', 'worst']
    with pytest.raises(ValueError, match='loss'):
        e.train_gradient_probe(*args, targets=kw['targets'], target_nums=kw['target_nums'], eps=eps, iters=20, loss='match')


# ---- 6. the probe -------------------------------------------------------------------------------------------------------------------
def run_probe(golden, kw, wset, tape, kind, label):
    """the probe on a fresh context; checks that it is what its two halves give and that it changes no weight -> the dict"""
    k32 = step32_kw(kw, kind)
    H = kw['states'].shape[1] - 1
    e = new_engine(U.weights_of(golden, wset), tape)
    try:
        e.train_begin(H, 1e-3, 0.9)
        w0 = e.get_weights().copy()
        p = e.train_gradient_probe(kw['states'], kw.get('states_delta'), kw['attrs'], kw['particle_nums'], kw['particle_dens'],
                                   actions=kw.get('actions'), targets=kw['targets'], target_nums=kw['target_nums'], loss=kind,
                                   match_weight=W)
        np.testing.assert_array_equal(e.get_weights(), w0)
        loss32, g32, m32 = e.train_step_loss(mode='grad', want_grad=True, want_match=True, **k32)
        loss64, _, g64, info = call64(e, kw, kind, match_in=m32, want_info=True)
        assert p['loss32'] == loss32 and p['loss64'] == loss64
        assert p['flipped'] == int((info['match'] != m32).any(axis=2).sum()) and p['rows_flipped'] == int((info['match'] != m32).sum())
        assert p['cost_gap'] == ((info['cost'] - info['opt_cost']) / info['opt_cost']).max()
        off = 0
        for key, shape in weights.STATE_DICT_KEYS:
            n = int(np.prod(shape))
            assert p['tensors'][key]['max_abs_err'] == np.abs(g32[off:off + n].astype(np.float64) - g64[off:off + n]).max()
            assert p['tensors'][key]['max_abs_ref'] == np.abs(g64[off:off + n]).max()
            off += n
    finally:
        e.close()
    assert p['tape'] == tape and p['loss_kind'] == kind and len(p['tensors']) == 18
    assert ('min_margin' in p) == (kind == 'chamfer+match') and ('rel_own' in p) == (p['flipped'] > 0)
    rel_loss = p['loss_diff'] / abs(p['loss64'])
    print('[match-probe] %s: worst %s rel %.3e, loss rel %.3e, flipped %d (%d rows), cost_gap %.3e%s%s'
          % (label, p['worst'], p['rel'], rel_loss, p['flipped'], p['rows_flipped'], p['cost_gap'],
             ', min_margin %.3e' % p['min_margin'] if 'min_margin' in p else '', ', rel_own %.3e' % p['rel_own'] if 'rel_own' in p else ''))
    for key, t in p['tensors'].items():
        assert t['max_abs_err'] <= GRAD_REL * t['max_abs_ref'], (label, key, t['rel'])
    assert p['rel'] == max(t['rel'] for t in p['tensors'].values()) and p['rel'] <= GRAD_REL
    assert rel_loss <= LOSS_REL
    return p, info


@pytest.mark.parametrize('kind', R.LOSSES)
@pytest.mark.parametrize('impulses', IMPULSES)
@pytest.mark.parametrize('tape', ['fused', 'mfma'])
@pytest.mark.parametrize('name,wset', U.TRAIN_CASES)
def test_probe(golden, name, wset, tape, impulses, kind):
    """MEASURED on one MI355X, the worst tensor's rel over the two batches against the bound GRAD_REL = 2e-4 (flipped 0 and
    cost_gap 0 on all 32 cases; DESIGN.md 2 has the mix's rows):
         match  fused  seed-0  data 5.8e-7  pushes 1.3e-6     trained  data 2.5e-6  pushes 6.7e-6
         match  mfma   seed-0  data 1.2e-6  pushes 2.0e-6     trained  data 3.3e-6  pushes 7.8e-6
    and the loss within 2.5e-7 relative (LOSS_REL = 1e-4)"""
    kw = F.train_kw(golden, name, impulses, 'dense', wset)
    p, _ = run_probe(golden, kw, wset, tape, kind, '%s %s %s %s %s' % (name, wset, tape, impulses, kind))
    # the margins of tests/test_match_f64_host.py (d) are 2.5 x the drift: the fp32 side has the float64 side's partners
    assert p['flipped'] == 0 and p['rows_flipped'] == 0 and p['cost_gap'] == 0.0


@pytest.mark.parametrize('kind', R.LOSSES)
def test_probe_on_the_degenerate_batches(golden, kind):
    for label, batch in (('tiny', U.tiny_batch()), ('single point', U.single_point_batch(golden))):
        p, _ = run_probe(golden, F.batch_kw(batch), 'seed0', 'fused', kind, '%s %s' % (label, kind))
        assert p['flipped'] == 0 and p['cost_gap'] == 0.0


@pytest.mark.parametrize('tape', ['fused', 'mfma'])
def test_a_flipped_partner_is_reported_and_not_mistaken_for_error(golden, tape):
    """two target rows one float32 spacing apart: the fp32 side may take either.  The gradients are compared on ITS pairs, so
    rel stays within GRAD_REL whichever it took; what it took costs, in double, at most the drift more than the optimum"""
    kw = F.flip_kw(golden)
    p, info = run_probe(golden, kw, 'seed0', tape, 'match', 'flip batch %s' % tape)
    excess = info['cost'] - info['opt_cost']
    print('[match-probe] flip batch %s: cost over the float64 optimum, worst %.3e (the drift %.1e)' % (tape, excess.max(), R.DRIFT))
    assert p['rel'] <= GRAD_REL
    assert p['cost_gap'] == 0.0 or (excess <= R.DRIFT).all()
    assert (excess >= 0).all()


# ---- 7. the trainer's hook -----------------------------------------------------------------------------------------------------------
def _model(golden):
    import torch
    model = PropNetDiffDenModel(syn.default_config(), True)
    model.load_state_dict({k[2:]: torch.from_numpy(golden.weights_seed0[k]) for k in golden.weights_seed0.files
                           if k.startswith('w/')}, strict=False)
    model.engine.set_camera(*A.camera_args())
    return model


def hook_batches(impulses):
    """three collate_untracked-shaped batches of two rollout steps; with pushes they are depth-only: no impulses, marked so"""
    out = []
    for it in range(3):
        if impulses == 'actions':
            st, ac, at, nums, dens = A.synthetic_batch([12, 9], 2, 90 + it)
            sd = None
        else:
            st, sd, at, nums, dens = syn.push_batch(it, batch_size=2, n_rollout=2)
            ac = None
        tg, tn = U.make_targets(st, nums, 40 + it)
        data = TG.PaddedBatch((st, sd, at, nums, dens, None, tg, tn))
        data.actions = ac
        data.depth_only = impulses == 'actions'
        out.append(data)
    return out


@pytest.mark.parametrize('kind', R.LOSSES)
@pytest.mark.parametrize('impulses', IMPULSES)
def test_the_trainers_hook_changes_no_weight(golden, impulses, kind):
    config = syn.default_config()
    config['train'].update({'n_rollout': 2, 'n_history': 1, 'lr': 2e-4, 'adam_beta1': 0.9, 'log_per_iter': 1, 'n_epoch': 1})
    batches = hook_batches(impulses)
    res, lines = {}, {}
    for every in (0, 1):
        model = _model(golden)
        lines[every] = []
        r = TG.train(config, model, {'train': batches, 'valid': batches[:1]}, log=lines[every].append, loss=kind, impulses=impulses,
                     match_weight=0.4, match_probe_every=every)
        res[every] = (r, model.engine.get_weights().copy())
        model.engine.close()
    np.testing.assert_array_equal(res[0][1], res[1][1])
    probes = [h for h in res[1][0]['history'] if h[1] == 'grad_probe']
    probe_lines = [ln for ln in lines[1] if ln.startswith('grad_probe')]
    for ln in probe_lines:
        print('[match-probe] hook %s %s: %s' % (impulses, kind, ln))
    assert len(probes) == 3 and all(np.isfinite(h[2]) and h[2] > 0 for h in probes)
    assert [h for h in res[1][0]['history'] if h[1] != 'grad_probe'] == res[0][0]['history']
    assert [ln for ln in lines[1] if not ln.startswith('grad_probe')] == lines[0]
    assert len(probe_lines) == 3 and all('flipped' in ln and 'cost_gap' in ln for ln in probe_lines)
    # the older options still refuse the loss, with a model in hand too
    model = _model(golden)
    try:
        model.engine.train_begin(2, 2e-4, 0.9)
        with pytest.raises(ValueError, match='no float64 yardstick'):
            TG.probe_batch(model, batches[0], impulses, loss=kind)
        pr = TG.probe_batch_match(model, batches[0], impulses, kind, 0.4)
        assert pr['loss_kind'] == kind and float(pr['rel']) == probes[0][2]    # the hook's first probe: the same batch, seed-0 weights
    finally:
        model.engine.close()


@pytest.fixture(scope='module')
def depth_episodes(tmp_path_factory):
    """tests/test_gpu_gnn_frames.py's episodes: depth PNGs and actions.p alone"""
    import os
    import shutil
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import make_golden_gnn_frames as mk
    full = str(tmp_path_factory.mktemp('match64_tracked'))
    syn.write_episodes(full, **mk.EPISODES)
    d = str(tmp_path_factory.mktemp('match64_depth'))
    for ep in os.listdir(full):
        os.makedirs(os.path.join(d, ep))
        for f in os.listdir(os.path.join(full, ep)):
            if not (f.endswith('_particles.npy') or f.endswith('_color.png')):
                shutil.copy(os.path.join(full, ep, f), os.path.join(d, ep, f))
    return d


def test_main_on_depth_episodes_with_the_option(depth_episodes, tmp_path):
    """main(data='depth', loss='chamfer+match', match_probe_every=1): every training batch of a depth-only run is probed"""
    import os
    cfg = TG.default_config()
    cfg['dataset'].update(n_episode=4, n_timestep=6)
    cfg['train'].update(n_rollout=2, batch_size=4, train_valid_ratio=0.5, lr=2e-4, ckp_per_iter=2, log_per_iter=1)
    out = str(tmp_path / 'run')
    eng = Engine(0)
    try:
        result, d = TG.main(cfg, data_root=depth_episodes, train_dir=out, threads=4, n_epoch=1, engine=eng, data='depth',
                            loss='chamfer+match', match_weight=0.4, match_probe_every=1)
    finally:
        eng.close()
    probes = [h for h in result['history'] if h[1] == 'grad_probe']
    log = open(os.path.join(out, 'log.txt')).read().splitlines()
    probe_lines = [ln for ln in log if ln.startswith('grad_probe')]
    for ln in probe_lines:
        print('[match-probe] depth: %s' % ln)
    assert len(probes) >= 1 and len(probe_lines) == len(probes)
    assert all(np.isfinite(h[2]) for h in probes) and all('flipped' in ln and 'cost_gap' in ln for ln in probe_lines)
    rmse = [r for (_, ph, r) in result['history'] if ph in ('train', 'valid')]
    assert len(rmse) == 2 and np.isfinite(rmse).all()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(golden):
    import ctypes
    FP, IP, DP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    kw = F.train_kw(golden, 'b2_r5', 'data', 'dense', 'seed0')
    st, sd, at, nums, dens, tg, tn = (np.ascontiguousarray(kw[k]) for k in ('states', 'states_delta', 'attrs', 'particle_nums',
                                                                            'particle_dens', 'targets', 'target_nums'))
    nums, tn = nums.astype(np.int32), tn.astype(np.int32)
    ac = np.ascontiguousarray(F.train_kw(golden, 'b2_r5', 'actions', 'dense', 'seed0')['actions'])
    B, T1, N, _ = st.shape
    H, M = T1 - 1, tg.shape[2]

    def call(e, sd_=sd, ac_=None, tg_=tg, tn_=tn, M_=M, N_=N, nums_=nums, H_=H, kind_=2, w_=0.5, match_=None):
        f = lambda a, T_: None if a is None else a.ctypes.data_as(T_)
        return e.lib.drp_train_grad_f64_match(e.h, f(st, FP), f(sd_, FP), f(ac_, FP), f(at, FP), f(nums_, IP), f(dens, FP), B, N_, H_,
                                              f(tg_, FP), f(tn_, IP), M_, kind_, w_, f(match_, IP), None, None, None, None, None, None,
                                              None)
    e = Engine(0)
    try:
        assert call(e) == -2 and 'weights not loaded' in e.lib.drp_last_error(e.h).decode()        # DRP_ESTATE
        e.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
        good = call64(e, kw, 'match', want_state=True, want_info=True)                             # no train_begin needed
        valid = np.ascontiguousarray(good[4]['match'], dtype=np.int32)

        def still_works():
            for a, b in zip(flat(call64(e, kw, 'match', want_state=True, want_info=True)), flat(good)):
                np.testing.assert_array_equal(a, b)
        zero_t, big_t = tn.copy(), tn.copy()
        zero_t[1, 1], big_t[0, 0] = 0, M + 1
        dup, far, few, pad = (valid.copy() for _ in range(4))
        dup[1, 0, 1] = dup[1, 0, 0]
        far[2, 1, 0] = tn[1, 2]
        few[0, 1, 2] = -1
        assert nums[1] < N
        pad[3, 1, N - 1] = 0
        refused = [('both impulse sources', dict(ac_=ac), -1), ('neither impulse source', dict(sd_=None), -1),
                   ('pushes without a camera', dict(sd_=None, ac_=ac), -2),
                   ('null targets', dict(tg_=None), -1), ('null target_nums', dict(tn_=None), -1),
                   ('M = 0', dict(M_=0), -1), ('M = 1025', dict(M_=1025), -1), ('N = 1025', dict(N_=1025), -1),
                   ('a target count of 0', dict(tn_=zero_t), -1), ('a target count above M', dict(tn_=big_t), -1),
                   ('a particle count of 0', dict(nums_=np.array([nums[0], 0], np.int32)), -1),
                   ('n_rollout = 0', dict(H_=0), -1), ('n_rollout = 65', dict(H_=65), -1),
                   ('the Chamfer kind', dict(kind_=1), -1), ('kind 0', dict(kind_=0), -1), ('kind 4', dict(kind_=4), -1),
                   ('the mix at w = 0', dict(kind_=3, w_=0.0), -1), ('the mix at w = 1', dict(kind_=3, w_=1.0), -1),
                   ('the mix at w = nan', dict(kind_=3, w_=float('nan')), -1),
                   ('match_in: a duplicate partner', dict(match_=dup), -1), ('match_in: a partner out of range', dict(match_=far), -1),
                   ('match_in: too few pairs', dict(match_=few), -1), ('match_in: a partner on padding', dict(match_=pad), -1)]
        for label, k, rc in refused:
            got = call(e, **k)
            msg = e.lib.drp_last_error(e.h).decode()
            print('[train-f64-match] refusal, %s: %d (%s)' % (label, got, msg))
            assert got == rc, label
            if label.startswith('match_in'):
                assert 'sample' in msg and 'step' in msg and 'row' in msg
            still_works()
        assert call(e, kind_=2, w_=7.0) == 0                                 # match_weight is read by the mix only
        assert call(e, match_=valid) == 0
        e.set_camera(*A.camera_args())
        assert call(e, sd_=None, ac_=ac) == 0
        still_works()
    finally:
        e.close()
