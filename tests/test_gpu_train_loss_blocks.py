"""GPU: the staged input blocks and the result blocks of a trainer call (csrc/train_host.h: the block table) lie where the kernels
read and write them, for every loss kind of both trainers, at the smallest shape at which every block boundary is odd.

The batch: B = 3, n_rollout = 3, N = 5 (particle_nums 5, 3, 4: tests/test_gpu_train_f64.py's hand_made), M = 3 (the first rows of
tests/_untracked_ref.py's make_targets, target_nums a Latin square of 1..3: different within every sample and every step), eps,
reach and mass_q different for every sample (mass_q for every (step, sample); within [1/8, 8]; reach >= 4 eps).  B H = 9 ints,
B H M 3 = 81 floats and B H N 3 = 135 floats each end on an odd word: a block that is misplaced or misaligned lands inside its
neighbour.

Two conditions per loss kind (MSE, Chamfer, match, chamfer+match, transport -- fp32 only --, divergence, divergence with a reach),
both on deterministic kernels, so every comparison is bit for bit:
  1. optional blocks move nothing: the call with every optional output asked for against the call with none -- the loss, the terms
     and the gradient blob, on both trainers (match_in is an input and not part of this);
  2. per-sample blocks follow their sample (float64 trainer): the batch rolled by one sample, with its eps, reach, mass_q column,
     targets and counts, permutes the columns of terms, margin, col_err, self_err, transported, cost, the partners and the rows of
     the state gradient.  The weight-gradient blob is left out: its sum over the samples changes order."""
import numpy as np
import pytest

import _untracked_ref as U
from test_gpu_train_f64 import hand_made, new_engine

pytestmark = pytest.mark.gpu
NUMS, H, M, ITERS = (5, 3, 4), 3, 3, 20
TNUMS = np.array([[1, 2, 3], [2, 3, 1], [3, 1, 2]], np.int32)       # [B][H]
KINDS = ('mse', 'chamfer', 'match', 'chamfer+match', 'transport', 'divergence', 'divergence reach')
MIX = 0.3


def make_batch():
    five = hand_made(list(NUMS), H)
    targets, made = U.make_targets(five[0], five[3], 1)
    assert (made >= TNUMS).all(), made                  # every kept row is a row make_targets drew
    targets = np.ascontiguousarray(targets[:, :, :M])
    for b in range(len(NUMS)):
        for t in range(H):
            targets[b, t, TNUMS[b, t]:] = 0.0
    eps = 1.0 / np.asarray(five[4], np.float64)         # 1/300, 1/350, 1/400
    reach = eps * np.array([4.0, 6.0, 8.0])
    mass_q = np.ascontiguousarray((TNUMS / np.asarray(NUMS, np.float64)[:, None]).T)      # [H][B]: nine different masses
    assert len(set(mass_q.ravel())) == 9 and mass_q.min() >= 0.125 and mass_q.max() <= 8.0
    return {'five': five, 'targets': targets, 'tnums': TNUMS.copy(), 'eps': eps, 'reach': reach, 'mass_q': mass_q}


def rolled(bt):
    """the batch with sample b at b + 1"""
    r = {k: np.roll(v, 1, axis=0) for k, v in bt.items() if k not in ('five', 'mass_q')}
    r['five'] = [np.roll(a, 1, axis=0) for a in bt['five']]
    r['mass_q'] = np.ascontiguousarray(np.roll(bt['mass_q'], 1, axis=1))
    return r


@pytest.fixture(scope='module')
def engine(golden):
    e = new_engine(golden.weights_seed0)
    e.train_begin(H, 1e-3, 0.9)
    yield e
    e.close()


@pytest.fixture(scope='module')
def batch():
    return make_batch()


def step32(e, kind, bt, full, want_grad=True):
    """a fp32 mode='grad' step -> (loss, blob or None)"""
    states, sd, attrs, nums, dens = bt['five']
    six = (states, attrs, nums, dens, bt['targets'], bt['tnums'])
    kw = {'states_delta': sd, 'mode': 'grad', 'want_grad': want_grad}
    if kind == 'mse':
        return e.train_step(*bt['five'], mode='grad', want_grad=want_grad)[:2]
    if kind == 'chamfer':
        return e.train_step_untracked(*bt['five'], bt['targets'], bt['tnums'], mode='grad', want_grad=want_grad)[:2]
    if kind in ('match', 'chamfer+match'):
        return e.train_step_loss(*six, loss=kind, match_weight=MIX, want_match=full, **kw)[:2]
    if kind == 'transport':
        return e.train_step_transport(*six, bt['eps'], ITERS, want_col_err=full, **kw)[:2]
    more = {'reach': bt['reach'], 'mass_q': bt['mass_q']} if kind == 'divergence reach' else {}
    return e.train_step_divergence(*six, bt['eps'], ITERS, want_err=full, **kw, **more)[:2]


def grad64(e, kind, bt, full):
    """a float64 trainer call -> (loss, terms, blob, {name: every further output that was asked for})"""
    states, sd, attrs, nums, dens = bt['five']
    seven = bt['five'] + [bt['targets'], bt['tnums']]
    if kind == 'mse':
        out = e.train_grad_f64(*bt['five'], want_state=full)
        more = {'state': out[3]} if full else {}
    elif kind == 'chamfer':
        out = e.train_grad_f64_untracked(*seven, want_state=full)
        more = {'margin': out[3]}
        if full:
            more['state'] = out[4]
    elif kind in ('match', 'chamfer+match'):
        out = e.train_grad_f64_match(*seven, kind, MIX, want_state=full, want_info=full)
        more = dict(out[4], state=out[3]) if full else {}
        if full and more['chamfer_margin'] is None:
            del more['chamfer_margin']
    else:
        kw = {'reach': bt['reach'], 'mass_q': bt['mass_q']} if kind == 'divergence reach' else {}
        out = e.train_grad_f64_divergence(*seven, bt['eps'], ITERS, want_state=full, want_err=full, **kw)
        more = dict(zip(('state', 'col_err', 'self_err', 'transported'), out[3:])) if full else {}
    return out[0], out[1], out[2], more


@pytest.mark.parametrize('kind', KINDS)
def test_optional_blocks_move_nothing(engine, batch, kind):
    bare, plain, full = (step32(engine, kind, batch, False, False), step32(engine, kind, batch, False),
                         step32(engine, kind, batch, True))
    assert bare[0] == plain[0] == full[0] and np.isfinite(full[0])
    np.testing.assert_array_equal(plain[1], full[1])
    assert np.abs(full[1]).max() > 0
    if kind == 'transport':
        return                                          # no float64 yardstick for the transport loss
    none, every = grad64(engine, kind, batch, False), grad64(engine, kind, batch, True)
    assert none[0] == every[0] and np.isfinite(every[0])
    np.testing.assert_array_equal(none[1], every[1])
    np.testing.assert_array_equal(none[2], every[2])
    assert np.abs(every[2]).max() > 0
    for k, v in none[3].items():                        # (the Chamfer call's margins come back either way)
        np.testing.assert_array_equal(v, every[3][k])


@pytest.mark.parametrize('kind', [k for k in KINDS if k != 'transport'])
def test_per_sample_blocks_follow_their_sample(engine, batch, kind):
    loss, terms, _, more = grad64(engine, kind, batch, True)
    loss_r, terms_r, _, more_r = grad64(engine, kind, rolled(batch), True)
    assert np.unique(terms, axis=1).shape[1] == len(NUMS)           # the samples differ: a column in the wrong place shows
    np.testing.assert_array_equal(terms_r, np.roll(terms, 1, axis=1))
    assert sorted(more) == sorted(more_r) and 'state' in more
    for k, v in more.items():
        np.testing.assert_array_equal(more_r[k], np.roll(v, 1, axis=0 if k == 'state' else 1), err_msg=k)
