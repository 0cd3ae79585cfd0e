"""GPU: the trainer's weight-gradient sums held to a componentwise bound.

The 38 403 gradients of a training pass are fp32 sums over rows the backward kernels leave in device memory (kt_wgrad_mfma_list /
kt_wgrad_list, kt_wgrad_reduce_lists, kt_colsum3, planned by plan_wgrad_lists).  With deferred weight gradients every operand of
every job is still there when the call returns: the debug taps "train_wgrad_*" hand them out, tests/_wgrad_ref.py sums them in
float64 and bounds the fp32 error of every entry by (D + 2) 2^-24 sum |g| |x| + rows 2^-126 with the depth D derived from the
kernels' loops (its docstring).  Every entry of every tensor must be within that bound, every entry must be written by a job,
and an entry whose terms are all zero (the attribute columns, dead units) must be exactly 0.0.

The only yardstick is the float64 reconstruction: nothing here compares the device with its own sums.  What this does not hold:
the rows themselves (under the norm-wise bound of tests/test_gpu_train_f64.py: one ReLU that flips between fp32 and float64 moves
single entries by 1e5 units of this bound), and a job that was never queued, which only those tests see -- the job table is
checked here against the 18 jobs a rollout step must queue.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import _wgrad_cases as C
from dyn_res_pile_manip_amd import _lib, synthetic as syn, weights
from dyn_res_pile_manip_amd._lib import DrpError
from dyn_res_pile_manip_amd.engine import Engine

pytestmark = pytest.mark.gpu
BATCHES = [('hand', nums, H) for nums, H in C.HAND] + [('fixture', name, wset) for name, wset in C.FIXTURES]


def batch_id(b):
    return 'n%s-H%d' % ('_'.join(str(n) for n in b[1]), b[2]) if b[0] == 'hand' else '%s-%s' % b[1:]


def new_engine(w, monkeypatch, tape=None, valu=False, camera=False, flushed=False):
    for k, on in (('DRP_NO_WGRAD_MFMA', valu), ('DRP_NO_WGRAD_DEFER', flushed)):      # read when the context is made
        if on:
            monkeypatch.setenv(k, '1')
        else:
            monkeypatch.delenv(k, raising=False)
    e = Engine(0)
    e.load_weights(weights.blob_from_state_dict(w), 0.08)
    if camera:
        e.set_camera(*C.camera_args())
    if tape is not None:
        e.set_engine(tape)
    return e


def assert_ratios(ratios, label):
    for key, r in ratios.items():
        assert r <= 1.0, (label, key, r)


@pytest.mark.parametrize('sums', ['mfma', 'valu'])
@pytest.mark.parametrize('tape', ['fused', 'mfma'])
@pytest.mark.parametrize('b', BATCHES, ids=batch_id)
def test_every_gradient_entry_within_the_bound_of_its_sum(golden, monkeypatch, b, tape, sums):
    if b[0] == 'hand':
        batch, w = C.hand_made(list(b[1]), b[2]), golden.weights_seed0
    else:
        batch, w = C.fixture_batch(golden, b[1]), C.weights_of(golden, b[2])
    B, T1, N, _ = batch[0].shape
    e = new_engine(w, monkeypatch, tape, valu=sums == 'valu')
    try:
        e.train_begin(T1 - 1, 1e-3, 0.9)
        e.dispatch_reset()
        loss, grad = e.train_step(*batch, mode='grad', want_grad=True)
        ran = e.last_dispatch()
        label = '%s %s/%s' % (batch_id(b), tape, sums)
        ratios = C.measure(e, grad, B, N, T1 - 1, sums == 'mfma', label)
    finally:
        e.close()
    assert 'train:deferred wgrad lists' in ran and ('train:kt_wgrad_mfma' in ran) == (sums == 'mfma') \
        and ('train:kt_wgrad' in ran) == (sums == 'valu'), ran
    assert_ratios(ratios, label)


def test_through_the_push_and_against_untracked_clouds(golden, monkeypatch):
    """drp_train_step_actions (the MSE through the push) and drp_train_step_untracked (the Chamfer loss): the same queue behind
    another seed and another impulse source"""
    e = new_engine(golden.weights_trained, monkeypatch, camera=True)
    try:
        assert_ratios(C.pass_actions(e, golden), 'actions')
        assert_ratios(C.pass_untracked(e, golden), 'untracked')
    finally:
        e.close()


def test_the_accumulate_path_and_an_update_keep_the_taps(golden, monkeypatch):
    """tests/_wgrad_cases.py: pass_accumulate_and_update"""
    e = new_engine(golden.weights_seed0, monkeypatch)
    try:
        acc, upd = C.pass_accumulate_and_update(e, golden)
    finally:
        e.close()
    assert_ratios(acc, 'accumulate')
    assert_ratios(upd, 'update')


def test_refusals(golden, monkeypatch):
    batch = C.fixture_batch(golden, 'b2_r5')
    H = batch[0].shape[1] - 1
    e = new_engine(golden.weights_seed0, monkeypatch)
    try:
        with pytest.raises(DrpError, match='not populated'):                    # nothing has run
            e.train_wgrad_jobs()
        e.train_begin(H, 1e-3, 0.9)
        with pytest.raises(DrpError, match='not populated'):
            e.train_wgrad_jobs()
        e.train_step(*batch, mode='grad')
        n = len(e.train_wgrad_jobs())
        assert n == 18 * H + 1
        # a bad index, a bad name: DRP_EINVAL, and the taps stay
        for name in ('train_wgrad_g:%d' % n, 'train_wgrad_x:%d' % (n - 1), 'train_wgrad_g:-1', 'train_wgrad_x:1x', 'train_wgrad_g:',
                     'train_wgrad_rows'):
            with pytest.raises(DrpError, match='drp error -1:'):
                e.debug_fetch(name, (1 << 20,))
        with pytest.raises(DrpError, match='needs'):                            # a buffer too small
            e.debug_fetch('train_wgrad_g:0', (8,))
        assert e.debug_fetch('train_wgrad_g:%d' % (n - 1), (H * batch[0].shape[0] * batch[0].shape[2], 3)).shape[1] == 3
        # no reverse pass: DRP_TRAIN_EVAL, train_predict
        e.train_step(*batch, mode='eval')
        with pytest.raises(DrpError, match='not populated'):
            e.train_wgrad_jobs()
        e.train_step(*batch, mode='grad')
        e.train_wgrad_jobs()
        e.train_predict(batch[0], batch[2], batch[3], batch[4], states_delta=batch[1])
        with pytest.raises(DrpError, match='not populated'):
            e.debug_fetch('train_wgrad_dens', (batch[0].shape[0],))
        # a refused trainer call
        e.train_step(*batch, mode='grad')
        bad = [a.copy() for a in batch]
        bad[3][0] = 0
        with pytest.raises(DrpError):
            e.train_step(*bad, mode='grad')
        with pytest.raises(DrpError, match='not populated'):
            e.train_wgrad_jobs()
        # a trainer call refused before it looks at its batch: no impulse source, through the C ABI itself (the wrapper would not)
        e.train_step(*batch, mode='grad')
        e.train_wgrad_jobs()
        st, at, nums, dn = (np.ascontiguousarray(batch[i]) for i in (0, 2, 3, 4))
        fp, ip = (lambda a: a.ctypes.data_as(_lib.c_float_p)), (lambda a: a.ctypes.data_as(_lib.c_int32_p))
        pred = np.empty((st.shape[0], H, st.shape[2], 3), np.float32)
        assert e.lib.drp_train_predict(e.h, fp(st), None, None, fp(at), ip(nums), fp(dn), st.shape[0], st.shape[2], fp(pred)) == -1
        with pytest.raises(DrpError, match='not populated'):
            e.train_wgrad_jobs()
        # calls that stage a step's inputs where the operands lie: a forward step, the float64 pass
        s, dens, attr = syn.make_pile(20, 2, seed=1)
        sd = 0.004 * np.random.default_rng(1).standard_normal(s.shape).astype(np.float32)
        for other in (lambda: e.step(attr, s, sd, dens), lambda: e.train_grad_f64(*batch)):
            e.train_step(*batch, mode='grad')
            e.train_wgrad_jobs()
            other()
            with pytest.raises(DrpError, match='not populated'):
                e.train_wgrad_jobs()
            with pytest.raises(DrpError, match='not populated'):
                e.debug_fetch('train_wgrad_g:0', (1 << 20,))
    finally:
        e.close()
    # a pass that did not defer
    e = new_engine(golden.weights_seed0, monkeypatch, flushed=True)
    try:
        e.train_begin(H, 1e-3, 0.9)
        e.train_step(*batch, mode='grad')
        with pytest.raises(DrpError, match='not populated'):
            e.train_wgrad_jobs()
    finally:
        e.close()
