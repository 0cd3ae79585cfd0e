"""The cases of tests/test_gpu_wgrad_cw.py and tools/wgrad_cw.py: batches, the pass through the trainer, the taps, the float64
reconstruction (tests/_wgrad_ref.py) and the job table a pass of B x N x H must have queued.  Needs the library and a device."""
import numpy as np

import _train_actions_ref as A
import _untracked_ref as U
import _wgrad_ref as R
from dyn_res_pile_manip_amd import synthetic as syn, weights

BATCH_KEYS = ('states', 'states_delta', 'attrs', 'particle_nums', 'particle_dens')
# hand-made batches (nums, H): M = 3 and 30; M = 51, odd, padded; one step; an unpadded pair; a sample of one particle; and
# 887 x 10 rows a step -- edge jobs of 9 000 rows > 64 x 128, where the block cap binds and the chains lengthen
HAND = [((3,), 2), ((5, 17, 16), 3), ((33,), 1), ((20, 20), 3), ((7, 1), 1), ((300, 287, 300), 2)]
FIXTURES = [(b, w) for b in ('b4_r3', 'b2_r5') for w in ('seed0', 'trained')]

OFF = {}
_o = 0
for _k, _s in weights.STATE_DICT_KEYS:
    OFF[_k[len('model.'):]] = _o
    _o += int(np.prod(_s))
assert _o == R.N_BLOB


def hand_made(nums, H, seed=0):
    """collate_fn's layout by hand, the construction of tests/test_gpu_train_f64.py: piles away from the origin, where the padding sits"""
    rng = np.random.default_rng(seed)
    B, N = len(nums), max(nums)
    states = np.zeros((B, H + 1, N, 3), np.float32)
    sdelta = np.zeros((B, H, N, 3), np.float32)
    attrs = np.zeros((B, H + 1, N), np.float32)
    dens = np.array([300.0 + 50 * b for b in range(B)], np.float32)
    for b, n in enumerate(nums):
        s, _, _ = syn.make_pile(n, 1, seed=5 + b + seed, kind='blob')
        for t in range(H + 1):
            states[b, t, :n] = s[0] * 0.3 + 0.002 * t * rng.standard_normal((n, 3)).astype(np.float32) + [0, 0, 0.52]
        sdelta[b, :, :n] = 0.004 * rng.standard_normal((H, n, 3)).astype(np.float32)
    return [states, sdelta, attrs, np.asarray(nums, np.int32), dens]


def fixture_batch(golden, name):
    return [golden.train[name + '/' + k] for k in BATCH_KEYS]


def weights_of(golden, wset):
    return golden.weights_seed0 if wset == 'seed0' else golden.weights_trained


def expected_targets(B, N, H):
    """dW offset -> (jobs, M, in, lane_stride, k_stride, db, dwd, rows_per_sample, dens_mod) of a pass of H steps of B x N:
    18 jobs a rollout step -- the predictor's two layers; per propagation step the aggregate block of the particle
    propagator and the receiver and sender blocks of the relation propagator; the particle propagator's encoder block with
    its density column and bias; the particle encoder's two layers; the relation propagator's encoder block with its density
    column and bias and the relation encoder's three layers, over the B N 10 edge slots (capi_train.h, capi_pipeline.h:
    NodeWgrad)"""
    bn, bnk = B * N, B * N * 10
    pp, rp = OFF['particle_propagator.linear.weight'], OFF['relation_propagator.linear.weight']

    def lin(key, M, IN, count=1):
        return (count * H, M, IN, IN, 1, OFF[key + '.bias'], -1, 1, 1)
    return {
        OFF['particle_encoder.model.0.weight']: lin('particle_encoder.model.0', bn, 5),
        OFF['particle_encoder.model.2.weight']: lin('particle_encoder.model.2', bn, 64),
        OFF['relation_encoder.model.0.weight']: lin('relation_encoder.model.0', bnk, 6),
        OFF['relation_encoder.model.2.weight']: lin('relation_encoder.model.2', bnk, 64),
        OFF['relation_encoder.model.4.weight']: lin('relation_encoder.model.4', bnk, 64),
        pp: (H, bn, 64, 129, 1, OFF['particle_propagator.linear.bias'], pp + 128, N, B),
        pp + 64: (3 * H, bn, 64, 129, 1, -1, -1, 1, 1),
        rp: (H, bnk, 64, 193, 1, OFF['relation_propagator.linear.bias'], rp + 192, N * 10, B),
        rp + 64: (3 * H, bn, 64, 193, 1, -1, -1, 1, 1),
        rp + 128: (3 * H, bn, 64, 193, 1, -1, -1, 1, 1),
        OFF['particle_predictor.linear_0.weight']: lin('particle_predictor.linear_0', bn, 64),
        # the 3-wide layer goes in with g and x swapped: 64 lanes of hidden units, 3 columns of output gradient
        OFF['particle_predictor.linear_1.weight']: (H, bn, 3, 1, 64, -1, -1, 1, 1),
    }


def check_structure(jobs, B, N, H):
    """the job table of a pass: 18 H jobs and the column sums; per target the expected count and shape; node jobs of B N
    rows, edge jobs of B N 10"""
    assert len(jobs) == 18 * H + 1, len(jobs)
    want = expected_targets(B, N, H)
    seen = {}
    for q, j in enumerate(jobs[:-1]):
        assert j['dW'] in want, (q, j)
        n, M, IN, ls, ks, db, dwd, rps, dm = want[j['dW']]
        got = (j['M'], j['in'], j['lane_stride'], j['k_stride'], j['db'], j['dwd'], j['rows_per_sample'], j['dens_mod'], j['dens'])
        assert got == (M, IN, ls, ks, db, dwd, rps, dm, int(dwd >= 0)), (q, j, want[j['dW']])
        assert j['blocks'] == min(R.MAX_BLOCKS, -(-M // 64)), (q, j)
        seen[j['dW']] = seen.get(j['dW'], 0) + 1
    assert seen == {k: v[0] for k, v in want.items()}, seen
    for t in range(H):                          # a rollout step's 18 jobs lie together
        assert sorted(j['M'] for j in jobs[18 * t:18 * t + 18]) == [B * N] * 14 + [B * N * 10] * 4
    cs = jobs[-1]
    assert (cs['M'], cs['in'], cs['dW'], cs['db'], cs['dwd']) == (H * B * N, 3, -1, OFF['particle_predictor.linear_1.bias'], -1), cs


def measure(e, grad, B, N, H, mfma, label):
    """after a pass that left `grad`: the taps, the structure, the reconstruction, coverage and exact zeros
    -> {state-dict key: worst |grad - float64 sum| / bound}, printed"""
    jobs, ops, dens = e.train_wgrad_tap()
    check_structure(jobs, B, N, H)
    blob64, blob_abs, depth, rows, cover = R.reconstruct(jobs, ops, dens, mfma=mfma)
    assert grad.dtype == np.float32 and np.isfinite(grad).all()
    dead = R.check_coverage_and_zeros(grad, blob_abs, cover)
    ratios = R.ratio(grad, blob64, blob_abs, depth, rows, weights.STATE_DICT_KEYS)
    off = 0
    for key, shape in weights.STATE_DICT_KEYS:       # nothing vacuous: every tensor has entries with terms to sum
        n = int(np.prod(shape))
        assert blob_abs[off:off + n].max() > 0, key
        off += n
    small = float(np.mean(np.abs(blob64) < 2e-4 * np.abs(blob64).max()))
    print('[wgrad-cw] %s: B=%d N=%d H=%d, %s sums, depth %d..%d, %d entries with all-zero terms, %.0f %% of the blob below 2e-4 of its '
          'largest entry' % (label, B, N, H, 'mfma' if mfma else 'valu', depth.min(), depth.max(), dead, 100 * small))
    for key, _ in weights.STATE_DICT_KEYS:
        print('[wgrad-cw] %s %-45s %.4f of the bound' % (label, key[len('model.'):], ratios[key]))
    return ratios


# ---- the sibling calls: they share the queue ---------------------------------------------------------------------------
def camera_args():
    return A.camera_args()


def pass_actions(e, golden, label='actions b3_n24'):
    """drp_train_step_actions, the MSE through the push (the camera must be set)"""
    b = A.batch(golden, 'b3_n24')
    B, T1, N, _ = b[0].shape
    e.train_begin(T1 - 1, 1e-3, 0.9)
    loss, grad = e.train_step_actions(*b, mode='grad', want_grad=True)
    return measure(e, grad, B, N, T1 - 1, True, label)


def pass_untracked(e, golden, label='untracked b2_r5'):
    """drp_train_step_untracked, the Chamfer loss"""
    b = U.untracked_batch(golden, 'b2_r5')
    B, T1, N, _ = b[0].shape
    e.train_begin(T1 - 1, 1e-3, 0.9)
    loss, grad = e.train_step_untracked(*b, mode='grad', want_grad=True)
    return measure(e, grad, B, N, T1 - 1, True, label)


def pass_accumulate_and_update(e, golden):
    """train_accumulate and train_apply write none of the operands: the taps stay, and what train_apply stepped on -- the float64
    accumulator of ONE pass at weight 1, scale 1, unclipped, back in float32: the pass's own bits -- is within the same bound.
    Then an update pass at the weights that step left: it leaves its operands behind as well.  -> (ratios, ratios)"""
    batch = fixture_batch(golden, 'b2_r5')
    B, T1, N, _ = batch[0].shape
    e.train_begin(T1 - 1, 1e-3, 0.9)
    e.train_step(*batch, mode='grad')
    e.train_accumulate(1.0)
    jobs = e.train_wgrad_jobs()
    out = e.train_apply(1.0, None, want_grad=True)
    assert out['applied'] and out['clip'] == 1.0
    assert e.train_wgrad_jobs() == jobs
    acc = measure(e, out['grad'], B, N, T1 - 1, True, 'accumulate b2_r5')
    loss, grad = e.train_step(*batch, mode='update', want_grad=True)
    return acc, measure(e, grad, B, N, T1 - 1, True, 'update b2_r5')
