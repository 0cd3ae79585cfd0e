"""GPU: the edge branches of the update kernels (csrc/k_mppi.h) that records made from real rollouts never reach -- exact
reward ties (to the lower global index), NaN rewards (sorted last), padded ranks (reward -inf, index -1), fewer valid records
than k, no valid record at all -- driven directly with host records through drp_mpc_update_elite / drp_mpc_update, and the
local kernels on real rewards that hold exact ties.

The yardstick of the elite selection is a brute-force numpy selection written here (filter, lexsort, sum in pick order): the
nominal is asserted bit for bit.  sharding.combine_elite_records / combine_records, the host mirrors, are held to the same."""
import math

import numpy as np
import pytest

from dyn_res_pile_manip_amd import sharding, synthetic as syn, weights
from dyn_res_pile_manip_amd.planners import world2cam_affine

gpu = pytest.mark.gpu

N = 16
ELITE_CASES = ['ties', 'nan', 'padded', 'short', 'nan_short', 'none']
# (ranks, k, H): the bitonic sort in LDS; the k dependent rounds (8192 records x 20 bytes and 1024 sequences are beyond the
# 150 KB the sort path may take: launch_elite_update in csrc/capi_mpc.h)
ELITE_PATHS = {'sort': (2, 8, 2), 'rounds': (8, 1024, 1)}


def elite_records(case, n_ranks, k, H, seed=0):
    """[n_ranks, k, 2 + 4H] records in no particular order (the combine may not rely on one): distinct sequences, distinct
    global indices that do not follow the positions, and the case's rewards"""
    rng = np.random.default_rng(seed)
    n, HJ = n_ranks * k, 4 * H
    rec = np.empty((n, 2 + HJ))
    rec[:, 2:] = rng.uniform(-3.0, 3.0, (n, HJ))
    rec[:, 1] = rng.permutation(4 * n)[:n]
    rec[:, 0] = rng.uniform(-1.0, 0.5, n)
    pos = rng.permutation(n)

    def pad(where):
        rec[where, 0], rec[where, 1] = -np.inf, -1.0
        rec[where, 2:] = 1e6                        # a padded record's sequence must never reach the mean

    if case == 'ties':
        # k/4 winners, all equal: all taken, in index order; then k + k/4 equal records across the k-th place: the
        # k - k/4 of them with the lowest indices are taken.  pos scatters both groups within and across the ranks.
        a, g = k // 4, k + k // 4
        rec[pos[:a], 0] = 2.0
        rec[pos[a:a + g], 0] = 1.0
    elif case == 'nan':
        rec[pos[:n // 4], 0] = np.nan               # valid indices, NaN rewards: 3n/4 >= k valid records remain
        rec[pos[n // 4], 0] = np.inf                # and an infinite reward is a reward: first
    elif case == 'padded':
        pad(np.arange((n_ranks - 1) * k + 3, n))    # the last rank had three samples
    elif case in ('short', 'nan_short'):
        keep = k // 2 + 1                           # fewer valid records than k: taken < k
        gone = pos[keep:]
        pad(gone)
        if case == 'nan_short':
            half = gone[::2]
            rec[half, 0], rec[half, 1] = np.nan, rng.permutation(4 * n)[:half.size]
        rec[pos[0], 0] = -np.inf                    # a valid record whose reward is -inf: the worst of the elite
    elif case == 'none':
        pad(pos)
        half = pos[::2]
        rec[half, 0], rec[half, 1] = np.nan, np.arange(half.size)
    return rec.reshape(n_ranks, k, 2 + HJ)


def brute_elite(records, k, nominal_before):
    """(nominal, elite size, worst elite reward): drop index < 0 and NaN rewards, order by reward descending then index
    ascending, mean of the first min(k, valid) sequences summed in pick order; nothing valid: the nominal stays"""
    rec = records.reshape(-1, records.shape[-1])
    v = rec[(rec[:, 1] >= 0.0) & ~np.isnan(rec[:, 0])]
    order = np.lexsort((v[:, 1], -v[:, 0]))[:k]
    if order.size == 0:
        return np.asarray(nominal_before, np.float64), 0, 0.0
    acc = np.zeros(rec.shape[1] - 2)
    for e in order:
        acc = acc + v[e, 2:]
    return (acc / float(order.size)).reshape(-1, 4), int(order.size), float(v[order[-1], 0])


@pytest.mark.parametrize('path', sorted(ELITE_PATHS))
@pytest.mark.parametrize('case', ELITE_CASES)
def test_host_mirror_is_the_brute_force_selection(case, path):
    """(no GPU) sharding.combine_elite_records on the injected records: the brute-force selection, bit for bit"""
    n_ranks, k, H = ELITE_PATHS[path]
    rec = elite_records(case, n_ranks, k, H)
    before = syn.nominal_pushes(H, seed=2)
    want, n_el, worst = brute_elite(rec, k, before)
    nominal, m_el, m_worst = sharding.combine_elite_records(rec, k)
    assert m_el == n_el == {'ties': k, 'nan': k, 'padded': k, 'short': k // 2 + 1, 'nan_short': k // 2 + 1, 'none': 0}[case]
    if n_el == 0:
        assert nominal is None and m_worst == 0.0
    else:
        np.testing.assert_array_equal(nominal, want)
        assert m_worst == worst and np.isfinite(want).all()
    if case == 'ties':
        # the tie is decided by the index, and the decision shows: taking the group's highest indices gives another mean
        flat = rec.reshape(-1, rec.shape[-1])
        wrong = np.lexsort((-flat[:, 1], -flat[:, 0]))[:k]
        assert not np.allclose(flat[wrong, 2:].mean(0).reshape(-1, 4), want)
        assert worst == 1.0
    if case in ('short', 'nan_short'):
        assert worst == -np.inf


@pytest.fixture(scope='module')
def eng(golden):
    from dyn_res_pile_manip_amd.engine import Engine
    e = Engine(0)
    e.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
    e.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
    obs_goal = syn.goal_distance_image(syn.goal_mask('disc'))
    e.set_goal(syn.goal_field(obs_goal), syn.goal_coor_strided(obs_goal, 5 * N))
    yield e
    e.close()


def begin(eng, H, n_sample, nb=1, sample_offset=0, nominal=None):
    s0, dens, attr = syn.make_pile(N, nb, seed=1)
    lo, hi = syn.action_limits()
    nominal = syn.nominal_pushes(H, seed=2) if nominal is None else nominal
    eng.mpc_begin(s0, attr, dens, nominal, n_sample=n_sample, sigma=0.6, beta_filter=0.7, reward_weight=0.1, act_lo=lo,
                  act_hi=hi, sample_offset=sample_offset)
    return nominal


def stats8(eng):
    """the statistics block: [0..6) mean, std, max, argmax, Z, m of the softmax combine; [6] elite size, [7] worst elite reward"""
    import ctypes
    out = np.empty((8,), dtype=np.float64)
    eng._ck(eng.lib.drp_debug_fetch(eng.h, b'stats', out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
    return out


# ---- 1. injected elite records -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('path', sorted(ELITE_PATHS))
@pytest.mark.parametrize('case', ELITE_CASES)
def test_elite_update_on_injected_records(eng, case, path):
    n_ranks, k, H = ELITE_PATHS[path]
    rec = elite_records(case, n_ranks, k, H)
    before = begin(eng, H, n_sample=4)
    want, n_el, worst = brute_elite(rec, k, before)
    got = eng.mpc_update_elite(rec, k)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(eng.mpc_get(nominal=True)['nominal'], want)       # and it is the session's nominal now
    st = stats8(eng)
    assert st[6] == n_el and st[7] == worst, (st[6:], n_el, worst)


@gpu
def test_elite_update_does_not_depend_on_the_order_of_the_records(eng):
    """the same records, the ranks reversed and each rank's records reversed: the same elite in the same pick order"""
    for path in sorted(ELITE_PATHS):
        n_ranks, k, H = ELITE_PATHS[path]
        rec = elite_records('ties', n_ranks, k, H, seed=3)
        begin(eng, H, n_sample=4)
        a = eng.mpc_update_elite(rec, k)
        b = eng.mpc_update_elite(rec[::-1, ::-1].copy(), k)
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, brute_elite(rec, k, None)[0])


# ---- 2. injected softmax partials --------------------------------------------------------------------------------
def softmax_combine(recs, n_total):
    """k_mppi_update in python floats (IEEE doubles), in the kernel's order"""
    G, HJ = recs.shape[0], recs.shape[1] - 6
    m = -math.inf
    for g in range(G):
        m = max(m, recs[g, 0])
    scale = [math.exp(recs[g, 0] - m) for g in range(G)]
    Z = 0.0
    for g in range(G):
        Z += recs[g, 1] * scale[g]
    nominal = np.empty(HJ)
    for j in range(HJ):
        a = 0.0
        for g in range(G):
            a += recs[g, 2 + j] * scale[g]
        nominal[j] = a / Z
    s1 = s2 = 0.0
    rmax, arg = -math.inf, 0.0
    for g in range(G):
        s1 += recs[g, 2 + HJ]
        s2 += recs[g, 3 + HJ]
        if recs[g, 4 + HJ] > rmax:
            rmax, arg = recs[g, 4 + HJ], recs[g, 5 + HJ]
    mean = s1 / n_total
    var = max((s2 - s1 * mean) / (n_total - 1.0), 0.0) if n_total > 1 else 0.0
    return nominal.reshape(-1, 4), {'mean': mean, 'std': math.sqrt(var), 'max': rmax, 'argmax': int(arg), 'Z': Z, 'm': m}


def softmax_case(case, H=2, ns=4):
    """(records [n_ranks, 6 + 4H], samples per rank, rewards of all ranks, the argmax the combine must report)"""
    rng = np.random.default_rng(11)
    n_ranks = 1 if case == 'one_sample' else 2
    ns = 1 if case == 'one_sample' else ns
    r = rng.uniform(-30.0, -10.0, (n_ranks, ns))
    acts = rng.uniform(-3.0, 3.0, (n_ranks, ns, H, 4))
    if case in ('equal_max', 'equal_max_swapped'):
        r[0, 1] = r[1, 2] = -5.0                    # both ranks attain the maximum: global samples 1 and ns + 2
    if case == 'underflow':
        r[1] -= 1e5                                 # lambda r is 1e4 below the other rank's: exp underflows to 0
    recs = np.stack([sharding.make_record(0.1, r[g], acts[g], g * ns) for g in range(n_ranks)])
    want_arg = int(np.argmax(r.ravel()))
    if case == 'equal_max_swapped':                 # the first RECORD that attains the maximum wins (the kernel's `>`)
        recs = recs[::-1].copy()
        want_arg = ns + 2
    return recs, ns, r, acts, want_arg


@gpu
@pytest.mark.parametrize('case', ['equal_max', 'equal_max_swapped', 'underflow', 'one_sample'])
def test_softmax_update_on_injected_partials(eng, case):
    H = 2
    recs, ns, r, acts, want_arg = softmax_case(case, H)
    begin(eng, H, n_sample=ns)
    got = eng.mpc_update(recs)
    st = eng.mpc_stats()
    n_total = ns * recs.shape[0]
    for nominal, stats in (softmax_combine(recs, float(n_total)), sharding.combine_records(recs, n_total)):
        np.testing.assert_allclose(got, nominal, rtol=1e-12, atol=0)
        for key in ('mean', 'std', 'max', 'Z', 'm'):
            np.testing.assert_allclose(st[key], stats[key], rtol=1e-12, atol=0, err_msg=key)
        assert st['argmax'] == stats['argmax'] == want_arg
    assert st['max'] == r.max() and np.isfinite(got).all()
    if case.startswith('equal_max'):
        assert recs[0, 4 + 4 * H] == recs[1, 4 + 4 * H]
    if case == 'underflow':
        # the far rank's weight is exactly 0: the nominal is the near rank's own softmax mean, its statistics still count
        assert math.exp(recs[1, 0] - recs[0, 0]) == 0.0
        np.testing.assert_allclose(got, (recs[0, 2:2 + 4 * H] / recs[0, 1]).reshape(H, 4), rtol=1e-12, atol=0)
        np.testing.assert_allclose(st['mean'], r.mean(), rtol=1e-12)
    if case == 'one_sample':
        assert st['std'] == 0.0 and st['mean'] == r[0, 0]
        np.testing.assert_allclose(got, acts[0, 0], rtol=1e-12, atol=0)


# ---- 3. the local kernels on real rewards with ties --------------------------------------------------------------
def tied_session(eng, nb, H=2):
    """64 samples = 8 distinct sequences x 8 copies in a fixed shuffle, rolled out: (pushes [64,H,4], group of every sample,
    per-sample reward as the kernels form it: the float64 mean over the nb columns)"""
    member = np.random.default_rng(1).permutation(np.repeat(np.arange(8), 8))
    acts = syn.sample_pushes(8, H, seed=5)[member]
    begin(eng, H, n_sample=64, nb=nb)
    eng.mpc_set_actions(np.repeat(acts, nb, axis=0))
    eng.mpc_rollout()
    return acts, member, sample_rewards(eng, 64, nb)


def sample_rewards(eng, ns, nb):
    r = eng.mpc_get(rewards=True)['rewards'].reshape(ns, nb).astype(np.float64)
    acc = np.zeros(ns)
    for j in range(nb):
        acc = acc + r[:, j]
    return acc / float(nb)


@gpu
@pytest.mark.parametrize('nb', [1, 2])
def test_copies_of_a_sequence_get_the_same_reward_bits(eng, nb):
    _, member, r = tied_session(eng, nb)
    assert np.isfinite(r).all()
    for g in range(8):
        assert len(set(r[member == g].tolist())) == 1, 'the 8 copies of sequence %d got %d different rewards' % (
            g, len(set(r[member == g].tolist())))
    assert len(set(r.tolist())) == 8


@gpu
@pytest.mark.parametrize('nb', [1, 2])
@pytest.mark.parametrize('k', [8, 12])
def test_local_kernels_break_real_ties_by_the_lower_index(eng, nb, k):
    acts, member, r = tied_session(eng, nb)
    top = np.sort(r)[::-1][:k]
    assert (np.diff(top) == 0).any(), 'no exact tie among the top %d rewards: the test would pass vacuously' % k
    rec = eng.mpc_elite(k)
    np.testing.assert_array_equal(rec, sharding.make_elite_records(r, acts, k))
    assert (np.diff(rec[:, 0]) <= 0).all()
    tie = np.diff(rec[:, 0]) == 0
    assert (np.diff(rec[:, 1])[tie] > 0).all()                     # within a tie the indices ascend
    # softmax statistics: the lowest index attaining the maximum
    part = eng.mpc_partials()
    eng.mpc_update(part)
    first = int(np.flatnonzero(r == r.max())[0])
    assert (r == r.max()).sum() > 1 and eng.mpc_stats()['argmax'] == first == int(part[-1])
    # both updates on the device: the elite of the local records, in pick order
    want, n_el, worst = brute_elite(rec, k, None)
    eng.mpc_update_elite_device(k)
    np.testing.assert_array_equal(eng.mpc_get(nominal=True)['nominal'], want)
    st = stats8(eng)
    assert st[3] == first and st[6] == n_el == k and st[7] == worst


@gpu
@pytest.mark.parametrize('k,path', [(8, 'sort'), (16, 'rounds')])
def test_fewer_samples_than_k_pads_the_records(eng, k, path):
    """5 samples, three of them copies of one sequence.  k = 8 = the sort's 2^m >= 5: the sort path, its padding entries
    behind the samples; k = 16 > 8: the k rounds (launch_elite_local in csrc/capi_mpc.h), five of them finding a record."""
    H, ns, offset = 2, 5, 2 ** 33 + 7
    two = syn.sample_pushes(2, H, seed=6)
    acts = two[[0, 1, 0, 1, 0]]
    begin(eng, H, n_sample=ns, sample_offset=offset)
    eng.mpc_set_actions(acts)
    eng.mpc_rollout()
    r = sample_rewards(eng, ns, 1)
    assert r[0] == r[2] == r[4] and r[1] == r[3] and r[0] != r[1], r
    eng.dispatch_reset()
    rec = eng.mpc_elite(k)
    assert 'mppi:k_elite_local %s' % path in eng.last_dispatch()
    np.testing.assert_array_equal(rec, sharding.make_elite_records(r, acts, k, offset))
    assert np.isneginf(rec[ns:, 0]).all() and (rec[ns:, 1] == -1.0).all() and (rec[ns:, 2:] == 0.0).all()
    np.testing.assert_array_equal(rec[:ns, 1] - offset, [0, 2, 4, 1, 3] if r[0] > r[1] else [1, 3, 0, 2, 4])
    want, n_el, worst = brute_elite(rec, k, None)
    np.testing.assert_array_equal(eng.mpc_update_elite(rec, k), want)
    st = stats8(eng)
    assert n_el == ns and st[6] == ns and st[7] == worst == r.min()
