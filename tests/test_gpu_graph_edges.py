"""GPU: every neighbour-list builder against the host oracle (oracle/propnet_sparse.build_neighbours, itself held to the
reference's arithmetic by tests/test_graph_edge_host.py) on the cases of tests/_graph_edge_cases.py -- pairs an ulp to either
side of the radius at seven radii, particles on the strip and band boundaries, exact ties at the cut, lines, one strip, a tiny
and a zero radius -- and the reversed lists of every kernel that builds them against reverse_lists_np of the lists fetched
beside them.  Every comparison is equality of integers, and every call is asked which kernel served it (last_dispatch): a case
does not pass by running another builder."""
import numpy as np
import pytest

import _graph_edge_cases as G
import _train_actions_ref as A
from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd.planners import world2cam_affine
from oracle import propnet_sparse as osp

pytestmark = pytest.mark.gpu
K = G.K

SWITCHES = ('DRP_NO_GRAPH_STRIPS', 'DRP_NO_GRAPH_CELLS', 'DRP_GRAPH_CELLS_MIN_N', 'DRP_GRAPH_CELLS_HB', 'DRP_GRAPH_CELLS_HALO',
            'DRP_GRAPH_Q4', 'DRP_NO_GRAPH_ENCODE', 'DRP_NO_GRAPH_REV', 'DRP_REV_GLOBAL')
Q4_ENCODE = 'graph:km_graph_q4_encode (+ particle encoder)'
STRIPS128, STRIPS256 = 'graph:k_graph_strips_q<128>', 'graph:k_graph_strips_q<256>'

# builder -> (switches, the variant last_dispatch must name; None: by the particle count)
BUILDERS = {
    'plain': ({'DRP_NO_GRAPH_STRIPS': '1', 'DRP_GRAPH_Q4': '0'}, 'graph:k_graph'),
    'q4': ({'DRP_NO_GRAPH_STRIPS': '1', 'DRP_GRAPH_Q4': '2'}, 'graph:k_graph_q4'),
    'strips': ({'DRP_NO_GRAPH_CELLS': '1'}, None),                  # <128>, from 800 particles <256>
    'cells': ({'DRP_GRAPH_CELLS_MIN_N': '1'}, 'graph:k_graph_cells'),
}
for _hb in ('0.02', '0.7'):
    for _halo in ('0.005', '0.1'):
        BUILDERS['cells_hb%s_halo%s' % (_hb, _halo)] = ({'DRP_GRAPH_CELLS_MIN_N': '1', 'DRP_GRAPH_CELLS_HB': _hb,
                                                         'DRP_GRAPH_CELLS_HALO': _halo}, 'graph:k_graph_cells')

_blob = []
_ref = {}


def new_engine(monkeypatch, env, radius, engine=None, goal_n=0):
    """a context created under exactly the switches of `env`"""
    from dyn_res_pile_manip_amd.engine import Engine
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if not _blob:
        _blob.append(weights.blob_from_state_dict(weights.random_state_dict(seed=0)))
    e = Engine(0, engine=engine)
    e.load_weights(_blob[0], radius)
    e.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
    if goal_n:
        obs_goal = syn.goal_distance_image(syn.goal_mask('I'))
        e.set_goal(syn.goal_field(obs_goal), syn.goal_coor_strided(obs_goal, 5 * goal_n))
    return e


def oracle_lists(c):
    """the case's lists by the host oracle, computed once and left unchanged"""
    if c.name not in _ref:
        idx, cnt = osp.build_neighbours(c.s_cur, c.s_delta, c.radius)
        idx.setflags(write=False)
        cnt.setflags(write=False)
        _ref[c.name] = (idx, cnt)
    return _ref[c.name]


def graph_marks(ran):
    return [n for n in ran if n.startswith('graph:')]


def describe(c, idx, cnt, ref_idx, ref_cnt):
    """what differs, in the shell's terms where the case has them (printed before the assertion)"""
    msg = '%s: %d of %d receivers with another count' % (c.name, int((cnt.astype(np.int32) != ref_cnt).sum()), cnt.size)
    if 'send_cls' in c.meta:
        for k in G.CLASSES:
            listed = total = 0
            for b in range(c.B):
                send, recv, cls = c.meta['send'][b], c.meta['send_recv'][b], c.meta['send_cls'][b]
                for j, i in zip(send[cls == k].tolist(), recv[cls == k].tolist()):
                    total += 1
                    listed += int(j in idx[b, i, :cnt[b, i]].tolist())
            msg += '; T%+d ulp senders listed with their receiver: %d of %d' % (k, listed, total)
    return msg


def assert_same_senders(idx, cnt, ref_idx, ref_cnt, label):
    """per receiver the oracle's count and set of senders; unused slots -1; the receiver itself first and the rest ascending, or
    everything ascending"""
    B, N, _ = idx.shape
    idx, cnt = idx.astype(np.int32), cnt.astype(np.int32)
    used = np.arange(K)[None, None, :] < cnt[..., None]
    assert np.array_equal(cnt, ref_cnt), label
    assert (idx[~used] == -1).all(), label
    big = np.int32(1 << 20)
    assert np.array_equal(np.sort(np.where(used, idx, big), -1), np.where(ref_idx >= 0, ref_idx, big)), label
    me = np.broadcast_to(np.arange(N, dtype=np.int32)[None, :], (B, N))
    self_first = (cnt > 0) & (idx[..., 0] == me)
    asc = np.where(used, idx, big)
    rest_ok = (np.diff(asc[..., 1:], axis=-1) >= 0).all(-1)
    all_ok = (np.diff(asc, axis=-1) >= 0).all(-1)
    assert np.where(self_first, rest_ok, all_ok).all(), label
    return self_first


# ---- 1. drp_build_graph: every case on every builder ------------------------------------------------------------------------
@pytest.mark.parametrize('builder', list(BUILDERS))
@pytest.mark.parametrize('name', G.CASE_NAMES)
def test_builder_gives_the_oracles_lists(monkeypatch, name, builder):
    c = G.case(name)
    ref_idx, ref_cnt = oracle_lists(c)
    env, want = BUILDERS[builder]
    if want is None:
        want = STRIPS256 if c.N >= 800 else STRIPS128
    e = new_engine(monkeypatch, env, c.radius)         # (a zero radius is loaded like any other: nothing to refuse)
    try:
        e.dispatch_reset()
        idx, cnt = e.build_graph(c.s_cur, c.s_delta)
        ran = e.last_dispatch()
    finally:
        e.close()
    assert graph_marks(ran) == [want], ran
    print('[graph-edges] %s %s' % (builder, describe(c, idx, cnt, ref_idx, ref_cnt)))
    assert np.array_equal(cnt.astype(np.int32), ref_cnt)
    assert np.array_equal(idx.astype(np.int32), ref_idx)


def test_both_strip_widths_are_reached():
    """the <256> variant needs 800 particles: the 820-particle lattice is the case that runs it"""
    sizes = [G.case(n).N for n in G.CASE_NAMES]
    assert max(sizes) == 820 and min(sizes) > 128


# ---- 2. inside a step: data impulses, the fused engine's launches and the fp32 matrix engine's ----------------------------------
STEP_CASES = ('shell_r0.08', 'shell_r0.1', 'lattice_n300_r0.08')
STEP_RUNS = {
    'fused_q4_encode': ('fused', {'DRP_NO_GRAPH_STRIPS': '1'}, Q4_ENCODE),
    'fused_strips': ('fused', {}, STRIPS128),
    'mfma_strips': ('mfma', {}, STRIPS128),
    'mfma_q4': ('mfma', {'DRP_NO_GRAPH_STRIPS': '1'}, 'graph:k_graph_q4'),
}


@pytest.mark.parametrize('run', list(STEP_RUNS))
@pytest.mark.parametrize('name', STEP_CASES)
def test_lists_inside_a_step(monkeypatch, name, run):
    c = G.case(name)
    ref_idx, ref_cnt = oracle_lists(c)
    engine, env, want = STEP_RUNS[run]
    e = new_engine(monkeypatch, env, c.radius, engine=engine)
    try:
        e.dispatch_reset()
        out = e.step(np.zeros((c.B, c.N), np.float32), c.s_cur, c.s_delta, np.full((c.B,), c.N / 0.16, np.float32))
        ran = e.last_dispatch()
        idx = e.debug_fetch('nbr_idx', (c.B, c.N, K), np.int16)
        cnt = e.debug_fetch('nbr_cnt', (c.B, c.N), np.uint8)
    finally:
        e.close()
    assert graph_marks(ran) == [want], ran
    assert np.isfinite(out).all()
    print('[graph-edges] step %s %s' % (run, describe(c, idx, cnt, ref_idx, ref_cnt)))
    assert_same_senders(idx, cnt, ref_idx, ref_cnt, (name, run))


@pytest.mark.parametrize('name', STEP_CASES)
def test_self_loop_first_in_the_trainers_forward(monkeypatch, name):
    """The trainer's forward pass hands its steps the per-sample self-edge constant, so its lists start with the self loop, and
    with data impulses on the fused tape lists and particle encoder share a launch (km_graph_q4_encode): the oracle's senders
    per receiver, the receiver first, the rest ascending; and the reversed lists of that pass (kb_reverse_lists<256> with every
    receiver real) are reverse_lists_np of those lists."""
    c = G.case(name)
    ref_idx, ref_cnt = oracle_lists(c)
    B, N = c.B, c.N
    e = new_engine(monkeypatch, {}, c.radius)
    try:
        e.train_begin(1, 1e-3, 0.9)
        e.dispatch_reset()
        states = np.stack([c.s_cur, c.s_cur], 1)
        loss, _ = e.train_step(states, c.s_delta[:, None], np.zeros((B, 2, N), np.float32), np.full((B,), N, np.int32),
                               np.full((B,), N / 0.16, np.float32), mode='grad')
        ran = e.last_dispatch()
        idx = e.debug_fetch('train_nbr_idx', (1, B, N, K), np.int16)[0]
        cnt = e.debug_fetch('train_nbr_cnt', (1, B, N), np.uint8)[0]
        rev_off = e.debug_fetch('train_rev_off', (1, B, N + 1), np.int32)[0]
        rev = e.debug_fetch('train_rev', (1, B, N * K), np.int32)[0]
    finally:
        e.close()
    assert graph_marks(ran) == [Q4_ENCODE] and 'kb_reverse_lists<256>' in ran, ran
    assert np.isfinite(loss)
    self_first = assert_same_senders(idx, cnt, ref_idx, ref_cnt, name)
    assert self_first.all()
    assert_reversed(idx, cnt, rev_off, rev, None, name)


# ---- 3. reversed lists ---------------------------------------------------------------------------------------------------------
def assert_reversed(idx, cnt, rev_off, rev, n_recv, label):
    want_off, want_rev = G.reverse_lists_np(idx, cnt, n_recv)
    assert np.array_equal(rev_off, want_off), label
    for b in range(idx.shape[0]):
        assert np.array_equal(rev[b, :rev_off[b, -1]], want_rev[b]), (label, b)


# (N, switches, the marks the pass must leave)
REV_RUNS = {
    'graph_rev_n7': (7, {}, ['graph:k_graph_rev']),
    'graph_rev_n128': (128, {}, ['graph:k_graph_rev']),
    'own_launch_n128': (128, {'DRP_NO_GRAPH_REV': '1'}, ['kb_reverse_lists<256>']),
    'lds256_n300': (300, {}, ['kb_reverse_lists<256>']),
    'lds1024_n520': (520, {}, ['kb_reverse_lists<1024>']),
    'global_n300': (300, {'DRP_REV_GLOBAL': '1'}, ['kb_reverse_lists<256>']),
}


@pytest.mark.parametrize('run', list(REV_RUNS))
def test_reversed_lists_of_a_planner_pass(monkeypatch, run):
    """gd_begin + gd_grad at horizon 1: the pass's lists (of the pushed positions, the self loop first on the fused tape) and
    the reversed lists its backward pass gathered over.  The lists themselves are the oracle's on the fetched impulses."""
    N, env, marks = REV_RUNS[run]
    B = 6
    s0, dens, attr = syn.make_pile(N, 1, seed=N)
    acts = syn.sample_pushes(B, 1, seed=N)
    lo, hi = syn.action_limits()
    e = new_engine(monkeypatch, env, 0.08, goal_n=N)
    try:
        e.gd_begin(s0, attr, dens, acts, 0.05, lo, hi)
        e.dispatch_reset()
        r, g, _ = e.gd_grad()
        ran = e.last_dispatch()
        idx = e.debug_fetch('nbr_idx', (B, N, K), np.int16)
        cnt = e.debug_fetch('nbr_cnt', (B, N), np.uint8)
        sd = e.debug_fetch('s_delta', (B, N, 3))
        rev_off = e.debug_fetch('rev_off', (B, N + 1), np.int32)
        rev = e.debug_fetch('rev', (B, N * K), np.int32)
    finally:
        e.close()
    own_launch = [n for n in ran if n.startswith('kb_reverse_lists')]
    if marks == ['graph:k_graph_rev']:
        assert 'graph:k_graph_rev' in ran and not own_launch, ran
    else:
        assert own_launch == marks and 'graph:k_graph_rev' not in ran, ran
    assert np.isfinite(r).all() and np.isfinite(g).all() and np.abs(sd).max() > 0
    ref_idx, ref_cnt = osp.build_neighbours(np.tile(s0, (B, 1, 1)), sd, 0.08)
    assert_same_senders(idx, cnt, ref_idx, ref_cnt, run)
    assert cnt.min() >= 1 and rev_off[:, -1].min() >= N
    assert_reversed(idx, cnt, rev_off, rev, None, run)


def self_first_neighbours(s_cur, s_delta, radius):
    """build_neighbours with the one thing the self-first emission order decides otherwise: among senders at the SAME distance
    the receiver itself comes before the lower indices.  It matters only where more than ten senders sit at distance 0 -- the
    coincident zero rows of a padded batch -- a tie the reference's topk leaves open; the ascending order (drp_build_graph)
    keeps the ten lowest indices there, the self-first order the receiver and the nine lowest others.  A sort per receiver."""
    p = np.asarray(s_cur, np.float32) + np.asarray(s_delta, np.float32)
    B, N, _ = p.shape
    thr = np.float32(radius * radius)
    idx = -np.ones((B, N, K), np.int32)
    cnt = np.zeros((B, N), np.int32)
    for b in range(B):
        d = G.dis32(p[b][None, :, :] - p[b][:, None, :])
        bits = d.view(np.uint32)
        for i in range(N):
            order = sorted(range(N), key=lambda j: (int(bits[i, j]), j != i, j))[:K]
            keep = sorted(j for j in order if (d[i, j] - thr) < 0)
            idx[b, i, :len(keep)] = keep
            cnt[b, i] = len(keep)
    return idx, cnt


def test_reversed_lists_of_a_padded_training_batch(monkeypatch, golden):
    """Counts 24 / 17 / 9 in N = 24, data impulses: the reversed lists leave the padded receivers out (DESIGN.md section 11,
    item 1c) -- reverse_lists_np with n_recv = particle_nums -- on every rollout step of the pass.  The lists themselves are the
    oracle's on the real receivers and self_first_neighbours' on all of them (fifteen coincident zero rows in the third sample:
    more ties at distance 0 than slots)."""
    st, _, at, nums, dens = A.batch(golden, 'b3_n24')
    B, T1, N, _ = st.shape
    H = T1 - 1
    rng = np.random.default_rng(5)
    sd = (0.004 * rng.standard_normal((B, H, N, 3))).astype(np.float32)
    for b in range(B):
        sd[b, :, nums[b]:] = 0.0                       # collate_fn's zero rows
    e = new_engine(monkeypatch, {}, 0.08)
    try:
        e.train_begin(H, 1e-3, 0.9)
        e.dispatch_reset()
        loss, _ = e.train_step(st, sd, at, nums, dens, mode='grad')
        ran = e.last_dispatch()
        idx = e.debug_fetch('train_nbr_idx', (H, B, N, K), np.int16)
        cnt = e.debug_fetch('train_nbr_cnt', (H, B, N), np.uint8)
        rev_off = e.debug_fetch('train_rev_off', (H, B, N + 1), np.int32)
        rev = e.debug_fetch('train_rev', (H, B, N * K), np.int32)
        states = e.debug_fetch('train_states', (B, H, N, 3))
    finally:
        e.close()
    assert 'kb_reverse_lists<256>' in ran and graph_marks(ran) == ['graph:k_graph'], ran
    assert np.isfinite(loss)
    for t in range(H):
        # the step's lists are the oracle's on the state the step read: the batch's first state, then the pass's own predictions
        s_in = st[:, 0] if t == 0 else states[:, t - 1]
        ref_idx, ref_cnt = self_first_neighbours(s_in, sd[:, t], 0.08)
        first = assert_same_senders(idx[t], cnt[t], ref_idx, ref_cnt, t)
        assert first.all()
        asc_idx, asc_cnt = osp.build_neighbours(s_in, sd[:, t], 0.08)
        for b in range(B):
            assert np.array_equal(ref_cnt[b, :nums[b]], asc_cnt[b, :nums[b]]) and np.array_equal(ref_idx[b, :nums[b]], asc_idx[b, :nums[b]])
        if t == 0:
            assert not np.array_equal(ref_idx[2], asc_idx[2])           # the two tie rules do part on the coincident rows
        assert_reversed(idx[t], cnt[t], rev_off[t], rev[t], nums, t)
        full = G.reverse_lists_np(idx[t], cnt[t], None)[0]
        assert (rev_off[t][1:, -1] < full[1:, -1]).all()                 # the padded samples' lists ARE shorter: the rule binds
