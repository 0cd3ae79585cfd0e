"""TEST INFRASTRUCTURE of the matching losses' float64 yardstick (drp_cloud_match_f64, drp_train_grad_f64_match;
csrc/k_match_f64.h): the cases and the certificates.  The definition itself is tests/_match_ref.py's (match64(exact32=False),
train_match64, assign64); nothing is restated here.

  wide_case(shape, B)              _untracked_ref.chamfer_case's clouds with p as float64 whose low bits are random (no widened
                                   floats: every bit of p enters the costs), q float32
  one_shot_reference(shape, B)     match64(exact32=False) of that case, with its uniqueness margins, computed once
  certificate(...)                 what the duals prove without a second solve: u_i + v_j <= C_ij, equality on the pairs,
                                   sum u + sum v = cost, the matching one-to-one with r pairs
  grid_case()                      points on an integer grid scaled by a power of two, rows duplicated: every cost and dual exact
  train_kw(golden, name, ...)      the trainer's batches: the fixtures with _match_ref.dense_targets or their own targets, the tiny
                                   batch, the single-point batch; flip_kw: a target with two rows closer than the fp32 drift
"""
import numpy as np

import _match_ref as R
import _train_actions_ref as A
import _untracked_ref as U

# (n_p, n_q, N, M): one row each, both orientations, a lane stripe (64 columns) exactly and one past it either way, and past the
# stripes of two and of four column slots (128, 256), which a kernel with slot-count variants would treat apart
SHAPES = [(1, 1, 1, 1), (5, 3, 8, 8), (3, 5, 8, 8), (64, 64, 64, 64), (65, 64, 65, 64), (64, 65, 64, 65), (70, 130, 70, 130),
          (129, 128, 129, 128), (257, 300, 257, 300)]
BATCHES = (1, 3)
# the certificate alone (no O(n^3) numpy solve): the cap, a few rows against nearly the cap, the cap against one row
BIG_SHAPES = [(1024, 1024, 1024, 1024), (17, 1023, 20, 1023), (1024, 1, 1024, 4)]
# the seed of a case whose seed-0 clouds leave a uniqueness margin below R.MARGIN_MIN (tests/test_match_f64_host.py holds the rest)
SEED = {((257, 300, 257, 300), 3): 1}        # seed 0: sample 0's second-best matching is 6.3e-10 away


def wide_case(shape, B, seed=None):
    """-> (p [B, N, 3] float64, q [B, M, 3] float32, n_p, n_q): chamfer_case's clouds, every coordinate of p moved by a random
    fraction (up to half) of its float32 spacing, so that its low 29 bits are random; the padding keeps its rubbish"""
    if seed is None:
        seed = SEED.get((tuple(shape), B), 0)
    p, q, n_p, n_q = U.chamfer_case(shape, B, seed)
    rng = np.random.default_rng(5000 + 31 * seed + 7 * shape[0] + 13 * shape[1] + B)
    p64 = p.astype(np.float64) + (rng.random(p.shape) - 0.5) * np.spacing(np.abs(p)).astype(np.float64)
    assert (p64.astype(np.float32).astype(np.float64) != p64).mean() > 0.9
    return p64, q, n_p, n_q


_cache = {}


def one_shot_reference(shape, B, want_margin=False):
    key = (tuple(shape), B)
    if key not in _cache or (want_margin and not _cache[key][1]):
        p, q, n_p, n_q = wide_case(shape, B)
        ref = R.match64(p, q, n_p, n_q, exact32=False, want_margin=want_margin)
        for v in ref.values():
            v.setflags(write=False)
        _cache[key] = (ref, want_margin)
    return _cache[key][0]


def certificate(p, q, n, m, u, v, match_pq, cost):
    """one problem: p [n, 3] float64, q [m, 3], duals u [n], v [m], p's partners [n], the reported sum of C over them -> the
    figures {'slack': the most by which a dual pair exceeds its cost, 'tight': the most by which a matched pair's duals miss it,
    'sum': |sum u + sum v - cost|, 'cost': |cost - sum C over the pairs|}, all relative to max C; asserts the matching is
    one-to-one with r = min(n, m) pairs"""
    C = R.cost64(p[:n], q[:m])
    top = float(C.max())
    on = np.nonzero(match_pq[:n] >= 0)[0]
    partners = match_pq[:n][on]
    r = min(n, m)
    assert len(on) == r and len(set(partners.tolist())) == r and partners.min() >= 0 and partners.max() < m
    red = u[:n, None] + v[None, :m] - C
    return {'slack': float(red.max()) / top, 'tight': float(np.abs(red[on, partners]).max()) / top,
            'sum': abs(float(u[:n].sum() + v[:m].sum()) - cost) / top, 'cost': abs(float(C[on, partners].sum()) - cost) / top,
            'r': r}


def grid_case():
    """-> (p [2, 12, 3] float64, q [2, 14, 3] float32, n_p, n_q): integer grid points times 2^-6 with duplicated rows in both
    clouds: every difference, cost, dual and shortest distance is an integer multiple of 2^-14 far below 2^53 of them, so the
    solver's arithmetic is exact and ties are ties in every implementation; sample 1 is the other orientation, its target half a
    grid step away in x so that no cost is zero"""
    rng = np.random.default_rng(12)
    s = 2.0 ** -6
    p = np.zeros((2, 12, 3))
    q = np.zeros((2, 14, 3), np.float32)
    base = rng.integers(0, 4, (8, 3)).astype(np.float64)
    p[0, :10] = np.concatenate([base[:6], base[:4]]) * s                # four rows twice
    q[0, :14] = (np.concatenate([base, base[:6]]) * s).astype(np.float32)
    p[1, :12] = np.concatenate([base, base[:4]]) * s
    q[1, :7] = ((np.concatenate([base[2:7], base[2:4]]) + [0.5, 0.0, 0.0]) * s).astype(np.float32)
    return p, q, np.array([10, 12], np.int32), np.array([14, 7], np.int32)


# ---- the trainer's batches ------------------------------------------------------------------------------------------------------
TRAIN_BATCHES = ('b4_r3', 'b2_r5')
TARGETS = ('dense', 'sparse')
# A case's smallest uniqueness margin AND smallest Chamfer arg-min margin (the mix) on the float64 prediction must be at least
# this for the fp32 side to be held to the float64 side's partners: 2.5 x R.DRIFT, the fp32-vs-float64 drift of a squared distance
# of a predicted state.  tests/test_match_f64_host.py holds every case below to it on the CPU.
PROBE_MARGIN_MIN = 1e-7
# dense_targets' seed per (batch, weight set, impulse source): the first of 0..59 that gives PROBE_MARGIN_MIN (the duplicated
# rows' jitter of 1e-3 leaves near-ties: seed 0 gives 8e-10 on b4_r3 / seed0 / data)
DENSE_SEED = {('b4_r3', 'seed0', 'data'): 8, ('b4_r3', 'seed0', 'actions'): 2, ('b4_r3', 'trained', 'data'): 20,
              ('b4_r3', 'trained', 'actions'): 0, ('b2_r5', 'seed0', 'data'): 2, ('b2_r5', 'seed0', 'actions'): 0,
              ('b2_r5', 'trained', 'data'): 1, ('b2_r5', 'trained', 'actions'): 0}


def train_kw(golden, name, impulses='data', targets='dense', wset='seed0'):
    """-> the keyword arguments of Engine.train_step_loss for fixture batch `name` (data impulses or pushes) against
    _match_ref.dense_targets (more target rows than predicted ones: every predicted row has a partner; seeded per weight set) or the
    batch's own untracked targets (fewer: predicted rows are left unmatched)"""
    if impulses == 'data':
        st, sd, at, nums, dens = U.fixture_batch(golden, name)
        kw = dict(states=st, attrs=at, particle_nums=nums, particle_dens=dens, states_delta=sd)
    else:
        st, acts, at, nums, dens = A.batch(golden, name)
        kw = dict(states=st, attrs=at, particle_nums=nums, particle_dens=dens, actions=acts)
    if targets == 'dense':
        kw['targets'], kw['target_nums'] = R.dense_targets(st, nums, DENSE_SEED[(name, wset, impulses)])
    else:
        kw['targets'], kw['target_nums'] = (U.make_targets(st, nums, U.TARGET_SEED[name]) if impulses == 'data'
                                            else A.targets_of(golden, name))
    return kw


def batch_kw(batch):
    st, sd, at, nums, dens, tg, tn = batch
    return dict(states=st, attrs=at, particle_nums=nums, particle_dens=dens, targets=tg, target_nums=tn, states_delta=sd)


def flip_kw(golden):
    """b2_r5 against dense targets where, in every (sample, step), target row 1 is row 0 moved by one float32 spacing in x: whichever
    predicted row takes one of the two, the other costs it about 2 |p - q| 3e-8 < 1e-9 more -- far less than the fp32 drift of a
    squared distance (R.DRIFT = 4e-8), so the fp32 side may pick either"""
    kw = train_kw(golden, 'b2_r5', 'data', 'dense', 'seed0')
    tg = kw['targets'].copy()
    tg[:, :, 1] = tg[:, :, 0]
    tg[:, :, 1, 0] = np.nextafter(tg[:, :, 0, 0], np.float32(np.inf))
    kw['targets'] = tg
    return kw


def reference(kw, W, matches=None, kind='match', weight=0.5):
    return R.train_match64(W, kw['states'], kw.get('states_delta'), kw['attrs'], kw['particle_nums'], kw['particle_dens'],
                           kw['targets'], kw['target_nums'], matches=matches, kind=kind, weight=weight, actions=kw.get('actions'))


_train_cache = {}


def train_reference(golden, name, wset, impulses, targets, kind, weight=0.25):
    """train_match64 of a fixture case with the matching solved on its own prediction, computed once and left unchanged"""
    key = (name, wset, impulses, targets, kind, weight)
    if key not in _train_cache:
        _train_cache[key] = reference(train_kw(golden, name, impulses, targets, wset), U.weights_of(golden, wset), None, kind, weight)
    return _train_cache[key]
