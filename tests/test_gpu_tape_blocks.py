"""GPU: the backward tape written by more than one km_prop3 launch, and the cache-size fallback.

run_step_mfma (csrc/capi_pipeline.h) launches km_prop3 once per block of samples (csrc/dispatch.h: cut_blocks), the tape's
launches included: block q > 0 starts b_off * N rows into the neighbour lists, the effect / mask / aggregate histories, the
per-sample states and the self-loop constants, and the kernel takes the whole batch's slot stride (hist_rows).  A wrong offset
there crashes nothing and leaves the forward states right: the tape of block 1 would land on block 0's rows and the gradients
of the tail samples would be silently wrong.  On 256 CUs the tape is cached up to 40 particles and a launch holds at least
1792 samples, so only the batches below are cut -- the smallest that are: a cut needs more than one workgroup of up to 288
rows per CU.  Every test first proves by the launch count (probe_prop_launches: kernels inside the 'prop' probe's regions)
that the cut, or the fallback, is what ran.

Shapes (chunk = n_cu * max(1, (288 if N <= 64 else 256) // N) // nb * nb, from the device's own CU count):
  A  N = 40,  nb = 1,  H = 2, B = 2 * chunk    two equal blocks: the same samples per workgroup, the same kernel variant
  B  N = 40,  nb = 30, H = 2, B = chunk + 30   a tail block of one unit of batch columns, per-particle attributes in every
                                               column (the self loop runs the encoder chain like any other edge)
  M  as B, per-particle attributes in every other column only: see test_mixed_attribute_columns...
  C  N = 17,  nb = 1,  H = 1, B = chunk + 3    rows no multiple of 16 or 32, paired tiles in the tail, the reversed lists
                                               from the lists' own launch (H = 1)
  D  N = 100, nb = 1,  H = 2, B = chunk + 5    DRP_ECACHE_TAPE_MAX_N=128: 256 rows = two samples per workgroup

Bounds.  The measure is gradient_probe's: max |g32 - g64| / max |g64| over the compared rows, per quantity (rewards, d / d push,
d / d state), against gd_grad_f64 on exactly the compared samples as a batch of their own (the call is sample-independent:
test_gpu_gd_f64.py::test_same_bits_alone_in_any_batch_run_and_chunking).  The yardstick is the SAME samples through the path the
suite already holds -- a batch of their own that fits one launch -- and the cut run is held to 5 x the worst yardstick figure
over the four shapes, capped by the loosest fused entry of test_gpu_gd_f64.PROBE_BOUND (3.8e-5).  Measured on an MI355X
(256 CUs), uncut / cut, worst of A ... D:
    rewards     1.20e-7 / 1.20e-7   (A)
    d / d push  1.35e-6 / 1.35e-6   (D)
    d / d state 2.79e-6 / 2.79e-6   (D)
(per shape the cut and the uncut figures agree to every printed digit); the fallback on B: 8.6e-8 / 9.5e-7 / 8.1e-7.
The trainer (N = 40, one rollout step, B = chunk + 7, ragged particle counts on both sides of the boundary) against
train_grad_f64 on the whole batch, by train_gradient_probe's rel (worst tensor's max |g32 - g64| / max |g64|); yardstick: the
first `chunk` samples of the same batch, one launch; bound 5 x that, capped by test_gpu_train_f64.PROBE_TOL (2e-4).  Measured,
uncut / cut: rel 1.246e-5 / 1.244e-5.  The loss is ONE number: its relative difference (measured 1.5e-8 uncut, 8.2e-8 cut --
a sample's term is a double sum times an fp32 factor, 2^-24 = 6e-8) is a single draw of rounding noise and no yardstick for
another draw, so it is held to PROBE_TOL alone, the bound test_gpu_train_f64.py has; seven wrong samples of 1799 would move it
by up to 4e-3.  The float64 pass over the 1799 samples takes 0.2 s.

Same bits wherever a sample lands: every row of every shape, the rows that change block included, is byte-equal under a roll of
the batch (measured: no row differs -- both blocks are cached, and km_prop3's cache / cache+rows and paired / unpaired variants
order every sum alike).  One exception, confirmed from the kernel and pinned by
test_mixed_attribute_columns_change_bits_with_the_tile_mates_only_where_the_self_constant_applies: a batch that MIXES columns
of uniform and of per-particle attributes.  train_step returns no per-sample loss terms, so the trainer has no such check."""
import numpy as np
import pytest

from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.planners import world2cam_affine

pytestmark = pytest.mark.gpu
# the worst uncut figure of the four shapes per quantity, and of the trainer (measured; see above)
YARD = {'reward': 1.20e-7, 'grad_act': 1.35e-6, 'grad_state': 2.79e-6}
YARD_TRAIN = 1.246e-5
GD_CAP, TRAIN_CAP = 3.8e-5, 2e-4          # test_gpu_gd_f64.PROBE_BOUND[('trained', 'fused')], test_gpu_train_f64.PROBE_TOL
BOUND = {k: min(5 * v, GD_CAP) for k, v in YARD.items()}
BOUND_TRAIN = {'rel': min(5 * YARD_TRAIN, TRAIN_CAP), 'loss': TRAIN_CAP}
QUANTITIES = ('reward', 'grad_act', 'grad_state')
SHAPES = {'A': dict(N=40, nb=1, H=2, tail=None), 'B': dict(N=40, nb=30, H=2, tail=30), 'C': dict(N=17, nb=1, H=1, tail=3),
          'D': dict(N=100, nb=1, H=2, tail=5), 'M': dict(N=40, nb=30, H=2, tail=30)}
ENV_D = {'DRP_ECACHE_TAPE_MAX_N': '128'}
SWITCHES = ('DRP_ECACHE_MAX_MB', 'DRP_ECACHE_HARD_MAX_MB', 'DRP_ECACHE_MAX_N', 'DRP_ECACHE_TAPE_MAX_N', 'DRP_NO_PROP3', 'DRP_NO_SELF_CONST')
M34 = world2cam_affine(syn.demo_cam_extrinsics())
CAM = syn.demo_cam_params()
LO, HI = syn.action_limits()
MISS = np.array([7.5, 7.5, 7.9, 7.9], np.float32)     # a short push in a corner of the workspace: it moves nothing
_goal = []


def goal():
    """(the goal's distance image, its field), built once"""
    if not _goal:
        obs = syn.goal_distance_image(syn.goal_mask('I'))
        _goal.extend([obs, syn.goal_field(obs)])
    return _goal


def chunk_of(n_cu, N, nb):
    """csrc/dispatch.h ec_chunk: samples per launch of a cached shape"""
    return n_cu * max(1, (288 if N <= 64 else 256) // N) // nb * nb


def new_engine(golden, mp, **env):
    """a context under exactly the switches of `env`: the policy is read when the context is created"""
    for k in SWITCHES:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)
    e = Engine(0)
    e.load_weights(weights.blob_from_state_dict(golden.weights_seed0), 0.08)
    e.set_camera(M34, 24.0, CAM)
    return e


@pytest.fixture(scope='module')
def eng(golden):
    mp = pytest.MonkeyPatch()
    e = new_engine(golden, mp)
    mp.undo()
    yield e
    e.close()


_cases = {}


def case(name, n_cu):
    """the inputs of a shape, built once: piles, pushes (the samples on both sides of the block boundary miss the pile), the
    goal's pixels, and the picked rows -- 8 on each side of the boundary, the first and the last"""
    if (name, n_cu) not in _cases:
        k = SHAPES[name]
        N, nb, H = k['N'], k['nb'], k['H']
        chunk = chunk_of(n_cu, N, nb)
        B = 2 * chunk if k['tail'] is None else chunk + k['tail']
        s0, dens, attr = syn.make_pile(N, nb, seed=N + nb)
        if name in ('B', 'M'):                        # M: the even columns keep their uniform attributes
            for col in range(1 if name == 'M' else 0, nb, 2 if name == 'M' else 1):
                attr[col, col % 3::3] = 1.0
        acts = syn.sample_pushes(B, H, seed=N + H)
        acts[chunk - 1], acts[chunk] = MISS, MISS
        pick = np.unique(np.clip(np.r_[0, np.arange(chunk - 8, chunk + 8), B - 1], 0, B - 1))
        c = dict(name=name, N=N, nb=nb, H=H, chunk=chunk, B=B, s0=s0, dens=dens, attr=attr, acts=acts, pick=pick,
                 goal_coor=syn.goal_coor_strided(goal()[0], 5 * N), miss=np.array([chunk - 1, chunk]))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cases[(name, n_cu)] = c
    return _cases[(name, n_cu)]


def picked(c):
    """the picked samples as a batch of their own: a batch column each"""
    col = c['pick'] % c['nb']
    return c['s0'][col], c['attr'][col], c['dens'][col], c['acts'][c['pick']]


_ref64 = {}


def ref64(e, c):
    """gd_grad_f64 on the picked samples, once per shape"""
    if c['name'] not in _ref64:
        e.set_goal(goal()[1], c['goal_coor'])
        out = e.gd_grad_f64(*picked(c), want_state_grad=True)
        for v in out:
            v.setflags(write=False)
        _ref64[c['name']] = out
    return _ref64[c['name']]


def gd_grad(e, c, n_blocks, acts=None, inputs=None):
    """gd_begin + gd_grad with the state gradient, the launch count asserted: H regions of n_blocks km_prop3 launches"""
    s0, attr, dens, a = inputs if inputs is not None else (c['s0'], c['attr'], c['dens'], c['acts'] if acts is None else acts)
    e.set_goal(goal()[1], c['goal_coor'])
    e.gd_begin(s0, attr, dens, a, 0.05, LO, HI)
    e.probe_begin('prop')
    out = e.gd_grad(want_state_grad=True)
    regions, kernels = e.probe_read()[1], e.probe_prop_launches()
    e.probe_begin('')
    assert (regions, kernels) == (c['H'], c['H'] * n_blocks), (c['name'], regions, kernels)
    return out


def rels(got, want):
    return {q: float(np.abs(g.astype(np.float64) - w).max() / np.abs(w).max()) for q, g, w in zip(QUANTITIES, got, want)}


def same_bytes(a, b, label, rows=None):
    for q, x, y in zip(QUANTITIES, a, b):
        if rows is not None:
            x, y = x[rows], y[rows]
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.tobytes() != y.tobytes():
            bad = np.flatnonzero((x.reshape(len(x), -1).view(np.uint32) != y.reshape(len(y), -1).view(np.uint32)).any(axis=1))
            raise AssertionError('%s: %s differs in %d rows, first %s' % (label, q, len(bad), bad[:8]))


def check_against_f64(e, c, out, label):
    want = ref64(e, c)
    got = [v[c['pick']] for v in out]
    r = rels(got, want)
    print('[tape-blocks] %s: %s' % (label, ' '.join('%s %.3e' % (q, r[q]) for q in QUANTITIES)))
    # a push that misses the pile: nothing reaches it through s_delta, exactly zero on both sides; every other row is not
    miss = np.isin(c['pick'], c['miss'])
    for g in (got[1], want[1]):
        assert not g[miss].any(), label
        assert (np.abs(g[~miss]).reshape((~miss).sum(), -1).max(axis=1) > 0).all(), label
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    for q in QUANTITIES:
        assert r[q] <= BOUND[q], (label, q, r[q], BOUND[q])
    return r


# ---- a. against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['A', 'B', 'C', 'D'])
def test_the_cut_tape_against_float64(golden, monkeypatch, eng, name):
    e = new_engine(golden, monkeypatch, **ENV_D) if name == 'D' else eng
    try:
        c = case(name, e.device_info()['n_cu'])
        want = ref64(e, c)
        uncut = gd_grad(e, c, 1, inputs=picked(c))                  # the yardstick: the same samples, one launch
        r = rels(uncut, want)
        print('[tape-blocks] %s uncut: %s' % (name, ' '.join('%s %.3e' % (q, r[q]) for q in QUANTITIES)))
        check_against_f64(e, c, gd_grad(e, c, 2), name + ' cut')
    finally:
        if e is not eng:
            e.close()


# ---- b. same bits wherever a sample lands -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['A', 'B', 'C', 'D'])
def test_same_bits_in_either_block_and_from_run_to_run(golden, monkeypatch, eng, name):
    """A: rolled by a block, every sample changes block and workgroup.  B ... D: rolled by one unit of batch columns, the last
    unit of the first block moves into the tail and the tail to the front; every row stays byte-equal, those included."""
    e = new_engine(golden, monkeypatch, **ENV_D) if name == 'D' else eng
    try:
        c = case(name, e.device_info()['n_cu'])
        by = c['chunk'] if name == 'A' else c['nb']
        out = gd_grad(e, c, 2)
        rolled = gd_grad(e, c, 2, acts=np.roll(c['acts'], by, axis=0))
        back = [np.roll(v, -by, axis=0) for v in rolled]
        moved = np.r_[np.arange(c['chunk'] - by, c['chunk']), np.arange(c['B'] - by, c['B'])]
        stay = np.setdiff1d(np.arange(c['B']), moved)
        same_bytes(out, back, name + ' rows that keep their block', stay if name != 'A' else None)
        same_bytes(out, back, name + ' rows that change block', moved if name != 'A' else None)
        same_bytes(out, gd_grad(e, c, 2), name + ' a second run')
    finally:
        if e is not eng:
            e.close()


def test_mixed_attribute_columns_change_bits_with_the_tile_mates_only_where_the_self_constant_applies(eng):
    """The one place where a sample's bits depend on what travels with it, confirmed from the kernel (k_mlp_split.h tile_first:
    f.ks = __all(ok && ...)): the self-edge constant replaces the encoder chain on the self loop for a TILE, when every row of it
    belongs to a sample of uniform attributes; a tile that mixes such a sample with one of per-particle attributes runs the chain
    for all its rows (DESIGN_NOTES.md, "The self-edge constant": the last place of a sum).  With seven samples to a workgroup
    in the first block and one in the tail, a sample of uniform attributes that changes block may change path.  So, M rolled by a
    unit of batch columns: the samples of per-particle attributes -- the chain always -- are byte-equal wherever they land; the
    others hold the bound against float64 in both runs (the picked rows are the ones that change block)."""
    c = case('M', eng.device_info()['n_cu'])
    out = gd_grad(eng, c, 2)
    back = [np.roll(v, -c['nb'], axis=0) for v in gd_grad(eng, c, 2, acts=np.roll(c['acts'], c['nb'], axis=0))]
    same_bytes(out, back, 'M samples of per-particle attributes', np.flatnonzero(np.arange(c['B']) % c['nb'] % 2 == 1))
    check_against_f64(eng, c, out, 'M cut')
    check_against_f64(eng, c, back, 'M cut, rolled')
    same_bytes(out, gd_grad(eng, c, 2), 'M a second run')


# ---- c. stale tape ----------------------------------------------------------------------------------------------------------
def test_a_one_launch_batch_in_between_leaves_nothing_behind(eng):
    """B, then another batch of `chunk` samples in one launch over the same history buffers, then B again: a block that wrote
    outside its slice into history a later pass reads would show"""
    c = case('B', eng.device_info()['n_cu'])
    first = gd_grad(eng, c, 2)
    s0, dens, attr = syn.make_pile(c['N'], c['nb'], seed=77)
    gd_grad(eng, c, 1, inputs=(s0, attr, dens, syn.sample_pushes(c['chunk'], c['H'], seed=78)))
    same_bytes(first, gd_grad(eng, c, 2), 'B after a one-launch batch')


# ---- d. the fallback ----------------------------------------------------------------------------------------------------------
def test_the_cache_size_fallback_recomputes_in_one_launch(golden, monkeypatch, eng):
    c = case('B', eng.device_info()['n_cu'])
    out = {}
    for env in ({'DRP_ECACHE_HARD_MAX_MB': '1'}, {'DRP_ECACHE_MAX_MB': '0'}):
        e = new_engine(golden, monkeypatch, **env)
        try:
            e.dispatch_reset()
            out[tuple(env)] = gd_grad(e, c, 1)
            names = [n for n in e.last_dispatch() if n.startswith('km_prop')]
            assert names == ['km_prop3<tape>'], names
        finally:
            e.close()
    a, b = out.values()
    same_bytes(a, b, 'fallback against DRP_ECACHE_MAX_MB=0')          # both recompute, neither is cut
    check_against_f64(eng, c, a, 'B fallback')


# ---- e. gd_step ---------------------------------------------------------------------------------------------------------------
def test_three_adam_iterations_over_a_cut_batch(eng):
    c = case('B', eng.device_info()['n_cu'])
    res = []
    for by in (0, c['nb']):
        eng.set_goal(goal()[1], c['goal_coor'])
        eng.gd_begin(c['s0'], c['attr'], c['dens'], np.roll(c['acts'], by, axis=0), 0.05, LO, HI)
        eng.probe_begin('prop')
        for _ in range(3):
            eng.gd_step()
        assert (eng.probe_read()[1], eng.probe_prop_launches()) == (3 * c['H'], 3 * c['H'] * 2)
        eng.probe_begin('')
        res.append(np.roll(eng.gd_actions(), -by, axis=0))
    assert res[0].tobytes() == res[1].tobytes()
    assert np.abs(res[0] - c['acts']).max() > 0
    assert (res[0] >= LO.astype(np.float32)).all() and (res[0] <= HI.astype(np.float32)).all()


# ---- f. the trainer -------------------------------------------------------------------------------------------------------------
def train_batch(B, N, chunk):
    """collate_fn's layout (the construction of test_gpu_train_f64.py's hand_made): piles away from the origin, where the padding
    sits; ragged counts on both sides of the block boundary, a single particle and a full sample on each"""
    rng = np.random.default_rng(11)
    nums = np.full(B, N, np.int32)
    nums[chunk - 4:chunk + 4] = [1, 17, 33, N, N, 25, 1, 9]
    nums[5], nums[B - 1] = 23, 31
    s, _, _ = syn.make_pile(N, B, seed=12, kind='blob')
    states = np.zeros((B, 2, N, 3), np.float32)
    for t in range(2):
        states[:, t] = s * 0.3 + 0.002 * t * rng.standard_normal((B, N, 3)).astype(np.float32) + np.float32([0, 0, 0.52])
    sdelta = (0.004 * rng.standard_normal((B, 1, N, 3))).astype(np.float32)
    real = np.arange(N)[None, :] < nums[:, None]
    states *= real[:, None, :, None]
    sdelta *= real[:, None, :, None]
    dens = (300.0 + 50 * (np.arange(B) % 8)).astype(np.float32)
    return [states, sdelta, np.zeros((B, 2, N), np.float32), nums, dens]


def train_rel(e, batch, n_blocks):
    """train_gradient_probe's figures, with the launch count of the forward pass asserted"""
    e.train_begin(1, 1e-3, 0.9)
    e.probe_begin('prop')
    loss32, g32 = e.train_step(*batch, mode='grad', want_grad=True)
    regions, kernels = e.probe_read()[1], e.probe_prop_launches()
    e.probe_begin('')
    assert (regions, kernels) == (1, n_blocks), (regions, kernels)
    loss64, _, g64 = e.train_grad_f64(*batch)
    worst, off = 0.0, 0
    for key, shape in weights.STATE_DICT_KEYS:
        n = int(np.prod(shape))
        err = float(np.abs(g32[off:off + n].astype(np.float64) - g64[off:off + n]).max())
        worst = max(worst, err / max(float(np.abs(g64[off:off + n]).max()), 1e-300))
        off += n
    assert off == g32.size and np.isfinite(g32).all()
    return {'rel': worst, 'loss': abs(loss32 - loss64) / abs(loss64)}


def test_the_trainers_cut_tape_against_float64(eng):
    N = 40
    chunk = chunk_of(eng.device_info()['n_cu'], N, 1)
    batch = train_batch(chunk + 7, N, chunk)
    eng.set_f64_cap(0)
    uncut = train_rel(eng, [v[:chunk] for v in batch], 1)
    print('[tape-blocks] trainer uncut: rel %.3e loss %.3e' % (uncut['rel'], uncut['loss']))
    cut = train_rel(eng, batch, 2)
    print('[tape-blocks] trainer cut: rel %.3e loss %.3e' % (cut['rel'], cut['loss']))
    for k in ('rel', 'loss'):
        assert cut[k] <= BOUND_TRAIN[k], (k, cut[k], BOUND_TRAIN[k])
