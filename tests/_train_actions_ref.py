"""TEST INFRASTRUCTURE of training through the push (drp_train_step_actions, drp_train_grad_f64_actions): the float64 reference,
the batches the GPU tests run on, and the preconditions of every GPU comparison -- built here so that
tests/test_train_actions_host.py can assert them on the CPU.

  train_actions64(W, states, actions, ...)   tests/_f64_train_ref.py's loop with sd[:, t] replaced by
                                             _f64_grad_ref.gen_s_delta(s_cur[b, :n], actions[b, t], m34, gs) on the real rows and
                                             zeros on the padding; the MSE term, or tests/_untracked_ref.py's Chamfer term when
                                             targets are given; torch float64 autograd (the hard mask is a comparison: constant)
  push_margin(s, action)                     how far every row of s is from a decision of gen_s_delta that fp32 could flip

The margin.  Positions are about 0.2 in x and y and 0.75 in z, so u, v and L are sums of three products of such numbers: their
fp32 rounding is a few ulp of 0.75, 2e-7.  The fp32 drift of a predicted state against float64 is about 1e-6 (the figure
tests/_untracked_ref.py derives its MARGIN_MIN from).  1.2e-6 in all: PUSH_MARGIN_MIN = 1e-5 is eight times that.  |u| and |u - L|
above it keep the hard mask, ||v| - w| above it keeps the side of the soft mask's kink.  Over a few hundred rows with spacings of
1e-2 a draw lands inside 1e-5 of one of the three lines with a probability of a few percent: the seeds below are those for which
none does, and tests/test_train_actions_host.py holds every one of them; no case is skipped at run time.

The mask case puts real rows next to the zero rows, so there its graphs are held as well (graph_margin): every sender of a real
receiver, padded ones included, is further than the same 1e-5 from the radius and from a tie at the top-10 cut.
"""
import numpy as np
import torch

from oracle import propnet_sparse as osp
from oracle.propnet_dense import adjacency
from dyn_res_pile_manip_amd import synthetic as syn
import _f64_grad_ref as R
from _f64_grad_ref import _d, step, weights64
from _f64_train_ref import PARAMS, blob64, real_rows  # noqa: F401  (re-exported for the tests)
import _untracked_ref as U

GS = 24.0
M34 = np.ascontiguousarray(osp.world2cam_affine(syn.demo_cam_extrinsics(), GS), np.float64)     # the fixture camera
PUSH_MARGIN_MIN = 1e-5
LOSS_REL = 1e-4
GRAD_REL = 2e-4


def camera_args():
    """what Engine.set_camera takes for the fixture camera"""
    return M34, GS, syn.demo_cam_params()


def _frame(action):
    """[B, 4] float64 tensor -> (sc, ec, dirn [B, 3], length [B]) of planners.py:231-240"""
    m34 = torch.from_numpy(M34)
    B = action.shape[0]
    zero = torch.zeros((B, 1), dtype=torch.float64)
    one = torch.ones((B, 1), dtype=torch.float64)
    sc = torch.cat([action[:, 0:1], zero, -action[:, 1:2], one], 1) @ m34.t() / GS
    ec = torch.cat([action[:, 2:3], zero, -action[:, 3:4], one], 1) @ m34.t() / GS
    d = ec - sc
    length = torch.linalg.norm(d, dim=1)
    return sc, ec, d / length[:, None], length


def push_margin(s, action):
    """s [n, 3], action [4] (float64 tensors or arrays) -> the smallest of |u|, |u - L| and ||v| - w| over the rows"""
    s = torch.as_tensor(np.asarray(s, np.float64))
    a = torch.as_tensor(np.asarray(action, np.float64))[None]
    sc, _, dirn, length = _frame(a)
    rel = s - sc
    u = rel @ dirn[0]
    v = rel[:, 1] * dirn[0, 0] - rel[:, 0] * dirn[0, 1]
    m = torch.minimum(torch.minimum(u.abs(), (u - length[0]).abs()), (v.abs() - R.PUSHER_W).abs())
    return float(m.min())


def graph_margin(p, nums, adj_thresh=0.08):
    """p [B, N, 3] (the positions a step's graph is built on, s_cur + impulse), nums -> over every real receiver: the smallest
    | |p_j - p_i| - adj_thresh | over all senders j, padded ones included, and the smallest gap between its 10th and 11th
    nearest sender where the 10th is inside the radius and the two are not both padded rows.  (Padded rows coincide and carry
    the same state, so which of them fill the last slots changes nothing a real row receives; the count is 10 either way.)"""
    p = np.asarray(p, np.float64)
    radius, gap = np.inf, np.inf
    for b, n in enumerate(nums):
        assert (p[b, n:] == p[b, n:n + 1]).all()
        d = np.linalg.norm(p[b, :n, None] - p[b, None], axis=-1)
        radius = min(radius, float(np.abs(d - adj_thresh).min()))
        order = np.argsort(d, axis=1, kind='stable')
        d = np.take_along_axis(d, order, 1)
        for i in range(n if d.shape[1] > 10 else 0):
            if d[i, 9] < adj_thresh and not (order[i, 9] >= n and order[i, 10] >= n):
                gap = min(gap, float(d[i, 10] - d[i, 9]))
    return radius, gap


def impulses64(s_cur, actions_t, nums):
    """s_cur [B, N, 3], actions_t [B, 4] float64 tensors -> [B, N, 3]: gen_s_delta per sample on its real rows, zeros below"""
    m34 = torch.from_numpy(M34)
    rows = []
    for b, n in enumerate(nums):
        sd = R.gen_s_delta(s_cur[b:b + 1, :n], actions_t[b:b + 1], m34, GS)[0]
        rows.append(torch.cat([sd, torch.zeros((s_cur.shape[1] - n, 3), dtype=torch.float64)], 0))
    return torch.stack(rows)


def train_actions64(W, states, actions, attrs, particle_nums, particle_dens, targets=None, target_nums=None, adj_thresh=0.08,
                    keep64=False, nudge=None, masked=True):
    """-> (loss, terms [H, B], {key: gradient}, d loss / d every step's predicted state [B, H, N, 3], info), float64.
    info: 'push_margin' (the smallest push_margin over steps and samples), 'margin' (the smallest Chamfer arg-min margin, inf with
    the MSE), 'preds' [B, H, N, 3] (the predicted states), 'sdelta' [B, H, N, 3] (the impulses used), 'graphs' (per-step
    adjacency).  nudge = (t, b, i, k, h): h added to coordinate k of row i of sample b's prediction of step t.  masked=False: the
    padded rows get gen_s_delta's value too (what an unmasked kernel would compute; the mask test's counter-example)."""
    if keep64:
        W = dict((k, torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float64)))) for k, v in W.items())
    else:
        W = weights64(W)
    W = dict((k, v.clone().requires_grad_(True)) for k, v in W.items())
    st, ac, at, dens = _d(states), _d(actions), _d(attrs), _d(particle_dens)
    nums = [int(n) for n in np.asarray(particle_nums)]
    B, T1, N, _ = st.shape
    H = T1 - 1
    chamfer = targets is not None
    if chamfer:
        tg, tnums = _d(targets), np.asarray(target_nums)
    s_cur, a_cur = st[:, 0], at[:, 0]
    terms, preds, sds, graphs = [], [], [], []
    pmargin, cmargin = np.inf, np.inf
    for t in range(H):
        for b in range(B):
            pmargin = min(pmargin, push_margin(s_cur[b, :nums[b]].detach(), ac[b, t]))
        sd = impulses64(s_cur, ac[:, t], nums if masked else [N] * B)
        adj, _ = adjacency(s_cur.detach().float(), sd.detach().float(), adj_thresh)
        s_pred = step(W, a_cur, s_cur, sd, dens, adj.double())
        if nudge is not None and nudge[0] == t:
            bump = torch.zeros_like(s_pred)
            bump[nudge[1], nudge[2], nudge[3]] = nudge[4]
            s_pred = s_pred + bump
        s_pred.retain_grad()
        preds.append(s_pred)
        sds.append(sd.detach())
        graphs.append(adj.bool().numpy())
        row = []
        for b in range(B):
            n = nums[b]
            if chamfer:
                m = int(tnums[b, t])
                pb, qb = s_pred[b, :n], tg[b, t, :m]
                a, _, ma = U._nearest(pb.detach().numpy(), qb.numpy())
                c, _, mc = U._nearest(qb.numpy(), pb.detach().numpy())
                cmargin = min(cmargin, float(ma.min()), float(mc.min()))
                row.append((((pb - qb[torch.from_numpy(a)]) ** 2).mean() + ((qb - pb[torch.from_numpy(c)]) ** 2).mean()) / (H * B))
            else:
                row.append(((s_pred[b, :n] - st[b, t + 1, :n]) ** 2).mean() / (H * B))
        terms.append(torch.stack(row))
        s_cur = s_pred
    terms = torch.stack(terms)
    loss = terms.sum()
    loss.backward()
    grads = dict((k, W[k].grad.numpy().copy()) for k in PARAMS)
    g_state = np.stack([p.grad.numpy() if p.grad is not None else np.zeros((B, N, 3)) for p in preds], 1)
    info = {'push_margin': pmargin, 'margin': cmargin, 'preds': np.stack([p.detach().numpy() for p in preds], 1),
            'sdelta': np.stack([s.numpy() for s in sds], 1), 'graphs': graphs}
    return float(loss.item()), terms.detach().numpy(), grads, g_state, info


# ---- the batches ----------------------------------------------------------------------------------------------------------
def _sd32(cur, push):
    """the impulse of one push on one cloud [n, 3], float64 arithmetic, as float32 (the generator of recorded next states)"""
    sd = R.gen_s_delta(torch.from_numpy(cur[None].astype(np.float64)), torch.from_numpy(push[None].astype(np.float64)),
                       torch.from_numpy(M34), GS)[0]
    return sd.numpy().astype(np.float32)


def synthetic_batch(nums, H, seed, kinds=('uniform', 'blob')):
    """-> [states [B, H+1, N, 3], actions [B, H, 4], attrs [B, H+1, N], particle_nums, particle_dens]: piles of syn.make_pile, each step a push of syn.pushes_through
    across the current pile, the recorded next state = state + 0.7 impulse + 1.5e-3 jitter (tests/golden/make_golden_train.py's
    recipe), zero-padded to max(nums) as collate_fn pads"""
    rng = np.random.default_rng(31000 + seed)
    B, N = len(nums), max(nums)
    states = np.zeros((B, H + 1, N, 3), np.float32)
    actions = np.zeros((B, H, 4), np.float32)
    dens = np.zeros((B,), np.float32)
    for b, n in enumerate(nums):
        s, d, _ = syn.make_pile(n, 1, seed=seed * 10 + b, kind=kinds[b % len(kinds)])
        dens[b] = d[0] * rng.uniform(0.6, 1.4)
        cur = s[0]
        states[b, 0, :n] = cur
        for t in range(H):
            actions[b, t] = syn.pushes_through(cur[None], seed=seed * 100 + b * 10 + t)[0]
            cur = (cur + 0.7 * _sd32(cur, actions[b, t]) + 0.0015 * rng.standard_normal(cur.shape)).astype(np.float32)
            states[b, t + 1, :n] = cur
    return [states, actions, np.zeros((B, H + 1, N), np.float32), np.asarray(nums, np.int32), dens]


def fixture_actions(states, particle_nums, seed):
    """seeded pushes across the pile for a fixture batch: actions[b, t] crosses states[b, t, :n_b]"""
    B, T1 = states.shape[:2]
    acts = np.zeros((B, T1 - 1, 4), np.float32)
    for b in range(B):
        n = int(particle_nums[b])
        for t in range(T1 - 1):
            acts[b, t] = syn.pushes_through(states[b, t, :n][None], seed=seed * 100 + b * 10 + t)[0]
    return acts


# The seeds chosen (tests/test_train_actions_host.py holds every margin they give, push and Chamfer, on both weight sets):
SEEDS = {'b3_n24': 0, 'b4_r3': 0, 'b2_r5': 0, 'n300': 0, 'tiny': 0, 'mask': 0, 'golden': 0}
TARGET_SEED = {'b3_n24': 0, 'b4_r3': 1, 'b2_r5': 0}      # b4_r3: seed 0 leaves an arg-min margin of 1.4e-8 on the trained weights
CASE_NAMES = ('b3_n24', 'b4_r3', 'b2_r5')
TRAIN_CASES = [(b, w) for b in CASE_NAMES for w in ('seed0', 'trained')]

_batches = {}


def batch(golden, name):
    """the five arrays of train_step_actions for a named case (computed once, read-only):
      b3_n24   B = 3, N = 24 with counts 24 / 17 / 9, H = 3
      b4_r3, b2_r5   the fixture batches of train.npz with seeded pushes across the pile in place of their impulses
      n300     B = 2, N = 300 (counts 300 / 270: beyond one pass of a 256-thread block), H = 2
      tiny     B = 1, N = n = 5, H = 1, unpadded
      mask     b3_n24's shapes with every push from (-3, 0) to (3, 0): over the camera-frame origin, where the zero rows sit.
               Sample 1 (17 of 24) lies in the plane z = 0 instead of 0.75, around its 7 zero rows, so that they are senders of
               real rows and what an unmasked kernel does to them reaches the loss (the impulse does not read z: the demo
               camera looks straight down, every push runs at z = 0.75 with no z component).  Sample 2 (9 of 24) stays at
               0.75: a real receiver among 15 coincident zero rows would leave its top-10 to a tie
      golden   tests/golden/train_actions.npz's batch: B = 2, N = 16 with counts 16 / 11, H = 3"""
    if name not in _batches:
        if name == 'b3_n24':
            out = synthetic_batch([24, 17, 9], 3, 40 + SEEDS[name])
        elif name in ('b4_r3', 'b2_r5'):
            st, _, at, nums, dens = U.fixture_batch(golden, name)
            out = [st, fixture_actions(st, nums, SEEDS[name]), at, nums, dens]
        elif name == 'n300':
            out = synthetic_batch([300, 270], 2, 50 + SEEDS[name])
        elif name == 'tiny':
            out = synthetic_batch([5], 1, 60 + SEEDS[name], kinds=('blob',))
        elif name == 'mask':
            out = synthetic_batch([24, 17, 9], 3, 70 + SEEDS[name])
            out[1][:] = np.array([-3.0, 0.0, 3.0, 0.0], np.float32)
            out[0][1, :, :17, 2] -= np.float32(0.75)
        elif name == 'golden':
            out = synthetic_batch([16, 11], 3, 80 + SEEDS[name])
        else:
            raise KeyError(name)
        out = [np.ascontiguousarray(a) for a in out]
        for a in out:
            a.setflags(write=False)
        _batches[name] = out
    return list(_batches[name])


def targets_of(golden, name):
    """untracked target clouds of a case's recorded states (tests/_untracked_ref.py: make_targets)"""
    b = batch(golden, name)
    return list(U.make_targets(b[0], b[3], 500 + TARGET_SEED[name]))


def weights_of(golden, wset):
    return golden.weights_seed0 if wset == 'seed0' else golden.weights_trained


_cache = {}


def reference(golden, name, wset, loss='mse', masked=True):
    """train_actions64 of a case, computed once and left unchanged -> (loss, terms, gradient blob, g_state on real rows, info)"""
    key = (name, wset, loss, masked)
    if key not in _cache:
        b = batch(golden, name)
        extra = targets_of(golden, name) if loss == 'chamfer' else []
        l, terms, grads, gs, info = train_actions64(weights_of(golden, wset), *(b + extra), masked=masked)
        out = (l, terms, blob64(grads), real_rows(gs, b[3]), info)
        for v in out[1:4]:
            v.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def adam_trajectory64(golden, name, lr, beta1, steps=3):
    """`steps` Adam steps (torch.optim.Adam's update, eps = 1e-8, beta2 = 0.999) in numpy float64 on train_actions64's MSE
    gradients from the seed-0 weights -> (losses before each update, the blob after the last, the first step's gradient blob, the
    smallest push margin on the way)"""
    key = ('adam', name, float(lr), float(beta1), steps)
    if key not in _cache:
        b = batch(golden, name)
        W = dict((k, v.numpy().copy()) for k, v in weights64(golden.weights_seed0).items())
        m = dict((k, np.zeros_like(W[k])) for k in PARAMS)
        v = dict((k, np.zeros_like(W[k])) for k in PARAMS)
        losses, margin, g0 = [], np.inf, None
        for it in range(1, steps + 1):
            loss, _, grads, _, info = train_actions64(W, *b, keep64=True)
            losses.append(loss)
            margin = min(margin, info['push_margin'])
            if g0 is None:
                g0 = blob64(grads)
            for k in PARAMS:
                m[k] = beta1 * m[k] + (1 - beta1) * grads[k]
                v[k] = 0.999 * v[k] + 0.001 * grads[k] ** 2
                W[k] = W[k] - lr * (m[k] / (1 - beta1 ** it)) / (np.sqrt(v[k] / (1 - 0.999 ** it)) + 1e-8)
        _cache[key] = (losses, blob64(W), g0, margin)
    return _cache[key]
