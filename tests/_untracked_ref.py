"""TEST INFRASTRUCTURE of the untracked (Chamfer) loss: the float64 references of drp_cloud_chamfer and
drp_train_step_untracked, and the batches their GPU tests run on -- built here so that tests/test_untracked_host.py can assert,
on the CPU, the precondition of every GPU comparison: each arg-min of the float64 reference wins by a margin above MARGIN_MIN.

  chamfer64(p, q, n_p, n_q)        numpy float64 on the fp32 inputs widened exactly; np.argmin takes the first occurrence, which
                                   IS the tie rule (lowest index); also each arg-min's margin (second best - best squared distance)
  train_untracked64(W, ...)        tests/_f64_train_ref.py's loop with the term replaced (same step, weights64 and adjacency)
  make_targets(states, nums, seed) dataset_gnn_dyn.drop_correspondence plus a seeded jitter of 1e-3: the arg-min partner is not
                                   the tracked one for a good share of the rows
"""
import numpy as np
import torch

from oracle.propnet_dense import adjacency
from _f64_grad_ref import _d, step, weights64
from _f64_train_ref import PARAMS, blob64, real_rows  # noqa: F401  (re-exported for the tests)

# Positions are about 0.2 and spacings about 0.02, so squared distances are about 4e-4: 1e-7 is far above the fp32 rounding of a
# squared distance (4 x 2^-24 x 4e-4 = 1e-10) and above the fp32-vs-float64 drift of a predicted state (1e-6 x 0.02 x 2 = 4e-8)
MARGIN_MIN = 1e-7
JITTER = 1e-3
BATCH_KEYS = ('states', 'states_delta', 'attrs', 'particle_nums', 'particle_dens')


# ---- the metric ---------------------------------------------------------------------------------------------------------
def _nearest(a, b):
    """rows of a [n, 3] against rows of b [m, 3] (float64) -> (argmin [n], best squared distance [n], margin [n])"""
    d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    arg = np.argmin(d, axis=1)                                  # first occurrence: the lowest index on a tie
    best = d[np.arange(len(a)), arg]
    if b.shape[0] > 1:
        d2 = d.copy()
        d2[np.arange(len(a)), arg] = np.inf
        margin = d2.min(axis=1) - best
    else:
        margin = np.full(len(a), np.inf)
    return arg, best, margin


def chamfer64(p, q, n_p, n_q):
    """p [B, N, 3], q [B, M, 3] (any float dtype, widened), counts [B] -> dict of float64 / int arrays: fwd, bwd [B]; grad
    [B, N, 3] = d (fwd + bwd) / d p (0 on padding); nn_pq [B, N], nn_qp [B, M] (-1 on padding); margin_pq [B, N], margin_qp [B, M]
    (inf on padding and where the other cloud has one row)"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    B, N, _ = p.shape
    M = q.shape[1]
    out = {'fwd': np.zeros(B), 'bwd': np.zeros(B), 'grad': np.zeros((B, N, 3)), 'nn_pq': -np.ones((B, N), np.int64),
           'nn_qp': -np.ones((B, M), np.int64), 'margin_pq': np.full((B, N), np.inf), 'margin_qp': np.full((B, M), np.inf)}
    for b in range(B):
        n, m = int(n_p[b]), int(n_q[b])
        pb, qb = p[b, :n], q[b, :m]
        a, da, ma = _nearest(pb, qb)
        c, dc, mc = _nearest(qb, pb)
        out['fwd'][b] = da.sum() / (3 * n)
        out['bwd'][b] = dc.sum() / (3 * m)
        g = 2.0 / (3 * n) * (pb - qb[a])
        for j in range(m):                                      # ascending j, as the kernel's gather
            g[c[j]] += 2.0 / (3 * m) * (pb[c[j]] - qb[j])
        out['grad'][b, :n] = g
        out['nn_pq'][b, :n], out['nn_qp'][b, :m] = a, c
        out['margin_pq'][b, :n], out['margin_qp'][b, :m] = ma, mc
    return out


def min_margin(ref):
    return float(min(ref['margin_pq'].min(), ref['margin_qp'].min()))


# ---- the batches of tests/test_gpu_chamfer.py -----------------------------------------------------------------------------
# (n_p, n_q in N, M); the kernel has ONE path (the other cloud tiled through LDS, 1024 points a tile), so no threshold shapes
CHAMFER_SHAPES = [(1, 1, 1, 1), (5, 3, 8, 8), (3, 5, 8, 8), (70, 130, 70, 130), (300, 257, 300, 300), (64, 64, 64, 64),
                  (1, 300, 4, 300)]


# the seed of a case where seed 0 leaves an arg-min margin too close to MARGIN_MIN (several hundred arg-mins over random
# clouds: the smallest margin is a fraction of a thousandth of a squared spacing); tests/test_untracked_host.py holds the rest
CHAMFER_SEED = {((70, 130, 70, 130), 3): 2, ((300, 257, 300, 300), 1): 1, ((300, 257, 300, 300), 3): 2, ((64, 64, 64, 64), 1): 2}


def chamfer_case(shape, B, seed=None):
    """-> (p [B, N, 3], q [B, M, 3] float32, n_p, n_q [B] int32): clouds of the piles' scale (positions ~0.2, spacing ~0.02; the
    padding holds rubbish, which nothing may read as a point); at B = 3 the three samples have three different counts (sample 0
    the shape's own, then each count reduced, at least 1)"""
    n_p, n_q, N, M = shape
    if seed is None:
        seed = CHAMFER_SEED.get((tuple(shape), B), 0)
    rng = np.random.default_rng(1000 * seed + 7 * n_p + 13 * n_q + B)
    p = (5.0 + rng.standard_normal((B, N, 3))).astype(np.float32)        # rubbish in the padding
    q = (-5.0 + rng.standard_normal((B, M, 3))).astype(np.float32)
    nps = np.array([max(1, n_p - (b * (n_p // 3 + 1))) for b in range(B)], np.int32)
    nqs = np.array([max(1, n_q - (b * (n_q // 4 + 1))) for b in range(B)], np.int32)
    for b in range(B):
        side = 0.02 * max(nps[b], nqs[b]) ** (1.0 / 3.0)
        p[b, :nps[b]] = (0.2 + side * rng.random((nps[b], 3))).astype(np.float32)
        q[b, :nqs[b]] = (0.2 + side * rng.random((nqs[b], 3))).astype(np.float32)
    return p, q, nps, nqs


def chamfer_cases():
    return [(shape, B) for shape in CHAMFER_SHAPES for B in (1, 3)]


# ---- the trainer --------------------------------------------------------------------------------------------------------
def make_targets(states, particle_nums, seed=0):
    """states [B, H+1, N, 3] (collated, tracked) -> (targets [B, H, M, 3] float32 zero-padded, target_nums [B, H] int32): target t
    of sample b is drop_correspondence's subset of states[b, t+1, :n_b] in random order, each coordinate moved by JITTER x a
    standard normal draw"""
    from dyn_res_pile_manip_amd.dataset_gnn_dyn import drop_correspondence
    states = np.asarray(states, np.float32)
    B, T1, N, _ = states.shape
    H = T1 - 1
    rng = np.random.default_rng(77000 + seed)
    per = []
    for b in range(B):
        n = int(particle_nums[b])
        sample = (states[b, :, :n], np.zeros((H, n, 3), np.float32), np.zeros((T1, n), np.float32), n, 1.0, None)
        tg = drop_correspondence(sample, rng)[6]
        per.append([(t + JITTER * rng.standard_normal(t.shape)).astype(np.float32) for t in tg])
    M = max(t.shape[0] for tg in per for t in tg)
    targets = np.zeros((B, H, M, 3), np.float32)
    tnums = np.zeros((B, H), np.int32)
    for b, tg in enumerate(per):
        for t, cloud in enumerate(tg):
            targets[b, t, :cloud.shape[0]] = cloud
            tnums[b, t] = cloud.shape[0]
    return targets, tnums


def train_untracked64(W, states, states_delta, attrs, particle_nums, particle_dens, targets, target_nums, adj_thresh=0.08,
                      want_graphs=False, keep64=False, nudge=None):
    """tests/_f64_train_ref.py's train_loss_and_grads64 with the term of (step t, sample b) replaced by
    (fwd + bwd)(s_pred[b, :n_b], targets[b, t, :m_bt]) / (n_rollout B), the arg-mins taken from the detached double prediction
    -> (loss, terms [H, B], {key: gradient}, d loss / d every step's predicted state [B, H, N, 3], info) with info = {'margin': the
    smallest arg-min margin of all steps and samples, 'nn': [(a, c) per (t, b)], 'graphs': per-step adjacency (want_graphs)}.
    nudge = (t, b, i, k, h): h is added to coordinate k of row i of sample b's prediction of step t (central differences of the
    state gradient)."""
    if keep64:
        W = dict((k, torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float64)))) for k, v in W.items())
    else:
        W = weights64(W)
    W = dict((k, v.clone().requires_grad_(True)) for k, v in W.items())
    st, sd, at, dens = _d(states), _d(states_delta), _d(attrs), _d(particle_dens)
    tg = _d(targets)
    nums = [int(n) for n in np.asarray(particle_nums)]
    tnums = np.asarray(target_nums)
    B, T1, N, _ = st.shape
    H = T1 - 1
    s_cur, a_cur = st[:, 0], at[:, 0]
    terms, preds, graphs, nn = [], [], [], []
    margin = np.inf
    for t in range(H):
        adj, _ = adjacency(s_cur.detach().float(), sd[:, t].float(), adj_thresh)
        s_pred = step(W, a_cur, s_cur, sd[:, t], dens, adj.double())
        if nudge is not None and nudge[0] == t:
            bump = torch.zeros_like(s_pred)
            bump[nudge[1], nudge[2], nudge[3]] = nudge[4]
            s_pred = s_pred + bump
        s_pred.retain_grad()
        preds.append(s_pred)
        graphs.append(adj.bool().numpy())
        row = []
        for b in range(B):
            n, m = nums[b], int(tnums[b, t])
            pb, qb = s_pred[b, :n], tg[b, t, :m]
            a, _, ma = _nearest(pb.detach().numpy(), qb.numpy())
            c, _, mc = _nearest(qb.numpy(), pb.detach().numpy())
            margin = min(margin, float(ma.min()), float(mc.min()))
            nn.append((a, c))
            fwd = ((pb - qb[torch.from_numpy(a)]) ** 2).mean()
            bwd = ((qb - pb[torch.from_numpy(c)]) ** 2).mean()
            row.append((fwd + bwd) / (H * B))
        terms.append(torch.stack(row))
        s_cur = s_pred
    terms = torch.stack(terms)
    loss = terms.sum()
    loss.backward()
    grads = dict((k, W[k].grad.numpy().copy()) for k in PARAMS)
    g_state = np.stack([p.grad.numpy() if p.grad is not None else np.zeros((B, N, 3)) for p in preds], 1)
    info = {'margin': margin, 'nn': nn}
    if want_graphs:
        info['graphs'] = graphs
    return float(loss.item()), terms.detach().numpy(), grads, g_state, info


def weights_of(golden, wset):
    return golden.weights_seed0 if wset == 'seed0' else golden.weights_trained


def fixture_batch(golden, name):
    return [golden.train[name + '/' + k] for k in BATCH_KEYS]


TRAIN_CASES = [(b, w) for b in ('b4_r3', 'b2_r5') for w in ('seed0', 'trained')]
TARGET_SEED = {'b4_r3': 19, 'b2_r5': 0}        # tests/test_untracked_host.py holds every margin these give above MARGIN_MIN


def untracked_batch(golden, name):
    """the fixture batch `name` and its untracked targets -> the seven arrays of train_step_untracked"""
    batch = fixture_batch(golden, name)
    return batch + list(make_targets(batch[0], batch[3], TARGET_SEED[name]))


def single_point_batch(golden):
    """the hand-checkable configuration: b4_r3 with ONE target point per (sample, step), M = 1 -- fwd is the mean squared distance
    of the prediction to that point, bwd the squared distance of the point to its single nearest row c"""
    batch = fixture_batch(golden, 'b4_r3')
    st, nums = batch[0], batch[3]
    B, T1 = st.shape[:2]
    targets = np.zeros((B, T1 - 1, 1, 3), np.float32)
    for b in range(B):
        for t in range(T1 - 1):
            targets[b, t, 0] = st[b, t + 1, :nums[b]].mean(0) + np.float32(0.003) * np.array([1, -2, 0.5], np.float32)
    return batch + [targets, np.ones((B, T1 - 1), np.int32)]


def tiny_batch():
    """B = 1, N = n = 5, M = 3, H = 1, unpadded on both sides"""
    from dyn_res_pile_manip_amd import synthetic as syn
    rng = np.random.default_rng(3)
    s, _, _ = syn.make_pile(5, 1, seed=11, kind='blob')
    states = np.zeros((1, 2, 5, 3), np.float32)
    states[0, 0] = s[0] * 0.3 + [0, 0, 0.52]
    states[0, 1] = states[0, 0] + 0.002 * rng.standard_normal((5, 3)).astype(np.float32)
    sdelta = (0.004 * rng.standard_normal((1, 1, 5, 3))).astype(np.float32)
    targets = (states[0, 1][[3, 0, 4]] + JITTER * rng.standard_normal((3, 3))).astype(np.float32)[None, None]
    return [states, sdelta, np.zeros((1, 2, 5), np.float32), np.array([5], np.int32), np.array([300.0], np.float32), targets,
            np.array([[3]], np.int32)]


_cache = {}


def reference(golden, name, wset):
    """train_untracked64 of a fixture case, computed once and left unchanged: (loss, terms, gradient blob, g_state on real rows,
    info)"""
    if (name, wset) not in _cache:
        batch = untracked_batch(golden, name)
        loss, terms, grads, gs, info = train_untracked64(weights_of(golden, wset), *batch)
        out = (loss, terms, blob64(grads), real_rows(gs, batch[3]), info)
        for v in out[1:4]:
            v.setflags(write=False)
        _cache[(name, wset)] = out
    return _cache[(name, wset)]


def adam_trajectory64(golden, name, lr, beta1, steps=3):
    """`steps` Adam steps (torch.optim.Adam's update, eps = 1e-8, beta2 = 0.999) in numpy float64 on train_untracked64's gradients,
    from the seed-0 weights -> (losses before each update, the blob after the last, the first step's gradient blob, the smallest
    arg-min margin on the way)"""
    key = ('adam', name, float(lr), float(beta1), steps)
    if key not in _cache:
        batch = untracked_batch(golden, name)
        W = dict((k, v.numpy().copy()) for k, v in weights64(golden.weights_seed0).items())
        m = dict((k, np.zeros_like(W[k])) for k in PARAMS)
        v = dict((k, np.zeros_like(W[k])) for k in PARAMS)
        losses, margin, g0 = [], np.inf, None
        for it in range(1, steps + 1):
            loss, _, grads, _, info = train_untracked64(W, *batch, keep64=True)
            losses.append(loss)
            margin = min(margin, info['margin'])
            if g0 is None:
                g0 = blob64(grads)
            for k in PARAMS:
                m[k] = beta1 * m[k] + (1 - beta1) * grads[k]
                v[k] = 0.999 * v[k] + 0.001 * grads[k] ** 2
                W[k] = W[k] - lr * (m[k] / (1 - beta1 ** it)) / (np.sqrt(v[k] / (1 - 0.999 ** it)) + 1e-8)
        _cache[key] = (losses, blob64(W), g0, margin)
    return _cache[key]
