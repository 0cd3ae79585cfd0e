"""TEST INFRASTRUCTURE of the one-to-one matching loss (drp_cloud_match, drp_train_step_loss; csrc/k_match.h): a self-contained
oracle -- the GPU machine may lack scipy.

  cost32(p, q)                     the kernel's fp32 cost matrix, bit for bit: fp32 differences, dx*dx + dy*dy + dz*dz in that order
  assign64(C)                      the rectangular linear assignment problem in numpy float64, O(n^3) shortest augmenting paths
                                   (rows inserted in ascending index, the lowest column among equal shortest reduced costs) ->
                                   the matching, its cost and its UNIQUENESS MARGIN: second-best minus best total cost, found by
                                   re-solving with each chosen pair forbidden in turn
  match64(p, q, n_p, n_q)          term, gradient and partners of a padded batch
  train_match64(W, ...)            tests/_untracked_ref.py's train_untracked64 loop (or tests/_train_actions_ref.py's, with
                                   actions=) with the term replaced

The margin.  The optimum of the cost matrix in double is computed with one rounding per dual update and inserted row, each of a
quantity below max C: r 2^-52 max C, about 1e-14 at these sizes (r <= 300, C <= 1e-2).  MARGIN_MIN = 1e-9 is 10^5 times that:
where the second-best matching is further than that, every exact solver returns the same partners.
"""
import numpy as np
import torch

import _untracked_ref as U
from _untracked_ref import PARAMS, blob64, real_rows  # noqa: F401  (re-exported for the tests)

MARGIN_MIN = 1e-9
# the fp32-vs-float64 drift of a squared distance of a predicted state (tests/_untracked_ref.py derives it: 1e-6 x 0.02 x 2)
DRIFT = 4e-8
LOSSES = ('match', 'chamfer+match')


# ---- the cost matrix ------------------------------------------------------------------------------------------------------
def cost32(p, q):
    """p [n, 3], q [m, 3] -> float32 [n, m]: |p_i - q_j|^2 with the kernel's operations (numpy rounds every float32 operation and
    fuses none)"""
    p, q = np.asarray(p, np.float32), np.asarray(q, np.float32)
    dx = p[:, None, 0] - q[None, :, 0]
    dy = p[:, None, 1] - q[None, :, 1]
    dz = p[:, None, 2] - q[None, :, 2]
    c = dx * dx + dy * dy + dz * dz
    assert c.dtype == np.float32
    return c


def cost64(p, q):
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    d = p[:, None, :] - q[None, :, :]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


# ---- the solver -----------------------------------------------------------------------------------------------------------
def _insert_row(C, u, v, col4row, row4col, i):
    """one augmentation: the shortest path over reduced costs from row i to a free column, the dual update, the flip; False
    where no free column can be reached at a finite cost"""
    c = C.shape[1]
    sh = np.full(c, np.inf)
    pred = np.full(c, i, np.int64)
    scanned = np.zeros(c, bool)
    cur, minval, sink = i, 0.0, -1
    for _ in range(c):
        free = ~scanned
        d = minval + C[cur] - u[cur] - v
        better = free & (d < sh)
        sh[better] = d[better]
        pred[better] = cur
        cand = np.where(free, sh, np.inf)
        j = int(np.argmin(cand))                                # the first occurrence: the lowest index among equals
        if not np.isfinite(cand[j]):
            return False
        minval = cand[j]
        scanned[j] = True
        if row4col[j] < 0:
            sink = j
            break
        cur = int(row4col[j])
    assert sink >= 0
    delta = minval - sh
    taken = scanned & (row4col >= 0)
    u[row4col[taken]] += delta[taken]
    u[i] += minval
    v[scanned] -= delta[scanned]
    j = sink
    while True:
        i2 = int(pred[j])
        row4col[j] = i2
        col4row[i2], j = j, col4row[i2]
        if i2 == i:
            break
    return True


def _solve(C):
    r, c = C.shape
    assert r <= c
    u, v = np.zeros(r), np.zeros(c)
    col4row, row4col = -np.ones(r, np.int64), -np.ones(c, np.int64)
    for i in range(r):
        ok = _insert_row(C, u, v, col4row, row4col, i)
        assert ok
    return u, v, col4row, row4col


def assign64(C, want_margin=True):
    """C [r, c] with r <= c (any float dtype, widened exactly) -> (col [r]: the column of every row, cost = sum C[i, col[i]],
    margin, (u [r], v [c]) the duals).  margin: the least cost of a matching that differs in at least one pair, minus cost; inf
    where there is no other matching (None unless want_margin).  It is found on the problem padded to a square with rows of zero
    cost, where every column is taken: there, freeing one chosen pair at an infinite cost leaves an optimal partial matching
    with feasible duals, and one more augmentation is its re-solve."""
    C = np.ascontiguousarray(np.asarray(C, np.float64))
    r, c = C.shape
    u, v, col, _ = _solve(C)
    cost = float(C[np.arange(r), col].sum())
    margin = None
    if want_margin:
        S = np.vstack([C, np.zeros((c - r, c))])
        su, sv, scol, srow = _solve(S)
        base = float(S[np.arange(c), scol].sum())
        margin = np.inf
        for i in range(r):
            S2, u2, v2, col2, row2 = S.copy(), su.copy(), sv.copy(), scol.copy(), srow.copy()
            j = int(col2[i])
            S2[i, j] = np.inf
            col2[i], row2[j] = -1, -1                           # (the duals stay feasible: one cost went up)
            if _insert_row(S2, u2, v2, col2, row2, i):
                margin = min(margin, float(S2[np.arange(c), col2].sum()) - base)
    return col, cost, margin, (u, v)


def brute_force(C):
    """the least cost over ALL injections of the rows into the columns (tiny problems)"""
    from itertools import permutations
    C = np.asarray(C, np.float64)
    r, c = C.shape
    return min(float(C[np.arange(r), list(perm)].sum()) for perm in permutations(range(c), r))


# ---- the metric -----------------------------------------------------------------------------------------------------------
def solve_pair(C, want_margin=True):
    """C [n_p, n_q] -> (partner of every row of p [n_p], of q [n_q] (-1: unmatched), cost, margin, u [n_p], v [n_q]): the rows
    of the solver are the smaller cloud's, p's where the counts are equal"""
    n, m = C.shape
    if n <= m:
        col, cost, margin, (u, v) = assign64(C, want_margin)
        pq, qp = col.copy(), -np.ones(m, np.int64)
        qp[col] = np.arange(n)
        return pq, qp, cost, margin, u, v
    col, cost, margin, (u, v) = assign64(np.ascontiguousarray(np.asarray(C).T), want_margin)
    qp, pq = col.copy(), -np.ones(n, np.int64)
    pq[col] = np.arange(m)
    return pq, qp, cost, margin, v, u


def term_and_grad(pb, qb, pq, diff32=False):
    """[n, 3], [m, 3] and p's partners -> (sum over the pairs / (3 r), d / d p [n, 3]) in float64 on the inputs widened.
    diff32: the term takes the float32 differences of the inputs as float32, widened, as the kernel does (squares and sums in
    double); the gradient is float64 throughout either way."""
    on = pq >= 0
    r = int(on.sum())
    p64, q64 = np.asarray(pb, np.float64), np.asarray(qb, np.float64)
    diff = np.zeros_like(p64)
    diff[on] = p64[on] - q64[pq[on]]
    if diff32:
        d32 = (np.asarray(pb, np.float32)[on] - np.asarray(qb, np.float32)[pq[on]]).astype(np.float64)
        term = float((d32 * d32).sum() / (3 * r))
    else:
        term = float((diff ** 2).sum() / (3 * r))
    return term, 2.0 * diff / (3 * r)


def match64(p, q, n_p, n_q, matches=None, exact32=True, want_margin=True):
    """p [B, N, 3], q [B, M, 3], counts [B] -> dict: match [B], cost [B] (sum of the cost matrix over the pairs), margin [B], grad
    [B, N, 3] float64 (0 on unmatched rows and padding), match_pq [B, N], match_qp [B, M] (-1: unmatched, padding), u [B, N],
    v [B, M].  exact32: the matching is solved on cost32 of the inputs as float32 and the term sums the squares of their float32
    differences in double, both as the kernel; otherwise float64 squared distances and differences.  The gradient is float64.  matches [B, N]: take these partners instead of solving.  The margin
    costs a second solve on the problem padded to a square: want_margin=False leaves it inf."""
    B, N, _ = np.shape(p)
    M = np.shape(q)[1]
    p64, q64 = np.asarray(p, np.float64), np.asarray(q, np.float64)
    out = {'match': np.zeros(B), 'cost': np.zeros(B), 'margin': np.full(B, np.inf), 'grad': np.zeros((B, N, 3)),
           'match_pq': -np.ones((B, N), np.int64), 'match_qp': -np.ones((B, M), np.int64), 'u': np.zeros((B, N)), 'v': np.zeros((B, M))}
    for b in range(B):
        n, m = int(n_p[b]), int(n_q[b])
        C = cost32(p[b, :n], q[b, :m]) if exact32 else cost64(p64[b, :n], q64[b, :m])
        if matches is None:
            pq, qp, cost, margin, u, v = solve_pair(C, want_margin)
            out['margin'][b], out['u'][b, :n], out['v'][b, :m] = (margin if want_margin else np.inf), u, v
        else:
            pq = np.asarray(matches[b][:n], np.int64)
            qp = -np.ones(m, np.int64)
            qp[pq[pq >= 0]] = np.nonzero(pq >= 0)[0]
            cost = float(np.asarray(C, np.float64)[np.nonzero(pq >= 0)[0], pq[pq >= 0]].sum())
        out['cost'][b] = cost
        out['match'][b], out['grad'][b, :n] = term_and_grad(p[b][:n], q[b][:m], pq, diff32=exact32)
        out['match_pq'][b, :n], out['match_qp'][b, :m] = pq, qp
    return out


# ---- the batches of tests/test_gpu_match.py ---------------------------------------------------------------------------------
# beyond tests/_untracked_ref.py's chamfer_cases(): the cap, one column past a lane stripe (64 columns a stripe), a few rows
# against nearly the cap.  (n_p, n_q, N, M), B = 1
EXTRA_SHAPES = [(1024, 1024, 1024, 1024), (1024, 1, 1024, 4), (65, 64, 65, 64), (64, 65, 64, 65), (17, 1023, 20, 1023)]


# ---- the trainer --------------------------------------------------------------------------------------------------------
def train_match64(W, states, states_delta, attrs, particle_nums, particle_dens, targets, target_nums, matches=None, kind='match',
                  weight=0.5, actions=None, adj_thresh=0.08, keep64=False):
    """tests/_untracked_ref.py's train_untracked64 loop (actions [B, H, 4] given: tests/_train_actions_ref.py's impulses in place
    of states_delta) with the term of (step t, sample b) replaced by match / (n_rollout B) (kind 'match') or
    ((1 - weight) (fwd + bwd) + weight match) / (n_rollout B) (kind 'chamfer+match'); the Chamfer arg-mins from the detached double
    prediction.  matches [H, B, N] (every predicted row's partner): the matching is the caller's; None: solved on the double
    prediction -> (loss, terms [H, B], {key: gradient}, d loss / d predicted states [B, H, N, 3], info) with info = {'match'
    [H, B, N]: the matching used, 'cost' [H, B]: its cost on the double prediction, 'opt_cost' [H, B]: the optimum's there, 'r'
    [H, B], 'margin': the smallest uniqueness margin of those optima, 'chamfer_margin'}"""
    from oracle.propnet_dense import adjacency
    from _f64_grad_ref import _d, step, weights64
    assert kind in LOSSES
    if keep64:
        W = dict((k, torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float64)))) for k, v in W.items())
    else:
        W = weights64(W)
    W = dict((k, v.clone().requires_grad_(True)) for k, v in W.items())
    st, at, dens = _d(states), _d(attrs), _d(particle_dens)
    if actions is None:
        sd_all = _d(states_delta)
    else:
        import _train_actions_ref as A
        ac = _d(actions)
    tg = _d(targets)
    nums = [int(n) for n in np.asarray(particle_nums)]
    tnums = np.asarray(target_nums)
    B, T1, N, _ = st.shape
    H = T1 - 1
    s_cur, a_cur = st[:, 0], at[:, 0]
    terms, preds = [], []
    used = -np.ones((H, B, N), np.int64)
    cost, opt_cost, rr = np.zeros((H, B)), np.zeros((H, B)), np.zeros((H, B), np.int64)
    margin, cmargin = np.inf, np.inf
    for t in range(H):
        sd = sd_all[:, t] if actions is None else A.impulses64(s_cur, ac[:, t], nums)
        adj, _ = adjacency(s_cur.detach().float(), sd.detach().float(), adj_thresh)
        s_pred = step(W, a_cur, s_cur, sd, dens, adj.double())
        s_pred.retain_grad()
        preds.append(s_pred)
        row = []
        for b in range(B):
            n, m = nums[b], int(tnums[b, t])
            pb, qb = s_pred[b, :n], tg[b, t, :m]
            C = cost64(pb.detach().numpy(), qb.numpy())
            pq, _, oc, mar, _, _ = solve_pair(C)
            margin = min(margin, mar)
            opt_cost[t, b] = oc
            if matches is not None:
                pq = np.asarray(matches[t][b][:n], np.int64)
            on = np.nonzero(pq >= 0)[0]
            r = min(n, m)
            assert len(on) == r and len(set(pq[on].tolist())) == r and pq[on].max() < m
            used[t, b, :n], rr[t, b] = pq, r
            cost[t, b] = float(C[on, pq[on]].sum())
            term = ((pb[torch.from_numpy(on)] - qb[torch.from_numpy(pq[on])]) ** 2).sum() / (3 * r)
            if kind == 'chamfer+match':
                a, _, ma = U._nearest(pb.detach().numpy(), qb.numpy())
                c, _, mc = U._nearest(qb.numpy(), pb.detach().numpy())
                cmargin = min(cmargin, float(ma.min()), float(mc.min()))
                cham = ((pb - qb[torch.from_numpy(a)]) ** 2).mean() + ((qb - pb[torch.from_numpy(c)]) ** 2).mean()
                term = (1.0 - weight) * cham + weight * term
            row.append(term / (H * B))
        terms.append(torch.stack(row))
        s_cur = s_pred
    terms = torch.stack(terms)
    loss = terms.sum()
    loss.backward()
    grads = dict((k, W[k].grad.numpy().copy()) for k in PARAMS)
    g_state = np.stack([p.grad.numpy() if p.grad is not None else np.zeros((B, N, 3)) for p in preds], 1)
    info = {'match': used, 'cost': cost, 'opt_cost': opt_cost, 'r': rr, 'margin': margin, 'chamfer_margin': cmargin}
    return float(loss.item()), terms.detach().numpy(), grads, g_state, info


_cache = {}


def adam_trajectory64(golden, name, lr, beta1, kind='match', weight=0.5, steps=3):
    """tests/_untracked_ref.py's adam_trajectory64 on train_match64's gradients (the matching solved on the double prediction),
    from the seed-0 weights -> (losses before each update, the blob after the last, the first step's gradient blob, the smallest
    uniqueness margin on the way)"""
    from _f64_grad_ref import weights64
    key = ('adam', name, float(lr), float(beta1), kind, float(weight), steps)
    if key not in _cache:
        batch = U.untracked_batch(golden, name)
        W = dict((k, v.numpy().copy()) for k, v in weights64(golden.weights_seed0).items())
        m = dict((k, np.zeros_like(W[k])) for k in PARAMS)
        v = dict((k, np.zeros_like(W[k])) for k in PARAMS)
        losses, margin, g0 = [], np.inf, None
        for it in range(1, steps + 1):
            loss, _, grads, _, info = train_match64(W, *batch, kind=kind, weight=weight, keep64=True)
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


def dense_targets(states, particle_nums, seed=0):
    """targets with MORE rows than the prediction (the other orientation of the matching: every predicted row gets a partner):
    target t of sample b is states[b, t + 1, :n_b] and a second copy of its first n_b // 2 rows, every coordinate moved by JITTER
    x a standard normal draw, in random order -> (targets [B, H, M, 3] float32 zero-padded, target_nums [B, H] int32)"""
    states = np.asarray(states, np.float32)
    B, T1, N, _ = states.shape
    H = T1 - 1
    rng = np.random.default_rng(88000 + seed)
    nums = [int(n) for n in particle_nums]
    M = max(n + n // 2 for n in nums)
    targets = np.zeros((B, H, M, 3), np.float32)
    tnums = np.zeros((B, H), np.int32)
    for b, n in enumerate(nums):
        for t in range(H):
            cloud = np.concatenate([states[b, t + 1, :n], states[b, t + 1, :n // 2]], 0)
            cloud = (cloud + U.JITTER * rng.standard_normal(cloud.shape))[rng.permutation(len(cloud))]
            targets[b, t, :len(cloud)] = cloud.astype(np.float32)
            tnums[b, t] = len(cloud)
    return targets, tnums
