"""TEST INFRASTRUCTURE of the float64 yardstick of the Sinkhorn divergence (drp_cloud_divergence_f64,
drp_train_grad_f64_divergence; csrc/k_sinkhorn.h): tests/_divergence_ref.py's definition with nothing in fp32 -- its
pair64(None, q, eps, K, p64=p) path, the one its own central differences use: costs and differences in float64 from the float64
prediction and the float32 targets widened.

  divergence64_wide(p, q, n_p, n_q, eps, K)    a padded batch, p float64
  train_sinkhorn64(...)                        _divergence_ref.train_divergence64's loop with the plans of step t computed from the
                                               float64 prediction of step t itself (detached: constants of the derivative)
  train_case(...), reference(...)              the cases of tests/test_gpu_train_f64_divergence.py, each reference computed once

The device adds the same terms in another fixed order; every other operation is the same IEEE double operation in
the same order, and exp and log are each library's own."""
import numpy as np

import _divergence_ref as D
import _transport_ref as T


def divergence64_wide(p, q, n_p, n_q, eps, K, scale=1.0):
    """p [B, N, 3] float64, q [B, M, 3] float32 with n_p, n_q real rows, eps a number or [B] -> _divergence_ref.divergence64's
    dict, every entry float64"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float32)
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    eps = np.broadcast_to(np.asarray(eps, np.float64).reshape(-1), (B,))
    out = {'divergence': np.zeros(B), 'grad': np.zeros((B, N, 3)), 'f': np.zeros((B, N)), 'g': np.zeros((B, M)),
           'h_p': np.zeros((B, N)), 'h_q': np.zeros((B, M)), 'col_err': np.zeros(B), 'self_err': np.zeros((B, 2))}
    for b in range(B):
        n, m = int(n_p[b]), int(n_q[b])
        value, grad, f, g, h_p, h_q, ce, se = D.pair64(None, q[b, :m], float(eps[b]), K, scale, p64=p[b, :n])
        out['divergence'][b], out['col_err'][b], out['self_err'][b] = value, ce, se
        out['grad'][b, :n], out['f'][b, :n], out['g'][b, :m], out['h_p'][b, :n], out['h_q'][b, :m] = grad, f, g, h_p, h_q
    return out


def train_sinkhorn64(W, states, states_delta, attrs, particle_nums, particle_dens, targets, target_nums, eps, K, actions=None,
                     adj_thresh=0.08, see=None):
    """_divergence_ref.train_divergence64 with plans[t][b] = pair64(None, q, eps_b, K, p64 = the detached float64 prediction of
    (step t, sample b))'s (P, S_p, value) -> (loss, terms [H, B], {key: gradient}, d loss / d predicted states [B, H, N, 3], info)
    with info = {'plans': [t][b] -> (P, S_p, value), 'col_err' [H, B], 'self_err' [H, B, 2]}.  see(t, b, x [n, 3], cur [n, 3]) ->
    [n, 3] (optional, float64): what the loss is SHOWN in place of the prediction x when its plans and its value are formed (cur:
    the state the step read) -- the reverse pass still starts at x (a drift of the states the loss sees, or a nudge for central
    differences of the reported loss)"""
    import torch
    from oracle.propnet_dense import adjacency
    from _f64_grad_ref import _d, step, weights64
    from _f64_train_ref import PARAMS
    W = dict((k, v.clone().requires_grad_(True)) for k, v in weights64(W).items())
    st, at, dens = _d(states), _d(attrs), _d(particle_dens)
    if actions is None:
        sd_all = _d(states_delta)
    else:
        import _train_actions_ref as A
        ac = _d(actions)
    tg = _d(targets)
    q32 = np.asarray(targets, np.float32)
    nums = [int(n) for n in np.asarray(particle_nums)]
    tnums = np.asarray(target_nums)
    B, T1, N, _ = st.shape
    H = T1 - 1
    eps = np.broadcast_to(np.asarray(eps, np.float64).reshape(-1), (B,))
    s_cur, a_cur = st[:, 0], at[:, 0]
    terms, preds, plans = [], [], []
    col_err, self_err = np.zeros((H, B)), np.zeros((H, B, 2))
    for t in range(H):
        sd = sd_all[:, t] if actions is None else A.impulses64(s_cur, ac[:, t], nums)
        adj, _ = adjacency(s_cur.detach().float(), sd.detach().float(), adj_thresh)
        s_pred = step(W, a_cur, s_cur, sd, dens, adj.double())
        s_pred.retain_grad()
        preds.append(s_pred)
        row, prow = [], []
        for b in range(B):
            n, m = nums[b], int(tnums[b, t])
            x = s_pred[b, :n].detach().numpy().copy()
            if see is not None:
                x = np.asarray(see(t, b, x, s_cur[b, :n].detach().numpy().copy()), np.float64)
            out = D.pair64(None, q32[b, t, :m], float(eps[b]), K, p64=x, want_plans=True)
            P, S, value = out[8], out[9], out[0]
            col_err[t, b], self_err[t, b] = out[6], out[7]
            prow.append((P, S, value))
            d = s_pred[b, :n, None, :] - tg[b, t, None, :m, :]
            dd = s_pred[b, :n, None, :] - s_pred[b, None, :n, :]
            sur = ((torch.from_numpy(P) * (d ** 2).sum(-1)).sum() - 0.5 * (torch.from_numpy(S) * (dd ** 2).sum(-1)).sum()) / 3.0
            row.append((sur - sur.detach() + float(value)) / (H * B))
        plans.append(prow)
        terms.append(torch.stack(row))
        s_cur = s_pred
    terms = torch.stack(terms)
    loss = terms.sum()
    loss.backward()
    grads = dict((k, W[k].grad.numpy().copy()) for k in PARAMS)
    g_state = np.stack([p.grad.numpy() if p.grad is not None else np.zeros((B, N, 3)) for p in preds], 1)
    return float(loss.item()), terms.detach().numpy(), grads, g_state, {'plans': plans, 'col_err': col_err, 'self_err': self_err}


# ---- the cases of the device tests -----------------------------------------------------------------------------------------------
K = 50
EPS_SCALES = (1.0, 0.25)


def eps_of(dens, scale=1.0):
    return float(scale) / np.asarray(dens, np.float64).reshape(-1)


def train_case(impulses, scale=1.0):
    """_transport_ref.train_batch() (2 x 2 x 9, M = 12, ragged counts on both sides) -> the keyword arguments of
    Engine.train_grad_f64_divergence"""
    st, sd, ac, at, nums, dens, tg, tn = T.train_batch()
    kw = dict(states=st, states_delta=sd if impulses == 'data' else None, attrs=at, particle_nums=nums, particle_dens=dens,
              targets=tg, target_nums=tn, eps=eps_of(dens, scale), iters=K)
    if impulses == 'actions':
        kw['actions'] = ac
    return kw


def tiny_case():
    """B = 1, H = 1, 5 particles, 3 targets, unpadded (_untracked_ref.tiny_batch)"""
    import _untracked_ref as U
    st, sd, at, nums, dens, tg, tn = U.tiny_batch()
    return dict(states=st, states_delta=sd, attrs=at, particle_nums=nums, particle_dens=dens, targets=tg, target_nums=tn,
                eps=eps_of(dens), iters=K)


def single_case():
    """train_batch() with its second sample cut to ONE particle and one target point at its first step (n_q = 1)"""
    kw = train_case('data')
    kw['particle_nums'] = np.array([kw['particle_nums'][0], 1], np.int32)
    kw['states'], kw['states_delta'] = kw['states'].copy(), kw['states_delta'].copy()
    kw['states'][1, :, 1:] = 0.0                        # collate_fn's padding: zero rows
    kw['states_delta'][1, :, 1:] = 0.0
    tn = kw['target_nums'].copy()
    tn[0, 0] = 1
    kw['target_nums'] = tn
    return kw


def host_reference(w, kw):
    """-> (loss, terms, gradient blob, g_state [B, H, N, 3], col_err, self_err) of train_sinkhorn64, read-only"""
    import _untracked_ref as U
    loss, terms, grads, gs, info = train_sinkhorn64(w, kw['states'], kw['states_delta'], kw['attrs'], kw['particle_nums'],
                                                    kw['particle_dens'], kw['targets'], kw['target_nums'], kw['eps'], kw['iters'],
                                                    actions=kw.get('actions'))
    out = (loss, terms, np.asarray(U.blob64(grads), np.float64), gs, info['col_err'], info['self_err'])
    for v in out[1:]:
        v.setflags(write=False)
    return out


_cache = {}


def reference(golden, wset, impulses):
    """host_reference of train_case(impulses) on a weight set, computed once and left unchanged"""
    import _untracked_ref as U
    if (wset, impulses) not in _cache:
        _cache[(wset, impulses)] = host_reference(U.weights_of(golden, wset), train_case(impulses))
    return _cache[(wset, impulses)]
