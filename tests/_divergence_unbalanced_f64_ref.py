"""TEST INFRASTRUCTURE of the float64 yardstick of the unbalanced Sinkhorn divergence (drp_cloud_divergence_unbalanced_f64,
drp_train_grad_f64_divergence_unbalanced; csrc/k_sinkhorn.h: kd64_sweeps_unbalanced): tests/_divergence_unbalanced_ref.py's
definition with nothing in fp32 -- its pair64(None, q, eps, rho, w, K, p64=p) path: costs and differences in float64 from the
float64 prediction and the float32 targets widened.

  divergence64_wide(p64, q, n_p, n_q, eps, rho, w, K)   a padded batch, p float64
  train_sinkhorn64_unbalanced(...)                      _divergence_f64_ref.train_sinkhorn64's loop with that pair function and
                                                        per-problem rho[b], w[t, b]; the surrogate is unchanged (the cost enters
                                                        the relaxed problem through <P, C> alone); info also has 'transported'
  train_case(...), reference(...)                       the cases of tests/test_gpu_train_f64_divergence_unbalanced.py, each
                                                        reference computed once

rho = inf with w = 1 is the balanced code of tests/_divergence_f64_ref.py: the same bits."""
import numpy as np

import _divergence_f64_ref as R
import _divergence_unbalanced_ref as UB
import _transport_ref as T
from dyn_res_pile_manip_amd import train_gnn_dyn as TG

K = R.K
REACH_SCALE = 4.0                   # rho = 4 eps at eps scale 1: a reach of two particle spacings
MASSES = ('unit', 'count')


def divergence64_wide(p64, q, n_p, n_q, eps, rho, w, K, scale=1.0):
    """p64 [B, N, 3] float64, q [B, M, 3] float32 with n_p, n_q real rows; eps, rho, w numbers or [B] ->
    _divergence_unbalanced_ref.divergence64's dict, every entry float64"""
    p, q = np.asarray(p64, np.float64), np.asarray(q, np.float32)
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    eps, rho, w = (np.broadcast_to(np.asarray(v, np.float64).reshape(-1), (B,)) for v in (eps, rho, w))
    out = {'divergence': np.zeros(B), 'grad': np.zeros((B, N, 3)), 'f': np.zeros((B, N)), 'g': np.zeros((B, M)),
           'h_p': np.zeros((B, N)), 'h_q': np.zeros((B, M)), 'col_err': np.zeros(B), 'self_err': np.zeros((B, 2)),
           'transported': np.zeros(B)}
    for b in range(B):
        n, m = int(n_p[b]), int(n_q[b])
        value, grad, f, g, h_p, h_q, ce, se, tr = UB.pair64(None, q[b, :m], eps[b], rho[b], w[b], K, scale, p64=p[b, :n])
        out['divergence'][b], out['col_err'][b], out['self_err'][b], out['transported'][b] = value, ce, se, tr
        out['grad'][b, :n], out['f'][b, :n], out['g'][b, :m], out['h_p'][b, :n], out['h_q'][b, :m] = grad, f, g, h_p, h_q
    return out


def train_sinkhorn64_unbalanced(W, states, states_delta, attrs, particle_nums, particle_dens, targets, target_nums, eps, rho, w, K,
                                actions=None, adj_thresh=0.08, see=None):
    """_divergence_f64_ref.train_sinkhorn64 with plans[t][b] = _divergence_unbalanced_ref.pair64(None, q, eps_b, rho_b, w_tb, K,
    p64 = the detached float64 prediction)'s (P, S_p, value); rho a number or [B], w a number, [B] or [H, B] -> (loss, terms [H, B],
    {key: gradient}, d loss / d predicted states [B, H, N, 3], info) with info = {'plans', 'col_err' [H, B], 'self_err' [H, B, 2],
    'transported' [H, B]}.  see: train_sinkhorn64's hook"""
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
    rho = np.broadcast_to(np.asarray(rho, np.float64).reshape(-1), (B,))
    w = np.broadcast_to(np.asarray(w, np.float64), (H, B))
    s_cur, a_cur = st[:, 0], at[:, 0]
    terms, preds, plans = [], [], []
    col_err, self_err, moved = np.zeros((H, B)), np.zeros((H, B, 2)), np.zeros((H, B))
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
            out = UB.pair64(None, q32[b, t, :m], float(eps[b]), float(rho[b]), float(w[t, b]), K, p64=x, want_plans=True)
            P, S, value = out[9], out[10], out[0]
            col_err[t, b], self_err[t, b], moved[t, b] = out[6], out[7], out[8]
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
    return float(loss.item()), terms.detach().numpy(), grads, g_state, {'plans': plans, 'col_err': col_err, 'self_err': self_err,
                                                                        'transported': moved}


# ---- the cases of the device tests -----------------------------------------------------------------------------------------------
def reach_of(dens, scale=REACH_SCALE):
    """TG.sinkhorn_reach, with one sample's reach scaled where the batch's densities would give equal ones: the batch must carry
    two DIFFERENT reaches, or a reach indexed by the chunk instead of the batch would not show"""
    rho = np.array(TG.sinkhorn_reach(dens, scale), np.float64)
    if len(rho) > 1 and rho[0] == rho[1]:
        rho[1] *= 1.5
    return rho


def with_reach(kw, mass, scale=1.0):
    """a case of _divergence_f64_ref plus reach [B] (rho = REACH_SCALE x eps at eps scale 1; x the eps scale otherwise, so that
    rho / eps stays 4) and mass_q [H, B] as the trainer forms them"""
    kw = dict(kw)
    kw['reach'] = reach_of(kw['particle_dens'], REACH_SCALE * scale)
    kw['mass_q'] = np.array(TG.sinkhorn_mass_q(mass, kw['particle_nums'], kw['target_nums']), np.float64)
    return kw


def train_case(impulses, mass, scale=1.0):
    """_transport_ref.train_batch() (2 x 2 x 9, M = 12, counts 9/6, target counts 12,7 / 5,10) -> the keyword arguments of
    Engine.train_grad_f64_divergence(reach=, mass_q=); 'count' gives the four masses 12/9, 5/6, 7/9, 10/6 as [H, B]"""
    return with_reach(R.train_case(impulses, scale), mass, scale)


def tiny_case(mass='count'):
    return with_reach(R.tiny_case(), mass)


def single_case(mass='unit'):
    return with_reach(R.single_case(), mass)


def run(w, kw, see=None, K=None):
    return train_sinkhorn64_unbalanced(w, kw['states'], kw['states_delta'], kw['attrs'], kw['particle_nums'], kw['particle_dens'],
                                       kw['targets'], kw['target_nums'], kw['eps'], kw['reach'], kw['mass_q'],
                                       kw['iters'] if K is None else K, actions=kw.get('actions'), see=see)


def host_reference(w, kw):
    """-> (loss, terms, gradient blob, g_state [B, H, N, 3], col_err, self_err, transported), read-only"""
    import _untracked_ref as U
    loss, terms, grads, gs, info = run(w, kw)
    out = (loss, terms, np.asarray(U.blob64(grads), np.float64), gs, info['col_err'], info['self_err'], info['transported'])
    for v in out[1:]:
        v.setflags(write=False)
    return out


_cache = {}


def reference(golden, wset, impulses, mass):
    """host_reference of train_case(impulses, mass) on a weight set, computed once and left unchanged"""
    import _untracked_ref as U
    key = (wset, impulses, mass)
    if key not in _cache:
        _cache[key] = host_reference(U.weights_of(golden, wset), train_case(impulses, mass))
    return _cache[key]
