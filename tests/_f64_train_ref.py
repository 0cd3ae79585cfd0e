"""TEST INFRASTRUCTURE: the body of the training loop (train/train_gnn_dyn.py:167-203) restated in torch float64 with autograd,
on the step of tests/_f64_grad_ref.py.  Each step's graph comes from oracle.propnet_dense.adjacency on the fp32 roundings of the
double state and of the impulse -- the convention of the device's float64 calls (drp_step_f64, drp_gd_grad_f64,
drp_train_grad_f64) -- so both sides differentiate the same piecewise-smooth function.

Inputs are the fp32 values the device is given, widened exactly; the weights may be float64 (central differences).
tests/test_f64_train_host.py pins this restatement to the reference's own model run in double (tests/golden/train_f64.npz) and to
its own central differences."""
import numpy as np
import torch

from oracle.propnet_dense import adjacency
from _f64_grad_ref import _d, step, weights64

KEYS = ['model.particle_encoder.model.0', 'model.particle_encoder.model.2', 'model.relation_encoder.model.0',
        'model.relation_encoder.model.2', 'model.relation_encoder.model.4', 'model.particle_propagator.linear',
        'model.relation_propagator.linear', 'model.particle_predictor.linear_0', 'model.particle_predictor.linear_1']
PARAMS = [k + s for k in KEYS for s in ('.weight', '.bias')]          # state_dict order


def train_loss_and_grads64(W, states, states_delta, attrs, particle_nums, particle_dens, adj_thresh=0.08, want_graphs=False,
                           keep64=False):
    """-> (loss, loss_terms [n_rollout, B], {state_dict key: d loss / d parameter}, d loss / d every step's predicted state
    [B, n_rollout, N, 3]) as float64; loss_terms[t, b] = mse(s_pred[b, :n_b], states[b, t+1, :n_b]) / (n_rollout B), loss their
    sum.  want_graphs: also every step's adjacency (bool arrays).  keep64: float64 weights are taken as they are."""
    if keep64:
        W = dict((k, torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float64)))) for k, v in W.items())
    else:
        W = weights64(W)
    W = dict((k, v.clone().requires_grad_(True)) for k, v in W.items())
    st, sd, at, dens = _d(states), _d(states_delta), _d(attrs), _d(particle_dens)
    nums = [int(n) for n in np.asarray(particle_nums)]
    B, T1, N, _ = st.shape
    H = T1 - 1
    s_cur, a_cur = st[:, 0], at[:, 0]
    terms, preds, graphs = [], [], []
    for t in range(H):
        adj, _ = adjacency(s_cur.detach().float(), sd[:, t].float(), adj_thresh)
        s_pred = step(W, a_cur, s_cur, sd[:, t], dens, adj.double())
        s_pred.retain_grad()
        preds.append(s_pred)
        graphs.append(adj.bool().numpy())
        terms.append(torch.stack([((s_pred[b, :nums[b]] - st[b, t + 1, :nums[b]]) ** 2).mean() for b in range(B)]) / (H * B))
        s_cur = s_pred
    terms = torch.stack(terms)
    loss = terms.sum()
    loss.backward()
    grads = dict((k, W[k].grad.numpy().copy()) for k in PARAMS)
    g_state = np.stack([p.grad.numpy() if p.grad is not None else np.zeros((B, N, 3)) for p in preds], 1)
    out = (float(loss.item()), terms.detach().numpy(), grads, g_state)
    return out + (graphs,) if want_graphs else out


def blob64(grads):
    """{key: array} -> the 38 403 values in state_dict order"""
    return np.concatenate([np.asarray(grads[k], np.float64).ravel() for k in PARAMS])


def real_rows(a, particle_nums):
    """[B, H, N, 3] with the rows past a sample's particle count zeroed (what padded rows hold is not part of the contract)"""
    a = np.array(a, copy=True)
    for b, n in enumerate(np.asarray(particle_nums)):
        a[b, :, int(n):] = 0.0
    return a
