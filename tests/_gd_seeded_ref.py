"""TEST INFRASTRUCTURE: one iteration of the gradient-descent planner on a cost of the caller's, restated in torch float64 with
autograd -- tests/_f64_grad_ref.py's loop (its gen_s_delta, step and adjacency, imported, with its graph convention: each step's
lists from the fp32 roundings of the double state and impulse) with the loss as an argument.  The yardstick of
drp_gd_predict_f64 / drp_gd_grad_f64_seeded (tests/test_gpu_gd_f64_seeded.py); tests/test_gd_seeded_host.py pins it to
gd_loss_and_grads64 and to its own central differences."""
import numpy as np
import torch

import _f64_grad_ref as R
from oracle.propnet_dense import adjacency


def gd_cost_and_grads64(W, s0, dens, attr, act_seqs, cost_torch, m34, global_scale, adj_thresh=0.08, want_decisions=False):
    """cost_torch(pred [B,H,N,3] float64 tensor) -> values [B] tensor; the loss is values.sum().
    -> (values [B], pred [B,H,N,3], d loss / d act_seqs [B,H,4], d loss / d state_pred [B,H,N,3]: every step's TOTAL gradient,
    the cost's own share included) as float64 arrays[, the discrete decisions: per step adjacency and hard mask]."""
    W = R.weights64(W)
    s0, dens, attr, m34 = R._d(s0), R._d(dens), R._d(attr), R._d(m34).reshape(3, 4)
    gs = float(np.float32(global_scale))
    acts = R._d(act_seqs, keep64=True).clone().requires_grad_(True)
    B, H, _ = acts.shape
    nb, N, _ = s0.shape
    ns = B // nb
    s, d, a = s0.repeat(ns, 1, 1), dens.repeat(ns), attr.repeat(ns, 1)
    states, dec = [], []
    for t in range(H):
        sd, hard = R.gen_s_delta(s, acts[:, t], m34, gs, want_mask=True)
        adj, _ = adjacency(s.detach().float(), sd.detach().float(), adj_thresh)
        s = R.step(W, a, s, sd, d, adj)
        s.retain_grad()
        states.append(s)
        dec += [adj.bool().numpy(), hard.numpy()]
    values = cost_torch(torch.stack(states, 1))
    assert values.shape == (B,), values.shape
    values.sum().backward()
    g_state = np.stack([st.grad.numpy() if st.grad is not None else np.zeros((B, N, 3)) for st in states], 1)
    g_act = acts.grad.numpy() if acts.grad is not None else np.zeros((B, H, 4))
    out = (values.detach().numpy(), torch.stack(states, 1).detach().numpy(), g_act, g_state)
    return out + (dec,) if want_decisions else out


def make_case(N, H, nb=2, B=4, seed=None):
    """the smallest shapes that reach the branches: nb start columns x (B / nb) push sequences on a synthetic pile of N particles
    (the generators tests/test_gpu_gd_f64.py's synthetic_case draws from) -> the dict of a gradient case, plus 'targets' [H,N,3]:
    the start pile of column 0 shifted a little further each step (a tracked target for quadratic_cost) and 'weights' [H]"""
    from dyn_res_pile_manip_amd import synthetic as syn
    seed = N + 7 * H if seed is None else seed
    s0, dens, attr = syn.make_pile(N, nb, seed=seed)
    acts = syn.sample_pushes(B, H, seed=seed).astype(np.float32)
    coor = syn.goal_coor_strided(syn.goal_distance_image(syn.goal_mask('I')), 5 * N)
    shift = np.array([0.01, -0.005, 0.0], np.float32)
    targets = np.stack([s0[0] + (t + 1) * shift for t in range(H)]).astype(np.float32)
    return {'s_cur': s0, 'dens': dens, 'attr': attr, 'act_seqs': acts, 'goal_coor': coor, 'targets': targets,
            'weights': np.linspace(1.0, 2.0, H).astype(np.float32)}


def seed_cost(seed):
    """the cost whose state gradient IS `seed` [B,H,N,3], whatever the prediction: values[b] = <seed[b], pred[b]>"""
    sd = torch.from_numpy(np.ascontiguousarray(np.asarray(seed, np.float64)))
    return lambda pred: (pred * sd).sum(dim=(1, 2, 3))


def quadratic_torch(targets, step_weights=None):
    """costs.quadratic_cost in torch: values[b] = sum_t w_t mean_n |pred[b,t,n] - targets[t,n]|^2"""
    tg = torch.from_numpy(np.ascontiguousarray(np.asarray(targets, np.float64)))

    def cost(pred):
        B, H, N, _ = pred.shape
        w = torch.ones(H, dtype=torch.float64) if step_weights is None else torch.from_numpy(np.asarray(step_weights, np.float64))
        return ((pred - tg) ** 2 * (w / N).reshape(1, H, 1, 1)).sum(dim=(1, 2, 3))
    return cost
