"""TEST INFRASTRUCTURE: one iteration of the gradient-descent planner (planners.py:685-745) restated in torch float64 with
autograd -- gen_s_delta (planners.py:211-257), the dense step (model/gnn_dyn.py:147-198), the rollout, the reward
(env/flex_rewards.py:189-214) with grid_sample written out as its explicit bilinear form, and the one-sided chamfer.  Written
from the formulas of oracle/propnet_dense.py, which is fp32 by construction and stays as it is; nothing of it is used here but
`adjacency`: each step's graph comes from the fp32 roundings of the double state and impulse, the convention of the device's
float64 calls (drp_step_f64, drp_gd_grad_f64), so both sides differentiate the same piecewise-smooth function.

Inputs are the fp32 values the device is given (weights, camera map, intrinsics, goal field, goal points), widened exactly; the
pushes may be float64 (central differences).  `pin_to_fixture` pins this restatement to the reference's own autograd
(tests/test_f64_grad_host.py)."""
import numpy as np
import torch

from oracle.propnet_dense import adjacency

PSTEP = 3
DENS_SCALE = 5000.0
PUSHER_W = 0.8 / 24.0        # planners.py:228, in double as the expression gives it
SOFT_MASK_SCALE = 0.01       # planners.py:251


def _d(x, keep64=False):
    """the fp32 value the device is given, widened exactly (keep64: float64 input is taken as it is)"""
    a = x.detach().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if not (keep64 and a.dtype == np.float64):
        a = a.astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.float64)))


def weights64(W):
    """state_dict-keyed arrays or tensors ('model.…', or 'w/model.…' of a golden file) -> float64 tensors"""
    keys = W.files if hasattr(W, 'files') else W.keys()
    out = {}
    for k in keys:
        if k.startswith('w/'):
            out[k[2:]] = _d(W[k])
        elif k.startswith('model.'):
            out[k] = _d(W[k])
    return out


def _lin(W, name, x):
    return x @ W[name + '.weight'].t() + W[name + '.bias']


def gen_s_delta(s_cur, action, m34, gs, want_mask=False):
    B, N, _ = s_cur.shape
    zero = torch.zeros((B, 1), dtype=torch.float64)
    one = torch.ones((B, 1), dtype=torch.float64)
    sc = torch.cat([action[:, 0:1], zero, -action[:, 1:2], one], 1) @ m34.t() / gs
    ec = torch.cat([action[:, 2:3], zero, -action[:, 3:4], one], 1) @ m34.t() / gs
    dvec = ec - sc
    length = torch.linalg.norm(dvec, dim=1)
    dirn = dvec / length[:, None]
    ortho = torch.cat([-dirn[:, 1:2], dirn[:, 0:1], zero], 1)
    rel = s_cur - sc[:, None, :]
    v = (rel * ortho[:, None, :]).sum(-1)
    u = (rel * dirn[:, None, :]).sum(-1)
    hard = ((u < length[:, None]) & (u > 0.0))
    soft = torch.maximum(torch.clamp(-PUSHER_W - v, min=0.0), torch.clamp(v - PUSHER_W, min=0.0))
    soft = torch.exp(-soft / SOFT_MASK_SCALE)
    to_end = ((ec[:, None, :] - s_cur) * dirn[:, None, :]).sum(-1)
    out = to_end[..., None] * dirn[:, None, :] * hard.double()[..., None] * soft[..., None]
    return (out, hard) if want_mask else out


def relations(adj):
    """model/gnn_dyn.py:242-251: edges in (b, receiver, sender) order as dense one-hot Rr / Rs [B, max_E, N], float64"""
    B, N, _ = adj.shape
    n_rels = adj.sum(dim=(1, 2)).long()
    n_rel = int(n_rels.max().item())
    rels = adj.nonzero()
    within = torch.cat([torch.arange(int(n)) for n in n_rels])
    Rr = torch.zeros((B, n_rel, N), dtype=torch.float64)
    Rs = torch.zeros((B, n_rel, N), dtype=torch.float64)
    Rr[rels[:, 0], within, rels[:, 1]] = 1
    Rs[rels[:, 0], within, rels[:, 2]] = 1
    return Rr, Rs


def step(W, a_cur, s_cur, s_delta, dens, adj):
    """model/gnn_dyn.py:147-198 on the given adjacency"""
    B, N = a_cur.shape
    Rr, Rs = relations(adj)
    E = Rr.shape[1]
    d = dens / DENS_SCALE
    dn = d[:, None, None].expand(B, N, 1)
    de = d[:, None, None].expand(B, E, 1)
    a_r, a_s = Rr.bmm(a_cur[..., None]), Rs.bmm(a_cur[..., None])
    s_r, s_s = Rr.bmm(s_cur), Rs.bmm(s_cur)
    h = torch.relu(_lin(W, 'model.particle_encoder.model.0', torch.cat([s_delta, a_cur[:, :, None], dn], 2)))
    pe = torch.relu(_lin(W, 'model.particle_encoder.model.2', h))
    h = torch.relu(_lin(W, 'model.relation_encoder.model.0', torch.cat([a_r, a_s, s_r - s_s, de], 2)))
    h = torch.relu(_lin(W, 'model.relation_encoder.model.2', h))
    re = torch.relu(_lin(W, 'model.relation_encoder.model.4', h))
    effect = pe
    for _ in range(PSTEP):
        e_rel = torch.relu(_lin(W, 'model.relation_propagator.linear', torch.cat([re, Rr.bmm(effect), Rs.bmm(effect), de], 2)))
        agg = Rr.transpose(1, 2).bmm(e_rel)
        effect = torch.relu(_lin(W, 'model.particle_propagator.linear', torch.cat([pe, agg, dn], 2)) + effect)
    h = torch.relu(_lin(W, 'model.particle_predictor.linear_0', effect))
    return _lin(W, 'model.particle_predictor.linear_1', h) + s_cur


def reward(state, G, cam_params, goal_coor, want_decisions=False):
    """env/flex_rewards.py:189-214: projection, border-clamped bilinear sample of G (align_corners=False), one-sided chamfer"""
    B, N, _ = state.shape
    Hh, Ww = G.shape
    fx, fy, cx, cy = [float(v) for v in cam_params]
    px = state[:, :, 0] * fx / state[:, :, 2] + cx
    py = state[:, :, 1] * fy / state[:, :, 2] + cy
    ix = torch.clamp(((px / Hh * 2 - 1) + 1) * Ww / 2 - 0.5, 0, Ww - 1)
    iy = torch.clamp(((py / Hh * 2 - 1) + 1) * Hh / 2 - 0.5, 0, Hh - 1)
    x0, y0 = torch.floor(ix).detach(), torch.floor(iy).detach()
    tx, ty = ix - x0, iy - y0
    x0, y0 = x0.long(), y0.long()
    x1, y1 = torch.clamp(x0 + 1, max=Ww - 1), torch.clamp(y0 + 1, max=Hh - 1)
    r1 = (G[y0, x0] * (1 - tx) * (1 - ty) + G[y0, x1] * tx * (1 - ty) + G[y1, x0] * (1 - tx) * ty + G[y1, x1] * tx * ty).sum(1)
    pix = torch.stack([px, py], 2)
    dist = torch.sqrt(((goal_coor[None, :, None, :] - pix[:, None, :, :]) ** 2).sum(3))
    mn = dist.min(dim=2)
    r = -(r1 + mn.values.sum(1)) / N
    return (r, (x0, y0, mn.indices)) if want_decisions else r


def gd_loss_and_grads64(W, s0, dens, attr, act_seqs, G, cam_params, goal_coor, m34, global_scale, adj_thresh=0.08,
                        want_decisions=False):
    """-> (reward [B], d loss / d act_seqs [B,H,4], d loss / d state_pred [B,H,N,3]) as float64 arrays, loss = -sum(reward).
    Every step's slice of the state gradient is the total gradient of that step's predicted state (what drp_gd_grad returns);
    the reference's retained gradient of its in-place-filled tensor shows the final step's slice only.
    want_decisions: also the discrete decisions taken (per step adjacency and hard mask, bilinear cell, arg-min)."""
    W = weights64(W)
    s0, dens, attr, G, goal_coor, m34 = _d(s0), _d(dens), _d(attr), _d(G), _d(goal_coor), _d(m34).reshape(3, 4)
    cam_params = _d(cam_params).tolist()
    gs = float(np.float32(global_scale))
    acts = _d(act_seqs, keep64=True).clone().requires_grad_(True)
    B, H, _ = acts.shape
    nb, N, _ = s0.shape
    ns = B // nb
    s, d, a = s0.repeat(ns, 1, 1), dens.repeat(ns), attr.repeat(ns, 1)
    states, dec = [], []
    for t in range(H):
        sd, hard = gen_s_delta(s, acts[:, t], m34, gs, want_mask=True)
        adj, _ = adjacency(s.detach().float(), sd.detach().float(), adj_thresh)
        s = step(W, a, s, sd, d, adj)
        s.retain_grad()
        states.append(s)
        dec += [adj.bool().numpy(), hard.numpy()]
    r, rd = reward(states[-1], G, cam_params, goal_coor, want_decisions=True)
    torch.sum(-r).backward()
    gs_pred = np.stack([st.grad.numpy() if st.grad is not None else np.zeros((B, N, 3)) for st in states], 1)
    out = (r.detach().numpy(), acts.grad.numpy(), gs_pred)
    if want_decisions:
        return out + (dec + [v.numpy() for v in rd],)
    return out


# ---- central differences in push space (tests/test_f64_grad_host.py; on the device tests/test_gpu_gd_f64.py) ----------------
FD_H = 2.0 ** -14


def fd_point(act_seqs):
    """the pushes on the 2^-10 grid: with the directions of fd_direction, a +- FD_H d is exact in fp32, so the device (whose
    pushes are fp32) and the restatement evaluate the very same points"""
    return np.round(np.asarray(act_seqs, np.float64) * 1024.0) / 1024.0


def fd_direction(shape, rng):
    """a random direction of unit length up to its quantisation to multiples of 2^-6"""
    d = rng.standard_normal(shape)
    return np.round(d / np.linalg.norm(d) * 64.0) / 64.0


def fd_check(fn, acts, n_dir=8, max_redraw=2, seed=0):
    """fn(acts) -> (reward [B], grad_act, decisions: list of arrays).  For n_dir directions d: the central difference of
    sum(reward) at +- FD_H d against -(grad . d); a direction along which a discrete decision differs at +-h is redrawn
    (at most max_redraw times in all).  -> list of (central difference, -(g . d))"""
    rng = np.random.default_rng(seed)
    a0 = fd_point(acts)
    _, g0, _ = fn(a0)
    out, redrawn = [], 0
    while len(out) < n_dir:
        d = fd_direction(a0.shape, rng)
        rp, _, dp = fn(a0 + FD_H * d)
        rm, _, dm = fn(a0 - FD_H * d)
        if not all(np.array_equal(x, y) for x, y in zip(dp, dm)):
            redrawn += 1
            assert redrawn <= max_redraw, 'more than %d directions flip a discrete decision at h = %g' % (max_redraw, FD_H)
            continue
        out.append(((rp.sum() - rm.sum()) / (2 * FD_H), -float((g0 * d).sum())))
    return out


# worst |central difference + g . d| / |g| over the 8 directions of tests/test_f64_grad_host.py, as measured there
FD_RESIDUAL = {'n20_h1': 1.9e-9, 'h2': 2.2e-8}
