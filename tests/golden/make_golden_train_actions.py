#!/usr/bin/env python3
"""Golden vectors for training through the push (drp_train_step_actions), captured with the reference's model and the
reference's gen_s_delta.

The body of the loop at `train/train_gnn_dyn.py:159-189` on the REFERENCE's `PropNetDiffDenModel` (imported as
make_golden_train.py does), with `states_delta[:, t]` replaced by `PlannerGD.gen_s_delta` (`planners.py:211-257`) evaluated per
sample on `s_cur[b, :n_b]` -- the state the step actually reads -- and zeros on the padded rows, in fp32 autograd: the push's
position dependence is part of the graph, the hard mask a comparison.  One batch (tests/_train_actions_ref.py: 'golden'; B = 2,
N = 16 with counts 16 and 11, H = 3, seed-0 weights); written: the batch, the loss and the 18 gradient tensors.
Usage:
    python tests/golden/make_golden_train_actions.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import make_golden as mg  # noqa: E402


def main():
    from dyn_res_pile_manip_amd import synthetic as syn
    import _train_actions_ref as A
    torch, PropNetDiffDenModel, ref_planners, _ = mg.load_reference()
    import torch.nn.functional as F
    torch.set_num_threads(1)                                        # one summation order: the same bytes on regeneration
    config = syn.default_config()
    planner = ref_planners.PlannerGD(config, syn.SyntheticEnv(config))
    model = mg.make_model(torch, PropNetDiffDenModel, config, seed=0)
    model.train(True)
    states, actions, attrs, pnums, dens = A.batch(None, 'golden')
    st, ac, at, pd = [torch.from_numpy(np.array(x)) for x in (states, actions, attrs, dens)]
    B, n_rollout, N = st.shape[0], st.shape[1] - 1, st.shape[2]
    model.zero_grad()
    loss = 0.
    s_cur = st[:, 0]
    a_cur = at[:, 0]
    for idx_step in range(n_rollout):
        s_nxt = st[:, idx_step + 1]
        rows = []
        for j in range(B):
            n = int(pnums[j])
            planner.particle_num = n
            sd = planner.gen_s_delta(s_cur[j:j + 1, :n], ac[j:j + 1, idx_step])[0]
            rows.append(torch.cat([sd, torch.zeros((N - n, 3), dtype=sd.dtype)], 0))
        s_delta = torch.stack(rows)
        s_pred = model.predict_one_step(a_cur, s_cur, s_delta, pd)
        for j in range(B):
            loss += F.mse_loss(s_pred[j, :pnums[j]], s_nxt[j, :pnums[j]])
        s_cur = s_pred
    loss = loss / (n_rollout * B)
    loss.backward()
    out = {'states': states, 'actions': actions, 'attrs': attrs, 'particle_nums': pnums, 'particle_dens': dens,
           'loss': np.float64(loss.item())}
    for k, v in model.named_parameters():
        out['grad/' + k] = v.grad.detach().numpy().copy()
    assert len([k for k in out if k.startswith('grad/')]) == 18
    path = os.path.join(HERE, 'train_actions.npz')
    np.savez_compressed(path, **out)
    print('loss %.9e' % out['loss'])
    print('train_actions.npz %.1f KB' % (os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
