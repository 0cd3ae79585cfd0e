"""CPU: the float64 reward reference of tests/_reward_ref.py and the cases of tests/_reward_cases.py, before any kernel is
held to them (tests/test_gpu_reward_edges.py).

1. The reference IS the reference's operation: value and gradient equal env/flex_rewards.py:189-214 written with F.grid_sample
   and torch.norm(...).min under float64 autograd (not a torch.clamp restatement) to 1e-12 relative, on every case of the GPU
   test -- the particles exactly on the border, the ties and the zero distance included.
2. The random cases are conditioned: every ix, iy is at least 8 fp32 error bounds from every integer and every other particle's
   squared distance at least 8 bounds from the best, so an fp32 kernel takes the float64 cell and arg-min; nothing is excluded.
3. The lattice cases are exact: every intermediate is a float32 number.
4. The bound is tight enough: each mutant of the reference, scored against the true reference on the same inputs, exceeds the
   fp32 bound on at least one case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _reward_cases as C
import _reward_ref as R


@pytest.fixture(scope='module')
def all_cases():
    cases, refs = C.cases()
    extra = C.scenes_case()
    return list(cases) + extra, list(refs) + [R.evaluate(c['state'], c['G'], c['cam'], c['goal']) for c in extra]


def torch_reward(state, G, cam, goal_coor):
    """env/flex_rewards.py:186-214 in float64 -> (value [B], value_raw [B], d(-sum value) / d state, arg-min [B,M])"""
    state = torch.tensor(np.asarray(state, np.float64), requires_grad=True)
    goal = torch.tensor(np.asarray(G, np.float64))
    goal_coor = torch.tensor(np.asarray(goal_coor, np.float64))
    fx, fy, cx, cy = [float(v) for v in cam]
    B, N, _ = state.shape
    H, W = goal.shape
    goal = torch.tile(goal[None, None, ...], (B, 1, 1, 1))
    goal_coor = torch.tile(goal_coor[None, ...], (B, 1, 1))
    pix = torch.stack([state[:, :, 0] * fx / state[:, :, 2] + cx, state[:, :, 1] * fy / state[:, :, 2] + cy], 2)
    pix = pix.unsqueeze(1)
    norm_pix = pix / H * 2 - 1
    rewards = F.grid_sample(goal, norm_pix, padding_mode='border', align_corners=False)
    rewards = rewards.squeeze(1).squeeze(1).sum(dim=1)
    dist_to_pix = torch.norm(goal_coor[:, :, None, :] - pix, dim=3)
    min_dist_to_pix, idx = dist_to_pix.min(dim=2)
    rewards = rewards + min_dist_to_pix.sum(dim=1)
    raw = -rewards
    value = -(rewards / N)
    (-value.sum()).backward()
    return value.detach().numpy(), raw.detach().numpy(), state.grad.numpy(), idx.numpy()


def test_the_cases_are_the_ones_asked_for(all_cases):
    cases, refs = all_cases
    rand = [c for c in cases if c['kind'] == 'random' and not c['name'].startswith('scene')]
    assert [(c['state'].shape[1], c['goal'].shape[0]) for c in rand] == C.NM
    assert {c['G'].shape for c in rand} == set(C.SIZES)
    assert all(3 <= c['state'].shape[0] <= 6 for c in cases if not c['name'].startswith('scene'))
    assert [c['G'].shape for c in cases if c['kind'] == 'lattice'] == [(64, 32), (32, 64)]


def test_reference_is_grid_sample_and_norm_min_under_autograd(all_cases):
    cases, refs = all_cases
    for c, t in zip(cases, refs):
        value, raw, grad, idx = torch_reward(c['state'], c['G'], c['cam'], c['goal'])
        assert np.all(np.isfinite(t['value'])) and np.all(np.isfinite(t['grad'])), c['name']
        np.testing.assert_allclose(t['value'], value, rtol=1e-12, atol=0, err_msg=c['name'])
        np.testing.assert_allclose(t['value_raw'], raw, rtol=1e-12, atol=0, err_msg=c['name'])
        np.testing.assert_allclose(t['grad'], grad, rtol=1e-12, atol=1e-12 * np.abs(grad).max(), err_msg=c['name'])
        assert np.array_equal(t['arg'], idx), c['name']


def test_random_cases_are_conditioned_and_nothing_is_excluded(all_cases):
    cases, refs = all_cases
    for c, t in zip(cases, refs):
        if c['kind'] != 'random':
            continue
        B, N, _ = c['state'].shape
        mi, mg = R.fp32_margins(t)
        assert mi.shape == (B, N, 2) and mg.shape == (B, c['goal'].shape[0])
        excluded = int((mi.min(-1) < C.MARGIN).sum() + (mg < C.MARGIN).sum())
        print('[reward-cases] %s: B=%d, %d redrawn, %d excluded, margins ix/iy %.1f goal %.1f'
              % (c['name'], B, c['redrawn'], excluded, mi.min(), mg.min()))
        assert excluded == 0, c['name']
        # every particle is still of its class: the last cell, the clamped half pixel, outside each side and corner
        Hh, Ww = c['G'].shape
        for b in range(B):
            for n in range(N):
                assert C._in_class(t['ix_raw'][b, n], c['classes'][b][n][0], Ww), (c['name'], b, n)
                assert C._in_class(t['iy_raw'][b, n], c['classes'][b][n][1], Hh), (c['name'], b, n)
        if N >= 40:
            flat = [k for row in c['classes'] for k in row]
            out = [k for k in flat if k[0][:2] in ('lo', 'hi') or k[1][:2] in ('lo', 'hi')]
            assert len(out) >= 0.1 * len(flat)
            assert {(k[0][:2], k[1][:2]) for k in out} >= {('lo', 'in'), ('hi', 'in'), ('in', 'lo'), ('in', 'hi'), ('lo', 'lo'),
                                                           ('hi', 'lo'), ('lo', 'hi'), ('hi', 'hi')}
            assert any(k[0].endswith('far') or k[1].endswith('far') for k in out)
            assert {('last', 'in'), ('in', 'last'), ('half', 'in'), ('in', 'half'), ('in', 'in')} <= set(flat)
            far = np.abs(t['ix_raw']).max()
            assert far > 3e3


def test_lattice_cases_are_exact_in_fp32(all_cases):
    cases, refs = all_cases

    def is_f32(a):
        a = np.asarray(a, np.float64)
        return np.array_equal(a.astype(np.float32).astype(np.float64), a)
    for c, t in zip(cases, refs):
        if c['kind'] != 'lattice':
            continue
        for k in ('u', 'v', 'nx', 'ny', 'ix_raw', 'iy_raw', 'tx', 'ty', 'terms', 'bil', 'r1', 'r2', 'dist', 'value_raw', 'value'):
            assert is_f32(t[k]), (c['name'], k)
        assert np.array_equal(t['dist'], np.round(t['dist']))                  # 0, 5, 10: the roots are exact
        assert np.array_equal(np.cumsum(t['bil'], 1) * 4, np.round(np.cumsum(t['bil'], 1) * 4))     # quarters: any order of the sum is exact
        N = c['state'].shape[1]
        assert N & (N - 1) == 0                                                # / N is exact
        # the edges the case is for
        assert (t['ix_raw'] == 0).any() and (t['ix_raw'] == c['G'].shape[1] - 1).any()
        assert (t['iy_raw'] == 0).any() and (t['iy_raw'] == c['G'].shape[0] - 1).any()
        inside = (t['ix_raw'] > 0) & (t['ix_raw'] < c['G'].shape[1] - 1)
        assert (inside & (t['tx'] == 0)).any() and (t['tx'] == 0.5).any()
        assert np.all(t['dist'][:, C.LATTICE_ZERO] == 0)
        for b in range(c['state'].shape[0]):
            pos = {int(k): n for n, k in enumerate(c['order'][b])}             # particle of the specification -> its index in row b
            d2 = t['d2'][b]
            assert d2[C.LATTICE_TIE, pos[10]] == d2[C.LATTICE_TIE, pos[11]] == 25.0 == t['dist'][b, C.LATTICE_TIE] ** 2
            assert t['arg'][b, C.LATTICE_TIE] == min(pos[10], pos[11])         # the first index
            assert np.array_equal(c['state'][b, pos[12]], c['state'][b, pos[13]])
            assert t['arg'][b, C.LATTICE_DUP] == min(pos[12], pos[13])
            assert t['arg'][b, C.LATTICE_ZERO] == pos[14]
        firsts = {bool(np.flatnonzero(c['order'][b] == 10)[0] < np.flatnonzero(c['order'][b] == 11)[0]) for b in range(3)}
        assert firsts == {True, False}                                         # either particle of the tie comes first in some row
        assert np.isnan(c['G'][C.POISON]) and np.isfinite(np.delete(c['G'].ravel(), C.POISON[0] * c['G'].shape[1])).all()


def test_every_mutant_exceeds_the_fp32_bound_on_some_case(all_cases):
    cases, refs = all_cases
    bounds = [R.bound(t, R.U32, 'kb_reward') for t in refs]
    missed = []
    for mutant in R.MUTANTS:
        worst, where = 0.0, None
        for c, t, bd in zip(cases, refs, bounds):
            m = R.evaluate(c['state'], c['G'], c['cam'], c['goal'], mutant=mutant)
            r = max(R.ratio(m['value'], t['value'], bd['value']), R.ratio(m['value_raw'], t['value_raw'], bd['value_raw']),
                    R.ratio(m['grad'], t['grad'], bd['grad']))
            if r > worst:
                worst, where = r, c['name']
        print('[reward-mutant] %-16s worst err / bound %.3e on %s' % (mutant, worst, where))
        if not worst > 1.0:
            missed.append(mutant)
    assert not missed, 'no case catches %s' % missed


def test_the_bound_grows_with_the_roundoff_and_is_finite(all_cases):
    cases, refs = all_cases
    for c, t in zip(cases, refs):
        for kernel in R.KERNELS:
            b32, b64 = R.bound(t, R.U32, kernel), R.bound(t, R.U64, kernel)
            for k in ('value', 'value_raw', 'grad'):
                assert np.all(np.isfinite(b32[k])) and np.all(b32[k] >= b64[k]) and np.all(b64[k] >= 0), (c['name'], kernel, k)
