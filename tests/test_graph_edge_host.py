"""CPU: the preconditions of tests/test_gpu_graph_edges.py.  Every case of tests/_graph_edge_cases.py is what its generator
says it is, oracle/propnet_sparse.build_neighbours decides it as the reference's own arithmetic does (oracle/propnet_dense.adjacency:
torch fp32 against a threshold that is a Python double), and the host restatement of the reversed lists is right.  Nothing here
is skipped: a seed that breaks a condition is replaced, the condition stays."""
import numpy as np
import pytest

import _graph_edge_cases as G
from oracle import propnet_dense as od
from oracle import propnet_sparse as osp

K = G.K


def _oracle(c):
    if 'oracle' not in c.meta:
        c.meta['oracle'] = osp.build_neighbours(c.s_cur, c.s_delta, c.radius)
    return c.meta['oracle']


def _dis(c, b):
    """[recv, send] fp32 squared distances of sample b in the oracle's operation order"""
    p = c.s_cur[b] + c.s_delta[b]
    return G.dis32(p[None, :, :] - p[:, None, :])


def _edge_sets(idx, cnt):
    return [[set(int(j) for j in idx[b, i, :cnt[b, i]]) for i in range(idx.shape[1])] for b in range(idx.shape[0])]


# ---- the table of the issue: the reference's thresholds ---------------------------------------------------------------------
def test_reference_threshold_bits():
    """fp32(r * r) with r * r in Python doubles, the scalar torch rounds once in (dis - threshold) < 0, and what squaring the
    fp32 rounding of the radius gives instead: another pattern at 0.05, 0.1 and 0.7, the same at the other four"""
    import torch
    squared_fp32_radius = {}
    for r in G.SHELL_RADII:
        want = G.THRESHOLD_BITS[r]
        assert int(np.float32(r * r).view(np.uint32)) == want
        # torch's own rounding of the Python scalar: the largest fp32 d with (d - r * r) < 0 is the one under fp32(r * r)
        t = torch.tensor([want - 1, want, want + 1], dtype=torch.int32).view(torch.float32)
        assert ((t - r * r) < 0).tolist() == [True, False, False]
        squared_fp32_radius[r] = int(np.float32(np.float64(np.float32(r)) ** 2).view(np.uint32)) - want
    assert squared_fp32_radius == {0.02: 0, 0.05: 1, 0.08: 0, 0.0801: 0, 0.1: 1, 0.3: 0, 0.7: -1}


# ---- shell ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius', G.SHELL_RADII)
def test_shell_is_what_it_says(radius):
    c = G.case('shell_r%g' % radius)
    tb = G.THRESHOLD_BITS[radius]
    assert c.B == 2 and 129 <= c.N <= 350 and not c.s_delta.any()
    assert not np.array_equal(c.s_cur[0, :100], c.s_cur[1, :100])
    # on the 2^-20 grid: every coordinate difference is exact in fp32
    scaled = c.s_cur.astype(np.float64) / G.GRID
    assert np.array_equal(scaled, np.round(scaled)) and np.abs(scaled).max() < 2 ** 24
    for b in range(c.B):
        recv, send, send_recv, cls = (c.meta[k][b] for k in ('recv', 'send', 'send_recv', 'send_cls'))
        for k in G.CLASSES:
            assert (cls == k).sum() >= 40, (radius, b, k)
        assert np.bincount(send_recv, minlength=c.N).max() <= 8
        d = _dis(c, b)
        bits = d.view(np.uint32).astype(np.int64)
        assert np.array_equal(bits[send_recv, send] - tb, cls)
        assert np.array_equal(bits[send, send_recv] - tb, cls)
        # centres more than twice the radius apart, and a receiver sees nobody but its own group inside 1.02 radii: its
        # top-10 cut never binds
        centres = c.s_cur[b][recv].astype(np.float64)
        gap = np.linalg.norm(centres[:, None] - centres[None], axis=-1) + 1e9 * np.eye(len(recv))
        assert gap.min() > 2.0 * radius
        near = d[recv] < np.float32((1.02 * radius) ** 2)
        assert near.sum(1).max() <= 9
        for g, r in enumerate(recv):
            members = set(send[send_recv == r].tolist()) | {int(r)}
            assert set(np.nonzero(near[g])[0].tolist()) == members
        # no tie at the cut inside the radius anywhere in the sample: topk's tie order cannot matter
        srt = np.sort(bits, axis=1)
        assert not ((srt[:, K - 1] == srt[:, K]) & (srt[:, K - 1] < tb)).any()


@pytest.mark.parametrize('radius', G.SHELL_RADII)
def test_oracle_decides_the_shell_on_the_last_bit(radius):
    c = G.case('shell_r%g' % radius)
    idx, cnt = _oracle(c)
    sets = _edge_sets(idx, cnt)
    for b in range(c.B):
        send, send_recv, cls = (c.meta[k][b] for k in ('send', 'send_recv', 'send_cls'))
        for j, i, k in zip(send.tolist(), send_recv.tolist(), cls.tolist()):
            assert (j in sets[b][i]) == (k < 0), (radius, b, i, j, k)       # T - 1 ulp: an edge; T and T + 1 ulp: none
            assert (i in sets[b][j]) == (k < 0), (radius, b, j, i, k)       # ... in both directions


@pytest.mark.parametrize('radius', G.SHELL_RADII)
def test_dense_reference_arithmetic_gives_the_oracles_edges(radius):
    """oracle/propnet_dense.adjacency -- torch fp32, (dis - threshold) < 0 with the threshold a Python double -- on the shell:
    this pins the threshold's rounding to the reference's arithmetic and not to ours"""
    import torch
    c = G.case('shell_r%g' % radius)
    idx, cnt = _oracle(c)
    adj, dis = od.adjacency(torch.from_numpy(c.s_cur.copy()), torch.from_numpy(c.s_delta.copy()), c.radius)
    adj = adj.numpy() > 0
    mine = np.zeros_like(adj)
    for b in range(c.B):
        # torch's reduction gives the oracle's bits here (three terms, exact differences)
        assert np.array_equal(dis[b].numpy(), _dis(c, b))
        for i in range(c.N):
            mine[b, i, idx[b, i, :cnt[b, i]]] = True
    assert np.array_equal(adj, mine)
    assert np.array_equal(adj.sum(2), cnt)


# ---- every case: the oracle against a restatement with no partition --------------------------------------------------------------
def brute_force_neighbours(s_cur, s_delta, radius):
    p = np.asarray(s_cur, np.float32) + np.asarray(s_delta, np.float32)
    B, N, _ = p.shape
    thr = np.float32(radius * radius)
    idx = -np.ones((B, N, K), np.int32)
    cnt = np.zeros((B, N), np.int32)
    for b in range(B):
        d = G.dis32(p[b][None, :, :] - p[b][:, None, :])
        bits = d.view(np.uint32)
        for i in range(N):
            order = sorted(range(N), key=lambda j: (int(bits[i, j]), j))[:K]
            keep = sorted(j for j in order if (d[i, j] - thr) < 0)
            idx[b, i, :len(keep)] = keep
            cnt[b, i] = len(keep)
    return idx, cnt


@pytest.mark.parametrize('name', G.CASE_NAMES)
def test_oracle_equals_a_sort_per_receiver(name):
    c = G.case(name)
    idx, cnt = _oracle(c)
    bidx, bcnt = brute_force_neighbours(c.s_cur, c.s_delta, c.radius)
    assert np.array_equal(cnt, bcnt)
    assert np.array_equal(idx, bidx)
    assert idx.dtype == np.int32 and (idx[np.arange(K)[None, None, :] >= cnt[..., None]] == -1).all()


# ---- the other cases are what they say ------------------------------------------------------------------------------------------
def _strip(x):
    t = (x.astype(np.float32) - np.float32(-0.32)) * np.float32(100.0)
    return np.minimum(np.maximum(t, np.float32(0)), np.float32(63)).astype(np.int32)


def _band(y, hb=0.02):
    gy = max(1, min(32, int(np.ceil(np.float32(0.64) / np.float32(hb)))))
    t = (y.astype(np.float32) - np.float32(-0.32)) * (np.float32(gy) / np.float32(0.64))
    return np.minimum(np.maximum(t, np.float32(0)), np.float32(gy - 1)).astype(np.int32)


@pytest.mark.parametrize('name', [n for n in G.CASE_NAMES if n.startswith('lattice')])
def test_lattice_sits_on_the_strip_and_band_boundaries(name):
    """graph_strip / graph_band of csrc/k_graph.h restated: an ulp to one side of a particle lies another strip (band) for a good
    share of the sample, and exact ties at the top-10 cut exist inside the radius"""
    c = G.case(name)
    tb = int(np.float32(c.radius * c.radius).view(np.uint32))
    for b in range(c.B):
        x, y = c.s_cur[b, :, 0], c.s_cur[b, :, 1]
        for f, v in ((_strip, x), (_band, y)):
            edge = (f(np.nextafter(v, np.float32(-1))) != f(v)) | (f(np.nextafter(v, np.float32(1))) != f(v))
            assert edge.sum() > c.N // 10, (name, b, f.__name__, int(edge.sum()))
            assert len(np.unique(f(v))) >= 8                       # spread over several strips (bands), none clamped
            assert f(v).min() > 0 and f(v).max() < (63 if f is _strip else 31)
        bits = np.sort(_dis(c, b).view(np.uint32).astype(np.int64), axis=1)
        ties = (bits[:, K - 1] == bits[:, K]) & (bits[:, K - 1] < tb)
        print('[graph-edges] %s sample %d: %d receivers with an exact tie at the cut' % (name, b, int(ties.sum())))
        assert ties.sum() >= 5


def test_lines_strip_and_tiny_piles():
    for name in ('xline_r0.08', 'xline_r0.02', 'yline_r0.08', 'yline_r0.02'):
        c = G.case(name)
        axis = 0 if name[0] == 'x' else 1
        p = c.s_cur + c.s_delta
        assert c.N == 300
        beyond = (np.abs(p[..., axis]) > 0.32).mean()
        assert 0.25 < beyond < 0.42, (name, beyond)
        assert np.abs(p[..., 1 - axis]).max() < 0.05
    c = G.case('one_strip_r0.08')
    p = c.s_cur + c.s_delta
    assert c.N == 200 and (p[..., 0] > 0.35).all() and (_strip(p[..., 0]) == 63).all()
    c = G.case('tiny_r0.0001')
    idx, cnt = _oracle(c)
    assert c.N == 150 and (cnt == 1).all() and np.array_equal(idx[..., 0], np.broadcast_to(np.arange(c.N), cnt.shape))
    z = G.case('tiny_r0')
    assert np.array_equal(z.s_cur, c.s_cur) and np.array_equal(z.s_delta, c.s_delta) and z.radius == 0.0
    idx, cnt = _oracle(z)
    assert (cnt == 0).all() and (idx == -1).all()                    # (0 - 0) < 0 is false: not even the self loop


# ---- reversed lists -----------------------------------------------------------------------------------------------------------
def reverse_lists_loops(nbr_idx, nbr_cnt, n_recv):
    B, N, _ = nbr_idx.shape
    off = np.zeros((B, N + 1), np.int32)
    rev = []
    for b in range(B):
        out = []
        for j in range(N):
            for i in range(N):
                for k in range(K):
                    if k < nbr_cnt[b, i] and nbr_idx[b, i, k] == j and i < n_recv[b]:
                        out.append(i * K + k)
            off[b, j + 1] = len(out)
        rev.append(np.asarray(out, np.int32))
    return off, rev


@pytest.mark.parametrize('N,B,seed', [(7, 2, 0), (23, 3, 1)])
def test_reverse_lists_np_against_a_triple_loop(N, B, seed):
    rng = np.random.default_rng(seed)
    s = np.zeros((B, N, 3), np.float32)
    s[..., :2] = rng.uniform(-0.1, 0.1, (B, N, 2))
    s[..., 2] = 0.75
    idx, cnt = osp.build_neighbours(s, np.zeros_like(s), 0.08)
    # the device's other emission order too: the self loop first, the rest ascending
    first = idx.copy()
    for b in range(B):
        for i in range(N):
            row = [j for j in idx[b, i, :cnt[b, i]] if j != i]
            first[b, i, :cnt[b, i]] = [i] + row
    for lists in (idx, first):
        for n_recv in (None, rng.integers(1, N + 1, B)):
            off, rev = G.reverse_lists_np(lists, cnt, n_recv)
            loff, lrev = reverse_lists_loops(lists, cnt, np.full(B, N) if n_recv is None else n_recv)
            assert off.dtype == np.int32 and off.shape == (B, N + 1)
            assert np.array_equal(off, loff)
            for b in range(B):
                assert np.array_equal(rev[b], lrev[b])
            if n_recv is None:
                assert np.array_equal(off[:, N], cnt.sum(1))
