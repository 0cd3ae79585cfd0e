"""PropModuleDiffDen.forward (model/gnn_dyn.py:147-198) restated in numpy float64 from the weight dict and receiver-major
neighbour lists, with every intermediate: the host yardstick the device's float64 evaluation (csrc/k_prop_f64.h) is held
against.  The reference's own formulation, not the factored one of oracle/propnet_sparse.py: the relation propagator runs
over cat[relation_encode, effect_r, effect_s, dens], the particle propagator over cat[particle_encode, agg, dens].

Taps (the device's names and layouts, Engine.f64_tap): particle_encode [B,N,64], relation_encode [B,N,10,64] (zeros past a
receiver's count), effect_rel_p [B,N,10,64], agg_p [B,N,64], effect_p [B,N,64] for p = 0..2, particle_pred [B,N,3]."""
import numpy as np

K = 10
PSTEP = 3
TAPS = (['particle_encode', 'relation_encode'] + ['%s_%d' % (t, p) for p in range(PSTEP) for t in ('effect_rel', 'agg', 'effect')]
        + ['particle_pred'])


def weights64(W):
    """{'model....': array} (or an npz with 'w/' prefixes) -> the same in float64 (an fp32 value widens exactly)"""
    keys = W.files if hasattr(W, 'files') else W.keys()
    out = {}
    for k in keys:
        kk = k[2:] if k.startswith('w/') else k
        if kk.startswith('model.'):
            v = np.asarray(W[k])
            assert v.dtype == np.float32, (k, v.dtype)
            out[kk] = v.astype(np.float64)
    return out


def _lin(x, W, name):
    return x @ W[name + '.weight'].T + W[name + '.bias']


def forward64(W, a_cur, s_cur, s_delta, dens, nbr_idx, nbr_cnt, taps=None):
    """W: weights64(...); a_cur [B,N], s_cur / s_delta [B,N,3], dens [B] fp32; lists nbr_idx [B,N,10], nbr_cnt [B,N]
    -> s_pred [B,N,3] float64"""
    for v in (a_cur, s_cur, s_delta, dens):
        assert np.asarray(v).dtype == np.float32
    a, s, sd = [np.asarray(v).astype(np.float64) for v in (a_cur, s_cur, s_delta)]
    B, N = a.shape
    d = np.asarray(dens).astype(np.float64) / 5000.0                                  # :158
    relu = lambda x: np.maximum(x, 0.0)
    cnt = np.asarray(nbr_cnt).astype(np.int64)
    valid = np.arange(K)[None, None, :] < cnt[:, :, None]                            # [B,N,K]
    send = np.where(valid, np.asarray(nbr_idx).astype(np.int64), 0)
    assert send.min() >= 0 and send.max() < N
    bidx = np.arange(B)[:, None, None]
    dn = np.broadcast_to(d[:, None, None], (B, N, 1))
    de = np.broadcast_to(d[:, None, None, None], (B, N, K, 1))
    vm = valid[..., None]

    h = relu(_lin(np.concatenate([sd, a[..., None], dn], 2), W, 'model.particle_encoder.model.0'))      # :174-175
    pe = relu(_lin(h, W, 'model.particle_encoder.model.2'))
    a_r = np.broadcast_to(a[:, :, None, None], (B, N, K, 1))
    x = np.concatenate([a_r, a[bidx, send][..., None], s[:, :, None, :] - s[bidx, send], de], 3)      # :166-171,:179-180
    h = relu(_lin(x, W, 'model.relation_encoder.model.0'))
    h = relu(_lin(h, W, 'model.relation_encoder.model.2'))
    re = np.where(vm, relu(_lin(h, W, 'model.relation_encoder.model.4')), 0.0)
    if taps is not None:
        taps.update(particle_encode=pe, relation_encode=re)
    eff = pe
    for p in range(PSTEP):
        eff_r = np.broadcast_to(eff[:, :, None, :], (B, N, K, 64))                   # :183-184
        erel = relu(_lin(np.concatenate([re, eff_r, eff[bidx, send], de], 3), W, 'model.relation_propagator.linear'))
        erel = np.where(vm, erel, 0.0)
        agg = np.zeros((B, N, 64))
        for k in range(K):                                                           # :189, a receiver's entries in slot order
            agg = agg + erel[:, :, k]
        eff = relu(_lin(np.concatenate([pe, agg, dn], 2), W, 'model.particle_propagator.linear') + eff)   # :191-193, :82-85
        if taps is not None:
            taps['effect_rel_%d' % p] = erel
            taps['agg_%d' % p] = agg
            taps['effect_%d' % p] = eff
    h = relu(_lin(eff, W, 'model.particle_predictor.linear_0'))                       # :196, :110
    pred = _lin(h, W, 'model.particle_predictor.linear_1')
    if taps is not None:
        taps['particle_pred'] = pred
    return pred + s                                                                  # :198
