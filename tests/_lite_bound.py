"""A componentwise forward running error bound, in numpy float64, of one predict_one_step on the `lite` engine (include/drp.h:
DRP_ENGINE_LITE) against the float64 evaluation, and a float64 restatement of the engine's quantisation for the host test.

TWO STATEMENTS.  lite_bound: a sound worst case, which no arithmetic that stays finite can leave (it grows by the norm of |W|
per layer and ends far above the displacement itself: it documents the roundings, it does not discriminate).  lite_ceiling
(further down): a first-order statistical estimate of the same roundings times a stated margin, a few 1e-3 of the displacement:
the limit a wrong operand breaks.  The tests assert both.

WHAT IS BOUNDED.  |s_pred_lite - s_pred_f64| per particle and component.  The exact quantities are the float64 evaluation's:
its taps where one exists (Engine.f64_tap: particle_encode, relation_encode, effect_rel_p, agg_p, effect_p, particle_pred), and
the hidden layers no tap holds recomputed here in float64 from the same weights, inputs and lists.  The errors are propagated
through the FACTORED formulation the kernels compute (csrc/k_mlp_split.h):
    c_node = W_ppe pe + b_pp + d w_d        P_r | P_s = (W_r | W_s) eff        q = W_e relation_encode
    erel   = relu(q + b_rp + d w_d' + P_r[i] + P_s[j])      agg = sum_k erel      eff' = relu(c_node + W_agg agg + eff)
    s_pred = W_1 relu(W_0 eff_3 + b_0) + b_1 + s

DERIVATION, per linear layer y = W x + c0 with the computed input x~ = x + e (|e| <= err_in, componentwise):
  the kernel multiplies W^ (the weight as stored) by x^ (the input as converted) and accumulates in fp32.  Exactly,
      |W^ x^ - W x| <= |W^| |x^ - x| + |W^ - W| |x|,      |x^ - x| <= e + u_x (|x| + e) + f_x,      |W^ - W| <= u_w |W| + f_w,
  whose first-order reading is the issue's   err_out <= |W| err_in + (u_w + u_x + u_w u_x) |W| |x| + gamma_k |W| |x| + floor;
  the code evaluates the exact inequality (the second-order terms are below 2^-9 of the first-order ones) so that the bound is
  sound, not approximately so.  ReLU is 1-Lipschitz, the gather moves errors with their rows, the segmented sum is linear.
  CHAIN (relation encoder's three layers and W_e; one product W_hi x_hi per k-step):
      u_x = 2^-10   activations rounded TOWARD ZERO to fp16 (v_cvt_pkrtz_f16_f32): 11 significant bits, error < one unit = 2^-10 |x|
      u_w = 2^-11   weights rounded to NEAREST fp16 on the host (host_f16_rne): half a unit
      floor         below fp16's normal range (2^-14) the spacing is 2^-24: f_x = 2^-24 (toward zero), f_w = 2^-25 (nearest), in
                    the scale the operand is converted in.  The hidden activations and the first layer's weights travel times
                    2^k, k = range_info()['shift'], so in unshifted units f_x = 2^-24 2^-k for the hidden layers (2^-24 for the
                    first layer's inputs, which are not shifted) and f_w = 2^-25 2^-k for the first layer (2^-25 for the others).
      The products are exact in fp32 (11 x 11 bits).
  NODE LAYERS (particle encoder, W_ppe, W_agg, W_r | W_s, predictor layer 0; bf16 terms w = w0 + w1 + r_w, x = p0 + p1 + r_x, each
  term rounded to nearest: |r| <= 2^-18 |.|, |w1|, |p1| <= (2^-9 + 2^-18) |.|; products w0 p0 + w0 p1 + w1 p0 = (w0 + w1)(p0 + p1) - w1 p1):
      |w x - (w0 p0 + w0 p1 + w1 p0)| <= |w r_x| + |r_w x| + |r_w r_x| + |w1 p1| <= (3 2^-18 + 2^-26 + 2^-35) |w| |x| <= U_NODE |w| |x|,
      U_NODE = 2^-16 + 3 2^-24, the issue's constant (the dropped cross and third terms).  bf16 has fp32's exponent range: no floor.
  ACCUMULATION.  gamma_n = n u / (1 - n u) over the n additions of an accumulator (k products per term count, plus the initial
      value), u = 2^-23: one unit in the last place per addition whatever the matrix pipe's rounding direction inside a k-step.
  FP32 GLUE (the bias rows, b + d w_d, q 2^-k + (...), the sums over the slots, the residual, the predictor's fp32 dot product,
      dens / 5000 and s_i - s_j in fp32 where float64 has them exact): gamma_m of the magnitudes added, m the number of operations.
  SELF EDGE.  Engine.step prepares no self-edge constant, so its self edges run the chain like any other edge and are bounded
      like one.  Rows named in `self_const` (rollouts with uniform attributes: k_cself) carry the fused engine's term only: the
      plain fp32 chain's gamma bound.
  The float64 evaluation itself is within 1e-10 of its largest value (tests/test_gpu_f64.py: TOL): added.
Every constant above is a property of the number formats or of the instruction sequence; none is measured."""
import numpy as np

import _f64_ref as R

K = R.K
PSTEP = R.PSTEP
U_X = 2.0 ** -10
U_W = 2.0 ** -11
U_NODE = 2.0 ** -16 + 3 * 2.0 ** -24
U32 = 2.0 ** -23          # per addition (see ACCUMULATION)
U24 = 2.0 ** -24          # one correctly rounded fp32 operation
F64_TOL = 1e-10


def gamma(n, u=U32):
    return n * u / (1.0 - n * u)


def _split_weights(W):
    """the matrices of the factored formulation, float64"""
    rp, pp = W['model.relation_propagator.linear.weight'], W['model.particle_propagator.linear.weight']
    return dict(
        pe0=np.concatenate([W['model.particle_encoder.model.0.weight'], W['model.particle_encoder.model.0.bias'][:, None]], 1),
        pe2=W['model.particle_encoder.model.2.weight'], b_pe2=W['model.particle_encoder.model.2.bias'],
        re0=np.concatenate([W['model.relation_encoder.model.0.weight'], W['model.relation_encoder.model.0.bias'][:, None]], 1),
        re2=W['model.relation_encoder.model.2.weight'], b_re2=W['model.relation_encoder.model.2.bias'],
        re4=W['model.relation_encoder.model.4.weight'], b_re4=W['model.relation_encoder.model.4.bias'],
        rpe=rp[:, :64], rpr=rp[:, 64:128], rps=rp[:, 128:192], wd_rp=rp[:, 192], b_rp=W['model.relation_propagator.linear.bias'],
        ppe=pp[:, :64], agg=pp[:, 64:128], wd_pp=pp[:, 128], b_pp=W['model.particle_propagator.linear.bias'],
        pr0=W['model.particle_predictor.linear_0.weight'], b_pr0=W['model.particle_predictor.linear_0.bias'],
        pr1=W['model.particle_predictor.linear_1.weight'], b_pr1=W['model.particle_predictor.linear_1.bias'])


# ---- the two layer rules ------------------------------------------------------------------------------------------
def chain_layer(Wm, x, e, f_x, f_w, c0_abs=0.0, e_c0=0.0, u_x=U_X, u_w=U_W):
    """error bound of W^ x^ + c0 (one fp16 product per k-step, fp32 accumulation) against W x + c0; x, e [..., in]"""
    Wa = np.abs(Wm)
    dW = u_w * Wa + f_w
    Wh = Wa + dW
    xa = np.abs(x)
    dx = e + u_x * (xa + e) + f_x
    lin = dx @ Wh.T + xa @ dW.T
    mag = (xa + dx) @ Wh.T + c0_abs + e_c0
    return lin + e_c0 + gamma(Wm.shape[1] + 1) * mag


def node_layer(Wm, x, e, c0_abs=0.0, e_c0=0.0, u_node=U_NODE):
    """error bound of the three-product bf16 form of W x~ + c0 against W x + c0"""
    Wa = np.abs(Wm)
    xt = np.abs(x) + e
    lin = e @ Wa.T + u_node * (xt @ Wa.T)
    mag = (1.0 + u_node) * (xt @ Wa.T) + c0_abs + e_c0
    return lin + e_c0 + gamma(3 * Wm.shape[1] + 1) * mag


def fp32_layer(Wm, x, e, c0_abs=0.0, e_c0=0.0):
    """error bound of a plain fp32 fma chain W x~ + c0 (k_cself, the predictor's last layer)"""
    Wa = np.abs(Wm)
    xt = np.abs(x) + e
    return e @ Wa.T + e_c0 + gamma(Wm.shape[1] + 1, U24) * (xt @ Wa.T + c0_abs + e_c0)


# ---- the bound ------------------------------------------------------------------------------------------------------
def lite_bound(W, a_cur, s_cur, s_delta, dens, nbr_idx, nbr_cnt, taps, shift, self_const=None, u_x=U_X, u_w=U_W, u_node=U_NODE):
    """W: _f64_ref.weights64(...); the step's fp32 inputs and lists; taps: {name: float64 array} of the float64 evaluation of
    the same step (Engine.f64_tap / _f64_ref.forward64); shift: range_info()['shift']; self_const: [B] bool or None
    -> bound [B,N,3] float64 on |s_pred_lite - s_pred_f64|"""
    M = _split_weights(W)
    a, s, sd = [np.asarray(v).astype(np.float64) for v in (a_cur, s_cur, s_delta)]
    B, N = a.shape
    d = np.asarray(dens).astype(np.float64) / 5000.0
    e_d = U24 * np.abs(d)                                              # dens / 5000 in fp32
    relu = lambda v: np.maximum(v, 0.0)
    cnt = np.asarray(nbr_cnt).astype(np.int64)
    valid = np.arange(K)[None, None, :] < cnt[:, :, None]
    send = np.where(valid, np.asarray(nbr_idx).astype(np.int64), 0)
    bidx = np.arange(B)[:, None, None]
    two_k = 2.0 ** -shift                                              # a shifted-scale quantity in unshifted units
    dn = np.broadcast_to(d[:, None, None], (B, N, 1))
    e_dn = np.broadcast_to(e_d[:, None, None], (B, N, 1))
    one_n = np.ones((B, N, 1))
    zero_n = np.zeros((B, N, 1))

    # particle encoder, node constant (node layers)
    x = np.concatenate([sd, a[..., None], dn, one_n], 2)
    e_x = np.concatenate([np.zeros((B, N, 4)), e_dn, zero_n], 2)
    h = relu(x @ M['pe0'].T)
    e_h = node_layer(M['pe0'], x, e_x, u_node=u_node)
    pe = taps['particle_encode']
    e_pe = node_layer(M['pe2'], h, e_h, np.abs(M['b_pe2']), u_node=u_node)
    c0 = np.abs(M['b_pp']) + np.abs(dn * M['wd_pp'])
    e_c0 = e_dn * np.abs(M['wd_pp']) + gamma(2, U24) * c0
    c_node = pe @ M['ppe'].T + M['b_pp'] + dn * M['wd_pp']
    e_cnode = node_layer(M['ppe'], pe, e_pe, c0, e_c0, u_node=u_node)

    # relation encoder chain per edge slot -> q = W_e relation_encode
    de = np.broadcast_to(d[:, None, None, None], (B, N, K, 1))
    e_de = np.broadcast_to(e_d[:, None, None, None], (B, N, K, 1))
    dpos = s[:, :, None, :] - s[bidx, send]
    xr = np.concatenate([np.broadcast_to(a[:, :, None, None], (B, N, K, 1)), a[bidx, send][..., None], dpos, de, np.ones((B, N, K, 1))], 3)
    e_xr = np.concatenate([np.zeros((B, N, K, 2)), U24 * np.abs(dpos), e_de, np.zeros((B, N, K, 1))], 3)
    kw = dict(u_x=u_x, u_w=u_w)
    h1 = relu(xr @ M['re0'].T)
    e_h1 = chain_layer(M['re0'], xr, e_xr, 2.0 ** -24, 2.0 ** -25 * two_k, **kw)
    h2 = relu(h1 @ M['re2'].T + M['b_re2'])
    e_h2 = chain_layer(M['re2'], h1, e_h1, 2.0 ** -24 * two_k, 2.0 ** -25, np.abs(M['b_re2']), **kw)
    re = taps['relation_encode']
    e_re = chain_layer(M['re4'], h2, e_h2, 2.0 ** -24 * two_k, 2.0 ** -25, np.abs(M['b_re4']), **kw)
    q = re @ M['rpe'].T
    bd = np.abs(M['b_rp']) + np.abs(de * M['wd_rp'])                   # |b_rp| + |d w_d'|, per edge
    e_bd = e_de * np.abs(M['wd_rp'])
    if self_const is not None:
        # the fused engine's self-edge term: the chain in plain fp32 on [a, a, 0, 0, 0, d, 1]
        xs = np.concatenate([a[..., None], a[..., None], np.zeros((B, N, 3)), dn, one_n], 2)
        e_xs = np.concatenate([np.zeros((B, N, 5)), e_dn, zero_n], 2)
        g1 = relu(xs @ M['re0'].T)
        e_g1 = fp32_layer(M['re0'], xs, e_xs)
        g2 = relu(g1 @ M['re2'].T + M['b_re2'])
        e_g2 = fp32_layer(M['re2'], g1, e_g1, np.abs(M['b_re2']))
        g3 = relu(g2 @ M['re4'].T + M['b_re4'])
        e_g3 = fp32_layer(M['re4'], g2, e_g2, np.abs(M['b_re4']))
        e_qself = fp32_layer(M['rpe'], g3, e_g3)

    # propagation steps
    eff, e_eff = pe, e_pe
    for p in range(PSTEP):
        pr, ps = eff @ M['rpr'].T, eff @ M['rps'].T
        e_pr = node_layer(M['rpr'], eff, e_eff, u_node=u_node)
        e_ps = node_layer(M['rps'], eff, e_eff, u_node=u_node)
        # the chain's last layer starts from 2^k (b + d w_d' + P_r[i]); the sender's row is added with the unshift
        c0 = bd + np.abs(pr)[:, :, None, :]
        e_c0 = e_bd + e_pr[:, :, None, :] + gamma(3, U24) * c0
        e_q = chain_layer(M['rpe'], re, e_re, 2.0 ** -24 * two_k, 2.0 ** -25, c0, e_c0, **kw)
        ps_j, e_ps_j = ps[bidx, send], e_ps[bidx, send]
        mag = np.abs(q) + c0 + np.abs(ps_j)
        e_erel = e_q + e_ps_j + gamma(4, U24) * (mag + e_q + e_ps_j)
        if self_const is not None:
            # the entry of a row that is the row itself, in a sample that has the constant
            is_self = np.asarray(self_const, bool)[:, None, None] & valid & (send == np.arange(N)[None, :, None])
            e_self = e_qself[:, :, None, :] + e_c0 + e_ps_j + gamma(4, U24) * (mag + e_qself[:, :, None, :] + e_ps_j)
            e_erel = np.where(is_self[..., None], e_self, e_erel)
        e_erel = np.where(valid[..., None], e_erel, 0.0)
        erel = taps['effect_rel_%d' % p]
        agg = taps['agg_%d' % p]
        e_agg = e_erel.sum(2) + gamma(K + 1, U24) * (erel.sum(2) + e_erel.sum(2))       # erel >= 0
        c0 = np.abs(c_node) + np.abs(eff)
        e_c0 = e_cnode + e_eff + gamma(2, U24) * (c0 + e_cnode + e_eff)
        e_eff = node_layer(M['agg'], agg, e_agg, c0, e_c0, u_node=u_node)
        eff = taps['effect_%d' % p]

    # predictor
    hp = relu(eff @ M['pr0'].T + M['b_pr0'])
    e_hp = node_layer(M['pr0'], eff, e_eff, np.abs(M['b_pr0']), u_node=u_node)
    pred = taps['particle_pred']
    sa = np.abs(s)
    e_out = fp32_layer(M['pr1'], hp, e_hp, np.abs(M['b_pr1']) + sa)
    e_out = e_out + gamma(3, U24) * (np.abs(pred) + sa + e_out)
    return e_out + F64_TOL * max(np.abs(pred + s).max(), 1e-300)


# ---- the first-order estimate: what the error should BE, not what it cannot exceed -------------------------------------
# The worst case above grows by the norm of |W| at every layer and by ten at every aggregation: through fourteen layers it ends
# orders of magnitude above any error the arithmetic can make, so it cannot tell a correct kernel from one that feeds a wrong
# operand.  The ceiling the tests assert beside it is a first-order statistical statement of the SAME roundings:
#   chain, activation:  x^ = x~ (1 - delta), delta uniform on [0, u_x)  (toward zero: one sign)  -> mean -(u_x / 2) x~, variance (u_x^2 / 12) x~^2
#   chain, weight:      W^ = W (1 + eps), eps uniform on [-u_w, u_w]                              -> mean 0, variance (u_w^2 / 3) W^2
#   node layers:        the dropped terms, within +-U_NODE |w| |x|, uniform                       -> mean 0, variance (U_NODE^2 / 3) W^2 x^2
# propagated to first order through the factored formulation: a linear layer maps the mean error mu through W and adds
# -(u_x / 2) W x (the common shrink of every input is a shrink of the exact product), and the variance v through W^2 (errors of
# different inputs taken as independent) plus the per-product variances; ReLU passes both where the exact pre-activation is
# positive; the gather moves them with their rows; in the sum over a receiver's slots the sender terms add as independent, the
# receiver's own term P_r[i], common to all its slots, adds coherently (count^2).  Not modelled: correlations between the
# features of one row (they share their inputs' errors) and between the propagation steps (the chain's output is the same in
# all three); sign changes of a pre-activation under the error; fp32 rounding (2^-24 against 2^-10).  LITE_SIGMAS pays for them.
# The asserted ceiling on a component is   LITE_SIGMAS max(|mu| + sqrt(v), r) + 4 2^-24 (|s_pred| + |pred|) + F64_TOL max|s_pred|,
# r = the root mean square of sqrt(mu^2 + v) over the components of its sample: a pre-activation whose sign the error changes
# moves an error of the sample's typical size into a component whose own estimate may be far smaller, so a component's
# estimate is not trusted below that size.
# six standard deviations put a Gaussian tail below 2e-9 per component (the tests look at fewer than 1e6), doubled to twelve for
# what the model leaves out (three equal, fully correlated contributions where it assumes independent ones are a factor sqrt(3));
# the second term is the output's own fp32 roundings (the sum pred + b + s and its store).  A wrong operand -- the low half of a
# weight, a dropped layer, a missing term -- is an error of the order of the displacement: hundreds of these standard deviations.
LITE_SIGMAS = 12.0


def _lin_stat(Wm, x, mu, v, q_var, shrink):
    """first-order mean / variance of the error of W x^ against W x: inputs' (mu, v), per-product relative variance q_var,
    relative shrink of every input `shrink` (u_x / 2 toward zero, 0 for rounding to nearest)"""
    W2 = Wm * Wm
    return mu @ Wm.T - shrink * (x @ Wm.T), v @ W2.T + q_var * ((x * x) @ W2.T)


def lite_estimate(W, a_cur, s_cur, s_delta, dens, nbr_idx, nbr_cnt, taps, self_const=None, u_x=U_X, u_w=U_W, u_node=U_NODE):
    """-> (mu, v) [B,N,3]: first-order mean and variance of s_pred_lite - s_pred_f64 (see above); arguments as lite_bound's"""
    M = _split_weights(W)
    a, s, sd = [np.asarray(v_).astype(np.float64) for v_ in (a_cur, s_cur, s_delta)]
    B, N = a.shape
    d = np.asarray(dens).astype(np.float64) / 5000.0
    cnt = np.asarray(nbr_cnt).astype(np.int64)
    valid = np.arange(K)[None, None, :] < cnt[:, :, None]
    send = np.where(valid, np.asarray(nbr_idx).astype(np.int64), 0)
    bidx = np.arange(B)[:, None, None]
    dn = np.broadcast_to(d[:, None, None], (B, N, 1))
    de = np.broadcast_to(d[:, None, None, None], (B, N, K, 1))
    qc, sh = u_x * u_x / 12.0 + u_w * u_w / 3.0, u_x / 2.0
    qn = u_node * u_node / 3.0
    gate = lambda y, mu, v: (np.where(y > 0, mu, 0.0), np.where(y > 0, v, 0.0))

    x = np.concatenate([sd, a[..., None], dn, np.ones((B, N, 1))], 2)
    y = x @ M['pe0'].T
    mu, v = gate(y, *_lin_stat(M['pe0'], x, 0.0 * x, 0.0 * x, qn, 0.0))
    h = np.maximum(y, 0.0)
    y = h @ M['pe2'].T + M['b_pe2']
    mu_pe, v_pe = gate(y, *_lin_stat(M['pe2'], h, mu, v, qn, 0.0))
    pe = taps['particle_encode']
    mu_cn, v_cn = _lin_stat(M['ppe'], pe, mu_pe, v_pe, qn, 0.0)
    c_node = pe @ M['ppe'].T + M['b_pp'] + dn * M['wd_pp']

    xr = np.concatenate([np.broadcast_to(a[:, :, None, None], (B, N, K, 1)), a[bidx, send][..., None], s[:, :, None, :] - s[bidx, send],
                         de, np.ones((B, N, K, 1))], 3)
    y = xr @ M['re0'].T
    mu, v = gate(y, *_lin_stat(M['re0'], xr, 0.0 * xr, 0.0 * xr, qc, sh))
    h = np.maximum(y, 0.0)
    y = h @ M['re2'].T + M['b_re2']
    mu, v = gate(y, *_lin_stat(M['re2'], h, mu, v, qc, sh))
    h = np.maximum(y, 0.0)
    y = h @ M['re4'].T + M['b_re4']
    mu, v = gate(y, *_lin_stat(M['re4'], h, mu, v, qc, sh))
    re = taps['relation_encode']
    mu_q, v_q = _lin_stat(M['rpe'], re, mu, v, qc, sh)
    if self_const is not None:                                          # those entries carry the full-precision constant
        is_self = np.asarray(self_const, bool)[:, None, None] & valid & (send == np.arange(N)[None, :, None])
        mu_q, v_q = np.where(is_self[..., None], 0.0, mu_q), np.where(is_self[..., None], 0.0, v_q)

    eff, mu_e, v_e = pe, mu_pe, v_pe
    for p in range(PSTEP):
        mu_pr, v_pr = _lin_stat(M['rpr'], eff, mu_e, v_e, qn, 0.0)
        mu_ps, v_ps = _lin_stat(M['rps'], eff, mu_e, v_e, qn, 0.0)
        on = (taps['effect_rel_%d' % p] > 0) & valid[..., None]         # the slots whose ReLU passes
        n_on = on.sum(2)
        mu_a = np.where(on, mu_q + mu_ps[bidx, send], 0.0).sum(2) + n_on * mu_pr
        v_a = np.where(on, v_q + v_ps[bidx, send], 0.0).sum(2) + n_on * n_on * v_pr
        agg = taps['agg_%d' % p]
        mu, v = _lin_stat(M['agg'], agg, mu_a, v_a, qn, 0.0)
        y = c_node + agg @ M['agg'].T + eff
        mu_e, v_e = gate(y, mu + mu_cn + mu_e, v + v_cn + v_e)
        eff = taps['effect_%d' % p]
    y = eff @ M['pr0'].T + M['b_pr0']
    mu, v = gate(y, *_lin_stat(M['pr0'], eff, mu_e, v_e, qn, 0.0))
    return mu @ M['pr1'].T, v @ (M['pr1'] * M['pr1']).T


def lite_ceiling(W, a_cur, s_cur, s_delta, dens, nbr_idx, nbr_cnt, taps, self_const=None, **kw):
    """-> [B,N,3]: the asserted ceiling on |s_pred_lite - s_pred_f64| (LITE_SIGMAS, above)"""
    mu, v = lite_estimate(W, a_cur, s_cur, s_delta, dens, nbr_idx, nbr_cnt, taps, self_const, **kw)
    s = np.asarray(s_cur).astype(np.float64)
    pred = taps['particle_pred']
    r = np.sqrt((mu * mu + v).mean(axis=(1, 2), keepdims=True))
    return (LITE_SIGMAS * np.maximum(np.abs(mu) + np.sqrt(v), r) + 4 * U24 * (np.abs(pred + s) + np.abs(pred))
            + F64_TOL * max(np.abs(pred + s).max(), 1e-300))


# ---- the engine's quantisation restated in float64 (host test) ---------------------------------------------------
def round_toward_zero(x, bits=11, emin=-14):
    """x with `bits` significant bits, rounded toward zero; below 2^emin the spacing stays 2^(emin - bits + 1) (fp16: 11, -14)"""
    x = np.asarray(x, np.float64)
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** emin)))
    e = np.where(np.abs(x) >= 2.0 ** (e + 1), e + 1, e)                # log2's own rounding at a power of two
    e = np.where(np.abs(x) < 2.0 ** e, e - 1, e)
    e = np.maximum(e, emin)
    ulp = 2.0 ** (e - bits + 1)
    return np.trunc(x / ulp) * ulp


def round_nearest(x, bits, emin=None):
    """x with `bits` significant bits, rounded to nearest even (emin: as in round_toward_zero; None: no floor)"""
    x = np.asarray(x, np.float64)
    ax = np.abs(x)
    lo = 2.0 ** emin if emin is not None else 1e-300
    e = np.floor(np.log2(np.maximum(ax, lo)))
    e = np.where(ax >= 2.0 ** (e + 1), e + 1, e)
    e = np.where((ax < 2.0 ** e) & (ax >= lo), e - 1, e)
    if emin is not None:
        e = np.maximum(e, emin)
    ulp = 2.0 ** (e - bits + 1)
    return np.rint(x / ulp) * ulp                                        # rint: half to even


def lite_model(W, a_cur, s_cur, s_delta, dens, nbr_idx, nbr_cnt, shift, x_bits=11):
    """The lite engine's arithmetic with every operand quantised as include/drp.h specifies and everything else -- the sums, the
    glue -- in float64: chain weights fp16 to nearest (the first layer's after the shift), chain activations to `x_bits`
    significant bits toward zero in the shifted scale (11: fp16; fewer: a deliberately wrong quantiser), node layers on the
    two-term bf16 split with the three products.  -> s_pred [B,N,3] float64"""
    M = _split_weights(W)
    a, s, sd = [np.asarray(v).astype(np.float64) for v in (a_cur, s_cur, s_delta)]
    B, N = a.shape
    d = np.asarray(dens).astype(np.float64) / 5000.0
    relu = lambda v: np.maximum(v, 0.0)
    cnt = np.asarray(nbr_cnt).astype(np.int64)
    valid = np.arange(K)[None, None, :] < cnt[:, :, None]
    send = np.where(valid, np.asarray(nbr_idx).astype(np.int64), 0)
    bidx = np.arange(B)[:, None, None]
    sc = 2.0 ** shift
    w16 = lambda w: round_nearest(w, 11, -14)
    x16 = lambda v: round_toward_zero(v, x_bits, -14)
    bf = lambda v: round_nearest(v, 8)

    def node(Wm, x):
        w0 = bf(Wm)
        w1 = bf(Wm - w0)
        p0 = bf(x)
        p1 = bf(x - p0)
        return p0 @ w0.T + p1 @ w0.T + p0 @ w1.T

    dn = np.broadcast_to(d[:, None, None], (B, N, 1))
    x = np.concatenate([sd, a[..., None], dn, np.ones((B, N, 1))], 2)
    pe = relu(node(M['pe2'], relu(node(M['pe0'], x))) + M['b_pe2'])
    c_node = node(M['ppe'], pe) + M['b_pp'] + dn * M['wd_pp']
    de = np.broadcast_to(d[:, None, None, None], (B, N, K, 1))
    xr = np.concatenate([np.broadcast_to(a[:, :, None, None], (B, N, K, 1)), a[bidx, send][..., None], s[:, :, None, :] - s[bidx, send],
                         de, np.ones((B, N, K, 1))], 3)
    h = relu(x16(xr) @ w16(sc * M['re0']).T)                            # shifted from here on
    h = relu(x16(h) @ w16(M['re2']).T + sc * M['b_re2'])
    h = relu(x16(h) @ w16(M['re4']).T + sc * M['b_re4'])
    q = (x16(h) @ w16(M['rpe']).T) / sc
    eff = pe
    for p in range(PSTEP):
        pr, ps = node(M['rpr'], eff), node(M['rps'], eff)
        erel = relu(q + M['b_rp'] + de * M['wd_rp'] + pr[:, :, None, :] + ps[bidx, send])
        agg = np.where(valid[..., None], erel, 0.0).sum(2)
        eff = relu(c_node + node(M['agg'], agg) + eff)
    hp = relu(node(M['pr0'], eff) + M['b_pr0'])
    return hp @ M['pr1'].T + M['b_pr1'] + s
