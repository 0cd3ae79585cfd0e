"""TEST INFRASTRUCTURE of the unbalanced Sinkhorn divergence (drp_cloud_divergence_unbalanced, drp_train_step_divergence_unbalanced;
csrc/k_sinkhorn.h: kd_sweeps_unbalanced): include/drp.h's definition in numpy float64, operation for operation, on
tests/_divergence_ref.py's helpers.  The terms of every sum are added in ascending index.

  reach (rho) > 0 in eps's unit, the target's total mass w:  a = 1 / n_p, b = w / n_q, lambda = rho / (rho + eps)
  sinkhorn64(C, eps, rho, w, K)        the cross problem's damped sweeps -> (f, g)
  self64(x, eps, rho, mass, K)         the damped, averaged Jacobi sweeps of one cloud with per-row mass `mass` -> (h, S, C, d)
  pair64(p, q, eps, rho, w, K, scale)  one pair of real rows -> (value, gradient, f, g, h_p, h_q, col_err, self_err [2], transported)
  divergence64(p, q, n_p, n_q, eps, rho, w, K)    a padded batch
  train_divergence64(...)              _divergence_ref.train_divergence64: the surrogate it differentiates is the same expression in
                                       the plans it is fed

reach = inf (with w = 1, anything else is refused) calls the balanced code of tests/_divergence_ref.py: the same bits, and
transported = the sum of a over the rows."""
import numpy as np

import _divergence_ref as D
import _transport_ref as T
from _divergence_ref import _cost_and_diff, _rows_asc, _sum_asc

MIN_REACH_PER_EPS = 1.0 / 1024.0
MASS_RANGE = (0.125, 8.0)

train_divergence64 = D.train_divergence64


def check_params(eps, rho, w):
    """the ranges include/drp.h refuses outside of"""
    if not (eps > 0 and np.isfinite(eps)):
        raise ValueError('eps=%r is not a positive finite number' % (eps,))
    if not (rho == np.inf or (np.isfinite(rho) and rho >= eps * MIN_REACH_PER_EPS)):
        raise ValueError('rho=%r is neither +inf nor a finite number of at least eps/1024' % (rho,))
    if not (MASS_RANGE[0] <= w <= MASS_RANGE[1]):
        raise ValueError('mass_q=%r outside %r..%r' % ((w,) + MASS_RANGE))
    if rho == np.inf and w != 1.0:
        raise ValueError('mass_q=%r with rho=+inf: balanced transport needs equal masses' % (w,))


def sinkhorn64(C, eps, rho, w, K):
    C = np.asarray(C, np.float64)
    n, m = C.shape
    lam = rho / (rho + eps)
    log_a, log_b = np.log(1.0 / n), np.log(w / m)
    f, g = np.zeros(n), np.zeros(m)
    for _ in range(int(K)):
        g = lam * (-eps * T._lse_rows((f[:, None] - C) / eps + log_a))
        f = lam * (-eps * T._lse_rows((g[:, None] - C.T) / eps + log_b))
    return f, g


def self64(x, eps, rho, mass, K, wide=False):
    C, d = _cost_and_diff(x, x, wide)
    n = C.shape[0]
    lam = rho / (rho + eps)
    log_m = np.log(mass)
    h = np.zeros(n)
    for _ in range(int(K)):
        h = 0.5 * (h + lam * (-eps * T._lse_rows((h[:, None] - C) / eps + log_m)))     # every h on the right: the previous sweep's
    S = (mass * mass) * np.exp((h[:, None] + h[None, :] - C) / eps)
    return h, S, C, d


def _cols_asc(P):
    return _rows_asc(P.T)


def pair64(p, q, eps, rho, w, K, scale=1.0, p64=None, want_plans=False):
    """one pair of real rows -> (value, grad [n, 3] float64 before the fp32 rounding, f, g, h_p, h_q, col_err, self_err [2],
    transported)[+ (P, S_p)].  p64: the point the value is differentiated at where it is not the float32 p (central differences)"""
    eps, rho, w = float(eps), float(rho), float(w)
    check_params(eps, rho, w)
    if rho == np.inf:
        out = D.pair64(p, q, eps, K, scale, p64=p64, want_plans=want_plans)
        n = len(p64 if p64 is not None else p)
        return out[:8] + (_sum_asc(np.full(n, 1.0 / n)),) + out[8:]
    wide = p64 is not None
    pp = p64 if wide else p
    C, d = _cost_and_diff(pp, q, wide)
    n, m = C.shape
    a, b = 1.0 / n, w / m
    f, g = sinkhorn64(C, eps, rho, w, K)
    P = (a * b) * np.exp((f[:, None] + g[None, :] - C) / eps)
    h_p, S_p, _, d_pp = self64(pp, eps, rho, a, K, wide)
    h_q, S_q, _, _ = self64(q, eps, rho, b, K, wide)
    cross = _sum_asc(np.concatenate([a * -np.expm1(-f / rho), b * -np.expm1(-g / rho)]))
    total = cross - _sum_asc(a * -np.expm1(-h_p / rho)) - _sum_asc(b * -np.expm1(-h_q / rho))
    value = scale * (((rho + 0.5 * eps) * total) / 3.0)
    grad = (2.0 * scale / 3.0) * (_rows_asc(P[:, :, None] * d) - _rows_asc(S_p[:, :, None] * d_pp))
    col_err = _sum_asc(np.abs(_cols_asc(P) - b * np.exp(-g / rho)))
    self_err = np.array([_sum_asc(np.abs(_rows_asc(S_p) - a * np.exp(-h_p / rho))),
                         _sum_asc(np.abs(_rows_asc(S_q) - b * np.exp(-h_q / rho)))])
    transported = _sum_asc(a * np.exp(-f / rho))
    out = (value, grad, f, g, h_p, h_q, col_err, self_err, transported)
    return out + (P, S_p) if want_plans else out


def divergence64(p, q, n_p, n_q, eps, rho, w, K, scale=1.0):
    """p [B, N, 3], q [B, M, 3] float32 with n_p, n_q real rows; eps, rho, w numbers or [B] -> _divergence_ref.divergence64's
    dict plus 'transported' [B]"""
    p, q = np.asarray(p, np.float32), np.asarray(q, np.float32)
    B, N, M = p.shape[0], p.shape[1], q.shape[1]
    eps, rho, w = (np.broadcast_to(np.asarray(v, np.float64).reshape(-1), (B,)) for v in (eps, rho, w))
    out = {'divergence': np.zeros(B), 'grad': np.zeros((B, N, 3)), 'f': np.zeros((B, N)), 'g': np.zeros((B, M)),
           'h_p': np.zeros((B, N)), 'h_q': np.zeros((B, M)), 'col_err': np.zeros(B), 'self_err': np.zeros((B, 2)),
           'transported': np.zeros(B)}
    for b in range(B):
        n, m = int(n_p[b]), int(n_q[b])
        value, grad, f, g, h_p, h_q, ce, se, tr = pair64(p[b, :n], q[b, :m], eps[b], rho[b], w[b], K, scale)
        out['divergence'][b], out['col_err'][b], out['self_err'][b], out['transported'][b] = value, ce, se, tr
        out['grad'][b, :n], out['f'][b, :n], out['g'][b, :m], out['h_p'][b, :n], out['h_q'][b, :m] = grad, f, g, h_p, h_q
    return out


# ---- the half-seen pile of DESIGN.md 9 ------------------------------------------------------------------------------------
HALF_SEEN_COLS, HALF_SEEN_ROWS, HALF_SEEN_FROM = 12, 6, 6


def half_seen_pile(seed=0):
    """-> (p [72, 3], q [36, 3], col [72]): the prediction is a 12 x 6 grid (12 columns of 6) of spacing 0.02 with 0.002 jitter,
    the target the same points without columns 6..11 -- a correct prediction of a pile whose far half was not observed; col:
    the column of every predicted row"""
    ij = np.stack(np.meshgrid(np.arange(HALF_SEEN_COLS), np.arange(HALF_SEEN_ROWS), indexing='ij'), -1).reshape(-1, 2)
    base = np.concatenate([0.2 + D.GRID_SPACING * ij, np.full((len(ij), 1), 0.5)], axis=1)
    p = (base + 0.1 * D.GRID_SPACING * np.random.default_rng(seed).standard_normal(base.shape)).astype(np.float32)
    return p, p[ij[:, 0] < HALF_SEEN_FROM].copy(), ij[:, 0].copy()


def column_norms(grad, col):
    """mean gradient norm of every column -> [12]"""
    norm = np.sqrt((np.asarray(grad, np.float64) ** 2).sum(-1))
    return np.array([norm[col == c].mean() for c in range(HALF_SEEN_COLS)])
