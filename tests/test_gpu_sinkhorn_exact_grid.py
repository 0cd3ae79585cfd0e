"""GPU: the fp32 and the float64 Sinkhorn divergence are ONE computation where the fp32 cost is exact (csrc/k_sinkhorn.h: the two
differ only in the points view that forms C_ij and in the gradient's last rounding).

Inputs: tests/_match_f64_ref.grid_case -- every coordinate an integer times 2^-6 (integers 0..3, one target moved by half a step),
(B, N, M) = (2, 12, 14) with ragged counts (10, 12) x (14, 7) and duplicated rows.  A difference is then an integer multiple of
2^-7 of magnitude at most 7, a square an integer multiple of 2^-14 of at most 49 of them and the sum of three at most 147: all
far inside fp32's 24 bits, so the fp32 view's differences and costs, widened, ARE the float64 view's.  Everything behind the cost
is the same double operations in the same order in both kernels (same PARTS by the counts, same butterfly, same exp and log), so
  terms, duals, col_err, self_err and transported are bit-identical, and
  the fp32 gradient is the float64 gradient rounded once to float32 (the device's conversion and numpy's are both
  round-to-nearest-even).
No tolerance: equality of bits.  iters = 5; without a reach and with one (rho = 4 eps, w = n_q / n_p), eps per sample."""
import numpy as np
import pytest

import _match_f64_ref as MF
from dyn_res_pile_manip_amd.engine import Engine

pytestmark = pytest.mark.gpu
ITERS = 5
EPS = np.array([2.0 ** -10, 1.5 * 2.0 ** -10])         # about the squared grid step 2^-12 times four and six
KW = dict(want_grad=True, want_dual=True, want_col_err=True, want_self_err=True)


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)                       # no weights: the metric needs none
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize('reach', [False, True])
def test_fp32_and_float64_agree_bit_for_bit_on_an_exact_grid(eng, reach):
    p, q, n_p, n_q = MF.grid_case()
    p32 = p.astype(np.float32)
    assert p.shape == (2, 12, 3) and q.shape == (2, 14, 3) and np.array_equal(p32.astype(np.float64), p)
    assert np.array_equal(np.round(p * 64), p * 64) and np.array_equal(np.round(q.astype(np.float64) * 128), q.astype(np.float64) * 128)
    kw = dict(KW)
    if reach:
        kw.update(reach=4.0 * EPS, mass_q=n_q / n_p.astype(np.float64), want_transported=True)
    lo = eng.cloud_divergence(p32, q, n_p, n_q, eps=EPS, iters=ITERS, **kw)
    hi = eng.cloud_divergence_f64(p, q, n_p, n_q, eps=EPS, iters=ITERS, **kw)
    assert sorted(lo) == sorted(hi) and ('transported' in lo) == reach
    assert lo['grad'].dtype == np.float32 and hi['grad'].dtype == np.float64
    for k in sorted(lo):
        if k != 'grad':
            assert lo[k].dtype == np.float64 and np.array_equal(bits(lo[k]), bits(hi[k])), (k, lo[k], hi[k])
    assert np.array_equal(bits(lo['grad']), bits(hi['grad'].astype(np.float32))), np.abs(lo['grad'] - hi['grad']).max()
    # the case is no empty one: the values and the gradient are numbers, the gradient is there on real rows and +0.0 on padding
    assert np.all(np.isfinite(lo['divergence'])) and np.all(np.isfinite(hi['grad']))
    assert np.abs(lo['grad'][0, :10]).max() > 0 and not bits(lo['grad'][0, 10:]).any()
