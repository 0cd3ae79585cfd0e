"""CPU: the host restatement of the device sampler (tests/_philox_ref.py) held to what is known independently of it -- the
published Random123 known-answer vectors of philox4x32 10, the shard identity of the counter layout, the corners of the
Box-Muller inputs and the moments of N(0, 1).  tests/test_gpu_sampler.py then holds the device to this restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _philox_ref as P  # noqa: E402

# Random123's kat_vectors, `philox4x32 10`: counter, key -> output
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize('ctr,key,want', KAT)
def test_known_answer_vectors(ctr, key, want):
    got = P.philox4x32_10(np.array(ctr, np.uint32), key[0] | (key[1] << 32))
    assert [hex(int(x)) for x in got] == [hex(x) for x in want]


def test_block_function_is_elementwise():
    """a batch of counters gives each counter's own block"""
    ctr = np.array([k[0] for k in KAT[:1]] * 3 + [(1, 2, 3, 4)], np.uint32).reshape(2, 2, 4)
    out = P.philox4x32_10(ctr, 7)
    for i in range(2):
        for j in range(2):
            np.testing.assert_array_equal(out[i, j], P.philox4x32_10(ctr[i, j], 7))
    assert not np.array_equal(out[0, 0], out[1, 1])


@pytest.mark.parametrize('base', [0, 2 ** 32 - 3 - 32, 2 ** 40 + 5])
def test_shard_identity(base):
    """a shard of a job draws what the whole job draws -- also where the low counter word wraps and the high word becomes 1"""
    seed, H, it = 2 ** 63 + 17, 3, 5
    whole = P.raw_words(seed, base, 65, H, it)
    np.testing.assert_array_equal(whole[32:], P.raw_words(seed, base + 32, 33, H, it))
    assert len({tuple(w) for w in whole.reshape(-1, 4)}) == 65 * H               # and no two (sample, t) share a block


def test_counter_words():
    """every counter word and both key words reach the block, each in its own place"""
    seed, H = 42, 3
    w = P.raw_words(seed, 2 ** 32 - 3, 5, H, 9)
    for s in range(5):
        gs = 2 ** 32 - 3 + s
        for t in range(H):
            np.testing.assert_array_equal(w[s, t], P.philox4x32_10(np.array([gs & 0xffffffff, gs >> 32, t, 9], np.uint32), seed))
    assert (w[3] != P.raw_words(seed, 0, 1, H, 9)[0]).any()                       # gs = 2^32 is not gs = 0: the high word
    np.testing.assert_array_equal(P.raw_words(seed, 0, 4, H, 2 ** 32 + 9), P.raw_words(seed, 0, 4, H, 9))    # iteration mod 2^32
    assert (P.raw_words(seed, 0, 4, H, 2 ** 31) != P.raw_words(seed, 0, 4, H, 0)).any()
    assert (P.raw_words(seed + 2 ** 32, 0, 4, H, 9) != P.raw_words(seed, 0, 4, H, 9)).any()                  # the high key word
    # t and iteration are different words
    assert (P.raw_words(seed, 0, 1, 2, 0)[0, 1] != P.raw_words(seed, 0, 1, 1, 1)[0, 0]).any()


def test_uniform24_is_exact():
    w = np.array([0, 0xff, 0x100, 0x80000000, 0xffffff00, 0xffffffff], np.uint32)
    u = P.uniform24(w)
    assert u.dtype == np.float32
    np.testing.assert_array_equal(u.astype(np.float64), (w >> 8).astype(np.float64) / 2.0 ** 24)
    assert u.min() == 0.0 and u.max() == 1.0 - 2.0 ** -24
    d = P.draws(w[2:], 'uniform')
    assert d.dtype == np.float32
    np.testing.assert_array_equal(d.astype(np.float64), 2.0 * u[2:].astype(np.float64) - 1.0)       # 2u - 1 stays exact


def test_normal_inputs_corners():
    top = 2 ** 32 - 1
    words = np.array([[0, 0, top, top],                      # a = 0: the smallest u1, the largest radius
                      [top, 0, 2 ** 32 - 128, 0x40000000],   # a >= 2^32 - 128 rounds to 2^32: u1 = 1, radius 0
                      [2 ** 32 - 129, top, 1, 0x80000000],   # just below: u1 < 1
                      [0x80000000, 0xc0000000, 0, 0x40000000]], np.uint32)
    ni = P.normal_inputs(words)
    assert ni.u1.dtype == np.float32 and ni.angle.dtype == np.float32
    assert ni.u1[0, 0] == ni.u1[0, 1] == np.float32(2.0 ** -32)
    np.testing.assert_allclose(ni.r[0, :2], np.sqrt(64 * np.log(2.0)), rtol=1e-15)
    assert abs(ni.r[0, 0] - 6.66) < 0.01 and ni.r.max() == ni.r[0, 0]
    np.testing.assert_array_equal(ni.u1[0, 2:], 1.0)
    np.testing.assert_array_equal(ni.u1[1], 1.0)
    np.testing.assert_array_equal(ni.r[1], 0.0)
    np.testing.assert_array_equal(ni.n[1], 0.0)
    assert not np.signbit(ni.r[1]).any()
    assert ni.u1[2, 0] == np.float32(1.0 - 2.0 ** -24) and ni.r[2, 0] > 0.0
    # the pair of a component: c = 0, 1 read words 0, 1; c = 2, 3 read words 2, 3; even cos, odd sin
    assert ni.u1[3, 0] == ni.u1[3, 1] == np.float32(0.5 + 2.0 ** -32) == np.float32(0.5)
    np.testing.assert_array_equal(ni.angle[3], np.float32(6.283185307179586) * np.array([0.75, 0.75, 0.25, 0.25], np.float32))
    r01, r23 = np.sqrt(2.0 * np.log(2.0)), np.sqrt(64 * np.log(2.0))
    ang = ni.angle[3].astype(np.float64)
    np.testing.assert_allclose(ni.n[3], [r01 * np.cos(ang[0]), r01 * np.sin(ang[1]), r23 * np.cos(ang[2]), r23 * np.sin(ang[3])],
                               rtol=1e-15, atol=0)
    assert abs(ni.n[3, 1] + r01) < 1e-6 and abs(ni.n[3, 3] - r23) < 1e-6 and abs(ni.n[3, 0]) < 1e-6
    for f in ni:
        assert np.isfinite(f).all()
    assert (ni.u1 > 0).all() and (ni.u1 <= 1).all() and (ni.angle >= 0).all() and (ni.angle <= np.float32(6.283185307179586)).all()


def test_corner_samples_of_the_stream():
    """the global samples the GPU test visits for the two ends of u1 hold what _philox_ref.CORNER_SAMPLES says"""
    gs, c = P.CORNER_SAMPLES['u1_one']
    w = P.raw_words(42, gs, 1, 1, 0)[0, 0]
    ni = P.normal_inputs(w)
    assert w[c] == 0xffffffbe and ni.u1[c] == ni.u1[c + 1] == 1.0 and ni.r[c] == ni.n[c] == ni.n[c + 1] == 0.0
    assert ni.r[2 - c] > 0.0
    gs, c = P.CORNER_SAMPLES['u1_small']
    w = P.raw_words(42, gs, 1, 1, 0)[0, 0]
    ni = P.normal_inputs(w)
    assert w[c] == 12 and ni.u1[c] == np.float32(13 * 2.0 ** -32) and 6.2 < ni.r[c] < 6.3


def test_normal_moments():
    """2^18 normals of the restatement: mean, standard deviation, the correlation of the two outputs of a Box-Muller pair and
    that of the two pairs of a block, each within 4 standard errors of N(0, 1)'s"""
    words = P.raw_words(1234, 0, 2 ** 14, 4, 0)
    ni = P.normal_inputs(words)
    assert np.isfinite(ni.n).all() and np.abs(ni.n).max() <= ni.r.max() <= 6.67
    z = ni.n.reshape(-1, 4)
    n = z.size
    assert n == 2 ** 18
    assert abs(z.mean()) < 4.0 / np.sqrt(n)
    assert abs(z.std() - 1.0) < 4.0 / np.sqrt(2.0 * n)
    for c in range(4):
        assert abs(z[:, c].mean()) < 4.0 / np.sqrt(n / 4) and abs(z[:, c].std() - 1.0) < 4.0 / np.sqrt(2.0 * n / 4)
    pairs = n // 4
    for c, d in ((0, 1), (2, 3), (0, 2), (1, 3)):
        assert abs(np.mean(z[:, c] * z[:, d])) < 4.0 / np.sqrt(pairs), (c, d)
    # uniforms of the same words: mean 1/2, variance 1/12
    u = P.uniform24(words).astype(np.float64).ravel()
    assert abs(u.mean() - 0.5) < 4.0 * np.sqrt(1.0 / 12.0 / u.size)
    assert abs(u.var() - 1.0 / 12.0) < 4.0 * np.sqrt(1.0 / 180.0 / u.size)


@pytest.mark.parametrize('noise_type', P.NOISE_TYPES)
def test_actions_restates_the_filter(noise_type):
    """the vectorised filter against a scalar loop of python floats (IEEE doubles), and its plain properties"""
    rng = np.random.default_rng(3)
    ns, H = 7, 4
    nominal = rng.uniform(-3, 3, (H, 4))
    lo, hi = np.array([-4.5, -4.5, -3.15, -3.15]), np.array([4.5, 4.5, 3.15, 3.15])
    d = P.draws(P.raw_words(5, 0, ns, H, 0), noise_type).astype(np.float32)
    sigma, beta = 4.0, 0.7
    got = P.actions(nominal, d, sigma, beta, lo, hi, noise_type)
    assert got.dtype == np.float32 and got.shape == (ns, H, 4)
    lo32, hi32 = [float(np.float32(x)) for x in lo], [float(np.float32(x)) for x in hi]
    for s in range(ns):
        for c in range(4):
            resid = 0.0
            for t in range(H):
                n = float(d[s, t, c])
                if noise_type == 'total_rand':
                    a = lo32[c] + n * (hi32[c] - lo32[c])
                else:
                    resid = beta * (sigma * n) + resid * (1.0 - beta)
                    a = min(max(float(nominal[t, c]) + resid, lo32[c]), hi32[c])
                assert got[s, t, c] == np.float32(a), (s, t, c)
    assert (got >= lo.astype(np.float32)).all() and (got <= hi.astype(np.float32)).all()
    if noise_type != 'total_rand':
        assert ((got == lo.astype(np.float32)) | (got == hi.astype(np.float32))).any()          # the clip is exercised
    # beta = 1, nominal 0, a box the draws stay inside: the action is the scaled draw itself
    raw = P.actions(np.zeros((H, 4)), d, 1.0 if noise_type != 'normal' else 0.125, 1.0,
                    [0.0 if noise_type == 'total_rand' else -1.0] * 4, [1.0] * 4, noise_type)
    np.testing.assert_array_equal(raw, d * np.float32(0.125) if noise_type == 'normal' else d)
