"""Host restatement of the device sampler k_mppi_sample (csrc/k_mppi.h; the stream's contract is in include/drp.h at
drp_mpc_params.seed).  Pure numpy: it imports neither the library nor the device.

  philox4x32_10   the Random123 block function, in uint64 arithmetic
  raw_words       the four words of every (sample, t): counter (gs lo, gs hi, t, iteration mod 2^32), key = seed
  uniform24       a word's top 24 bits as a float32 in [0, 1): exact
  normal_inputs   Box-Muller: its float32 inputs reproduced exactly, the transcendental functions in float64
  actions         the temporal filter, the clip and the rounding to float32, in float64 in the kernel's order
"""
import collections

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
TWO_PI_F32 = np.float32(6.283185307179586)
NOISE_TYPES = ('normal', 'uniform', 'total_rand')

# Corner inputs of Box-Muller in the stream of seed 42, t = 0, iteration 0 (a search over the first 2^26 global samples):
# name -> (global sample, first component of the pair).  'u1_one': word 2 = 0xffffffbe >= 2^32 - 128, u1 = 1, radius 0;
# 'u1_small': word 0 = 12, u1 = 13 * 2^-32, radius 6.27.
CORNER_SAMPLES = {'u1_one': (52825872, 2), 'u1_small': (26967075, 0)}


def philox4x32_10(counter, key):
    """counter u32 [..., 4], key u64 (a scalar) -> u32 [..., 4]: ten rounds, the key bumped between them"""
    c = np.asarray(counter, dtype=np.uint32).astype(np.uint64)
    assert c.shape[-1] == 4
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = key & 0xFFFFFFFF, key >> 32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    for _ in range(10):
        p0 = np.uint64(M0) * c0                 # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK32,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK32)
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def raw_words(seed, sample_offset, n_sample, H, iteration):
    """u32 [n_sample, H, 4]: the Philox block of global sample gs = sample_offset + s at step t"""
    gs = (np.arange(n_sample, dtype=np.uint64) + np.uint64(int(sample_offset) & 0xFFFFFFFFFFFFFFFF))    # wraps modulo 2^64
    ctr = np.empty((n_sample, H, 4), dtype=np.uint32)
    ctr[..., 0] = (gs & MASK32).astype(np.uint32)[:, None]
    ctr[..., 1] = (gs >> np.uint64(32)).astype(np.uint32)[:, None]
    ctr[..., 2] = np.arange(H, dtype=np.uint32)[None, :]
    ctr[..., 3] = np.uint32(int(iteration) & 0xFFFFFFFF)
    return philox4x32_10(ctr, seed)


def uniform24(words):
    """(w >> 8) * 2^-24 as float32: a 24-bit integer times a power of two, exact"""
    w = np.asarray(words, dtype=np.uint32)
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


NormalInputs = collections.namedtuple('NormalInputs', 'u1 angle r n')


def normal_inputs(words):
    """words u32 [..., 4] -> (u1 f32, angle f32, r f64, n f64), each [..., 4], one entry per component c.
    Component c uses the pair (a, b) = (w[c & 2], w[(c & 2) + 1]):
        u1 = float32(float32(a) + 1) * 2^-32  in (0, 1],   u2 = float32(b) * 2^-32,   angle = float32(float32(2 pi) * u2)
    -- the float32 roundings the kernel makes, to nearest even -- and r = sqrt(-2 ln u1), n = r cos(angle) for c even,
    r sin(angle) for c odd, evaluated in float64 on those float32 values."""
    w = np.asarray(words, dtype=np.uint32)
    assert w.shape[-1] == 4
    a = w[..., [0, 0, 2, 2]]
    b = w[..., [1, 1, 3, 3]]
    scale = np.float32(2.0 ** -32)
    u1 = (a.astype(np.float32) + np.float32(1.0)) * scale
    u2 = b.astype(np.float32) * scale
    angle = TWO_PI_F32 * u2
    assert u1.dtype == np.float32 and angle.dtype == np.float32
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64))) + 0.0            # (+ 0.0: u1 = 1 gives +0, not -0)
    ang = angle.astype(np.float64)
    trig = np.where(np.arange(4) % 2 == 0, np.cos(ang), np.sin(ang))
    return NormalInputs(u1, angle, r, r * trig)


def draws(words, noise_type):
    """what the kernel calls n, the form host-fed noise has too: standard normal (float64 here) / 2u - 1 / u (float32, exact)"""
    if noise_type == 'normal':
        return normal_inputs(words).n
    u = uniform24(words)
    return np.float32(2.0) * u - np.float32(1.0) if noise_type == 'uniform' else u


def actions(nominal, draws, sigma, beta, lo, hi, noise_type):
    """nominal [H,4] f64, draws [n_sample,H,4] (the values the kernel holds in a float: float32-valued) -> f32 [n_sample,H,4].
    float64 throughout, in the kernel's order:
        resid = beta * (sigma * n) + resid * (1 - beta);   a = clip(nominal + resid, lo, hi)
        total_rand: no residual, a = lo + n * (hi - lo)
    lo / hi rounded to float32 first, as the ABI carries them; the result rounded to float32."""
    assert noise_type in NOISE_TYPES
    nominal = np.asarray(nominal, dtype=np.float64)
    n = np.asarray(draws).astype(np.float64)
    ns, H, _ = n.shape
    lo = np.asarray(lo, dtype=np.float32).astype(np.float64)
    hi = np.asarray(hi, dtype=np.float32).astype(np.float64)
    sigma, beta = float(sigma), float(beta)
    out = np.empty((ns, H, 4), dtype=np.float64)
    resid = np.zeros((ns, 4), dtype=np.float64)
    for t in range(H):
        z = np.zeros((ns, 4)) if noise_type == 'total_rand' else sigma * n[:, t]
        resid = beta * z + resid * (1.0 - beta)
        a = np.minimum(np.maximum(nominal[t] + resid, lo), hi)
        if noise_type == 'total_rand':
            a = lo + n[:, t] * (hi - lo)
        out[:, t] = a
    return out.astype(np.float32)
