"""The inputs of tests/test_reward_ref_host.py and tests/test_gpu_reward_edges.py: random cases on five image sizes with every
particle class at the image's edges, and exact-lattice cases where every intermediate is exact in fp32.

A random case is conditioned so that an fp32 evaluation takes the float64 decisions (_reward_ref.fp32_margins >= MARGIN): a
particle whose ix or iy comes too near an integer, or that left its class when x, y were rounded to fp32, is drawn again, and
so is a goal pixel whose two nearest particles are too nearly equidistant.  Nothing is left out: every case has its N particles
and M goal pixels, and `redrawn` only counts the draws."""
import numpy as np

import _reward_ref as R

MARGIN = 8.0
SIZES = [(48, 80), (80, 48), (1, 16), (16, 1), (720, 720)]                     # (H, W)
NM = [(1, 1), (3, 2), (4, 255), (5, 256), (63, 257), (64, 1), (65, 1000), (255, 2), (256, 256), (257, 257), (600, 1000)]
# twenty particles in turn: half interior, the last cell and the clamped half pixel of either axis, six outside
CLASSES = ['in'] * 10 + ['last_x', 'last_y', 'half_x', 'half_y'] + ['out'] * 6
SIDES = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)]   # four sides, four corners


def camera(Hh, Ww):
    """intrinsics that put the image's width on the pixel range [0, H) the reference's normalisation gives it; fx != fy"""
    s = float(max(Hh, Ww))
    return np.float32([1.1 * s, 0.9 * s, 0.5 * Hh - 0.3, 0.5 * Hh + 0.2])


def _axis(rng, kind, size):
    """a sample coordinate (ix or iy, before the clamp) of the class `kind` on an axis of `size` pixels"""
    if kind == 'in':
        return rng.uniform(0.0, size - 1.0) if size > 1 else rng.uniform(-0.5, 0.5)
    if kind == 'last':
        return rng.uniform(size - 2.0, size - 1.0) if size > 1 else rng.uniform(-0.5, 0.5)
    if kind == 'half':
        return rng.uniform(-0.5, 0.0)
    far = 1.0e4 * rng.uniform(0.5, 1.5) if kind.endswith('far') else rng.uniform(0.5, 40.0)
    return -far if kind.startswith('lo') else size - 1.0 + far


def _class_of(b, n):
    """(class on x, class on y) of particle n of row b"""
    c = CLASSES[(n + 7 * b) % 20]
    if c == 'out':
        sx, sy = SIDES[(n // 2 + 3 * b) % 8]
        far = 'far' if (n + b) % 3 == 0 else ''
        name = {-1: 'lo' + far, 1: 'hi' + far, 0: 'in'}
        return name[sx], name[sy]
    return {'in': ('in', 'in'), 'last_x': ('last', 'in'), 'last_y': ('in', 'last'), 'half_x': ('half', 'in'),
            'half_y': ('in', 'half')}[c]


def _in_class(i, kind, size):
    if kind == 'in' or kind == 'last':
        lo, hi = (0.0 if kind == 'in' else size - 2.0), size - 1.0
        return (lo < i < hi) if size > 1 else (-0.5 < i < 0.5)
    if kind == 'half':
        return -0.5 < i < 0.0
    return i < -0.5 if kind.startswith('lo') else i > size - 0.5


def _particle(rng, kx, ky, Hh, Ww, cam):
    fx, fy, cx, cy = [float(v) for v in cam]
    ix, iy = _axis(rng, kx, Ww), _axis(rng, ky, Hh)
    u, v = (ix + 0.5) * Hh / Ww, iy + 0.5                   # ix = u W / H - 1 / 2, iy = v - 1 / 2
    z = rng.uniform(0.6, 0.9)
    return np.float32([(u - cx) * z / fx, (v - cy) * z / fy, z])


def random_case(index, B=None):
    """case `index` of NM on SIZES[index % 5] -> dict(name, state [B,N,3], G [H,W], cam [4], goal [M,2], classes, redrawn)"""
    N, M = NM[index]
    Hh, Ww = SIZES[index % len(SIZES)]
    return make_random('%dx%d N=%d M=%d' % (Hh, Ww, N, M), Hh, Ww, N, M, B if B is not None else (3 if N * M > 100000 else 4),
                       seed=100 + index)


def make_random(name, Hh, Ww, N, M, B, seed):
    rng = np.random.default_rng(seed)
    cam = camera(Hh, Ww)
    G = (rng.uniform(0.0, 1.0, (Hh, Ww)) + rng.integers(0, 6, (Hh, Ww))).astype(np.float32)     # integer jumps between pixels
    classes = [[_class_of(b, n) for n in range(N)] for b in range(B)]
    state = np.empty((B, N, 3), np.float32)
    for b in range(B):
        for n in range(N):
            state[b, n] = _particle(rng, classes[b][n][0], classes[b][n][1], Hh, Ww, cam)

    def goal_pixel():
        return np.float32([rng.integers(0, Ww), rng.integers(0, Hh)])          # (col, row), an image pixel
    goal = np.stack([goal_pixel() for _ in range(M)])
    redrawn = 0
    for _ in range(200):
        t = R.evaluate(state, G, cam, goal)
        mi, mg = R.fp32_margins(t)
        bad_p = [(b, n) for b in range(B) for n in range(N)
                 if mi[b, n].min() < MARGIN or not _in_class(t['ix_raw'][b, n], classes[b][n][0], Ww)
                 or not _in_class(t['iy_raw'][b, n], classes[b][n][1], Hh)]
        for b, n in bad_p:
            state[b, n] = _particle(rng, classes[b][n][0], classes[b][n][1], Hh, Ww, cam)
        bad_g = [] if bad_p else [m for m in range(M) if mg[:, m].min() < MARGIN]
        for m in bad_g:
            goal[m] = goal_pixel()
        redrawn += len(bad_p) + len(bad_g)
        if not bad_p and not bad_g:
            break
    else:
        raise AssertionError('%s: no conditioned draw in 200 rounds' % name)
    return dict(name=name, kind='random', state=state, G=G, cam=cam, goal=goal, classes=classes, redrawn=redrawn)


# ---- exact lattices ----------------------------------------------------------------------------------------------------------
# fx = fy = 64, cx = cy = 16, z a power of two, x and y dyadic, G integer-valued, goal pixels integer, distances 0, 5, 10
# (3-4-5 offsets): every intermediate of every kernel is exact in fp32, so the value must be the reference's to the bit.
# A particle is given by its sample coordinates ('i', ix, iy) or by its pixel ('p', u, v).
POISON = (8, 0)          # G[8, 0] is NaN: the pixel BEHIND the last pixel of row 7 in memory; no tap of a correct kernel reads it


def _lattice_particles(Hh, Ww):
    return [('i', 0.0, 5.5),                 # 0  exactly on ix = 0
            ('i', Ww - 1.0, 7.0),            # 1  exactly on ix = W - 1, in row 7: an unclamped upper tap is POISON
            ('i', 5.0, 0.0),                 # 2  exactly on iy = 0
            ('i', 6.5, Hh - 1.0),            # 3  exactly on iy = H - 1
            ('i', 10.0, Hh - 10.0),          # 4  an interior integer on both axes
            ('i', 10.5, Hh - 11.5),          # 5  half integers
            ('i', Ww - 1.0, Hh - 1.0),       # 6  the last pixel
            ('i', 0.0, 0.0),                 # 7  the first pixel
            ('i', -3.0, 9.5),                # 8  outside, left
            ('i', Ww + 4.0, Hh + 3.5),       # 9  outside, the far corner
            ('p', 9.0, 17.0),                # 10 \ equidistant (5) from the goal pixel (12, 21)
            ('p', 15.0, 25.0),               # 11 /
            ('p', 21.0, 9.0),                # 12 \ a duplicated particle, 5 from the goal pixel (24, 13)
            ('p', 21.0, 9.0),                # 13 /
            ('p', 5.0, 27.0),                # 14 its pixel IS the goal pixel (5, 27)
            ('p', 27.0, 29.0)]               # 15 10 from the goal pixel (27, 19)


LATTICE_GOAL = np.float32([[12, 21], [24, 13], [5, 27], [27, 19], [12, 13], [15, 30]])
LATTICE_TIE, LATTICE_DUP, LATTICE_ZERO = 0, 1, 2           # goal points: the tie of 10 / 11, of the duplicates 12 / 13, dist == 0


def lattice_case(Hh, Ww, B=3):
    rng = np.random.default_rng(Hh)
    cam = np.float32([64.0, 64.0, 16.0, 16.0])
    G = rng.integers(0, 8, (Hh, Ww)).astype(np.float32)
    G[POISON] = np.nan
    spec = _lattice_particles(Hh, Ww)
    N = len(spec)
    state = np.empty((B, N, 3), np.float32)
    order = np.empty((B, N), np.int64)
    for b in range(B):
        order[b] = np.roll(np.arange(N), 5 * b)[::(-1 if b == 2 else 1)]         # row 2 reversed: the other particle of a tie is first
        for n in range(N):
            kind, a, c = spec[order[b, n]]
            u, v = ((a + 0.5) * Hh / Ww, c + 0.5) if kind == 'i' else (a, c)
            k = 12 if order[b, n] == 13 else int(order[b, n])                     # the duplicate has its twin's depth too
            z = [0.5, 1.0, 2.0][(k + b) % 3]
            state[b, n] = [(u - 16.0) * z / 64.0, (v - 16.0) * z / 64.0, z]
    return dict(name='lattice %dx%d' % (Hh, Ww), kind='lattice', state=state, G=G, cam=cam, goal=LATTICE_GOAL.copy(),
                order=order, redrawn=0)


_cache = {}


def cases():
    """every case of the GPU test, built once and left read-only"""
    if not _cache:
        out = [random_case(i) for i in range(len(NM))] + [lattice_case(64, 32), lattice_case(32, 64)]
        for c in out:
            for v in c.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _cache['cases'] = out
        _cache['ref'] = [R.evaluate(c['state'], c['G'], c['cam'], c['goal']) for c in out]
    return _cache['cases'], _cache['ref']


def scenes_case():
    """three goals of one image size [3,48,80] with m = (1, 255, 257) goal pixels, two rows of 65 particles each"""
    key = 'scenes'
    if key not in _cache:
        _cache[key] = [make_random('scene %d' % k, 48, 80, 65, m, 2, seed=300 + k) for k, m in enumerate((1, 255, 257))]
    return _cache[key]
