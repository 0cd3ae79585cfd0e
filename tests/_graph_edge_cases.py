"""Neighbour-list inputs at the edges where a builder can go wrong (pure numpy, seeded, no GPU), and the host restatement
of the reversed lists.  tests/test_graph_edge_host.py holds the preconditions every case must meet;
tests/test_gpu_graph_edges.py runs the cases through every builder; tools/fuzz_graph.py takes its line piles from here.

Every case is a `Case`: s_cur, s_delta [B, N, 3] float32 (read-only), the radius as the Python float a config holds, and
`meta` (what the generator knows about the case).  cases() computes each one once.

  shell(radius)        isolated groups of one receiver and six or eight senders whose fp32 squared distance to it -- in the
                       oracle's operation order (dx*dx + dy*dy) + dz*dz -- is exactly T - 1 ulp, T or T + 1 ulp, T =
                       fp32(radius * radius): the radius test decided on the last bit.  Coordinates lie on a 2^-20 grid with
                       s_delta = 0, so every difference is exact in fp32.
  aligned_lattice      pitch 0.01 on x, y = fp32(-0.32 + k * 0.01) moved by -1 / 0 / +1 ulp: particles on and to either side
                       of the strip boundaries (graph_strip) and, with a 2-cm band height, the band boundaries (graph_band).
                       A tenth of the sites hold two particles at z = 0.75 +- 2^-9: equidistant from every third particle in the
                       plane, so exact ties at the top-10 cut exist.
  xline, yline         a line along x / y (every particle in a few strips / in one strip), a third of it beyond +-0.32
  one_strip            everything at x > 0.35: strip 63 holds the whole sample and nothing is pruned
  tiny_radius          a jittered pile at radius 1e-4 (self loops only) and at radius 0.0 (no edge at all: (0 - 0) < 0 is false)
"""
import numpy as np

K = 10
GRID = 2.0 ** -20
SHELL_RADII = (0.02, 0.05, 0.08, 0.0801, 0.1, 0.3, 0.7)
# The reference's threshold fp32(r * r), r * r in Python doubles (model/gnn_dyn.py:229, :236), as bit patterns
THRESHOLD_BITS = {0.02: 970045207, 0.05: 992204554, 0.08: 1003599639, 0.0801: 1003634021, 0.1: 1008981770, 0.3: 1035489772,
                  0.7: 1056629064}
CLASSES = (-1, 0, 1)           # a sender's squared distance in ulps from T


class Case(object):
    def __init__(self, name, s_cur, s_delta, radius, meta=None):
        self.name, self.radius, self.meta = name, float(radius), dict(meta or {})
        self.s_cur = np.ascontiguousarray(s_cur, dtype=np.float32)
        self.s_delta = np.ascontiguousarray(s_delta, dtype=np.float32)
        assert self.s_cur.ndim == 3 and self.s_cur.shape == self.s_delta.shape and self.s_cur.shape[2] == 3
        self.s_cur.setflags(write=False)
        self.s_delta.setflags(write=False)

    @property
    def B(self):
        return self.s_cur.shape[0]

    @property
    def N(self):
        return self.s_cur.shape[1]

    def __repr__(self):
        return 'Case(%s, B=%d, N=%d, radius=%r)' % (self.name, self.B, self.N, self.radius)


def dis32(d):
    """squared length of fp32 differences d [..., 3] as the oracle and torch evaluate it: ((dx*dx + dy*dy) + dz*dz) in fp32"""
    d = np.asarray(d, dtype=np.float32)
    sq = d * d
    return (sq[..., 0] + sq[..., 1]) + sq[..., 2]


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)


# ---- shell ---------------------------------------------------------------------------------------------------------------
def shell_offsets(radius, rng, per_class):
    """{-1, 0, +1: [per_class, 3] float64 offsets on the 2^-20 grid} whose dis32 is T - 1 ulp, T, T + 1 ulp.
    A direction in the x-y plane (a quarter of them along x, a quarter along y: the strips and the bands prune on one
    coordinate alone), its length such that a dz of a few times ulp(T) * 2^19 completes T; then dz walks in steps of 2^-20, each
    of which moves the distance by about an ulp of T, and every step that lands on one of the three patterns is a hit."""
    T = np.float32(radius * radius)
    tb = int(_bits(T))
    k0 = max(4, int(round(float(np.spacing(T)) * 2.0 ** 19 / GRID)))
    walk = 512
    rho = np.sqrt(float(T) - ((k0 + walk / 2) * GRID) ** 2)
    out = {c: [] for c in CLASSES}
    for _ in range(200):
        if min(len(v) for v in out.values()) >= per_class:
            break
        m = 512
        theta = rng.uniform(0.0, 2.0 * np.pi, m)
        kind = rng.integers(0, 4, m)
        half = rng.integers(0, 2, m) * np.pi
        theta = np.where(kind == 0, half, np.where(kind == 1, half + 0.5 * np.pi, theta))
        dx = np.round(rho * np.cos(theta) / GRID) * GRID
        dy = np.round(rho * np.sin(theta) / GRID) * GRID
        dz = (k0 + np.arange(walk))[None, :] * GRID * rng.choice([-1.0, 1.0], m)[:, None]
        d = np.stack([np.broadcast_to(dx[:, None], dz.shape), np.broadcast_to(dy[:, None], dz.shape), dz], -1)
        rel = _bits(dis32(d.astype(np.float32))) - tb
        for c in CLASSES:
            rows, cols = np.nonzero(rel == c)
            _, first = np.unique(rows, return_index=True)          # one hit per direction
            out[c].extend(d[rows[first], cols[first]])
    for c in CLASSES:
        if len(out[c]) < per_class:
            raise RuntimeError('shell(%r): %d offsets of class %+d found, %d wanted' % (radius, len(out[c]), c, per_class))
        pick = rng.permutation(len(out[c]))[:per_class]
        out[c] = np.asarray(out[c], np.float64)[pick]
    return out


def _shell_sample(radius, seed):
    """one sample: positions [N, 3] float32, receivers [G], senders [S], each sender's receiver [S] and class [S]"""
    rng = np.random.default_rng(seed)
    if radius <= 0.1:
        nx, ny, per_group = 7, 7, 6              # 49 groups of 1 + 6: N = 343, 98 senders of each class
    else:
        nx, ny, per_group = 5, 3, 8              # 15 groups of 1 + 8: N = 135, 40 senders of each class
    groups = nx * ny
    # group g's senders: classes in rotation, so that the three are equally many over the sample
    cls_of = np.array([[CLASSES[(g + t) % 3] for t in range(per_group)] for g in range(groups)])
    per_class = int((cls_of == 0).sum())
    offs = shell_offsets(radius, rng, per_class)
    used = {c: 0 for c in CLASSES}
    # centres 3.1 radii apart at the least (jitter included): more than twice the radius, and nobody of another group is
    # nearer than 1.1 radii to a sender either, so the cut binds for no pair at the radius, in either direction
    pitch = 3.3 * radius
    pos, recv, send, send_recv, send_cls = [], [], [], [], []
    for g in range(groups):
        ix, iy = g % nx, g // nx
        c = np.array([(ix - (nx - 1) / 2.0) * pitch, (iy - (ny - 1) / 2.0) * pitch, 0.75])
        c[:2] += rng.uniform(-0.1, 0.1, 2) * radius
        c[2] += rng.uniform(-0.002, 0.002)
        c = np.round(c / GRID) * GRID
        r = len(pos)
        pos.append(c)
        recv.append(r)
        for t in range(per_group):
            k = int(cls_of[g, t])
            send.append(len(pos))
            send_recv.append(r)
            send_cls.append(k)
            pos.append(c + offs[k][used[k]])
            used[k] += 1
    pos = np.asarray(pos, np.float64)
    p32 = pos.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), pos)                    # on the grid and inside fp32's 24 bits
    perm = rng.permutation(len(pos))                                      # receivers and senders interleaved
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    p32 = p32[perm]
    recv, send, send_recv = inv[np.asarray(recv)], inv[np.asarray(send)], inv[np.asarray(send_recv)]
    send_cls = np.asarray(send_cls)
    rel = _bits(dis32(p32[send] - p32[send_recv])) - int(_bits(np.float32(radius * radius)))
    assert np.array_equal(rel, send_cls)                                  # the placed pairs have the patterns asked for
    return p32, recv, send, send_recv, send_cls


def shell(radius, seeds=(11, 12)):
    samples = [_shell_sample(radius, s + int(round(radius * 1e4)) * 100) for s in seeds]
    s_cur = np.stack([s[0] for s in samples])
    meta = {'recv': [s[1] for s in samples], 'send': [s[2] for s in samples], 'send_recv': [s[3] for s in samples],
            'send_cls': [s[4] for s in samples]}
    return Case('shell_r%g' % radius, s_cur, np.zeros_like(s_cur), radius, meta)


# ---- lattice on the strip and band boundaries ------------------------------------------------------------------------------
def aligned_lattice(N, radius, seeds=(21, 22)):
    nx, ny = {300: (18, 15), 820: (41, 18)}[N]
    pairs = N - nx * ny                           # sites that hold two particles, at z = 0.75 +- 2^-9
    assert 0 < pairs < nx * ny
    out = []
    for seed in seeds:
        rng = np.random.default_rng(seed + N)
        kx = (64 - nx) // 2 + np.arange(nx)
        ky = (64 - ny) // 2 + np.arange(ny)
        gx, gy = np.meshgrid(kx, ky, indexing='ij')
        x = np.float32(-0.32 + gx.ravel() * 0.01)
        y = np.float32(-0.32 + gy.ravel() * 0.01)

        def nudge(v):
            step = rng.integers(-1, 2, v.shape)
            up, dn = np.nextafter(v, np.float32(1)), np.nextafter(v, np.float32(-1))
            return np.where(step > 0, up, np.where(step < 0, dn, v)).astype(np.float32)
        x, y = nudge(x), nudge(y)
        double = np.zeros(nx * ny, bool)
        double[rng.permutation(nx * ny)[:pairs]] = True
        h = np.float32(2.0 ** -9)
        p = np.concatenate([np.stack([x[~double], y[~double], np.full((~double).sum(), 0.75, np.float32)], 1),
                            np.stack([x[double], y[double], np.full(pairs, np.float32(0.75) + h, np.float32)], 1),
                            np.stack([x[double], y[double], np.full(pairs, np.float32(0.75) - h, np.float32)], 1)]).astype(np.float32)
        assert p.shape == (N, 3)
        out.append(p[rng.permutation(N)])
    s_cur = np.stack(out)
    return Case('lattice_n%d_r%g' % (N, radius), s_cur, np.zeros_like(s_cur), radius)


# ---- piles (the line piles are tools/fuzz_graph.py's too) ---------------------------------------------------------------------
def line_pile(rng, N, axis):
    """[N, 3] float64: a line along x (axis 0) or y (axis 1) over +-0.3, 3 mm wide, z within a centimetre under 0.75"""
    s = np.empty((N, 3), np.float64)
    s[:, axis] = rng.uniform(-0.3, 0.3, N)
    s[:, 1 - axis] = rng.normal(0, 0.003, N)
    s[:, 2] = 0.75 - rng.uniform(0, 0.01, N)
    return s


def _line(axis, radius, seed, B=2, N=300):
    rng = np.random.default_rng(seed)
    s = np.stack([line_pile(rng, N, axis) for _ in range(B)])
    s[..., :2] *= 1.6                             # the line reaches +-0.48: a third of it beyond the +-0.32 of the strips
    s = s.astype(np.float32)
    sd = (0.004 * rng.standard_normal(s.shape)).astype(np.float32)
    return Case('%sline_r%g' % ('xy'[axis], radius), s, sd, radius)


def xline(radius=0.08, seed=31):
    return _line(0, radius, seed)


def yline(radius=0.08, seed=32):
    return _line(1, radius, seed)


def one_strip(radius=0.08, seed=33, B=2, N=200):
    rng = np.random.default_rng(seed)
    s = np.empty((B, N, 3), np.float64)
    s[..., 0] = rng.uniform(0.36, 0.5, (B, N))
    s[..., 1] = rng.uniform(-0.15, 0.15, (B, N))
    s[..., 2] = 0.75 - rng.uniform(0, 0.01, (B, N))
    s = s.astype(np.float32)
    sd = (0.002 * rng.standard_normal(s.shape)).astype(np.float32)
    sd[..., 0] = np.abs(sd[..., 0])               # displaced positions stay beyond 0.35
    return Case('one_strip_r%g' % radius, s, sd, radius)


def tiny_radius(radius, seed=34, B=2, N=150):
    rng = np.random.default_rng(seed)
    s = np.empty((B, N, 3), np.float64)
    s[..., :2] = rng.uniform(-0.2, 0.2, (B, N, 2))
    s[..., 2] = 0.75 - rng.uniform(0, 0.01, (B, N))
    s = s.astype(np.float32)
    sd = (0.004 * rng.standard_normal(s.shape)).astype(np.float32)
    return Case('tiny_r%g' % radius, s, sd, radius)


CASE_NAMES = (['shell_r%g' % r for r in SHELL_RADII] +
              ['lattice_n300_r0.08', 'lattice_n300_r0.02', 'lattice_n820_r0.08', 'lattice_n820_r0.02',
               'xline_r0.08', 'xline_r0.02', 'yline_r0.08', 'yline_r0.02', 'one_strip_r0.08', 'tiny_r0.0001', 'tiny_r0'])
_cases = {}


def case(name):
    """the named case, computed once and read-only"""
    if name not in _cases:
        kind, _, r = name.rpartition('_r')
        radius = float(r)
        if kind == 'shell':
            c = shell(radius)
        elif kind.startswith('lattice_n'):
            c = aligned_lattice(int(kind[len('lattice_n'):]), radius)
        elif kind == 'xline':
            c = xline(radius)
        elif kind == 'yline':
            c = yline(radius)
        elif kind == 'one_strip':
            c = one_strip(radius)
        elif kind == 'tiny':
            c = tiny_radius(radius)
        else:
            raise KeyError(name)
        assert c.name == name, (c.name, name)
        _cases[name] = c
    return _cases[name]


def cases():
    return [case(n) for n in CASE_NAMES]


# ---- the reversed lists, restated ------------------------------------------------------------------------------------------
def reverse_lists_np(nbr_idx, nbr_cnt, n_recv=None):
    """nbr_idx [B, N, 10], nbr_cnt [B, N] -> (rev_off [B, N + 1] int32, rev: B int32 arrays of rev_off[b, N] entries).
    Sender j's list rev[b][rev_off[b, j]:rev_off[b, j + 1]] holds, ascending, the edge slots i * 10 + k it feeds: k < cnt[i],
    idx[i, k] == j and receiver i < n_recv[b] (None: every receiver)."""
    nbr_idx, nbr_cnt = np.asarray(nbr_idx).astype(np.int64), np.asarray(nbr_cnt).astype(np.int64)
    B, N, k = nbr_idx.shape
    assert k == K and nbr_cnt.shape == (B, N)
    n_recv = np.full(B, N) if n_recv is None else np.asarray(n_recv).astype(np.int64)
    rev_off = np.zeros((B, N + 1), np.int32)
    rev = []
    slot = np.arange(N * K).reshape(N, K)
    for b in range(B):
        live = (np.arange(K)[None, :] < nbr_cnt[b][:, None]) & (np.arange(N)[:, None] < n_recv[b])
        senders, slots = nbr_idx[b][live], slot[live]
        order = np.lexsort((slots, senders))                             # by sender, then by slot
        rev_off[b, 1:] = np.cumsum(np.bincount(senders, minlength=N))
        rev.append(slots[order].astype(np.int32))
    return rev_off, rev
