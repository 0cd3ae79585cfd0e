"""Test-side restatement of the resolution regressor (model/res_regressor.py) -- not the library's code:

  area_tabs / resize_area   INTER_AREA downscaling as its published definition states it, in numpy float32 and in the order
                            the device follows (horizontal weighted sums per source row, then the vertical accumulation);
                            integer scale on both axes: the block mean.  Signature of cv2.resize, so the golden generator
                            can install it in place of cv2's.
  resize_exact              a different algorithm: the piecewise-constant source integrated over each cell in float64.
  stack                     infer_param's input (:146-175) from two masks and a distance transform.
  forward64                 the network in float64 through torch.nn.functional on the CPU, with every tap.
  rand_input, stack_summary how tests/golden/rgr.npz names its random inputs (a seed) and keeps its stacks (a grid + moments).
"""
import numpy as np


def area_tab(ssize, dsize):
    """[(source index, weight)] per destination index: destination d covers [d s, (d+1) s), s = ssize / dsize; a source
    pixel weighs the part of it the cell covers over the cell width min(s, ssize - d s) (double, stored as float32);
    covers <= 1e-3 are dropped."""
    scale = ssize / dsize
    tab = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s2 = min(int(np.floor(f2)), ssize - 1)
        s1 = min(int(np.ceil(f1)), s2)
        t = []
        if s1 - f1 > 1e-3:
            t.append((s1 - 1, np.float32((s1 - f1) / cell)))
        for sx in range(s1, s2):
            t.append((sx, np.float32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            t.append((s2, np.float32(min(min(f2 - s2, 1.0), cell) / cell)))
        tab.append(t)
    return tab


def _padded(tab):
    T = max(len(t) for t in tab)
    idx = np.zeros((len(tab), T), np.int64)
    wgt = np.zeros((len(tab), T), np.float32)
    for d, t in enumerate(tab):
        for j, (i, a) in enumerate(t):
            idx[d, j], wgt[d, j] = i, a
    return idx, wgt


def resize_area(img, dsize, interpolation=None):
    """cv2.resize(img, dsize=(W, H), interpolation=INTER_AREA) for a downscale, float32 out."""
    W, H = dsize
    src = np.asarray(img).astype(np.float32)
    h, w = src.shape
    assert h >= H and w >= W, 'downscaling only'
    if h % H == 0 and w % W == 0:
        fy, fx = h // H, w // W
        acc = np.zeros((H, W), np.float32)
        for r in range(fy):                      # the block in row-major order
            for q in range(fx):
                acc = acc + src[r::fy, q::fx]
        return acc * np.float32(1.0 / (fx * fy))
    xi, xa = _padded(area_tab(w, W))
    yi, ya = _padded(area_tab(h, H))
    hs = np.zeros((h, W), np.float32)
    for j in range(xi.shape[1]):                 # horizontal: per source row, taps in table order (padding adds +0)
        hs = hs + src[:, xi[:, j]] * xa[:, j][None, :]
    out = np.zeros((H, W), np.float32)
    for j in range(yi.shape[1]):                 # vertical
        out = out + ya[:, j][:, None] * hs[yi[:, j], :]
    return out


def _cover(ssize, dsize):
    """[dsize, ssize] float64: the length of [s, s+1) inside destination cell d, over the cell's width"""
    scale = ssize / dsize
    R = np.zeros((dsize, ssize))
    for d in range(dsize):
        a, b = d * scale, min((d + 1) * scale, ssize)
        for s in range(int(np.floor(a)), min(int(np.ceil(b)), ssize)):
            R[d, s] = max(0.0, min(b, s + 1) - max(a, s))
        R[d] /= (b - a)
    return R


def resize_exact(img, dsize):
    W, H = dsize
    src = np.asarray(img, np.float64)
    return _cover(src.shape[0], H) @ src @ _cover(src.shape[1], W).T


def stack(init, goal, dist_transform):
    """infer_param's [6,224,224] float32 input; dist_transform(src) = cv2.distanceTransform(src, DIST_L2, 5) (float32)"""
    init = np.asarray(init).astype(np.float32)
    goal = np.asarray(goal).astype(np.float32)
    h = init.shape[0]
    d_i = dist_transform((1 - init).astype(np.uint8)).astype(np.float32) / h
    d_g = dist_transform((1 - goal).astype(np.uint8)).astype(np.float32) / h
    ex_i = np.logical_and(init, 1 - goal).astype(np.float32)
    ex_g = np.logical_and(goal, 1 - init).astype(np.float32)
    return np.stack([resize_area(c, (224, 224)) for c in (init, goal, d_i, d_g, ex_i, ex_g)])


def rand_input(seed, B=2):
    """[B,6,224,224] float32 in [0, 1) from an integer hash of (seed, index): the same values under any numpy version, so a
    fixture can name the seed instead of storing the array"""
    i = np.arange(B * 6 * 224 * 224, dtype=np.uint64) + np.uint64((seed * 0x9E3779B97F4A7C15) % 2 ** 64)
    with np.errstate(over='ignore'):
        i ^= i >> np.uint64(33)
        i *= np.uint64(0xFF51AFD7ED558CCD)
        i ^= i >> np.uint64(33)
        i *= np.uint64(0xC4CEB9FE1A85EC53)
        i ^= i >> np.uint64(33)
    return ((i >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(B, 6, 224, 224)


STACK_STRIDE = 7        # the fixture keeps a stack on this pixel grid, plus per-channel float64 sums and sums of squares
TAP_STRIDE = 7          # and the conv5 taps (flattened per sample) at this stride


def stack_summary(st):
    """(grid [6,32,32], sum [6], sum of squares [6]) of a [6,224,224] stack"""
    s64 = np.asarray(st, np.float64).reshape(6, -1)
    return (np.ascontiguousarray(st[:, ::STACK_STRIDE, ::STACK_STRIDE]), s64.sum(axis=1), (s64 * s64).sum(axis=1))


def fixture_masks(z, p):
    """mask pair p of tests/golden/rgr.npz: (init, goal) uint8 0/1"""
    shape = tuple(int(v) for v in z['mask%d_shape' % p])
    n = shape[0] * shape[1]
    return (np.unpackbits(z['mask%d_init' % p])[:n].reshape(shape),
            np.unpackbits(z['mask%d_goal' % p])[:n].reshape(shape))


def fixture_inputs(z):
    """the fixture's 5 network inputs [5,6,224,224]: the 3 stacks (restated, with the exact transform the fixture was
    captured with) and the 2 random inputs"""
    from oracle import goal as og
    st = [stack(*fixture_masks(z, p), lambda s: np.asarray(og.distance_transform_edt(s), np.float32)) for p in range(3)]
    return np.concatenate([np.stack(st), rand_input(int(z['rand_seed']))]).astype(np.float32)


def check_stack(st, z, p, tol=1e-6):
    """a [6,224,224] stack against the fixture's record of the reference's stack p (grid values, channel moments)"""
    grid, s1, s2 = stack_summary(st)
    assert float(np.abs(grid - z['stack%d_grid' % p]).max()) <= tol, p
    np.testing.assert_allclose(s1, z['stack%d_sum' % p], rtol=tol, atol=tol)
    np.testing.assert_allclose(s2, z['stack%d_sumsq' % p], rtol=tol, atol=tol)


def forward64(sd, x):
    """float64 forward of the state_dict sd on x [B,6,224,224]: (out [B,n_out], taps {'c1'..'c5','f1'..'f4'})"""
    import torch
    import torch.nn.functional as F

    def p(k):
        v = sd[k]
        return (v.detach() if hasattr(v, 'detach') else torch.from_numpy(np.asarray(v))).to(torch.float64)

    h = torch.from_numpy(np.asarray(x, np.float64))
    taps = {}
    with torch.no_grad():
        for n, i in enumerate((0, 2, 4, 6, 8)):
            h = F.leaky_relu(F.conv2d(h, p('model.%d.weight' % i), p('model.%d.bias' % i), stride=2, padding=1), 0.2)
            taps['c%d' % (n + 1)] = h.numpy()
        h = h.flatten(1)
        for n, i in enumerate((11, 13, 15, 17)):
            h = F.leaky_relu(F.linear(h, p('model.%d.weight' % i), p('model.%d.bias' % i)), 0.2)
            taps['f%d' % (n + 1)] = h.numpy()
        out = F.linear(h, p('model.19.weight'), p('model.19.bias'))
    return out.numpy(), taps
