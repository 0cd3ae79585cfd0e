"""A plain float64 reference of config_reward_ptcl downstream of the distance transform (env/flex_rewards.py:189-214), its
gradient with the rules of the reference's own operations written out, the discrete decisions it takes, a componentwise
first-order error bound for an evaluation at unit roundoff u, and the mutants that show the bound is tight enough.

    pix_n  = (x fx / z + cx, y fy / z + cy)
    r1     = sum_n bilinear(G, pix_n / H * 2 - 1)     grid_sample(padding_mode='border', align_corners=False); BOTH axes are
                                                      normalised with H (:197), so ix = u W / H - 1/2 and d ix / d u = W / H
    r2     = sum_m min_n |q_m - pix_n|
    reward = -(r1 + r2) / N,    loss = -sum_b reward_b

The gradient's rules (what torch does, checked by tests/test_reward_ref_host.py against F.grid_sample + torch.norm(...).min
under float64 autograd):
    * grid_sample's border clamp passes no gradient where ix <= 0 or ix >= W - 1 (clip_coordinates_set_grad), the border
      itself included -- torch.clamp would pass it there;
    * min takes the FIRST index on an exact tie, and only that index receives gradient;
    * a goal point at distance exactly 0 contributes nothing (torch.norm's backward at 0 is 0, not 0 / 0).

Inputs are the fp32 arrays the kernels read, widened to double; nothing here rounds to fp32."""
import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
KERNELS = ('k_reward', 'kb_reward', 'kg_reward')
MUTANTS = ('x_by_w',            # x normalised by W
           'dix_du_one',        # d ix / d u = 1 in place of W / H
           'align_corners',     # align_corners=True mapping
           'tap_unclamped',     # upper tap not clamped in the value (reads the next row's first pixel: row-major memory)
           'border_grad',       # border gradient passed at ix == 0 and ix == W - 1
           'last_min',          # last minimum in place of the first on ties
           'chamfer_sign',      # chamfer term's sign flipped
           'z_without_y',       # z component without its y term
           'drop_last_goal',    # the last goal point dropped
           'goal_mult_256',     # goal points beyond a multiple of 256 dropped
           'particles_and_3',   # particles beyond N & ~3 dropped from the chamfer sweep
           'div_by_m')          # division by M in place of N


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def evaluate(state, G, cam, goal, mutant=None):
    """state [B,N,3], G [H,W], cam [fx,fy,cx,cy], goal [M,2] (col,row) -> dict:
    value [B] (normalised), value_raw [B], grad [B,N,3] = d(-sum_b value_b) / d state, the decisions x0, y0 [B,N] (cell of the
    clamped coordinate), clamp_x, clamp_y [B,N] (-1: ix <= 0, +1: ix >= W - 1, 0: inside), arg [B,M], dist [B,M], runner_up
    [B,M] (the smallest distance of a particle other than arg; inf for N = 1), and the intermediates bound() reads."""
    assert mutant is None or mutant in MUTANTS, mutant
    s, G, goal = _d(state), _d(G), _d(goal)
    fx, fy, cx, cy = [float(np.float32(v)) for v in cam]
    B, N, _ = s.shape
    Hh, Ww = G.shape
    M = goal.shape[0]
    x, y, z = s[..., 0], s[..., 1], s[..., 2]
    u = x * fx / z + cx
    v = y * fy / z + cy
    nx = u / (Ww if mutant == 'x_by_w' else Hh) * 2.0 - 1.0
    ny = v / Hh * 2.0 - 1.0
    if mutant == 'align_corners':
        ix_raw, iy_raw = (nx + 1.0) / 2.0 * (Ww - 1), (ny + 1.0) / 2.0 * (Hh - 1)
        mx0, my0 = (Ww - 1) / float(Hh), (Hh - 1) / float(Hh)
    else:
        ix_raw, iy_raw = ((nx + 1.0) * Ww - 1.0) / 2.0, ((ny + 1.0) * Hh - 1.0) / 2.0
        mx0, my0 = Ww / float(Hh), 1.0
    if mutant == 'dix_du_one':
        mx0 = 1.0

    def clamp(i, size):
        if mutant == 'border_grad':
            flag = np.where(i < 0.0, -1, np.where(i > size - 1.0, 1, 0))
        else:
            flag = np.where(i <= 0.0, -1, np.where(i >= size - 1.0, 1, 0))       # clip_coordinates_set_grad
        return np.clip(i, 0.0, size - 1.0), flag

    ix, clamp_x = clamp(ix_raw, Ww)
    iy, clamp_y = clamp(iy_raw, Hh)
    mx = np.where(clamp_x == 0, mx0, 0.0)
    my = np.where(clamp_y == 0, my0, 0.0)
    x0f, y0f = np.floor(ix), np.floor(iy)
    tx, ty = ix - x0f, iy - y0f
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, Ww - 1), np.minimum(y0 + 1, Hh - 1)
    g00, g01, g10, g11 = G[y0, x0], G[y0, x1], G[y1, x0], G[y1, x1]
    if mutant == 'tap_unclamped':
        flat = np.concatenate([G.ravel(), np.zeros(Ww + 2)])      # what lies behind the image is not the test's to say
        v00, v01 = flat[y0 * Ww + x0], flat[y0 * Ww + x0 + 1]
        v10, v11 = flat[(y0 + 1) * Ww + x0], flat[(y0 + 1) * Ww + x0 + 1]
    else:
        v00, v01, v10, v11 = g00, g01, g10, g11
    A, Bw = 1.0 - tx, 1.0 - ty
    terms = np.stack([v00 * (A * Bw), v01 * (tx * Bw), v10 * (A * ty), v11 * (tx * ty)])
    bil = terms.sum(0)                                               # [B,N]
    r1 = bil.sum(1)
    ex0, ex1, ey0, ey1 = g01 - g00, g11 - g10, g10 - g00, g11 - g01
    dgx = ex0 * Bw + ex1 * ty
    dgy = ey0 * A + ey1 * tx
    scale = 1.0 / (M if mutant == 'div_by_m' else N)
    a0x, a0y = scale * dgx * mx, scale * dgy * my                    # the bilinear term's addends of d loss / d pix

    Mu = M
    if mutant == 'drop_last_goal':
        Mu = M - 1
    elif mutant == 'goal_mult_256':
        Mu = M & ~255
    Nu = (N & ~3) if mutant == 'particles_and_3' else N
    arg = np.zeros((B, M), np.int64)
    dist = np.zeros((B, M))
    runner = np.full((B, M), np.inf)
    d2_all = np.empty((B, M, N))
    cx_add, cy_add = np.zeros((B, M)), np.zeros((B, M))              # each goal point's addend to its arg-min particle
    used = np.zeros((B, M), bool)
    for b in range(B):
        dx = goal[:, None, 0] - u[b][None, :]                        # [M,N]
        dy = goal[:, None, 1] - v[b][None, :]
        d2 = dx * dx + dy * dy
        d2_all[b] = d2
        for m in range(Mu):
            row = d2[m, :Nu]
            if Nu == 0:
                dist[b, m] = np.inf
                used[b, m] = True
                continue
            best = row.min()
            ties = np.flatnonzero(row == best)
            a = int(ties[-1] if mutant == 'last_min' else ties[0])   # torch.min: the first index
            arg[b, m] = a
            dist[b, m] = np.sqrt(best)
            used[b, m] = True
            if Nu > 1:
                runner[b, m] = np.sqrt(np.delete(row, a).min())
            if dist[b, m] > 0.0 and np.isfinite(dist[b, m]):         # torch.norm's backward: 0 at 0
                sign = 1.0 if mutant == 'chamfer_sign' else -1.0
                cx_add[b, m] = sign * scale * dx[m, a] / dist[b, m]
                cy_add[b, m] = sign * scale * dy[m, a] / dist[b, m]
    r2 = np.where(used, dist, 0.0).sum(1)
    gu, gv = a0x.copy(), a0y.copy()
    for b in range(B):
        np.add.at(gu[b], arg[b][used[b]], cx_add[b][used[b]])
        np.add.at(gv[b], arg[b][used[b]], cy_add[b][used[b]])
    grad = np.empty((B, N, 3))
    grad[..., 0] = gu * fx / z
    grad[..., 1] = gv * fy / z
    grad[..., 2] = -(gu * x * fx + (0.0 if mutant == 'z_without_y' else 1.0) * gv * y * fy) / (z * z)
    raw = -(r1 + r2)
    return dict(value=raw * scale, value_raw=raw, grad=grad, x0=x0, y0=y0, clamp_x=clamp_x, clamp_y=clamp_y, arg=arg, dist=dist,
                runner_up=runner, used=used,
                # intermediates
                B=B, N=N, M=M, Hh=Hh, Ww=Ww, cam=(fx, fy, cx, cy), x=x, y=y, z=z, u=u, v=v, nx=nx, ny=ny, ix_raw=ix_raw,
                iy_raw=iy_raw, tx=tx, ty=ty, taps=(g00, g01, g10, g11), terms=terms, bil=bil, r1=r1, r2=r2, a0x=a0x, a0y=a0y,
                mx=mx, my=my, goal=goal, cx_add=cx_add, cy_add=cy_add, gu=gu, gv=gv, d2=d2_all, scale=scale)


# ---- the error bound ---------------------------------------------------------------------------------------------------------
def _pixel_bounds(t, u):
    """|error| of pix = (x fx / z + cx, ...) [B,N] and of the un-normalised sample coordinates ix, iy [B,N] (before the clamp)"""
    fx, fy, cx, cy = t['cam']
    du = u * (2.0 * np.abs(t['x'] * fx / t['z']) + np.abs(t['u']))          # 1 mul + 1 div on x fx / z, 1 add of cx
    dv = u * (2.0 * np.abs(t['y'] * fy / t['z']) + np.abs(t['v']))

    def coord(p, dp, nrm, size):
        q = p / t['Hh']
        d = dp / t['Hh'] + u * np.abs(q)                                     # 1 div
        d = 2.0 * d + u * np.abs(nrm)                                        # * 2 exact, 1 sub: nrm = 2 q - 1
        d = d + u * np.abs(nrm + 1.0)                                        # 1 add
        d = size * d + u * np.abs((nrm + 1.0) * size)                        # 1 mul
        d = d + u * np.abs((nrm + 1.0) * size - 1.0)                         # 1 sub
        return d / 2.0                                                       # / 2 exact
    return du, dv, coord(t['u'], du, t['nx'], t['Ww']), coord(t['v'], dv, t['ny'], t['Hh'])


def fp32_margins(t):
    """What the decisions of an fp32 evaluation need to be the float64 ones: (margin of every ix, iy [B,N,2]: the distance to
    the nearest integer over its own fp32 error bound; margin of every goal point [B,M]: the smallest gap d2_n - d2_best over
    the sum of the two fp32 error bounds, n != arg).  The host test asks for >= 8 of both."""
    du, dv, dix, diy = _pixel_bounds(t, U32)
    mi = np.stack([np.abs(t['ix_raw'] - np.round(t['ix_raw'])) / dix, np.abs(t['iy_raw'] - np.round(t['iy_raw'])) / diy], -1)
    B, N, M = t['B'], t['N'], t['M']
    mg = np.full((B, M), np.inf)
    for b in range(B):
        dx = t['goal'][:, None, 0] - t['u'][b][None, :]
        dy = t['goal'][:, None, 1] - t['v'][b][None, :]
        ddx, ddy = du[b][None, :] + U32 * np.abs(dx), dv[b][None, :] + U32 * np.abs(dy)        # 1 sub
        dd2 = 2.0 * np.abs(dx) * ddx + 2.0 * np.abs(dy) * ddy + 2.0 * U32 * t['d2'][b]         # 2 mul, 1 add
        rows = np.arange(M)
        best, dbest = t['d2'][b][rows, t['arg'][b]], dd2[rows, t['arg'][b]]
        ratio = (t['d2'][b] - best[:, None]) / (dd2 + dbest[:, None])
        ratio[rows, t['arg'][b]] = np.inf
        mg[b] = ratio.min(1)
    return mi, mg


def _tree_depth(kernel, n):
    """roundings a term of a sum of n meets.  The fp32 kernels: a thread adds its ceil(n / 256) terms in turn (the first to 0.0,
    exact), six butterfly levels sum a wave, three adds the four waves.  kg_reward: thread 0 adds the n terms in turn."""
    if kernel == 'kg_reward':
        return max(n - 1, 0)
    return (n + 255) // 256 - 1 + 6 + 3


def bound(t, u, kernel):
    """Componentwise bound of |kernel - reference| for an evaluation of `kernel` at unit roundoff u with the reference's
    decisions: first-order propagation of one rounding per operation, counted from the kernel's own expressions, times 2 for the
    second-order terms.  -> dict(value [B], value_raw [B], grad [B,N,3])."""
    assert kernel in KERNELS
    fx, fy, cx, cy = t['cam']
    N, M = t['N'], t['M']
    x, y, z = t['x'], t['y'], t['z']
    du, dv, dix, diy = _pixel_bounds(t, u)
    # weights: tx = ix - floor(ix) is exact; a clamped coordinate is exact
    dtx = np.where(t['clamp_x'] == 0, dix, 0.0)
    dty = np.where(t['clamp_y'] == 0, diy, 0.0)
    tx, ty = t['tx'], t['ty']
    A, Bw = 1.0 - tx, 1.0 - ty
    dA, dB = dtx + u * A, dty + u * Bw                                         # 1 sub
    g00, g01, g10, g11 = [np.abs(g) for g in t['taps']]
    # value of a particle: four terms g * (w w'), 2 mul each, 3 adds
    dw = g00 * (dA * Bw + A * dB) + g01 * (dtx * Bw + tx * dB) + g10 * (dA * ty + A * dty) + g11 * (dtx * ty + tx * dty)
    dbil = dw + (2 + 3) * u * np.abs(t['terms']).sum(0)
    dr1 = dbil.sum(1) + _tree_depth(kernel, N) * u * np.abs(t['bil']).sum(1)
    # chamfer: the distance to the arg-min particle
    rows = np.arange(t['B'])[:, None]
    a = t['arg']
    dx = t['goal'][None, :, 0] - t['u'][rows, a]                               # [B,M]
    dy = t['goal'][None, :, 1] - t['v'][rows, a]
    ddx, ddy = du[rows, a] + u * np.abs(dx), dv[rows, a] + u * np.abs(dy)      # 1 sub
    dist = t['dist']
    pos = dist > 0.0
    sd = np.where(pos, dist, 1.0)
    # d2 = dx dx + dy dy: 2 mul + 1 add = 2 u d2, through the root u dist; the root 1: 2 u dist.  At dist == 0: | |a| - |b| | <= |a - b|
    ddist = np.where(pos, (np.abs(dx) * ddx + np.abs(dy) * ddy) / sd + 2 * u * dist, ddx + ddy)
    dr2 = ddist.sum(1) + _tree_depth(kernel, M) * u * dist.sum(1)
    mag = np.abs(t['r1']) + np.abs(t['r2'])
    draw = dr1 + dr2 + u * mag                                                 # 1 add
    dval = draw / N + u * mag / N                                              # 1 div
    # gradient: the bilinear addend scale * dg * m
    ex0, ex1 = np.abs(t['taps'][1] - t['taps'][0]), np.abs(t['taps'][3] - t['taps'][2])
    ey0, ey1 = np.abs(t['taps'][2] - t['taps'][0]), np.abs(t['taps'][3] - t['taps'][1])
    # dg = e (1 - t') + e' t': per product 1 sub (e) + 1 mul, then 1 add: 3 u
    ddgx = ex0 * dB + ex1 * dty + 3 * u * (ex0 * Bw + ex1 * ty)
    ddgy = ey0 * dA + ey1 * dtx + 3 * u * (ey0 * A + ey1 * tx)
    s = t['scale']
    da0x = s * t['mx'] * ddgx + 4 * u * np.abs(t['a0x'])                       # scale = 1 / N, m = W / H, 2 mul
    da0y = s * t['my'] * ddgy + 3 * u * np.abs(t['a0y'])                       # scale = 1 / N, 2 mul (m = 1)
    # the chamfer addend -scale (q - p) / dist: 1 / N, 1 mul, 1 div; the unit vector moves with p and with dist
    dcx = np.where(pos, s * (ddx / sd + np.abs(dx) * ddist / (sd * sd)) + 3 * u * np.abs(t['cx_add']), 0.0)
    dcy = np.where(pos, s * (ddy / sd + np.abs(dy) * ddist / (sd * sd)) + 3 * u * np.abs(t['cy_add']), 0.0)
    dgu, dgv = da0x.copy(), da0y.copy()
    sumx, sumy = np.abs(t['a0x']), np.abs(t['a0y'])
    k = np.zeros(t['u'].shape)
    for b in range(t['B']):
        np.add.at(dgu[b], a[b], dcx[b])
        np.add.at(dgv[b], a[b], dcy[b])
        np.add.at(sumx[b], a[b], np.abs(t['cx_add'][b]))
        np.add.at(sumy[b], a[b], np.abs(t['cy_add'][b]))
        np.add.at(k[b], a[b], 1.0)
    if kernel == 'kg_reward':
        adds = k                                                               # the k chamfer addends join the sum in turn
        quant = 0.0
    else:
        adds = 1.0                                                             # integer adds are exact; 1 conversion to fp32
        quant = ((1.0 + k) + 1.0) * 2.0 ** -41 if kernel == 'kb_reward' else 0.0   # every addend rounded to 2^-40 fixed point
    dgu = dgu + adds * u * sumx + quant
    dgv = dgv + adds * u * sumy + quant
    gu, gv = t['gu'], t['gv']
    dg = np.empty(t['grad'].shape)
    dg[..., 0] = dgu * np.abs(fx / z) + 2 * u * np.abs(gu * fx / z)            # 1 mul, 1 div
    dg[..., 1] = dgv * np.abs(fy / z) + 2 * u * np.abs(gv * fy / z)
    tz = np.abs(gu * x * fx) + np.abs(gv * y * fy)
    # 2 mul per product, 1 add, z z, 1 div: 5 u
    dg[..., 2] = (dgu * np.abs(x * fx) + dgv * np.abs(y * fy)) / (z * z) + 5 * u * tz / (z * z)
    return dict(value=2.0 * dval, value_raw=2.0 * draw, grad=2.0 * dg)


def ratio(got, want, bnd):
    """max |got - want| / bound, NaN or inf in `got` counting as inf; 0 / 0 (an exact zero held to a zero bound) as 0"""
    got, want, bnd = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bnd, np.float64)
    err = np.abs(got - want)
    err = np.where(np.isfinite(got), err, np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0.0, 0.0, err / bnd)
    return float(r.max()) if r.size else 0.0
