"""Fuzz the three neighbour-list kernels against the host oracle (oracle/propnet_sparse.build_neighbours) and against each
other: plain sweep (k_graph), x strips (k_graph_strips), two-dimensional cells (k_graph_cells, forced for every size, random
band height and first halo) -- random particle counts, batch sizes (so that the rounded-up grids of spread_item() have idle
workgroups), pile shapes (uniform, blob, a line along x, a line along y -- tests/_graph_edge_cases.py's --, clusters of
coincident particles, lattice = exact distance ties), scales and radii (0.05 and 0.1 among them: the radii whose threshold
differs when the fp32 rounding of the radius is squared).  Lists must agree bit for bit.  The suite's own edge cases (pairs an
ulp from the radius, strip and band boundaries) are tests/test_gpu_graph_edges.py.   python tools/fuzz_graph.py [cases] [seed]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _graph_edge_cases as edge_cases
from dyn_res_pile_manip_amd import synthetic as syn, weights
from dyn_res_pile_manip_amd.planners import world2cam_affine
from oracle import propnet_sparse as osp


def engine(env, radius):
    from dyn_res_pile_manip_amd.engine import Engine
    for k in ('DRP_NO_GRAPH_STRIPS', 'DRP_NO_GRAPH_CELLS', 'DRP_GRAPH_CELLS_MIN_N', 'DRP_GRAPH_CELLS_HB', 'DRP_GRAPH_CELLS_HALO'):
        os.environ.pop(k, None)
    os.environ.update(env)
    e = Engine(0)
    e.load_weights(BLOB, radius)
    e.set_camera(M34, 24.0, syn.demo_cam_params())
    return e


def pile(rng, N, kind):
    if kind in ('xline', 'yline'):
        return edge_cases.line_pile(rng, N, 0 if kind == 'xline' else 1)
    s = np.empty((N, 3), np.float64)
    if kind == 'uniform':
        s[:, :2] = rng.uniform(-0.2, 0.2, (N, 2))
    elif kind == 'blob':
        r = 0.12 * np.sqrt(rng.uniform(0, 1, N)); th = rng.uniform(0, 2 * np.pi, N)
        s[:, 0] = r * np.cos(th); s[:, 1] = r * np.sin(th)
    elif kind == 'dupes':
        c = rng.uniform(-0.2, 0.2, (max(N // 12, 1), 2))
        s[:, :2] = c[rng.integers(0, len(c), N)]
    elif kind == 'lattice':
        m = int(np.ceil(np.sqrt(N)))
        g = np.stack(np.meshgrid(np.arange(m), np.arange(m)), -1).reshape(-1, 2)[:N]
        s[:, :2] = (g - m / 2) * (0.4 / m)
    s[:, 2] = 0.75 - (rng.uniform(0, 0.01, N) if kind not in ('dupes', 'lattice') else 0.0)
    return s


cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
BLOB = weights.blob_from_state_dict(weights.random_state_dict(seed=0))
M34 = world2cam_affine(syn.demo_cam_extrinsics())
bad = 0
for c in range(cases):
    N = int(rng.choice([rng.integers(129, 400), rng.integers(400, 1300), rng.integers(1300, 3000)], p=[0.4, 0.4, 0.2]))
    B = int(rng.integers(1, 12))
    kind = str(rng.choice(['uniform', 'blob', 'xline', 'yline', 'dupes', 'lattice']))
    scale = float(rng.choice([0.3, 1.0, 1.0, 2.5]))
    radius = float(rng.choice([0.02, 0.05, 0.08, 0.08, 0.1, 0.3]))
    hb = float(rng.choice([0.02, 0.035, 0.05, 0.09, 0.2, 0.7]))
    halo = float(rng.choice([0.005, 0.02, 0.04, 0.1]))
    s = np.stack([pile(rng, N, kind) for _ in range(B)]).astype(np.float32)
    s[..., :2] *= scale
    sd = np.zeros_like(s) if kind in ('dupes', 'lattice') else (0.004 * rng.standard_normal(s.shape)).astype(np.float32)
    oidx, ocnt = osp.build_neighbours(s, sd, radius)
    ref = (oidx.astype(np.int16), ocnt.astype(np.uint8))
    for name, env in (('plain', {'DRP_NO_GRAPH_STRIPS': '1'}), ('strips', {'DRP_NO_GRAPH_CELLS': '1'}),
                      ('cells', {'DRP_GRAPH_CELLS_MIN_N': '1', 'DRP_GRAPH_CELLS_HB': repr(hb), 'DRP_GRAPH_CELLS_HALO': repr(halo)})):
        e = engine(env, radius)
        idx, cnt = e.build_graph(s, sd)
        e.close()
        if not (np.array_equal(idx, ref[0]) and np.array_equal(cnt, ref[1])):
            bad += 1
            print('MISMATCH %s against the oracle: case %d N=%d B=%d %s scale=%g radius=%g hb=%g halo=%g: %d rows differ' %
                  (name, c, N, B, kind, scale, radius, hb, halo, int((idx != ref[0]).any(-1).sum())))
print('%d cases, %d mismatches' % (cases, bad))
sys.exit(1 if bad else 0)
