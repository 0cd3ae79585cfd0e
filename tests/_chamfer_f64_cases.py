"""TEST INFRASTRUCTURE of the float64 Chamfer yardstick (drp_cloud_chamfer_f64, drp_train_grad_f64_untracked): the stand-alone
clouds its GPU tests add to those of tests/_untracked_ref.py -- built here so that tests/test_chamfer_f64_host.py can assert
their margins and tile crossings on the CPU, where the seeds were picked; no case is skipped at run time.

  tiling_case(shape)      (n_p, n_q) on the jittered lattices of tests/test_gpu_chamfer.py (different pitch per cloud, so every
                          arg-min margin is far above MARGIN_MIN): the sizes around the kernel's 256-row chunk and 1024-point tile
  boundary_case()         tests/test_gpu_chamfer.py's 258 x 1030 pair, the same draw
"""
import numpy as np

# around one 256-row chunk and one 1024-point tile in either direction; a single row against three tiles; the largest cloud
# (c(.) fills its LDS array) on either side
TILING_SHAPES = [(255, 1023), (256, 1024), (257, 1025), (1025, 257), (1, 2049), (300, 4096), (4096, 300)]
# seeds for which every margin is above MARGIN_MIN and, where the shape has a second tile or chunk, some arg-min lies in it
# (tests/test_chamfer_f64_host.py holds both)
TILING_SEED = {(255, 1023): 0, (256, 1024): 0, (257, 1025): 3, (1025, 257): 1, (1, 2049): 1, (300, 4096): 0, (4096, 300): 1}
TILE, CHUNK = 1024, 256


def lattice(rng, n, pitch, off):
    k = int(np.ceil(n ** (1.0 / 3.0)))
    g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing='ij'), -1).reshape(-1, 3)[rng.permutation(k ** 3)[:n]]
    return (0.1 + off + pitch * g + 0.2 * pitch * rng.random((n, 3))).astype(np.float32)


def tiling_case(shape, seed=None):
    """-> (p [1, n_p, 3], q [1, n_q, 3] float32, n_p [1], n_q [1] int32), unpadded"""
    n_p, n_q = shape
    rng = np.random.default_rng(500 + (TILING_SEED[tuple(shape)] if seed is None else seed))
    p, q = lattice(rng, n_p, 0.031, 0.0)[None], lattice(rng, n_q, 0.02, 0.003)[None]
    return p, q, np.array([n_p], np.int32), np.array([n_q], np.int32)


def crossings(ref, shape):
    """which of the kernel's boundaries the reference's arg-mins cross for a shape, and which the shape has at all:
    -> {'tile': (has, crossed), 'chunk': (has, crossed)}.  A later tile: an arg-min at index >= 1024 of a cloud that has that
    many rows (both clouds pass through the tiles).  A later chunk: a target whose nearest predicted row is row >= 256, so a
    row of a later 256-row pass of the workgroup owns an entry of c(.) and gathers it (tests/test_gpu_chamfer.py's criterion)"""
    n_p, n_q = shape
    a, c = ref['nn_pq'][0, :n_p], ref['nn_qp'][0, :n_q]
    tile = [bool((a >= TILE).any())] * (n_q > TILE) + [bool((c >= TILE).any())] * (n_p > TILE)
    return {'tile': (len(tile) > 0, len(tile) > 0 and all(tile)), 'chunk': (n_p > CHUNK, bool((c >= CHUNK).any()))}


def boundary_case():
    """tests/test_gpu_chamfer.py: test_across_the_tile_and_chunk_boundaries' clouds (n_p = 258, n_q = 1030), the same draw"""
    rng = np.random.default_rng(5)
    p, q = lattice(rng, 258, 0.031, 0.0)[None], lattice(rng, 1030, 0.02, 0.003)[None]
    return p, q, np.array([258], np.int32), np.array([1030], np.int32)
