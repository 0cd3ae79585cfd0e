"""CPU: the row layout of a multi-scene session (include/drp.h: drp_mpc_begin_scenes) -- scene_rows and the interleave helpers
of engine.py against a brute-force loop.  Pure numpy: no device, no library."""
import numpy as np
import pytest

from dyn_res_pile_manip_amd.engine import Engine, interleave_scenes, scene_rows, split_scenes

SHAPES = [(S, u, nb) for S in (1, 2, 3, 5) for nb in (1, 2, 3) for u in (1, 2, 7)]


def brute_rows(S, n_units, nb):
    rows = [[] for _ in range(S)]
    r = 0
    for u in range(n_units):
        for k in range(S):
            for c in range(nb):
                rows[k].append(r)
                r += 1
    return np.array(rows, dtype=np.int64)


@pytest.mark.parametrize('S,n_units,nb', SHAPES)
def test_scene_rows_is_the_loop(S, n_units, nb):
    rows = scene_rows(S, n_units, nb)
    assert rows.shape == (S, n_units * nb)
    np.testing.assert_array_equal(rows, brute_rows(S, n_units, nb))
    # every row of the session belongs to exactly one scene
    np.testing.assert_array_equal(np.sort(rows.reshape(-1)), np.arange(S * n_units * nb))
    for k in range(S):
        # the rollout's rule: scene(row) = (row // nb) % S, and row % (S * nb) is the start column (scene-major columns)
        np.testing.assert_array_equal((rows[k] // nb) % S, k)
        np.testing.assert_array_equal(rows[k] % (S * nb), k * nb + np.tile(np.arange(nb), n_units))
        # within a scene the rows keep a single-scene session's order: unit * nb + column
        np.testing.assert_array_equal(rows[k] // (S * nb) * nb + rows[k] % nb, np.arange(n_units * nb))


@pytest.mark.parametrize('S,n_units,nb', SHAPES)
def test_interleave_and_split_round_trip(S, n_units, nb):
    rng = np.random.default_rng(S * 100 + n_units * 10 + nb)
    per = rng.normal(size=(S, n_units * nb, 3, 4)).astype(np.float32)
    sess = interleave_scenes(per, nb)
    assert sess.shape == (S * n_units * nb, 3, 4) and sess.dtype == per.dtype
    ref = np.empty_like(sess)
    rows = brute_rows(S, n_units, nb)
    for k in range(S):
        for q in range(n_units * nb):
            ref[rows[k, q]] = per[k, q]
    np.testing.assert_array_equal(sess, ref)
    np.testing.assert_array_equal(split_scenes(sess, S, nb), per)
    np.testing.assert_array_equal(interleave_scenes(list(per), nb), sess)          # a sequence of S arrays
    # one-dimensional per-row values (rewards)
    r = rng.normal(size=(S, n_units * nb))
    np.testing.assert_array_equal(split_scenes(interleave_scenes(r, nb), S, nb), r)


def test_one_scene_is_the_identity():
    a = np.arange(12.0).reshape(1, 6, 2)
    np.testing.assert_array_equal(interleave_scenes(a, 3), a[0])
    np.testing.assert_array_equal(split_scenes(a[0], 1, 3), a)


def test_bad_shapes_raise():
    with pytest.raises(ValueError):
        scene_rows(0, 1, 1)
    with pytest.raises(ValueError):
        interleave_scenes(np.zeros((2, 5)), 2)          # 5 rows are no multiple of nb = 2
    with pytest.raises(ValueError):
        split_scenes(np.zeros((7, 2)), 2, 2)


def test_the_engine_class_carries_the_helpers():
    np.testing.assert_array_equal(Engine.scene_rows(2, 2, 1), [[0, 2], [1, 3]])
    assert Engine.interleave_scenes is not None and Engine.split_scenes is not None
