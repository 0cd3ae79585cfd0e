"""CPU: the harness of tests/test_gpu_wgrad_cw.py (tests/_wgrad_ref.py) held against a float32 restatement of the kernels' own
summation order, and against mutants of it.

1. emulate32 -- wgrad_valu_body's row striding, the wave merges, the reduce kernel's tree and the targets' lists in numpy
   float32 -- stays inside the derived bound on random normal operands with a heavy-tailed g (every column of g scaled by
   10 ** uniform(-6, 0)), at row counts around every edge of the kernels (one row, odd counts, 64-row blocks, the 128-block
   cap) and the four input widths the trainer queues.
2. The depth D of the bound equals the additions counted while emulate32 executes them.
3. Six mutants leave the bound (ratio > 1) in the stated tensors and stay inside it everywhere else.  The norm-wise rule of
   the gradient tests, 2e-4 x max |g| per tensor, is printed beside each.  It PASSES (b) x rounded to 11 significant bits --
   at 0.27 and 0.43 of its tolerance -- and (f) small entries zeroed, by construction: the gap this bound closes.  At these
   sizes (129 rows) it catches the other four: (a) a dropped row (a hundredth of a sum here; 1e-4 of one at a workload's
   12 000 rows), (c) the density column one sample off (2.3 x its tolerance), (d) columns k >= in read and (e) a dropped job.

   The mutants' operands are not centred: x is clamped at zero and g carries a component common to its rows (normal + 1), as
   the rows of a backward pass do -- activations are non-negative and no bias gradient sum_rows g is zero.  On centred iid
   operands a sum and its rounding error are both random walks over the same terms, so mutant (b) sits AT the old rule's
   tolerance whatever the data (the rms relative error of rounding to 11 bits is 2^-12 sqrt(2 / 3) = 2.0e-4 of a term), which
   shows nothing either way; test_mutant_b_on_centred_operands prints that figure and holds the new bound to it as well."""
import numpy as np
import pytest

import _wgrad_ref as R

# (769, 900, 1800, 2817: 13, 15, 29 and 45 blocks -- 13..15 mod 16, where the reduce tree's longest chain is not wave 0's)
MS = (1, 2, 3, 33, 63, 64, 65, 127, 129, 511, 513, 769, 900, 1800, 2817, 8191, 8193, 9000)
INS = (3, 5, 6, 64)


def make_job(M, IN, dW, lane_stride, k_stride=1, db=-1, dwd=-1, rps=1, dens_mod=1):
    return {'M': M, 'in': IN, 'rows_per_sample': rps, 'dens_mod': dens_mod, 'blocks': min(R.MAX_BLOCKS, -(-M // 64)),
            'lane_stride': lane_stride, 'k_stride': k_stride, 'dW': dW, 'db': db, 'dwd': dwd, 'dens': int(dwd >= 0)}


def operands(rng, M, ldx, col_scale, centred=True):
    """g [M, 64] normal with heavy-tailed columns, x [M, ldx] normal.  Not centred: the rows of a backward pass -- x clamped at
    zero (an activation), g with a component common to the rows (normal + 1: a bias gradient sum_rows g is not zero)"""
    g, x = rng.standard_normal((M, 64)), rng.standard_normal((M, ldx))
    if not centred:
        g, x = g + 1.0, np.maximum(x, 0.0)
    return (g * col_scale).astype(np.float32), x.astype(np.float32)


def one_target(rng, M, IN, extras, n_jobs, samples=3):
    """a propagator-like target: W [64][IN (+ 1 density column)], a bias, the column sums of a [M, 3] behind them"""
    ld = IN + 1 if extras else IN
    n_w = 64 * ld
    rps = max(1, -(-M // samples))
    job = make_job(M, IN, 0, ld, 1, n_w if extras else -1, IN if extras else -1, rps if extras else 1, samples if extras else 1)
    jobs = [dict(job) for _ in range(n_jobs)] + [{**make_job(M, 3, -1, 0, 0), 'db': n_w + 64, 'blocks': 0}]
    scale = 10.0 ** rng.uniform(-6, 0, 64)
    ops = [operands(rng, M, IN, scale) for _ in range(n_jobs)]
    ops.append(((rng.standard_normal((M, 3)) * scale[:3]).astype(np.float32), None))
    dens = rng.uniform(100, 900, samples).astype(np.float32)
    tensors = [('W', (64, ld)), ('b', (64,)), ('cs', (3,))]
    return jobs, ops, dens, tensors, n_w + 64 + 3


@pytest.mark.parametrize('IN', INS)
@pytest.mark.parametrize('M', MS)
def test_the_kernels_order_in_float32_stays_inside_the_bound(M, IN):
    rng = np.random.default_rng(1000 * IN + M)
    # every combination up to 513 rows; at the block cap the two that differ in every respect (a case there is 0.5 M entries)
    combos = [(e, n) for e in (True, False) for n in (1, 3)] if M <= 513 else [(True, 2), (False, 1)]
    for extras, n_jobs in combos:
        jobs, ops, dens, tensors, n = one_target(rng, M, IN, extras, n_jobs)
        blob64, blob_abs, depth, rows, cover = R.reconstruct(jobs, ops, dens, mfma=False, n_blob=n)
        dev, count = R.emulate32_blob(jobs, ops, dens, n_blob=n)
        r = R.ratio(dev, blob64, blob_abs, depth, rows, tensors)
        print('[wgrad-cw host] M=%d in=%d extras=%d jobs=%d: D=%d, ratios %s' % (
            M, IN, extras, n_jobs, depth[0], {k: '%.3f' % v for k, v in r.items()}))
        assert max(r.values()) <= 1.0, (M, IN, extras, n_jobs, r)
        # 2. the derived depth is the executed one, entry by entry
        np.testing.assert_array_equal(depth[cover > 0], count[cover > 0])
        if extras:
            R.check_coverage_and_zeros(dev, blob_abs, cover)
        else:
            assert (cover[64 * IN:64 * IN + 64] == 0).all() and not dev[64 * IN:64 * IN + 64].any()


def test_depth_by_hand():
    """the formula at figures worked out from the kernels' loops by hand"""
    assert R.tree_len(1) == 1 + 4 and R.tree_len(4) == 1 + 4 and R.tree_len(5) == 2 + 4
    assert R.tree_len(12) == 3 + 4                          # no wave has a round: partials 0, 4, 8 into wave 0's t0
    # 13 blocks: wave 0 one round (0, 4, 8, 12 into t0..t3) and nothing left; wave 1 no round (1 + 12 < 13 fails), 1, 5, 9 into t0
    assert R.tree_len(13) == 3 + 4 and R.tree_len(14) == 3 + 4 and R.tree_len(15) == 3 + 4
    assert R.tree_len(16) == 1 + 4 and R.tree_len(17) == 2 + 4      # every wave one round; then block 16 into wave 0's t0
    assert R.tree_len(29) == 4 + 4 and R.tree_len(45) == 5 + 4      # wave 1: one / two rounds, then three partials one by one
    assert R.tree_len(128) == 8 + 4
    assert R.chain_len(9000, 128, False) == 18 and R.chain_len(9000, 128, True) == 2 * 9
    assert R.chain_len(3, 1, False) == 1 and R.chain_len(3, 1, True) == 2
    assert R.chain_len(51, 1, False) == 13 and R.chain_len(51, 1, True) == 2 * 7
    assert R.colsum_depth(1025) == 2 + 22


def test_depth_equals_the_counted_additions_at_every_block_count():
    """1 .. 128 workgroups, the last one a row short of full: the derived D against the additions emulate32 executes"""
    rng = np.random.default_rng(5)
    for blocks in range(1, R.MAX_BLOCKS + 1):
        M = 64 * blocks - 1
        job = make_job(M, 3, 0, 3)
        assert job['blocks'] == blocks
        g, x = operands(rng, M, 3, 1.0)
        _, counted = R.emulate32(job, g, x)
        assert R.job_depth(job, False) == counted, (blocks, R.job_depth(job, False), counted)


# ---- 3. mutants ----------------------------------------------------------------------------------------------------------
M_MUT = 129
TENSORS = [('A.weight', (64, 65)), ('A.bias', (64,)), ('B.weight', (64, 5)), ('B.bias', (64,)), ('cs', (3,))]
OFF_A, OFF_AB, OFF_B, OFF_BB, OFF_CS = 0, 64 * 65, 64 * 65 + 64, 64 * 65 + 64 + 320, 64 * 65 + 64 + 320 + 64
N_MUT = OFF_CS + 3


def scenario(centred=False):
    """target A: three jobs of 129 rows, in = 64, a density column (3 samples of 43 rows) and a bias -- the particle
    propagator's shape; target B: one job with in = 5 out of rows of 8 floats and a bias -- the particle encoder's"""
    rng = np.random.default_rng(7)
    scale = 10.0 ** rng.uniform(-6, 0, 64)
    a = make_job(M_MUT, 64, OFF_A, 65, 1, OFF_AB, OFF_A + 64, 43, 3)
    b = make_job(M_MUT, 5, OFF_B, 5, 1, OFF_BB)
    jobs = [dict(a), dict(a), dict(a), b, {**make_job(M_MUT, 3, -1, 0, 0), 'db': OFF_CS, 'blocks': 0}]
    ops = [operands(rng, M_MUT, 64, scale, centred) for _ in range(3)] + [operands(rng, M_MUT, 8, scale, centred)]
    ops.append(((rng.standard_normal((M_MUT, 3)) * scale[:3]).astype(np.float32), None))
    dens = np.array([300.0, 350.0, 400.0], np.float32)
    return jobs, ops, dens


def run_mutant(name, centred=False):
    jobs, ops, dens = scenario(centred)
    true_ops = [(g, x[:, :j['in']].copy() if x is not None else None) for j, (g, x) in zip(jobs, ops)]
    blob64, blob_abs, depth, rows, cover = R.reconstruct(jobs, true_ops, dens, mfma=False, n_blob=N_MUT)
    mj, mo = [dict(j) for j in jobs], list(ops)
    post = None
    if name == 'none':
        pass
    elif name == 'a':                       # the last row dropped when M is odd
        assert M_MUT % 2 == 1
        for q in range(4):
            mj[q]['M'] -= 1
            mj[q]['blocks'] = min(R.MAX_BLOCKS, -(-mj[q]['M'] // 64))
            mo[q] = (ops[q][0][:-1], ops[q][1][:-1])
    elif name == 'b':                       # x rounded to 11 significant bits
        for q in range(4):
            m, e = np.frexp(ops[q][1])
            mo[q] = (ops[q][0], np.ldexp(np.round(m * 2048.0) / 2048.0, e).astype(np.float32))
    elif name == 'c':                       # the density column's sample index one row early at each boundary
        pass
    elif name == 'd':                       # columns k >= in not read as zero (and what they sum to scattered with the job's strides)
        mj[3] = {**mj[3], 'in': 8}
    elif name == 'e':                       # one job left out of a target's list of three
        del mj[1], mo[1]
    elif name == 'f':                       # every entry below 2e-4 x its tensor's largest set to zero
        def post(blob):
            off = 0
            for _, shape in TENSORS:
                n = int(np.prod(shape))
                t = blob[off:off + n]
                t[np.abs(t) < 2e-4 * np.abs(t).max()] = 0.0
                off += n
            return blob
    else:
        raise KeyError(name)
    def shifted(job, d):                    # (c): the sample index of the row behind
        row = np.arange(job['M'], dtype=np.int64) + 1
        return (np.asarray(d, np.float32) / R.DENS_SCALE)[(row // job['rows_per_sample']) % job['dens_mod']]
    dev, _ = R.emulate32_blob(mj, mo, dens, n_blob=N_MUT, dens_rows_fn=shifted if name == 'c' else R.dens_rows)
    if post is not None:
        dev = post(dev)
    new = R.ratio(dev, blob64, blob_abs, depth, rows, TENSORS)
    old = R.old_rule(dev, blob64, TENSORS)
    print('[wgrad-cw host] mutant %s: componentwise ratio %s' % (name, {k: '%.3g' % v for k, v in new.items()}))
    print('[wgrad-cw host] mutant %s: old rule, error / (2e-4 max|g|) %s' % (name, {k: '%.3g' % v for k, v in old.items()}))
    return new, old


def test_the_unmutated_scenario_is_inside_both_rules():
    new, old = run_mutant('none')
    assert max(new.values()) <= 1.0 and max(old.values()) <= 1.0


# mutant -> (the tensors in which it must leave the bound, whether the old rule passes it in EVERY tensor)
MUTANTS = {
    'a': (('A.weight', 'A.bias', 'B.weight', 'B.bias'), False),
    'b': (('A.weight', 'B.weight'), True),
    'c': (('A.weight',), False),
    'd': (('B.weight', 'B.bias'), False),               # (lane 63's columns 5..7 land behind the weight, in the bias)
    'e': (('A.weight', 'A.bias'), False),
    'f': (('A.weight', 'A.bias', 'B.weight', 'B.bias'), True),
}


@pytest.mark.parametrize('name', sorted(MUTANTS))
def test_mutants_leave_the_bound(name):
    where, old_passes = MUTANTS[name]
    new, old = run_mutant(name)
    assert where, name
    for key in where:
        assert new[key] > 1.0, (name, key, new[key])
    for key, _ in TENSORS:                  # and nowhere else: the mutant touches nothing but what it says
        if key not in where:
            assert new[key] <= 1.0, (name, key, new[key])
    assert (max(old.values()) <= 1.0) == old_passes, (name, old)


def test_mutant_b_on_centred_operands():
    new, old = run_mutant('b', centred=True)
    assert new['A.weight'] > 1.0 and new['B.weight'] > 1.0
    assert max(new[k] for k in ('A.bias', 'B.bias', 'cs')) <= 1.0
