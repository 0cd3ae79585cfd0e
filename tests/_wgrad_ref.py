"""The trainer's weight-gradient sums, reconstructed in float64 from the rows the device summed over, and their fp32 error bound.

numpy only: no device, no library.  The kernels under test (csrc/k_train.h) compute plain fp32 sums

    dW[lane * lane_stride + k * k_stride] += sum_rows g[row][lane] * x[row][k]                              k < in
    db[lane]                              += sum_rows g[row][lane]
    dwd[lane * lane_stride]               += sum_rows g[row][lane] * (dens[(row / rows_per_sample) % dens_mod] / 5000)

over rows that the backward kernels left in device memory.  Given those rows (the debug taps "train_wgrad_*", engine.py:
train_wgrad_tap) the exact sums are float64 matmuls, and the fp32 result has the textbook bound of a sum of products:

    |fl(sum) - sum| <= (D + 2) u sum |g| |x|  +  rows 2^-126,        u = 2^-24

where D, the summation depth, is the largest number of fp32 additions a term passes through on its way into the blob.  The 2
covers the rounding of the product (none under fmaf, one where the matrix cores round it) with one to spare for the second-order
terms of (1 + u)^D; the last term covers products and partial sums flushed to zero on the matrix cores, one per row at most.

D IS DERIVED FROM THE KERNELS, NOT MEASURED (line numbers: csrc/k_train.h).  A job of M rows on `blocks` workgroups:

  chain    kt_wgrad_multi / kt_wgrad_list (wgrad_valu_body, l. 220-262): wave w of block b walks rows 4 b + w + 4 blocks t
           (l. 231), one fmaf per row into acc[k] (l. 235; bias l. 236, density column l. 237).  The longest chain is that of
           block 0, wave 0:                                                  L = ceil(M / (4 blocks)) additions.
           kt_wgrad_mfma_multi / _list (wgrad_mfma_body, l. 310-401): the same striding over row PAIRS (2p, 2p + 1), p = 4 b + w
           + 4 blocks t (l. 327-328, 343-346); one v_mfma_f32_32x32x2_f32 per pair adds two products into the accumulator
           (l. 350-354), counted as two additions:                            L = 2 ceil(ceil(M / 2) / (4 blocks)).
           (Its bias and density columns are per-lane sums over one row of each pair, ceil(M / 2) / (4 blocks) additions, and
           one more for even + odd (l. 363-368): never more than L.)
  merge    waves 1..3 park their sums in LDS, wave 0 adds them in wave order (l. 247-255 / 385-398):          3 additions.
  tree     kt_wgrad_reduce_multi / kt_wgrad_reduce_lists (l. 277-301 / 418-450): wave w adds the partials w, w + 4, ... into four
           running sums t0..t3 -- sixteen partials a round while b + 12 < blocks, the rest into t0 (l. 434-440) -- then
           (t0 + t1) + (t2 + t3) (l. 442) and (s0 + s1) + (s2 + s3) over the waves (l. 444).  The longest chain is a t0, but not
           always wave 0's: with blocks = 13, 14 or 15 mod 16 wave 0 ends in whole rounds, while a later wave fails `b + 12 <
           blocks` a round earlier and adds that round's partials -- up to four -- into t0 one by one (blocks = 13: wave 0 one
           round, t0 one addition; wave 1 no round, partials 1, 5, 9 into t0, three additions).  So
                                                                              R = max over w of (rounds(w) + rest(w)) + 2 + 2.
  list     kt_wgrad_reduce_lists adds the sums of the jobs of one target in list order into `tot` (l. 428, 444):
                                                                              J additions for J jobs.
           (`dW += tot`, l. 447-449, adds into the zero the loss kernel left: exact, not counted.)

                                           D = L + 3 + R + J

kt_colsum3 (l. 456-473): a strided pass per thread, ceil(M / 1024) additions; wave_sum, 6; the 16 waves' sums in order, 16:
D = ceil(M / 1024) + 22.  Its `out += t` meets a zero as well.

What this holds: the sums, given the device's rows.  What it does not: the rows themselves (they stay under the float64
yardstick's norm-wise bound, tests/test_gpu_train_f64.py), and a job that was never queued (it is in neither side)."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
DENS_SCALE = np.float32(5000.0)
N_BLOB = 38403
MAX_BLOCKS = 128


def chain_len(M, blocks, mfma):
    """L: the additions of the longest (block, wave) chain"""
    if mfma:
        return 2 * -(-((M + 1) // 2) // (4 * blocks))
    return -(-M // (4 * blocks))


def tree_len(blocks):
    """R: the additions a partial passes through in the reduce kernel -- the longest t0 of the four waves, then the two pairings"""
    longest = 0
    for w in range(4):
        b, n = w, 0
        while b + 12 < blocks:              # a round of sixteen: one addition into each of t0..t3
            b += 16
            n += 1
        while b < blocks:                   # the rest, into t0
            b += 4
            n += 1
        longest = max(longest, n)
    return longest + 2 + 2


def job_depth(job, mfma):
    """L + 3 + R of one job: everything but the target's list"""
    return chain_len(job['M'], job['blocks'], mfma) + 3 + tree_len(job['blocks'])


def colsum_depth(M):
    return -(-M // 1024) + 6 + 16


def dens_rows(job, dens):
    """the fp32 quotient dens / 5000 every row of the job multiplies by (l. 237 / 337), as float32 [M]"""
    row = np.arange(job['M'], dtype=np.int64)
    dq = np.asarray(dens, np.float32) / DENS_SCALE
    return dq[(row // job['rows_per_sample']) % job['dens_mod']]


def job_entries(job):
    """(offsets [64, in] of dW, offsets [64] of db or None, offsets [64] of dwd or None) inside the blob"""
    lane = np.arange(64, dtype=np.int64)[:, None]
    k = np.arange(job['in'], dtype=np.int64)[None, :]
    w = job['dW'] + lane * job['lane_stride'] + k * job['k_stride']
    b = job['db'] + lane[:, 0] if job['db'] >= 0 else None
    d = job['dwd'] + lane[:, 0] * job['lane_stride'] if job['dwd'] >= 0 else None
    return w, b, d


def check_bounds(jobs, n_blob=N_BLOB):
    """every job writes inside the blob; the jobs of one target (one dW: what the reduce kernel keys its lists on) agree in
    everything it takes from the list's first job; two targets share no entry"""
    seen = np.zeros(n_blob, np.int64)
    targets = {}
    for q, job in enumerate(jobs):
        assert 1 <= job['in'] <= 64 and job['M'] >= 1 and 1 <= job['blocks'] <= MAX_BLOCKS, (q, job)
        assert job['blocks'] == min(MAX_BLOCKS, -(-job['M'] // 64)), (q, job)
        key = tuple(job[f] for f in ('M', 'in', 'lane_stride', 'k_stride', 'db', 'dwd'))
        if job['dW'] in targets:
            assert targets[job['dW']] == key, (q, job)
            continue
        targets[job['dW']] = key
        for off in job_entries(job):
            if off is not None:
                assert off.min() >= 0 and off.max() < n_blob, (q, int(off.min()), int(off.max()))
                seen[off.ravel()] += 1
    assert seen.max() <= 1, 'two targets (or two entries of one) share a blob entry: %s' % np.flatnonzero(seen > 1)[:8]


def reconstruct(jobs, operands, dens, mfma=True, n_blob=N_BLOB):
    """jobs: the job table (dicts of M, in, rows_per_sample, dens_mod, blocks, lane_stride, k_stride, dW, db, dwd, dens), the
    last one the column sums' (M, db); operands: (g [M,64], x [M,in]) float32 per job and (g [M,3], None) for the column sums;
    dens: the float32 densities.  mfma: which kernel summed (the chain length differs).
    -> (blob64, blob_abs, depth, rows, cover): per blob entry the float64 sum, the same with |g| |x|, the summation depth D, the
    rows summed and the number of jobs that wrote it."""
    blob64, blob_abs = np.zeros(n_blob), np.zeros(n_blob)
    depth, rows, cover = np.zeros(n_blob, np.int64), np.zeros(n_blob, np.int64), np.zeros(n_blob, np.int64)
    check_bounds(jobs[:-1], n_blob)

    def add(off, val, val_abs, d, m):
        off = off.ravel()
        blob64[off] += val.ravel()
        blob_abs[off] += val_abs.ravel()
        depth[off] = np.maximum(depth[off], d)
        rows[off] += m
        cover[off] += 1

    for job, (g, x) in zip(jobs[:-1], operands[:-1]):
        M = job['M']
        assert g.dtype == np.float32 and x.dtype == np.float32 and g.shape == (M, 64) and x.shape == (M, job['in'])
        g64, x64 = g.astype(np.float64), x.astype(np.float64)
        d = job_depth(job, mfma)
        w, b, dw = job_entries(job)
        add(w, g64.T @ x64, np.abs(g64).T @ np.abs(x64), d, M)
        if b is not None:
            add(b, g64.sum(0), np.abs(g64).sum(0), d, M)
        if dw is not None:
            assert job['dens'], 'a density column that reads no density'
            dq = dens_rows(job, dens).astype(np.float64)
            add(dw, g64.T @ dq, np.abs(g64).T @ np.abs(dq), d, M)
    depth += cover                                  # J: one addition per job of the entry's target
    cs, (g, _) = jobs[-1], operands[-1]
    assert g.dtype == np.float32 and g.shape == (cs['M'], 3)
    off = cs['db'] + np.arange(3)
    assert not cover[off].any(), 'the column sums share their target with a job'
    add(off, g.astype(np.float64).sum(0), np.abs(g.astype(np.float64)).sum(0), colsum_depth(cs['M']), cs['M'])
    return blob64, blob_abs, depth, rows, cover


def bound(blob_abs, depth, rows):
    return (depth + 2) * U * blob_abs + rows * TINY


def ratio(blob_dev, blob64, blob_abs, depth, rows, tensors):
    """max over a tensor's entries of |dev - blob64| / bound; tensors: [(key, shape)] in blob order -> {key: ratio}"""
    blob_dev = np.asarray(blob_dev)
    assert blob_dev.dtype == np.float32 and blob_dev.shape == blob64.shape
    err, bnd = np.abs(blob_dev.astype(np.float64) - blob64), bound(blob_abs, depth, rows)
    with np.errstate(divide='ignore', invalid='ignore'):       # an entry nothing writes has a bound of 0: it must be 0.0
        r = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
    out, off = {}, 0
    for key, shape in tensors:
        n = int(np.prod(shape))
        out[key] = float(r[off:off + n].max())
        off += n
    assert off == blob64.size
    return out


def old_rule(blob_dev, blob_ref, tensors, tol=2e-4):
    """the norm-wise rule of the gradient tests: max |dev - ref| / max |ref| per tensor -> {key: that figure / tol}"""
    out, off = {}, 0
    for key, shape in tensors:
        n = int(np.prod(shape))
        a, b = np.asarray(blob_dev[off:off + n], np.float64), np.asarray(blob_ref[off:off + n], np.float64)
        out[key] = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300) / tol)
        off += n
    return out


def check_coverage_and_zeros(blob_dev, blob_abs, cover):
    """every entry is written by a job or the column sums; an entry whose terms are all zero is exactly 0.0 on the device"""
    assert (cover >= 1).all(), 'entries no job writes: %s' % np.flatnonzero(cover < 1)[:8]
    dead = blob_abs == 0
    bad = np.flatnonzero(dead & (np.asarray(blob_dev) != 0))
    assert not bad.size, 'entries with all-zero terms that are not 0.0: %s' % bad[:8]
    return int(dead.sum())


# ---- the VALU body's and the reduce kernel's order in numpy float32 (to exercise the harness and the mutants on the CPU) ------
def _fma32(a, b, c):
    """fmaf: the product of two floats is exact in double; one rounding to double (innocuous: 53 >= 2 * 24 + 2 but for
    cancellation-free ties, far inside the bound) and one to float"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate32(job, g, x, dq=None):
    """wgrad_valu_body + the per-job part of kt_wgrad_reduce_lists for one job: rows to (block, wave) chains, the three wave
    merges, the partial tree.  g [M, 64], x [M, >= in] float32 (columns k >= in are not read), dq: dens_rows(job, dens) for a job
    with a density column.  -> (sums [66, 64] float32: rows k < in the columns of dW^T, row 64 the bias, row 65 the density
    column; the largest number of additions a term passed through, counted as they are executed)."""
    M, IN, blocks = job['M'], job['in'], job['blocks']
    g = np.asarray(g, np.float32)
    x = np.asarray(x, np.float32)[:, :IN]
    nch = 4 * blocks                                        # chain c = 4 b + w
    acc = np.zeros((nch, 66, 64), np.float32)
    cnt = np.zeros(nch, np.int64)
    t = 0
    while t * nch < M:
        r0 = t * nch
        n = min(nch, M - r0)
        gv, xv = g[r0:r0 + n], x[r0:r0 + n]
        acc[:n, :IN] = _fma32(gv[:, None, :], xv[:, :, None], acc[:n, :IN])
        acc[:n, 64] = acc[:n, 64] + gv
        if dq is not None:
            acc[:n, 65] = _fma32(gv, np.asarray(dq, np.float32)[r0:r0 + n, None], acc[:n, 65])
        cnt[:n] += 1
        t += 1
    acc, cnt = acc.reshape(blocks, 4, 66, 64), cnt.reshape(blocks, 4)
    part, pc = acc[:, 0].copy(), cnt[:, 0].copy()
    for w in range(1, 4):
        part = part + acc[:, w]
        pc = np.maximum(pc, cnt[:, w]) + 1
    s_w, s_c = [], []
    for w in range(4):
        tt = [np.zeros((66, 64), np.float32) for _ in range(4)]
        tc = [0, 0, 0, 0]
        b = w
        while b + 12 < blocks:
            for i in range(4):
                tt[i] = tt[i] + part[b + 4 * i]
                tc[i] = max(tc[i], int(pc[b + 4 * i])) + 1
            b += 16
        while b < blocks:
            tt[0] = tt[0] + part[b]
            tc[0] = max(tc[0], int(pc[b])) + 1
            b += 4
        s_w.append((tt[0] + tt[1]) + (tt[2] + tt[3]))
        s_c.append(max(max(tc[0], tc[1]) + 1, max(tc[2], tc[3]) + 1) + 1)
    out = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3])
    return out, max(max(s_c[0], s_c[1]) + 1, max(s_c[2], s_c[3]) + 1) + 1


def emulate32_blob(jobs, operands, dens, n_blob=N_BLOB, dens_rows_fn=dens_rows):
    """kt_wgrad_reduce_lists over whole job lists and kt_colsum3's sums (in its order too): the float32 blob the kernels would
    leave, and per entry the additions counted.  jobs / operands / dens as reconstruct takes them; dens_rows_fn: what stands
    for dens_rows (a mutant's indexing)."""
    blob = np.zeros(n_blob, np.float32)
    count = np.zeros(n_blob, np.int64)
    tot, totc = {}, {}
    for job, (g, x) in zip(jobs[:-1], operands[:-1]):
        dq = dens_rows_fn(job, dens) if job['dwd'] >= 0 else None
        s, c = emulate32(job, g, x, dq)
        key = job['dW']
        if key not in tot:
            tot[key], totc[key] = (job, np.zeros((66, 64), np.float32)), 0
        tot[key] = (tot[key][0], tot[key][1] + s)
        totc[key] = max(totc[key], c) + 1
    for key, (job, s) in tot.items():
        w, b, d = job_entries(job)
        np.add.at(blob, w.ravel(), s[:job['in']].T.ravel())       # (add.at: a mutant's strides may hit an entry twice)
        count[w.ravel()] = totc[key]
        if b is not None:
            np.add.at(blob, b, s[64])
            count[b] = totc[key]
        if d is not None:
            np.add.at(blob, d, s[65])
            count[d] = totc[key]
    cs, (g, _) = jobs[-1], operands[-1]
    g = np.asarray(g, np.float32)
    M = cs['M']
    a = np.zeros((1024, 3), np.float32)
    ac = np.zeros(1024, np.int64)
    for r0 in range(0, M, 1024):
        n = min(1024, M - r0)
        a[:n] = a[:n] + g[r0:r0 + n]
        ac[:n] += 1
    a, c = a.reshape(16, 64, 3), int(ac.max())
    off = 32
    while off:
        a = a + a[:, np.arange(64) ^ off]
        c += 1
        off >>= 1
    tsum = np.zeros(3, np.float32)
    for w in range(16):
        tsum = tsum + a[w, 0]
        c += 1
    blob[cs['db'] + np.arange(3)] += tsum
    count[cs['db'] + np.arange(3)] = c
    return blob, count
