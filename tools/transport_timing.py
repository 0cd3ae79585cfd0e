"""Time the entropy-regularised transport loss (csrc/k_sinkhorn.h) next to the Chamfer and the matching loss it stands beside
-> profiles/transport_timing.txt.

  python tools/transport_timing.py [output file]

(a) device time of kt_transport for B x H = 20 problems in one launch at n = m in {20, 50, 100, 300} and at 100 x 130, at the
    default sweep count and eps = the squared spacing, and of kc_chamfer and ka_match on the same clouds: HIP events around the
    kernel (drp_probe_begin("loss")), the three interleaved launch by launch, the median of 21 rounds after 3 warm-up ones;
(b) a whole mode='update' step at 4 x 5 x 100 (B x n_rollout x N = M) under 'chamfer', 'match' and 'transport', interleaved on one
    context: host time of the call (it returns when the step is complete on the device), the median of 6 blocks of 10 after
    warm-up, as tools/match_timing.py measures its steps.
(c) python tools/transport_timing.py --divergence [output file] -> profiles/divergence_timing.txt: the Sinkhorn divergence
    (csrc/k_sinkhorn.h: kd_sweeps and kd_combine, one timed region) beside kt_transport on the same clouds, 20 problems at
    100 x 100 and 300 x 300, measured as (a); and a whole update at 4 x 5 x 100 under 'transport' and 'sinkhorn', measured as (b).
(d) python tools/transport_timing.py --divergence-f64 [output file] -> profiles/divergence_f64_timing.txt: the float64 yardstick
    (csrc/k_sinkhorn.h: kd64_sweeps and kd64_combine, one timed region) beside kd_sweeps + kd_combine on the same clouds
    (p widened exactly), 20 problems at 100 x 100 and 300 x 300, measured as (a).  A yardstick's cost, not an engine's.
(e) python tools/transport_timing.py --unbalanced [output file] -> profiles/divergence_unbalanced_timing.txt: the unbalanced
    divergence (kd_sweeps_unbalanced and kd_combine, one timed region; rho = 4 eps) beside the balanced kernels, interleaved on
    one context on the same clouds, 20 problems at 100 x 100 and 300 x 300, measured as (a); and a whole update at 4 x 5 x 100
    under 'sinkhorn' with and without a reach, measured as (b).
(f) python tools/transport_timing.py --unbalanced --f64 [output file] -> profiles/divergence_unbalanced_f64_timing.txt: the
    unbalanced float64 yardstick (csrc/k_sinkhorn.h: kd64_sweeps_unbalanced and kd64_combine_unbalanced, one timed region;
    rho = 4 eps) beside the balanced kd64 pair, interleaved on one context on the same clouds, 20 problems at 100 x 100 and
    300 x 300, measured as (a); and a whole Engine.train_gradient_probe call at 4 x 5 x 100 under 'sinkhorn' with and without a
    reach, measured as (b) in blocks of 3.  With --ab OLD.so NEW.so behind it (libraries as tools/ab.sh takes them: paths from the
    repository root) the balanced kd64 pair is also timed under each library in turn, three rounds interleaved OLD NEW OLD NEW ...,
    one process each: both builds' medians and the spread of OLD's own rounds -- the margin NEW is held to -- go into the file.
Each measurement runs in a child process of its own under a time limit (a stuck step ends there, and nothing follows it)."""
import os
import subprocess
import sys
import time

sys.path.insert(0, '.')
import numpy as np

SIZES = ((20, 20), (50, 50), (100, 100), (300, 300), (100, 130))
DIVERGENCE_SIZES = (100, 300)
PROBLEMS = 20
STEP_LIMIT_S = 120
SPACING = 0.02


def clouds(n, m, seed):
    rng = np.random.default_rng(seed)
    side = SPACING * max(n, m) ** (1.0 / 3.0)                       # the piles' scale: spacing about 0.02
    p = (0.2 + side * rng.random((PROBLEMS, n, 3))).astype(np.float32)
    q = (0.2 + side * rng.random((PROBLEMS, m, 3))).astype(np.float32)
    return p, q


def kernel_times(n, m):
    from dyn_res_pile_manip_amd import train_gnn_dyn as TG
    from dyn_res_pile_manip_amd.engine import Engine
    eng = Engine(0)
    p, q = clouds(n, m, 7 * n + m)
    eps, K = TG.TRANSPORT_EPS_SCALE * SPACING ** 2, TG.TRANSPORT_ITERS
    calls = (('kt_transport', lambda: eng.cloud_transport(p, q, eps=eps, iters=K, want_grad=True)),
             ('ka_match', lambda: eng.cloud_match(p, q, want_grad=True)),
             ('kc_chamfer', lambda: eng.cloud_chamfer(p, q, want_grad=True)))
    for _ in range(3):
        for _, call in calls:
            call()
    took = dict((name, []) for name, _ in calls)
    for _ in range(21):                                             # interleaved: every round times each form once
        for name, call in calls:
            eng.probe_begin('loss')
            call()
            ms, launches = eng.probe_read()
            assert launches == 1
            took[name].append(ms)
    eng.probe_begin(None)
    col_err = float(eng.cloud_transport(p, q, eps=eps, iters=K, want_col_err=True)['col_err'].max())
    eng.close()
    med = dict((name, float(np.median(took[name]))) for name in took)
    print('%d problems of %d x %d, K = %d: %s; kt_transport = %.1f x kc_chamfer = %.2f x ka_match; col_err at most %.1e'
          % (PROBLEMS, n, m, K, ', '.join('%s %.4f ms (%.4f .. %.4f)' % (name, med[name], min(took[name]), max(took[name]))
                                          for name, _ in calls),
             med['kt_transport'] / med['kc_chamfer'], med['kt_transport'] / med['ka_match'], col_err), flush=True)


def divergence_kernel_times(n, m):
    from dyn_res_pile_manip_amd import train_gnn_dyn as TG
    from dyn_res_pile_manip_amd.engine import Engine
    eng = Engine(0)
    p, q = clouds(n, m, 7 * n + m)
    eps, K = TG.TRANSPORT_EPS_SCALE * SPACING ** 2, TG.TRANSPORT_ITERS
    calls = (('kt_transport', lambda: eng.cloud_transport(p, q, eps=eps, iters=K, want_grad=True)),
             ('kd_sweeps + kd_combine', lambda: eng.cloud_divergence(p, q, eps=eps, iters=K, want_grad=True)))
    for _ in range(3):
        for _, call in calls:
            call()
    took = dict((name, []) for name, _ in calls)
    for _ in range(21):
        for name, call in calls:
            eng.probe_begin('loss')
            call()
            ms, launches = eng.probe_read()
            assert launches == 1
            took[name].append(ms)
    eng.probe_begin(None)
    self_err = float(eng.cloud_divergence(p, q, eps=eps, iters=K, want_self_err=True)['self_err'].max())
    eng.close()
    med = dict((name, float(np.median(took[name]))) for name in took)
    print('%d problems of %d x %d, K = %d: %s; the divergence = %.2f x kt_transport; self_err at most %.1e'
          % (PROBLEMS, n, m, K, ', '.join('%s %.4f ms (%.4f .. %.4f)' % (name, med[name], min(took[name]), max(took[name]))
                                          for name, _ in calls),
             med['kd_sweeps + kd_combine'] / med['kt_transport'], self_err), flush=True)


def divergence_f64_kernel_times(n, m):
    from dyn_res_pile_manip_amd import train_gnn_dyn as TG
    from dyn_res_pile_manip_amd.engine import Engine
    eng = Engine(0)
    p, q = clouds(n, m, 7 * n + m)
    p64 = p.astype(np.float64)
    eps, K = TG.TRANSPORT_EPS_SCALE * SPACING ** 2, TG.TRANSPORT_ITERS
    calls = (('kd_sweeps + kd_combine', lambda: eng.cloud_divergence(p, q, eps=eps, iters=K, want_grad=True)),
             ('kd64_sweeps + kd64_combine', lambda: eng.cloud_divergence_f64(p64, q, eps=eps, iters=K, want_grad=True)))
    for _ in range(3):
        for _, call in calls:
            call()
    took = dict((name, []) for name, _ in calls)
    for _ in range(21):
        for name, call in calls:
            eng.probe_begin('loss')
            call()
            ms, launches = eng.probe_read()
            assert launches == 1
            took[name].append(ms)
    eng.probe_begin(None)
    eng.close()
    med = dict((name, float(np.median(took[name]))) for name in took)
    print('%d problems of %d x %d, K = %d: %s; the float64 yardstick = %.2f x the fp32-cost kernels'
          % (PROBLEMS, n, m, K, ', '.join('%s %.4f ms (%.4f .. %.4f)' % (name, med[name], min(took[name]), max(took[name]))
                                          for name, _ in calls),
             med['kd64_sweeps + kd64_combine'] / med['kd_sweeps + kd_combine']), flush=True)


UNBALANCED_REACH_PER_EPS = 4.0      # a reach of two particle spacings


def unbalanced_kernel_times(n, m):
    from dyn_res_pile_manip_amd import train_gnn_dyn as TG
    from dyn_res_pile_manip_amd.engine import Engine
    eng = Engine(0)
    p, q = clouds(n, m, 7 * n + m)
    eps, K = TG.TRANSPORT_EPS_SCALE * SPACING ** 2, TG.TRANSPORT_ITERS
    rho = UNBALANCED_REACH_PER_EPS * eps
    calls = (('kd_sweeps + kd_combine', lambda: eng.cloud_divergence(p, q, eps=eps, iters=K, want_grad=True)),
             ('kd_sweeps_unbalanced + kd_combine', lambda: eng.cloud_divergence(p, q, eps=eps, iters=K, want_grad=True, reach=rho)))
    for _ in range(3):
        for _, call in calls:
            call()
    took = dict((name, []) for name, _ in calls)
    for _ in range(21):
        for name, call in calls:
            eng.probe_begin('loss')
            call()
            ms, launches = eng.probe_read()
            assert launches == 1
            took[name].append(ms)
    eng.probe_begin(None)
    moved = eng.cloud_divergence(p, q, eps=eps, iters=K, reach=rho, want_transported=True)['transported']
    eng.close()
    med = dict((name, float(np.median(took[name]))) for name in took)
    print('%d problems of %d x %d, K = %d, rho = %g eps: %s; unbalanced = %.3f x balanced; transported %.3f .. %.3f'
          % (PROBLEMS, n, m, K, UNBALANCED_REACH_PER_EPS,
             ', '.join('%s %.4f ms (%.4f .. %.4f)' % (name, med[name], min(took[name]), max(took[name])) for name, _ in calls),
             med['kd_sweeps_unbalanced + kd_combine'] / med['kd_sweeps + kd_combine'], moved.min(), moved.max()), flush=True)


def _engine():
    """Engine(0); a library from before an entry point existed (--ab's OLD) binds what it has"""
    import ctypes
    from dyn_res_pile_manip_amd import _lib
    have = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
        del _lib.SIGNATURES[name]
    from dyn_res_pile_manip_amd.engine import Engine
    return Engine(0)


def _timed(eng, calls, rounds=21, warm=3):
    for _ in range(warm):
        for _, call in calls:
            call()
    took = dict((name, []) for name, _ in calls)
    for _ in range(rounds):                                         # interleaved: every round times each form once
        for name, call in calls:
            eng.probe_begin('loss')
            call()
            ms, launches = eng.probe_read()
            assert launches == 1
            took[name].append(ms)
    eng.probe_begin(None)
    return took


def unbalanced_f64_kernel_times(n, m):
    from dyn_res_pile_manip_amd import train_gnn_dyn as TG
    eng = _engine()
    p, q = clouds(n, m, 7 * n + m)
    p64 = p.astype(np.float64)
    eps, K = TG.TRANSPORT_EPS_SCALE * SPACING ** 2, TG.TRANSPORT_ITERS
    rho = UNBALANCED_REACH_PER_EPS * eps
    calls = (('kd64_sweeps + kd64_combine', lambda: eng.cloud_divergence_f64(p64, q, eps=eps, iters=K, want_grad=True)),
             ('kd64_sweeps_unbalanced + kd64_combine_unbalanced',
              lambda: eng.cloud_divergence_f64(p64, q, eps=eps, iters=K, want_grad=True, reach=rho)))
    took = _timed(eng, calls)
    moved = eng.cloud_divergence_f64(p64, q, eps=eps, iters=K, reach=rho, want_transported=True)['transported']
    eng.close()
    med = dict((name, float(np.median(took[name]))) for name in took)
    print('%d problems of %d x %d, K = %d, rho = %g eps: %s; unbalanced = %.3f x balanced; transported %.3f .. %.3f'
          % (PROBLEMS, n, m, K, UNBALANCED_REACH_PER_EPS,
             ', '.join('%s %.4f ms (%.4f .. %.4f)' % (name, med[name], min(took[name]), max(took[name])) for name, _ in calls),
             med['kd64_sweeps_unbalanced + kd64_combine_unbalanced'] / med['kd64_sweeps + kd64_combine'], moved.min(), moved.max()),
          flush=True)


def balanced_f64_kernel_times(label):
    """the balanced kd64 pair alone, under whatever library DRP_LIB names: one round of --ab"""
    from dyn_res_pile_manip_amd import train_gnn_dyn as TG
    eng = _engine()
    eps, K = TG.TRANSPORT_EPS_SCALE * SPACING ** 2, TG.TRANSPORT_ITERS
    out = []
    for n in DIVERGENCE_SIZES:
        p, q = clouds(n, n, 7 * n + n)
        p64 = p.astype(np.float64)
        took = _timed(eng, (('kd64', lambda: eng.cloud_divergence_f64(p64, q, eps=eps, iters=K, want_grad=True)),))['kd64']
        out.append('%d x %d %.4f ms (%.4f .. %.4f)' % (n, n, float(np.median(took)), min(took), max(took)))
    eng.close()
    print('ab %s: kd64_sweeps + kd64_combine, %d problems, K = %d: %s' % (label, PROBLEMS, K, ', '.join(out)), flush=True)


def probe_times():
    """a whole Engine.train_gradient_probe call (the fp32 step in mode 'grad' and the float64 reverse pass) with and without a reach"""
    from dyn_res_pile_manip_amd import synthetic as syn, train_gnn_dyn as TG, weights
    from dyn_res_pile_manip_amd.engine import Engine
    eng = Engine(0)
    eng.load_weights(weights.blob_from_state_dict(weights.random_state_dict(0)), 0.08)
    rng = np.random.default_rng(0)
    B, H, N = 4, 5, 100
    states = np.zeros((B, H + 1, N, 3), np.float32)
    dens = np.zeros((B,), np.float32)
    for b in range(B):
        s, d, _ = syn.make_pile(N, 1, seed=b)
        dens[b] = d[0]
        for t in range(H + 1):
            states[b, t] = s[0] + 0.003 * t * rng.standard_normal((N, 3)).astype(np.float32)
    sdelta = (0.004 * rng.standard_normal((B, H, N, 3))).astype(np.float32)
    attrs = np.zeros((B, H + 1, N), np.float32)
    pn = np.full((B,), N, np.int32)
    targets = np.stack([np.stack([states[b, t + 1][rng.permutation(N)] for t in range(H)]) for b in range(B)])
    tn = np.full((B, H), N, np.int32)
    eps, K = TG.transport_eps(dens), TG.TRANSPORT_ITERS
    eng.train_begin(H, 1e-3, 0.9)
    kinds = {'sinkhorn': {}, 'sinkhorn, reach': {'reach': UNBALANCED_REACH_PER_EPS * eps}}

    def probe(k):
        return eng.train_gradient_probe(states, sdelta, attrs, pn, dens, targets=targets, target_nums=tn, eps=eps, iters=K, **kinds[k])
    for k in kinds:
        probe(k)
    took = dict((k, []) for k in kinds)
    for rep in range(6):                                            # interleaved blocks; the median of each
        for k in kinds:
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(3):
                pr = probe(k)
                assert np.isfinite(pr['rel']), (k, pr['rel'])
            eng.sync()
            took[k].append((time.perf_counter() - t0) / 3 * 1e3)
    last = probe('sinkhorn, reach')
    eng.close()
    med = dict((k, float(np.median(took[k]))) for k in kinds)
    print('probe at B=%d n_rollout=%d N=M=%d, K = %d: %s; a probe with a reach costs %.3f balanced ones; worst rel %.2e, transported '
          '%.3f, transported_diff %.1e' % (B, H, N, K, ', '.join("'%s' %.3f ms (blocks %.3f .. %.3f)" % (k, med[k], min(took[k]), max(took[k]))
                                                                 for k in kinds),
                                           med['sinkhorn, reach'] / med['sinkhorn'], last['rel'], last['transported'],
                                           last['transported_diff']), flush=True)


def update_times(kinds=('chamfer', 'match', 'transport')):
    from dyn_res_pile_manip_amd import synthetic as syn, train_gnn_dyn as TG, weights
    from dyn_res_pile_manip_amd.engine import Engine
    eng = Engine(0)
    eng.load_weights(weights.blob_from_state_dict(weights.random_state_dict(0)), 0.08)
    rng = np.random.default_rng(0)
    B, H, N = 4, 5, 100
    states = np.zeros((B, H + 1, N, 3), np.float32)
    dens = np.zeros((B,), np.float32)
    for b in range(B):
        s, d, _ = syn.make_pile(N, 1, seed=b)
        dens[b] = d[0]
        for t in range(H + 1):
            states[b, t] = s[0] + 0.003 * t * rng.standard_normal((N, 3)).astype(np.float32)
    sdelta = (0.004 * rng.standard_normal((B, H, N, 3))).astype(np.float32)
    attrs = np.zeros((B, H + 1, N), np.float32)
    pn = np.full((B,), N, np.int32)
    targets = np.stack([np.stack([states[b, t + 1][rng.permutation(N)] for t in range(H)]) for b in range(B)])
    tn = np.full((B, H), N, np.int32)
    eps, K = TG.transport_eps(dens), TG.TRANSPORT_ITERS
    eng.train_begin(H, 1e-3, 0.9)

    def step(k):
        if k == 'transport':
            return eng.train_step_transport(states, attrs, pn, dens, targets, tn, eps, K, states_delta=sdelta, mode='update')
        if k == 'sinkhorn':
            return eng.train_step_divergence(states, attrs, pn, dens, targets, tn, eps, K, states_delta=sdelta, mode='update')
        if k == 'sinkhorn, reach':
            return eng.train_step_divergence(states, attrs, pn, dens, targets, tn, eps, K, states_delta=sdelta, mode='update',
                                             reach=UNBALANCED_REACH_PER_EPS * eps)
        return eng.train_step_loss(states, attrs, pn, dens, targets, tn, states_delta=sdelta, loss=k, mode='update')
    for k in kinds:
        step(k), step(k)
    took = dict((k, []) for k in kinds)
    for rep in range(6):                                            # interleaved blocks; the median of each
        for k in kinds:
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(10):
                loss, _ = step(k)
                assert np.isfinite(loss), (k, loss)
            eng.sync()
            took[k].append((time.perf_counter() - t0) / 10 * 1e3)
    eng.close()
    med = dict((k, float(np.median(took[k]))) for k in kinds)
    print('update at B=%d n_rollout=%d N=M=%d, K = %d: %s' % (B, H, N, K, ', '.join("'%s' %.3f ms (blocks %.3f .. %.3f)"
          % (k, med[k], min(took[k]), max(took[k])) for k in kinds)), flush=True)
    if 'sinkhorn, reach' in kinds:
        print("a 'sinkhorn' update with a reach costs %.3f balanced ones" % (med['sinkhorn, reach'] / med['sinkhorn'],), flush=True)
    elif 'sinkhorn' in kinds:
        print("a 'sinkhorn' update costs %.2f 'transport' updates" % (med['sinkhorn'] / med['transport'],), flush=True)
    else:
        print("a 'transport' update costs %.2f 'chamfer' updates and %.2f 'match' updates"
              % (med['transport'] / med['chamfer'], med['transport'] / med['match']), flush=True)


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--kernel':
        kernel_times(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == '--update':
        update_times()
    elif len(sys.argv) > 1 and sys.argv[1] == '--divergence-kernel':
        divergence_kernel_times(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == '--divergence-update':
        update_times(('transport', 'sinkhorn'))
    elif len(sys.argv) > 1 and sys.argv[1] == '--divergence-f64-kernel':
        divergence_f64_kernel_times(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == '--unbalanced-kernel':
        unbalanced_kernel_times(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == '--unbalanced-update':
        update_times(('sinkhorn', 'sinkhorn, reach'))
    elif len(sys.argv) > 1 and sys.argv[1] == '--unbalanced-f64-kernel':
        unbalanced_f64_kernel_times(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == '--unbalanced-f64-probe':
        probe_times()
    elif len(sys.argv) > 1 and sys.argv[1] == '--balanced-f64-kernel':
        balanced_f64_kernel_times(sys.argv[2])
    else:
        divergence = len(sys.argv) > 1 and sys.argv[1] == '--divergence'
        f64 = len(sys.argv) > 1 and sys.argv[1] == '--divergence-f64'
        unbalanced = len(sys.argv) > 1 and sys.argv[1] == '--unbalanced'
        rest = sys.argv[2:] if divergence or f64 or unbalanced else sys.argv[1:]
        unbalanced_f64 = unbalanced and rest[:1] == ['--f64']
        ab = []
        if unbalanced_f64:
            unbalanced, rest = False, rest[1:]
            if '--ab' in rest:
                ab, rest = rest[rest.index('--ab') + 1:], rest[:rest.index('--ab')]
                assert len(ab) == 2, '--ab OLD.so NEW.so'
        out = rest[0] if rest else ('profiles/divergence_unbalanced_f64_timing.txt' if unbalanced_f64 else 'profiles/divergence_timing.txt' if divergence else
                                    'profiles/divergence_f64_timing.txt' if f64 else
                                    'profiles/divergence_unbalanced_timing.txt' if unbalanced else 'profiles/transport_timing.txt')
        lines = ['tools/transport_timing.py: device time of the loss kernels by HIP events (median of 21 interleaved launches, min ..',
                 'max), and host time of whole update steps (median of 6 interleaved blocks of 10); one MI355X', '']
        jobs = [['--kernel', str(n), str(m)] for n, m in SIZES] + [['--update']]
        if divergence:
            lines[0] = lines[0].replace('tools/transport_timing.py:', 'tools/transport_timing.py --divergence:')
            jobs = [['--divergence-kernel', str(n), str(n)] for n in DIVERGENCE_SIZES] + [['--divergence-update']]
        if f64:
            lines[0] = lines[0].replace('tools/transport_timing.py:', 'tools/transport_timing.py --divergence-f64:')
            jobs = [['--divergence-f64-kernel', str(n), str(n)] for n in DIVERGENCE_SIZES]
        if unbalanced:
            lines[0] = lines[0].replace('tools/transport_timing.py:', 'tools/transport_timing.py --unbalanced:')
            jobs = [['--unbalanced-kernel', str(n), str(n)] for n in DIVERGENCE_SIZES] + [['--unbalanced-update']]
        if unbalanced_f64:
            lines[0] = lines[0].replace('tools/transport_timing.py:', 'tools/transport_timing.py --unbalanced --f64:')
            lines[1] = lines[1].replace('whole update steps (median of 6 interleaved blocks of 10)',
                                        'whole probe calls (median of 6 interleaved blocks of 3)')
            jobs = [['--unbalanced-f64-kernel', str(n), str(n)] for n in DIVERGENCE_SIZES] + [['--unbalanced-f64-probe']]
            jobs += [['--balanced-f64-kernel', '%s round %d' % (('OLD', 'NEW')[k], rnd), os.path.abspath(ab[k])]
                     for rnd in range(3) for k in range(len(ab))]
        for job in jobs:
            env = None
            if job[0] == '--balanced-f64-kernel':
                env, job = dict(os.environ, DRP_LIB=job[2]), job[:2]
            r = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT_S), sys.executable, __file__] + job, stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, universal_newlines=True, env=env)
            print(r.stdout, end='', flush=True)
            if r.returncode != 0:
                raise SystemExit('step %s ended with status %d: nothing further is started' % (job, r.returncode))
            lines += [ln for ln in r.stdout.splitlines() if 'problems of' in ln or 'update' in ln or ln.startswith(('probe at', 'ab '))]
        if ab:
            import re
            for size in DIVERGENCE_SIZES:
                pat = re.compile(r'ab (OLD|NEW) round \d.*?%d x %d ([0-9.]+) ms' % (size, size))
                got = {'OLD': [], 'NEW': []}
                for m in filter(None, map(pat.search, lines)):
                    got[m.group(1)].append(float(m.group(2)))
                old, new = float(np.median(got['OLD'])), float(np.median(got['NEW']))
                lines.append('kd64_sweeps + kd64_combine at %d x %d: OLD %s ms (median %.4f, spread of its own rounds %.2f %%), NEW %s ms '
                             '(median %.4f): NEW = %.4f x OLD' % (size, size, ' '.join('%.4f' % v for v in got['OLD']), old,
                                                                  100.0 * (max(got['OLD']) - min(got['OLD'])) / old,
                                                                  ' '.join('%.4f' % v for v in got['NEW']), new, new / old))
        if unbalanced:
            # the balanced kernels in this run against the figures profiles/divergence_timing.txt recorded for them: a templating
            # that leaked into the balanced path shows here
            import re
            pat = re.compile(r'(\d+ x \d+), K = \d+.*?kd_sweeps \+ kd_combine ([0-9.]+) ms')
            now = dict(m.groups() for m in map(pat.search, lines) if m)
            with open('profiles/divergence_timing.txt') as f:
                then = dict(m.groups() for m in map(pat.search, f) if m)
            lines.append('kd_sweeps + kd_combine in this run against profiles/divergence_timing.txt: ' + ', '.join(
                '%s %s against %s ms (%.3f x)' % (k, now[k], then[k], float(now[k]) / float(then[k])) for k in now if k in then))
        with open(out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
