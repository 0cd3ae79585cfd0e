"""Time the one-to-one matching loss (csrc/k_match.h) next to the Chamfer loss it stands beside -> profiles/match_timing.txt.

  python tools/match_timing.py [output file]

(a) device time of ka_match for B x H = 20 problems in one launch at n = m in {20, 50, 100, 300} and at 100 x 130, and of kc_chamfer
    on the same clouds: HIP events around the kernel (drp_probe_begin("loss")), the median of 21 launches after 3 warm-up ones;
(b) a whole mode='update' step at 4 x 5 x 100 (B x n_rollout x N = M) under 'chamfer', 'match' and 'chamfer+match', interleaved
    on one context: host time of the call (it returns when the step is complete on the device), the median of 6 blocks of 10
    after warm-up, as tools/train_timing.py measures its steps.
Each measurement runs in a child process of its own under a time limit (a stuck step ends there, and nothing follows it).

  python tools/match_timing.py --f64 [output file]  -> profiles/match_f64_timing.txt

(c) the float64 yardstick's kernel (csrc/k_match_f64.h: ka64_match) beside ka_match on the same clouds, p widened exactly, at (a)'s
    sizes: the same events and counts, the two kernels' launches interleaved.  A yardstick's cost: recorded, no condition."""
import subprocess
import sys
import time

sys.path.insert(0, '.')
import numpy as np

SIZES = ((20, 20), (50, 50), (100, 100), (300, 300), (100, 130))
PROBLEMS = 20
STEP_LIMIT_S = 120


def clouds(n, m, seed):
    rng = np.random.default_rng(seed)
    side = 0.02 * max(n, m) ** (1.0 / 3.0)                          # the piles' scale: spacing about 0.02
    p = (0.2 + side * rng.random((PROBLEMS, n, 3))).astype(np.float32)
    q = (0.2 + side * rng.random((PROBLEMS, m, 3))).astype(np.float32)
    return p, q


def kernel_times(n, m):
    from dyn_res_pile_manip_amd.engine import Engine
    eng = Engine(0)
    p, q = clouds(n, m, 7 * n + m)
    out = {}
    for name, call in (('ka_match', lambda: eng.cloud_match(p, q, want_grad=True)),
                       ('kc_chamfer', lambda: eng.cloud_chamfer(p, q, want_grad=True))):
        for _ in range(3):
            call()
        took = []
        for _ in range(21):
            eng.probe_begin('loss')
            call()
            ms, launches = eng.probe_read()
            assert launches == 1
            took.append(ms)
        eng.probe_begin(None)
        out[name] = (float(np.median(took)), min(took), max(took))
    eng.close()
    print('%d problems of %d x %d: ka_match %.4f ms (%.4f .. %.4f), kc_chamfer %.4f ms (%.4f .. %.4f): %.1f x'
          % ((PROBLEMS, n, m) + out['ka_match'] + out['kc_chamfer'] + (out['ka_match'][0] / out['kc_chamfer'][0],)), flush=True)


def f64_kernel_times(n, m):
    from dyn_res_pile_manip_amd.engine import Engine
    eng = Engine(0)
    p, q = clouds(n, m, 7 * n + m)
    p64 = p.astype(np.float64)                                      # widened exactly: the two kernels solve the same clouds
    calls = (('ka_match', lambda: eng.cloud_match(p, q, want_grad=True)),
             ('ka64_match', lambda: eng.cloud_match_f64(p64, q, want_grad=True)))
    for _, call in calls:
        for _ in range(3):
            call()
    took = dict((name, []) for name, _ in calls)
    for _ in range(21):                                             # interleaved
        for name, call in calls:
            eng.probe_begin('loss')
            call()
            ms, launches = eng.probe_read()
            assert launches == 1
            took[name].append(ms)
    eng.probe_begin(None)
    eng.close()
    out = dict((k, (float(np.median(v)), min(v), max(v))) for k, v in took.items())
    print('%d problems of %d x %d: ka64_match %.4f ms (%.4f .. %.4f), ka_match %.4f ms (%.4f .. %.4f): %.2f x'
          % ((PROBLEMS, n, m) + out['ka64_match'] + out['ka_match'] + (out['ka64_match'][0] / out['ka_match'][0],)), flush=True)


def update_times():
    from dyn_res_pile_manip_amd import synthetic as syn, weights
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
    eng.train_begin(H, 1e-3, 0.9)
    kinds = ('chamfer', 'match', 'chamfer+match')
    step = lambda k: eng.train_step_loss(states, attrs, pn, dens, targets, tn, states_delta=sdelta, loss=k, mode='update')
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
    print('update at B=%d n_rollout=%d N=M=%d: %s' % (B, H, N, ', '.join("'%s' %.3f ms (blocks %.3f .. %.3f)"
          % (k, med[k], min(took[k]), max(took[k])) for k in kinds)), flush=True)
    print("a 'match' update costs %.2f 'chamfer' updates, a 'chamfer+match' update %.2f"
          % (med['match'] / med['chamfer'], med['chamfer+match'] / med['chamfer']), flush=True)


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--kernel':
        kernel_times(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == '--f64-kernel':
        f64_kernel_times(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == '--update':
        update_times()
    else:
        f64 = len(sys.argv) > 1 and sys.argv[1] == '--f64'
        rest = sys.argv[2:] if f64 else sys.argv[1:]
        out = rest[0] if rest else ('profiles/match_f64_timing.txt' if f64 else 'profiles/match_timing.txt')
        if f64:
            lines = ['tools/match_timing.py --f64: device time of the float64 assignment kernel beside the fp32 one on the same clouds, by',
                     'HIP events (median of 21 interleaved launches, min .. max); one MI355X', '']
            jobs = [['--f64-kernel', str(n), str(m)] for n, m in SIZES]
        else:
            lines = ['tools/match_timing.py: device time of the loss kernels by HIP events (median of 21 launches, min .. max), and host',
                     'time of whole update steps (median of 6 interleaved blocks of 10); one MI355X', '']
            jobs = [['--kernel', str(n), str(m)] for n, m in SIZES] + [['--update']]
        for job in jobs:
            r = subprocess.run(['timeout', '-k', '10', str(STEP_LIMIT_S), sys.executable, __file__] + job, stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, universal_newlines=True)
            print(r.stdout, end='', flush=True)
            if r.returncode != 0:
                raise SystemExit('step %s ended with status %d: nothing further is started' % (job, r.returncode))
            lines += [ln for ln in r.stdout.splitlines() if 'problems of' in ln or 'update' in ln]
        with open(out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
