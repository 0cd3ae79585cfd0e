"""`fused` against `lite` (include/drp.h: DRP_ENGINE_LITE) on ONE context, interleaved: 1024 samples x {20, 50, 300} particles x
10 steps, the whole MPPI iteration (sample, rollout, reward, device update) and the propagation launches alone (the `prop`
probe), then one counted iteration per engine (`prop+work`: executed MFMAs and the clock under load), then the planner-level
effect of one iteration from the same seed on the trained weights.  Run it on one box and keep the output:

    python tools/lite_timing.py | tee profiles/lite_timing.txt
"""
import sys
import time

sys.path.insert(0, '.')
import numpy as np

from dyn_res_pile_manip_amd import synthetic as syn, weights, _lib
from dyn_res_pile_manip_amd.engine import Engine
from dyn_res_pile_manip_amd.planners import world2cam_affine

NS, H, ROUNDS, ITERS, WARM = 1024, 10, 5, 10, 3
ENGINES = ('fused', 'lite')


def session(eng, N, seed=1234):
    s0, dens, attr = syn.make_pile(N, 1, seed=0)
    lo, hi = syn.action_limits()
    eng.set_goal_image(syn.goal_distance_image(syn.goal_mask('I')), 5 * N, fps_init=0, mode='cv5')
    eng.mpc_begin(s0, attr, dens, syn.nominal_pushes(H, seed=0), n_sample=NS, sigma=0.3 * 24 / 12.0, beta_filter=0.7,
                  reward_weight=0.1, act_lo=lo, act_hi=hi, seed=seed)


def iteration(eng, it, update=True):
    eng.mpc_sample(it)
    eng.mpc_rollout(False)
    if update:
        eng.mpc_update_device()


def timing(eng, N):
    ms = {e: [] for e in ENGINES}
    prop = {e: [0.0, 0] for e in ENGINES}
    for e in ENGINES:                                   # warm both up on this shape
        eng.set_engine(e)
        session(eng, N)
        for it in range(WARM):
            iteration(eng, it)
    eng.sync()
    for r in range(ROUNDS):
        for e in (ENGINES if r % 2 == 0 else ENGINES[::-1]):          # interleaved, the order alternating
            eng.set_engine(e)
            session(eng, N)
            iteration(eng, 0)
            eng.sync()
            eng.probe_begin('prop')
            t0 = time.perf_counter()
            for it in range(1, 1 + ITERS):
                iteration(eng, it)
            eng.sync()
            ms[e].append((time.perf_counter() - t0) / ITERS * 1e3)
            p_ms, p_n = eng.probe_read()
            eng.probe_begin(None)
            prop[e][0] += p_ms
            prop[e][1] += p_n
    work = {}
    for e in ENGINES:
        eng.set_engine(e)
        session(eng, N)
        iteration(eng, 0)
        eng.probe_begin('prop+work')
        eng.dispatch_reset()
        iteration(eng, 1)
        eng.sync()
        work[e] = eng.probe_work()
        work[e]['ran'] = [n.replace(',work', '') for n in eng.last_dispatch() if n.startswith('km_')]   # (the counting twins of what was timed)
        eng.probe_begin(None)
    print('shape %d x %d x %d' % (NS, N, H))
    for e in ENGINES:
        w = work[e]
        print('  %-5s ms per MPPI iteration: median %.4f  min %.4f  max %.4f (rounds of %d iterations: %s)'
              % (e, np.median(ms[e]), min(ms[e]), max(ms[e]), ITERS, ' '.join('%.4f' % v for v in ms[e])))
        print('  %-5s average propagation launch %.4f ms over %d launches: %s' % (e, prop[e][0] / max(prop[e][1], 1), prop[e][1], ' | '.join(w['ran'])))
        print('  %-5s counted iteration: chain slots %d, cached slots %d, tiles %d + %d last, encoder tiles %d, executed MFMAs %d, '
              'sclk_mhz_under_load %.0f' % (e, w['chain_slots'], w['cached_slots'], w['tiles'], w['tiles_last'], w['encoder_tiles'],
                                            w['mfmas'], 100.0 * w['clk_cycles'] / max(w['clk_ticks'], 1)))
    f, l = np.median(ms['fused']), np.median(ms['lite'])
    print('  lite / fused: iteration %.3f, propagation launch %.3f, executed MFMAs %.3f'
          % (l / f, (prop['lite'][0] / max(prop['lite'][1], 1)) / (prop['fused'][0] / max(prop['fused'][1], 1)),
             work['lite']['mfmas'] / max(work['fused']['mfmas'], 1)))


def planner_effect(eng, N):
    """one 1024-row MPPI iteration from the same seed on either engine: what the planner sees of the difference"""
    got = {}
    for e in ENGINES:
        eng.set_engine(e)
        session(eng, N, seed=99)
        iteration(eng, 0)
        r = eng.mpc_get(rewards=True, nominal=True)
        got[e] = (np.asarray(r['rewards'], np.float64).reshape(NS, -1)[:, -1], np.asarray(r['nominal'], np.float64))
    (rf, nf), (rl, nl) = got['fused'], got['lite']
    dr = np.abs(rl - rf)
    spread = rf.max() - rf.min()
    print('planner %d x %d x %d, trained weights, seed 99: update difference max %.3e (largest |nominal| %.3f), arg-max row fused %d lite %d, '
          'reward difference 50 / 90 / 99 %%: %.3e / %.3e / %.3e (reward spread over the rows %.3e)'
          % (NS, N, H, np.abs(nl - nf).max(), np.abs(nf).max(), int(rf.argmax()), int(rl.argmax()),
             np.percentile(dr, 50), np.percentile(dr, 90), np.percentile(dr, 99), spread))


def main():
    eng = Engine(0)
    eng.set_camera(world2cam_affine(syn.demo_cam_extrinsics()), 24.0, syn.demo_cam_params())
    print('device', eng.device_info())
    eng.load_weights(weights.blob_from_state_dict(weights.random_state_dict(seed=0)), 0.08)
    for N in (20, 50, 300):
        timing(eng, N)
    eng.load_weights(weights.blob_from_state_dict(np.load('tests/golden/weights_trained.npz')), 0.08)
    batch = eng.probe_batch()
    for e in ENGINES:
        p = eng.accuracy_probe(*batch, engine=_lib.ENGINES[e])
        print('probe, trained weights, %-5s: max |err| %.3e, %.3e of the largest displacement' % (e, p['abs'], p['disp_rel']))
    for N in (20, 50, 300):
        planner_effect(eng, N)
    eng.close()


if __name__ == '__main__':
    main()
