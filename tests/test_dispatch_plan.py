"""CPU: csrc/dispatch.h is pure host code.  tests/dispatch_dump.cpp is compiled against it with the host compiler alone
(-Wall -Werror, no HIP header in reach) and asked what the library would launch: the same names as the built library reported on
a GPU (tests/dispatch_table.txt), the pairing rule on both sides of its threshold, the sharding contract of the edge-chain cache
(DESIGN.md 9), the tape's launches cut into blocks and the cache-size fallback, the environment table field by field, and
DESIGN_NOTES.md 9c's list of switches."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, 'tests', 'dispatch_table.txt')
# switches of DESIGN_NOTES.md 9c that are not the dispatch's (read in drp_create / _lib.py / the RCCL binding)
NOT_DISPATCH = {'DRP_NO_REPACK_DEVICE', 'DRP_NO_WGRAD_DEFER', 'DRP_COMM_ALWAYS', 'DRP_COMM_TIMEOUT_S', 'DRP_COMM_INIT_TIMEOUT_S',
                'DRP_RCCL_LIB', 'DRP_LIB'}
DEFAULTS = dict(agg_global_only=0, rev_global_only=0, self_const=1, prop3=1, prop3_min_b=0, prop3_min_tiles=1, bwd_fused_min_tiles=1,
                graph_cells=1, graph_cells_min_n=400, graph_cells_halo=0, graph_cells_hb=0, graph_strips=1, bwd_fused=1, graph_rev=1,
                graph_encode=1, train_fused=-1, train_coop=-1, train_parts=0, bwd_rows=1, prop3_order=1, prop_pair_rows=128,
                prop_pair_always=64, prop_pair_deg10=83, prop3e=1, rollout_fused=1, rollout_max_n=64, rollout_mid_n=256,
                rollout_mid_rows=256, rollout_max_rows=704, ecache_max_mb=192, ecache_hard_max_mb=4096, ecache_max_n=128,
                ecache_full_n=225, ecache_tape_max_n=40, graph_q4=1, wgrad_mfma=1, prop_spread=1)
# switch -> (value, the fields it changes): its documented effect (DESIGN_NOTES.md 9c, csrc/dispatch.h)
EFFECTS = {
    'DRP_NO_SELF_CONST': ('1', dict(self_const=0)), 'DRP_NO_PROP3': ('1', dict(prop3=0)), 'DRP_NO_GRAPH_STRIPS': ('1', dict(graph_strips=0)),
    'DRP_NO_GRAPH_CELLS': ('1', dict(graph_cells=0)), 'DRP_GRAPH_CELLS_MIN_N': ('300', dict(graph_cells_min_n=300)),
    'DRP_GRAPH_CELLS_HB': ('0.5', dict(graph_cells_hb=0.5)), 'DRP_GRAPH_CELLS_HALO': ('0.25', dict(graph_cells_halo=0.25)),
    'DRP_NO_ROLLOUT_FUSED': ('1', dict(rollout_fused=0)), 'DRP_NO_PROP_SPREAD': ('1', dict(prop_spread=0)),
    'DRP_NO_WGRAD_MFMA': ('1', dict(wgrad_mfma=0)), 'DRP_GRAPH_Q4': ('2', dict(graph_q4=2)),
    'DRP_ROLLOUT_MAX_N': ('100', dict(rollout_max_n=100, rollout_mid_n=0, rollout_max_rows=3072)),
    'DRP_PROP_PAIR_ROWS': ('1000', dict(prop_pair_rows=256)), 'DRP_PROP_PAIR_ALWAYS': ('-5', dict(prop_pair_always=0)),
    'DRP_PROP_PAIR_DEG10': ('-1', dict(prop_pair_deg10=0)), 'DRP_NO_BWD_FUSED': ('1', dict(bwd_fused=0)),
    'DRP_NO_BWD_ROWS': ('1', dict(bwd_rows=0)), 'DRP_TRAIN_PARTS': ('3', dict(train_parts=3)), 'DRP_TRAIN_COOP': ('0', dict(train_coop=0)),
    'DRP_NO_GRAPH_ENCODE': ('1', dict(graph_encode=0)), 'DRP_TRAIN_FUSED': ('1', dict(train_fused=1)),
    'DRP_NO_GRAPH_REV': ('1', dict(graph_rev=0)), 'DRP_REV_GLOBAL': ('1', dict(rev_global_only=1)),
    'DRP_ECACHE_MAX_MB': ('-3', dict(ecache_max_mb=0)), 'DRP_ECACHE_MAX_N': ('64', dict(ecache_max_n=64, ecache_full_n=257)),
    'DRP_ECACHE_TAPE_MAX_N': ('50', dict(ecache_tape_max_n=50)), 'DRP_ECACHE_HARD_MAX_MB': ('-2', dict(ecache_hard_max_mb=0)),
}


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('dispatch') / 'dispatch_dump')
    # an empty include directory first in line is not needed: the driver includes nothing of HIP, and -Werror keeps it honest
    subprocess.check_call([cxx, '-std=c++17', '-Wall', '-Werror', '-O1', '-o', exe, os.path.join(ROOT, 'tests', 'dispatch_dump.cpp')])

    def run(*args, env=None):
        e = {k: v for k, v in os.environ.items() if not k.startswith('DRP_')}
        e.update(env or {})
        return subprocess.check_output([exe] + [str(a) for a in args], env=e).decode().splitlines()
    return run


def test_the_header_compiles_on_its_own_with_the_host_compiler():
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    subprocess.check_call([cxx, '-std=c++17', '-Wall', '-Werror', '-fsyntax-only', '-x', 'c++',
                           os.path.join(ROOT, 'dyn_res_pile_manip_amd', 'csrc', 'dispatch.h')])
    text = open(os.path.join(ROOT, 'dyn_res_pile_manip_amd', 'csrc', 'dispatch.h')).read()
    assert not re.search(r'#include\s*[<"](hip|rccl)', text)


def test_the_plans_name_what_the_library_launched(dump):
    lines = open(TABLE).read().splitlines()
    n_cu = int(re.search(r'n_cu (\d+)', lines[0]).group(1))
    want = [l for l in lines[1:] if l.split()[1] in ('step', 'rollout', 'mppi', 'gd')]
    assert len(want) > 250 and {l.split()[1] for l in want} == {'step', 'rollout', 'mppi', 'gd'}
    got = dump('table', TABLE, n_cu)
    assert len(got) == len(want)
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, 'first of %d: recorded %r, planned %r' % (len(bad), bad[0][0], bad[0][1])


def test_pairing_on_both_sides_of_the_in_degree_threshold(dump):
    # one sample of 100 particles per workgroup (65 ... 128 rows: the in-degree decides), a batch of 256: 25 600 rows in the statistic
    rows = 25600
    assert dump('pair', 1, 100, 256) == ['1']                                   # unknown: paired
    assert dump('pair', 1, 100, 256, rows * 83 // 10, rows, 100) == ['1']       # mean in-degree 8.3: at the bound
    assert dump('pair', 1, 100, 256, rows * 83 // 10 + 1, rows, 100) == ['0']   # just above
    assert dump('pair', 1, 100, 256, rows * 10, rows, 96) == ['1']              # stale: another pile size
    assert dump('pair', 1, 100, 256, rows * 10, rows - 100, 100) == ['1']       # stale: another batch
    assert dump('pair', 1, 100, 256, 0, 0, 100) == ['1']                        # no rows counted
    assert dump('pair', 1, 64, 256, rows * 10, 64 * 256, 64) == ['1']           # up to 64 rows: always
    assert dump('pair', 1, 129, 256, 0, 65536, 129) == ['0']                    # above 128 rows: never
    assert dump('pair', 1, 100, 256, rows * 5, rows, 100, env={'DRP_PROP_PAIR_DEG10': '40'}) == ['0']


def test_the_cache_decision_is_a_function_of_the_pile_size_alone(dump):
    """a B / 8 shard, the batch and twice the batch of one pile size get the same kind of kernel (cached or not)."""
    seen = {}
    for line in dump('cache', 256):
        N, B, nb, step, roll = map(int, line.split())
        for kind, v in (('step', step), ('rollout', roll)):
            if v >= 0:
                seen.setdefault((N, kind), set()).add(v)
    assert {N for N, _ in seen} == set(range(1, 301))
    assert all(len(v) == 1 for v in seen.values()), sorted(k for k, v in seen.items() if len(v) != 1)[:5]
    # a one-launch rollout and a step-by-step one agree too, and the bands are the documented ones
    for N in range(1, 301):
        kinds = set().union(*(seen.get((N, k), set()) for k in ('step', 'rollout')))
        assert kinds == {1 if (N <= 128 or 225 <= N <= 256) else 0}, N


def blocks_of(dump, B, N, nb, H, tape=1, env=None):
    """the 'blocks' mode, parsed: per rollout step (prop3, cache, n, chunk, cache_bytes, [block dicts])"""
    steps = []
    for line in dump('blocks', 256, B, N, nb, H, tape, env=env):
        f = line.split()
        if f[0] == 'step':
            steps.append(dict(prop3=int(f[2]), cache=int(f[3]), n=int(f[4]), chunk=int(f[5]), cache_bytes=int(f[6]), blocks=[]))
        else:
            names = ('q', 'b_off', 'Bc', 'spw', 'grid', 'pair', 'cache', 'ec_stride', 'cache_bytes')
            steps[-1]['blocks'].append(dict(zip(names, map(int, f[1:]))))
    assert len(steps) == H and all(len(s['blocks']) == s['n'] for s in steps)
    return steps


def test_the_tape_is_cut_into_blocks_and_falls_back_by_the_cache_size(dump):
    """The tape's launches (gradient-descent planner, trainer) at 256 CUs: 40 particles are 7 samples = 280 rows per workgroup,
    1792 samples per launch (1770 in whole multiples of 30 batch columns).  Both rollout steps of a call are cut alike: the first
    reads the start state by batch column, the others a state per sample."""
    tile_bytes = 10 * 512 * 16                                      # K x EC_UNITS float4 per unpaired tile of 32 receivers
    for nb, chunk, grid0, tail in ((1, 1792, 256, 8), (30, 1770, 253, 30)):
        steps = blocks_of(dump, 1800, 40, nb, 2)
        assert steps[0] == steps[1]
        s = steps[0]
        assert (s['prop3'], s['cache'], s['n'], s['chunk']) == (1, 1, 2, chunk) and chunk % nb == 0
        first, second = s['blocks']
        assert first == dict(q=0, b_off=0, Bc=chunk, spw=7, grid=grid0, pair=0, cache=1, ec_stride=9 * 10 * 512,
                             cache_bytes=grid0 * 9 * tile_bytes)
        # the tail: a sample per workgroup, 40 rows as three paired tiles of 16 (5 x 512 float4 each), rows kept in registers
        assert second == dict(q=1, b_off=chunk, Bc=tail, spw=1, grid=tail, pair=1, cache=2, ec_stride=3 * 5 * 512,
                              cache_bytes=tail * 3 * 5 * 512 * 16)
        assert s['cache_bytes'] == first['cache_bytes'] >= second['cache_bytes']          # the buffer is the first block's
    # two equal blocks; one launch at exactly a block; 41 particles are never cached on the tape
    s = blocks_of(dump, 3584, 40, 1, 2)[1]
    assert s['n'] == 2 and s['blocks'][1] == dict(s['blocks'][0], q=1, b_off=1792)
    s = blocks_of(dump, 1792, 40, 1, 2)[0]
    assert (s['cache'], s['n'], s['chunk'], s['blocks'][0]['Bc'], s['blocks'][0]['cache']) == (1, 1, 1792, 1792, 1)
    for B in (8, 1800, 8192):
        s = blocks_of(dump, B, 41, 1, 1)[0]
        assert (s['prop3'], s['cache'], s['n'], s['chunk'], s['cache_bytes']) == (1, 0, 1, B, 0) and s['blocks'][0]['cache'] == 0
    # the fallback: the first launch's 178 MB are above 1 MB, the whole batch recomputes in one launch
    for nb in (1, 30):
        for s in blocks_of(dump, 1800, 40, nb, 2, env={'DRP_ECACHE_HARD_MAX_MB': '1'}):
            assert (s['prop3'], s['cache'], s['n'], s['chunk'], s['cache_bytes']) == (1, 0, 1, 1800, 0)
            assert s['blocks'] == [dict(q=0, b_off=0, Bc=1800, spw=8, grid=225, pair=0, cache=0, ec_stride=s['blocks'][0]['ec_stride'],
                                        cache_bytes=0)]
    # ... and a limit the first launch fits under changes nothing
    assert blocks_of(dump, 1800, 40, 30, 2, env={'DRP_ECACHE_HARD_MAX_MB': '178'}) == blocks_of(dump, 1800, 40, 30, 2)
    assert blocks_of(dump, 1800, 40, 30, 2, env={'DRP_ECACHE_HARD_MAX_MB': '177'})[0]['cache'] == 0
    # the forward launches of the same shape are cut the same way (held on a GPU by test_edge_cache_against_the_oracle)
    assert [b['Bc'] for b in blocks_of(dump, 1800, 40, 30, 1, tape=0)[0]['blocks']] == [1770, 30]


def test_the_environment_table_field_by_field(dump):
    def policy(env=None):
        return {k: float(v) for k, v in (l.split('=') for l in dump('policy', env=env))}
    assert policy() == {k: float(v) for k, v in DEFAULTS.items()}
    names = dump('env')
    assert sorted(names) == sorted(EFFECTS) and len(set(names)) == len(names)
    for name, (value, effect) in EFFECTS.items():
        want = dict(DEFAULTS, **effect)
        assert policy({name: value}) == {k: float(v) for k, v in want.items()}, name


def test_the_documented_switches_are_the_tables(dump):
    text = open(os.path.join(ROOT, 'DESIGN_NOTES.md')).read()
    sec = text[text.index('### 9c.'):]
    sec = sec[:sec.index('\n### ', 5)]
    rows = [l for l in sec.splitlines() if l.startswith('| `DRP_')]
    doc = set()
    for r in rows:
        doc |= set(re.findall(r'DRP_[A-Z0-9_]+', r.split('|')[1]))
    assert doc - NOT_DISPATCH == set(dump('env'))
    assert NOT_DISPATCH <= doc


def wgrad_grid():
    """(blocks, target id) per job: 25 jobs per rollout step is what the trainer queues; block counts all equal, strictly
    decreasing and with ties (the stable order must show); targets all distinct, all equal and interleaved (queue order within a
    target must show)"""
    for n in (1, 2, 24, 25, 75):
        for blocks in ([7] * n, [n + 3 - q for q in range(n)], [(3, 16, 3, 1, 16)[q % 5] for q in range(n)]):
            for targets in ([100 + q for q in range(n)], [5] * n, [(9, 4, 9, 2)[q % 4] + 10 * (q % 25 // 12) for q in range(n)]):
                yield list(zip(blocks, targets))


def wgrad_lists(jobs):
    """csrc/dispatch.h plan_wgrad_lists, restated"""
    n, blocks = len(jobs), [b for b, _ in jobs]
    part_off = [66 * 64 * sum(blocks[:q]) for q in range(n)]
    order = sorted(range(n), key=lambda q: -blocks[q])                  # (sorted is stable)
    seen = list(dict.fromkeys(t for _, t in jobs))                      # first-seen order
    lists = [[q for q in range(n) if jobs[q][1] == t] for t in seen]
    tgt_off = [sum(len(l) for l in lists[:k]) for k in range(len(seen) + 1)]
    return part_off, 66 * 64 * sum(blocks), order, len(seen), order + tgt_off + [q for l in lists for q in l]


def test_the_deferred_weight_gradients_lists(dump):
    cases = list(wgrad_grid())
    assert len(cases) == 45
    for jobs in cases:
        got = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in dump('wgrad', *[v for job in jobs for v in job])}
        part_off, part_floats, order, n_targets, idx = wgrad_lists(jobs)
        assert got == dict(part_off=part_off, part_floats=[part_floats], order=order, n_targets=[n_targets], idx=idx), jobs
    # the stable order and the queue order within a target, spelled out once: ties keep their queue order
    got = dump('wgrad', 3, 9, 16, 4, 3, 9, 1, 2, 16, 4)
    assert got[2] == 'order 1 4 0 2 3' and got[3] == 'n_targets 3' and got[4] == 'idx 1 4 0 2 3 0 2 4 5 0 2 1 4 3'
