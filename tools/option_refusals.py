"""Which combinations of the trainer's options train_gnn_dyn refuses, and with what words: a fixed grid walked through train() and
through every check_* function, each point recorded as 'accepted' or as the exception's type and full message.

  python tools/option_refusals.py > tests/golden/train_option_refusals.json        (no device needed)

Run at two commits, the two files are compared entry for entry (tests/test_train_option_refusals.py does it against the
committed file): a refactor of the option checks moves no entry -- the ORDER of the refusals included, which decides the message
a user sees when two apply.  train() is called with a stub model whose engine.train_begin raises a sentinel: reaching it is
'accepted'.  Only public names of train_gnn_dyn are called, so the script runs unchanged at either commit.  The grid:
  schedules   every loss name, a callable and an unknown name x the six probe schedules at 0, 2, -1 and 1.5, alone and in every pair
  options     the same losses x sinkhorn_reach_scale {None, 4.0, inf, 0.0} x sinkhorn_mass x match_weight {0.5, 0.0} x
              transport_iters {50, 0} x impulses {'data', 'actions', 'bogus'}
  reach       'mse', 'sinkhorn' and the callable x each schedule at 2 x sinkhorn_reach_scale x sinkhorn_mass
walk() -> {'outcomes': the distinct outcomes, 'train': [[the point's name, index into outcomes], ...], 'checks': the same per call
of a check_* function, every distinct argument list the grid gives it once}; the file holds compact() of it: the outcomes, and
per section the SHA-256 of the names and the indices alone."""
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dyn_res_pile_manip_amd import train_gnn_dyn as T  # noqa: E402

SCHEDULES = ('grad_probe_every', 'probe_every', 'sinkhorn_probe_every', 'match_probe_every', 'sinkhorn_reach_probe_every',
             'custom_probe_every')
EVERY = (0, 2, -1, 1.5)
DEFAULTS = dict({s: 0 for s in SCHEDULES}, sinkhorn_reach_scale=None, sinkhorn_mass='unit', match_weight=0.5, transport_iters=50,
                impulses='data', transport_eps_scale=T.TRANSPORT_EPS_SCALE)


class CustomLoss(object):
    """a callable loss whose name and repr are the same at every run (a function's repr carries its address)"""
    __name__ = 'custom_loss'

    def __call__(self, pred, context):
        raise AssertionError('the grid never trains')

    def __repr__(self):
        return '<custom_loss>'


custom_loss = CustomLoss()

LOSSES = T.LOSSES + T.MATCH_LOSSES + T.TRANSPORT_LOSSES + T.DIVERGENCE_LOSSES + (custom_loss, 'bogus')


class Reached(Exception):
    pass


class StubEngine(object):
    def train_begin(self, *a, **k):
        raise Reached()


class StubModel(object):
    engine = StubEngine()


CONFIG = {'train': {'n_rollout': 2, 'n_history': 1, 'lr': 1e-3, 'adam_beta1': 0.9, 'n_epoch': 1, 'log_per_iter': 1, 'ckp_per_iter': 1}}


def grid():
    """-> the points, each a dict of the options that differ from DEFAULTS plus 'loss'"""
    points = []
    for loss in LOSSES:
        points.append({'loss': loss})
        for s in SCHEDULES:
            points += [{'loss': loss, s: v} for v in EVERY[1:]]
        for s, t in itertools.combinations(SCHEDULES, 2):
            points += [{'loss': loss, s: v, t: w} for v in EVERY[1:] for w in EVERY[1:]]
    for loss in LOSSES:
        for reach, mass, weight, iters, impulses in itertools.product((None, 4.0, float('inf'), 0.0), T.SINKHORN_MASSES, (0.5, 0.0),
                                                                      (50, 0), ('data', 'actions', 'bogus')):
            points.append({'loss': loss, 'sinkhorn_reach_scale': reach, 'sinkhorn_mass': mass, 'match_weight': weight,
                           'transport_iters': iters, 'impulses': impulses})
    for loss in ('mse', 'sinkhorn', custom_loss):
        for s, reach, mass in itertools.product(SCHEDULES, (None, 4.0, float('inf'), 0.0), T.SINKHORN_MASSES):
            points.append({'loss': loss, s: 2, 'sinkhorn_reach_scale': reach, 'sinkhorn_mass': mass})
    return points


def label(value):
    return value.__name__ if callable(value) else repr(value)


def outcome(fn, *args, **kwargs):
    try:
        fn(*args, **kwargs)
    except Reached:
        return 'accepted'
    except Exception as e:          # noqa: BLE001  (whatever it is, its type and words are the record)
        return '%s: %s' % (type(e).__name__, e)
    return 'accepted'


# every check_* function with the options it takes, in its positional order
CHECKS = (('check_loss', ('loss', 'match_weight', 'transport_eps_scale', 'transport_iters')),
          ('check_sinkhorn_options', ('loss', 'sinkhorn_reach_scale', 'sinkhorn_mass', 'sinkhorn_probe_every', 'transport_eps_scale')),
          ('check_probe_options', ('loss', 'grad_probe_every', 'probe_every')),
          ('check_sinkhorn_probe_option', ('loss', 'sinkhorn_probe_every', 'grad_probe_every', 'probe_every')),
          ('check_match_probe_option', ('loss', 'match_probe_every', 'grad_probe_every', 'probe_every', 'sinkhorn_probe_every')),
          ('check_sinkhorn_reach_probe_option', ('loss', 'sinkhorn_reach_probe_every', 'sinkhorn_reach_scale', 'grad_probe_every',
                                                 'probe_every', 'sinkhorn_probe_every', 'match_probe_every')),
          ('check_custom_probe_option', ('loss', 'custom_probe_every', 'grad_probe_every', 'probe_every', 'sinkhorn_probe_every',
                                         'match_probe_every', 'sinkhorn_reach_probe_every')))


def walk():
    outcomes, index = [], {}

    def record(rows, name, text):
        if text not in index:
            index[text] = len(outcomes)
            outcomes.append(text)
        rows.append([name, index[text]])

    train, checks, seen = [], [], set()
    for point in grid():
        name = ' '.join('%s=%s' % (k, label(point[k])) for k in sorted(point))
        record(train, name, outcome(T.train, CONFIG, StubModel(), {'train': [], 'valid': []}, **point))
        full = dict(DEFAULTS, **point)
        for fn, names in CHECKS:
            args = tuple(full[k] for k in names)
            call = '%s(%s)' % (fn, ', '.join(label(a) for a in args))
            if call not in seen:
                seen.add(call)
                record(checks, call, outcome(getattr(T, fn), *args))
    return {'outcomes': outcomes, 'train': train, 'checks': checks}


def compact(record):
    """walk()'s record as the file holds it: the points' names are the grid's own, which the script regenerates, so a section
    keeps the SHA-256 of its names (one per line) and every point's index into 'outcomes', in the grid's order"""
    out = {'outcomes': record['outcomes']}
    for section in ('train', 'checks'):
        names = '\n'.join(name for name, _ in record[section])
        out[section] = {'names_sha256': hashlib.sha256(names.encode()).hexdigest(), 'outcome': [k for _, k in record[section]]}
    return out


def dumps(small, per_line=60):
    """compact()'s dict as JSON text a diff can show: one outcome per line, the indices per_line to a line"""
    def rows(ks):
        return ',\n'.join('   ' + ','.join('%d' % k for k in ks[i:i + per_line]) for i in range(0, len(ks), per_line))
    text = '{\n "outcomes": [\n%s\n ]' % ',\n'.join('  ' + json.dumps(o) for o in small['outcomes'])
    for section in ('train', 'checks'):
        text += ',\n "%s": {\n  "names_sha256": "%s",\n  "outcome": [\n%s\n  ]\n }' % (
            section, small[section]['names_sha256'], rows(small[section]['outcome']))
    return text + '\n}\n'


if __name__ == '__main__':
    sys.stdout.write(dumps(compact(walk())))
