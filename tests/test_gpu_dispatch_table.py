"""GPU: the built library serves every call of tests/dispatch_table.txt -- recorded by tools/dispatch_table.py on the commit its
first line names -- with the kernel variants recorded there, line for line."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_recorded_call_gets_the_recorded_variants():
    from dyn_res_pile_manip_amd.engine import Engine
    want = open(os.path.join(ROOT, 'tests', 'dispatch_table.txt')).read().splitlines()
    e = Engine(0)
    n_cu = e.device_info()['n_cu']
    e.close()
    rec = int(re.search(r'n_cu (\d+)', want[0]).group(1))
    assert rec == n_cu, 'the table was recorded on a device of %d CUs, this one has %d: record it again, do not compare' % (rec, n_cu)
    env = {k: v for k, v in os.environ.items() if not k.startswith('DRP_') or k == 'DRP_LIB'}
    got = subprocess.check_output([sys.executable, os.path.join(ROOT, 'tools', 'dispatch_table.py')], env=env, timeout=900).decode().splitlines()
    assert len(got) == len(want)
    bad = [(w, g) for w, g in zip(want[1:], got[1:]) if w != g]
    assert not bad, 'first of %d: recorded %r, now %r' % (len(bad), bad[0][0], bad[0][1])
