"""GPU: a context gives back everything it allocated.  One child process (tests/_ctx_lifecycle_child.py) runs three cycles of
create, exercise, destroy -- each cycle a rollout at a km_rollout size and at a km_prop3 size, an MPC session with both
drp_mpc_fetch_async slots, a GD session with drp_gd_step_async, a drp_train_step, the regressor's load, forward, training
step and timing entry points, a drp_ptcl_dataset_batch and a probe -- then destroys one context straight after a refused
call (DRP_EINVAL) and one with iterations still pending in both GD slots, and reads the device's free memory after every
destroy.  The first cycle warms the runtime's own pools; every later reading must equal the first cycle's."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The allowance is what the commit before the owning members (teardown by a hand-kept list in drp_destroy) showed on an MI355X
# with this very child: 0 bytes on every reading (308 279 246 848 bytes free after each of the three cycles, after the refused
# call and after the destroy with pending slots; 308 556 070 912 before the first context).  Another tenant of a shared device
# moves the figure either way: a disturbed run is repeated, the allowance stays.
LEAK_ALLOWANCE_BYTES = 0


def test_three_lifecycles_end_at_the_same_free_memory(tmp_path):
    import __graft_entry__ as g
    g.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_ctx_lifecycle_child.py'), str(tmp_path / 'episodes')],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    text = out.stdout.decode(errors='replace')
    assert out.returncode == 0, text[-4000:]
    rec = json.loads([ln for ln in text.splitlines() if ln.startswith('LIFECYCLE ')][-1][len('LIFECYCLE '):])
    first = rec['cycles'][0]
    later = dict(cycle2=rec['cycles'][1], cycle3=rec['cycles'][2], after_refusal=rec['after_refusal'],
                 after_pending=rec['after_pending'])
    lost = {k: first - v for k, v in later.items()}
    print('free bytes at start %d, after cycle 1 %d; lost since cycle 1: %s' % (rec['start'], first, lost))
    assert all(abs(v) <= LEAK_ALLOWANCE_BYTES for v in lost.values()), lost
