"""train_gnn_dyn's option checks, held to the record of the commit before they were folded into one table
(tests/golden/train_option_refusals.json, written by tools/option_refusals.py): every point of the grid is accepted or refused
as it was, with the same exception type and the same words -- so the order of the refusals, which decides the message a user
sees when two apply, is held too.  No device."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('option_refusals', os.path.join(ROOT, 'tools', 'option_refusals.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_option_combination_is_refused_or_accepted_as_recorded():
    with open(os.path.join(ROOT, 'tests', 'golden', 'train_option_refusals.json')) as f:
        want = json.load(f)
    tool = _tool()
    got = tool.walk()
    small = tool.compact(got)
    for section in ('train', 'checks'):
        assert small[section]['names_sha256'] == want[section]['names_sha256']              # the same grid, in the same order
        assert len(got[section]) == len(want[section]['outcome']) > 1000
        for (name, g_k), w_k in zip(got[section], want[section]['outcome']):
            assert got['outcomes'][g_k] == want['outcomes'][w_k], name
    assert sum(want['outcomes'][k] == 'accepted' for k in want['train']['outcome']) > 50   # (the stub's train_begin was reached)
