"""Host: the context's device buffers, pinned blocks, events and stream are owned by the members that hold them
(csrc/capi_ctx.h), so the raw allocate / free calls of the HIP runtime each have one home in csrc/ and drp_destroy frees by
destruction.  Read from the sources; nothing is compiled or run."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'dyn_res_pile_manip_amd', 'csrc')


def _sources():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, '*.h')) + glob.glob(os.path.join(CSRC, '*.hip')))}


def _sites(needle):
    """(file, line number, line) of every occurrence in csrc/"""
    return [(f, i + 1, ln) for f, text in _sources().items() for i, ln in enumerate(text.splitlines()) for _ in range(ln.count(needle))]


def _body(text, head):
    """the text of the block that opens on the first line containing `head`, braces matched"""
    start = text.index(head)
    i = text.index('{', start)
    depth = 0
    for j in range(i, len(text)):
        depth += text[j] == '{'
        depth -= text[j] == '}'
        if depth == 0:
            return text[start:j + 1]
    raise AssertionError('unbalanced block after %r' % head)


def _only_inside(needle, fname, head):
    block = _body(_sources()[fname], head)
    sites = _sites(needle)
    assert sites, needle
    assert all(f == fname and ln.strip() in block for f, _, ln in sites), (needle, sites)
    return sites


def test_each_free_has_one_home_in_its_owner():
    for needle, head in (('hipFree(', 'struct DevBuf {'), ('hipHostFree(', 'struct PinBuf {'), ('hipEventDestroy(', 'struct Event {'),
                         ('hipStreamDestroy(', 'struct Stream {')):
        assert len(_only_inside(needle, 'capi_ctx.h', head)) == 1, needle


def test_each_allocation_has_one_home():
    _only_inside('hipMalloc(', 'capi_pipeline.h', 'int ensure(drp_ctx* c, DevBuf& b, size_t bytes) {')
    _only_inside('hipHostMalloc(', 'capi_pipeline.h', 'int ensure_pinned(drp_ctx* c, PinBuf& b, size_t bytes) {')
    _only_inside('hipEventCreate', 'capi_ctx.h', 'struct Event {')


def test_the_stream_is_the_first_member_and_the_context_has_no_destructor():
    ctx = _body(_sources()['capi_ctx.h'], 'struct drp_ctx {')
    members = [ln.strip() for ln in ctx.splitlines()[1:] if ln.strip() and not ln.strip().startswith('//')]
    assert members[0].startswith('Stream stream;'), members[0]
    assert '~drp_ctx' not in ctx
    # no resource is held as a bare pointer or handle any more
    assert not re.search(r'hipEvent_t\s+\w+(\[|\s*=|;)', ctx) and 'hipStream_t stream' not in ctx
    for gone in ('gd_pin_floats', 'mpc_pin_floats', 'tr_pin_cap', 'pd_pin_cap'):
        assert all(gone not in text for text in _sources().values()), gone


def test_drp_destroy_frees_by_destruction():
    body = _body(_sources()['capi_core.h'], 'void drp_destroy(drp_ctx* c) {')
    assert '&c->' not in body and 'bufs' not in body
    assert len(body.splitlines()) <= 12, body
    for step in ('hipSetDevice(c->device)', 'guarded_wait(c, nullptr)', 'helpers_wait(', 'CommDestroy(c->comm)', 'delete c;'):
        assert step in body, step
    assert body.index('guarded_wait') < body.index('delete c;')
    create = _body(_sources()['capi_core.h'], 'int drp_create(int device, drp_ctx** out) {')
    assert 'std::unique_ptr<drp_ctx>' in create and 'c.release()' in create and 'delete c' not in create


def test_the_owners_are_move_only():
    text = _sources()['capi_ctx.h']
    m = re.search(r'static_assert\((.*?)"a resource has one owner"\);', text, re.S)
    assert m, 'the static_assert on the owners is gone'
    for t in ('DevBuf', 'PinBuf', 'Event'):
        assert '!std::is_copy_constructible<%s>::value' % t in m.group(1), t
        assert '!std::is_copy_assignable<%s>::value' % t in m.group(1), t
        owner = _body(text, 'struct %s {' % t)
        assert '%s(const %s&) = delete;' % (t, t) in owner and '%s& operator=(const %s&) = delete;' % (t, t) in owner, t
        assert '~%s() { (void)release(); }' % t in owner, t


# ---- a step's engine and buffers are arguments (StepArgs); a float64 call swaps one struct (StepWs) -----------------------
def test_nobody_but_the_owners_assigns_an_owned_pointer():
    """`x.p = ...` outside DevBuf / PinBuf would make an owner hold memory it did not allocate (a view is a plain pointer)"""
    for f, text in _sources().items():
        if f == 'capi_ctx.h':
            for owner in ('struct DevBuf {', 'struct PinBuf {'):
                text = text.replace(_body(text, owner), '')
        hits = [ln.strip() for ln in text.splitlines() if re.search(r'\.p\s*=[^=]', ln)]
        assert not hits, (f, hits)


def test_the_selected_engine_is_written_by_its_two_entry_points_only():
    core = _sources()['capi_core.h']
    homes = _body(core, 'int drp_create(int device, drp_ctx** out) {') + _body(core, 'int drp_set_engine(drp_ctx* c, int engine) {')
    sites = [(f, n, ln) for f, text in _sources().items() for n, ln in enumerate(text.splitlines(), 1) if re.search(r'->engine\s*=[^=]', ln)]
    assert len(sites) == 3, sites
    assert all(f == 'capi_core.h' and ln.strip() in homes for f, _, ln in sites), sites


def test_ensure_step_ws_and_stepws_name_the_same_fourteen_buffers():
    ws = _body(_sources()['capi_ctx.h'], 'struct StepWs {')
    members = [m for decl in re.findall(r'DevBuf\s+([^;]+);', ws) for m in re.findall(r'\w+', decl)]
    assert len(members) == 14 and len(set(members)) == 14, members
    named = set(re.findall(r'\bws\.(\w+)', _body(_sources()['capi_pipeline.h'], 'int ensure_step_ws(drp_ctx* c, StepWs& ws,')))
    assert named == set(members), (sorted(named), sorted(members))
    # and the float64 calls swap the struct whole: no list of buffers to keep in step
    scope = _body(_sources()['capi_f64.h'], 'struct F64Scope {')
    assert scope.count('std::swap(c->ws, c->f64_ws);') == 2 and 'DevBuf' not in scope, scope


# ---- a gradient pass takes its outputs as arguments (GdPass, TrainPass); the weight-gradient queue is one struct; one guard drains ----
def test_no_gradient_pass_patches_the_context():
    for gone in ('gd_adam', 'gd_host_rewards', 'gd_host_actions', 'tr_loss_host', 'tr_engine', 'wg_defer_now', 'LossHostReset'):
        assert not _sites(gone), (gone, _sites(gone)[:3])


def test_the_weight_gradient_queue_keeps_its_state_to_itself():
    for needle in ('wg_jobs', 'wg_uploaded', 'wg_jobs_dev', 'wg_idx_dev'):
        _only_inside(needle, 'capi_pipeline.h', 'struct WgradQueue {')


def test_the_guard_stands_before_the_first_launch_and_no_exit_drains_by_hand():
    """DrainOnError (capi_pipeline.h) waits for the stream on every exit but the DRP_OK one: constructed before anything is
    launched, disarmed by the last return"""
    train, gd = _sources()['capi_train.h'], _sources()['capi_gd.h']
    launch = r'hipLaunchKernelGGL|gd_iteration\(|gd_forward_backward\(|train_stage_batch\(|train_attempt\(|train_forward_backward\('
    for text, head in ((train, 'int train_step_body(drp_ctx* c,'), (gd, 'int drp_gd_grad(drp_ctx* c,'),
                       (gd, 'int drp_gd_step(drp_ctx* c,'), (gd, 'int drp_gd_step_async(drp_ctx* c,')):
        body = _body(text, head)
        guard = body.index('DrainOnError drain(c);')
        launches = [m.start() for m in re.finditer(launch, body)]
        assert launches and guard < min(launches), head
        assert body.count('drain.ok()') == 1 and body.rstrip('} \n').endswith('return drain.ok();'), head
    # what train_step_body calls before its guard launches nothing; the staging and the attempts come behind it
    for head in ('int train_check_args(drp_ctx* c,', 'int train_ensure_workspace(drp_ctx* c,'):
        assert 'hipLaunchKernelGGL' not in _body(train, head), head
    for head in ('int train_stage_batch(drp_ctx* c,', 'int train_attempt(drp_ctx* c,'):
        assert 'hipLaunchKernelGGL' in _body(train, head), head
    assert '(void)drp_sync(c); return' not in train
