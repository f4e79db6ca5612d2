"""Host side of the plan layer (engine._Item / _Compiled / Plan) without a GPU: which gad_plan handles Plan.patch writes through.
Nothing is enqueued before gad_plan_run, so plans are compiled, patched and destroyed here and never run.  The library's
gad_plan_create / gad_plan_destroy / gad_plan_patch are wrapped: a handle is LIVE from its create to its destroy, and a patch is
judged by membership in that set when it is made -- not by address, the allocator hands a destroyed plan's address out again.  A
patch of a handle that is not live is recorded and NOT forwarded to the library."""
import gc
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Calls(object):
    def __init__(self):
        self.live = set()          # handles created and not yet destroyed
        self.patches = []          # (handle, handle was live, item index, word index, value)

    def take(self):
        out, self.patches = self.patches, []
        return out


@pytest.fixture
def calls(monkeypatch):
    from ga_ddpg_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    L = hip.lib()
    create, destroy, patch = L.gad_plan_create, L.gad_plan_destroy, L.gad_plan_patch
    rec = _Calls()

    def gad_plan_create(ref):
        rc = create(ref)
        if rc == 0:
            rec.live.add(ref._obj.value)
        return rc

    def gad_plan_destroy(h):
        rec.live.discard(h.value)
        return destroy(h)

    def gad_plan_patch(h, item, word, value):
        live = h.value in rec.live
        rec.patches.append((h.value, live, item, word, value.value))
        return patch(h, item, word, value) if live else 0

    monkeypatch.setattr(L, "gad_plan_create", gad_plan_create, raising=False)
    monkeypatch.setattr(L, "gad_plan_destroy", gad_plan_destroy, raising=False)
    monkeypatch.setattr(L, "gad_plan_patch", gad_plan_patch, raising=False)
    gc.collect()
    yield rec
    gc.collect()                   # (plans of the test that are still around go while the wrappers are in place)


def _noise_plan():
    """a one-launch plan: gad_target_noise(pi, u, B, level, normal, out) -> (plan, item); argument 3 is the float to patch"""
    from ga_ddpg_amd import engine, hip
    sub = engine.Plan()
    it = sub.call("gad_target_noise", hip.Ptr(0x1000), hip.Ptr(0x2000), 4, 0.5, 0, hip.Ptr(0x3000))
    return sub, it


def test_patch_of_a_shared_item_reaches_only_the_live_compiled_plan(calls):
    from ga_ddpg_amd import engine
    sub, it = _noise_plan()
    outer = engine.Plan()
    outer.extend(sub)                                  # on=0: the SAME item sits in both plans
    assert outer.calls[0] is it
    c1 = engine._Compiled(outer)
    del c1
    gc.collect()
    assert not calls.live
    c2 = engine._Compiled(outer)
    engine.Plan.patch(it, 3, 0.25)
    assert calls.take() == [(c2.handles[0].value, True, 0, 3, engine._float_word(0.25))]
    assert len(it.cpos) == 1
    for k in range(50):                                # an item that outlives many compiled plans collects no positions
        del c2
        gc.collect()
        c2 = engine._Compiled(outer)
        assert len(it.cpos) == 1 and len(calls.live) == 1
    engine.Plan.patch(it, 3, 0.75)
    assert calls.take() == [(c2.handles[0].value, True, 0, 3, engine._float_word(0.75))]


def test_patch_reaches_a_clone_while_its_plan_lives_and_not_after(calls):
    from ga_ddpg_amd import engine
    sub, it = _noise_plan()
    own = engine._Compiled(sub)
    outer = engine.Plan()
    outer.extend(sub, on=20)                           # on != 0: outer holds a copy of the item on logical stream 20
    clone = outer.calls[0]
    assert clone is not it and clone.on == 20 and list(it.clones) == [clone]
    co = engine._Compiled(outer)
    assert co.whichs == [0, 20]
    engine.Plan.patch(it, 3, 0.25)
    got = calls.take()
    assert sorted(got) == sorted((h.value, True, 0, 3, engine._float_word(0.25)) for h in (own.handles[0], co.handles[0]))
    del clone, co, outer
    gc.collect()
    assert len(calls.live) == 1
    assert list(it.clones) == []                       # the source no longer reaches the dropped copy
    engine.Plan.patch(it, 3, 0.5)
    assert calls.take() == [(own.handles[0].value, True, 0, 3, engine._float_word(0.5))]


def test_recompile_through_plan_leaves_no_position_in_the_replaced_form(calls):
    """Plan._add resets the compiled form; what Plan.run does next is `self._c = _Compiled(self)` (run itself needs a stream)"""
    from ga_ddpg_amd import engine, hip
    plan, it = _noise_plan()
    plan._c = engine._Compiled(plan)
    first = plan._c.handles[0].value
    assert calls.live == {first}
    it2 = plan.call("gad_target_noise", hip.Ptr(0x1000), hip.Ptr(0x2000), 4, 0.5, 0, hip.Ptr(0x4000))
    assert plan._c is None
    gc.collect()
    assert not calls.live
    plan._c = engine._Compiled(plan)
    h = plan._c.handles[0].value
    engine.Plan.patch(it, 3, 0.25)
    engine.Plan.patch(it2, 3, 0.125)
    assert calls.take() == [(h, True, 0, 3, engine._float_word(0.25)), (h, True, 1, 3, engine._float_word(0.125))]
    assert calls.live == {h} and len(it.cpos) == 1


def test_patch_of_memcpy_and_event_items(calls):
    from ga_ddpg_amd import engine

    class Holder(object):                              # (stands in for engine.EventHolder, which records a real event)
        def __init__(self, handle):
            self.handle = handle

    plan = engine.Plan()
    cp = plan.memcpy(0x10, 0x20, 64, on=2)
    rec = plan.record(None)
    wev = plan.wait_event(Holder(0x500), on=2)
    c = engine._Compiled(plan)
    h = c.handles[0].value
    engine.Plan.patch(cp, 0, 0x30)
    engine.Plan.patch(cp, 1, 0x40)
    assert cp.words == [0x30, 0x40, 64]
    assert calls.take() == [(h, True, 0, 0, 0x30), (h, True, 0, 1, 0x40)]
    a = Holder(0x600)
    engine.Plan.patch(rec, 0, a)
    engine.Plan.patch(wev, 0, None)
    assert rec.holder is a and wev.holder is None
    assert calls.take() == [(h, True, 1, 0, 0x600), (h, True, 2, 0, 0)]


def test_no_exception_from_a_compiled_plan_at_interpreter_exit():
    code = ("from ga_ddpg_amd import engine, hip\n"
            "p = engine.Plan()\n"
            "p.call('gad_target_noise', hip.Ptr(0x1000), hip.Ptr(0x2000), 4, 0.5, 0, hip.Ptr(0x3000))\n"
            "c = engine._Compiled(p)\n"
            "print('compiled', len(c.handles))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and b"compiled 1" in r.stdout, r.stderr.decode()
    assert b"Exception ignored" not in r.stderr, r.stderr.decode()
