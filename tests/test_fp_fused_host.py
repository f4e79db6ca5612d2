"""Host side of the feature-propagation entry points (include/gaddpg.h section C.2) and of PointnetFPModule's `fused` switch: the
symbols, their declarations, the plan registry, the argument checks (which run before any launch) and the module's constructor
and CPU behaviour.  Needs the built library, no GPU."""
import ctypes as C
import os
import re

import torch

NEW = ("gad_fp_rows", "gad_fp_rows_grad", "gad_rows_act_out", "gad_rows_act_bwd_stats")
ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from ga_ddpg_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return hip.lib()


def test_symbols_are_exported_declared_and_replayable():
    from ga_ddpg_amd import hip
    L = _lib()
    header = open(os.path.join(ROOT, "include", "gaddpg.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in hip.EXPORTS and name in hip._SIGNATURES, name
        assert re.search(r"^int %s\(" % name, header, re.M), name + " is not declared in include/gaddpg.h"
        # the ctypes signature has the declaration's argument count
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        assert len(hip._SIGNATURES[name]) == len(decl.split(",")), name
    plan = {L.gad_plan_entry_name(i).decode() for i in range(L.gad_plan_entry_count())}
    assert set(NEW) <= plan
    assert L.gad_abi_version() == 12                  # additive: no bump
    assert "propagate.hip" in open(os.path.join(ROOT, "ga-ddpg_amd", "csrc", "Makefile")).read()


def test_plan_accepts_the_calls_and_refuses_a_wrong_kind():
    from ga_ddpg_amd import engine, hip
    L = _lib()
    p = hip.Ptr(0x1000)
    calls = (("gad_fp_rows", (p, 8, p, p, 1, 4, 3, 8, p, 16, 4)),
             ("gad_fp_rows_grad", (p, 16, 4, p, p, 1, 4, 3, 8, p, 8)),
             ("gad_rows_act_out", (p, 8, p, p, 1, 4, 8, p)),
             ("gad_rows_act_bwd_stats", (p, p, 8, p, p, p, p, 1, 4, 8, p, 8, p, p, 8)))
    h = C.c_void_p()
    hip.check(L.gad_plan_create(C.byref(h)), "gad_plan_create")
    try:
        for name, a in calls:
            words, kinds = engine._pack_words(hip._args(*a))
            k = len(words)
            rc = L.gad_plan_add_call(h, name.encode(), (C.c_uint64 * k)(*words), (C.c_uint8 * k)(*kinds), k, 0)
            assert rc >= 0, (name, L.gad_last_error())
            kinds[1] = 2                                # a float where the entry point takes an int
            assert L.gad_plan_add_call(h, name.encode(), (C.c_uint64 * k)(*words), (C.c_uint8 * k)(*kinds), k, 0) == ERR_SHAPE
            assert L.gad_plan_add_call(h, name.encode(), (C.c_uint64 * k)(*words), (C.c_uint8 * k)(*kinds), k - 1, 0) == ERR_SHAPE
        assert L.gad_plan_size(h) == len(calls)
    finally:
        L.gad_plan_destroy(h)


def test_bad_arguments_are_status_codes_with_a_message():
    L = _lib()
    null, p = C.c_void_p(None), C.c_void_p(0x1000)
    err = lambda: L.gad_last_error()

    fr = L.gad_fp_rows           # (known_pm, k_pitch, idx, weight, B, n, m, C2, rows, r_pitch, col_off, stream)
    for bad in range(4):
        a = [p, 8, p, p, 1, 4, 3, 8, p, 16, 4, null]
        a[(0, 2, 3, 8)[bad]] = null
        assert fr(*a) == ERR_NULL and b"fp_rows: null pointer" in err()
    assert fr(p, 8, p, p, -1, 4, 3, 8, p, 16, 4, null) == ERR_SHAPE and b"negative size" in err()
    assert fr(p, 7, p, p, 1, 4, 3, 8, p, 16, 4, null) == ERR_SHAPE and b"pitch 7" in err()
    assert fr(p, 8, p, p, 1, 4, 3, 8, p, 16, 9, null) == ERR_SHAPE and b"outside a row of pitch 16" in err()
    assert fr(p, 8, p, p, 1, 4, 3, 8, p, 16, -4, null) == ERR_SHAPE and b"outside a row" in err()
    assert fr(p, 8, p, p, 1 << 16, 1 << 15, 3, 8, p, 16, 4, null) == ERR_SHAPE and b"too large" in err()
    assert fr(p, 8, p, p, 1, 4, 0, 8, p, 16, 4, null) == ERR_SHAPE and b"no known point" in err()
    for B, n, c2 in ((0, 4, 8), (1, 0, 8), (1, 4, 0)):          # nothing to write: GAD_OK without a launch
        assert fr(p, 8, p, p, B, n, 0, c2, p, 16, 4, null) == 0

    fg = L.gad_fp_rows_grad      # (drows, r_pitch, col_off, idx, weight, B, n, m, C2, gknown_pm, k_pitch, stream)
    for bad in (0, 3, 4, 9):
        a = [p, 16, 4, p, p, 1, 4, 3, 8, p, 8, null]
        a[bad] = null
        assert fg(*a) == ERR_NULL and b"fp_rows_grad: null pointer" in err()
    assert fg(p, 16, 4, p, p, 1, -4, 3, 8, p, 8, null) == ERR_SHAPE and b"negative size" in err()
    assert fg(p, 16, 12, p, p, 1, 4, 3, 8, p, 8, null) == ERR_SHAPE and b"outside a row" in err()
    assert fg(p, 16, 4, p, p, 1, 4, 3, 8, p, 4, null) == ERR_SHAPE and b"pitch 4" in err()
    assert fg(p, 16, 4, p, p, 1, 4, 0, 8, p, 8, null) == ERR_SHAPE and b"no known point" in err()
    assert fg(p, 16, 4, p, p, 0, 4, 3, 8, p, 8, null) == 0 and fg(p, 16, 4, p, p, 1, 4, 3, 0, p, 8, null) == 0
    from ga_ddpg_amd import hip
    hip.set_option("deterministic", 1)
    try:                                                         # the deterministic mode: refused before any launch
        assert fg(p, 16, 4, p, p, 1, 4, 3, 8, p, 8, null) == ERR_UNSUPPORTED and b"no ordered form" in err()
    finally:
        hip.set_option("deterministic", hip.get_option_default("deterministic"))

    ao = L.gad_rows_act_out      # (z, z_pitch, scale, shift, B, n, C, out, stream)
    for bad in (0, 2, 3, 7):
        a = [p, 8, p, p, 1, 4, 8, p, null]
        a[bad] = null
        assert ao(*a) == ERR_NULL and b"rows_act_out: null pointer" in err()
    assert ao(p, 7, p, p, 1, 4, 8, p, null) == ERR_SHAPE and b"row pitch 7" in err()
    assert ao(p, 8, p, p, 1, 4, -8, p, null) == ERR_SHAPE and b"C=-8" in err()
    assert ao(p, 8, p, p, -1, 4, 8, p, null) == ERR_SHAPE and b"B=-1" in err()
    assert ao(p, 8, p, p, 0, 4, 8, p, null) == 0 and ao(p, 8, p, p, 1, 0, 8, p, null) == 0 and ao(p, 8, p, p, 1, 4, 0, p, null) == 0

    bs = L.gad_rows_act_bwd_stats    # (dout, z, z_pitch, scale, shift, mean, istd, B, n, C, G, g_pitch, dbeta, dgamma, stat_stride, stream)
    for bad in (0, 1, 3, 4, 5, 6, 10, 12, 13):
        a = [p, p, 8, p, p, p, p, 1, 4, 8, p, 8, p, p, 8, null]
        a[bad] = null
        assert bs(*a) == ERR_NULL and b"rows_act_bwd_stats: null pointer" in err()
    assert bs(p, p, 7, p, p, p, p, 1, 4, 8, p, 8, p, p, 8, null) == ERR_SHAPE and b"row pitches 7 / 8" in err()
    assert bs(p, p, 8, p, p, p, p, 1, 4, 8, p, 6, p, p, 8, null) == ERR_SHAPE and b"row pitches 8 / 6" in err()
    assert bs(p, p, 8, p, p, p, p, 1, 4, 8, p, 8, p, p, 7, null) == ERR_SHAPE and b"stat_stride 7" in err()
    assert bs(p, p, 8, p, p, p, p, 1, -4, 8, p, 8, p, p, 8, null) == ERR_SHAPE and b"n=-4" in err()
    assert bs(p, p, 8, p, p, p, p, 0, 4, 8, p, 8, p, p, 8, null) == 0 and bs(p, p, 8, p, p, p, p, 1, 4, 0, p, 8, p, p, 0, null) == 0


def test_fused_switch_leaves_the_state_dict_alone():
    from ga_ddpg_amd.pointnet2_ops.pointnet2_modules import PointnetFPModule
    spec = [13, 32, 16]
    torch.manual_seed(0)
    a = PointnetFPModule(spec)
    torch.manual_seed(0)
    b = PointnetFPModule(spec, fused=True)
    assert a.fused is False and b.fused is True and b.last_route is None
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert not any("fused" in k for k in sb)
    assert list(PointnetFPModule(spec, bn=False, fused=True).state_dict()) == list(PointnetFPModule(spec, bn=False).state_dict())
    a.fused = True                                               # a plain attribute: may be set after construction
    assert list(a.state_dict()) == list(sb)
    try:
        PointnetFPModule(spec, True, True)
    except TypeError:
        pass
    else:
        raise AssertionError("fused must be keyword-only")


def test_cpu_call_with_fused_takes_the_composition():
    from ga_ddpg_amd.pointnet2_ops.pointnet2_modules import PointnetFPModule
    B, n, C1, C2 = 2, 9, 3, 4
    torch.manual_seed(1)
    a = PointnetFPModule([C1 + C2, 8, 8])
    b = PointnetFPModule([C1 + C2, 8, 8], fused=True)
    b.load_state_dict(a.state_dict())
    unknown, uf, kf = torch.rand(B, n, 3), torch.randn(B, C1, n), torch.randn(B, C2, 1)
    outs = []
    for mod in (a, b):
        u, k = uf.clone().requires_grad_(True), kf.clone().requires_grad_(True)
        y = mod(unknown, None, u, k)                              # known=None: the only form torch alone evaluates on the CPU
        y.square().sum().backward()
        outs.append([y.detach(), u.grad, k.grad] + [p.grad for p in mod.parameters()] + list(mod.state_dict().values()))
    assert a.last_route == "composed" and b.last_route == "composed"
    assert len(outs[0]) == len(outs[1]) and all(torch.equal(x, y) for x, y in zip(*outs))
    assert "_gad_rt" not in b.__dict__                           # nothing of the fused path was built
