"""The launch emitters of engine.py (one spelling per launch of a set-abstraction stage, shared by the update step, the stand-alone
module path and the heads) without a GPU: every emitter is called into a Plan over small CPU tensors, in each of its forms, and the
plan is compiled.  gad_plan_add_call checks the argument count and kinds of an item against the entry point's real signature when
the item is added, so a dropped or transposed positional argument of the 13-to-27-argument calls fails here; for the struct
emitters the fields that are derived rather than passed through are asserted.  Nothing is enqueued: launches the constructors make
(hip.call) are stubbed out, and no plan is run."""
import os

import pytest
import torch

CPU = torch.device("cpu")


@pytest.fixture
def host(monkeypatch):
    from ga_ddpg_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    hip.lib()
    monkeypatch.setattr(hip, "call", lambda *a, **k: None)

    class _Event(object):                      # (Plan.wait makes one per fork / join; it is only used when a plan is walked)
        pass
    monkeypatch.setattr(torch.cuda, "Event", _Event)


def _stage(group_all=False, mlp=(32, 32, 32, 64)):
    """(net, run) of a small stand-alone module on the CPU: 32 feature channels, so layer 1 has a split-bf16 mirror"""
    from ga_ddpg_amd import sa_function
    from ga_ddpg_amd.pointnet2_ops import pointnet2_modules as pm
    torch.manual_seed(0)
    kw = {} if group_all else dict(npoint=4, radius=0.3, nsample=4)
    mod = pm.PointnetSAModule(mlp=list(mlp), **kw)
    net = sa_function._StageNet(mod, CPU)
    return net, sa_function._StageRun(net, mod, 2, 8, CPU, with_backward=True)


def _off(p, t):
    """byte offset of pointer field / hip.Ptr p from the base of tensor t"""
    return int(p) - t.data_ptr()


def _compiles(plan):
    """every item but the fork / join waits (the library creates their events: that needs a device) and host callbacks"""
    from ga_ddpg_amd import engine
    host = engine.Plan()
    host.calls = [it for it in plan.calls if it.kind not in ("wait", "py")]
    assert sum(it.kind == "call" for it in host.calls) >= 1
    c = engine._Compiled(host)
    assert c.n_items == len(host.calls) and len(c.handles) == 1


def test_forward_emitters_in_every_form(host):
    from ga_ddpg_amd import engine
    net, run = _stage()
    v, tot = run.view, run.tot
    plan = engine.Plan()
    for l in range(3):
        o = v.bn_off[l]
        for stats in (True, False):                              # train / the module path's eval forward
            for pooled in ((False, True) if l == 2 else (False,)):
                a = engine.fwd_gemm_args(net, v, l, v.Z[l], stats=stats, pooled=pooled)
                plan.call_struct("gad_gemm_fwd", a)
                assert a.n_groups == 1 and a.n_out[0] == v.mats[l].n_out and a.stat_stride == 2 * tot
                assert (a.pool_key is not None) == pooled and (a.pool_gamma is not None) == pooled
                if stats:
                    assert _off(a.stat_sum, v.stats) == 8 * o and _off(a.stat_sq, v.stats) == 8 * (tot + o)
                else:
                    assert a.stat_sum is None and a.stat_sq is None
                assert (a.mode, a.grp_per_sample) == ((1, run.M) if l == 0 else (0, 1))
                assert (a.W_split is not None) and a.W_split_pitch == (32 if l == 0 else v.mats[l].Kp)
        for update_running in (True, False):
            engine.emit_bn_finalize(plan, net, v, l, update_running)
            if l > 0:                                            # the input layer's BatchNorm finalised by the consumer; recomputed input
                a = engine.fwd_gemm_args(net, v, l, v.Z[l], in_bn=update_running, recompute=l == 1)
                plan.call_struct("gad_gemm_fwd", a)
                po = v.bn_off[l - 1]
                assert _off(a.in_stat_sum, v.stats) == 8 * po and _off(a.in_stat_sq, v.stats) == 8 * (tot + po)
                assert a.in_stat_stride == 2 * tot and a.in_count == v.count and a.mode == (2 if l == 1 else 0)
                assert (a.in_running_mean is not None) == update_running and (a.in_running_var is not None) == update_running
                assert _off(a.in_mean, v.mean) == 4 * po and _off(a.scale, v.scale) == 4 * po
        engine.emit_bn_eval_affine(plan, net, v, l)
    for train in (True, False):
        for update_running in (True, False):
            engine.emit_pool_finalize(plan, net, v, train, update_running)
    assert [it.name for it in plan.calls].count("gad_pool_finalize") == 4
    _compiles(plan)


def test_backward_emitters_in_every_form(host):
    from ga_ddpg_amd import engine
    net, run = _stage()
    v, tot, fl, r = run.view, run.tot, net.flat, run.rows
    ws = torch.empty(1024)
    plan = engine.Plan()
    engine.emit_pool_bwd_stats(plan, v)
    for l in range(3):
        o, m = v.bn_off[l], v.mats[l]
        for accumulate in (True, False):
            engine.emit_bn_bwd_coef(plan, net, v, l, v.count, accumulate=accumulate)
        src = dict(pooled=True) if l == 2 else dict(G=v.G[1 - l])
        for inline in (None, v.count, float("inf")):             # coefficient launch / formed in the consumer's prologue (train, eval)
            for accumulate in (True, False):
                d = engine.bn_dz(net, v, l, inline_count=inline, accumulate=accumulate, **src)
                assert d.c == m.n_out and d.z_pitch == m.n_out and d.gmode == (1 if l == 2 else 0)
                assert _off(d.coefP, v.coef) == 4 * o and _off(d.coefQ, v.coef) == 4 * (tot + o) and _off(d.coefS, v.coef) == 4 * (2 * tot + o)
                if inline is None:
                    assert d.bn_dbeta is None and d.bn_stride == 0 and d.gacc_gamma is None
                else:
                    assert _off(d.bn_dbeta, v.bstats) == 8 * o and _off(d.bn_dgamma, v.bstats) == 8 * (tot + o)
                    assert d.bn_stride == 2 * tot and d.bn_count == inline
                    assert (d.gacc_gamma is not None) == accumulate and (d.gacc_beta is not None) == accumulate
                    if accumulate:
                        assert _off(d.gacc_gamma, fl.gacc) == 8 * m.g_off and _off(d.gacc_beta, fl.gacc) == 8 * m.b_off
                aw = engine.dw_args(fl, [m], engine.layer_input(net, v, l), d, ws)
                assert aw.row_splits == 0 and list(aw.dz_off) == [0, 0, 0] and aw.partial_elems == 1024
                assert aw.inp.n_groups == 1 and aw.inp.w_off[0] == m.w_off and aw.inp.n_out[0] == m.n_out
                if l > 0:
                    pm, po = v.mats[l - 1], v.bn_off[l - 1]
                    a = engine.dx_args(fl, d, m, pm.n_out, r["cap"], engine._ptr(r["n"]), epilogue=0, gout=engine._ptr(v.G[2 - l]),
                                       gout_pitch=pm.n_out, **engine.prev_block(v, l - 1))
                    assert _off(a.prev_dbeta, v.bstats) == 8 * po and _off(a.prev_dgamma, v.bstats) == 8 * (tot + po)
                    assert a.stat_stride == 2 * tot and a.store_masked == 1 and a.zprev_pitch == pm.n_out
                    assert _off(a.prev_mean, v.mean) == 4 * po and _off(a.prev_istd, v.istd) == 4 * po
                    plan.call("gad_gemm_bwd", a, aw)
                else:
                    a = engine.dx_args(fl, d, m, net.c_pad, r["cap"], engine._ptr(r["n"]), epilogue=1, dfeat=engine._ptr(run.dfeat),
                                       feat_c=net.c_pad, row_pt=engine._ptr(r["pt"]), row_grp=engine._ptr(r["grp"]), act_c=0,
                                       grp_per_sample=run.M)
                    assert a.grp_per_sample == run.M and a.W_split_t is not None and a.W_split_t_pitch == m.n_out
                    plan.call_struct("gad_gemm_dw", aw)
                assert a.n_groups == 1 and a.k_valid == (net.c_pad if l == 0 else v.mats[l - 1].n_out) and a.n_rows == r["cap"]
                assert a.n_out[0] == m.n_out and list(a.w_off) == [0, 0, 0] and _off(a.W, fl.packed) == 4 * m.w_off
                plan.call_struct("gad_gemm_dx", a)
    _compiles(plan)


def test_grouped_dx_and_dw_args(host):
    """the heads' form: groups over the whole packed buffer, each with its own dZ / weight / output offset"""
    from ga_ddpg_amd import engine
    net, run = _stage()
    fl, mats = net.flat, net.mats[1:]                            # two 32-wide matrices stand in for a head's trunks
    d = engine._dz(z=None, z_pitch=0, relu=0, gmode=0, G=engine._ptr(run.dF), g_pitch=64, c=64)
    inp = dict(n_rows=2, mode=0, zin=engine._ptr(run.F), zin_pitch=64, c_in=32, relu=1, ones_col=-1, zin_off=[0, 32])
    aw = engine.dw_args(fl, mats, inp, d, torch.empty(512), dz_off=[0, 32])
    assert aw.inp.n_groups == 2 and list(aw.inp.w_off)[:2] == [m.w_off for m in mats] and list(aw.inp.zin_off)[:2] == [0, 32]
    assert list(aw.inp.n_out)[:2] == [m.n_out for m in mats] and list(aw.dz_off) == [0, 32, 0] and aw.row_splits == 0
    gout = torch.empty(2, 64)
    a = engine.dx_args(fl, d, mats[0], 32, 2, groups=[(mats[0], 0, 0), (mats[1], 32, 32)], epilogue=0, gout=engine._ptr(gout),
                       gout_pitch=64)
    assert a.n_groups == 2 and a.n_rows_dev is None and a.n_rows == 2 and a.k_valid == 32 and _off(a.W, fl.packed) == 0
    assert list(a.w_off)[:2] == [m.w_off for m in mats] and list(a.dz_off) == [0, 32, 0] and list(a.gout_off) == [0, 32, 0]
    assert list(a.n_out)[:2] == [m.n_out for m in mats]
    plan = engine.Plan()
    plan.call_struct("gad_gemm_dw", aw)
    plan.call_struct("gad_gemm_dx", a)
    _compiles(plan)


def test_group_all_has_no_centroids(host):
    from ga_ddpg_amd import engine
    net, run = _stage(group_all=True)
    a = engine.fwd_gemm_args(net, run.view, 0, run.Z[0])
    assert a.ctr_xyz is None and a.src_xyz is not None and a.grp_per_sample == 1 and a.feat_c == net.c_pad
    assert a.c_in == net.c_pad + 3 and a.action is None and a.act_c == 0
    plan = engine.Plan()
    plan.call_struct("gad_gemm_fwd", a)
    _compiles(plan)


@pytest.mark.parametrize("group_all", [False, True])
@pytest.mark.parametrize("mlp", [(32, 32, 32, 64), (6, 32, 32, 32)])       # fused pool / padded features and the segment-pool fallback
def test_module_plans_compile(host, group_all, mlp):
    net, run = _stage(group_all, mlp)
    assert run.fused_pool == (mlp[-1] % 64 == 0)
    for plan in (run.plans[True], run.plans[False], run.bwd, run.coord_backward(net)):
        _compiles(plan)


def test_encoder_and_head_plans_compile(host):
    """the update step's callers of the same emitters, at B = 2: every plan compiles against the library's signatures"""
    from ga_ddpg_amd import engine, heads
    from ga_ddpg_amd.core import networks
    from ga_ddpg_amd.synth_data import PandaTaskSpace6D
    torch.manual_seed(0)
    B = 2
    fe = networks.PointNetFeature(input_dim=5, extra_latent=1, action_concat=True)
    enc = engine.EncoderNet(fe.value_encoder, CPU)
    geo = engine.Geometry(B, 1024, engine.SAConfig(32, 0.02, 64), engine.SAConfig(32, 0.04, 128), CPU)
    slot, action = engine.EncoderSlot(geo, enc, CPU), torch.zeros(B, 6)
    views = engine.encoder_views(enc, slot, action)
    assert [v.grp_per_sample for v in views[:3]] == [32, 32, 1] and [v.act_c for v in views[:3]] == [6, 0, 0]
    assert views[2].ctr_xyz is None and views[3].rows is None and views[1].feat is slot.F[0]
    for train in (True, False):
        for update_running in (True, False):
            _compiles(engine.plan_encoder_forward(enc, slot, action=action, train=train, update_running=update_running))
        _compiles(engine.plan_encoder_backward(enc, slot, torch.zeros(B, 512), action=action, want_daction=True, train=train))
    crit = networks.QNetwork(513, 0, 256, extra_pred_dim=7)
    pol = networks.GaussianPolicy(513, 6, 256, PandaTaskSpace6D(), extra_pred_dim=7)
    cr, po = heads.CriticNet(crit, CPU), heads.PolicyNet(pol, CPU)
    time = torch.zeros(B)
    _compiles(heads.plan_critic_backward(cr, heads.HeadSlot(B, cr.width, 9, CPU), enc, slot, time, join_dw=True))
    _compiles(heads.plan_policy_backward(po, heads.HeadSlot(B, po.hidden, 13, CPU), enc, slot, time))
