"""gad_sa_coord_grad (include/gaddpg.h section C) and the `coordinate_grad` switch of the set-abstraction modules, as far as they
go without a GPU: every refusal is a host-side check in front of the launches, so bad arguments come back as status codes with a
message (RuntimeError through hip.check), the empty shapes are GAD_OK, the deterministic mode refuses, a plan checks the item's
argument words against the real signature, and the switch is a keyword-only constructor argument outside state_dict."""
import ctypes as C

import pytest

GAD_OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED = 0, -1, -2, -4
P = 0x10000          # a non-null, 16-byte aligned dummy address: nothing below dereferences it


def _dz(n_out=32, **kw):
    from ga_ddpg_amd import hip
    d = hip.DzSrc()
    d.z, d.z_pitch, d.G, d.g_pitch, d.c = P, n_out, P, n_out, n_out
    d.coefP, d.coefQ, d.coefS, d.row_w = P, P, P, P
    d.gmode, d.relu, d.premasked = 0, 1, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(dz=None, W=P, Kp=16, n_out=32, col0=4, n_dev=P, n_rows=300, row_pt=P, row_grp=P, ctr=P, g_new=P, G=8, n_pts=64, dxyz=P,
          dctr=P):
    from ga_ddpg_amd import hip
    L = hip.lib()
    dz = _dz(n_out) if dz is None else dz
    rc = L.gad_sa_coord_grad(dz if dz != 0 else None, W, Kp, n_out, col0, n_dev, n_rows, row_pt, row_grp, ctr, g_new, G, n_pts,
                             dxyz, dctr, None)
    return rc, L.gad_last_error().decode()


def test_argument_refusals_are_status_codes():
    from ga_ddpg_amd import hip
    assert hip.get_option("deterministic") == 0
    for kw in (dict(dz=0), dict(W=None), dict(row_pt=None), dict(dxyz=None)):
        rc, msg = _call(**kw)
        assert rc == ERR_NULL and "null" in msg, (kw, rc, msg)
    for kw in (dict(Kp=-8), dict(n_out=-1), dict(col0=-1), dict(n_rows=-1), dict(G=-1), dict(n_pts=-1)):
        rc, msg = _call(**kw)
        assert rc == ERR_SHAPE and "negative" in msg, (kw, rc, msg)
    rc, msg = _call(Kp=16, col0=14)                                   # columns 14, 15, 16: one past the packed row
    assert rc == ERR_SHAPE and "Kp 16" in msg
    rc, msg = _call(n_out=0, dz=_dz(0))
    assert rc == ERR_SHAPE and "n_out 0" in msg
    assert _call(n_out=1025, dz=_dz(1025))[0] == ERR_SHAPE
    # row_grp given without the centroids' point numbers or without dctr; centroids or g_new_xyz without what they need
    for kw in (dict(ctr=None), dict(dctr=None), dict(row_grp=None, g_new=None), dict(row_grp=None, ctr=None, dctr=None)):
        rc, msg = _call(**kw)
        assert rc == ERR_NULL, (kw, rc, msg)
    # the gradient source must be the first layer's: dense, premasked, coefficients together, c == n_out
    assert _call(dz=_dz(gmode=1))[0] == ERR_NULL
    assert _call(dz=_dz(G=None))[0] == ERR_NULL
    assert _call(dz=_dz(premasked=0))[0] == ERR_UNSUPPORTED
    assert _call(dz=_dz(coefQ=None))[0] == ERR_NULL
    assert _call(dz=_dz(z=None))[0] == ERR_NULL
    assert _call(dz=_dz(c=16))[0] == ERR_SHAPE
    assert _call(dz=_dz(g_pitch=16))[0] == ERR_SHAPE
    assert _call(dz=_dz(bn_dbeta=P))[0] == ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match="gad_sa_coord_grad failed.*Kp 8"):
        # (hip.call = these arguments converted by hip._args, the current stream appended -- which needs a device -- then hip.check)
        argv = hip._args(_dz(), hip.Ptr(P), 8, 32, 6, hip.Ptr(P), 300, hip.Ptr(P), hip.Ptr(P), hip.Ptr(P), hip.Ptr(P), 8, 64,
                         hip.Ptr(P), hip.Ptr(P))
        hip.check(hip.lib().gad_sa_coord_grad(*(argv + [None])), "gad_sa_coord_grad")


def test_empty_shapes_are_ok_without_a_launch():
    assert _call(n_rows=0)[0] == GAD_OK
    assert _call(G=0)[0] == GAD_OK
    assert _call(n_rows=0, row_grp=None, ctr=None, g_new=None, dctr=None, G=4)[0] == GAD_OK      # the GroupAll form


def test_deterministic_mode_refuses():
    from ga_ddpg_amd import hip
    try:
        hip.set_option("deterministic", 1)
        rc, msg = _call()
        assert rc == ERR_UNSUPPORTED and "deterministic" in msg
        assert _call(row_grp=None, ctr=None, g_new=None, dctr=None)[0] == ERR_UNSUPPORTED
        assert _call(n_rows=0)[0] == GAD_OK                          # nothing to add: nothing to order
    finally:
        hip.set_option("deterministic", hip.get_option_default("deterministic"))


def test_plan_item_is_checked_against_the_signature():
    from ga_ddpg_amd import engine, hip
    L = hip.lib()
    names = {L.gad_plan_entry_name(i).decode() for i in range(L.gad_plan_entry_count())}
    assert "gad_sa_coord_grad" in names
    dz = _dz()
    argv = hip._args(dz, hip.Ptr(P), 16, 32, 4, hip.Ptr(P), 300, hip.Ptr(P), None, None, None, 8, 64, hip.Ptr(P), None)
    words, kinds = engine._pack_words(argv)
    assert kinds == [1, 1, 0, 0, 0, 1, 0, 1, 1, 1, 1, 0, 0, 1, 1] and words[0] == C.addressof(dz)
    n = len(words)
    h = C.c_void_p()
    assert L.gad_plan_create(C.byref(h)) == 0
    try:
        W, K = (C.c_uint64 * n)(*words), (C.c_uint8 * n)(*kinds)
        assert L.gad_plan_add_call(h, b"gad_sa_coord_grad", W, K, n, 0) == 0
        assert L.gad_plan_add_call(h, b"gad_sa_coord_grad", W, K, n - 1, 0) < 0 and b"takes 15 arguments" in L.gad_last_error()
        K[2] = 1                                                     # Kp packed as a pointer-sized word
        assert L.gad_plan_add_call(h, b"gad_sa_coord_grad", W, K, n, 0) < 0 and b"argument 2" in L.gad_last_error()
        K[2], K[13] = 0, 2                                           # dxyz packed as a float
        assert L.gad_plan_add_call(h, b"gad_sa_coord_grad", W, K, n, 0) < 0 and b"argument 13" in L.gad_last_error()
        assert L.gad_plan_size(h) == 1
    finally:
        assert L.gad_plan_destroy(h) == 0


def test_constructor_keyword():
    import inspect
    from ga_ddpg_amd.pointnet2_ops import pointnet2_modules as pm
    for cls, kw in ((pm.PointnetSAModule, dict(mlp=[4, 8, 8, 8], npoint=8, radius=0.1, nsample=8)),
                    (pm.PointnetSAModuleMSG, dict(npoint=8, radii=[0.1, 0.2], nsamples=[4, 8], mlps=[[4, 8, 8, 8], [4, 8, 8, 16]]))):
        par = inspect.signature(cls.__init__).parameters["coordinate_grad"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False
        m = cls(**kw)
        assert m.coordinate_grad is False
        keys = list(m.state_dict().keys())
        on = cls(coordinate_grad=True, **kw)
        assert on.coordinate_grad is True and list(on.state_dict().keys()) == keys and not any("coord" in k for k in keys)
        m.coordinate_grad = True                                     # a plain attribute: may be set after construction
        assert list(m.state_dict().keys()) == keys and "coordinate_grad" not in dict(m.named_buffers())
        m.load_state_dict(on.state_dict())
    with pytest.raises(TypeError):
        pm.PointnetSAModule([4, 8, 8, 8], 8, 0.1, 8, True, True, True)       # keyword-only
