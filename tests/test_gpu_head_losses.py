"""The head-loss kernels of ga-ddpg_amd/csrc/losses.hip called directly (hip.call), against a float64 evaluation of the
reference formulas (oracle/ref_step.py: goal_pred_loss, pose_bc_loss, target_noise, PolicyNet.sample's formulas,
_unit_quat_head) with autograd for the gradients.

Criterion (the style of tests/test_gpu_forced_decisions.py): per output tensor, the kernel's max error relative to the
tensor's max |float64| is at most max(3 x torch float32's own error on the same inputs, 1e-6); counts are exact.  Every
output the header documents as written for every row starts as a NaN sentinel and must come back written (NaN exactly
where the float64 reference is NaN: torch's mean over an empty mask).  Random draws keep every L1 / smooth-L1 argument at
least 1e-4 away from its kink; the kink cases put arguments exactly on it (then both sides evaluate the same exact value).
B > 256 is the first size where one thread of the single-workgroup kernels loops over several rows; 512 is configs[4]."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BS = (1, 7, 64, 255, 256, 257, 512, 1000)
KINK = 1e-4
GAMMA = float(np.float32(0.95))


# ----------------------------------------------------------------------------- plumbing
def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))


def _dev(a):
    return torch.from_numpy(_f32(a)).cuda()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().astype(np.float64)


def _T(a, dtype):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype)


def _np(t):
    return t.detach().double().numpy()


def _space(kind):
    """(scale, bias) as the policy holds them (float32 buffers); bias None = symmetric bounds (the kernels' NULL)"""
    from oracle import ref_step
    from oracle.detfill import AsymTaskSpace6D
    if kind is None:
        return _f32(ref_step.ACTION_HIGH), None
    s = AsymTaskSpace6D()
    return _f32((s.high - s.low) / 2.0), _f32((s.high + s.low) / 2.0)


def _check(what, got, r64, r32):
    """max |got - f64| / max |f64| <= max(3 x the same for torch float32, 1e-6); NaN exactly where the reference is NaN"""
    got, r64, r32 = (np.asarray(x, dtype=np.float64) for x in (got, r64, r32))
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    nan = np.isnan(r64)
    bad = np.isnan(got) != nan
    assert not bad.any(), "%s: %d entries NaN / written where the float64 reference is not (first flat index %d)" % (
        what, int(bad.sum()), int(np.flatnonzero(bad)[0]))
    if nan.all():
        return
    scale = np.abs(r64[~nan]).max()
    if scale == 0.0:
        assert (got[~nan] == 0.0).all(), "%s: reference is all zero, kernel max |.| %.3e" % (what, np.abs(got[~nan]).max())
        return
    eh = np.abs(got - r64)[~nan].max() / scale
    e32 = np.abs(r32 - r64)[~nan].max() / scale
    assert eh <= max(3.0 * e32, 1e-6), "%s: max err / max|f64| = %.3e (at flat index %d), torch float32 %.3e" % (
        what, eh, int(np.argmax(np.where(nan, -1.0, np.abs(got - r64)))), e32)


def _redraw(draw, bad_rows, B, rng):
    """rows drawn by draw(rng, idx) -> dict of (len(idx), ...) arrays for the row indices idx; rows with bad_rows(dict)
    True are drawn again (draw keeps whatever structure a case puts on a row index)"""
    d = draw(rng, np.arange(B))
    for _ in range(200):
        bad = np.flatnonzero(bad_rows(d))
        if not len(bad):
            return {k: _f32(v) for k, v in d.items()}
        nd = draw(rng, bad)
        for k in d:
            d[k][bad] = nd[k]
    raise AssertionError("could not draw rows away from the kinks")


def _near(a, at=0.0):
    """within KINK of `at` without being exactly on it (exact hits are the kink cases)"""
    a = np.abs(np.asarray(a, dtype=np.float64) - at)
    return (a > 0) & (a < KINK)


def _near_kink(d):
    """per row: some L1 argument within KINK of zero without being exactly zero"""
    return _near(d.reshape(d.shape[0], -1)).any(1)


def _unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def _goal_pts(g):
    """(n,7) float64 tensor, quaternion already normalised -> (n,6,3) control points (core/loss.py:17-23)"""
    from oracle import ref_step
    cp = ref_step.control_points(True, "cpu", g.dtype)[None]
    return ref_step.quat_rotate(g[:, None, :4].expand(-1, 6, -1), cp.expand(g.shape[0], -1, -1)) + g[:, None, 4:]


def _goal_args(pred7, goal7):
    from oracle import ref_step
    p = ref_step._unit_quat_head(_T(_f32(pred7), torch.float64))
    return (_goal_pts(p) - _goal_pts(_T(_f32(goal7), torch.float64))).numpy()


def _bc_pts(a):
    from oracle import ref_step
    cp = ref_step.control_points(False, "cpu", a.dtype)[None]
    R = ref_step.euler_matrix(a[:, 3], a[:, 4], a[:, 5])
    return cp.expand(a.shape[0], -1, -1) @ R.transpose(1, 2) + a[:, None, :3]


def _bc_args(pi, act):
    return (_bc_pts(_T(pi, torch.float64)) - _bc_pts(_T(_f32(act), torch.float64))).numpy()


def _goal_rows(rng, n, spread=0.15):
    return np.concatenate([_unit(rng.normal(size=(n, 4))), rng.uniform(-spread, spread, (n, 3))], 1)


def _returns(rng, n, p=0.5):
    return np.where(rng.random(n) < p, rng.uniform(0.01, 1.0, n), np.where(rng.random(n) < 0.5, 0.0, -0.5))


# ----------------------------------------------------------------------------- gad_critic_loss
def _critic_ref(x, critic_aux, dtype):
    """core/ddpg.py:61-88,119-130 + core/loss.py:17-23 in `dtype`: (y, aux_norm, g_out9, closs, aloss)"""
    from oracle import ref_step
    o = _T(x["out9"], dtype).requires_grad_(True)
    tgt = _T(x["tgt9"], dtype)
    y = _T(x["reward"], dtype) + (1 - _T(x["done"], dtype)) * GAMMA * torch.min(tgt[:, 0], tgt[:, 1])
    keep = torch.from_numpy(x["perturb"] < 1)
    gm = torch.from_numpy(x["ret"] > 0)
    closs = F.smooth_l1_loss(o[:, 0][keep], y[keep]) + F.smooth_l1_loss(o[:, 1][keep], y[keep])
    aux = ref_step._unit_quat_head(o[:, 2:9])
    aloss = ref_step.goal_pred_loss(aux[gm], _T(x["goal"], dtype)[gm]) if critic_aux else torch.zeros((), dtype=dtype)
    (closs + aloss).backward()
    return {"y": _np(y), "aux_norm": _np(aux), "g_out9": _np(o.grad),
            "scalars": np.array([float(closs), float(aloss), float(keep.sum()), float(gm.sum())])}


def _critic_inputs(rng, B, variant):
    def draw(r, idx):
        n = len(idx)
        q = r.normal(0.5, 1.0, (n, 2))
        x = {"out9": np.concatenate([q, r.normal(size=(n, 4)), r.uniform(-0.15, 0.15, (n, 3))], 1),
             "tgt9": r.normal(size=(n, 9)), "reward": r.random(n), "done": (r.random(n) < 0.3).astype(np.float64),
             "perturb": np.where(r.random(n) < 0.2, 1.0, np.where(r.random(n) < 0.5, 0.0, 0.5)),
             "ret": _returns(r, n), "goal": _goal_rows(r, n)}
        if variant == "kinks":
            # smooth-L1 exactly at |d| = 1 (q1) and at d = 0 (q2) on even rows: done = 1 makes y = reward exactly;
            # goal-loss arguments exactly zero: the whole pose on rows 0 mod 3, the translation (control points 0, 1) on 1 mod 3
            k = idx % 2 == 0
            x["done"][k] = 1.0
            x["reward"][k] = r.integers(0, 1024, k.sum()) / 1024.0
            x["perturb"][k] = 0.0
            x["out9"][k, 0] = x["reward"][k] + np.where(idx[k] % 4 == 0, 1.0, -1.0)
            x["out9"][k, 1] = x["reward"][k]
            full, trans = idx % 3 == 0, idx % 3 == 1
            x["ret"][full | trans] = 0.5
            x["out9"][full, 2:6] = 2.0 ** r.integers(-3, 4, (full.sum(), 1))          # normalises to exactly 0.5 each
            x["goal"][full, :4] = 0.5
            x["out9"][full, 6:9] = np.round(r.uniform(-0.15, 0.15, (full.sum(), 3)) * 1024) / 1024
            x["goal"][full | trans, 4:] = x["out9"][full | trans, 6:9]
        elif variant == "tiny_quat":
            # aux quaternion norm below F.normalize's 1e-12 clamp on rows 0 mod 3: q = x / 1e-12, dq/dx = 1/1e-12
            k = idx % 3 == 0
            x["out9"][k, 2:6] = r.normal(size=(k.sum(), 4)) * 1e-14
            x["ret"][k] = 0.5
        elif variant == "all_perturbed":
            x["perturb"][:] = 1.0
        elif variant == "no_return":
            x["ret"] = np.where(idx % 2 == 0, 0.0, -1.0)
        return x

    def bad(d):
        x = {k: _f32(v).astype(np.float64) for k, v in d.items()}
        y = x["reward"] + (1 - x["done"]) * GAMMA * np.minimum(x["tgt9"][:, 0], x["tgt9"][:, 1])
        dq = np.abs(x["out9"][:, :2] - y[:, None])
        return _near(dq).any(1) | _near(dq, 1.0).any(1) | _near_kink(_goal_args(x["out9"][:, 2:9], x["goal"]))

    return _redraw(draw, bad, B, rng)


CRITIC_CASES = [                   # (name, critic_aux, aux_norm requested)
    ("aux1-norm", 1, True), ("aux0-null", 0, False), ("aux1-null", 1, False), ("aux0-norm", 0, True),
    ("kinks", 1, True), ("tiny_quat", 1, True), ("all_perturbed", 1, True), ("no_return", 1, True)]


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("case,critic_aux,want_norm", CRITIC_CASES, ids=[c[0] for c in CRITIC_CASES])
def test_critic_loss_vs_float64(case, critic_aux, want_norm, B):
    from ga_ddpg_amd import hip
    rng = np.random.default_rng(1000 + B)
    x = _critic_inputs(rng, B, case)
    y, an, g, sc = _nan(B), (_nan(B, 7) if want_norm else None), _nan(B, 9), _nan(4)
    hip.call("gad_critic_loss", _dev(x["out9"]), _dev(x["tgt9"]), _dev(x["reward"]), _dev(x["done"]), _dev(x["perturb"]),
             _dev(x["ret"]), _dev(x["goal"]), B, GAMMA, critic_aux, None, y, an, g, sc)
    r64, r32 = _critic_ref(x, critic_aux, torch.float64), _critic_ref(x, critic_aux, torch.float32)
    _check("y", _host(y), r64["y"], r32["y"])
    if want_norm:
        _check("aux_norm", _host(an), r64["aux_norm"], r32["aux_norm"])
    got_g = _host(g)
    if case == "tiny_quat":           # gradients of 1e12 scale on those rows: each group against its own scale
        tiny = np.zeros(B, bool)
        tiny[::3] = True
        _check("g_out9 (tiny-norm rows)", got_g[tiny], r64["g_out9"][tiny], r32["g_out9"][tiny])
        _check("g_out9 (other rows)", got_g[~tiny], r64["g_out9"][~tiny], r32["g_out9"][~tiny])
    else:
        _check("g_out9", got_g, r64["g_out9"], r32["g_out9"])
    s = _host(sc)
    _check("critic_loss", s[0], r64["scalars"][0], r32["scalars"][0])
    _check("critic_aux_loss", s[1], r64["scalars"][1], r32["scalars"][1])
    assert s[2] == r64["scalars"][2] and s[3] == r64["scalars"][3], (s, r64["scalars"])
    if case == "kinks":               # exact values on the kinks
        k = np.arange(B)[::2]
        inv_k = np.float32(1) / np.float32(s[2])
        assert (got_g[k, 0] == np.where(k % 4 == 0, inv_k, -inv_k)).all() and (got_g[k, 1] == 0).all()
        assert (got_g[::3, 2:] == 0).all(), "pose exactly on the goal: zero gradient (d|x|/dx = 0 at 0)"
    if case == "all_perturbed":
        assert np.isnan(s[0]) and (got_g[:, :2] == 0).all()
    if case == "no_return":
        assert np.isnan(s[1]) and (got_g[:, 2:] == 0).all()


# ----------------------------------------------------------------------------- gad_policy_outputs
POLICY_OUTPUT_CASES = [            # (name, bounds, pitch, saturated means)
    ("sym-p13", None, 13, False), ("asym-p13", "asym", 13, False), ("sym-p7", None, 7, False), ("asym-p7", "asym", 7, False),
    ("asym-p13-saturated", "asym", 13, True), ("sym-p7-saturated", None, 7, True)]
SATURATED = (5.0, 9.0, 12.0, 20.0)


def _policy_head(rng, B, pitch, saturated, tiny=False):
    """raw policy head rows [mean 6 | extra (pitch - 6)]: quaternion + translation in extra[:7] when pitch >= 13"""
    h = np.concatenate([rng.normal(0.0, 0.7, (B, 6)), rng.normal(size=(B, pitch - 6))], 1)
    if pitch >= 13:
        h[:, 10:13] = rng.uniform(-0.15, 0.15, (B, 3))
    if saturated:                  # |mean| in {5, 9, 12, 20} on a third of the entries
        s = rng.random((B, 6)) < 1 / 3
        h[:, :6] = np.where(s, rng.choice(SATURATED, (B, 6)) * rng.choice((-1.0, 1.0), (B, 6)), h[:, :6])
    return h


def _pi_ref(head, scale, bias, dtype):
    m = _T(head[:, :6], dtype)
    pi = torch.tanh(m) * _T(scale, dtype)
    return pi + _T(bias, dtype) if bias is not None else pi


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("case,bounds,pitch,saturated", POLICY_OUTPUT_CASES, ids=[c[0] for c in POLICY_OUTPUT_CASES])
def test_policy_outputs_vs_float64(case, bounds, pitch, saturated, B):
    from ga_ddpg_amd import hip
    from oracle import ref_step
    rng = np.random.default_rng(2000 + B)
    scale, bias = _space(bounds)
    head = _f32(_policy_head(rng, B, pitch, saturated))
    pi, aux = _nan(B, 6), (_nan(B, 7) if pitch >= 13 else None)
    hip.call("gad_policy_outputs", _dev(head), B, pitch, _dev(scale), None if bias is None else _dev(bias), pi, aux)
    r = {dt: _np(_pi_ref(head, scale, bias, dt)) for dt in (torch.float64, torch.float32)}
    _check("pi", _host(pi), r[torch.float64], r[torch.float32])
    if aux is not None:
        a = {dt: _np(ref_step._unit_quat_head(_T(head[:, 6:13], dt))) for dt in (torch.float64, torch.float32)}
        _check("aux_norm", _host(aux), a[torch.float64], a[torch.float32])


# ----------------------------------------------------------------------------- gad_actor_loss
def _actor_ref(x, pitch, bc_scale, policy_aux, scale, bias, dtype):
    """core/ddpg.py:169-177, core/bc.py:71-87, core/loss.py in `dtype`.  The BC loss is evaluated on the pi handed to the
    kernel (its input), the chain into the raw means through pi = tanh(mean) * scale + bias"""
    from oracle import ref_step
    o = _T(x["head"], dtype).requires_grad_(True)
    pi_in = _T(x["pi"], dtype).requires_grad_(True)
    em = torch.from_numpy(x["expert_flag"] >= 1)
    gm = torch.from_numpy(x["ret"] > 0)
    bc = ref_step.pose_bc_loss(pi_in[em], _T(x["expert_action"], dtype)[em]) * bc_scale
    pa = torch.zeros((), dtype=dtype)
    if policy_aux:
        pa = ref_step.goal_pred_loss(ref_step._unit_quat_head(o[:, 6:13])[gm], _T(x["goal"], dtype)[gm])
    (bc + pa).backward()
    gpi = pi_in.grad if pi_in.grad is not None else torch.zeros_like(pi_in)
    if x.get("gpc") is not None:
        gpi = gpi + _T(x["gpc"], dtype)
    pi_model = torch.tanh(o[:, :6]) * _T(scale, dtype) + (_T(bias, dtype) if bias is not None else 0.0)
    pi_model.backward(gpi)
    return {"g_pol": _np(o.grad), "scalars": np.array([float(bc), float(pa), float(em.sum()), float(gm.sum())])}


ACTOR_CASES = [                    # (name, bounds, pitch, policy_aux, g_pi_critic, rows)
    ("sym-p13-aux-gpc", None, 13, 1, True, "mixed"), ("asym-p13-aux-gpc", "asym", 13, 1, True, "mixed"),
    ("asym-p7-nogpc", "asym", 7, 0, False, "mixed"), ("sym-p7-gpc", None, 7, 0, True, "mixed"),
    ("asym-p13-noaux", "asym", 13, 0, True, "mixed"), ("asym-p16-aux", "asym", 16, 1, True, "mixed"),
    ("asym-saturated", "asym", 13, 1, True, "saturated"), ("sym-saturated-nogpc", None, 13, 1, False, "saturated"),
    ("asym-no-expert", "asym", 13, 1, True, "no_expert"), ("asym-all-expert-nogpc", "asym", 13, 1, False, "all_expert"),
    ("asym-no-return", "asym", 13, 1, True, "no_return"), ("asym-kinks", "asym", 13, 1, True, "kinks"),
    ("sym-kinks-p7", None, 7, 0, False, "kinks")]
BC_SCALE = 0.7


def _actor_inputs(rng, B, pitch, rows, scale, bias, with_gpc):
    lo, hi = (-scale if bias is None else bias - scale), (scale if bias is None else bias + scale)

    def draw(r, idx):
        n = len(idx)
        x = {"head": _policy_head(r, n, pitch, rows == "saturated"), "expert_action": r.uniform(lo, hi, (n, 6)),
             "expert_flag": np.where(r.random(n) < 0.6, 1.0, np.where(r.random(n) < 0.5, 0.0, 0.999)),
             "ret": _returns(r, n), "goal": _goal_rows(r, n)}
        if rows == "no_expert":
            x["expert_flag"][:] = np.where(idx % 2 == 0, 0.0, 0.5)
        elif rows == "all_expert":
            x["expert_flag"][:] = np.where(idx % 2 == 0, 1.0, 3.0)
        elif rows == "no_return":
            x["ret"][:] = 0.0
        elif rows == "kinks" and pitch >= 13:
            full, trans = idx % 3 == 0, idx % 3 == 1          # goal-loss arguments exactly zero (see the critic's kinks)
            x["ret"][full | trans] = 0.5
            x["head"][full, 6:10] = 2.0 ** r.integers(-3, 4, (full.sum(), 1))
            x["goal"][full, :4] = 0.5
            x["head"][full, 10:13] = np.round(r.uniform(-0.15, 0.15, (full.sum(), 3)) * 1024) / 1024
            x["goal"][full | trans, 4:] = x["head"][full | trans, 10:13]
        if rows == "kinks":                                  # BC arguments exactly zero: set from the kernel's pi below
            x["expert_flag"][idx % 4 < 2] = 1.0
        return x

    def bad(d):
        h = _f32(d["head"]).astype(np.float64)
        pi = np.tanh(h[:, :6]) * scale + (0.0 if bias is None else bias)
        out = _near_kink(_bc_args(pi, d["expert_action"]))
        if pitch >= 13:
            out |= _near_kink(_goal_args(h[:, 6:13], d["goal"]))
        return out

    x = _redraw(draw, bad, B, rng)
    x["gpc"] = (_f32(rng.normal(size=(B, 6)) * 0.1 / B).astype(np.float64)) if with_gpc else None
    return x


def _actor_call(x, B, pitch, policy_aux, scale_d, inv_n, g, sc):
    from ga_ddpg_amd import hip
    hip.call("gad_actor_loss", _dev(x["head"]), _dev(x["pi"]), _dev(x["expert_action"]), _dev(x["expert_flag"]),
             _dev(x["ret"]), _dev(x["goal"]), B, pitch, BC_SCALE, policy_aux, scale_d,
             None if x["gpc"] is None else torch.from_numpy(x["gpc"]).cuda(), inv_n, g, sc)


def _kernel_pi(x, B, pitch, scale, bias):
    from ga_ddpg_amd import hip
    pi = _nan(B, 6)
    hip.call("gad_policy_outputs", _dev(x["head"]), B, pitch, _dev(scale), None if bias is None else _dev(bias), pi, None)
    return _f32(_host(pi))


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("case,bounds,pitch,policy_aux,with_gpc,rows", ACTOR_CASES, ids=[c[0] for c in ACTOR_CASES])
def test_actor_loss_vs_float64(case, bounds, pitch, policy_aux, with_gpc, rows, B):
    rng = np.random.default_rng(3000 + B)
    scale, bias = _space(bounds)
    x = _actor_inputs(rng, B, pitch, rows, scale, bias, with_gpc)
    x["pi"] = _kernel_pi(x, B, pitch, scale, bias)
    if rows == "kinks":            # the whole pose on rows 0 mod 4, the translation (control points 0, 1) on 1 mod 4
        k = np.arange(B)
        x["expert_action"][k % 4 == 0] = x["pi"][k % 4 == 0]
        x["expert_action"][k % 4 == 1, :3] = x["pi"][k % 4 == 1, :3]
    g, sc = _nan(B, pitch), _nan(4)
    _actor_call(x, B, pitch, policy_aux, _dev(scale), None, g, sc)
    r64 = _actor_ref(x, pitch, BC_SCALE, policy_aux, scale, bias, torch.float64)
    r32 = _actor_ref(x, pitch, BC_SCALE, policy_aux, scale, bias, torch.float32)
    got, s = _host(g), _host(sc)
    _check("g_pol mean columns", got[:, :6], r64["g_pol"][:, :6], r32["g_pol"][:, :6])
    _check("g_pol extra columns", got[:, 6:], r64["g_pol"][:, 6:], r32["g_pol"][:, 6:])
    _check("bc_loss", s[0], r64["scalars"][0], r32["scalars"][0])
    _check("policy_aux_loss", s[1], r64["scalars"][1], r32["scalars"][1])
    assert s[2] == r64["scalars"][2] and s[3] == r64["scalars"][3], (s, r64["scalars"])
    if not policy_aux or pitch > 13:
        assert (got[:, 13 if policy_aux else 6:] == 0).all(), "columns without a loss term: zero gradient"
    if rows == "kinks" and pitch >= 13:
        assert (got[::3, 6:13] == 0).all(), "pose exactly on the goal: zero gradient"
    if rows == "kinks" and x["gpc"] is None:
        assert (got[::4, :6] == 0).all(), "pi exactly on the expert action: zero gradient"


# ----------------------------------------------------------------------------- gad_actor_critic_loss
def _ac_ref(x, ratio, dtype):
    o = _T(x["out9"], dtype).requires_grad_(True)
    keep = torch.from_numpy(~((x["expert_flag"] >= 1) & (x["ret"] > 0)))
    loss = -ratio * torch.min(o[:, 0][keep], o[:, 1][keep]).mean()
    loss.backward()
    return {"g_out9": _np(o.grad), "scalars": np.array([float(loss), float(keep.sum())])}


AC_CASES = ("mixed", "ties", "none_kept", "all_kept")
RATIO = float(np.float32(0.3))


def _ac_inputs(rng, B, case):
    x = {"out9": rng.uniform(0.5, 2.0, (B, 9)), "expert_flag": np.where(rng.random(B) < 0.5, 1.0, 0.0),
         "ret": _returns(rng, B)}
    if case == "ties":             # q1 == q2 exactly: torch.min sends half the gradient to each
        x["out9"][::2, 1] = x["out9"][::2, 0]
    elif case == "none_kept":
        x["expert_flag"][:], x["ret"][:] = 1.0, 0.5
    elif case == "all_kept":
        x["expert_flag"][:] = np.where(np.arange(B) % 2 == 0, 0.0, 1.0)
        x["ret"][:] = np.where(np.arange(B) % 2 == 0, 0.5, 0.0)
    return {k: _f32(v) for k, v in x.items()}


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("case", AC_CASES)
def test_actor_critic_loss_vs_float64(case, B):
    from ga_ddpg_amd import hip
    rng = np.random.default_rng(4000 + B)
    x = _ac_inputs(rng, B, case)
    g, sc = _nan(B, 9), _nan(2)
    hip.call("gad_actor_critic_loss", _dev(x["out9"]), _dev(x["expert_flag"]), _dev(x["ret"]), B, RATIO, None, g, sc)
    r64, r32 = _ac_ref(x, RATIO, torch.float64), _ac_ref(x, RATIO, torch.float32)
    got, s = _host(g), _host(sc)
    _check("g_out9", got, r64["g_out9"], r32["g_out9"])
    _check("actor_critic_loss", s[0], r64["scalars"][0], r32["scalars"][0])
    assert s[1] == r64["scalars"][1]
    assert (got[:, 2:] == 0).all()
    if case == "ties":
        keep = ~((x["expert_flag"] >= 1) & (x["ret"] > 0))
        t = np.zeros(B, bool)
        t[::2] = True
        assert (got[t & keep, 0] == got[t & keep, 1]).all() and (got[t & keep, 0] != 0).all()
    if case == "none_kept":
        assert np.isnan(s[0]) and s[1] == 0 and (got == 0).all()


# ----------------------------------------------------------------------------- gad_policy_sample
SAMPLE_CASES = [                   # (name, squash, extra_dim, eps, bounds ("none": scale and bias NULL), rows, pitch pad)
    ("squash-e7-asym", 1, 7, True, "asym", "mixed", 0), ("squash-e1-sym", 1, 1, True, None, "mixed", 0),
    ("squash-e0-null-bounds", 1, 0, True, "none", "mixed", 0), ("squash-e7-noeps", 1, 7, False, "asym", "mixed", 3),
    ("plain-e7", 0, 7, True, "none", "mixed", 0), ("plain-e1-noeps", 0, 1, False, "none", "mixed", 2),
    ("squash-e7-clamp", 1, 7, True, "asym", "clamp", 0), ("plain-e0-clamp-noeps", 0, 0, False, "none", "clamp", 0),
    ("squash-e1-saturated", 1, 1, True, "asym", "saturated", 0), ("squash-e0-saturated-sym", 1, 0, True, None, "saturated", 0)]
CLAMP_VALUES = (-10.0, 2.0, -15.0, 5.0, -10.5, 2.5)


def _sample_ref(head, eps, extra_dim, scale, bias, squash, dtype):
    """GaussianPolicy.forward + sample (core/networks.py:339-371; oracle/ref_step.py PolicyNet.sample) on the raw head"""
    from oracle import ref_step
    h = _T(head, dtype)
    mean, extra, ls = h[:, :6], h[:, 6:6 + extra_dim], h[:, 6 + extra_dim:12 + extra_dim]
    log_std = torch.clamp(ls, min=-10, max=2)
    std = log_std.exp()
    e = _T(eps, dtype) if eps is not None else torch.zeros_like(mean)
    x = mean + std * e
    sc = _T(scale, dtype) if scale is not None else 1.0
    bi = _T(bias, dtype) if bias is not None else 0.0
    if squash:
        y = torch.tanh(x)
        action, mean_sq = y * sc + bi, torch.tanh(mean) * sc + bi
    else:
        y, action, mean_sq = x, x, mean
    lp = -((x - mean) ** 2) / (2 * std ** 2) - log_std - np.log(np.sqrt(2 * np.pi))
    lp = (lp - torch.log(sc * (1 - y.pow(2)) + 1e-6)).sum(1)
    if extra_dim == 7:
        extra = ref_step._unit_quat_head(extra)
    return {"mean_sq": _np(mean_sq), "log_std": _np(log_std), "log_prob": _np(lp), "action": _np(action), "extra": _np(extra)}


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("case,squash,extra_dim,with_eps,bounds,rows,pad", SAMPLE_CASES, ids=[c[0] for c in SAMPLE_CASES])
def test_policy_sample_vs_float64(case, squash, extra_dim, with_eps, bounds, rows, pad, B):
    from ga_ddpg_amd import hip
    rng = np.random.default_rng(5000 + B)
    scale, bias = (None, None) if bounds == "none" else _space(bounds)
    pitch = 12 + extra_dim + pad
    head = rng.normal(size=(B, pitch))
    if squash:                     # |x| <= 3: 1 - tanh(x)^2 >= 1e-2, where float32 evaluates log(scale * (1 - y^2) + 1e-6) well
        head[:, :6] = rng.normal(0.0, 0.8, (B, 6)).clip(-1.5, 1.5)
        head[:, 6 + extra_dim:12 + extra_dim] = rng.uniform(-2.0, 0.0, (B, 6))
        eps = rng.normal(size=(B, 6)).clip(-1.5, 1.5)
    else:                          # unsquashed: keep |x| < 1, where log(1 - x^2 + 1e-6) is defined
        head[:, :6] = rng.uniform(-0.4, 0.4, (B, 6))
        head[:, 6 + extra_dim:12 + extra_dim] = rng.uniform(-4.0, np.log(0.15), (B, 6))
        eps = rng.uniform(-2.5, 2.5, (B, 6))
    if extra_dim == 7:
        head[:, 10:13] = rng.uniform(-0.15, 0.15, (B, 3))
    if rows == "clamp":            # log_std exactly on the clamp bounds -10 / 2 and beyond them
        head[:, 6 + extra_dim:12 + extra_dim] = rng.choice(CLAMP_VALUES, (B, 6))
        eps = eps.clip(-0.2, 0.2)  # std up to e^2: |x| stays <= 3
    elif rows == "saturated":      # |x| >= 15: y = tanh(x) = +-1 exactly in float32, log(scale * 0 + 1e-6)
        s = rng.random((B, 6)) < 0.5
        head[:, :6] = np.where(s, rng.choice((16.0, 20.0), (B, 6)) * rng.choice((-1.0, 1.0), (B, 6)), head[:, :6])
        head[:, 6 + extra_dim:12 + extra_dim] = np.where(s, rng.uniform(-3.0, 0.0, (B, 6)), head[:, 6 + extra_dim:12 + extra_dim])
        eps = eps.clip(-1, 1)
    head, eps = _f32(head), (_f32(eps) if with_eps else None)
    outs = {"mean_sq": _nan(B, 6), "log_std": _nan(B, 6), "log_prob": _nan(B), "action": _nan(B, 6),
            "extra": _nan(B, extra_dim) if extra_dim else None}
    hip.call("gad_policy_sample", _dev(head), B, pitch, extra_dim, None if eps is None else _dev(eps),
             None if scale is None else _dev(scale), None if bias is None else _dev(bias), squash,
             outs["mean_sq"], outs["log_std"], outs["log_prob"], outs["action"], outs["extra"])
    r64 = _sample_ref(head, eps, extra_dim, scale, bias, squash, torch.float64)
    r32 = _sample_ref(head, eps, extra_dim, scale, bias, squash, torch.float32)
    for k, t in outs.items():
        if t is not None:
            _check(k, _host(t), r64[k], r32[k])
    if rows == "clamp":
        assert (_host(outs["log_std"]) == np.clip(head[:, 6 + extra_dim:12 + extra_dim], -10, 2)).all()


# ----------------------------------------------------------------------------- gad_mask_counts
@pytest.mark.parametrize("B", BS)
def test_mask_counts_exact(B):
    from ga_ddpg_amd import hip
    rng = np.random.default_rng(6000 + B)
    ret = _f32(rng.choice((0.0, -0.0, 1e-30, 0.5, -0.5, 1.0), B))
    expert = _f32(rng.choice((1.0, 0.99999994, 0.0, 2.0, 0.5), B))
    perturb = _f32(rng.choice((1.0, 0.99999994, 0.0, 1.5, 0.25), B))
    out = _nan(4, dtype=torch.float64)
    hip.call("gad_mask_counts", _dev(ret), _dev(expert), _dev(perturb), B, out)
    reward, exp = ret > 0, expert >= 1
    want = np.array([(perturb < 1).sum(), reward.sum(), exp.sum(), (~(reward & exp)).sum()], dtype=np.float64)
    np.testing.assert_array_equal(_host(out), want)


# ----------------------------------------------------------------------------- gad_target_noise
NOISE_CASES = [                    # (name, normal, level)
    ("uniform-0.03", 0, 0.03),     # (u*3-6)*level <= -0.09: every translation entry on the -0.01 clamp
    ("uniform-0.002", 0, 0.002),   # [-0.012, -0.006): the clamp at u < 1/3 only
    ("normal-0.02", 1, 0.02)]      # u*level/2: u = +-1 lands exactly on +-0.01, |u| > 1 beyond it


def _noise_ref(pi, u, level, normal, dtype):
    from oracle import ref_step
    uu = _T(u, dtype)
    if normal:
        d = uu * level / 2.0
        d[:, 3:] *= 5
    else:
        d = ref_step.target_noise(uu.clone(), level)
    d[:, :3] = torch.clamp(d[:, :3], -0.01, 0.01)
    return _np(_T(pi, dtype) + d)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("case,normal,level", NOISE_CASES, ids=[c[0] for c in NOISE_CASES])
def test_target_noise_vs_float64(case, normal, level, B):
    from ga_ddpg_amd import hip
    rng = np.random.default_rng(7000 + B)
    level = float(np.float32(level))
    pi = _f32(rng.normal(size=(B, 6)) * 0.03)
    if normal:
        u = rng.normal(size=(B, 6))
        u[:, :3] = np.where(rng.random((B, 3)) < 0.3, rng.choice((-1.0, 1.0, -3.0, 3.0), (B, 3)), u[:, :3])
    else:
        u = rng.random((B, 6))
    u = _f32(u)
    out = _nan(B, 6)
    hip.call("gad_target_noise", _dev(pi), _dev(u), B, level, normal, out)
    _check("target action", _host(out), _noise_ref(pi, u, level, normal, torch.float64), _noise_ref(pi, u, level, normal, torch.float32))
    d = _host(out)[:, :3] - pi[:, :3].astype(np.float64)
    assert np.abs(d).max() <= 0.0100001


# ----------------------------------------------------------------------------- data-parallel composition
SPLITS = [(257, 743), (300, 64, 636)]   # rows 300:364 hold no kept, goal or expert row: an empty-mask shard of the 3-way split


def _bounds(sizes):
    e = np.cumsum(sizes)
    return [(int(b - n), int(b)) for n, b in zip(sizes, e)]


@pytest.mark.parametrize("sizes", SPLITS, ids=["2-shards", "3-shards"])
def test_sharded_losses_compose_to_the_full_batch(sizes):
    """The data-parallel path (ga_ddpg_amd/parallel.py) runs each loss kernel on its shard with the GLOBAL inverse counts
    (inverse_counts layout: critic at +0, actor at +2, actor-critic at +4) and all-reduces the gradients' consumers and the
    scalars: the concatenated shard gradients must be the single full-batch call's, the summed shard scalars its losses --
    and both the float64 reference's"""
    from ga_ddpg_amd import hip, parallel
    B = sum(sizes)
    rng = np.random.default_rng(8000 + len(sizes))
    xc = _critic_inputs(rng, B, "mixed")
    scale, bias = _space("asym")
    xa = _actor_inputs(rng, B, 13, "mixed", scale, bias, True)
    xa["pi"] = _kernel_pi(xa, B, 13, scale, bias)
    xa["ret"] = xc["ret"]
    xq = _ac_inputs(rng, B, "mixed")
    xq["ret"], xq["expert_flag"] = xc["ret"], xa["expert_flag"]
    for x in (xc, xa, xq):         # the empty-mask rows
        x["ret"][300:364] = 0.0
    xc["perturb"][300:364] = 1.0
    xa["expert_flag"][300:364] = 0.0
    xq["expert_flag"][300:364] = 0.0
    batch = {"return_batch": xc["ret"], "expert_flag_batch": xa["expert_flag"], "perturb_flag_batch": xc["perturb"]}
    shards = _bounds(sizes)
    counts = sum(parallel.mask_counts({k: v[a:b] for k, v in batch.items()}) for a, b in shards)
    np.testing.assert_array_equal(counts, parallel.mask_counts(batch))
    inv = _dev(parallel.inverse_counts(counts))
    dev = {"c": {k: _dev(v) for k, v in xc.items()}, "a": {k: (_dev(v) if v is not None else None) for k, v in xa.items()},
           "q": {k: _dev(v) for k, v in xq.items()}}
    gpc = torch.from_numpy(xa["gpc"]).cuda()
    scale_d = _dev(scale)

    def run(a, b, inv_c, inv_a, inv_q):
        n = b - a
        c, ac, q = dev["c"], dev["a"], dev["q"]
        y, an, g9, s1 = _nan(n), _nan(n, 7), _nan(n, 9), _nan(4)
        hip.call("gad_critic_loss", c["out9"][a:b], c["tgt9"][a:b], c["reward"][a:b], c["done"][a:b], c["perturb"][a:b],
                 c["ret"][a:b], c["goal"][a:b], n, GAMMA, 1, inv_c, y, an, g9, s1)
        g13, s2 = _nan(n, 13), _nan(4)
        hip.call("gad_actor_loss", ac["head"][a:b], ac["pi"][a:b], ac["expert_action"][a:b], ac["expert_flag"][a:b],
                 ac["ret"][a:b], ac["goal"][a:b], n, 13, BC_SCALE, 1, scale_d, gpc[a:b], inv_a, g13, s2)
        gq, s3 = _nan(n, 9), _nan(2)
        hip.call("gad_actor_critic_loss", q["out9"][a:b], q["expert_flag"][a:b], q["ret"][a:b], n, RATIO, inv_q, gq, s3)
        return [_host(t) for t in (y, an, g9, g13, gq)], [_host(t) for t in (s1, s2, s3)]

    full, full_s = run(0, B, None, None, None)
    parts = [run(a, b, inv[0:], inv[2:], inv[4:]) for a, b in shards]
    names = ("y", "aux_norm", "critic g_out9", "actor g_pol", "actor-critic g_out9")
    for i, what in enumerate(names):
        cat = np.concatenate([p[0][i] for p in parts])
        assert not np.isnan(cat).any(), what
        np.testing.assert_allclose(cat, full[i], rtol=0, atol=1e-6 * np.abs(full[i]).max(), err_msg=what)
    for j, k, what in ((0, 0, "critic_loss"), (0, 1, "critic_aux_loss"), (1, 0, "bc_loss"), (1, 1, "policy_aux_loss"),
                       (2, 0, "actor_critic_loss")):
        tot = sum(p[1][j][k] for p in parts)
        assert abs(tot - full_s[j][k]) <= 4e-6 * abs(full_s[j][k]), (what, tot, full_s[j][k])
    # ... and the float64 reference
    rc64, rc32 = _critic_ref(xc, 1, torch.float64), _critic_ref(xc, 1, torch.float32)
    ra64 = _actor_ref(xa, 13, BC_SCALE, 1, scale, bias, torch.float64)
    ra32 = _actor_ref(xa, 13, BC_SCALE, 1, scale, bias, torch.float32)
    rq64, rq32 = _ac_ref(xq, RATIO, torch.float64), _ac_ref(xq, RATIO, torch.float32)
    cat = [np.concatenate([p[0][i] for p in parts]) for i in range(5)]
    _check("sharded critic g_out9", cat[2], rc64["g_out9"], rc32["g_out9"])
    _check("sharded actor g_pol", cat[3], ra64["g_pol"], ra32["g_pol"])
    _check("sharded actor-critic g_out9", cat[4], rq64["g_out9"], rq32["g_out9"])
    for j, k, r64, r32 in ((0, 0, rc64, rc32), (0, 1, rc64, rc32), (1, 0, ra64, ra32), (1, 1, ra64, ra32), (2, 0, rq64, rq32)):
        _check("summed shard scalar %d.%d" % (j, k), sum(p[1][j][k] for p in parts), r64["scalars"][k], r32["scalars"][k])
