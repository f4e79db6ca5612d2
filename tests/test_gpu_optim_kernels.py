"""The optimiser / bookkeeping kernels of ga-ddpg_amd/csrc/optim.hip (include/gaddpg.h sections E, F, G) and the two BatchNorm
bookkeeping entry points, called directly and compared with the plain references of tests/optim_reference.py.

Yardsticks.  Copies, conversions, selections, maxima and counters: bit-exact.  Sums of squares: a derived bound
(optim_reference.sumsq_bound).  Adam / target / BatchNorm arithmetic: the head-loss criterion, err <= max(3 x the float32
reference's own error, 1e-6) in max-norm against the float64 reference -- per step, each step starting from the state the
kernel left, so the reference sees exactly the float32 inputs the kernel saw.  gad_optim_jobs against the single-purpose entry
points: bit-identical.

Every buffer lives inside a byte arena filled with 0xA5 with 64 guard bytes on both sides that must come back untouched; pure
outputs start as NaN.  All inputs come from seeded generators; nothing is skipped or filtered at run time.

What these tests found when they were written (all fixed; the cases stay): 1 - beta formed in float32 from the rounded beta
(exp_avg_sq 4e-6 ... 1.29e-5 off float64, 31 ... 3400 x the float32 reference's error; now equal to it, at most 1.1e-7); gad_polyak
and the job kernel contracting the soft update into different fused multiply-adds (1 ulp apart on 5 - 27 % of the elements); the
job kernel writing grad_scale into .grad although nothing clips; the absmax paths dropping a NaN and counting the gradient
of elements that have none.  A note for whoever mutates the kernel: in optim_jobs_kernel's merged 16-byte stores a lane whose
write flag is off holds the value it loaded, so "store o.g for every lane" changes nothing; storing only when all four lanes
are flagged, dropping the scalar tail, the mirror write, the hard_enable test or the counter guard does fail here."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import optim_reference as R

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099, (1 << 20) | 3)
GUARD = 64                      # bytes
FILL = 0xA5
MAX_JOBS, SLOTS = 4, 8          # GAD_MAX_OPTIM_JOBS, GAD_ABSMAX_SLOTS
ERR_NULL, ERR_SHAPE = -1, -2
SPECIAL64 = [1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, -(1.0 + 2.0 ** -24) - 2.0 ** -60, 1e39, -1e39, 3.4028235677973366e38,
             1e-40, 2.0 ** -150, 2.0 ** -149 * 1.5, -0.0, 0.0, -2.0 ** -126]


def _hip():
    from ga_ddpg_amd import hip
    return hip


# ----------------------------------------------------------------------------- plumbing
class Buf(object):
    """a device buffer holding `a` (numpy, any dtype) between two guard zones"""

    def __init__(self, a, shift=0):
        a = np.ascontiguousarray(a)
        self.dtype, self.shape, self.nbytes, self.shift = a.dtype, a.shape, a.nbytes, shift
        raw = np.full(GUARD + shift + a.nbytes + GUARD, FILL, np.uint8)
        raw[GUARD + shift:GUARD + shift + a.nbytes] = a.view(np.uint8).ravel()
        self.t = torch.from_numpy(raw).cuda()
        assert self.t.data_ptr() % 256 == 0
        self.ptr = _hip().Ptr(self.t.data_ptr() + GUARD + shift)

    def get(self, what="buffer"):
        torch.cuda.synchronize()
        raw = self.t.cpu().numpy()
        lo, hi = raw[:GUARD + self.shift], raw[GUARD + self.shift + self.nbytes:]
        assert (lo == FILL).all() and (hi == FILL).all(), "%s: guard bytes written" % what
        return raw[GUARD + self.shift:GUARD + self.shift + self.nbytes].copy().view(self.dtype).reshape(self.shape)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), "%s: %d of %d elements differ bitwise; first at %d: got %r want %r" % (
        what, int(bad.sum()), bad.size, int(np.flatnonzero(bad.ravel())[0]), got.ravel()[np.flatnonzero(bad.ravel())[0]],
        want.ravel()[np.flatnonzero(bad.ravel())[0]])


def _nan32(n):
    return np.full(n, np.nan, np.float32)


def _pattern32(n):
    """what an untouched float32 element of an arena looks like"""
    return np.full(4 * n, FILL, np.uint8).view(np.float32)


def _arena(rng, m2p, packed_n, special=True):
    """float64 gradient arena; the special values sit where the first master elements point"""
    ga = rng.normal(size=packed_n) * 10.0 ** rng.uniform(-6, 2, packed_n)
    if special:
        live = np.flatnonzero(m2p >= 0)[:len(SPECIAL64)]
        ga[m2p[live]] = SPECIAL64[:len(live)]
    return ga


@pytest.fixture(scope="module")
def optimisers():
    """hyper-parameters of the four optimisers, clip_grad and tau, as the agent holds them"""
    from ga_ddpg_amd.api import make_agent
    agent, cfg = make_agent("ddpg_td3_aux.yaml")
    out = {}
    for name, opt in (("policy", agent.policy_optim), ("critic", agent.critic_optim),
                      ("encoder", agent.state_feat_encoder_optim), ("val_encoder", agent.state_feat_val_encoder_optim)):
        g = opt.param_groups[0]
        assert not g.get("amsgrad", False) and not g.get("maximize", False)
        out[name] = {"lr": float(g["lr"]), "betas": tuple(float(b) for b in g["betas"]), "eps": float(g["eps"]),
                     "weight_decay": float(g["weight_decay"])}
        assert out[name]["betas"] == R.BETAS
    out["clip_grad"], out["tau"] = float(agent.clip_grad), float(agent.tau)
    del agent
    torch.cuda.synchronize()
    return out


# ----------------------------------------------------------------------------- 1. arena conversion, pack
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("accumulate", (0, 1))
def test_grad_from_arena_bit_exact(n, accumulate):
    hip = _hip()
    rng = np.random.default_rng(100 + n + accumulate)
    m2p, pn = R.injection(rng, n)
    k = min(n, len(SPECIAL64))                                                # the special values are all read: m2p[:k] >= 0
    free = np.setdiff1d(np.arange(pn), m2p[m2p >= 0])
    lost = np.flatnonzero(m2p[:k] < 0)
    m2p[lost] = free[:len(lost)]
    ga = _arena(rng, m2p, pn)
    g0 = (rng.normal(size=n) * 1e-3).astype(np.float32) if accumulate else _nan32(n)
    want = R.grad_from_arena(ga, m2p, g0, accumulate)
    assert (want[m2p < 0] == (g0[m2p < 0] if accumulate else 0)).all() and (n < 5 or np.isinf(want).any())
    bga, bm = Buf(ga), Buf(m2p)
    bg = Buf(g0)
    hip.call("gad_grad_from_arena", bga.ptr, bm.ptr, n, bg.ptr, accumulate)
    _same("grad_from_arena", bg.get(), want)
    # + the sum of squares (finite arena: an overflowed element makes the sum inf, asserted separately)
    bg2, ss = Buf(g0), Buf(np.array([0.75]))
    hip.call("gad_grad_from_arena_sumsq", bga.ptr, bm.ptr, n, bg2.ptr, accumulate, ss.ptr)
    _same("grad_from_arena_sumsq: grad", bg2.get(), want)
    if np.isinf(want).any():
        assert ss.get()[0] == np.inf
    else:
        ex = R.sumsq_exact(want)
        assert abs(float(ss.get()[0]) - (ex + 0.75)) <= R.sumsq_bound(n + 1, ex + 0.75)
    ga_f = np.where(np.abs(ga) > 1e38, 1e19, ga)
    want_f = R.grad_from_arena(ga_f, m2p, g0, accumulate)
    bga_f, bg3, ss3 = Buf(ga_f), Buf(g0), Buf(np.array([0.75]))
    hip.call("gad_grad_from_arena_sumsq", bga_f.ptr, bm.ptr, n, bg3.ptr, accumulate, ss3.ptr)
    _same("grad_from_arena_sumsq (finite): grad", bg3.get(), want_f)
    exact = R.sumsq_exact(want_f)
    got = float(ss3.get()[0])
    print("n %d sumsq err %.3e bound %.3e" % (n, abs(got - 0.75 - exact), R.sumsq_bound(n + 1, exact + 0.75)))
    assert abs(got - (exact + 0.75)) <= R.sumsq_bound(n + 1, exact + 0.75)
    for b in (bga, bm, bga_f):
        b.get("input")


@pytest.mark.parametrize("n", SIZES)
def test_pack_params_bit_exact(n):
    hip = _hip()
    rng = np.random.default_rng(200 + n)
    m2p, pn = R.injection(rng, n)
    p = rng.normal(size=n).astype(np.float32)
    p[:min(n, 4)] = np.array([-0.0, 1e-40, np.inf, -1e-45], np.float32)[:min(n, 4)]
    want = _pattern32(pn)
    want[m2p[m2p >= 0]] = p[m2p >= 0]
    bp, bm, bk = Buf(p), Buf(m2p), Buf(_pattern32(pn))
    hip.call("gad_pack_params", bp.ptr, bm.ptr, n, bk.ptr)
    _same("pack_params", bk.get(), want)                                      # slots no master element maps to: untouched
    _same("pack_params: p", bp.get(), p)


# ----------------------------------------------------------------------------- 2. / 3. sums of squares
def _sumsq_grads(rng, n, kind):
    if kind == "zero":
        return np.zeros(n, np.float32)
    if kind == "range":                                                       # squares over 1e30
        return (rng.normal(size=n) * 10.0 ** rng.uniform(-7.5, 7.5, n)).astype(np.float32)
    return (rng.normal(size=n) * 0.01).astype(np.float32)


@pytest.mark.parametrize("n", SIZES + (512 * 2048 + 5,))                      # the last one: above gad_sumsq's 512 workgroups x 2048
@pytest.mark.parametrize("kind", ("normal", "range", "zero"))
def test_sumsq_within_derived_bound(n, kind):
    """The kernel adds exact float64 squares (a float32 square has 48 significant bits) with round-to-nearest adds -- per
    thread, across the wavefront, across the four wavefronts, then one atomic add into *out: n adds in some order, hence
    |got - exact| <= n * 2**-52 * exact (optim_reference.sumsq_bound, checked on the CPU for several orders)."""
    hip = _hip()
    rng = np.random.default_rng(300 + n)
    g = _sumsq_grads(rng, n, kind)
    exact = R.sumsq_exact(g)
    for start in (0.0, 3.25):                                                 # "atomically accumulated": a non-zero *out is added to
        bg, out = Buf(g), Buf(np.array([start]))
        hip.call("gad_sumsq", bg.ptr, n, out.ptr)
        got = float(out.get()[0])
        assert abs(got - (exact + start)) <= R.sumsq_bound(n + 1, exact + start), (n, kind, start, got, exact)
        if kind == "zero":
            assert got == start
        _same("sumsq: grad", bg.get(), g)


def test_sumsq_deterministic_mode():
    """both sum-of-squares entry points in the deterministic mode: the same bound, bit-equal over three calls and on a
    second stream"""
    hip = _hip()
    rng = np.random.default_rng(301)
    hip.set_option("deterministic", 1)
    try:
        for n in (4099, (1 << 20) | 3, 512 * 2048 + 5):
            g = _sumsq_grads(rng, n, "range")
            m2p, pn = R.injection(rng, n)
            ga = _arena(rng, m2p, pn, special=False)
            gw = R.grad_from_arena(ga, m2p)
            bg, bga, bm = Buf(g), Buf(ga), Buf(m2p)
            side = torch.cuda.Stream()
            res = {"sumsq": [], "arena": []}
            for k in range(4):
                o1, o2, bgr = Buf(np.array([0.0])), Buf(np.array([0.0])), Buf(_nan32(n))
                torch.cuda.synchronize()
                if k == 3:
                    with torch.cuda.stream(side):
                        hip.call("gad_sumsq", bg.ptr, n, o1.ptr)
                        hip.call("gad_grad_from_arena_sumsq", bga.ptr, bm.ptr, n, bgr.ptr, 0, o2.ptr)
                else:
                    hip.call("gad_sumsq", bg.ptr, n, o1.ptr)
                    hip.call("gad_grad_from_arena_sumsq", bga.ptr, bm.ptr, n, bgr.ptr, 0, o2.ptr)
                res["sumsq"].append(o1.get()[0]); res["arena"].append(o2.get()[0])
                _same("deterministic grad_from_arena_sumsq: grad", bgr.get(), gw)
            for key, src in (("sumsq", g), ("arena", gw)):
                exact = R.sumsq_exact(src)
                assert abs(float(res[key][0]) - exact) <= R.sumsq_bound(n + 1, exact), (key, n)
                _same("deterministic %s: calls / streams" % key, np.array(res[key]), np.full(4, res[key][0]))
    finally:
        hip.set_option("deterministic", hip.get_option_default("deterministic"))


# ----------------------------------------------------------------------------- the job model (4. - 7.)
class Job(object):
    """One gad_optim_job over synthetic buffers + what the reference says it does.  hp None: no Adam.
    arena: None | "set" | "acc".  clip: None or the gradient norm as a multiple of clip_max (0 = an all-zero gradient).
    active / sel: None | "random" | "groups".  target: a target network is updated."""

    def __init__(self, rng, n, hp=None, t=1, active=None, arena=None, clip=None, clip_max=0.5, gscale=1.0, mirror=True,
                 target=False, sel=None, tau=1e-4, hard=0, tmirror=True, absmax_p=False, absmax_g=False, preload=False,
                 counter_n=None, counter_add=0, with_p=True, grad_buf=True):
        self.n, self.hp, self.t, self.arena, self.clip_max, self.gscale = n, hp, t, arena, clip_max, gscale
        self.target, self.tau, self.hard, self.counter_add = target, tau, hard, counter_add
        self.clip, self.with_p, self.grad_buf = clip, with_p, grad_buf
        h = self.h = {}
        h["p"] = (rng.normal(size=n) * 0.1).astype(np.float32)
        g = (rng.normal(size=n) * 0.02).astype(np.float32)
        if clip is not None:
            nrm = math.sqrt(R.sumsq_exact(g))
            g = (g * np.float32(clip * clip_max / nrm)).astype(np.float32) if (clip > 0 and nrm > 0) else np.zeros(n, np.float32)
        h["m"] = (rng.normal(size=n) * 0.01).astype(np.float32)                         # a state a few steps old
        h["v"] = (rng.normal(size=n) ** 2 * 1e-6 + 1e-12).astype(np.float32)
        self.active = None if active is None else (R.group_mask(rng, n) if active == "groups" else rng.integers(0, 2, n).astype(np.uint8))
        self.m2p, self.pn = R.injection(rng, n)
        if arena is None:
            h["g"] = g
        else:
            self.ga = np.zeros(self.pn)
            self.ga[self.m2p[self.m2p >= 0]] = g[self.m2p >= 0].astype(np.float64) * (1 + 2.0 ** -30)
            h["g"] = (rng.normal(size=n) * 0.01).astype(np.float32) if arena == "acc" else _nan32(n)
        packed = _pattern32(self.pn)
        packed[self.m2p[self.m2p >= 0]] = h["p"][self.m2p >= 0]
        h["packed"] = packed if mirror else None
        if target:
            h["tg"] = (rng.normal(size=n) * 0.1).astype(np.float32)
            self.sel = None if sel is None else (R.group_mask(rng, n, (0, 1, 2)) if sel == "groups" else rng.integers(0, 3, n).astype(np.uint8))
            self.tm2p, self.tpn = R.injection(rng, n)
            tp = _pattern32(self.tpn)
            tp[self.tm2p[self.tm2p >= 0]] = h["tg"][self.tm2p >= 0]
            h["tpacked"] = tp if tmirror else None
        for key, on in (("amax_p", absmax_p), ("amax_g", absmax_g)):
            h[key] = None if not on else (np.array([0, 0.001, 0, 1e-3, 0, 0, 5e-4, 0], np.float32) if preload else np.zeros(SLOTS, np.float32))
        h["counter"] = None if counter_n is None else ((1 << 33) + 17 + np.arange(max(counter_n, 1) + 3)).astype(np.int64)
        self.counter_n = counter_n or 0
        self.hyper = None if hp is None else R.hyper_block(hp, t, gscale)

    # the gradient after the arena conversion (bit-exact float32), and the clip's sum of squares over it
    def grad_in(self):
        g = self.h["g"]
        if self.arena is not None:
            g = R.grad_from_arena(self.ga, self.m2p, g, self.arena == "acc")
        return g

    def sumsq(self):
        return None if self.clip is None else R.sumsq_exact(self.grad_in())

    def reference(self, dtype):
        cache = self.__dict__.setdefault("_ref", {})
        if dtype not in cache:
            cache[dtype] = self._reference(dtype)
        return cache[dtype]

    def _reference(self, dtype):
        h = self.h
        out = {"p": h["p"].astype(dtype), "m": h["m"].astype(dtype), "v": h["v"].astype(dtype), "g": self.grad_in().astype(dtype)}
        if self.hp is not None:
            out["p"], out["g"], out["m"], out["v"] = R.adam_step(h["p"], self.grad_in(), h["m"], h["v"], self.hp, self.t, dtype,
                                                               active=self.active, sumsq=self.sumsq(),
                                                               clip_max=None if self.clip is None else self.clip_max, grad_scale=self.gscale)
        if self.target:
            out["tg"] = R.target_update(h["tg"], out["p"], self.sel, self.tau, self.hard, dtype)
        return out

    def upload(self):
        h, hip = self.h, _hip()
        d = self.d = {k: (None if v is None else Buf(v)) for k, v in h.items()}
        d["m2p"], d["active"] = Buf(self.m2p), None if self.active is None else Buf(self.active)
        d["ga"] = Buf(self.ga) if self.arena is not None else None
        d["hyper"] = None if self.hyper is None else Buf(self.hyper)
        d["ss"] = None if self.clip is None else Buf(np.array([self.sumsq()]))
        if self.target:
            d["sel"], d["tm2p"] = None if self.sel is None else Buf(self.sel), Buf(self.tm2p)
        return d

    def struct(self):
        hip, d = _hip(), self.upload()
        P = lambda k: None if d.get(k) is None else d[k].ptr
        j = hip.OptimJob()
        j.n = self.n
        if self.with_p:
            j.p = P("p")
        if self.grad_buf:
            j.grad = P("g")
        if self.hp is not None:
            j.exp_avg, j.exp_avg_sq, j.hyper = P("m"), P("v"), P("hyper")
        j.active, j.m2p, j.packed, j.gacc, j.accumulate = P("active"), P("m2p"), P("packed"), P("ga"), int(self.arena == "acc")
        if self.clip is not None:
            j.clip_sumsq, j.clip_max = P("ss"), self.clip_max
        if self.target:
            j.target, j.target_sel, j.target_m2p, j.target_packed = P("tg"), P("sel"), P("tm2p"), P("tpacked")
            j.tau, j.hard_enable = self.tau, self.hard
        j.absmax_p, j.absmax_grad = P("amax_p"), P("amax_g")
        if self.h["counter"] is not None:
            j.counter, j.counter_n, j.counter_add = P("counter"), self.counter_n, self.counter_add
        return j

    def run_chain(self):
        """the same work through the single-purpose entry points: gad_grad_from_arena -> gad_adam_step -> gad_polyak"""
        hip, d = _hip(), self.upload()
        P = lambda k: None if d.get(k) is None else d[k].ptr
        if self.arena is not None:
            hip.call("gad_grad_from_arena", P("ga"), P("m2p"), self.n, P("g"), int(self.arena == "acc"))
        if self.hp is not None:
            hip.call("gad_adam_step", P("p"), P("g"), P("m"), P("v"), P("active"), P("m2p"), P("packed"), self.n, P("hyper"), P("ss"),
                     float(self.clip_max if self.clip is not None else 0.0))
        if self.target:
            hip.call("gad_polyak", P("tg"), P("p"), P("sel"), P("tm2p"), P("tpacked"), self.n, float(self.tau), int(self.hard))
        return self.download()

    def download(self):
        out = {k: (None if b is None else b.get(k)) for k, b in self.d.items()}
        for k, src in (("m2p", self.m2p), ("active", self.active), ("hyper", self.hyper), ("ga", getattr(self, "ga", None)),
                       ("sel", getattr(self, "sel", None)), ("tm2p", getattr(self, "tm2p", None))):
            if out.get(k) is not None:
                _same("input " + k, out[k], src)
        return out

    def check(self, got, what, log=None):
        """everything the launch wrote, against the references; the untouched, bit for bit"""
        h = self.h
        r64, r32 = self.reference(np.float64), self.reference(np.float32)
        act = np.ones(self.n, bool) if self.active is None else self.active.astype(bool)
        adam = self.hp is not None
        errs = {}
        if adam:
            b64 = self.clip is not None and R.clip_coef(self.sumsq(), self.clip_max, np.float64) < 1
            b32 = self.clip is not None and R.clip_coef(self.sumsq(), self.clip_max, np.float32) < 1
            assert b64 == b32, "%s: float32 and float64 disagree on the clip branch" % what
            p0 = h["p"].astype(np.float64)
            if act.any() and self.n:
                errs["update"] = R.within(what + ": update p_after - p_before", got["p"].astype(np.float64) - p0, r64["p"] - p0,
                                          r32["p"].astype(np.float64) - p0)
                errs["exp_avg"] = R.within(what + ": exp_avg", got["m"], r64["m"], r32["m"])
                errs["exp_avg_sq"] = R.within(what + ": exp_avg_sq", got["v"], r64["v"], r32["v"])
                if self.clip is not None:
                    errs["grad"] = R.within(what + ": clip-scaled .grad", got["g"], r64["g"], r32["g"])
            for k in ("p", "m", "v"):
                _same(what + ": inactive " + k, got[k][~act], h[k][~act])
            if self.arena is None:
                _same(what + ": inactive .grad", got["g"][~act], h["g"][~act])
            else:
                _same(what + ": inactive .grad after the arena conversion", got["g"][~act], self.grad_in()[~act])
            if self.clip is None:
                _same(what + ": .grad without a clip", got["g"], self.grad_in())
        else:
            for k in ("p", "m", "v"):
                _same(what + ": no Adam, " + k, got[k], h[k])
            _same(what + ": .grad", got["g"], self.grad_in())
        if h["packed"] is not None:
            want = h["packed"].copy()
            live = self.m2p >= 0
            want[self.m2p[live]] = got["p"][live]
            _same(what + ": packed mirror", got["packed"], want)
        if self.target:
            errs["target"] = R.within(what + ": target", got["tg"], r64["tg"], r32["tg"])
            t0 = h["tg"].astype(np.float64)
            R.within(what + ": target update", got["tg"].astype(np.float64) - t0, r64["tg"] - t0, r32["tg"].astype(np.float64) - t0)
            sel = np.ones(self.n, np.uint8) if self.sel is None else self.sel
            keep = (sel == 0) | ((sel == 2) & (self.hard == 0))
            _same(what + ": target elements neither selected nor hard-enabled", got["tg"][keep], h["tg"][keep])
            hardc = (sel == 2) & (self.hard != 0)
            _same(what + ": hard-copied target elements", got["tg"][hardc], got["p"][hardc])
            if h["tpacked"] is not None:
                want = h["tpacked"].copy()
                wr = (self.tm2p >= 0) & ~keep
                want[self.tm2p[wr]] = got["tg"][wr]
                _same(what + ": target's packed mirror", got["tpacked"], want)
        if log is not None:
            log.append((what, {k: "%.2e/%.2e" % v for k, v in errs.items()}))
        return errs

    def check_stats(self, got, what):
        h = self.h
        act = None if self.active is None else self.active
        for key, ref in (("amax_p", lambda: R.absmax(got["p"])), ("amax_g", lambda: R.absmax(got["g"], include=act))):
            if h[key] is None:
                continue
            want = np.float32(max(float(ref()), float(h[key].max()))) if not np.isnan(ref()) else np.float32(np.nan)
            slots = got[key]
            if self.n == 0:
                _same(what + ": slots of an empty job", slots, h[key])
                continue
            if np.isnan(want):
                assert np.isnan(slots.max()), "%s: %s lost the NaN: %r" % (what, key, slots)
                continue
            assert not np.isnan(slots).any() and (slots >= h[key]).all(), "%s: %s slots shrank: %r" % (what, key, slots)
            _same(what + ": max over the %s slots" % key, np.float32(slots.max()), want)
        if h["counter"] is not None:
            want = h["counter"].copy()
            want[:self.counter_n] += self.counter_add
            _same(what + ": counters", got["counter"], want)


def _launch(jobs):
    hip = _hip()
    arr = (hip.OptimJob * len(jobs))(*[j.struct() for j in jobs])
    hip.check(hip.lib().gad_optim_jobs(arr, len(jobs), hip.stream()), "gad_optim_jobs")
    return [j.download() for j in jobs]


def _twins(what, a, b, keys):
    for k in keys:
        if a.get(k) is not None:
            _same("%s: gad_optim_jobs vs the single-purpose entry points, %s" % (what, k), b[k], a[k])


TWIN_KEYS = ("p", "m", "v", "g", "packed", "tg", "tpacked")

# (optimiser, first step, active, arena, clip: norm / max, grad_scale, target: (sel, tau, hard) or None)
ADAM_CASES = [
    ("policy", 1, None, None, None, 1.0, (None, 1e-4, 0)),
    ("critic", 1, "random", None, 3.0, 1.0, ("random", 1e-4, 1)),
    ("critic", 1, "groups", None, 0.5, 1.0, ("groups", 1e-4, 0)),
    ("critic", 1, None, None, 1.0 - 1e-3, 1.0, ("random", 0.05, 0)),
    ("critic", 1, "groups", None, 1.0 + 1e-3, 1.0, ("groups", 1.0, 1)),
    ("critic", 1, None, None, 0.0, 1.0, None),
    ("val_encoder", 1, None, "set", None, 1.0, None),
    ("encoder", 1, "groups", "set", None, 1.0, None),
    ("encoder", 1, "random", "acc", None, 0.25, None),
    ("policy", 1, "groups", "set", None, 1.0, (None, 0.05, 0)),
    ("policy", 10000, "random", "set", 3.0, 2.0, ("groups", 1e-4, 1)),
    ("encoder", 10000, None, None, None, 1.0, None),
]
ADAM_SIZES = {i: SIZES for i in (1, 2, 9, 10)}                                  # the rich cases run every size


def _adam_params():
    out = []
    for i, c in enumerate(ADAM_CASES):
        for n in ADAM_SIZES.get(i, (3, 257, 4099)):
            out.append(pytest.param(i, n, id="%d-%s-t%d-n%d" % (i, c[0], c[1], n)))
    return out


@pytest.mark.parametrize("case,n", _adam_params())
def test_adam_five_steps_both_forms(case, n, optimisers, capsys):
    """4. + 5. + 6.: five steps of gad_grad_from_arena -> gad_adam_step -> gad_polyak and of one gad_optim_jobs launch, each step
    from the state the single-purpose chain left: both within the yardstick of the float64 reference, and bit-identical"""
    name, t0, active, arena, clip, gscale, tgt = ADAM_CASES[case]
    rng = np.random.default_rng(1000 * case + n)
    log = []
    state = None
    for t in range(t0, t0 + 5):
        j = Job(rng, n, hp=optimisers[name], t=t, active=active, arena=arena, clip=clip, clip_max=optimisers["clip_grad"], gscale=gscale,
                target=tgt is not None, sel=tgt and tgt[0], tau=tgt and tgt[1], hard=tgt and tgt[2])
        if state is not None:                                                  # same masks / maps, new gradient, carried state
            j.active, j.m2p, j.pn = state.active, state.m2p, state.pn
            if arena is not None:
                g = np.where(j.m2p >= 0, rng.normal(size=n) * 0.02, 0.0)
                j.ga = np.zeros(j.pn); j.ga[j.m2p[j.m2p >= 0]] = g[j.m2p >= 0]
            for k in ("p", "m", "v", "packed"):
                j.h[k] = prev[k]
            if tgt is not None:
                j.sel, j.tm2p, j.tpn = state.sel, state.tm2p, state.tpn
                j.h["tg"], j.h["tpacked"] = prev["tg"], prev["tpacked"]
        a = j.run_chain()
        j.check(a, "step %d chain" % t, log)
        b = _launch([j])[0]
        j.check(b, "step %d jobs" % t, log)
        _twins("step %d" % t, a, b, TWIN_KEYS)
        state, prev = j, a
    with capsys.disabled():
        print("\n[adam case %d n %d] %s" % (case, n, log[-1]))


@pytest.mark.parametrize("n", SIZES)
def test_target_update_both_forms(n, optimisers):
    """6.: every (selector, hard_enable, tau) through gad_polyak and through a target-only job (no Adam: the source is p)"""
    rng = np.random.default_rng(600 + n)
    combos = [(sel, hard, tau, tm) for sel in (None, "random", "groups") for hard in (0, 1) for tau in (optimisers["tau"], 0.05, 1.0)
              for tm in ((True, False) if sel == "groups" else (True,))]
    if n > 4099:                                                               # the cross product runs at the twelve smaller sizes
        combos = [("groups", 1, 0.05, True), (None, 0, optimisers["tau"], True), ("random", 0, 1.0, False)]
    for sel, hard, tau, tmirror in combos:
        j = Job(rng, n, target=True, sel=sel, tau=tau, hard=hard, tmirror=tmirror, grad_buf=False)
        what = "polyak n %d sel %s hard %d tau %g" % (n, sel, hard, tau)
        a = j.run_chain()
        j.check(a, what + " (gad_polyak)")
        b = _launch([j])[0]
        j.check(b, what + " (job)")
        _twins(what, a, b, TWIN_KEYS)


# ----------------------------------------------------------------------------- 7. the step's five job arrays
def _step_jobs(rng, O, which, n):
    """the field combinations runtime._optim_job builds for the phases c, a, end, a+end, c+end over buffers of sizes n[...]"""
    venc = lambda: Job(rng, n["venc"], hp=O["val_encoder"], t=3, active="random", arena="set")
    cr = lambda **kw: Job(rng, n["cr"], hp=O["critic"], t=3, active="groups", clip=3.0, clip_max=O["clip_grad"], target=True, sel="groups",
                          tau=O["tau"], hard=1, absmax_p=True, **kw)
    pol = lambda: Job(rng, n["pol"], hp=O["policy"], t=3, active="random", arena="set", target=True, sel=None, tau=O["tau"], absmax_p=True)
    enc = lambda adam: Job(rng, n["enc"], hp=O["encoder"] if adam else None, t=3, active="random", arena="set", counter_n=n["cnt"], counter_add=2)
    end = lambda: Job(rng, n["cr"], active="groups", absmax_g=True, counter_n=n["cnt"], counter_add=3)
    return {"c": lambda: [venc(), cr()], "a": lambda: [pol(), enc(True)], "a_frozen": lambda: [pol(), enc(False)], "end": lambda: [end()],
            "a+end": lambda: [pol(), enc(True), end()],
            "c+end": lambda: [venc(), cr(absmax_g=True, counter_n=n["cnt"], counter_add=2)]}[which]()


@pytest.mark.parametrize("which", ("c", "a", "a_frozen", "end", "a+end", "c+end"))
@pytest.mark.parametrize("sizes", ({"venc": 4099, "cr": 1025, "pol": 3, "enc": 0, "cnt": 1},
                                   {"venc": (1 << 20) | 3, "cr": 3, "pol": 1027, "enc": 70001, "cnt": 256},
                                   {"venc": 0, "cr": (1 << 20) + 5, "pol": 255, "enc": 3, "cnt": 0}), ids=("small", "big_venc", "big_cr"))
def test_step_job_arrays(which, sizes, optimisers):
    rng = np.random.default_rng(700 + len(which) + sizes["cr"])
    jobs = _step_jobs(rng, optimisers, which, sizes)
    outs = _launch(jobs)
    for k, (j, o) in enumerate(zip(jobs, outs)):
        what = "%s job %d (n %d)" % (which, k, j.n)
        j.check(o, what)
        j.check_stats(o, what)


def test_four_jobs_of_very_different_sizes(optimisers):
    rng = np.random.default_rng(710)
    O = optimisers
    jobs = [Job(rng, 0, hp=O["policy"], t=2, arena="set", counter_n=256, counter_add=7, absmax_p=True, absmax_g=True),
            Job(rng, 3, hp=O["critic"], t=2, active="random", clip=2.0, absmax_p=True, absmax_g=True, preload=True, counter_n=1, counter_add=-1),
            Job(rng, (1 << 20) | 3, hp=O["encoder"], t=2, active="groups", arena="acc", target=True, sel="groups", hard=1, absmax_p=True,
                absmax_g=True, counter_n=256, counter_add=2),
            Job(rng, 4099, absmax_g=True, absmax_p=True, preload=True, counter_n=0, counter_add=5)]
    for count in (1, 2, 3, 4):
        outs = _launch(jobs[:count])
        for k, (j, o) in enumerate(zip(jobs, outs)):
            j.check(o, "%d jobs, job %d" % (count, k))
            j.check_stats(o, "%d jobs, job %d" % (count, k))


@pytest.mark.parametrize("n", (4099, (1 << 20) | 3))
@pytest.mark.parametrize("where,adam", [(w, a) for a in (False, True) for w in ("tail", "last_workgroup", "inactive", "first")] +
                         [("nan", False), ("inf", False)])
def test_absmax_slots_find_the_extreme_element(n, where, adam, optimisers):
    """the maximum over the slots equals the reference statistic exactly: max |p| after the update over every element,
    max |.grad| after the clip scaling over the elements that have a gradient (a parameter whose .grad is None counts 0 in
    module_max_gradient); a NaN is reported as NaN, as torch.abs(x).max() does.  The extreme element sits in the scalar tail,
    in the last workgroup, in an inactive element, in element 0 under pre-loaded slots."""
    rng = np.random.default_rng(720 + n)
    j = Job(rng, n, hp=optimisers["critic"] if adam else None, t=4, active="random", clip=3.0 if adam else None,
            clip_max=optimisers["clip_grad"], absmax_p=True, absmax_g=True, preload=(where == "first"))
    i = {"tail": n - 1, "last_workgroup": (n & ~3) - 2, "inactive": int(np.flatnonzero(j.active == 0)[-1]), "first": 0, "nan": n // 2,
         "inf": n // 3}[where]
    if where != "inactive":
        j.active[i] = 1
    big = np.float32({"nan": np.nan, "inf": -np.inf}.get(where, -7.5))
    j.h["p"][i] = big
    j.h["g"][i] = big
    if j.m2p[i] >= 0:
        j.h["packed"][j.m2p[i]] = big
    o = _launch([j])[0]
    what = "absmax %s n %d adam %d" % (where, n, adam)
    j.check(o, what)
    j.check_stats(o, what)
    if where == "inactive":
        assert o["amax_p"].max() == np.float32(7.5) and o["amax_g"].max() < np.float32(1.0)
    if where == "nan":
        assert np.isnan(o["amax_p"].max()) and np.isnan(o["amax_g"].max())


def test_optim_jobs_refusals_launch_nothing(optimisers):
    hip = _hip()
    rng = np.random.default_rng(730)
    L = hip.lib()

    def attempt(mutate, count, want):
        jobs = [Job(rng, 257, hp=optimisers["critic"], t=1, arena="set", target=True, absmax_p=True, counter_n=4, counter_add=1) for _ in range(5)]
        structs = [j.struct() for j in jobs]
        mutate(structs)
        arr = (hip.OptimJob * 5)(*structs)
        assert L.gad_optim_jobs(arr, count, hip.stream()) == want, L.gad_last_error()
        assert len(L.gad_last_error()) > 0
        for j in jobs:
            o = j.download()
            for k, v in j.h.items():
                if v is not None:
                    _same("refused launch: " + k, o[k], v)                      # .grad still NaN, counters and slots as they were
    attempt(lambda s: None, 0, ERR_SHAPE)
    attempt(lambda s: None, MAX_JOBS + 1, ERR_SHAPE)

    def misalign(s):
        s[1].p = s[1].p + 4
    attempt(misalign, 2, ERR_SHAPE)

    def misalign_mask(s):
        s[0].active = s[0].m2p + 2
    attempt(misalign_mask, 1, ERR_SHAPE)

    def drop(s):
        s[1].exp_avg = None
    attempt(drop, 2, ERR_NULL)

    def neg(s):
        s[0].n = -1
    attempt(neg, 1, ERR_SHAPE)


def test_optim_jobs_above_the_grid_cap():
    """16384 workgroups x 1024 elements is the launch's cap: beyond it the workgroups loop.  One case, Adam off (arena ->
    .grad, target from p, both statistics, counters): 16384 * 1024 + 1027 elements, about 0.6 GB of buffers."""
    rng = np.random.default_rng(740)
    n = 16384 * 1024 + 1027
    j = Job(rng, n, arena="set", active="random", target=True, sel="random", hard=1, tau=0.05, absmax_p=True, absmax_g=True, counter_n=256,
            counter_add=1, mirror=False, tmirror=False)
    j.h["p"][n - 1] = -9.0
    j.ga[j.m2p[n - 2] if j.m2p[n - 2] >= 0 else 0] = 11.0
    o = _launch([j])[0]
    j.check(o, "above the grid cap")
    j.check_stats(o, "above the grid cap")


# ----------------------------------------------------------------------------- 8. gad_absmax_segments
def test_absmax_segments_exact():
    hip = _hip()
    rng = np.random.default_rng(800)
    lens = [0, 1, 1, 5, 0, 16383, 16384, 16385, 40001, 1, 3, 2, 4, 0]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    x = (rng.normal(size=off[-1]) * 10.0 ** rng.uniform(-3, 3, off[-1])).astype(np.float32)
    x[off[1]] = -0.0                                    # a one-element segment holding -0.0 -> +0.0
    x[off[2]] = -3.5
    x[off[8] + 40000] = -1e30                           # the last element of a segment that straddles the 64 x 256 stride
    x[off[7] + 16384] = 2e30                            # first element past one stride
    x[off[10]:off[11]] = [1e-45, -3e-45, 2e-45]         # subnormals
    x[off[11]:off[12]] = [np.nan, 1.0]                  # a NaN is reported
    x[off[12]:off[13]] = [-np.inf, 1.0, 2.0, 3.0]
    want = np.array([R.absmax(x[off[s]:off[s + 1]]) for s in range(len(lens))], np.float32)
    assert want[0] == 0 and want[4] == 0 and np.isnan(want[11]) and want[12] == np.inf and want[10] == np.float32(3e-45)
    bx, bo, out = Buf(x), Buf(off), Buf(_nan32(len(lens)))
    hip.call("gad_absmax_segments", bx.ptr, bo.ptr, len(lens), out.ptr)
    got = out.get()
    assert np.isnan(got[11]), got
    got[11] = want[11]
    _same("absmax_segments", got, want)
    _same("absmax_segments: x", bx.get(), x)


# ----------------------------------------------------------------------------- 9. gad_zero_buffers / gad_copy_buffers
BYTES = (0, 4, 12, 16, 20, 4096, 4100, 4104, 4108)
ZERO_CAP = 2048 * 256 * 16
COPY_CAP = 1024 * 256 * 16


def _zero(segs):
    hip = _hip()
    a = []
    for s in segs + [None] * (6 - len(segs)):
        a += [C.c_void_p(None), C.c_longlong(0)] if s is None else [C.c_void_p(s[0]), C.c_longlong(s[1])]
    return hip.lib().gad_zero_buffers(*(a + [hip.stream()]))


def test_zero_buffers_heads_bodies_tails():
    rng = np.random.default_rng(900)
    combos = [(al, nb) for al in (0, 4, 8, 12) for nb in BYTES + (ZERO_CAP + 16 + al,)]
    for base in range(0, len(combos), 4):
        bufs = [Buf(rng.integers(1, 255, nb, dtype=np.uint8), shift=al) for al, nb in combos[base:base + 4]]
        # a NULL segment and a zero-length segment in the middle of the list
        spare = Buf(rng.integers(1, 255, 64, dtype=np.uint8))
        segs = [(int(bufs[0].ptr), bufs[0].nbytes), None, (int(bufs[1].ptr), bufs[1].nbytes), (int(spare.ptr), 0),
                (int(bufs[2].ptr), bufs[2].nbytes), (int(bufs[3].ptr), bufs[3].nbytes)]
        assert _zero(segs) == 0
        for b, (al, nb) in zip(bufs, combos[base:base + 4]):
            assert not b.get("zero_buffers align %d bytes %d" % (al, nb)).any(), (al, nb)
        assert spare.get().all()
    # refused on the host: a byte count or an address that is not a multiple of 4 -- nothing is written
    for al, nb in [(0, 6), (0, -4)] + [(al, 16) for al in range(1, 16) if al % 4]:
        b, ok = Buf(np.full(32, 7, np.uint8), shift=al), Buf(np.full(32, 7, np.uint8))
        assert _zero([(int(ok.ptr), 32), (int(b.ptr), nb)]) == ERR_SHAPE, (al, nb)
        assert (b.get() == 7).all() and (ok.get() == 7).all()
    assert _zero([]) == 0


def _copy(segs, count=None):
    hip = _hip()
    arr = (hip.CopySeg * max(len(segs), 1))()
    for k, (dst, src, nb, add) in enumerate(segs):
        arr[k].dst, arr[k].src, arr[k].bytes, arr[k].add = dst, src, nb, add
    return hip.lib().gad_copy_buffers(arr, len(segs) if count is None else count, hip.stream())


def _f32_payload(rng, nb):
    a = (rng.normal(size=nb // 4) * 10.0 ** rng.uniform(-3, 3, nb // 4)).astype(np.float32)
    a[:min(len(a), 4)] = np.array([-0.0, np.inf, 1e-40, -1.0], np.float32)[:min(len(a), 4)]
    return a


def test_copy_buffers_alignments_and_add():
    rng = np.random.default_rng(910)
    combos = [(da, sa, nb) for da in (0, 4, 8, 12) for sa in (0, 4, 8, 12) for nb in BYTES]
    combos += [(0, 0, COPY_CAP + 48), (4, 0, COPY_CAP + 20), (0, 8, COPY_CAP + 16), (12, 12, COPY_CAP + 4)]
    for add in (0.0, 0.5, -1.0):
        for base in range(0, len(combos), 14):
            chunk = combos[base:base + 14]
            srcs = [Buf(_f32_payload(rng, nb), shift=sa) for da, sa, nb in chunk]
            dsts = [Buf(_nan32(nb // 4), shift=da) for da, sa, nb in chunk]
            spare = Buf(_nan32(8))
            segs = [(int(d.ptr), int(s.ptr), s.nbytes, add) for d, s in zip(dsts, srcs)]
            segs.insert(3, (None, int(srcs[0].ptr), 16, add))                       # NULL destination
            segs.insert(7, (int(spare.ptr), int(srcs[0].ptr), 0, add))              # zero bytes
            assert len(segs) <= 16 and _copy(segs) == 0
            for d, s, c in zip(dsts, srcs, chunk):
                src = s.get("copy source")
                with np.errstate(invalid="ignore"):
                    want = src if add == 0.0 else (src + np.float32(add)).astype(np.float32)
                _same("copy_buffers dst align %d src align %d bytes %d add %g" % (c + (add,)), d.get("copy destination"), want)
            assert np.isnan(spare.get()).all()
    # in place
    a = _f32_payload(rng, 4108)
    b = Buf(a, shift=4)
    assert _copy([(int(b.ptr), int(b.ptr), 4108, 0.25)]) == 0
    _same("copy_buffers in-place add", b.get(), (a + np.float32(0.25)).astype(np.float32))
    # 16 segments run, 17 and a byte count of 6 are refused with nothing written
    srcs = [Buf(_f32_payload(rng, 20)) for _ in range(17)]
    dsts = [Buf(_nan32(5)) for _ in range(17)]
    segs = [(int(d.ptr), int(s.ptr), 20, 0.0) for d, s in zip(dsts, srcs)]
    assert _copy(segs[:16] + [segs[16]], 17) == ERR_SHAPE
    assert _copy([segs[0], (segs[1][0], segs[1][1], 6, 0.0)]) == ERR_SHAPE
    assert _copy([(segs[0][0] + 2, segs[0][1], 4, 0.0)]) == ERR_SHAPE
    assert all(np.isnan(d.get()).all() for d in dsts)
    assert _copy(segs[:16]) == 0
    for d, s in zip(dsts[:16], srcs[:16]):
        _same("copy_buffers 16 segments", d.get(), s.get())
    assert np.isnan(dsts[16].get()).all() and _copy([], 0) == 0


# ----------------------------------------------------------------------------- 10. gad_replay_gather
@pytest.mark.parametrize("B", (1, 3, 256))
@pytest.mark.parametrize("cloud_elems", (4120, 2, 6))
@pytest.mark.parametrize("with_next", (True, False))
def test_replay_gather_bit_exact(B, cloud_elems, with_next):
    hip = _hip()
    rng = np.random.default_rng(1000 + B + cloud_elems)
    cap = 64
    tag = lambda k, *shape: (k * 1000.0 + np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) * 0.25 + 0.125).astype(np.float32)
    src = {"point_state": tag(1, cap, cloud_elems), "action": tag(2, cap, 6), "expert_action": tag(3, cap, 6), "goal": tag(4, cap, 7),
           "reward": tag(5, cap), "returns": tag(6, cap), "terminal": tag(7, cap), "timestep": rng.integers(0, 30, cap).astype(np.float32),
           "expert_flags": tag(9, cap), "perturb_flags": tag(10, cap)}
    src["timestep"][:4] = [1e8, 3.0, 16777216.0, 0.5]                    # t[end] + 1 rounds before t[idx] is subtracted
    idx = rng.integers(0, cap, B).astype(np.int64)
    idx[0] = cap - 1
    if B > 1:
        idx[1], idx[2] = 0, 0                                            # an index at 0, and a repeated one
    nxt = (idx + 1) % cap                                                # wraps to 0 at cap - 1
    end = rng.integers(0, cap, B).astype(np.int64)
    end[0] = idx[0]                                                      # end == idx
    if B > 2:
        end[2], idx[2] = 0, 2                                            # float32(1e8 + 1) - 16777216
        nxt[2] = 3
    outs = {"out_point": (B, cloud_elems), "out_next_point": (B, cloud_elems), "out_action": (B, 6), "out_expert_action": (B, 6),
            "out_goal": (B, 7), "out_reward": (B,), "out_return": (B,), "out_mask": (B,), "out_time": (B,), "out_time_m1": (B,),
            "out_expert_flag": (B,), "out_perturb_flag": (B,)}
    bs = {k: Buf(v) for k, v in src.items()}
    bi = {"idx": Buf(idx), "nxt": Buf(nxt), "end": Buf(end)}
    bo = {k: Buf(_nan32(int(np.prod(s))).reshape(s)) for k, s in outs.items()}
    a = hip.ReplayGatherArgs()
    a.B, a.cloud_elems = B, cloud_elems
    for k, b in list(bs.items()) + list(bi.items()) + list(bo.items()):
        setattr(a, k, b.ptr)
    if not with_next:
        a.out_next_point = None
    hip.call_struct("gad_replay_gather", a)
    t = src["timestep"]
    tm = ((t[end] + np.float32(1)).astype(np.float32) - t[idx]).astype(np.float32)        # the kernel's order of operations
    want = {"out_point": src["point_state"][idx], "out_next_point": src["point_state"][nxt], "out_action": src["action"][idx],
            "out_expert_action": src["expert_action"][idx], "out_goal": src["goal"][idx], "out_reward": src["reward"][idx],
            "out_return": src["returns"][idx], "out_mask": src["terminal"][idx], "out_time": tm,
            "out_time_m1": (tm - np.float32(1)).astype(np.float32), "out_expert_flag": src["expert_flags"][idx],
            "out_perturb_flag": src["perturb_flags"][idx]}
    for k in outs:
        got = bo[k].get(k)
        if k == "out_next_point" and not with_next:
            assert np.isnan(got).all()
        else:
            _same("replay_gather " + k, got, np.ascontiguousarray(want[k]))
    for k, b in bs.items():
        _same("replay_gather source " + k, b.get(), src[k])


# ----------------------------------------------------------------------------- 11. gad_split_weights
def _bf16_bits(x32):
    """round-to-nearest-even bfloat16 of float32 values (torch's conversion), as uint16 bit patterns + the float32 value"""
    b = torch.from_numpy(np.ascontiguousarray(x32)).to(torch.bfloat16)
    return b.view(torch.int16).numpy().view(np.uint16), b.float().numpy()


def _split_planes(w):
    hi_b, hi = _bf16_bits(w)
    r1 = (w - hi).astype(np.float32)
    mid_b, mid = _bf16_bits(r1)
    r2 = (r1 - mid).astype(np.float32)
    lo_b, lo = _bf16_bits(r2)
    return (hi_b, mid_b, lo_b), (hi, mid, lo)


SPLIT_SHAPES = [(n_out, Ks) for n_out in (4, 36, 64, 516) for Ks in (32, 64, 96)]


@pytest.mark.parametrize("pair", range(0, len(SPLIT_SHAPES), 2))
def test_split_weights_planes_signs_and_layout(pair):
    from tests.split_cases import decode_mirror
    hip = _hip()
    rng = np.random.default_rng(1100 + pair)
    shapes = SPLIT_SHAPES[pair:pair + 2]
    layers, packed, cursor, ocur = [], [_nan32(12)], 12, 8
    for li, (n_out, Ks) in enumerate(shapes):
        Kp = Ks + 4 * (li + 1)
        w = np.full((n_out, Kp), np.nan, np.float32)                               # columns Ks .. Kp must not be read
        w[:, :Ks] = (rng.normal(size=(n_out, Ks)) * 10.0 ** rng.uniform(-4, 1, (n_out, Ks))).astype(np.float32)
        # stated expectations for the edge values: the planes are the RNE bf16 conversions of the exact float32 residuals
        # whatever the value (0 and -0.0 give signed zeros, 1e-38 is a float32 subnormal, 3e38 is just below bf16's maximum)
        w[0, :4] = np.array([0.0, -0.0, 1e-38, 3e38], np.float32)
        w[n_out - 1, 16:20] = np.array([-0.0, 0.0, -3e38, -1e-38], np.float32)      # the same in an odd block of 16
        plane = n_out * Ks
        layers.append((cursor, n_out, Kp, Ks, ocur, ocur + 3 * plane + 8, w))
        packed.append(w.ravel()); cursor += w.size
        ocur += 6 * plane + 16
    total = ocur
    bp = Buf(np.concatenate(packed))
    out0 = np.full(total, 0xA5A5, np.uint16)
    bo = Buf(out0)
    arr = (hip.SplitLayer * len(layers))()
    for k, (w_off, n_out, Kp, Ks, f_off, t_off, w) in enumerate(layers):
        arr[k].w_off, arr[k].n_out, arr[k].Kp, arr[k].Ks, arr[k].fwd_off, arr[k].t_off = w_off, n_out, Kp, Ks, f_off, t_off
    hip.check(hip.lib().gad_split_weights(C.c_void_p(int(bp.ptr)), arr, len(layers), C.c_void_p(int(bo.ptr)), hip.stream()), "gad_split_weights")
    got = bo.get("split mirrors")
    want = out0.copy()
    for (w_off, n_out, Kp, Ks, f_off, t_off, w) in layers:
        ws = np.ascontiguousarray(w[:, :Ks])
        bits, vals = _split_planes(ws)
        plane = n_out * Ks
        normal = np.abs(ws) >= 2.0 ** -100                                         # residuals stay above bf16's subnormals
        total64 = sum(v.astype(np.float64) for v in vals)
        assert (total64[normal] == ws.astype(np.float64)[normal]).all()            # the reference itself: hi + mid + lo == w exactly
        sk = np.where((np.arange(Ks) >> 4) & 1, 0x8000, 0).astype(np.uint16)[None, :]
        sn = np.where((np.arange(n_out) >> 4) & 1, 0x8000, 0).astype(np.uint16)[None, :]
        for p in range(3):
            want[f_off + p * plane:f_off + (p + 1) * plane] = (bits[p] ^ sk).ravel()
            want[t_off + p * plane:t_off + (p + 1) * plane] = (np.ascontiguousarray(bits[p].T) ^ sn).ravel()
        # the mirrors decoded the way the GEMM tests' helper reads them: hi + mid + lo == w exactly
        for off, rows, cols, wm in ((f_off, n_out, Ks, ws), (t_off, Ks, n_out, np.ascontiguousarray(ws.T))):
            dec = decode_mirror(torch.from_numpy(got[off:off + 3 * plane].view(np.int16).copy()), plane, rows, cols, 1).numpy()
            nm = np.abs(wm) >= 2.0 ** -100
            assert (dec[nm] == wm.astype(np.float64)[nm]).all(), "hi + mid + lo != w (%d x %d)" % (rows, cols)
            assert np.abs(dec - wm.astype(np.float64)).max() <= 2.0 ** -133                   # below: within bf16's subnormal step
    _same("split mirrors: planes, signs, transposition, untouched bytes", got, want)


# ----------------------------------------------------------------------------- 12. BatchNorm bookkeeping
@pytest.mark.parametrize("C_", (1, 255, 257))
@pytest.mark.parametrize("band", ((1e-8, 1e-6), (1e-6, 1e-4), (1e-2, 1.0), (1e2, 1e4), (1e-8, 1e4)))
def test_bn_running_update_and_eval_affine(C_, band):
    hip = _hip()
    rng = np.random.default_rng(1200 + C_)
    eps, mom = 1e-5, 0.1
    var = np.exp(rng.uniform(np.log(band[0]), np.log(band[1]), C_))
    mean = (rng.normal(size=C_) * 3).astype(np.float32)
    istd = (1.0 / np.sqrt(var + eps)).astype(np.float32)
    count = rng.choice(np.array([1, 2, 48, 2e5], np.float32), C_)
    count[:min(C_, 4)] = np.array([1, 2, 48, 2e5], np.float32)[:min(C_, 4)]
    rm0 = (rng.normal(size=C_)).astype(np.float32)
    rv0 = (var * rng.uniform(0.5, 2.0, C_)).astype(np.float32)
    brm, brv = Buf(rm0), Buf(rv0)
    bm, bi, bc = Buf(mean), Buf(istd), Buf(count)
    hip.call("gad_bn_running_update", bm.ptr, bi.ptr, bc.ptr, C_, float(eps), float(mom), brm.ptr, brv.ptr)
    rm, rv = brm.get("running_mean"), brv.get("running_var")
    rm64, rv64 = R.bn_running_update(mean, istd, count, eps, mom, rm0, rv0, np.float64)
    rm32, rv32 = R.bn_running_update(mean, istd, count, eps, mom, rm0, rv0, np.float32)
    R.within("bn_running_update: running_mean", rm, rm64, rm32)
    # the variance is rebuilt from a float32 1 / sqrt(var + eps): its attainable accuracy is relative to var + eps
    scale = float((1.0 / istd.astype(np.float64) ** 2).max())
    e, e32 = np.abs(rv - rv64).max() / scale, np.abs(rv32 - rv64).max() / scale
    assert not np.isnan(rv).any() and e <= max(3 * e32, R.FLOOR), (e, e32)
    for b, a in ((bm, mean), (bi, istd), (bc, count)):
        _same("bn_running_update input", b.get(), a)
    gamma, beta = rng.normal(size=C_).astype(np.float32), rng.normal(size=C_).astype(np.float32)
    bg, bb, bsc, bsh = Buf(gamma), Buf(beta), Buf(_nan32(C_)), Buf(_nan32(C_))
    brm2, brv2 = Buf(rm), Buf(rv)
    hip.call("gad_bn_eval_affine", bg.ptr, bb.ptr, brm2.ptr, brv2.ptr, C_, float(eps), bsc.ptr, bsh.ptr)
    sc64, sh64 = R.bn_eval_affine(gamma, beta, rm, rv, eps, np.float64)
    sc32, sh32 = R.bn_eval_affine(gamma, beta, rm, rv, eps, np.float32)
    R.within("bn_eval_affine: scale", bsc.get(), sc64, sc32)
    R.within("bn_eval_affine: shift", bsh.get(), sh64, sh32)
