"""The deterministic mode's GEMM-side ordered kernels (option "deterministic"; ga-ddpg_amd/csrc/gemm.hip, gemm_dx.hip, gemm_dw.hip) held
to the order they state, one launch per case through the C entry point:

  A  the ordered scatter of the gathered first layer (det_dx_launch: scatter_group_bounds / _run_heads / _runs, gather_action_ordered)
  B  the ordered dW reduce (the zeroed partial slab, gad_ordered_reduce in its linear and its tree form)
  C  the slot-plane statistics (det_stat_slots / det_stat_reduce) of the forward and of dX
  D  the mode's plumbing: hints, streams, the scratch buffers' growth and release, gad_gemm_bwd, the mode-2 refusal

A and B are equality: the operands of tests/det_reference.py make every GEMM product and partial sum exact, so the only rounding left
is the sum whose order the mode promises, and the numpy reference of that order must be met bit for bit -- from NON-ZERO initial
values, so that an overwrite in place of an add shows.  C is equality too (integer sums below 2^53, exact in any order: a lost or
stale slot, a block counted twice, a row past the live count all show exactly) plus the float64 gate of tests/gemm_cases.py on the
same shapes with random operands.  D: a call's result depends on nothing but its arguments.  Nothing here is a tuned tolerance.

Plumbing as in tests/test_gpu_group_ops.py: every device buffer of a case lies between two 64-byte guard zones that must come back
untouched, inputs must come back bit-identical, pure outputs start as NaN, accumulators start from seeded non-zero values, all inputs
come from seeded generators, every case asserts its route (gad_last_kernel: the mode takes the generic tile kernels only), options
are set through Case.run and restored in its `finally`.

GAD_DET_REPORT=<file>: every case's control-difference fraction (how much of the output the opposite order of summation changes:
what makes the equality a test of the order) and, for the random-operand cases, the worst err / bound are written there
(profiles/det_kernel_gates.txt is that file from an MI355X run)."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import det_reference as D

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
DET = {"deterministic": 1}
UNSUPPORTED = -4                # include/gaddpg.h GAD_ERR_UNSUPPORTED
_REPORT = []
# what a launch may write; every other tensor of a case is an input and must come back bit-identical
OUTPUTS = {"zout", "stats", "key", "gout", "bst", "dfeat", "daction", "gacc", "ws", "P", "Q", "S"}


class _Cases(object):
    """tests.gemm_cases, imported when a case is built (collection must not need the library)"""

    def __getattr__(self, k):
        from tests import gemm_cases
        return getattr(gemm_cases, k)


gc = _Cases()


def _hip():
    from ga_ddpg_amd import hip
    return hip


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    path = os.environ.get("GAD_DET_REPORT")
    if path and _REPORT:
        with open(path, "w") as f:
            f.write("# gates of the deterministic mode's ordered kernels (tests/test_gpu_deterministic_kernels.py)\n"
                    "# command: GAD_DET_REPORT=<this file> python -m pytest tests/test_gpu_deterministic_kernels.py\n"
                    "# A / B: case -> route | output: bit-equal to the ascending-order reference; `control`: the fraction of the written\n"
                    "#   elements the opposite order changes (>= 0.02 asserted on the CPU wherever an order exists; `-`: none exists)\n"
                    "# C / D random operands: the float64 gate of tests/gemm_cases.py, worst err / ((T + 2) * 2^-24 * abs_bound)\n")
            f.write("\n".join(_REPORT) + "\n")


# ----------------------------------------------------------------------------- plumbing
class Guarded(object):
    """moves every tensor of `case` (and of the cases it holds) between two guard zones and remembers the inputs' bits"""

    def __init__(self, case):
        self.zones, self.inputs, seen = [], [], {}
        self._walk(case, seen, set())
        torch.cuda.synchronize()

    def _move(self, name, t, seen):
        if t.numel() == 0 or not t.is_cuda:
            return t
        if id(t) in seen:
            return seen[id(t)]
        assert t.is_contiguous(), name
        n = t.numel() * t.element_size()
        raw = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8, device=t.device)
        assert raw.data_ptr() % 256 == 0
        view = raw[GUARD:GUARD + n].view(t.dtype).view(t.shape)
        view.copy_(t)
        seen[id(t)] = view
        self.zones.append((name, raw, n))
        if name.split(".")[-1].split("[")[0] not in OUTPUTS:
            self.inputs.append((name, raw, raw.clone()))
        return view

    def _walk(self, obj, seen, visited):
        if id(obj) in visited:
            return
        visited.add(id(obj))
        who = type(obj).__name__
        for k, v in list(vars(obj).items()):
            if torch.is_tensor(v):
                setattr(obj, k, self._move("%s.%s" % (who, k), v, seen))
            elif isinstance(v, list) and v and all(torch.is_tensor(x) for x in v):
                setattr(obj, k, [self._move("%s.%s[%d]" % (who, k, i), x, seen) for i, x in enumerate(v)])
            elif isinstance(v, gc.Case):
                self._walk(v, seen, visited)

    def check(self):
        torch.cuda.synchronize()
        for name, raw, n in self.zones:
            edge = torch.cat([raw[:GUARD], raw[GUARD + n:]])
            assert bool((edge == FILL).all()), "%s: guard bytes written" % name
        for name, raw, was in self.inputs:
            assert torch.equal(raw, was), "%s: an input was modified" % name


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _bytes(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.size, -1) if a.size else np.zeros((0, a.itemsize), np.uint8)


def _diff(what, got, want):
    """bit-for-bit gate of one output: [] or [message]"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    ne = (_bytes(got) != _bytes(want)).any(1)
    if not ne.any():
        return []
    i = int(np.flatnonzero(ne)[0])
    return ["%s: %d of %d elements differ bitwise; first at flat index %d: got %r want %r" % (
        what, int(ne.sum()), ne.size, i, got.ravel()[i], want.ravel()[i])]


def _same(first, again, what):
    """every output of `again` is bit-equal to `first` (NaN included)"""
    assert sorted(first) == sorted(again)
    for k in first:
        bad = _diff("%s: %s" % (what, k), _np(again[k]), _np(first[k]))
        assert not bad, bad[0]


@contextlib.contextmanager
def _mode_on():
    """the option held at 1 across several launches (a Case.run with the option would switch it off, and so free the scratch,
    after every launch); cases run inside with Case.run({}), which keeps the Python mirror in step"""
    hip = _hip()
    try:
        hip.set_option("deterministic", 1)
        yield
    finally:
        hip.set_option("deterministic", hip.get_option_default("deterministic"))


def _frac(diff, n, ordered=True):
    return "%.3f (%d / %d)" % (diff / n, diff, n) if ordered and n else "-"


# ----------------------------------------------------------------------------- A. the ordered scatter
@functools.lru_cache(maxsize=None)
def _scatter_set(name):
    return D.scatter_inputs(name)


@functools.lru_cache(maxsize=None)
def _scatter_ref(name, alter=None):
    return D.scatter_reference(_scatter_set(name), **({} if alter is None else {"order": "desc"} if alter == "desc" else {alter: True}))


def _scatter_case(c):
    init = {k: c[k + "0"] for k in ("dfeat", "daction") if c[k + "0"] is not None}
    return gc.Dx(c["rows"], [c["n_out"]], c["Kp"], c["kv"], z=False, relu=0, coef=False, row_w=False, live=c["live"],
                 scatter=dict(feat_c=c["feat_c"], act_c=c["act_c"], gps=c["gps"], dfeat=c["dfeat0"] is not None,
                              daction=c["daction0"] is not None),
                 maps={k: c[k] for k in ("row_pt", "row_grp", "npts", "nsmp")},
                 operands=dict(G=c["G"], W=c["W"].reshape(-1)), init=init)


@functools.lru_cache(maxsize=None)
def _scatter_run(name):
    """one guarded launch of scatter case `name` under the mode -> its outputs as numpy"""
    case = _scatter_case(_scatter_set(name))
    g = Guarded(case)
    out, route = case.run(DET)
    assert route == "gemm_dx", "%s: routed to %s" % (name, route)
    g.check()
    return {k: _np(v) for k, v in out.items()}


def _scatter_gate(name, out, alter=None):
    c, ref = _scatter_set(name), _scatter_ref(name, alter)
    bad = []
    for k, want in zip(("dfeat", "daction"), ref):
        assert (want is None) == (k not in out)
        if want is not None:
            bad += _diff("%s %s" % (name, k), out[k], want)
    return bad


@pytest.mark.parametrize("name", D.SCATTER)
def test_ordered_scatter(name):
    """gad_gemm_dx, epilogue 1, under the mode: dfeat is the float32 sum of the rows in ascending order on top of its initial value,
    daction the initial value plus the float64 sum of the sample's rows in ascending order, bit for bit -- over one run per sample,
    touching and descending point ranges, 600 / 513 groups with cuts inside chunks and on chunk borders, more runs than workgroups,
    empty groups, more group ids than the bounds arrays hold, live counts inside a group / of 0 / inside a sample, 260 feature
    columns, each output alone, one row.  Elements no row reaches keep their initial bits (they are part of the comparison)."""
    out = _scatter_run(name)
    bad = _scatter_gate(name, out)
    assert not bad, "\n".join(bad)
    sens = D.scatter_sensitivity(_scatter_set(name))
    _REPORT.append("A scatter.%-18s -> gemm_dx | %s" % (name, "  ".join(
        "%s bit-equal, control %s" % (k, _frac(*sens[k])) for k in ("dfeat", "daction") if k in out)))


@pytest.mark.parametrize("name", ("samples", "groups600", "live_in_group", "cols260"))
@pytest.mark.parametrize("alter", ("desc", "drop_last", "zero_start"))
def test_scatter_gate_rejects_an_altered_reference(name, alter):
    """negative controls (no kernel is altered): the gate fails the descending-order reference, one without the last live row and
    one that starts from zero in place of the initial values -- in every output the case has"""
    out = _scatter_run(name)
    assert not _scatter_gate(name, out)
    bad = _scatter_gate(name, out, alter)
    assert len(bad) == len(out), "%s %s: the altered reference passed for an output: %s" % (name, alter, bad)


# ----------------------------------------------------------------------------- B. the ordered dW reduce
@functools.lru_cache(maxsize=None)
def _dw_set(name):
    return D.dw_inputs(name)


def _dw_case(c):
    common = dict(stats=False, zout=False, row_w=False, live=c["live"])
    if c["gather"]:
        inp = gc.Fwd(c["rows"], c["Kp"], c["n_out"], gather=dict(feat_c=c["feat_c"], act_c=c["act_c"], gps=c["gps"]),
                     maps={k: c[k] for k in ("row_pt", "row_grp", "npts", "nsmp")},
                     operands={k: c[k] for k in ("feat", "src", "ctr", "action")}, **common)
    else:
        inp = gc.Fwd(c["rows"], c["Kp"], c["n_out"], c_in=c["c_in"], affine=False, relu=0, zin_off=c["zin_off"],
                     operands=dict(zin=c["zin"]), **common)
    assert inp.k_used == c["k_used"]
    dz = gc.Dx(c["rows"], c["n_out"], c["Kp"], c["k_used"], dz_off=c["dz_off"], z=False, relu=0, coef=False, row_w=False,
               live=c["live"], operands=dict(G=c["dZ"]))
    return gc.Dw(inp, dz, row_splits=c["splits"], init=dict(gacc=c["gacc0"]))


@functools.lru_cache(maxsize=None)
def _dw_run(name):
    case = _dw_case(_dw_set(name))
    g = Guarded(case)
    out, route = case.run(DET)
    assert route == "gemm_dw", "%s: routed to %s" % (name, route)
    g.check()
    return _np(out["gacc"])


@pytest.mark.parametrize("name", sorted(D.DW))
def test_ordered_dw_reduce(name):
    """gad_gemm_dw under the mode: the arena is its initial value plus the float64 sum of the splits' (exact) partials in slot order
    -- linear for 3 and 40 splits and for 300 splits over more than 4096 columns, the fixed tree for 300 splits over 72 x 40 --
    bit for bit; splits past the live rows add zeros; two groups of unequal n_out; a gathered input; the three tile shapes;
    row_splits 1 and 0: the exact integer sum, which is all the code promises there.  Words outside the groups' used columns keep
    their initial bits (they are part of the comparison)."""
    c = _dw_set(name)
    got = _dw_run(name)
    bad = _diff("%s gacc" % name, got, D.dw_reference(c))
    assert not bad, bad[0]
    diff, n = D.differs(D.dw_reference(c), D.dw_reference(c, order="desc"), D.dw_mask(c))
    form = "exact integer sum" if c["flat"] else "tree" if max(c["splits"], 1) > 256 and max(c["n_out"]) * c["Kp"] <= 4096 else "linear"
    _REPORT.append("B dw.%-23s -> gemm_dw | gacc bit-equal (%s, row_splits %d), control %s" % (name, form, c["splits"],
                                                                                             _frac(diff, n, not c["flat"])))


@pytest.mark.parametrize("name", ("splits3", "splits300.tree", "splits300.linear", "two_groups"))
def test_dw_gate_rejects_an_altered_reference(name):
    """negative controls: the opposite slot order (for the tree: the tree turned round as well, det_reference.reduce_tree), a dropped
    split, a start from zero; and the other form of the reduce for the two 300-split cases"""
    c, got = _dw_set(name), _dw_run(name)
    assert not _diff(name, got, D.dw_reference(c))
    for alter in (dict(order="desc"), dict(drop_split=1), dict(zero_start=True)):
        assert _diff(name, got, D.dw_reference(c, **alter)), "%s: the reference altered by %s passed" % (name, alter)
    if c["splits"] == 300:
        other = c["gacc0"].copy()
        for g, (n, wo) in enumerate(zip(c["n_out"], c["w_off"])):
            parts = D.dw_partials(c, g)
            s = D.reduce_linear(parts) if name.endswith("tree") else D.reduce_tree(parts)
            other[wo:wo + n * c["Kp"]].reshape(n, c["Kp"])[:, :c["k_used"]] += s
        assert _diff(name, got, other), "%s: the other form of the reduce passed" % name


# ----------------------------------------------------------------------------- C. slot statistics
BIG = 2048 * 64 + 65            # more 64-row tiles than GAD_GX_CAP = 2048: the grid-stride loop (tests/test_gpu_gemm_f64.py, table B)


def _stat_shapes():
    """name -> (kind, factory(**extra keywords)): the shapes of part C, built with random operands by default"""
    t = {}
    t["fwd.two_groups.live130"] = ("fwd", lambda **kw: gc.Fwd(200, 40, [36, 40], c_in=36, extra=True, ones=True, out_off=[0, 36], live=130, **kw))
    t["fwd.two_groups.live0"] = ("fwd", lambda **kw: gc.Fwd(200, 40, [36, 40], c_in=36, extra=True, ones=True, out_off=[0, 36], live=0, **kw))
    t["fwd.tree.r16449"] = ("fwd", lambda **kw: gc.Fwd(16449, 8, [8], c_in=4, extra=True, ones=True, **kw))       # 258 slots over 8 columns
    t["fwd.gridstride"] = ("fwd", lambda **kw: gc.Fwd(BIG, 8, [64], c_in=8, **kw))
    t["dx.two_groups.live130"] = ("dx", lambda **kw: gc.Dx(200, [36, 40], 40, 36, prev=True, live=130, **kw))
    t["dx.live0"] = ("dx", lambda **kw: gc.Dx(200, [72], 40, 36, prev=True, live=0, **kw))
    t["dx.kv20.live130"] = ("dx", lambda **kw: gc.Dx(200, [72], 24, 20, prev=True, live=130, **kw))                # 128 x 32 tile
    t["dx.tree.r16449"] = ("dx", lambda **kw: gc.Dx(16449, [8], 40, 40, prev=True, **kw))                          # 258 slots over 40 columns
    t["dx.gridstride.kv64"] = ("dx", lambda **kw: gc.Dx(BIG, [8], 64, 64, prev=True, **kw))
    return t


STATS = sorted(_stat_shapes())


def _int_case(name):
    """the shape `name` with integer operands: inputs in [-3, 3], weights in [-1, 1], row weights 1 / 2 / 4, no affine, no ReLU, no
    coefficients; dX: identity BatchNorm vectors of the previous layer (mean 0, istd 1, scale 1, shift 0) and an integer zprev"""
    kind, factory = _stat_shapes()[name]
    rng = np.random.default_rng(3000 + STATS.index(name))
    if kind == "fwd":
        case = factory(affine=False, relu=0)
        W = D.ints(rng, (sum(case.n_out), case.Kp), -1, 1)
        W[:, case.k_used:] = 0
        ops = dict(zin=D.ints(rng, tuple(case.zin.shape)), W=W.reshape(-1))
        if case.extra is not None:
            ops["extra"] = D.ints(rng, (case.rows,))
        case = factory(affine=False, relu=0, operands=ops)
    else:
        case = factory(z=False, relu=0, coef=False, row_w=False)
        one, zero = np.ones(case.width, np.float32), np.zeros(case.width, np.float32)
        ops = dict(G=D.ints(rng, tuple(case.G.shape)), W=D.ints(rng, (sum(case.n_out) * case.Kp,), -1, 1),
                   zprev=D.ints(rng, tuple(case.zprev.shape)), pvec=[one, zero, zero, one])
        case = factory(z=False, relu=0, coef=False, row_w=False, operands=ops)
    attr = "stats" if kind == "fwd" else "bst"
    n = getattr(case, attr).numel()
    case.init[attr] = (rng.integers(1, 64, n) * rng.choice([-1, 1], n)) / 8.0      # non-zero, few bits: prefill + integer is exact
    return kind, case, attr


@pytest.mark.parametrize("name", STATS)
def test_slot_statistics_exact(name):
    """stat_sum / stat_sq of the forward and prev_dbeta / prev_dgamma of dX under the mode, with integer operands: every statistic
    is an integer sum below 2^53, exact in any order, and is asserted with ==.  Replica 0 alone receives the sums, on top of its
    pre-filled value; replicas 1 .. R - 1 and the columns no group covers keep their pre-filled bits.  Shapes: two groups (slot
    width max(out_off + n)), live counts inside a tile and of 0, more than 256 slots over few columns (the tree reduce), the
    grid-stride loop, the 128 x 32 dX tile."""
    kind, case, attr = _int_case(name)
    keys = ("stat_sum", "stat_sq") if kind == "fwd" else ("dbeta", "dgamma")
    g = Guarded(case)
    out, route = case.run(DET)
    assert route == "gemm_" + kind
    g.check()
    R, width = gc.R, case.width
    got = _np(getattr(case, attr)).reshape(R, 2, width)
    pre = np.asarray(case.init[attr]).reshape(R, 2, width)
    exp = case.expect()
    # the in-block float32 sums are exact in any order: |w z^2| (|g x_hat|) over a 128-row tile stays below 2^24
    for k in keys:
        assert float(exp[k]["abs"].max()) < 2.0 ** 53
    if case.r and kind == "fwd":                         # terms w z^2 with w <= 4
        zmax = exp["z"]["abs"][:case.r].max().item()
        assert 4 * zmax * zmax * 128 < 2.0 ** 24
    elif case.r:                                         # terms g and g x_hat with |x_hat| <= 3
        assert 3 * exp["gout"]["abs"][:case.r].max().item() * 128 < 2.0 ** 24
    bad = []
    for which, k in enumerate(keys):
        ref = _np(torch.nan_to_num(exp[k]["ref"], nan=0.0))
        assert np.array_equal(ref, np.round(ref))
        if case.r:
            assert np.abs(ref).max() > 0
        bad += _diff("%s %s replica 0" % (name, k), got[0, which], pre[0, which] + ref)
        bad += _diff("%s %s replicas 1 .." % (name, k), got[1:, which], pre[1:, which])
    assert not bad, "\n".join(bad)
    # the launch's other outputs through the float64 gate (integer products: they are exact, the gate must pass)
    rest = {k: v for k, v in exp.items() if k not in keys}
    bad = gc.check(name, out, rest)
    assert not bad, "\n".join(bad)
    _REPORT.append("C stats.%-24s -> gemm_%s | %s == the integer sums on replica 0, replicas 1 .. %d and uncovered columns untouched" % (
        name, kind, " / ".join(keys), R - 1))


def _float_gate(name, case, options, route, tag):
    """the float64 gate of tests/gemm_cases.py on one launch under `options`, and bit-equality of a second launch"""
    out, routed = case.run(options)
    assert routed == route, "%s: routed to %s, expected %s" % (name, routed, route)
    lines = []
    got = case.outputs(out) if hasattr(case, "outputs") else out
    bad = gc.check("%s %s %s -> %s" % (tag, name, " ".join("%s=%d" % kv for kv in sorted(options.items())), routed), got, case.expect(), lines)
    bad += case.exact(out)
    _REPORT.extend(lines)
    assert not bad, "\n".join(bad)
    again, routed = case.run(options)
    assert routed == route
    _same(out, again, "%s: second run" % name)
    return out


@pytest.mark.parametrize("name", STATS)
def test_slot_statistics_random_operands(name):
    """the shapes of test_slot_statistics_exact with the ordinary random operands through the unchanged float64 gate of
    tests/gemm_cases.py (fwd.gridstride and dx.gridstride.kv64 are the cases of table B), and two runs bit-equal"""
    kind, factory = _stat_shapes()[name]
    _float_gate(name, factory(), DET, "gemm_" + kind, "C")


# ----------------------------------------------------------------------------- D. the mode's plumbing
def _plumbing_cases():
    """one case each of A, B and C (each with a device row count, which is what a grid-rows hint acts on), and a call of the same
    kind about 8 x larger with random operands"""
    return {
        "scatter": (lambda: _scatter_case(_scatter_set("live_in_group")), "gemm_dx",
                    lambda: gc.Dx(1500, [24], 16, 13, scatter=dict(feat_c=4, act_c=6, gps=4), live=1400)),
        "dw": (lambda: _dw_case(_dw_set("splits40")), "gemm_dw",
               lambda: gc.Dw(gc.Fwd(10400, 40, [72], c_in=36, stats=False, zout=False, live=10300), gc.Dx(10400, [72], 40, 36, live=10300), row_splits=320)),
        "stats": (lambda: _int_case("fwd.two_groups.live130")[1], "gemm_fwd",
                  lambda: gc.Fwd(1600, 40, [36, 40], c_in=36, extra=True, ones=True, out_off=[0, 36], live=1500)),
    }


@pytest.mark.parametrize("name", sorted(_plumbing_cases()))
def test_result_depends_on_nothing_but_the_arguments(name):
    """one case each of A, B and C: with grid-rows hints of 1, the live count and the capacity; on a second stream; after a call about
    8 x larger on the same stream has grown and dirtied the scratch; after the option was switched off and on again (release,
    reallocate); interleaved with a different case on another stream without synchronisation -- everything bit-equal to the case's
    own first result"""
    factory, route, bigger = _plumbing_cases()[name]
    case = factory()
    first, routed = case.run(DET)
    assert routed == route
    first = {k: v.clone() for k, v in first.items()}

    def again(what, **kw):
        out, routed = case.run(kw.get("options", DET))
        assert routed == route, what
        _same(first, out, "%s: %s" % (name, what))

    for hint in (1, case.r, case.inp.rows if name == "dw" else case.rows):
        case.hint = hint
        try:
            again("grid-rows hint %d" % hint)
        finally:
            case.hint = None
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        again("second stream")
    big = bigger()
    with _mode_on():
        again("inside one session", options={})
        out, routed = big.run({})
        assert routed == route
        again("after a larger call grew and dirtied the scratch", options={})
    again("after the option was switched off and on")
    # two cases on two streams, no synchronisation between the launches
    others = _plumbing_cases()
    other_factory, other_route, _ = others[sorted(others)[(sorted(others).index(name) + 1) % 3]]
    other = other_factory()
    other_first, routed = other.run(DET)
    assert routed == other_route
    other_first = {k: v.clone() for k, v in other_first.items()}
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with _mode_on():
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            o1 = case.launch()
        with torch.cuda.stream(s2):
            o2 = other.launch()
        with torch.cuda.stream(s1):
            o1b = case.launch()
        torch.cuda.synchronize()
    _same(first, o1, "%s: interleaved with another stream" % name)
    _same(first, o1b, "%s: interleaved with another stream, second launch" % name)
    _same(other_first, o2, "%s: the case on the other stream" % name)
    _REPORT.append("D plumbing.%-8s -> %s | hints 1 / live / capacity, second stream, grown scratch, off / on, two streams: bit-equal" % (name, route))


def _bwd_pairs():
    """the smallest mode-0 pairs of tests/test_gpu_gemm_f64_wide.py the fused backward takes: table D (wide) and table E (stream)"""
    from tests import test_gpu_gemm_f64_wide as wide
    L = wide.LIVES[0]
    return {"wide": (lambda later=False: gc.Bwd(gc.Dx(wide.ROWS, [128], 64, 64, prev=True, live=L), later=later), {"bwd_wide": 1}, "gemm_bwd(wide)"),
            "stream": (lambda later=False: gc.Bwd(wide._sdx(64, None), later=later), dict(wide.F32), "gemm_bwd(stream)")}


@pytest.mark.parametrize("name", ("wide", "stream"))
def test_gemm_bwd_under_the_mode(name):
    """gad_gemm_bwd on a pair its wide / streaming route takes by default: under the mode the route is the tile kernels (gad_gemm_dw
    then gad_gemm_dx), the results pass the float64 gate, two runs are bit-equal; with row_splits = GAD_DW_REDUCE_LATER dW is
    already complete when the call returns and a following gad_gemm_dw_reduce leaves the arena bit-unchanged"""
    factory, options, fused_route = _bwd_pairs()[name]
    case = factory()
    _, routed = case.run(options)
    assert routed == fused_route, "%s: the pair is not eligible for the fused route it is named for (%s)" % (name, routed)
    options = dict(options, **DET)
    out = _float_gate("bwd." + name, case, options, "gemm_dx", "D")
    later = factory(later=True)
    hip = _hip()
    try:
        for k, v in options.items():
            hip.set_option(k, v)
        later.dx.prepare()
        later.dw.prepare()
        ax, aw = later.dx.args(), later.dw.args()
        aw.row_splits = gc.DW_REDUCE_LATER
        later.call("gad_gemm_bwd", ax, aw)
        assert hip.lib().gad_last_kernel().decode() == "gemm_dx"
        torch.cuda.synchronize()
        before = later.dx.collect()
        before.update(later.dw.collect())
        later.call("gad_gemm_dw_reduce", ax, aw)
        torch.cuda.synchronize()
        after = later.dw.collect()
    finally:
        for k in options:
            hip.set_option(k, gc._default(k))
    _same(out, before, "bwd.%s: GAD_DW_REDUCE_LATER under the mode" % name)
    _same({"gacc": before["gacc"]}, {"gacc": after["gacc"]}, "bwd.%s: gad_gemm_dw_reduce after an unfused call" % name)


def test_mode2_forward_is_refused():
    """a mode-2 forward (the 64-channel input recomputed from the gathered rows) has no deterministic form: GAD_ERR_UNSUPPORTED,
    the message names the option, nothing is written"""
    from tests import test_gpu_gemm_f64_wide as wide
    case = gc.Fwd(wide.SROWS, 64, [64], c_in=64, gather=dict(feat_c=4), pre_Kp=8, live=wide.SLIVE)
    case.init["stats"] = np.arange(1, case.stats.numel() + 1) / 8.0
    g = Guarded(case)
    hip = _hip()
    try:
        hip.set_option("deterministic", 1)
        case.zout.fill_(float("nan"))
        case.stats.copy_(torch.from_numpy(case.init["stats"]))
        status = hip.lib().gad_gemm_fwd(ctypes.byref(case.args()), hip.stream())
        message = hip.lib().gad_last_error().decode()
        torch.cuda.synchronize()
    finally:
        hip.set_option("deterministic", hip.get_option_default("deterministic"))
    assert status == UNSUPPORTED, (status, message)
    assert "\"deterministic\"" in message and "mode 2" in message, message
    g.check()
    assert bool(torch.isnan(case.zout).all()), "zout was written"
    assert np.array_equal(_np(case.stats), case.init["stats"]), "the statistics were written"
    out, routed = case.run(dict(wide.F32))               # the same call is served once the option is off
    assert routed == "gemm_fwd(stream)"
