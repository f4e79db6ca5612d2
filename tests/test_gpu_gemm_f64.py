"""float64 gates of the layer GEMMs' skinny routes (A), generic 64 x 64 / 128 x 32 / 32 x 128 tile routes (B) and SA1 first-layer
streaming routes (C): one launch per case through the C entry point, compared with tests/gemm_reference.py (float64; pinned to
torch autograd by tests/test_gemm_reference.py).  The gate and its derivation: tests/gemm_cases.py.  Every case asserts the route it
took (gad_last_kernel): a gate that silently ran another kernel would be worthless.  Shapes are the smallest at which each path can
still go wrong; layer shapes named "head" / "critic" are those of ga_ddpg_amd/heads.py (512 features + time + bias -> 768 =
3 x 256 -> 3 x 256 -> [1, 1, 7]; the policy head ends in 6 + 7).

GAD_GEMM_F64_REPORT=<file>: the measured worst err / bound and the mean-error ratio against torch's float32 evaluation of every case
and output are written there (profiles/gemm_f64_gates.txt is that file from an MI355X run)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_REPORT = []


class _Cases(object):
    """tests.gemm_cases, imported when a case is built (collection must not need the library)"""

    def __getattr__(self, k):
        from tests import gemm_cases
        return getattr(gemm_cases, k)


gc = _Cases()


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    path = os.environ.get("GAD_GEMM_F64_REPORT")
    if path and _REPORT:
        with open(path, "w") as f:
            f.write("# float64 gates of the skinny / tile / SA1 first-layer GEMM routes (tests/test_gpu_gemm_f64.py)\n"
                    "# case [options] -> route | output, T, worst err / ((T + 2) * 2^-24 * abs_bound), mean |err|, the same for torch's float32\n"
                    "# evaluation of the identical operands, their ratio (gate: 1.5 x + floor), the floor.  ABOVE 1.5 x: a case listed and\n"
                    "# explained in ORDER_COST of the test -- one accumulation chain per element against a matmul that splits K -- held to\n"
                    "# 1.5 x torch's float32 evaluation in one chain instead\n")
            f.write("\n".join(_REPORT) + "\n")


OFFS = [0, 256, 512]


def _head_rows():
    return (24, 32, 33, 64, 1024)


def _fwd_cases():
    c = {}
    for r in _head_rows() + (1025,):
        c["fwd.head_l1.r%d" % r] = lambda r=r: gc.Fwd(r, 520, [72], c_in=512, extra=True, ones=True)
    c["fwd.head_l1.plain.r33"] = lambda: gc.Fwd(33, 520, [72], c_in=512, extra=True, ones=True, affine=False, relu=0)
    c["fwd.critic_l2.r33"] = lambda: gc.Fwd(33, 264, [256] * 3, c_in=256, ones=True, zin_off=OFFS, out_off=OFFS, affine=False)
    c["fwd.critic_l3.r33"] = lambda: gc.Fwd(33, 264, [1, 1, 7], c_in=256, ones=True, zin_off=OFFS, out_off=[0, 1, 2], zout_pitch=9, affine=False)
    c["fwd.kp8.r33"] = lambda: gc.Fwd(33, 8, [40], c_in=4, extra=True, ones=True, zout_pitch=44)
    c["fwd.kp40.r33"] = lambda: gc.Fwd(33, 40, [40], c_in=36, extra=True, ones=True, zout_pitch=44)
    c["fwd.kp1152.r33"] = lambda: gc.Fwd(33, 1152, [40], c_in=1024, extra=True, ones=True)
    c["fwd.kp1160.r33"] = lambda: gc.Fwd(33, 1160, [40], c_in=1024, extra=True, ones=True)
    c["fwd.fc_1024_512.stats.r64"] = lambda: gc.Fwd(64, 1024, [512], c_in=1024)
    c["fwd.fc_1024_512.in_stat.r33"] = lambda: gc.Fwd(33, 1024, [512], c_in=1024, in_stat=True)
    return c


def _dx_cases():
    c = {}
    for r in _head_rows() + (1025,):
        c["dx.head_l1.r%d" % r] = lambda r=r: gc.Dx(r, [768], 520, 512, relu=1, premasked=0, coef=False, row_w=False, prev=True)
    c["dx.critic_l2.r33"] = lambda: gc.Dx(33, [256] * 3, 264, 256, dz_off=OFFS, gout_off=OFFS, relu=1, premasked=0, coef=False, row_w=False)
    c["dx.n36_k40.r33"] = lambda: gc.Dx(33, [36], 40, 40)
    c["dx.n12_znull.r33"] = lambda: gc.Dx(33, [12], 264, 256, z=False, relu=0, coef=False, row_w=False)
    return c


def _critic_dw(r, layer, **kw):
    if layer == 3:          # n_out [1, 1, 7], dz_off [0, 1, 2], g_pitch 9: not vectorisable
        inp = gc.Fwd(r, 264, [1, 1, 7], c_in=256, ones=True, zin_off=OFFS, affine=False, stats=False, zout=False, row_w=False)
        dz = gc.Dx(r, [1, 1, 7], 264, 256, dz_off=[0, 1, 2], g_pitch=9, z=False, relu=0, coef=False, row_w=False)
    elif layer == 2:
        inp = gc.Fwd(r, 264, [256] * 3, c_in=256, ones=True, zin_off=OFFS, affine=False, stats=False, zout=False, row_w=False)
        dz = gc.Dx(r, [256] * 3, 264, 256, dz_off=OFFS, relu=1, premasked=0, coef=False, row_w=False)
    else:
        inp = gc.Fwd(r, 520, [768], c_in=512, extra=True, ones=True, stats=False, zout=False, row_w=False)
        dz = gc.Dx(r, [768], 520, 512, relu=1, premasked=0, coef=False, row_w=False)
    return gc.Dw(inp, dz, **kw)


def _dw_cases():
    c = {}
    for r in _head_rows() + (1025,):
        c["dw.critic_l2.r%d" % r] = lambda r=r: _critic_dw(r, 2)
    c["dw.critic_l3.r33"] = lambda: _critic_dw(33, 3)
    c["dw.critic_l1.r33"] = lambda: _critic_dw(33, 1)
    return c


def _table_a():
    """name -> (factory, options, route)"""
    t = {}
    for kind, cases in (("fwd", _fwd_cases()), ("dx", _dx_cases()), ("dw", _dw_cases())):
        for name, f in cases.items():
            tile = name.endswith("r1025") or "kp1160" in name
            t[name] = (f, {}, "gemm_%s" % kind if tile else "gemm_%s(skinny)" % kind)
    for name in ("fwd.head_l1.r33", "dx.head_l1.r33", "dw.critic_l2.r33"):
        t[name + ".nw4"] = (t[name][0], {"skinny_nw": 4}, t[name][2])
    return t


def _table_b():
    t = {}
    # fallback forms: every case of A on the tile kernels
    for name, (f, opts, route) in _table_a().items():
        if "nw4" in name or "(skinny)" not in route:
            continue
        kind = name.split(".")[0]
        t[name + ".tile"] = (f, {kind + "_skinny": 0}, "gemm_" + kind)
    L = dict(live=130)
    # device row count (static 200, live 130 / 0), reduction tail Kp 40 (KT = 32), tile shapes
    t["fwd.live130.n72"] = (lambda: gc.Fwd(200, 40, [72], c_in=36, extra=True, ones=True, zout_pitch=76, **L), {}, "gemm_fwd")
    t["fwd.live130.n9"] = (lambda: gc.Fwd(200, 40, [9], c_in=36, extra=True, ones=True, zout_pitch=13, **L), {}, "gemm_fwd")
    t["fwd.live0"] = (lambda: gc.Fwd(200, 40, [72], c_in=36, extra=True, ones=True, live=0), {}, "gemm_fwd")
    t["dx.live130.n72"] = (lambda: gc.Dx(200, [72], 40, 36, prev=True, **L), {}, "gemm_dx")
    t["dx.live130.kv20"] = (lambda: gc.Dx(200, [72], 24, 20, prev=True, **L), {}, "gemm_dx")
    t["dx.live0"] = (lambda: gc.Dx(200, [72], 40, 36, prev=True, live=0), {}, "gemm_dx")
    def dw(n_out, c_in, Kp, live=130, rows=200, **kw):
        inp = gc.Fwd(rows, Kp, n_out, c_in=c_in, extra=True, ones=True, stats=False, zout=False, live=live)
        return gc.Dw(inp, gc.Dx(rows, n_out, Kp, c_in, live=live), **kw)
    t["dw.live130.n9"] = (lambda: dw([9], 36, 40), {}, "gemm_dw")                       # nmax <= 32: 32 x 128
    t["dw.live130.k22"] = (lambda: dw([72], 20, 24), {}, "gemm_dw")                     # k_used <= 32: 128 x 32
    t["dw.live130.n72"] = (lambda: dw([72], 36, 40), {}, "gemm_dw")                     # neither: 64 x 64
    t["dw.live0"] = (lambda: dw([72], 36, 40, live=0), {}, "gemm_dw")
    for rs in (0, 1, 3):
        t["dw.splits%d.partial" % rs] = (lambda rs=rs: dw([72], 36, 40, live=700, rows=800, row_splits=rs), {}, "gemm_dw")
        t["dw.splits%d.atomics" % rs] = (lambda rs=rs: dw([72], 36, 40, live=700, rows=800, row_splits=rs, partial=False), {}, "gemm_dw")
    # gathered input (mode 1)
    t["fwd.gather.kp8"] = (lambda: gc.Fwd(200, 8, [72], gather=dict(feat_c=4), **L), {}, "gemm_fwd")
    t["fwd.gather.kp16.action"] = (lambda: gc.Fwd(200, 16, [72], gather=dict(feat_c=4, act_c=6, gps=4), **L), {}, "gemm_fwd")
    t["fwd.gather.kp16.noctr"] = (lambda: gc.Fwd(200, 16, [72], gather=dict(feat_c=4, act_c=6, gps=4, ctr=False), **L), {}, "gemm_fwd")
    t["fwd.gather.kp136"] = (lambda: gc.Fwd(2100, 136, [128], gather=dict(feat_c=128), live=2049), {"fwd_wide": 0}, "gemm_fwd")
    # fused max-pool
    t["fwd.pool.n64"] = (lambda: gc.Fwd(260, 64, [64], c_in=64, pool=dict(gsz=4)), {}, "gemm_fwd")
    t["fwd.pool.n128"] = (lambda: gc.Fwd(260, 64, [128], c_in=64, pool=dict(gsz=4)), {}, "gemm_fwd")
    t["fwd.pool.n64.gamma"] = (lambda: gc.Fwd(260, 64, [64], c_in=64, pool=dict(gsz=4, gamma="mixed")), {}, "gemm_fwd")
    t["fwd.pool.n64.nozout"] = (lambda: gc.Fwd(260, 64, [64], c_in=64, pool=dict(gsz=4, gamma="mixed"), zout=False), {}, "gemm_fwd")
    # dX: scalar loads (g_pitch 9 / 13, z NULL), scatter epilogue
    t["dx.scalar.g9"] = (lambda: gc.Dx(200, [1, 1, 7], 264, 256, dz_off=[0, 1, 2], gout_off=OFFS, g_pitch=9, z=False, relu=0, coef=False,
                                       row_w=False, **L), {}, "gemm_dx")
    t["dx.scalar.g13"] = (lambda: gc.Dx(200, [6, 7], 264, 256, dz_off=[0, 6], gout_off=[0, 256], g_pitch=13, z=False, relu=0, coef=False,
                                        row_w=False, **L), {}, "gemm_dx")
    t["dx.scatter"] = (lambda: gc.Dx(200, [72], 16, 13, scatter=dict(feat_c=4, act_c=6, gps=4), **L), {}, "gemm_dx")
    t["dx.scatter.dfeat_only"] = (lambda: gc.Dx(200, [72], 8, 7, scatter=dict(feat_c=4), **L), {}, "gemm_dx")
    # grid-stride loop: more row tiles than GAD_GX_CAP = 2048.  The forward (n_out 64) and a dX with k_valid > 32 take 64-row tiles:
    # 2050 of them; the dX with Kp 8 / n_out 64 (k_valid <= 32) takes 128-row tiles (1025: no loop), kept as the issue states it
    big = 2048 * 64 + 65
    t["fwd.gridstride"] = (lambda: gc.Fwd(big, 8, [64], c_in=8), {}, "gemm_fwd")
    t["dx.gridstride.kp8"] = (lambda: gc.Dx(big, [64], 8, 8, prev=True), {}, "gemm_dx")
    t["dx.gridstride.kv64"] = (lambda: gc.Dx(big, [8], 64, 64, prev=True), {}, "gemm_dx")
    return t


def _table_c():
    rows, live = 32768 + 1000, 32768 + 37
    t = {}
    g8, g16 = dict(feat_c=4), dict(feat_c=4, act_c=6, gps=4)
    for name, gth, Kp in (("kp8", g8, 8), ("kp16", g16, 16)):
        t["fwd.stream.gather." + name] = (lambda gth=gth, Kp=Kp: gc.Fwd(rows, Kp, [64], gather=gth, live=live), {}, "gemm_fwd(stream)")
        t["dw.gather_stream." + name] = (lambda gth=gth, Kp=Kp: gc.Dw(
            gc.Fwd(rows, Kp, [64], gather=gth, live=live, stats=False, zout=False),
            gc.Dx(rows, [64], Kp, gth["feat_c"] + 3 + gth.get("act_c", 0), dscale=True, live=live)), {}, "gemm_dw(gather stream)")
    act = dict(feat_c=4, act_c=6, gps=4, dfeat=False)
    t["dx.action_stream"] = (lambda: gc.Dx(rows, [64], 16, 13, scatter=act, live=live), {}, "gemm_dx(action stream)")
    t["dx.action_stream.bn"] = (lambda: gc.Dx(rows, [64], 16, 13, scatter=act, live=live, bn=True), {}, "gemm_dx(action stream)")
    for N in (64, 128):
        for src, pooled in (("dense", None), ("pooled", dict(gsz=4))):
            f = lambda N=N, pooled=pooled: gc.Dw(gc.Fwd(rows, 64, [N], c_in=64, live=live, stats=False, zout=False),
                                                 gc.Dx(rows, [N], 64, 64, dscale=True, pooled=pooled, live=live))
            t["dw.stream.n%d.%s" % (N, src)] = (f, {}, "gemm_dw(stream)")
            t["dw.stream.n%d.%s.f32" % (N, src)] = (f, {"mfma_split": 0}, "gemm_dw(stream)")
    return t


A, B, C = sorted(_table_a()), sorted(_table_b()), sorted(_table_c())
# Cases whose mean error lands ABOVE 1.5 x torch's float32 matmul (profiles/gemm_f64_gates.txt, MI355X; the ratio measured is
# given).  All are the generic tile kernels on a long reduction (514 .. 1026 products): gemm_fwd_kernel / gemm_dx_kernel keep one
# set of MFMA accumulators across all K-tiles, so every element is ONE chain of K rounded additions, whose error grows like
# sqrt(K) * u.  torch's matmul is no fixed yardstick here: for the same K its mean error is 6.6e-8 at 24, 33 and 64 rows but 1.2e-7
# at 32 and 1024 rows (dx.head_l1: the library picks a kernel that splits K at some shapes and one chain at others), and wherever
# it runs one chain the tile kernels sit at 0.99 .. 1.00 x of it (fwd.head_l1.r24 / r32 / r33 / r64.tile, dx.head_l1.r32 /
# r1024.tile).  The skinny kernels, which split K over 8 wavefronts, sit at 0.44 .. 0.82 x for the same reason.  The margin is not
# widened: for exactly these outputs a mean error above 1.5 x the matmul's must instead be within 1.5 x of torch's float32
# evaluation of the same operands in one chain (gemm_cases.chain32) -- the explanation is what is asserted -- and the derived
# per-element bound, which no order of summation may exceed, holds for them as for every other case (worst 0.009).
ORDER_COST = {
    "fwd.head_l1.r1025": ("z",),                       # 1.71
    "fwd.head_l1.r1024.tile": ("z",),                  # 1.71
    "fwd.kp1160.r33": ("z",),                          # 1.60
    "fwd.kp1152.r33.tile": ("z",),                     # 1.80
    "fwd.fc_1024_512.stats.r64.tile": ("z",),          # 1.79
    "fwd.fc_1024_512.in_stat.r33.tile": ("z",),        # 1.77
    "dx.head_l1.r24.tile": ("gout",),                  # 1.75
    "dx.head_l1.r33.tile": ("gout",),                  # 1.75
    "dx.head_l1.r64.tile": ("gout",),                  # 1.77
}
DET = {"fwd.live130.n72": "fwd", "dx.scatter": "dx", "dw.splits3.partial": "dw", "dx.live130.n72": "dx"}


def _nan_equal(a, b):
    return torch.equal(torch.nan_to_num(a.double(), nan=-7.25), torch.nan_to_num(b.double(), nan=-7.25))


def _gate(table, name, extra_options=None, tag=""):
    factory, options, route = table[name]
    options = dict(options, **(extra_options or {}))
    case = factory()
    out, routed = case.run(options)
    assert routed == route, "%s: routed to %s, expected %s" % (name, routed, route)
    got = case.outputs(out) if hasattr(case, "outputs") else out
    label = "%s%s %s -> %s" % (name, tag, " ".join("%s=%d" % kv for kv in sorted(options.items())), routed)
    bad = gc.check(label, got, case.expect(), _REPORT, chain_keys=ORDER_COST.get(name, ()))
    bad += case.exact(out)
    if getattr(case, "in_stat", False):
        bad += case.check_in_stat(out)
    if getattr(case, "bn", False) or getattr(getattr(case, "dz", None), "bn", False):
        bad += (case if hasattr(case, "check_bn") else case.dz).check_bn(out)
    assert not bad, "\n".join(bad)
    return case, out


@pytest.mark.parametrize("name", A)
def test_skinny_routes(name):
    """A: gemm_fwd(skinny) / gemm_dx(skinny) / gemm_dw(skinny) at 24, 32, 33, 64 and 1024 rows (a single live row in the second row tile,
    exact multiples, the last size the route takes), 1025 rows and Kp 1160 (must fall to the tile kernels), the head's layer shapes,
    three groups, the K-split edges (Kp 8: seven wavefronts without a share; Kp = SK_KCAP), statistics, the input layer's BatchNorm
    finalised in the prologue, and the 4-wavefront instantiation"""
    _gate(_table_a(), name)


@pytest.mark.parametrize("name", B)
def test_tile_routes(name):
    """B: gemm_fwd / gemm_dx / gemm_dw (the fallback of every shape): every skinny case again on the tile kernels, a device row count
    that ends inside a tile and one of 0, a partial last K-tile, the three tile shapes, the gathered input, the fused max-pool, scalar
    loads, the scatter epilogue, atomic / partial-slab dW with 0 / 1 / 3 row splits, the grid-stride loop"""
    _gate(_table_b(), name)


@pytest.mark.parametrize("name", C)
def test_sa1_first_layer_streaming_routes(name):
    """C: the gathered streaming forward (Kp 8 / 16), gemm_dw(gather stream), gemm_dx(action stream) (with and without the bn_* block)
    and the unfused gemm_dw(stream), at the smallest row count the route predicates take (>= 32768), live rows ending inside a slab"""
    _gate(_table_c(), name)


@pytest.mark.parametrize("name", sorted(DET))
def test_deterministic_mode(name):
    """option "deterministic": the slot-statistics forward, det_dx_launch (statistics slots; the ordered scatter) and the ordered dW
    reduce pass the same gates, and two runs are bit-equal"""
    table = _table_b()
    case, out = _gate(table, name, {"deterministic": 1}, tag=" det")
    again, routed = case.run(dict(table[name][1], deterministic=1))
    assert routed == table[name][2]
    for k, v in out.items():
        assert _nan_equal(v, again[k]), "%s: %s differs between two deterministic runs" % (name, k)


NEG = [(e, a) for e in ("fwd", "dx", "dw") for a in ("no_bias", "no_extra", "drop_last_row_stats", "shift_out_off")]


@pytest.mark.parametrize("entry,alter", NEG)
def test_gate_rejects_an_altered_reference(entry, alter):
    """negative controls (no kernel is altered): the gate must fail a reference without the bias column, without the `extra` column,
    with the last live row dropped from the row sums (statistics; for dW, the sum over rows IS the output), and with one group's
    output offset shifted by 4 -- and pass the unaltered one.  dX: k_valid covers the extra and bias columns of the layer below, whose
    gradient columns are the ones removed."""
    if entry == "fwd":
        case = gc.Fwd(33, 40, [36, 40], c_in=36, extra=True, ones=True, zin_off=[0, 36], zout_pitch=84)
    elif entry == "dx":
        case = gc.Dx(33, [36, 40], 40, 38, g_pitch=84, prev=True)
    else:
        case = gc.Dw(gc.Fwd(33, 40, [36, 40], c_in=36, extra=True, ones=True, zin_off=[0, 36], stats=False, zout=False),
                     gc.Dx(33, [36, 40], 40, 36, g_pitch=84))
    out, _ = case.run()
    got = case.outputs(out) if hasattr(case, "outputs") else out
    assert not gc.check("control", got, case.expect())
    bad = gc.check("altered", got, case.expect(alter))
    assert bad, "the gate accepted a reference with alteration '%s'" % alter
    if alter == "drop_last_row_stats" and entry != "dw":
        assert all(("stat" in b or "dbeta" in b or "dgamma" in b) for b in bad), bad


def test_dx_accumulate_is_refused_with_groups():
    """gad_gemm_dx_args.accumulate (groups adding into shared gout columns) is not implemented: more than one group with it set is
    GAD_ERR_UNSUPPORTED with a message that names the field; one group ignores it"""
    case = gc.Dx(33, [256] * 3, 264, 256, dz_off=OFFS, gout_off=[0, 0, 0], relu=1, premasked=0, coef=False, row_w=False)
    case.accumulate = 1
    with pytest.raises(RuntimeError, match=r"status -4.*accumulate"):
        case.run()
    assert bool(torch.isnan(case.gout).all()), "a refused call wrote gout"
    one = gc.Dx(33, [36], 40, 40)
    one.accumulate = 1
    out, routed = one.run()
    assert routed == "gemm_dx(skinny)" and not gc.check("accumulate, one group", out, one.expect())
