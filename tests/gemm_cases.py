"""Single-launch cases for the layer GEMM entry points (gad_gemm_fwd / gad_gemm_dx / gad_gemm_dw / gad_gemm_bwd) on their skinny,
generic-tile, wide-tile and SA1 streaming routes, and the float64 gate they are held to (tests/test_gpu_gemm_f64.py: skinny, tile,
SA1 first layer; tests/test_gpu_gemm_f64_wide.py: wide tile, SA1 layers 2 / 3, the fused backward, the grid-rows hint).  The case
classes follow tests/split_cases.Case: the argument block is built through engine._fwd_args / _dz / _ptr, the C entry point is called
once, clones of the outputs come back; the references are tests/gemm_reference.py (pinned to torch autograd by tests/test_gemm_reference.py).

The gate, per output element: with u = 2**-24 and T the number of float32 terms behind the element,
    |got - ref| <= (T + 2) * u * abs_bound + 1e-30,
abs_bound = the sum of |terms| in float64 -- the textbook worst case of a length-T float32 sum in ANY order (MFMA, FMA, split-K
partials alike; Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: gamma_T ~ T * u), which no correct kernel
exceeds, while a missing or duplicated term is ~ abs_bound / T.  T of every output is stated where its Spec is built.  The mean error
is held against a float32 baseline that is not code under test (torch's own float32 matmul / reduction of the identical
operands): mean |got - ref| <= 1.5 x the baseline's + floor, the floors of tests/test_gpu_split_families.check_case."""
import ctypes as C

import torch

from ga_ddpg_amd import hip
from ga_ddpg_amd.engine import _dz, _fwd_args, _ptr
from tests import gemm_reference as gr

U = 2.0 ** -24
MARGIN = 1.5
R = hip.STAT_REPLICAS
# library defaults of every switch a case may change (restored in `finally`)
OPTION_DEFAULTS = {"fwd_skinny": 1, "dx_skinny": 1, "dw_skinny": 1, "skinny_nw": 8, "fwd_wide": 1, "dx_wide": 1, "dw_wide": 1,
                   "fwd_stream": 1, "dx_stream": 1, "dw_stream": 1, "deterministic": 0,
                   "bwd_wide": 0, "bwd_fused": 1, "bwd_wide_slab": 4, "dw_wide_wgs": 256, "fwd_stream_wgs": 256, "fwd_stream_l1_wgs": 256,
                   "bwd_stream_wgs": 256, "fwd_bn_prologue": 1, "mfma_split": 1}


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _default(name):
    return hip.get_option_default(name) if name in ("mfma_split", "deterministic") else OPTION_DEFAULTS[name]


def _supplied(v, dev):
    """a caller-supplied array (numpy or torch) as a contiguous device tensor of its own dtype"""
    t = v if torch.is_tensor(v) else torch.from_numpy(v)
    return t.to(dev).contiguous()


def _supply(case, operands, dev):
    """caller-supplied operands: every entry replaces the case's drawn tensor of that name (shape and dtype are the caller's to get
    right: the drawn one is asserted against); `pvec`: the list of the previous layer's four vectors"""
    for k, v in (operands or {}).items():
        if isinstance(v, (list, tuple)):
            new = [_supplied(x, dev) for x in v]
            assert [tuple(x.shape) for x in new] == [tuple(x.shape) for x in getattr(case, k)], k
        else:
            new = _supplied(v, dev)
            old = getattr(case, k)
            assert old is not None and tuple(new.shape) == tuple(old.shape) and new.dtype == old.dtype, (k, new.shape, new.dtype)
        setattr(case, k, new)


def _prefill(t, init):
    """what an accumulator holds before the launch: zeros, or the caller's initial values"""
    if init is None:
        t.zero_()
    else:
        t.copy_(_supplied(init, t.device).reshape(t.shape))


def matmul32(a, b):
    """torch's float32 matmul (no TF32): the baseline that is not code under test"""
    was = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        return a.float() @ b.float()
    finally:
        torch.backends.cuda.matmul.allow_tf32 = was


def chain32(a, b):
    """a @ b^T in float32 as ONE accumulation chain per element, k ascending, one multiply-add per step, by torch's elementwise
    kernels: the order of summation of a tile kernel that keeps its accumulators across the K-tiles (not code under test)"""
    a, b = a.float(), b.float()
    acc = torch.zeros(a.shape[0], b.shape[0], device=a.device)
    for k in range(a.shape[1]):
        acc = torch.addcmul(acc, a[:, k:k + 1], b[None, :, k])
    return acc


def spec(ref, ab, T, base=None, reduced=False, slack=None, chain=None):
    """chain: callable -> the single-chain float32 evaluation of the same output (built only when the gate asks for it)"""
    return {"ref": ref, "abs": ab, "T": T, "base": base, "reduced": reduced, "slack": slack, "chain": chain}


def check(name, got, exp, report=None, chain_keys=()):
    """-> list of failures (empty: every output of `got` is inside the gate of its Spec in `exp`).  Elements whose reference is NaN
    are elements the launch must not write: they must still hold the NaN they were given.
    chain_keys: outputs of a case listed in tests/test_gpu_gemm_f64.ORDER_COST.  The margin over torch's float32 matmul stays 1.5 x
    for them too; where such an output lands above it, the stated cause -- the kernel sums every element in one chain where torch's
    matmul of that shape splits K -- is itself put to the test: the mean error must be within 1.5 x of torch's float32 evaluation
    of the identical operands in one chain (chain32), and the line of the table says so."""
    bad = []
    for k, s in exp.items():
        ref, g = s["ref"], got[k].double()
        if g.shape != ref.shape:
            bad.append("%s %s: shape %s, reference %s" % (name, k, tuple(g.shape), tuple(ref.shape)))
            continue
        live = ~torch.isnan(ref)
        if not bool(torch.isnan(g[~live]).all()):
            bad.append("%s %s: %d elements outside the launch's columns / rows were written" % (name, k, int((~torch.isnan(g[~live])).sum())))
        if not bool(live.any()):
            continue
        if bool(torch.isnan(g[live]).any()):
            bad.append("%s %s: %d elements left unwritten (NaN)" % (name, k, int(torch.isnan(g[live]).sum())))
            continue
        err = (g - ref).abs()[live]
        ab = s["abs"][live]
        bound = (s["T"] + 2) * U * ab + 1e-30
        if s["slack"] is not None:
            bound = bound + s["slack"][live]
        worst = float((err / bound).max())
        mean = float(err.mean())
        floor = 4e-9 * float(ab.max()) if s["reduced"] else 1e-9 * float(ref[live].abs().max())
        mbase = float((s["base"].double() - ref).abs()[live].mean()) if s["base"] is not None else float("nan")
        line = "%-44s %-9s T %6d  err/bound %.4f  mean %.3e  torch-f32 mean %.3e  ratio %6.3f  floor %.1e" % (
            name, k, s["T"], worst, mean, mbase, mean / mbase if mbase > 0 else float("nan"), floor)
        if worst > 1.0:
            bad.append("%s %s: derived bound exceeded, worst err / bound %.3f (T = %d)" % (name, k, worst, s["T"]))
        if s["base"] is not None and mean > MARGIN * mbase + floor:
            if k in chain_keys and s["chain"] is not None:
                mchain = float((s["chain"]().double() - ref).abs()[live].mean())
                line += "  ABOVE 1.5 x: order of summation -- torch-f32 one chain mean %.3e  ratio %6.3f" % (mchain, mean / mchain)
                if mean > MARGIN * mchain + floor:
                    bad.append("%s %s: mean error %.3e beyond %.1f x torch float32 in one chain %.3e + floor %.1e" % (name, k, mean, MARGIN, mchain, floor))
            else:
                bad.append("%s %s: mean error %.3e beyond %.1f x torch float32 %.3e + floor %.1e" % (name, k, mean, MARGIN, mbase, floor))
        if report is not None:
            report.append(line)
    return bad


class Case(object):
    """one launch: run(options) -> (outputs, route); expect() -> {key: Spec} (after run: a launch may publish vectors the reference reads)"""
    entry = None
    hint = None          # a host int: handed to gad_grid_rows_hint right before the launch, on the launching thread

    def call(self, name, *structs):
        """the entry point `name` on the argument blocks `structs`, with the case's grid-rows hint in front of it"""
        if self.hint is not None:
            h = C.c_int32(int(self.hint))
            hip.check(hip.lib().gad_grid_rows_hint(C.byref(h), hip.stream()), "gad_grid_rows_hint")
        hip.sync_deterministic()
        hip.check(getattr(hip.lib(), name)(*([C.byref(x) for x in structs] + [hip.stream()])), name)

    def run(self, options=None):
        options = dict(options or {})
        try:
            for k, v in options.items():
                hip.set_option(k, v)
            out = self.launch()
            route = hip.lib().gad_last_kernel().decode()
            torch.cuda.synchronize()
        finally:
            for k in options:
                hip.set_option(k, _default(k))
        return out, route


def _group_max(t, G, gs, fill):
    """(rows <= G * gs, C) -> (G, C): the maximum over every run of gs rows, the rows the last run lacks counting as `fill`"""
    pad = torch.full((G * gs - t.shape[0], t.shape[1]), fill, dtype=t.dtype, device=t.device)
    return torch.cat([t, pad]).view(G, gs, -1).max(1).values


def _with_rows(case, rows, fn):
    """fn() with the case's live row count set to `rows`"""
    was = case.r
    case.r = rows
    try:
        return fn()
    finally:
        case.r = was


def _replica_sum(buf, width, which):
    return buf.view(R, 2, width)[:, which].sum(0).clone()


# ----------------------------------------------------------------------------------------------------------------- forward
class Fwd(Case):
    """gad_gemm_fwd.  ACT input (c_in channels of zin at zin_off[g], optional affine + ReLU, `extra` column at c_in, bias column after
    it) or GATHER input (gather = dict(feat_c, act_c, gps, ctr)); groups through zin_off / out_off / n_out; live: device row count
    (rows = the static bound); pool = dict(gsz, gamma): the fused max-pool; in_stat: the input layer's BatchNorm finalised by the launch.
    split: the call carries the forward split-bf16 mirror of W (split_cases.Mirror; one group).  pre_Kp (with gather and c_in): mode 2,
    the c_in-channel ACT input recomputed from the gathered rows and pre_W (c_in, pre_Kp), then scale / shift / ReLU.
    Hooks (tests/test_gpu_deterministic_kernels.py; the drawn operands of a case without them are unchanged): maps = dict(row_pt,
    row_grp, npts, nsmp): the caller's row maps of a gathered input; operands = {attribute: array}: replaces drawn tensors of the
    same shape and dtype; init = {"stats": array}: what the statistics hold before the launch in place of zeros."""
    entry = "gad_gemm_fwd"

    def __init__(self, rows, Kp, n_out, c_in=None, extra=False, ones=False, affine=True, relu=1, zin_off=None, out_off=None,
                 zout_pitch=None, stats=True, row_w=True, live=None, gather=None, pool=None, in_stat=False, zout=True, seed=1,
                 w_scale=0.05, split=False, pre_Kp=None, maps=None, operands=None, init=None):
        dev = torch.device("cuda")
        g = _gen(seed)
        self.init = dict(init or {})
        self.rows, self.Kp, self.n_out, self.ng = rows, Kp, list(n_out), len(n_out)
        self.r = rows if live is None else live
        self.nrows = None if live is None else torch.tensor([live], dtype=torch.int32, device=dev)
        self.gather, self.pool, self.in_stat, self.has_stats, self.has_zout = gather, pool, in_stat, stats, zout
        self.relu, self.affine = relu, affine
        self.pre_Kp, self.mirror = pre_Kp, None
        self.zin_off = list(zin_off) if zin_off is not None else [0] * self.ng
        self.out_off = list(out_off) if out_off is not None else [sum(self.n_out[:i]) for i in range(self.ng)]
        self.w_off = [sum(n * Kp for n in self.n_out[:i]) for i in range(self.ng)]
        self.width = zout_pitch if zout_pitch is not None else max(o + n for o, n in zip(self.out_off, self.n_out))
        self.row_w = torch.pow(2.0, torch.randint(0, 3, (rows,), device=dev, generator=g).float()) if row_w else None
        if gather is not None:
            fc, ac, gps = gather["feat_c"], gather.get("act_c", 0), gather.get("gps", 1)
            self.gk = fc + 3 + ac                                         # columns the gathered rows fill
            self.c_in = self.k_used = self.gk if pre_Kp is None else c_in
            self.ones_col = -1
            npts = max(self.r // 3, 64)
            ngrp = (max(self.r // 8, 8) + gps - 1) // gps * gps
            if maps is not None:
                npts, ngrp = maps["npts"], maps["nsmp"] * gps
            self.npts, self.ngrp, self.nsmp = npts, ngrp, ngrp // gps
            self.feat = torch.randn(npts, fc, device=dev, generator=g).abs()
            self.src = torch.rand(npts, 3, device=dev, generator=g)
            self.ctr = torch.rand(ngrp, 3, device=dev, generator=g) if gather.get("ctr", True) else None
            self.action = torch.randn(self.nsmp, ac, device=dev, generator=g) if ac else None
            self.row_pt = torch.randint(0, npts, (rows,), device=dev, generator=g, dtype=torch.int32)
            self.row_grp = torch.sort(torch.randint(0, ngrp, (rows,), device=dev, generator=g, dtype=torch.int32)).values.contiguous()
            if maps is not None:
                self.row_pt, self.row_grp = _supplied(maps["row_pt"], dev), _supplied(maps["row_grp"], dev)
            if pre_Kp is not None:
                assert self.gk <= pre_Kp
                self.pre_W = torch.randn(c_in, pre_Kp, device=dev, generator=g) * 0.3
                self.pre_W[:, self.gk:] = 0
                self.scale = torch.rand(c_in, device=dev, generator=g) + 0.5
                self.shift = torch.randn(c_in, device=dev, generator=g) * 0.3
        else:
            self.c_in = c_in
            self.k_used = c_in + (1 if extra else 0) + (1 if ones else 0)
            self.ones_col = c_in + (1 if extra else 0) if ones else -1
            pitch = max(self.zin_off) + c_in
            self.zin = torch.randn(rows, pitch, device=dev, generator=g)
            self.extra = torch.randn(rows, device=dev, generator=g) if extra else None
            self.scale = (torch.rand(pitch, device=dev, generator=g) + 0.5) if affine else None
            self.shift = (torch.randn(pitch, device=dev, generator=g) * 0.3) if affine else None
        assert self.k_used <= Kp
        self.W = torch.randn(sum(n * Kp for n in self.n_out), device=dev, generator=g) * w_scale
        for wo, n in zip(self.w_off, self.n_out):                     # packed layout: zero padding behind the used columns
            self.W[wo:wo + n * Kp].view(n, Kp)[:, self.k_used:] = 0
        self.zout = torch.empty(rows, self.width, device=dev) if zout else None
        self.stats = torch.zeros(R * 2 * self.width, dtype=torch.float64, device=dev) if stats else None
        if pool is not None:
            self.gsz = pool["gsz"]
            self.pool_grp = (torch.arange(rows, device=dev, dtype=torch.int32) // self.gsz).contiguous()
            self.key = torch.zeros((rows + self.gsz - 1) // self.gsz, self.n_out[0], dtype=torch.int64, device=dev)
            self.gamma = torch.ones(self.n_out[0], device=dev)
            if pool.get("gamma") == "mixed":
                self.gamma = torch.randn(self.n_out[0], device=dev, generator=g)
                self.gamma[::5] = 0.0
        _supply(self, operands, dev)
        if in_stat:
            import numpy as np
            from tests import layer_reference as lr
            rng = np.random.default_rng(seed)
            C = c_in
            self.bn_count, self.bn_eps, self.bn_mom, self.bn_stride = float(rows), 1e-5, 0.1, C + 4
            mean, var = rng.normal(size=C) * 0.3, rng.uniform(0.5, 1.5, C)
            s1, s2 = lr.replicate(mean * rows, self.bn_stride, C, rng), lr.replicate((var + mean * mean) * rows, self.bn_stride, C, rng)
            self.in_sum, self.in_sq = torch.from_numpy(s1).to(dev), torch.from_numpy(s2).to(dev)
            self.in_gamma = torch.rand(C, device=dev, generator=g) + 0.5
            self.in_beta = torch.randn(C, device=dev, generator=g) * 0.3
            self.run_mean0 = torch.randn(C, device=dev, generator=g) * 0.1
            self.run_var0 = torch.rand(C, device=dev, generator=g) + 0.5
            self.zin = self.zin * torch.from_numpy(np.sqrt(var)).float().to(dev) + torch.from_numpy(mean).float().to(dev)
        if split:
            from tests.split_cases import Mirror
            assert self.ng == 1
            self.mirror = Mirror(self.W.view(self.n_out[0], Kp), gather["feat_c"] if gather is not None and pre_Kp is None else Kp)

    def args(self):
        kw = dict(n_rows_dev=_ptr(self.nrows), n_rows=self.rows, row_w=_ptr(self.row_w), W=_ptr(self.W), Kp=self.Kp, n_groups=self.ng,
                  n_out=self.n_out, w_off=self.w_off, out_off=self.out_off, zin_off=self.zin_off, zout=_ptr(self.zout),
                  zout_pitch=self.width)
        if self.has_stats:
            kw.update(stat_sum=_ptr(self.stats, 0, 8), stat_sq=_ptr(self.stats, self.width, 8), stat_stride=2 * self.width)
        kw.update(self.input_kw())
        if self.pool is not None:
            kw.update(pool_key=_ptr(self.key, 0, 8), pool_row_grp=_ptr(self.pool_grp), pool_gamma=_ptr(self.gamma))
        if self.in_stat:
            kw.update(in_stat_sum=_ptr(self.in_sum, 0, 8), in_stat_sq=_ptr(self.in_sq, 0, 8), in_stat_stride=self.bn_stride,
                      in_count=self.bn_count, in_gamma=_ptr(self.in_gamma), in_beta=_ptr(self.in_beta), in_eps=self.bn_eps,
                      in_momentum=self.bn_mom, in_running_mean=_ptr(self.run_mean), in_running_var=_ptr(self.run_var),
                      in_mean=_ptr(self.in_mean), in_istd=_ptr(self.in_istd))
        if self.mirror is not None:
            kw.update(self.mirror.fwd_kw())
        return _fwd_args(**kw)

    def input_kw(self):
        """the fields that describe how the input rows are produced (shared with gad_gemm_dw_args.in)"""
        if self.gather is not None:
            d = dict(mode=1, c_in=self.c_in, src_xyz=_ptr(self.src), ctr_xyz=_ptr(self.ctr), feat=_ptr(self.feat),
                     feat_c=self.gather["feat_c"], action=_ptr(self.action), act_c=self.gather.get("act_c", 0),
                     grp_per_sample=self.gather.get("gps", 1), row_pt=_ptr(self.row_pt), row_grp=_ptr(self.row_grp))
            if self.pre_Kp is not None:
                d.update(mode=2, pre_W=_ptr(self.pre_W), pre_Kp=self.pre_Kp, scale=_ptr(self.scale), shift=_ptr(self.shift), relu=self.relu)
            return d
        return dict(mode=0, zin=_ptr(self.zin), zin_pitch=self.zin.shape[1], c_in=self.c_in, scale=_ptr(self.scale),
                    shift=_ptr(self.shift), relu=self.relu, extra=_ptr(self.extra), ones_col=self.ones_col)

    def launch(self):
        nan = float("nan")
        if self.zout is not None:
            self.zout.fill_(nan)
        if self.stats is not None:
            _prefill(self.stats, self.init.get("stats"))
        if self.pool is not None:
            self.key.zero_()
        if self.in_stat:
            dev = self.W.device
            self.scale, self.shift = torch.full((self.c_in,), nan, device=dev), torch.full((self.c_in,), nan, device=dev)
            self.in_mean, self.in_istd = torch.full((self.c_in,), nan, device=dev), torch.full((self.c_in,), nan, device=dev)
            self.run_mean, self.run_var = self.run_mean0.clone(), self.run_var0.clone()
        self.call("gad_gemm_fwd", self.args())
        out = {}
        if self.zout is not None:
            out["z"] = self.zout.clone()                              # every row: rows past the live count must still hold NaN
        if self.stats is not None:
            out["stat_sum"], out["stat_sq"] = _replica_sum(self.stats, self.width, 0), _replica_sum(self.stats, self.width, 1)
        if self.pool is not None:
            out["key"] = self.key.clone()
            out["zmax"] = self.decode_keys(out["key"])
        if self.in_stat:
            for k in ("scale", "shift", "in_mean", "in_istd", "run_mean", "run_var"):
                out[k] = getattr(self, k).clone()
        return out

    def decode_keys(self, key):
        """the float32 value packed in every key's upper half (the decode of tests/test_gpu_split_families.check_case), times sgn(gamma);
        NaN for a key that is still 0 (no row)"""
        hi = (key >> 32) & 0xffffffff
        bits = torch.where((hi & 0x80000000) != 0, hi ^ 0x80000000, (~hi) & 0xffffffff).to(torch.int32)
        val = bits.view(torch.float32) * torch.where(self.gamma < 0, -1.0, 1.0)[None, :]
        return torch.where(key == 0, torch.full_like(val, float("nan")), val)

    def operands(self):
        r = self.r
        if self.pre_Kp is not None:
            return [self.recomputed()["A"]]
        if self.gather is not None:
            return [gr.gather_operand(self.feat, self.src, self.ctr, self.action, self.row_pt, self.row_grp, self.gather.get("gps", 1),
                                      self.Kp, r)]
        return [gr.act_operand(self.zin, zo, self.c_in, self.Kp, self.scale, self.shift, self.relu, self.extra, self.ones_col, r)
                for zo in self.zin_off]

    def recomputed(self):
        """mode 2: gemm_reference.recomputed_operand of the live rows"""
        G = gr.gather_operand(self.feat, self.src, self.ctr, self.action, self.row_pt, self.row_grp, self.gather.get("gps", 1),
                              self.pre_Kp, self.r)
        return gr.recomputed_operand(G, self.pre_W, self.gk, self.scale, self.shift, self.relu)

    def base_operands(self, As):
        """what the float32 baseline multiplies: the operands themselves; mode 2: the same chain in torch float32 (matmul32 of the
        gathered rows, one fused multiply-add, ReLU)"""
        if self.pre_Kp is None:
            return As
        G = gr.gather_operand(self.feat, self.src, self.ctr, self.action, self.row_pt, self.row_grp, self.gather.get("gps", 1),
                              self.pre_Kp, self.r)
        a = gr.fma32(matmul32(G, self.pre_W.t()), self.scale, self.shift)
        return [a.clamp_min(0) if self.relu else a]

    def _pad_rows(self, t):
        """(live rows, ...) -> (static rows, ...), NaN behind the live rows"""
        out = torch.full((self.rows,) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device=t.device)
        out[:self.r] = t
        return out

    def expect(self, alter=None):
        """T: z = k_used products.  stat_sum adds the rows a lane / workgroup sums in float32 before its f64 atomic (<= the live rows):
        k_used + rows.  stat_sq: each term w * z * z carries z's error twice and one rounding of w * z: 2 * k_used + rows + 1.
        mode 2: the operand itself is a float32 evaluation of a first layer; how far it may lie from the float64 chain
        (gemm_reference.recomputed_operand, A#slack) enters every bound as a slack: |dA| @ |W|^T for z, its weighted row sum for
        stat_sum, sum_r w * (2 * z#abs + dz) * dz for stat_sq.
        alter (negative controls): see tests/test_gpu_gemm_f64.py and tests/test_gpu_gemm_f64_wide.py"""
        if isinstance(alter, tuple) and alter[0] == "first_rows":         # the reference of a launch that stopped after alter[1] rows
            return _with_rows(self, alter[1], self.expect)
        r, K = self.r, self.k_used
        As = self.operands()
        out_off = list(self.out_off)
        if alter == "zero_tile_row":                         # the first row of the last 64-row tile
            As = [a.clone() for a in As]
            for a in As:
                a[(r - 1) // 64 * 64] = 0
        if alter == "no_bias":
            As = [a.clone() for a in As]
            for a in As:
                a[:, self.ones_col] = 0
        elif alter == "no_extra":
            As = [a.clone() for a in As]
            for a in As:
                a[:, self.c_in] = 0
        elif alter == "shift_out_off":
            out_off[-1] += 4
        ref = gr.forward(As, self.W, self.Kp, self.w_off, out_off, self.n_out, self.width + (4 if alter == "shift_out_off" else 0),
                         row_w=self.row_w)
        if alter == "shift_out_off":
            ref = {k: v[..., :self.width] for k, v in ref.items()}
        if alter == "drop_last_row_stats":
            sref = gr.forward([a[:r - 1] for a in As], self.W, self.Kp, self.w_off, out_off, self.n_out, self.width, row_w=self.row_w)
            for k in ("stat_sum", "stat_sq"):
                ref[k] = sref[k]
        if alter == "shift_block":                           # the second 128-column block of the output, 4 columns to the right
            for k in ("z", "stat_sum", "stat_sq"):
                ref[k][..., 128:256] = torch.roll(ref[k][..., 128:256], 4, -1)
        Ab = self.base_operands(As)
        z32 = torch.zeros(r, self.width, device=self.W.device)
        for A, wo, oo, n in zip(Ab, self.w_off, self.out_off, self.n_out):
            z32[:, oo:oo + n] = matmul32(A, self.W[wo:wo + n * self.Kp].view(n, self.Kp).t())
        w32 = self.row_w[:r, None] if self.row_w is not None else torch.ones(r, 1, device=z32.device)
        exp = {}
        zs = ss = qs = None
        if self.pre_Kp is not None:
            w64 = w32.double()
            dz = self.recomputed()["A#slack"] @ self.W.view(self.n_out[0], self.Kp).double().abs().t()
            zs, ss, qs = self._pad_rows(dz), (w64 * dz).sum(0), (w64 * (2 * ref["z#abs"] + dz) * dz).sum(0)

        def zchain():
            c32 = torch.zeros(r, self.width, device=self.W.device)
            for A, wo, oo, n in zip(Ab, self.w_off, self.out_off, self.n_out):
                c32[:, oo:oo + n] = chain32(A[:, :K], self.W[wo:wo + n * self.Kp].view(n, self.Kp)[:, :K])
            return self._pad_rows(c32)
        if self.has_zout:
            exp["z"] = spec(self._pad_rows(ref["z"]), self._pad_rows(ref["z#abs"]), K, self._pad_rows(z32), slack=zs, chain=zchain)
        if self.has_stats:
            # (a reference without the last row comes with the float32 baseline of the same rows: at 3e4 rows one row is far inside
            # the derived bound of a row sum, and it is the margin over the baseline that has to notice it)
            rs = r - 1 if alter == "drop_last_row_stats" else r
            exp["stat_sum"] = spec(ref["stat_sum"], ref["stat_sum#abs"], K + r, (w32 * z32)[:rs].sum(0), True, slack=ss)
            exp["stat_sq"] = spec(ref["stat_sq"], ref["stat_sq#abs"], 2 * K + r + 1, (w32 * z32 * z32)[:rs].sum(0), True, slack=qs)
        if self.pool is not None:
            # the pooled value is one of the group's z: |max got - max ref| <= the largest bound inside the group.  A last group
            # that the live rows end in pools its live rows only
            G, gs, sg = (r + self.gsz - 1) // self.gsz, self.gsz, torch.where(self.gamma < 0, -1.0, 1.0).double()[None, :]
            zmax = torch.full(tuple(self.key.shape), float("nan"), dtype=torch.float64, device=z32.device)
            zabs = torch.zeros_like(zmax)
            zmax[:G] = _group_max(ref["z"] * sg, G, gs, float("-inf")) * sg
            zabs[:G] = _group_max(ref["z#abs"], G, gs, 0.0)
            b32 = torch.zeros_like(zmax)
            b32[:G] = _group_max(z32.double() * sg, G, gs, float("-inf")) * sg
            exp["zmax"] = spec(zmax, zabs, K, b32)
        return exp

    def exact(self, out):
        """-> failures of the checks that are exact"""
        bad = []
        if self.pool is not None and "z" in out:            # keys decode to the maxima of the launch's own stored output
            G, gs = (self.r + self.gsz - 1) // self.gsz, self.gsz
            sg = torch.where(self.gamma < 0, -1.0, 1.0)[None, :]
            want = _group_max(out["z"][:self.r] * sg, G, gs, float("-inf")) * sg
            if not torch.equal(out["zmax"][:G], want):
                bad.append("pooled keys do not decode to the maxima of the stored output")
            row = 0xffffffff - (out["key"][:G] & 0xffffffff)
            first = torch.arange(G, device=row.device)[:, None] * gs
            if not bool(((row >= first) & (row < first + gs) & (row < self.r)).all()):
                bad.append("a pooled key names a row outside its group")
        if self.pool is not None and not bool((out["key"][(self.r + self.gsz - 1) // self.gsz:] == 0).all()):
            bad.append("keys of groups without live rows were written")
        return bad

    def check_in_stat(self, out):
        """the published BatchNorm vectors against layer_reference.bn_finalize, with the bounds derived in
        tests/test_gpu_layer_kernels._check_bn"""
        import numpy as np
        from tests import layer_reference as lr
        C = self.c_in
        ref = lr.bn_finalize(self.in_sum.cpu().numpy(), self.in_sq.cpu().numpy(), self.bn_stride, self.bn_count, self.in_gamma.cpu().numpy(),
                             self.in_beta.cpu().numpy(), self.bn_eps, self.bn_mom, self.run_mean0.cpu().numpy(), self.run_var0.cpu().numpy())
        beta = self.in_beta.cpu().numpy().astype(np.float64)
        bounds = {"scale": 3 * U * np.abs(ref["scale"]), "shift": 4 * U * (np.abs(beta) + np.abs(ref["mean"] * ref["scale"])),
                  "in_mean": U * np.abs(ref["mean"]), "in_istd": 1.25 * U * ref["istd"], "run_mean": 4 * U * ref["running_mean_abs"],
                  "run_var": 4 * U * ref["running_var_abs"]}
        names = {"in_mean": "mean", "in_istd": "istd", "run_mean": "running_mean", "run_var": "running_var"}
        bad = []
        for k, b in bounds.items():
            e = np.abs(out[k].cpu().numpy().astype(np.float64) - ref[names.get(k, k)])
            if not (e <= b).all():
                bad.append("in_stat %s: worst err / bound %.3f" % (k, float((e / np.maximum(b, 1e-300)).max())))
        return bad


# ----------------------------------------------------------------------------------------------------------------- dX
class Dx(Case):
    """gad_gemm_dx.  dZ = P*g - w*(Q + S*z) from z (cap, C) and a dense G (or pooled = dict(gsz): arg-max routing), groups through
    dz_off / gout_off / n_out; prev: the previous layer's BatchNorm-backward sums (+ store_masked); scatter = dict(feat_c, act_c, gps,
    dfeat, daction): epilogue 1.  P and the row weights are powers of two (tests/split_cases.DxWide): dZ has a single rounding.
    pad_cols: columns of gout / zprev behind the last group's that no group writes (0: pitch = k_valid, what the streaming routes
    take); split: the call carries the transposed split-bf16 mirror of W (split_cases.Mirror; one group).
    Hooks as for Fwd: maps (the scatter epilogue's row maps, point and sample counts), operands, init = {"dfeat" / "daction" /
    "bst": array}: the accumulators' contents before the launch in place of zeros."""
    entry = "gad_gemm_dx"

    def __init__(self, rows, n_out, Kp, k_valid, dz_off=None, gout_off=None, g_pitch=None, z=True, relu=1, premasked=1, dscale=False,
                 coef=True, row_w=True, prev=False, store_masked=1, live=None, pooled=None, scatter=None, bn=False, seed=2, w_scale=0.05,
                 pad_cols=4, split=False, maps=None, operands=None, init=None):
        dev = torch.device("cuda")
        g = _gen(seed)
        self.init = dict(init or {})
        self.rows, self.Kp, self.kv, self.n_out, self.ng = rows, Kp, k_valid, list(n_out), len(n_out)
        self.r = rows if live is None else live
        self.nrows = None if live is None else torch.tensor([live], dtype=torch.int32, device=dev)
        self.dz_off = list(dz_off) if dz_off is not None else [sum(self.n_out[:i]) for i in range(self.ng)]
        self.gout_off = list(gout_off) if gout_off is not None else [i * k_valid for i in range(self.ng)]
        self.w_off = [sum(n * Kp for n in self.n_out[:i]) for i in range(self.ng)]
        C = g_pitch if g_pitch is not None else max(o + n for o, n in zip(self.dz_off, self.n_out))
        self.C, self.relu, self.premasked, self.prev, self.store_masked, self.pooled, self.scatter, self.bn = C, relu, premasked, prev, store_masked, pooled, scatter, bn
        self.z = torch.randn(rows, C, device=dev, generator=g) if z else None
        self.row_w = torch.pow(2.0, torch.randint(0, 3, (rows,), device=dev, generator=g).float()) if row_w else None
        self.P = torch.pow(2.0, torch.randint(-1, 2, (C,), device=dev, generator=g).float()) if coef else None
        self.Q = torch.randn(C, device=dev, generator=g) * 0.1 if coef else None
        self.S = torch.randn(C, device=dev, generator=g) * 0.1 if coef else None
        self.dscale = (torch.rand(C, device=dev, generator=g) + 0.5) if dscale else None
        self.dshift = (torch.randn(C, device=dev, generator=g) * 0.3) if dscale else None
        self.W = torch.randn(sum(n * Kp for n in self.n_out), device=dev, generator=g) * w_scale
        if pooled is not None:
            gs = pooled["gsz"]
            self.row_grp_dz = (torch.arange(rows, device=dev, dtype=torch.int32) // gs).contiguous()
            ngrp = (rows + gs - 1) // gs
            self.argmax = (torch.arange(ngrp, device=dev, dtype=torch.int32)[:, None] * gs +
                           torch.randint(0, gs, (ngrp, C), device=dev, generator=g, dtype=torch.int32)).contiguous()
            self.dout = torch.randn(ngrp, C, device=dev, generator=g)
        else:
            self.G = torch.randn(rows, C, device=dev, generator=g)
        if scatter is not None:
            fc, ac, gps = scatter["feat_c"], scatter.get("act_c", 0), scatter.get("gps", 1)
            self.npts = max(self.r // 3, 64)
            ngrp = (max(self.r // 8, 8) + gps - 1) // gps * gps
            self.nsmp = ngrp // gps
            self.row_pt = torch.randint(0, self.npts, (rows,), device=dev, generator=g, dtype=torch.int32)
            self.row_pt[: rows // 3] = 5                                   # many rows on one point
            self.row_grp = torch.sort(torch.randint(0, ngrp, (rows,), device=dev, generator=g, dtype=torch.int32)).values.contiguous()
            if maps is not None:
                self.npts, self.nsmp = maps["npts"], maps["nsmp"]
                self.row_pt, self.row_grp = _supplied(maps["row_pt"], dev), _supplied(maps["row_grp"], dev)
            self.dfeat = torch.zeros(self.npts, fc, device=dev) if scatter.get("dfeat", True) else None
            self.daction = torch.zeros(self.nsmp, ac, dtype=torch.float64, device=dev) if (ac and scatter.get("daction", True)) else None
            self.width = k_valid
        else:
            self.width = max(self.gout_off) + k_valid + pad_cols           # (+ 4 columns no group writes)
            self.gout = torch.empty(rows, self.width, device=dev)
            if prev:
                self.zprev = torch.randn(rows, self.width, device=dev, generator=g)
                self.pvec = [torch.rand(self.width, device=dev, generator=g) + 0.5, torch.randn(self.width, device=dev, generator=g) * 0.3,
                             torch.randn(self.width, device=dev, generator=g) * 0.1, torch.rand(self.width, device=dev, generator=g) + 0.5]
                self.bst = torch.zeros(R * 2 * self.width, dtype=torch.float64, device=dev)
        if bn:                                  # the bn_* block: P / Q / S formed by gad_bn_bwd_coef into the coefP / Q / S scratch
            import numpy as np
            from tests import layer_reference as lr
            rng = np.random.default_rng(seed)
            self.bn_stride, self.bn_count = C + 4, float(rows)
            self.bn_db = torch.from_numpy(lr.replicate(rng.normal(size=C) * 20, self.bn_stride, C, rng)).to(dev)
            self.bn_dg = torch.from_numpy(lr.replicate(rng.normal(size=C) * 20, self.bn_stride, C, rng)).to(dev)
            self.bn_mean = torch.randn(C, device=dev, generator=g) * 0.1
            self.bn_istd = torch.rand(C, device=dev, generator=g) + 0.5
            self.dscale = torch.pow(2.0, torch.randint(-1, 2, (C,), device=dev, generator=g).float())     # P = scale: a power of two
            self.dshift = torch.randn(C, device=dev, generator=g) * 0.3
        _supply(self, operands, dev)
        self.mirror = None
        if split:
            from tests.split_cases import Mirror
            assert self.ng == 1
            self.mirror = Mirror(self.W.view(self.n_out[0], Kp), k_valid)

    def dz_kw(self):
        d = dict(z=_ptr(self.z), z_pitch=self.C if self.z is not None else 0, scale=_ptr(self.dscale), shift=_ptr(self.dshift),
                 relu=self.relu, premasked=self.premasked, row_w=_ptr(self.row_w), c=self.C, coefP=_ptr(self.P), coefQ=_ptr(self.Q),
                 coefS=_ptr(self.S))
        if self.pooled is not None:
            d.update(gmode=1, argmax=_ptr(self.argmax), dout=_ptr(self.dout), row_grp=_ptr(self.row_grp_dz))
        else:
            d.update(gmode=0, G=_ptr(self.G), g_pitch=self.C)
        if self.bn:
            d.update(bn_dbeta=_ptr(self.bn_db, 0, 8), bn_dgamma=_ptr(self.bn_dg, 0, 8), bn_stride=self.bn_stride, bn_count=self.bn_count,
                     bn_mean=_ptr(self.bn_mean), bn_istd=_ptr(self.bn_istd))
        return d

    def args(self):
        a = hip.GemmDxArgs()
        a.n_rows_dev, a.n_rows, a.dz, a.n_groups = _ptr(self.nrows), self.rows, _dz(**self.dz_kw()), self.ng
        for i in range(self.ng):
            a.dz_off[i], a.w_off[i], a.n_out[i], a.gout_off[i] = self.dz_off[i], self.w_off[i], self.n_out[i], self.gout_off[i]
        a.W, a.Kp, a.k_valid, a.grp_per_sample = _ptr(self.W), self.Kp, self.kv, 1
        a.accumulate = getattr(self, "accumulate", 0)
        if self.scatter is not None:
            a.epilogue, a.dfeat, a.feat_c, a.row_pt, a.row_grp = 1, _ptr(self.dfeat), self.scatter["feat_c"], _ptr(self.row_pt), _ptr(self.row_grp)
            a.daction, a.act_c, a.grp_per_sample = _ptr(self.daction, 0, 8), self.scatter.get("act_c", 0), self.scatter.get("gps", 1)
        else:
            a.epilogue, a.gout, a.gout_pitch = 0, _ptr(self.gout), self.width
            if self.prev:
                a.zprev, a.zprev_pitch = _ptr(self.zprev), self.width
                a.prev_scale, a.prev_shift, a.prev_mean, a.prev_istd = (_ptr(v) for v in self.pvec)
                a.prev_dbeta, a.prev_dgamma, a.stat_stride = _ptr(self.bst, 0, 8), _ptr(self.bst, self.width, 8), 2 * self.width
                a.store_masked = self.store_masked
        if self.mirror is not None:
            for k, v in self.mirror.t_kw().items():
                setattr(a, k, v)
        return a

    def prepare(self):
        """everything the launch may write, pre-filled"""
        self.bn_prepare()
        if self.scatter is not None:
            for k, t in (("dfeat", self.dfeat), ("daction", self.daction)):
                if t is not None:
                    _prefill(t, self.init.get(k))
        else:
            self.gout.fill_(float("nan"))
            if self.prev:
                _prefill(self.bst, self.init.get("bst"))

    def collect(self):
        out = {}
        if self.scatter is not None:
            if self.dfeat is not None:
                out["dfeat"] = self.dfeat.clone()
            if self.daction is not None:
                out["daction"] = self.daction.clone()
        else:
            out["gout"] = self.gout.clone()
            if self.prev:
                out["dbeta"], out["dgamma"] = _replica_sum(self.bst, self.width, 0), _replica_sum(self.bst, self.width, 1)
        self.bn_collect(out)
        return out

    def launch(self):
        self.prepare()
        self.call("gad_gemm_dx", self.args())
        return self.collect()

    def bn_prepare(self):
        self.bn_in_registers = False
        if self.bn:
            for v in (self.P, self.Q, self.S):
                v.fill_(float("nan"))

    def bn_collect(self, out):
        """the bn_* block: a route whose kernel reads P / Q / S per lane has gad_bn_bwd_coef publish them in the scratch (out["P"],
        ["Q"], ["S"]: check_bn).  The wide-tile kernels form them per channel in registers (dz_coef -> gad_bn_bwd_channel) and
        publish nothing: the scratch still holds the NaN it was given, and the reference's dZ takes the coefficients of
        layer_reference.bn_bwd_coef, rounded to float32 as that device function rounds its float64 evaluation -- the coefficients
        are then tested through every output of the launch."""
        if not self.bn or self.bn_in_registers:
            return
        if bool(torch.isnan(torch.cat([self.P, self.Q, self.S])).all()):
            self.bn_in_registers = True
            import numpy as np
            from tests import layer_reference as lr
            ref = lr.bn_bwd_coef(self.bn_db.cpu().numpy(), self.bn_dg.cpu().numpy(), self.bn_stride, self.dscale.cpu().numpy(),
                                 self.bn_mean.cpu().numpy(), self.bn_istd.cpu().numpy(), self.bn_count)
            for v, k in ((self.P, "P"), (self.Q, "Q"), (self.S, "S")):
                v.copy_(torch.from_numpy(np.asarray(ref[k]).astype(np.float32)))
        else:
            out["P"], out["Q"], out["S"] = self.P.clone(), self.Q.clone(), self.S.clone()

    def dz32(self):
        r = self.r
        dY = gr.route_pooled(self.argmax, self.dout, self.row_grp_dz, r) if self.pooled is not None else self.G[:r]
        return gr.dz_operand(dY, self.z, self.dscale, self.dshift, self.relu, self.premasked, self.P, self.Q, self.S, self.row_w)

    def expect(self, alter=None):
        """T: gout = the group's n_out products.  dbeta adds the rows summed in float32 before the f64 atomic: n_out + rows; dgamma's
        terms carry x_hat = (zprev - mean) * istd, two more roundings, and the fused multiply-add: n_out + rows + 3.  dfeat: float32
        atomics, one per row of the point: n_out + the most rows on one point.  daction: float64 sums of the float32 products: n_out."""
        if isinstance(alter, tuple) and alter[0] == "first_rows":         # the reference of a launch that stopped after alter[1] rows
            return _with_rows(self, alter[1], self.expect)
        r, n = self.r, max(self.n_out)
        dZ = self.dz32()
        if alter == "zero_tile_row":                         # the first row of the last 64-row tile
            dZ = dZ.clone()
            dZ[(r - 1) // 64 * 64] = 0
        gout_off = list(self.gout_off)
        W = self.W
        if alter == "shift_out_off":
            gout_off[-1] += 4
        elif alter in ("no_bias", "no_extra"):       # k_valid = c_in + 2 of the layer below: its extra and bias columns are the last two produced
            W = self.W.clone()
            for wo, nn in zip(self.w_off, self.n_out):
                W[wo:wo + nn * self.Kp].view(nn, self.Kp)[:, self.kv - (1 if alter == "no_bias" else 2)] = 0
        prev = dict(zprev=self.zprev, scale=self.pvec[0], shift=self.pvec[1], mean=self.pvec[2], istd=self.pvec[3]) if self.prev else None
        ref = gr.dx(dZ, W, self.Kp, self.kv, self.dz_off, self.w_off, self.n_out, gout_off, self.width, prev, self.store_masked)
        if alter == "drop_last_row_stats":
            sref = gr.dx(dZ[:r - 1], self.W, self.Kp, self.kv, self.dz_off, self.w_off, self.n_out, gout_off, self.width, prev, self.store_masked)
            ref["dbeta"], ref["dgamma"] = sref["dbeta"], sref["dgamma"]
        if alter == "shift_block":                           # the second 128-column block of the input gradient, 4 columns to the right
            for k in ("gx", "gout", "dbeta", "dgamma"):
                if k in ref:
                    ref[k] = ref[k].clone()
                    ref[k][..., 128:256] = torch.roll(ref[k][..., 128:256], 4, -1)
        g32 = torch.zeros(r, self.width, device=dZ.device)
        for do, wo, nn, go in zip(self.dz_off, self.w_off, self.n_out, self.gout_off):
            g32[:, go:go + self.kv] = matmul32(dZ[:, do:do + nn], self.W[wo:wo + nn * self.Kp].view(nn, self.Kp)[:, :self.kv])
        exp = {}
        if self.scatter is not None:
            fc, ac, gps = self.scatter["feat_c"], self.scatter.get("act_c", 0), self.scatter.get("gps", 1)
            sc = gr.scatter(ref["gx"], ref["gout#abs"], self.row_pt, self.row_grp, gps, fc, ac, self.npts, self.nsmp)
            pt = self.row_pt[:r].long()
            if self.dfeat is not None:
                b = torch.zeros(self.npts, fc, device=dZ.device).index_add_(0, pt, g32[:, :fc])
                exp["dfeat"] = spec(sc["dfeat"], sc["dfeat#abs"], n + int(torch.bincount(pt).max()), b, True)
            if self.daction is not None:
                smp = torch.div(self.row_grp[:r].long(), gps, rounding_mode="floor")
                b = torch.zeros(self.nsmp, ac, device=dZ.device).index_add_(0, smp, g32[:, fc + 3:fc + 3 + ac])
                exp["daction"] = spec(sc["daction"], sc["daction#abs"], n, b, True)
            return exp
        pad = lambda t: torch.cat([t, torch.full((self.rows - r, self.width), float("nan"), dtype=t.dtype, device=t.device)])
        base = g32
        masked = lambda t: t
        if self.prev:
            live = gr.fma32(self.zprev[:r], self.pvec[0], self.pvec[1]) > 0
            m32 = torch.where(live, g32, torch.zeros((), device=g32.device))
            if self.store_masked:
                base = m32
                masked = lambda t: torch.where(live, t, torch.zeros((), device=t.device))
            xhat32 = (self.zprev[:r] - self.pvec[2]) * self.pvec[3]
            rs = r - 1 if alter == "drop_last_row_stats" else r          # (the baseline of the rows the reference covers: Fwd.expect)
            exp["dbeta"] = spec(ref["dbeta"], ref["dbeta#abs"], n + r, m32[:rs].sum(0), True)
            exp["dgamma"] = spec(ref["dgamma"], ref["dgamma#abs"], n + r + 3, (m32 * xhat32)[:rs].sum(0), True)

        def gchain():
            c32 = torch.zeros(r, self.width, device=dZ.device)
            for do, wo, nn, go in zip(self.dz_off, self.w_off, self.n_out, self.gout_off):
                c32[:, go:go + self.kv] = chain32(dZ[:, do:do + nn], self.W[wo:wo + nn * self.Kp].view(nn, self.Kp)[:, :self.kv].t())
            return pad(masked(c32))
        exp["gout"] = spec(pad(ref["gout"]), pad(ref["gout#abs"]), n, pad(base), chain=gchain)
        return exp

    def exact(self, out):
        return []

    def check_bn(self, out):
        """P / Q / S left in the scratch by the coefficient launch against layer_reference.bn_bwd_coef (P bit-exact; Q, S: one float32
        rounding of a float64 evaluation, the bound of tests/test_gpu_layer_kernels); nothing where the route publishes none
        (bn_collect)"""
        if "P" not in out:
            return []
        import numpy as np
        from tests import layer_reference as lr
        ref = lr.bn_bwd_coef(self.bn_db.cpu().numpy(), self.bn_dg.cpu().numpy(), self.bn_stride, self.dscale.cpu().numpy(),
                             self.bn_mean.cpu().numpy(), self.bn_istd.cpu().numpy(), self.bn_count)
        bad = []
        if not np.array_equal(out["P"].cpu().numpy(), ref["P"]):
            bad.append("bn block: P is not the layer's scale")
        for k in ("Q", "S"):
            e = np.abs(out[k].cpu().numpy().astype(np.float64) - ref[k])
            b = U * np.abs(ref[k]) + 2.0 ** -50 * ref["Q_f64"]
            if not (e <= b).all():
                bad.append("bn block %s: worst err / bound %.3f" % (k, float((e / np.maximum(b, 1e-300)).max())))
        return bad


# ----------------------------------------------------------------------------------------------------------------- dW
class Dw(Case):
    """gad_gemm_dw: `inp` (a Fwd case: how the layer's input rows are produced) and `dz` (a Dx case: the gradient source) over the
    same rows.  The arena is pre-filled (the entry point ADDS); partial: the caller's split workspace or NULL (f64 atomics);
    init = {"gacc": array}: the caller's arena contents in place of the drawn pre-fill."""
    entry = "gad_gemm_dw"

    def __init__(self, inp, dz, dz_off=None, partial=True, row_splits=0, init=None):
        dev = torch.device("cuda")
        assert inp.rows == dz.rows and inp.r == dz.r
        self.inp, self.dz, self.row_splits = inp, dz, row_splits
        self.dz_off = list(dz_off) if dz_off is not None else dz.dz_off
        self.r = inp.r
        self.total = sum(n * inp.Kp for n in inp.n_out) + 16
        g = _gen(99)
        self.prefill = (torch.randint(-16, 17, (self.total,), device=dev, generator=g).double() / 8.0)     # non-zero, few bits
        self.prefill[self.prefill == 0] = 0.125
        if init is not None and "gacc" in init:                         # caller-supplied arena contents
            self.prefill = _supplied(init["gacc"], dev).double().reshape(-1)
            assert self.prefill.numel() == self.total
        self.gacc = self.prefill.clone()
        self.ws = torch.empty(8 * 1024 * 1024, device=dev) if partial else None

    def args(self):
        i, d = self.inp, self.dz
        a = hip.GemmDwArgs()
        kw = dict(n_rows_dev=_ptr(i.nrows), n_rows=i.rows, row_w=_ptr(d.row_w), Kp=i.Kp, n_groups=i.ng, n_out=i.n_out, w_off=i.w_off,
                  zin_off=i.zin_off)
        kw.update(i.input_kw())
        a.inp = _fwd_args(**kw)
        a.dz = _dz(**d.dz_kw())
        for k, o in enumerate(self.dz_off):
            a.dz_off[k] = o
        a.gacc, a.row_splits = _ptr(self.gacc, 0, 8), self.row_splits
        if self.ws is not None:
            a.partial, a.partial_elems = _ptr(self.ws), self.ws.numel()
        return a

    def prepare(self):
        self.gacc.copy_(self.prefill)
        self.dz.bn_prepare()

    def collect(self):
        out = {"gacc": self.gacc.clone()}
        self.dz.bn_collect(out)
        return out

    def launch(self):
        self.prepare()
        self.call("gad_gemm_dw", self.args())
        return self.collect()

    def expect(self, alter=None):
        """T: every element of dW is a sum over the live rows, in float32 inside a wavefront / workgroup / split, f64 across them: rows.
        The arena holds prefill + dW; `outputs` hands the gate gacc - prefill.  slack: the f64 adds into the arena (at most 1024
        partial values per word) and that subtraction round at 2**-53 of |prefill| + |dW|."""
        i = self.inp
        As = i.operands()
        dZ = self.dz.dz32()
        dz_off, w_off = list(self.dz_off), list(i.w_off)
        if alter == "no_bias":
            As = [a.clone() for a in As]
            for a in As:
                a[:, i.ones_col] = 0
        elif alter == "no_extra":
            As = [a.clone() for a in As]
            for a in As:
                a[:, i.c_in] = 0
        elif alter == "drop_last_row_stats":
            As, dZ = [a[:self.r - 1] for a in As], dZ[:self.r - 1]
        elif alter == "zero_tile_row":                       # the first row of the last 64-row tile
            dZ = dZ.clone()
            dZ[(self.r - 1) // 64 * 64] = 0
        elif alter == "shift_out_off":
            dz_off[-1] += 4
        ref = gr.dw(dZ, As, i.Kp, i.k_used, dz_off, w_off, i.n_out, self.total)
        if alter == "shift_block":                           # input columns 128 .. 255 of the one group's block, 4 to the right
            blk = ref["dW"][w_off[0]:w_off[0] + i.n_out[0] * i.Kp].view(i.n_out[0], i.Kp)
            blk[:, 128:256] = torch.roll(blk[:, 128:256], 4, -1)
        b32 = torch.zeros(self.total, device=dZ.device)
        for A, do, wo, n in zip(As, self.dz_off, i.w_off, i.n_out):
            b32[wo:wo + n * i.Kp].view(n, i.Kp)[:, :i.k_used] = matmul32(dZ[:, do:do + n].t(), A[:, :i.k_used])
        slack = 1024 * 2.0 ** -53 * (self.prefill.abs() + ref["dW#abs"])
        return {"dW": spec(ref["dW"], ref["dW#abs"], max(self.r, 1), b32, True, slack)}

    def outputs(self, out):
        """gacc -> what the call added"""
        return {"dW": out["gacc"] - self.prefill}

    def exact(self, out):
        """the columns k_used .. Kp of every group and the words of no group keep their pre-fill bit for bit"""
        i = self.inp
        mask = torch.zeros(self.total, dtype=torch.bool, device=self.gacc.device)
        for wo, n in zip(i.w_off, i.n_out):
            mask[wo:wo + n * i.Kp].view(n, i.Kp)[:, :i.k_used] = True
        if not torch.equal(out["gacc"][~mask], self.prefill[~mask]):
            return ["%d arena words outside the groups' used columns changed" % int((out["gacc"][~mask] != self.prefill[~mask]).sum())]
        return []


# ----------------------------------------------------------------------------------------------------------------- dX + dW
DW_REDUCE_LATER = -2          # include/gaddpg.h GAD_DW_REDUCE_LATER


def layer_input(dx):
    """the Fwd description of the layer whose input gradient the Dx case `dx` produces -- how gad_gemm_dw_args.in must describe the
    rows for gad_gemm_bwd to take both as one layer: the SAME zprev / scale / shift tensors as dx's previous-layer block (ACT), or a
    gathered input over dx's own row maps (scatter epilogue), and the same device row count"""
    live = None if dx.nrows is None else dx.r
    if dx.scatter is not None:
        gth = dict(feat_c=dx.scatter["feat_c"], act_c=dx.scatter.get("act_c", 0), gps=dx.scatter.get("gps", 1))
        inp = Fwd(dx.rows, dx.Kp, dx.n_out, gather=gth, live=live, stats=False, zout=False, row_w=False, seed=17)
        assert inp.npts == dx.npts
        inp.row_pt, inp.row_grp = dx.row_pt, dx.row_grp
    else:
        assert dx.prev and dx.Kp == dx.kv
        inp = Fwd(dx.rows, dx.Kp, dx.n_out, c_in=dx.kv, live=live, stats=False, zout=False, row_w=False, seed=17)
        inp.zin, inp.scale, inp.shift = dx.zprev, dx.pvec[0], dx.pvec[1]
    inp.nrows = dx.nrows
    return inp


class Bwd(Case):
    """gad_gemm_bwd: the dX description `dx` (a Dx case) and the dW description of the same layer (a Dw case over layer_input(dx) and
    dx's gradient source) in one call; later: the call is made with row_splits = GAD_DW_REDUCE_LATER and followed by an explicit
    gad_gemm_dw_reduce on the same argument blocks (while the case's options are still in force: the reduce recomputes the split count
    from them).  Outputs, references and exact checks are those of the two cases."""
    entry = "gad_gemm_bwd"

    def __init__(self, dx, later=False):
        self.dx, self.dz, self.later = dx, dx, later
        self.dw = Dw(layer_input(dx), dx)
        self.r = dx.r

    def launch(self):
        self.dx.prepare()
        self.dw.prepare()
        ax, aw = self.dx.args(), self.dw.args()
        if self.later:
            aw.row_splits = DW_REDUCE_LATER
        self.call("gad_gemm_bwd", ax, aw)
        if self.later:
            self.call("gad_gemm_dw_reduce", ax, aw)
        out = self.dx.collect()
        out.update(self.dw.collect())
        return out

    def outputs(self, out):
        return dict(out, **self.dw.outputs(out))

    def expect(self, alter=None):
        """T of gout / dbeta / dgamma / dfeat: Dx.expect; of dW: Dw.expect (the fused kernels keep one float32 partial block per
        workgroup over all its rows: at most the live rows per element, as for the separate kernels)"""
        exp = self.dx.expect(alter)
        exp.update(self.dw.expect(alter))
        return exp

    def exact(self, out):
        return self.dw.exact(out)
