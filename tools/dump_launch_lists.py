"""Writes every launch list the fused paths build as text, for `cmp` between two trees on the same box: a refactor of the host code
that describes the launches (engine.py, sa_function.py, heads.py) leaves this file byte-identical.

    python tools/dump_launch_lists.py --out lists.txt

Per item: `kind on on2 name tag`; per `call` item also every argument: ints and floats verbatim, pointers as 0 (NULL) or P
(addresses differ between processes), a ctypes structure or array expanded field by field under the same rule.  So the file pins
the entry points, their order, lanes and tags, every integer and float argument and every pointer's NULL-ness -- not WHICH buffer
a pointer names (tools/digest_sa_module.py and bench.py --dump-outputs in deterministic mode cover that).

Reaches the plans only through what every tree since the step-list refactor has: FusedRuntime._step_plan for the update steps and,
for runtime.feature_forward and the stand-alone PointnetSAModule path, a spy on engine.Plan.run that records each distinct plan at
its first run.

  step      B = 32, after two real steps: ddpg_td3_aux.yaml and bc_dagger_aux.yaml, both input sets, policy / non-policy step,
            train / update_parameters(test=True); step and prefetch lists with item count, whichs and segment count
  switches  the ddpg_td3_aux.yaml lists once per launch-selecting switch of engine.py at its non-default value
  feature   the four runtime.feature_forward plans (value x train) at B = 2
  module    forward-train, backward and forward-eval plans of the MODULE_CASES below (the smallest shapes that reach each branch of
            sa_function._StageRun), two of them again with coordinate_grad; a shape an entry point refuses when the plan runs
            (96 output channels: gad_segment_pool takes powers of two from 8 to 1024) leaves the refusal and the plans built so far"""
import argparse
import contextlib
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (name, module keywords, B, N); every module takes mlp[0] feature channels
MODULE_CASES = (
    ("fused_pool", dict(mlp=[4, 32, 32, 64], npoint=16, radius=0.3, nsample=8), 2, 64),
    ("segment_pool", dict(mlp=[4, 32, 32, 32], npoint=16, radius=0.3, nsample=8), 2, 64),             # 32 % 64 != 0: gad_segment_pool
    ("refused_96", dict(mlp=[4, 32, 32, 96], npoint=16, radius=0.3, nsample=8), 2, 64),               # gad_segment_pool has no C = 96
    ("padded_features", dict(mlp=[6, 32, 32, 64], npoint=16, radius=0.3, nsample=8), 2, 64),          # 6 -> 8 columns
    ("split_layer1", dict(mlp=[32, 32, 32, 64], npoint=16, radius=0.3, nsample=8), 2, 64),            # layer 1 gets a split mirror
    ("group_all", dict(mlp=[4, 32, 32, 64], npoint=None, radius=None, nsample=None), 2, 64),
    ("tiled_fps", dict(mlp=[4, 32, 32, 64], npoint=32, radius=0.3, nsample=8), 2, 20),                # npoint > N
    ("msg", dict(mlps=[[4, 32, 32, 64], [4, 32, 32, 64]], npoint=16, radii=[0.2, 0.4], nsamples=[8, 16]), 2, 64),
    ("sa1_streaming", dict(mlp=[4, 64, 64, 128], npoint=128, radius=0.1, nsample=64), 4, 1024),       # 32768 rows
)
COORD_CASES = ("fused_pool", "group_all")
SWITCHES = (("DEFER_BN_WIDE", False, {}), ("INLINE_BN_BWD", False, {}), ("FUSED_SA1_BWD", False, {}), ("FUSED_WIDE_BWD", True, {}),
            ("CONCURRENT_DW", False, {}), ("RECOMP_SA1", True, {"mfma_split": 0}))


def _words(x, typ, out):
    """x of ctypes type typ (an instance, or what a structure field of that type reads back as) -> words appended to out"""
    if issubclass(typ, C.Structure):
        for name, t in typ._fields_:
            _words(getattr(x, name), t, out)
    elif issubclass(typ, C.Array):
        for y in x:
            _words(y, typ._type_, out)
    else:
        v = x.value if isinstance(x, C._SimpleCData) else x
        if typ in (C.c_void_p, C.c_char_p):
            out.append("P" if v else "0")
        elif typ in (C.c_float, C.c_double):
            out.append(repr(float(v)))
        else:
            out.append(str(int(v)))


def item_line(it):
    head = "%s %s %s %s %s" % (it.kind, it.on, it.on2, it.name, it.tag)
    out = []
    if it.kind == "memcpy":
        out = ["P" if it.words[0] else "0", "P" if it.words[1] else "0", str(it.words[2])]
    elif it.kind == "call":
        for x in it.argv:
            _words(x, type(x), out)
    return head + (" | " + " ".join(out) if out else "")


def dump_plan(f, title, plan):
    from ga_ddpg_amd import engine
    c = engine._Compiled(plan)
    f.write("== %s: %d items, whichs %s, %d segments\n" % (title, len(plan.calls), c.whichs, len(c.handles)))
    for it in plan.calls:
        f.write(item_line(it) + "\n")


@contextlib.contextmanager
def spy_plans():
    """the distinct plans run inside the block, in the order of their first run"""
    from ga_ddpg_amd import engine
    seen, real = [], engine.Plan.run

    def run(self, *a, **k):
        if not any(p is self for p in seen):
            seen.append(self)
        return real(self, *a, **k)
    engine.Plan.run = run
    try:
        yield seen
    finally:
        engine.Plan.run = real


# ---------------------------------------------------------------------------------------------------------------- update steps
def _step_lists(f, label, cfg_name, B=32):
    import numpy as np
    import torch
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    from ga_ddpg_amd.experiments.config import load_cfg
    from ga_ddpg_amd.synth_data import fill_synthetic_buffer, sample_valid_batch
    from tests.test_gpu_step import _filled_agent
    torch.manual_seed(5)
    agent, _ = _filled_agent(cfg_name, 3)
    mem = BaseMemory(600, load_cfg(cfg_name), point_dtype=np.float32)
    fill_synthetic_buffer(mem, 600, seed=5)
    rng = np.random.default_rng(1)
    bc = not hasattr(agent, "critic")
    if not bc:
        agent.update_step = 1
    for i in range(2):
        batch = sample_valid_batch(mem, B, rng)
        kw = {} if bc else dict(noise_u=rng.random((B, 6)).astype(np.float32))
        agent.update_parameters(batch, agent.update_step, i, **kw)
        agent.step_scheduler(agent.update_step)
    torch.cuda.synchronize()
    rt = agent._rt
    for ev in ((False,) if bc else (False, True)):
        rt._eval = ev
        try:
            for st in (0, 1):
                for policy in ((False,) if bc else (False, True)):
                    ent = rt._step_plan(st, policy)
                    what = "%s %s set %d policy %d eval %d" % (label, cfg_name, st, policy, ev)
                    dump_plan(f, what + " step", ent["plan"])
                    dump_plan(f, what + " prefetch", ent["pre"])
        finally:
            rt._eval = False


def step_lists(f):
    for cfg_name in ("ddpg_td3_aux.yaml", "bc_dagger_aux.yaml"):
        _step_lists(f, "step", cfg_name)


def switch_lists(f):
    from ga_ddpg_amd import engine, hip
    for name, value, options in SWITCHES:
        keep = getattr(engine, name)
        keep_opt = {k: hip.get_option(k) for k in options}
        setattr(engine, name, value)
        for k, v in options.items():
            hip.set_option(k, v)
        try:
            _step_lists(f, "switch %s=%d" % (name, value), "ddpg_td3_aux.yaml")
        finally:
            setattr(engine, name, keep)
            for k, v in keep_opt.items():
                hip.set_option(k, v)


# ---------------------------------------------------------------------------------------------------------------- feature_forward
def feature_lists(f, B=2):
    import torch
    from ga_ddpg_amd import runtime
    from ga_ddpg_amd.core import networks
    torch.manual_seed(11)
    fe = networks.PointNetFeature(input_dim=5, extra_latent=1, action_concat=True).cuda()
    pc = torch.rand(B, 10, 1024, device="cuda") * 0.2
    for train in (True, False):
        fe.train(train)
        for value in (False, True):
            with spy_plans() as seen, torch.no_grad():
                runtime.feature_forward(fe, pc, value=value)
            for i, p in enumerate(seen):
                dump_plan(f, "feature value %d train %d plan %d" % (value, train, i), p)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- module path
def build_module(kw, coordinate_grad=False, seed=3):
    import torch
    from ga_ddpg_amd.pointnet2_ops import pointnet2_modules as pm
    torch.manual_seed(seed)
    extra = dict(coordinate_grad=True) if coordinate_grad else {}
    cls = pm.PointnetSAModuleMSG if "mlps" in kw else pm.PointnetSAModule
    return cls(**{k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()}, **extra).cuda()


def module_inputs(kw, B, N, seed=4):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = (kw["mlps"][0] if "mlps" in kw else kw["mlp"])[0]
    xyz = torch.rand(B, N, 3, device="cuda", generator=g)
    feats = torch.randn(B, c, N, device="cuda", generator=g)
    return xyz, feats


def run_module(mod, xyz, feats, coord=False):
    """one training forward + backward, then one eval forward -> (new_xyz, output of the training forward, eval output)"""
    import torch
    mod.train()
    xyz = xyz.clone().requires_grad_(coord)
    feats = feats.clone().requires_grad_(True)
    new_xyz, out = mod(xyz, feats)
    g = torch.Generator(device="cuda").manual_seed(9)
    loss = (out * torch.randn(out.shape, device="cuda", generator=g)).sum()
    if coord and new_xyz is not None:
        loss = loss + (new_xyz * torch.randn(new_xyz.shape, device="cuda", generator=g)).sum()
    loss.backward()
    mod.eval()
    with torch.no_grad():
        _, out_eval = mod(xyz.detach(), feats.detach())
    torch.cuda.synchronize()
    return new_xyz, out, out_eval, xyz, feats


def module_lists(f):
    cases = [(n, kw, B, N, False) for n, kw, B, N in MODULE_CASES]
    cases += [(n + "+coordinate_grad", kw, B, N, True) for n, kw, B, N in MODULE_CASES if n in COORD_CASES]
    for name, kw, B, N, coord in cases:
        mod = build_module(kw, coord)
        xyz, feats = module_inputs(kw, B, N)
        refused = None
        with spy_plans() as seen:
            try:
                run_module(mod, xyz, feats, coord)
            except RuntimeError as e:          # (an entry point that refuses the shape when the plan runs: the plans seen so far stay)
                refused = str(e)
        if refused is not None:
            f.write("-- module %s: refused at run: %s\n" % (name, refused))
        for i, p in enumerate(seen):
            dump_plan(f, "module %s B %d N %d plan %d" % (name, B, N, i), p)


SECTIONS = dict(step=step_lists, switches=switch_lists, feature=feature_lists, module=module_lists)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--sections", default="step,switches,feature,module")
    a = ap.parse_args()
    import torch
    from ga_ddpg_amd import engine
    if not torch.cuda.is_available():
        raise SystemExit("dump_launch_lists: needs a GPU (the plans are built over device buffers, after real steps)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for s in a.sections.split(","):
            SECTIONS[s](f)
            f.flush()
            print("section %s done" % s)
            sys.stdout.flush()
        f.write("side streams %s\n" % sorted(str(k) for k in engine._SIDE))
    import hashlib
    data = open(a.out, "rb").read()
    print("%s: %d lines, sha256 %s" % (a.out, data.count(b"\n"), hashlib.sha256(data).hexdigest()))


if __name__ == "__main__":
    main()
