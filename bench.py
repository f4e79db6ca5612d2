"""bench.py -- DDPG gradient steps / second of the fused MI355X path (BASELINE.json metric).

    python bench.py --gpus 1 --steps 200 --warmup 50
    python bench.py --gpus 1 --steps 200 --warmup 50 --full    # + every other figure and check listed below
    python bench.py --gpus 1 --steps 200 --warmup 50 --dump-outputs DIR
    python bench.py --gpus N --steps K --warmup W          # N > 1: launches the N ranks itself (torch.distributed.run)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, takes W warm-up steps, times K steps and prints the result line (`metric`, `value`, `unit`,
`higher_is_better`, `dtype`, `ms_per_step` = milliseconds of one timed step, `losses` of the last step).  Everything else on
the line -- the probe steps and in-kernel stamps behind `roofline` / `kernels`, the synchronous-loop and host-fed rates, both
arithmetic modes, `sa_kernel_hbm` / `sa_kernel_mfma`, `cpu_baseline`, the replica check of N > 1 -- is measured with `--full` only
(`--no-cpu-baseline`, `--no-host-rate`, `--no-sa-kernel` and `--probe-steps` trim a --full run).
--dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step computed as DIR/<name>.npy -- the loss dict
update_parameters returns (float64 scalars) and the step's policy / critic / TD-target tensors the agent keeps (float32; a
fixed, seeded sample of any array above 2 M values).  The inputs depend on the
arguments alone (seeded weights, replay buffer, minibatches and TD3 noise), so two builds compare output for output.  A step is
not bit-reproducible (f64 atomics in varying order, DESIGN.md section 8: one step repeats to rounding) and training amplifies
that from step to step (after 250 steps two runs differed in pi by up to 0.7).  So with --dump-outputs the last timed step starts
from the seeded initial state again -- parameters of every network and their Adam moments, restored between fences before it is
enqueued -- and takes its own minibatch, noise draw and step index: what it returns repeats from run to run to rounding.  The
agent's internal state is not dumped: the backward's atomic sums leave the actor phase's encoder gradients a few 1e-4 apart
(entry-relative) between runs, and Adam turns an entry whose gradient is zero up to rounding into a step of about +-lr.

Workload (BASELINE.json configs[1], SURVEY 8d "config 2"): DDPG/TD3 update with goal-auxiliary heads
(ddpg_td3_aux.yaml), batch 256 per GPU, 1024-point clouds, synthetic seeded replay buffer, random-init
weights, alternating policy / non-policy steps.  A "step" = one Agent.update_parameters call.
`value` is measured with the minibatches already resident in HBM (a ring of pre-sampled batches);
the host-sampling + PCIe inclusive rate is reported separately as `value_host_inclusive`.
N > 1: one process per GPU, batch rows sharded (256 per rank -> weak scaling), one RCCL all-reduce of
the flat gradients per optimiser phase (ga_ddpg_amd.parallel).  `value` is then the whole-job aggregate: B=256
minibatch-steps per second summed over the ranks (= optimiser iterations/s x N; `config.iterations_per_s` holds the
iteration rate), time = max over ranks between two barrier + synchronize fences.

Extra objects on the JSON line:
  roofline      the DOMINANT kernel of the step = the kernel symbol with the largest summed launch time per step (symbols within
                5 % of the largest: the one with the most stand-alone time per step -- in-step durations of side-lane kernels are
                inflated by what runs beside them); `roofline.by_kernel`: the five largest symbols in the same units
                (every tagged launch stamps its own first-wavefront-start / last-wavefront-end on the device wall clock:
                gad_timing_slot -- the dispatch duration a profiler reports; a `--probe-steps` pass during warm-up picks the symbol,
                its launches are then timed during the K timed steps).  MFMA-bound kernels (64x64 tile
                family): `achieved` = EXECUTED FLOPs (de-duplicated rows x K x N x 2, summed over the layers the
                symbol serves) / their summed duration, against the 157.3 TFLOP/s FP32-MFMA peak.  HBM-bound kernels
                (streaming SA1 family): algorithmic bytes / duration against 8 TB/s.  `frac` <= 1 by construction;
                `dense_equiv` is the same time priced with the padded-neighbourhood FLOPs the reference computes
                (SURVEY 8d); `traffic` = HBM bytes per launch from this round's rocprofv3 PMC passes of the same command
                (FETCH_SIZE / WRITE_SIZE in separate passes, tools/collect_profiles.sh -> profiles/rNN_traffic.json: counters
                cannot be collected inside an untraced run; `traffic_source` names the file read) or null; `kernel_avg_us` is
                what profiles/rNN_*kernel_stats* must agree with.
  kernels       the per-symbol table behind that choice (per-step time, launches, achieved fraction of its bound).
  cpu_baseline  the CPU oracle (pure-PyTorch port of the reference step) timed on this box's cores, rank 0 / N=1
                only: ONE full B=256 update step (about 20 - 30 s of CPU work) after a small warm-up step.
  sa_kernel_hbm BASELINE's second metric: HBM GB/s of the streaming set-abstraction kernels of this workload
                (HIP events; algorithmic bytes and PMC traffic) and of the materialising configs[3] kernel.
  value_host_inclusive / value_device_replay: the same loop fed by host sampling + PCIe upload / by the
                GPU-resident replay mirror (never `value`).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP32_MFMA_PEAK = 157.3e12     # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
BF16_MFMA_PEAK = 2500.0e12    # same table: v_mfma_f32_32x32x16_bf16, dense (no sparsity)
SPLIT_PRODUCTS = 6            # bf16 term products per f32-equivalent product in the split-bf16 form (csrc/gemm.hip)
DTYPE_F32 = "f32"
DTYPE_SPLIT = "f32 (3xbf16-split products, f32 accumulate)"
SEED = 20260928

# dense algorithmic MACs per sample of each shared-MLP layer, as the reference computes them
# (rows = npoint * nsample incl. padded duplicates), keyed by launch tag.
def dense_layer_macs(tag, c_in):
    sa = {"sa1": (32 * 64, [(3 + c_in, 64), (64, 64), (64, 128)]),
          "sa2": (32 * 128, [(131, 128), (128, 128), (128, 256)]),
          "sa3": (32, [(259, 256), (256, 256), (256, 512)])}
    kind, stage, layer = tag.split(".")
    rows, dims = sa[stage]
    k, n = dims[int(layer[1:]) - 1]
    return rows * k * n


def sa_kernel_hbm(iters=50):
    """BASELINE.json's second metric ("SA-kernel HBM GB/s") on configs[3] (B=128, N=4096, npoint 512, radius 0.1,
    nsample 64, C=4): the materialising ball-query + group kernel behind pointnet2_utils.query_and_group -- the
    HBM-bound member of the set-abstraction family (SURVEY 8d "config 4a": 148.9 MB algorithmic bytes per call: points in,
    indices + grouped (B,7,512,64) tensor out).  HIP events on the launching stream."""
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    B, N, M, S, C = 128, 4096, 512, 64, 4
    g = torch.Generator(device="cuda").manual_seed(SEED)
    xyz = torch.rand(B, N, 3, device="cuda", generator=g)
    feats = torch.randn(B, C, N, device="cuda", generator=g)
    new_xyz = pu.gather_operation(xyz.transpose(1, 2).contiguous(), pu.furthest_point_sample(xyz, M)).transpose(1, 2).contiguous()
    from ga_ddpg_amd import hip
    idx = torch.empty(B, M, S, dtype=torch.int32, device="cuda")
    out = torch.empty(B, 3 + C, M, S, dtype=torch.float32, device="cuda")

    def launch():                                                  # the C-ABI entry point, caller-allocated outputs
        hip.call("gad_query_and_group", new_xyz, xyz, feats, B, C, N, M, 0.1, S, idx, out)

    for _ in range(5):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    nbytes = B * N * (3 + C) * 4 + B * M * S * 4 + B * M * S * (3 + C) * 4
    gbps = nbytes / (ms * 1e-3) / 1e9
    return {"kernel": "ball_query_cells_kernel via gad_query_and_group (configs[3]: B=128, N=4096, npoint=512, r=0.1, nsample=64, "
                      "C=4)", "bound": "hbm", "algorithmic_bytes": nbytes, "launch_ms": ms, "achieved": gbps, "peak": 8000.0,
            "unit": "GB/s", "frac": gbps / 8000.0,
            "note": "back-to-back launches between HIP events on the launching stream; the output (134 MB) fits the 256 MB "
                    "Infinity Cache, so part of the write-back to HBM overlaps the next launch"}


def sa_kernel_mfma(iters=6):
    """SURVEY 8d "config 4b" (BASELINE configs[3]): the FUSED set-abstraction stack -- two PointnetSAModules, radii 0.1 / 0.2,
    B = 128, N = 4096 -- forward AND backward through the pointnet2_ops facade (torch.autograd.Function over the same
    gemm_fwd / dX / dW kernels as the update step, de-duplicated neighbourhood rows), as the MFMA-bound member of the family:
    executed FLOPs = live rows x K x N x 2 per layer, x 3 for forward + dX + dW, over the wall time of one
    forward + backward between two HIP events on the launching stream (geometry -- FPS, ball query, row compaction -- and
    the facade's hand-over transposes included: this is the operator as a user calls it inside a training iteration, gradients
    reset before every pass as optimizer.zero_grad() leaves them, not a kernel in isolation)."""
    from ga_ddpg_amd.pointnet2_ops import pointnet2_modules as pm
    from ga_ddpg_amd import hip as _hip
    split_active = bool(_hip.get_option("mfma_split"))
    B, N = 128, 4096
    g = torch.Generator(device="cuda").manual_seed(SEED)
    xyz = torch.rand(B, N, 3, device="cuda", generator=g)
    feats = torch.randn(B, 4, N, device="cuda", generator=g).requires_grad_(True)
    sa = [pm.PointnetSAModule(npoint=512, radius=0.1, nsample=64, mlp=[4, 64, 64, 128]).cuda().train(),
          pm.PointnetSAModule(npoint=128, radius=0.2, nsample=128, mlp=[128, 128, 128, 256]).cuda().train()]
    probe = torch.randn(B, 256, 128, device="cuda", generator=g)

    params = [p for m in sa for p in m.parameters()]

    def fwd_bwd():                                         # one training iteration's worth: gradients reset as optimizer.zero_grad()
        for p in params:                                   # does (set_to_none: the backward then assigns instead of accumulating)
            p.grad = None
        feats.grad = None
        x1, f1 = sa[0](xyz, feats)
        _, f2 = sa[1](x1, f1)
        (f2 * probe).sum().backward()

    for _ in range(2):
        fwd_bwd()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fwd_bwd()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    rows, flops = [], 0.0
    for mod, dims in ((sa[0], [(7, 64), (64, 64), (64, 128)]), (sa[1], [(131, 128), (128, 128), (128, 256)])):
        run = mod.__dict__["_gad_rt"]["net"].free[(B, N if mod is sa[0] else 512)][-1]
        n = int(run.rows["n"].item())
        rows.append(n)
        flops += 3.0 * sum(2.0 * n * k * c for k, c in dims)
    dense = 3.0 * B * (512 * 64 * (7 * 64 + 64 * 64 + 64 * 128) + 128 * 128 * (131 * 128 + 128 * 128 + 128 * 256)) * 2.0
    tf = flops / (ms * 1e-3) / 1e12
    return {"kernel": "PointnetSAModule x 2 forward + backward through ga_ddpg_amd.pointnet2_ops (configs[3]: B=128, N=4096, "
                      "npoint 512 / 128, radii 0.1 / 0.2, nsample 64 / 128)", "bound": "mfma", "ms_fwd_bwd": ms,
            "live_rows": rows, "padded_rows": [B * 512 * 64, B * 128 * 128], "executed_gflop": flops / 1e9,
            "achieved": tf, "peak": FP32_MFMA_PEAK / 1e12, "unit": "TFLOP/s", "frac": tf / (FP32_MFMA_PEAK / 1e12),
            # the stack's layer GEMMs run the split-bf16 kernels when the package default is active: the same time priced against
            # the pipe they use (6 bf16 term products per f32-equivalent product, 2.5 PF dense) -- VERDICT r05 weak 10
            "arithmetic": "split-bf16" if split_active else "f32 MFMA",
            "frac_bf16": (tf * SPLIT_PRODUCTS / (BF16_MFMA_PEAK / 1e12)) if split_active else None,
            "methodology": "gradients set to None before every pass (since round 5: not comparable with r04's accumulate-into-grad figure)",
            "dense_equiv_tflops": dense / (ms * 1e-3) / 1e12,
            "note": "whole operator incl. FPS (512 of 4096 points: one CU per cloud, VALU-bound), ball query, row compaction and "
                    "the autograd facade's copies; HIP events on the launching stream"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--no-sa-kernel", action="store_true", help="skip the configs[3] SA-kernel HBM measurement")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--buffer", type=int, default=20000, help="synthetic replay transitions per rank")
    ap.add_argument("--ring", type=int, default=8, help="pre-sampled minibatches kept resident in HBM")
    ap.add_argument("--probe-steps", type=int, default=10, help="eager steps with HIP events around every tagged launch "
                                                                "(roofline / kernel table), after the timed region")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-host-rate", action="store_true")
    ap.add_argument("--full", action="store_true", help="every figure and check beyond the headline rate (roofline, kernel "
                                                        "table, sync / host-fed rates, both modes, SA kernels, CPU baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's outputs as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


DUMP_CAP = 2 * 1024 * 1024       # values per dumped array; larger arrays are sampled at fixed, seeded positions
STATE_FLATS = ("pol", "pol_t", "cr", "cr_t", "enc", "venc")      # every network the update step reads and writes


def training_state(rt):
    """copies of what a step carries over to the next one: the parameters of every network (targets included) and their Adam
    moments (the optimiser's step counts, learning-rate schedules and the minibatch ring follow from the step index alone)"""
    return {n: [t.clone() for t in (f.master, f.exp_avg, f.exp_avg_sq)] for n in STATE_FLATS for f in [getattr(rt, n).flat]}


def restore_training_state(rt, state):
    for n, saved in state.items():
        f = getattr(rt, n).flat
        for dst, src in zip((f.master, f.exp_avg, f.exp_avg_sq), saved):
            dst.copy_(src)
        f.sync_packed()                                      # the packed layout and the split-bf16 mirrors follow `master`


def dump_outputs(out_dir, result, tensors):
    """`result`: the loss dict of the last timed step; `tensors`: name -> host copy of what that step left on the agent"""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"loss_" + k: np.asarray([float(v)], dtype=np.float64) for k, v in result.items()}
    for name, t in tensors.items():
        a = t.detach().float().cpu().numpy()
        if a.size > DUMP_CAP:
            pick = np.sort(np.random.default_rng(SEED).choice(a.size, DUMP_CAP, replace=False))
            a = a.reshape(-1)[pick]
        arrays[name] = np.ascontiguousarray(a, dtype=np.float32)
    total = sum(a.nbytes for a in arrays.values())
    assert total <= 64 * 1024 * 1024, "dump of %d bytes exceeds 64 MB" % total
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return total


def cpu_baseline(cfg, batch, noise):
    """The same workload on the host cores: ONE full DDPG update step (B = the bench batch, N = 1024) of the CPU oracle
    (a port of the reference step; the reference itself cannot travel) after an 8-row warm-up step.  Threads capped at
    64: torch's CPU kernels get slower beyond that on this many-core host (256 threads: 185 s for a B=256 step)."""
    from ga_ddpg_amd.experiments.config import load_cfg
    from oracle import ref_step
    cores = min(os.cpu_count() or 1, 64)
    torch.set_num_threads(cores)
    torch.manual_seed(1234)
    oracle = ref_step.OracleAgent(load_cfg("ddpg_td3_aux.yaml").RL_TRAIN)
    B = len(batch["reward_batch"])

    def head(n):
        return {k: (v[:n] if hasattr(v, "shape") and v.ndim > 0 and v.shape[0] == B else v) for k, v in batch.items()}
    oracle.update_parameters(head(8), noise_u=noise[:8])                 # page-in / warm-up on 8 rows
    t0 = time.time()
    oracle.update_parameters(batch, noise_u=noise)
    dt = time.time() - t0
    return {"value": 1.0 / dt, "unit": "steps/s", "cores": cores, "kind": "port",
            "sample": "1 full DDPG update step of the CPU oracle (B=%d, N=1024), %.1f s on %d threads" % (B, dt, cores)}


# ----------------------------------------------------------------------------------------------------------------------
# kernel table: tag -> (kernel symbol, bound, executed FLOPs, algorithmic bytes) per launch.  The symbol is the one the
# library REPORTS for the tagged call (gad_last_kernel -> engine.timing_routes(): csrc/gemm.hip routes SA1 (>= 32768 rows,
# 64-wide) to the streaming kernels (HBM-bound; SA1 layers 3 / 2 backward with weight gradients: the fused dX + dW
# kernel), SA2 / SA3 to the wide-tile kernels (FP32 MFMA-bound; generic 64x64 tiles where a shape does not fit), FC / heads
# (<= 1024 rows) to the skinny split-K kernels (latency-bound)); the prices are per layer.
# ----------------------------------------------------------------------------------------------------------------------
SA_DIMS = {"sa1": [(None, 64), (64, 64), (64, 128)], "sa2": [(131, 128), (128, 128), (128, 256)],
           "sa3": [(259, 256), (256, 256), (256, 512)], "fc": [(512, 1024), (1024, 512)]}
DENSE_ROWS = {"sa1": 32 * 64, "sa2": 32 * 128, "sa3": 32, "fc": 1}
ROUTE_SYMBOL = {"gemm_fwd(stream)": "gemm_fwd_stream_kernel", "gemm_fwd(wide)": "gemm_fwd_wide_kernel", "gemm_fwd(skinny)": "gemm_fwd_skinny_kernel",
                "gemm_fwd": "gemm_fwd_kernel", "gemm_dx(stream)": "gemm_dx_stream_kernel", "gemm_dx(wide)": "gemm_dx_wide_kernel",
                "gemm_dx(skinny)": "gemm_dx_skinny_kernel", "gemm_dx": "gemm_dx_kernel", "gemm_dx(action stream)": "dx_action_stream_kernel", "gemm_dw(stream)": "gemm_dw_stream_kernel",
                "gemm_dw(gather stream)": "gemm_dw_gather_stream_kernel", "gemm_dw(wide)": "gemm_dw_wide_kernel",
                "gemm_dw(skinny)": "gemm_dw_skinny_kernel", "gemm_dw": "gemm_dw_kernel", "gemm_bwd(stream)": "gemm_bwd_stream_kernel", "gemm_bwd(wide)": "gemm_bwd_wide_kernel",
                # split-bf16 forms (library option "mfma_split"): same layers, products on v_mfma_f32_32x32x16_bf16
                "gemm_fwd(stream split)": "gemm_fwd_stream_kernel<split>", "gemm_fwd(wide split)": "gemm_fwd_wide_kernel<split>",
                "gemm_dx(wide split)": "gemm_dx_wide_kernel<split>", "gemm_dw(wide split)": "gemm_dw_wide_split_kernel",
                "gemm_bwd(stream split)": "gemm_bwd_stream_split_kernel", "gemm_dx(stream split)": "gemm_bwd_stream_split_kernel<dX only>"}
ROUTES = {}                 # tag -> routed kernel family, filled from engine.timing_routes() after each probe


def tag_info(tag, rows, B):
    """(symbol, bound, executed_flops, algorithmic_bytes, dense_flops) of one launch of `tag`; rows = de-duplicated rows
    per stage"""
    parts = tag.split(".")
    kind, stage = parts[0], parts[1]
    if kind == "pool" or tag not in ROUTES:
        return None
    layer = int(parts[2][1:]) if len(parts) > 2 else 0
    if stage.startswith("fc"):                      # fwd.fc1 / fwd.fc2 carry the layer in the stage name
        layer, stage = (int(stage[2:]) if len(stage) > 2 else layer), "fc"
    if layer == 0:
        return None
    k, n = SA_DIMS[stage][layer - 1]
    if k is None:
        k = 13.0                                    # SA1 layer 1: 3 + 4 (policy encoder) or 3 + 10 (value encoder) inputs
    r = float(rows[stage])
    flops = 2.0 * r * k * n
    dense = 2.0 * B * DENSE_ROWS[stage] * k * n
    route = ROUTES[tag]
    sym = ROUTE_SYMBOL.get(route, route)
    stream = "stream" in route
    if kind == "fwd":
        nbytes = r * (min(k, 16 if stream and layer == 1 else k) + n) * 4.0
        if layer == 3 and stage != "fc":            # pooled layers: the keys of the fused max-pool are per group, not per row
            nbytes += 2.0 * (B * (32 if stage != "sa3" else 1)) * n * 4
    elif kind == "dx":
        nbytes = r * (2 * n + 2 * k) * 4.0           # z and dY of this layer in, dY of the previous layer out, its z for the sums
    elif kind == "bwd":                              # dX + dW in one pass: the dX kernel's traffic, twice the FLOPs
        nbytes = r * (2 * n + 2 * k) * 4.0
        flops, dense = 2.0 * flops, 2.0 * dense
    else:
        nbytes = r * (2 * n + k) * 4.0               # z, dY of this layer and the layer input
    bound = "hbm" if stream else ("latency" if "skinny" in route else "mfma")
    return sym, bound, flops, nbytes, dense


def kernel_table(by_tag, rows, B, steps):
    """aggregate the tagged launches by kernel symbol: per-step time, launches, executed TFLOP/s, algorithmic GB/s"""
    fam = {}
    for tag, ms in by_tag.items():
        info = tag_info(tag, rows, B)
        if info is None:
            continue
        sym, bound, fl, by, dense = info
        f = fam.setdefault(sym, {"bound": bound, "ms": 0.0, "launches": 0, "flops": 0.0, "bytes": 0.0, "dense": 0.0, "tags": []})
        f["ms"] += float(np.sum(ms))
        f["launches"] += len(ms)
        f["flops"] += fl * len(ms)
        f["bytes"] += by * len(ms)
        f["dense"] += dense * len(ms)
        f["tags"].append(tag)
    out = {}
    for sym, f in fam.items():
        sec = f["ms"] * 1e-3
        tf, gb = f["flops"] / sec / 1e12, f["bytes"] / sec / 1e9
        split = "split" in sym
        if f["bound"] == "hbm":
            frac = gb / 8000.0
        elif split:                                  # six bf16 MFMA products per f32-equivalent product, against the bf16 peak
            frac = SPLIT_PRODUCTS * tf / (BF16_MFMA_PEAK / 1e12)
        else:
            frac = tf / (FP32_MFMA_PEAK / 1e12)
        out[sym] = {"bound": f["bound"], "ms_per_step": f["ms"] / steps, "launches_per_step": f["launches"] / float(steps),
                    "kernel_avg_us": 1e3 * f["ms"] / f["launches"], "executed_tflops": tf, "algorithmic_gbps": gb,
                    "frac": frac, "dense_equiv_tflops": f["dense"] / sec / 1e12, "tags": sorted(f["tags"])}
        if split:                                    # (executed_tflops stays f32-equivalent: de-duplicated rows x K x N x 2)
            out[sym]["arithmetic"] = "split-bf16"
            out[sym]["frac_f32_equiv"] = tf / (FP32_MFMA_PEAK / 1e12)
            if f["bound"] != "hbm":
                out[sym]["executed_bf16_tflops"] = SPLIT_PRODUCTS * tf
    return out


def launch_ranks(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it (the driver's invocation form; the reference spreads
    over GPUs from one process as well: nn.DataParallel, core/utils.py:202): start N ranks of this file under
    torch.distributed.run -- one process per GPU, rendezvous on 127.0.0.1 -- and relay their output; rank 0's JSON line
    stays the last line."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")        # dmabuf IPC only on this driver (RCCL across processes)
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.call(cmd, env=env)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # GAD_BENCH_BACKEND=gloo lets the N > 1 path be exercised on a box with fewer GPUs than ranks (ranks then share
    # devices round-robin; RCCL refuses that) -- a plumbing check, not a measurement
    backend = os.environ.get("GAD_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local if backend == "nccl" else local % torch.cuda.device_count())
    dp = None
    # GAD_BENCH_FORCE_DP=1: run the data-parallel hooks (count exchange, gradient all-reduces, scalar reduction) over a
    # ONE-rank RCCL group -- what they cost per step without any transport, the floor under the N > 1 numbers
    force_dp = world == 1 and os.environ.get("GAD_BENCH_FORCE_DP", "0") == "1"
    if world > 1 or force_dp:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29571")
        dist.init_process_group(backend, rank=rank, world_size=world)
    from ga_ddpg_amd import engine
    from ga_ddpg_amd.api import make_agent
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    from ga_ddpg_amd.parallel import DataParallelContext, mask_counts
    from ga_ddpg_amd.synth_data import fill_synthetic_buffer, sample_valid_batch

    from ga_ddpg_amd import hip as _hip
    # arithmetic of the layer GEMMs' products in THIS run's `value`: the library default (0: FP32 MFMA; non-zero: split-bf16 MFMAs,
    # include/gaddpg.h "mfma_split"), or the GAD_OPT_mfma_split override
    split_mode = _hip.get_option_default("mfma_split")
    _hip.set_option("mfma_split", split_mode)
    torch.manual_seed(1234)                      # identical initial weights on every rank
    agent, cfg = make_agent("ddpg_td3_aux.yaml")
    B = args.batch
    mem = BaseMemory(args.buffer, cfg, point_dtype=np.float32)
    fill_synthetic_buffer(mem, args.buffer, seed=SEED + rank)
    rng = np.random.default_rng(SEED + 1000 + rank)
    host_batches = [sample_valid_batch(mem, B, rng) for _ in range(args.ring)]
    rt = agent.runtime(B, host_batches[0]["point_state_batch"].shape[2])
    if world > 1 or force_dp:
        dp = DataParallelContext()
        agent._dp = dp
        dp.attach(rt)
        dp.broadcast_parameters([rt.pol.flat, rt.pol_t.flat, rt.cr.flat, rt.cr_t.flat, rt.enc.flat, rt.venc.flat])
    # --dump-outputs: the seeded initial state, which the last timed step starts from again (see the module docstring)
    initial_state = training_state(rt) if args.dump_outputs else None
    from ga_ddpg_amd.runtime import BATCH_KEYS
    ring = []
    for hb in host_batches:
        d = {k: torch.as_tensor(np.ascontiguousarray(hb[k], dtype=np.float32)).cuda() for k in BATCH_KEYS}
        d["mask_counts"] = mask_counts(hb)
        ring.append(d)
    torch.cuda.synchronize()
    ready = torch.cuda.Event()
    ready.record()
    for d in ring:
        d["ready_event"] = ready          # resident and complete: the runtime's prefetch stream need not wait for the caller's

    def step(i, sync=False):
        # sync=False: the call returns once the step is enqueued (its result dict fills in on first read); the host stages
        # and enqueues the next step while this one runs.  Every step is complete at the closing fence.
        out = agent.update_parameters(ring[i % len(ring)], agent.update_step, i, sync=sync)
        agent.step_scheduler(agent.update_step)
        return out

    def fence():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for i in range(args.warmup):
        step(i)

    if args.full:
        # ---- which kernel dominates?  in-kernel wall-clock stamps of every tagged launch during a few extra warm-up
        # steps, inside the overlapped step -- and once more with the step serialised on one stream (the kernel by itself)
        def probe(serial, n):
            engine.SERIAL = serial
            engine.timing_start("*", capacity=n * 200)
            for i in range(n):
                step(args.warmup + i)
            acc = engine.timing_stop()
            ROUTES.update(engine.timing_routes())
            engine.SERIAL = False
            return acc
        probe_n = args.probe_steps + args.probe_steps % 2            # policy and non-policy steps in equal number
        by_tag = probe(False, probe_n)
        alone = probe(True, probe_n) if world == 1 else {}
        rows = {"sa1": int(rt.geo.rows[0]["n"].item()), "sa2": int(rt.geo.rows[1]["n"].item()),
                "sa3": int(rt.geo.rows[2]["n"].item()), "fc": B}
        table = kernel_table(by_tag, rows, B, probe_n)
        table_alone = kernel_table(alone, rows, B, probe_n) if alone else {}
        priced = {k: v for k, v in table.items() if v["bound"] in ("mfma", "hbm")}
        dom = max(priced, key=lambda k: priced[k]["ms_per_step"])
        # two symbols run neck and neck (the wide forward on the chains, 27 launches; the wide dW on its side lanes, 12 launches whose
        # in-step duration is inflated 2-3 x by what runs beside them) and the probe's order flipped from run to run: among the
        # symbols within 5 % of the largest in-step time, the one with the most STAND-ALONE time per step is the dominant kernel
        near = [k for k in priced if priced[k]["ms_per_step"] >= 0.95 * priced[dom]["ms_per_step"]]
        if len(near) > 1 and table_alone:
            dom = max(near, key=lambda k: table_alone.get(k, {}).get("ms_per_step", 0.0))
        # HIP events around the launches of the dominant kernel only, in the timed region below
        engine.timing_start(frozenset(table[dom]["tags"]), capacity=min(8192, int((args.steps // 4 + 1) * table[dom]["launches_per_step"] * 1.1) + 64))
    # ---- the timed region: K steps
    fence()
    t0 = time.perf_counter()
    for i in range(args.steps):
        if args.full:
            # the stamps cost the timed kernels ~3 % (two s_memrealtime + stores per wavefront): taken on a quarter of the steps
            engine.TIMING["enabled"] = (i % 8 in (0, 3))        # steps with and without the actor-critic term alike
        if initial_state is not None and i == args.steps - 1:
            # every earlier step is complete before the state is replaced, and the copies before the last step is enqueued
            agent.flush()
            fence()
            restore_training_state(rt, initial_state)
            fence()
        out = step(args.warmup + i)
    fence()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        # read before anything else runs on the agent: these are the buffers of the last timed step
        tensors = {"pi": agent.pi, "aux_pred": agent.aux_pred, "qf1": agent.qf1, "qf2": agent.qf2,
                   "next_q_value": agent.next_q_value, "critic_grasp_aux": agent.critic_grasp_aux}
        dump_outputs(args.dump_outputs, dict(out.items()), tensors)
    if args.full:
        timed_tags = engine.timing_stop()
        # the same steps with the host waiting for each result before it enqueues the next (the reference's loop reads its
        # losses with .item() every step): uploads, geometry and ~2 ms of launch calls then sit in front of every step
        n_sync = max(10, args.steps // 5)
        fence()
        t1 = time.perf_counter()
        for i in range(n_sync):
            step(args.warmup + args.steps + i, sync=True)
        fence()
        rate_sync = n_sync / (time.perf_counter() - t1)
        # ... and the same synchronous loop with the NEXT minibatch handed to agent.prefetch() before each update (what
        # core.train_test_offline.train_off_policy does by default: it samples one minibatch ahead): upload + geometry of step N + 1
        # run beside step N, the loop still reads every step's losses before it enqueues the next
        fence()
        t1 = time.perf_counter()
        base = args.warmup + args.steps + n_sync
        for i in range(n_sync):
            agent.prefetch(ring[(base + i + 1) % len(ring)])
            step(base + i, sync=True)
        fence()
        rate_sync_prefetch = n_sync / (time.perf_counter() - t1)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    dp_info = None
    if dp is not None:
        # self-proof of the multi-GPU line: the transport that carried the step's collectives, the rank count RCCL ITSELF
        # reports for it (ncclCommCount), and whether the replicas' parameters are still bit-identical after every step
        # of this run (all-reduced MAX / MIN of an int64 checksum) -- a collective, so every rank takes part
        torch.cuda.synchronize()
        dp_info = dp.transport()
        if args.full:
            dp_info["replicas_bit_identical"] = dp.replicas_agree([rt.pol.flat, rt.pol_t.flat, rt.cr.flat, rt.cr_t.flat, rt.enc.flat, rt.venc.flat])
        dp_info["bucketed_exchange"] = bool(getattr(rt, "bucketed", False))
        dp.close()
    def leave_group():
        # every rank leaves the process group BEFORE rank 0 prints: whatever RCCL writes to stdout while it initialises or
        # shuts down comes first and the JSON line is the last line of the job's output
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
    if rank != 0:
        leave_group()
        return
    steps_per_s = args.steps * 1.0 / dt
    # whole-job aggregate: every rank processes one B=256 minibatch per optimiser step (weak scaling), so the job does
    # world x (B=256 minibatch-steps) per iteration; at N=1 this is the plain step rate
    res = {"metric": "DDPG grad-steps/sec (B=%d, N=1024 pts)" % B, "value": steps_per_s * world, "unit": "steps/s",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": DTYPE_SPLIT if split_mode else DTYPE_F32, "data": "synthetic",
           "config": {"workload": "BASELINE configs[1]: DDPG/TD3 offline update (td3_critic_aux_policy_aux), "
                                  "batch=%d per GPU, 1024-pt clouds, synthetic replay buffer" % B,
                      "batch_per_gpu": B, "global_batch": B * world, "points": 1024,
                      "parallelism": "dp%d" % world, "iterations_per_s": steps_per_s, "mfma_split": split_mode,
                      "enqueue": "run-ahead (update_parameters(sync=False), all steps complete at the closing fence)",
                      "value_definition": "B=%d minibatch gradient steps per second summed over ranks (= iterations/s x n_gpus)" % B, "inputs": "HBM-resident ring of %d pre-sampled minibatches" % args.ring},
           "losses": {k: out[k] for k in ("critic_loss", "bc_loss", "actor_critic_loss")}}
    if args.full:
        n_stamped = sum(1 for i in range(args.steps) if i % 8 in (0, 3))
        table_timed = kernel_table(timed_tags, rows, B, n_stamped)
        d0 = table_timed.get(dom, table[dom])                           # measured over the timed region itself
        tj, tsrc = {}, None
        for rnd in ("r06", "r05", "r04", "r03", "r02"):                 # this round's PMC passes (tools/collect_profiles.sh)
            tpath = os.path.join(ROOT, "profiles", "%s_traffic.json" % rnd)
            if os.path.exists(tpath):
                tj = json.load(open(tpath))
                tsrc = "profiles/%s_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, not measured in this run)" % rnd
                break
        dom_split = "split" in dom and d0["bound"] == "mfma"
        roof = {"bound": d0["bound"], "kernel": dom, "layers": d0["tags"],
                # split-bf16 kernels: achieved = the bf16 term products the matrix pipe executed (6 per f32-equivalent product)
                # against the dense bf16 peak; frac_f32_equiv prices the same launches' f32-equivalent FLOPs against the FP32-MFMA peak
                "achieved": (d0.get("executed_bf16_tflops") if dom_split else d0["executed_tflops"]) if d0["bound"] == "mfma" else d0["algorithmic_gbps"],
                "peak": (BF16_MFMA_PEAK if dom_split else FP32_MFMA_PEAK) / 1e12 if d0["bound"] == "mfma" else 8000.0,
                "unit": "TFLOP/s" if d0["bound"] == "mfma" else "GB/s", "frac": d0["frac"],
                "frac_f32_equiv": d0.get("frac_f32_equiv"), "f32_equiv_tflops": d0["executed_tflops"] if d0["bound"] == "mfma" else None,
                "arithmetic": "split-bf16 (6 bf16 x bf16 term products per f32 product, f32 accumulate)" if "split" in dom else "f32 MFMA",
                "traffic": (tj.get(dom) or tj.get(dom.split("<")[0]) or tj.get(dom.split("<")[0].replace("_kernel", "_split_kernel")) or {}).get("bytes_per_launch"), "traffic_source": tsrc,
                "kernel_avg_us": d0["kernel_avg_us"], "launches_per_step": d0["launches_per_step"],
                "ms_per_step": d0["ms_per_step"], "dense_equiv_tflops": d0["dense_equiv_tflops"],
                "frac_alone": table_alone.get(dom, {}).get("frac"), "kernel_avg_us_alone": table_alone.get(dom, {}).get("kernel_avg_us"),
                "how": "in-kernel wall-clock stamps (gad_timing_slot) of every launch of the symbol on %d of the %d timed steps (the symbol "
                       "was chosen from a %d-step probe of every tagged launch); executed FLOPs = de-duplicated rows (sa1 %d, "
                       "sa2 %d, sa3 %d) x K x N x 2 per layer" % (n_stamped, args.steps, probe_n, rows["sa1"], rows["sa2"], rows["sa3"])}
        # the five largest symbols of the step in the same units (the driver's record keeps `roofline`, not the top-level `kernels` table)
        roof["by_kernel"] = [dict(kernel=k, bound=v["bound"], ms_per_step=v["ms_per_step"], launches_per_step=v["launches_per_step"],
                                  kernel_avg_us=v["kernel_avg_us"], frac=v["frac"], frac_f32_equiv=v.get("frac_f32_equiv"),
                                  kernel_avg_us_alone=table_alone.get(k, {}).get("kernel_avg_us"))
                             for k, v in sorted(priced.items(), key=lambda kv: -kv[1]["ms_per_step"])[:5]]
        res["config"].update(iterations_per_s_sync_each_step=rate_sync, iterations_per_s_sync_prefetch_next=rate_sync_prefetch)
        res["roofline"] = roof
    if dp_info is not None:
        res["config"].update(dp_info)
    # step-level view against the dense-FP32 roofline: mean 5.5078 GFLOP per sample and step
    res["step_dense_tflops"] = steps_per_s * world * B * 5.5078e9 / 1e12
    if args.full and world == 1 and not args.no_host_rate:
        rng2 = np.random.default_rng(7)
        n = max(40, args.steps // 4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            b = sample_valid_batch(mem, B, rng2)
            agent.update_parameters(b, agent.update_step, i)
        torch.cuda.synchronize()
        res["value_host_inclusive"] = res["config"]["value_host_inclusive"] = n / (time.perf_counter() - t0)
        # the same, with the sampling on a background thread into pinned staging sets (core/prefetch.PrefetchSampler) and
        # run-ahead steps: what a training loop over a HOST replay buffer gets
        from ga_ddpg_amd.core.prefetch import PrefetchSampler
        with PrefetchSampler(mem, B, depth=3, sample=lambda bs, clouds_out=None, pool=None: sample_valid_batch(mem, bs, rng2, clouds_out, pool)) as sampler:
            for i in range(20):                          # (the producer thread and its pinned sets reach steady state)
                agent.update_parameters(sampler.next(), agent.update_step, i, sync=False)
            torch.cuda.synchronize()
            n_pf = max(150, n)
            t0 = time.perf_counter()
            for i in range(n_pf):
                agent.update_parameters(sampler.next(), agent.update_step, i, sync=False)
            agent.flush()
            torch.cuda.synchronize()
            res["value_host_prefetch"] = res["config"]["value_host_prefetch"] = n_pf / (time.perf_counter() - t0)
        # same loop fed by the GPU-resident replay mirror: indices drawn on the host with the
        # reference's arithmetic, gather in HBM -- the rate a training loop sees without the 17 MB/step host gather
        from ga_ddpg_amd.core.device_replay import DeviceReplay
        dmem = DeviceReplay(mem)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            agent.update_parameters(dmem.sample_lazy(B, rng2), agent.update_step, i, sync=False)
        agent.flush()
        res["value_device_replay"] = res["config"]["value_device_replay"] = n / (time.perf_counter() - t0)
        # both arithmetic modes of the layer GEMMs in THIS process, alternating runs of the `value` loop (run-ahead, HBM ring):
        # config.value_f32_mfma = products on v_mfma_f32_32x32x2_f32, config.value_split = split-bf16 products (every family that has
        # the form).  `value` above is the one `dtype` names; the other is reported, not claimed.
        n_x = 150                                        # (shorter runs drown a 2 % difference in the run-ahead loop's start-up)
        rates = {}
        for flag in (0, 1, 0, 1):
            _hip.set_option("mfma_split", flag)
            for i in range(10):
                step(i)
            agent.flush()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n_x):
                step(i)
            agent.flush()
            torch.cuda.synchronize()
            rates.setdefault(flag, []).append(n_x / (time.perf_counter() - t0))
        _hip.set_option("mfma_split", split_mode)
        res["config"]["value_f32_mfma"] = float(np.mean(rates[0]))
        res["config"]["value_split"] = float(np.mean(rates[1]))
        # the long-run rate of the mode `dtype` names: a short --steps window is never the only number behind `value`
        res["config"]["value_long"] = float(np.mean(rates[1 if split_mode else 0]))
        res["config"]["value_modes_note"] = ("alternating %d-step runs of the value loop in this process: f32-MFMA %s, split-bf16 %s steps/s"
                                             % (n_x, [round(v, 1) for v in rates[0]], [round(v, 1) for v in rates[1]]))
    if args.full:
        res["kernels"] = {k: {kk: (round(vv, 4) if isinstance(vv, float) else vv) for kk, vv in v.items() if kk != "tags"}
                          for k, v in sorted(table.items(), key=lambda kv: -kv[1]["ms_per_step"])}
    if args.full and world == 1 and not args.no_sa_kernel:
        # BASELINE.json's second metric, "SA-kernel HBM GB/s": the streaming set-abstraction kernels of THIS workload (HBM-bound:
        # 0.5-1 KB moved per row) from the table above -- inside the overlapped step and alone -- plus the materialising
        # configs[3] kernel behind pointnet2_utils.query_and_group
        sa = {}
        for sym in ("gemm_fwd_stream_kernel", "gemm_fwd_stream_kernel<split>", "gemm_bwd_stream_kernel", "gemm_bwd_stream_split_kernel", "gemm_dx_stream_kernel",
                    "gemm_bwd_stream_split_kernel<dX only>", "gemm_dw_gather_stream_kernel", "gemm_dw_stream_kernel"):
            if sym in table:
                t, a1 = table[sym], table_alone.get(sym, {})
                sa[sym] = {"bound": "hbm", "kernel_avg_us": t["kernel_avg_us"], "achieved": t["algorithmic_gbps"], "peak": 8000.0,
                           "unit": "GB/s", "frac": t["frac"], "frac_alone": a1.get("frac"),
                           "traffic": (tj.get(sym) or tj.get(sym.split("<")[0]) or {}).get("bytes_per_launch"),
                           "note": "frac: inside the overlapped step (other encoder passes run beside it); frac_alone: the "
                                   "same launches with the step serialised on one stream"}
        sa["query_and_group"] = sa_kernel_hbm()
        sa["query_and_group"]["traffic"] = tj.get("query_and_group", {}).get("bytes_per_launch")
        res["sa_kernel_hbm"] = sa
        res["sa_kernel_mfma"] = sa_kernel_mfma()          # configs[3] "4b": the fused stack, forward + backward
        # BASELINE.json's second metric where the driver keeps it (it retains `roofline`, `config`, `cpu_baseline` only)
        qg, sm = sa["query_and_group"], res["sa_kernel_mfma"]
        res["roofline"]["sa_kernel_hbm"] = {"kernel": "ball_query_cells_kernel (query_and_group, configs[3]: B=128, N=4096)",
                                            "achieved": qg.get("achieved"), "unit": "GB/s", "peak": 8000.0, "frac": qg.get("frac"),
                                            "kernel_avg_us": 1e3 * qg["launch_ms"], "traffic": qg.get("traffic"),
                                            "sa1_streaming_in_step": {k: {"gbps": v["achieved"], "frac": v["frac"], "us": v["kernel_avg_us"]}
                                                                      for k, v in sa.items() if k != "query_and_group"}}
        res["roofline"]["sa_kernel_mfma"] = {k: sm.get(k) for k in sm if not isinstance(sm.get(k), (dict, list))}
    if args.full and world == 1 and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(cfg, host_batches[0], np.random.default_rng(3).random((B, 6)).astype(np.float32))
    else:
        res["cpu_baseline"] = None
    try:                                   # libraries' own stdio output (the RCCL banner) first: the JSON line stays the LAST line
        leave_group()
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    try:
        main()
    finally:
        import torch.distributed as _dist
        if _dist.is_available() and _dist.is_initialized():
            _dist.destroy_process_group()
