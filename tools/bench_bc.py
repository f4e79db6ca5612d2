"""Step rate of the BC update (configs[0] of BASELINE.json is a BC run) over DeviceReplay.sample_lazy handles, N = 1024, in the three
caller loops:
    (a) sample, update, read the losses -- no lookahead;
    (b) the same with agent.prefetch(next minibatch) in front of every update (train_off_policy's default loop);
    (c) update_parameters(sync=False), the losses read at a flush every 25 updates (train_off_policy(run_ahead=True)).
Also the host time per enqueued step of loop (c): the mean over the first engine.HOST_RING - 1 updates behind every flush, which
cannot block on a staging slot -- a host clock with no synchronisation inside.

    python tools/bench_bc.py [--batches 128,64] [--seconds 2] [--loops a,b,c] [--root OTHER_TREE] [--label NAME]
    python tools/bench_bc.py --fixed-steps 20 --loops a --batches 64      (a fixed number of steps: for a kernel trace)

One JSON line per (batch, loop).  --root measures another checkout of the project with this file (a tree from before
update_parameters took `sync` runs loop (a) only); environment switches (GAD_STEP_PLAN, GAD_FUSED_OPTIM, GAD_BC_PREFETCH_EARLY)
select the paths as everywhere else."""
import argparse
import inspect
import json
import os
import sys
import time


def _loop_a(agent, draw, n):
    for i in range(n):
        out = agent.update_parameters(draw(), agent.update_step, i)
        float(out["bc_loss"])


def _loop_b(agent, draw, n):
    nxt = draw()
    for i in range(n):
        cur = nxt
        if i + 1 < n:
            nxt = draw()
            agent.prefetch(nxt)
        out = agent.update_parameters(cur, agent.update_step, i)
        float(out["bc_loss"])


def _loop_c(agent, draw, n, ring, host):
    pending = []
    for i in range(n):
        t0 = time.perf_counter()
        pending.append(agent.update_parameters(draw(), agent.update_step, i, sync=False))
        if len(pending) < ring:                       # behind a flush: no staging slot to wait for
            host[0] += time.perf_counter() - t0
            host[1] += 1
        if len(pending) == 25 or i == n - 1:
            for p in pending:
                float(p["bc_loss"])
            pending = []


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="128,64")
    ap.add_argument("--seconds", type=float, default=2.0, help="length of a timed window")
    ap.add_argument("--loops", default="a,b,c")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default=None)
    ap.add_argument("--buffer", type=int, default=8000, help="transitions of the synthetic buffer")
    ap.add_argument("--fixed-steps", type=int, default=0, help="run this many steps per loop instead of timed windows")
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch
    from ga_ddpg_amd import engine
    from ga_ddpg_amd.api import make_agent
    from ga_ddpg_amd.core.bc import BC
    from ga_ddpg_amd.core.device_replay import DeviceReplay
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    from ga_ddpg_amd.synth_data import fill_synthetic_buffer
    has_sync = "sync" in inspect.signature(BC.update_parameters).parameters
    loops = [l for l in args.loops.split(",") if l == "a" or has_sync]
    label = args.label or os.path.basename(os.path.abspath(args.root))
    rows = []
    for B in (int(b) for b in args.batches.split(",")):
        torch.manual_seed(1)
        agent, cfg = make_agent("bc_dagger_aux.yaml")
        mem = BaseMemory(args.buffer, cfg, point_dtype=np.float32)
        fill_synthetic_buffer(mem, args.buffer, seed=1)
        dmem = DeviceReplay(mem)
        rng = np.random.default_rng(2)
        draw = lambda: dmem.sample_lazy(B, rng=rng)            # noqa: E731
        host = [0.0, 0]
        run = {"a": lambda n: _loop_a(agent, draw, n), "b": lambda n: _loop_b(agent, draw, n),
               "c": lambda n: _loop_c(agent, draw, n, engine.HOST_RING, host)}
        for l in loops:                                        # every loop of this shape once before anything is timed
            run[l](30)
        torch.cuda.synchronize()
        for l in loops:
            host[0], host[1] = 0.0, 0
            steps, chunk = 0, 50
            t0 = time.perf_counter()
            if args.fixed_steps:
                run[l](args.fixed_steps)
                steps = args.fixed_steps
            else:
                while time.perf_counter() - t0 < args.seconds:
                    run[l](chunk)
                    steps += chunk
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            row = {"tree": label, "B": B, "N": 1024, "loop": l, "steps": steps, "seconds": round(dt, 3), "steps_per_s": round(steps / dt, 1)}
            if l == "c" and host[1]:
                row["host_us_per_enqueued_step"] = round(1e6 * host[0] / host[1], 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


if __name__ == "__main__":
    main()
