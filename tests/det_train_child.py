"""Child process of tests/test_gpu_deterministic_runs.py: a seeded offline training run of 20 updates through
core.train_test_offline.train_off_policy (no injected noise), then one SHA-256 over every state tensor.  Run it as a fresh
process with GAD_OPT_deterministic=1; it prints `DIGEST <hex> <update_step>`."""
import hashlib
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 17


def main():
    random.seed(SEED)
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    from ga_ddpg_amd import hip
    from ga_ddpg_amd.api import make_agent
    from ga_ddpg_amd.core import train_test_offline as tto
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    from ga_ddpg_amd.synth_data import fill_synthetic_buffer
    agent, cfg = make_agent("ddpg_td3_aux.yaml")
    config = cfg.RL_TRAIN
    config.batch_size = 64
    config.updates_per_step = 10
    config.max_epoch = 21                   # update_step starts at 1: two epochs of ten updates
    config.save_epoch = []
    mem = BaseMemory(1500, cfg, point_dtype=np.float32)
    fill_synthetic_buffer(mem, 1500, seed=6)
    np.random.seed(SEED)                    # (the minibatch indices come from the global numpy stream)
    tto.train_off_policy(agent, mem, config, None, save_model=False)
    if hasattr(agent, "flush"):
        agent.flush()
    torch.cuda.synchronize()
    h = hashlib.sha256()
    nets = {"policy": agent.policy, "policy_target": agent.policy_target, "critic": agent.critic,
            "critic_target": agent.critic_target, "state_feature_extractor": agent.state_feature_extractor}
    for name in sorted(nets):
        for k, v in sorted(nets[name].state_dict().items()):
            h.update((name + "/" + k).encode())
            h.update(v.detach().cpu().contiguous().numpy().tobytes())
    agent._optim_states_out()
    for oname in ("policy_optim", "critic_optim", "state_feat_encoder_optim", "state_feat_val_encoder_optim"):
        opt = getattr(agent, oname)
        for i, p in enumerate(p for grp in opt.param_groups for p in grp["params"]):
            for k in ("exp_avg", "exp_avg_sq"):
                t = opt.state.get(p, {}).get(k)
                if t is not None:
                    h.update(("%s/%d/%s" % (oname, i, k)).encode())
                    h.update(t.detach().cpu().contiguous().numpy().tobytes())
    print("DIGEST %s %d %d" % (h.hexdigest(), agent.update_step, hip.get_option("deterministic")))


if __name__ == "__main__":
    main()
