"""Offline training driver: the caller loop of the update-step path (reference
core/train_test_offline.py: setup() :60-104, train_off_policy() :107-161, the __main__ wiring :325-360).

    python -m ga_ddpg_amd.core.train_test_offline --config_file ddpg_td3_aux.yaml --data path/to/buffer_dir \
        --save_model --max_epoch 2000 --output_dir output/run0

Kept from the reference: `updates_per_step` updates per epoch, each = memory.sample(batch_size) ->
agent.update_parameters(batch, agent.update_step, i) -> agent.step_scheduler(agent.update_step); `save_model` every
100 epochs (first inner iteration) and at every `save_epoch` step (surfix `epoch_<step>`); stop once
update_step >= max_epoch; batch size = cfg.OFFLINE_BATCH_SIZE (:351); a loss table per epoch.  Not kept (out of scope,
SURVEY section 2): the Ray harness, tensorboard writer, the test()/rollout branch and the PyBullet environment.
The replay buffer is mirrored in HBM by default when it fits (`device_replay="auto"`): sampling then costs one
gather launch instead of a 17 MB host gather + PCIe upload per step; `device_replay=False` / `--host_replay` keep the
reference's host sampling.  `device_relabel=True` / `--device_relabel` (off by default) also mirrors the poses and forms the
hindsight goals of a self-supervised on-policy buffer on the GPU (DeviceReplay(relabel="device")) instead of in a host loop."""
import argparse
import inspect
import itertools
import os
import time

import numpy as np

from .replay_memory import BaseMemory, sample_mixed
from .utils import get_loss_info_dict, migrate_model

LOG_INTERVAL = 4


def setup(config_file="ddpg_td3_aux.yaml", policy=None, pretrained=None, model_surfix="latest", batch_size=None,
          output_dir=None):
    """-> (agent, cfg): config merged as the reference does, networks / optimisers / schedulers built by
    make_nets_opts_schedulers, agent wired with setup_feature_extractor; an optional pretrained directory is migrated
    (BC -> DDPG file names) into output_dir and loaded with set_init_step=True (reference :347-349, utils.py:319-334)."""
    from ..api import make_agent
    agent, cfg = make_agent(config_file, kind=policy)
    cfg.RL_TRAIN.batch_size = int(batch_size if batch_size is not None else cfg.OFFLINE_BATCH_SIZE)   # reference :351
    if pretrained:
        src = pretrained
        # the migration renames BC_* files to DDPG_* (reference utils.py:319-334): only a DDPG agent reads those names
        if agent.name == "DDPG" and output_dir and os.path.abspath(output_dir) != os.path.abspath(pretrained):
            migrate_model(pretrained, output_dir, model_surfix)
            src = output_dir
        paths = agent._paths(src, model_surfix)
        if not (os.path.exists(paths["actor"]) or os.path.exists(paths["state_feat"])):
            raise FileNotFoundError("--pretrained %s: no %s_* actor / state_feat checkpoint with suffix '%s' found in %s"
                                    % (pretrained, agent.name, model_surfix, src))
        agent.load_model(src, surfix=model_surfix, set_init_step=True)
    return agent, cfg


def device_replay_fits(memory, reserve=0.5):
    """True when a float32 mirror of `memory` (DeviceReplay) takes less than `reserve` of the GPU's FREE memory -- 4 x 1030 x 4 B
    per transition: the reference's 2e5-transition offline buffer is 3.3 GB of a 288 GB MI355X"""
    import torch
    if not torch.cuda.is_available():
        return False
    need = int(np.prod(memory.point_state.shape)) * 4 + 64 * memory.point_state.shape[0] * 4
    free, _ = torch.cuda.mem_get_info()
    return need < reserve * free


def device_mirror(memory, relabel="host"):
    """the HBM mirror of `memory`, built ONCE per memory object and kept on it (a caller that alternates
    train_off_policy with buffer writes must neither re-allocate GBs per call nor train on a stale snapshot): a later call
    uploads what was written in between -- DeviceReplay.sync_writes(): the clouds of the slots push() wrote, everything up to
    upper_idx() when the buffer changed in any other way.  relabel: DeviceReplay's hindsight-goal mode; a mirror of each mode
    is kept under its own name (a caller that uses both on one memory pays for both); a buffer named "expert" never relabels,
    so its one mirror serves both modes."""
    from .device_replay import DeviceReplay
    if getattr(memory, "name", "") == "expert":
        relabel = "host"
    attr = "_gad_device_mirror" if relabel == "host" else "_gad_device_mirror_" + str(relabel)
    dmem = getattr(memory, attr, None)
    if dmem is None or dmem.cap != memory.point_state.shape[0]:
        dmem = DeviceReplay(memory, relabel=relabel)
        setattr(memory, attr, dmem)
    else:
        dmem.sync_writes()
    return dmem


def mixed_device_mirror(memory, online_memory, n_expert, n_online, relabel="host"):
    """device_mirror() of both buffers + ONE MixedDeviceReplay for the pair of mirrors and the split, kept on the expert memory
    (the last four pairings: a caller that alternates online buffers or relabel modes re-allocates no staging sets)"""
    from .device_replay import MixedDeviceReplay
    d0, d1 = device_mirror(memory, relabel), device_mirror(online_memory, relabel)
    kept = getattr(memory, "_gad_mixed_mirror", None) or []
    for ent in kept:
        if ent[0] is d0 and ent[1] is d1 and ent[2:4] == (int(n_expert), int(n_online)):
            return ent[4]
    ent = (d0, d1, int(n_expert), int(n_online), MixedDeviceReplay([(d0, n_expert), (d1, n_online)]))
    memory._gad_mixed_mirror = [ent] + list(kept)[:3]
    return ent[4]


def train_off_policy(agent, memory, config, model_output_dir=None, save_model=False, log=None, max_epochs=None,
                     sample=None, run_ahead=False, device_replay="auto", rng=None, online_memory=None, device_relabel=False):
    """The reference's train_off_policy() (:107-161) over an agent and a filled replay memory.
    config = cfg.RL_TRAIN (updates_per_step, batch_size, save_epoch, max_epoch).  `sample(batch_size)` overrides
    memory.sample (device-resident replay, prefetching samplers).  Returns the per-key loss history (deques, as the
    reference keeps them) and the number of epochs run.
    The default loop HOLDS TWO MINIBATCHES AT ONCE: minibatch i + 1 is drawn (and handed to agent.prefetch) before minibatch i is
    passed to update_parameters.  A `sample` callable must therefore return a batch that stays whole until the SECOND call after it:
    fresh arrays or tensors per call (memory.sample, DeviceReplay.sample / sample_lazy), or buffers it does not reuse that early.
    A callable that recycles its buffers says how many of its latest batches stay valid in an attribute `max_outstanding`
    (PrefetchSampler(outstanding=...); None = any number): with a value below 2 the loop draws nothing ahead and holds one batch at a
    time, as under GAD_TRAIN_LOOKAHEAD=0 and as run_ahead=True always does.  Under run_ahead a reused buffer must also not be
    rewritten before the upload of the step that reads it has run: the runtime puts that event into batch["uploaded_event"] when
    the batch dict has this key (PrefetchSampler waits for it).
    run_ahead: enqueue the `updates_per_step` updates of an epoch without waiting for each (update_parameters(sync=False));
    their losses are read at the end of the epoch, the host samples / stages the next minibatch while the GPU works.
    rng: a numpy Generator / RandomState for the minibatch indices of the mirrored path (default: the global np.random
    stream, which is what the reference's memory.sample draws from).
    online_memory: a second BaseMemory.  With config.onpolicy and n_on = int(batch_size * online_buffer_ratio) > 0 every
    update trains on batch_size rows of `memory` followed by n_on rows of `online_memory` (the reference learner's batch,
    core/trainer.py:212-232); the indices are drawn expert first.  Both buffers are mirrored in HBM under the same
    `device_replay` rule (one gather launch per minibatch), else the host forms the batch (replay_memory.sample_mixed).
    device_relabel: the mirrors are built with relabel="device": the hindsight goals of a buffer that relabels (self_supervision,
    not named "expert") are formed by one small launch behind the gather instead of BaseMemory.onpolicy_goals' host loop; equal
    to the host's goals to float32 rounding, not bit for bit.  No effect on the host sampling path."""
    if run_ahead and "sync" not in inspect.signature(agent.update_parameters).parameters:
        raise TypeError("train_off_policy(run_ahead=True): %s.update_parameters takes no `sync` argument, its updates cannot be "
                        "enqueued without waiting for each" % type(agent).__name__)
    relabel = "device" if device_relabel else "host"

    def relabel_note(*mems):
        """what the "mirrored in HBM" line says about hindsight goals when a buffer forms them"""
        if not any(bool(getattr(m, "self_supervision", False)) and getattr(m, "name", "") != "expert" for m in mems):
            return ""
        return "; hindsight goals formed on the %s" % ("device (gad_replay_relabel_goals)" if device_relabel else
                                                       "host (BaseMemory.onpolicy_goals); device_relabel=True forms them on the GPU")
    losses = get_loss_info_dict()
    n_on = int(config.batch_size * config.online_buffer_ratio) if (online_memory is not None and config.onpolicy) else 0
    total_batch = int(config.batch_size) + n_on
    if n_on > 0 and sample is None:
        if device_replay and hasattr(agent, "runtime") and (
                device_replay is True or (device_replay_fits(memory) and device_replay_fits(online_memory))):
            mixed = mixed_device_mirror(memory, online_memory, config.batch_size, n_on, relabel)
            sample = lambda batch_size: mixed.sample_lazy(rng=rng)                  # noqa: E731
            if log is not None:
                log("replay buffers mirrored in HBM (%d expert + %d online transitions); device_replay=False keeps the host "
                    "sampling path%s" % (len(memory), len(online_memory), relabel_note(memory, online_memory)))
        else:
            sample = lambda batch_size: sample_mixed((memory, online_memory), (batch_size, n_on), rng=rng)   # noqa: E731
    if sample is None and device_replay and (device_replay is True or device_replay_fits(memory)) and hasattr(agent, "runtime"):
        # default feeding path: the buffer mirrored in HBM, indices drawn on the host with the
        # reference's arithmetic and random stream (np.random, as memory.sample uses), ONE gather launch per minibatch --
        # the only feeding path that keeps up with a 3 ms update step (bench.py: value_device_replay vs value_host_inclusive)
        dmem = device_mirror(memory, relabel)
        sample = lambda batch_size: dmem.sample_lazy(batch_size, rng=rng)        # noqa: E731
        if log is not None:
            log("replay buffer mirrored in HBM (%d transitions); device_replay=False keeps the host sampling path%s"
                % (len(memory), relabel_note(memory)))
    sample = sample or memory.sample
    epochs = 0
    # The loop below is the reference's: sample, update, read the losses -- every iteration.  What keeps the GPU busy across that
    # host synchronisation: the NEXT minibatch is drawn one iteration early (same draws in the same order: nothing else consumes
    # the sampler's random stream in between) and handed to agent.prefetch(), which stages its upload + geometry beside the
    # running update (device-resident minibatches; a no-op otherwise).
    lookahead = (not run_ahead) and hasattr(agent, "prefetch") and os.environ.get("GAD_TRAIN_LOOKAHEAD", "1") == "1"
    # Drawn ahead, minibatch i + 1 exists while minibatch i has not been uploaded yet: a sampler that keeps only its latest batch
    # valid (PrefetchSampler's default) would refill i's buffers under it.  Such a sampler says so, and is not drawn ahead from:
    # its batches are host batches, which agent.prefetch() does not stage early anyway
    keeps = getattr(sample, "max_outstanding", None)
    if lookahead and keeps is not None and keeps < 2:
        lookahead = False
        if log is not None:
            log("sample.max_outstanding = %d: one minibatch at a time, the next one is not drawn ahead (outstanding=2 allows it)" % keeps)
    ahead = None

    def is_last(epoch, i):
        return i == config.updates_per_step - 1 and (agent.update_step + 1 >= config.max_epoch or
                                                      (max_epochs is not None and epoch >= max_epochs))
    for epoch in itertools.count(1):
        start_time = time.time()
        lrs = agent.get_lr()
        data_time, network_time = 0.0, 0.0
        pending = []
        for i in range(config.updates_per_step):
            batch_data = ahead if ahead is not None else sample(batch_size=config.batch_size)
            ahead = None
            if lookahead and not is_last(epoch, i):
                ahead = sample(batch_size=config.batch_size)
                agent.prefetch(ahead)
            data_time += time.time() - start_time
            start_time = time.time()
            if run_ahead:
                pending.append(agent.update_parameters(batch_data, agent.update_step, i, sync=False))
            else:
                pending.append(agent.update_parameters(batch_data, agent.update_step, i))
            network_time += time.time() - start_time
            agent.step_scheduler(agent.update_step)
            if not run_ahead or i == config.updates_per_step - 1:
                for loss in pending:                          # (run-ahead: the first read of a PendingLog waits for its step)
                    for k, v in loss.items():
                        if k in losses:
                            losses[k].append(v)
                pending = []
            start_time = time.time()
            if save_model and epoch % 100 == 0 and i == 0:
                agent.save_model(agent.update_step, output_dir=model_output_dir)
            if save_model and agent.update_step in config.save_epoch:
                agent.save_model(agent.update_step, output_dir=model_output_dir,
                                 surfix="epoch_{}".format(agent.update_step))
        epochs = epoch
        if log is not None:
            log("epoch: {} updates: {} lr: {:.6f} network time: {:.2f} data time: {:.2f} batch size: {}".format(
                epoch, agent.update_step, lrs["policy_lr"], network_time, data_time, total_batch))
            rows = [(name, float(np.mean(list(h)))) for name, h in losses.items() if np.mean(list(h)) != 0]
            try:
                import tabulate
                log(tabulate.tabulate(rows, ["loss name", "loss val"], tablefmt="psql"))
            except ImportError:
                for r in rows:
                    log("  %-28s %.6f" % r)
        if agent.update_step >= config.max_epoch or (max_epochs is not None and epoch >= max_epochs):
            break
    return losses, epochs


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config_file", default="ddpg_td3_aux.yaml")
    ap.add_argument("--policy", default=None, help="DDPG | BC (default: from cfg.RL_TRAIN.RL)")
    ap.add_argument("--data", default=None, help="directory holding the replay .npz written by BaseMemory.save (reference "
                                                 "format, file name = cfg RL_SAVE_DATA_NAME); default: a seeded synthetic buffer")
    ap.add_argument("--online_data", default=None, help="directory holding a second replay .npz, the ONLINE buffer: with "
                                                        "RL_TRAIN.onpolicy every update adds int(batch_size * online_buffer_ratio) "
                                                        "of its rows to the minibatch, behind the expert rows")
    ap.add_argument("--buffer", type=int, default=20000, help="transitions of the synthetic buffer")
    ap.add_argument("--pretrained", default=None)
    ap.add_argument("--model_surfix", default="latest")
    ap.add_argument("--output_dir", default="output/offline")
    ap.add_argument("--save_model", action="store_true")
    ap.add_argument("--batch_size", type=int, default=None)
    ap.add_argument("--max_epoch", type=int, default=None, help="overrides RL_TRAIN.max_epoch (update steps)")
    ap.add_argument("--host_replay", action="store_true", help="sample on the host and upload every minibatch (the reference's "
                                                               "loop); default: mirror the buffer in HBM when it fits")
    ap.add_argument("--device_relabel", action="store_true", help="form the hindsight goals of a self-supervised on-policy buffer "
                                                                  "on the GPU from mirrored poses (float32 closed form) instead "
                                                                  "of in the host's per-row loop; default: the host forms them")
    args = ap.parse_args(argv)
    agent, cfg = setup(args.config_file, args.policy, args.pretrained, args.model_surfix, args.batch_size, args.output_dir)
    config = cfg.RL_TRAIN
    if args.max_epoch is not None:
        config.max_epoch = args.max_epoch
    if args.data:
        memory = BaseMemory(int(cfg.OFFLINE_RL_MEMORY_SIZE) + 1, config)
        memory.load(args.data, int(cfg.OFFLINE_RL_MEMORY_SIZE))
    else:
        from ..synth_data import fill_synthetic_buffer
        memory = BaseMemory(args.buffer, config, point_dtype=np.float32)
        fill_synthetic_buffer(memory, args.buffer, seed=20260928)
    online = None
    if args.online_data:
        online = BaseMemory(int(cfg.OFFLINE_RL_MEMORY_SIZE) + 1, config, name="online")
        online.load(args.online_data, int(cfg.OFFLINE_RL_MEMORY_SIZE))
    losses, epochs = train_off_policy(agent, memory, config, args.output_dir, args.save_model, log=print,
                                      device_replay=False if args.host_replay else "auto", online_memory=online,
                                      device_relabel=args.device_relabel)
    if args.save_model:
        agent.save_model(agent.update_step, output_dir=args.output_dir)
    return losses, epochs


if __name__ == "__main__":
    main()
