"""Deterministic mode, the remaining acceptance checks: the user's case (the same seeded training script run twice, in two
fresh processes, through train_off_policy), the encoder on its own with two different grid-rows hints, and the
forced-decision float64 gate of a policy step in the mode."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ga_ddpg_amd import hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_det_seeded_training_runs_agree_across_processes():
    """two fresh processes, one after the other, each a seeded 20-update train_off_policy run with GAD_OPT_deterministic=1:
    the SHA-256 over every parameter, buffer, target network and Adam moment is the same"""
    env = dict(os.environ, GAD_OPT_deterministic="1")
    digests = []
    for _ in range(2):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "det_train_child.py")], cwd=ROOT, env=env,
                             capture_output=True, text=True, timeout=420)
        assert out.returncode == 0, out.stderr[-4000:]
        line = [l for l in out.stdout.splitlines() if l.startswith("DIGEST ")]
        assert line, out.stdout[-2000:]
        _, digest, step, mode = line[-1].split()
        assert int(step) == 21 and int(mode) == 1, line[-1]
        digests.append(digest)
    assert digests[0] == digests[1], digests


def _encoder_run(value, hint_live):
    """tests/test_gpu_kernel_families._run's encoder forward + backward (B = 96) in the mode, with the geometry's grid-rows
    hints at 0 (worst-case grids) or at the live row counts (smaller grids)"""
    from ga_ddpg_amd import engine
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    from ga_ddpg_amd.experiments.config import load_cfg
    from ga_ddpg_amd.synth_data import fill_synthetic_buffer, sample_valid_batch
    from tests.test_gpu_encoder import _feature_net, _geometry, _run_encoder
    B = 96
    torch.manual_seed(0)
    dev = torch.device("cuda")
    mem = BaseMemory(400, load_cfg("ddpg_td3_aux.yaml"), point_dtype=np.float32)
    fill_synthetic_buffer(mem, 400, seed=11)
    batch = sample_valid_batch(mem, B, np.random.default_rng(3))
    net = _feature_net()
    geo = _geometry(B)
    geo.run(torch.from_numpy(batch["point_state_batch"]).cuda())
    n = [int(geo.rows[s]["n"].item()) for s in range(3)]
    geo.rows_hint[:] = n[:2] if hint_live else 0
    action = torch.from_numpy(batch["action_batch"]).cuda() if value else None
    probe = torch.from_numpy(np.random.default_rng(5).normal(size=(B, 512)).astype(np.float32)).cuda()
    enc = engine.EncoderNet(net.value_encoder if value else net.encoder, dev)
    slot = engine.EncoderSlot(geo, enc, dev)
    z = _run_encoder(enc, slot, action, probe, value)
    out = {"z": z, "mean": slot.mean, "istd": slot.istd, "grad": enc.flat.grad, "running_mean": enc.running_mean,
           "running_var": enc.running_var}
    for s in range(3):
        for l in range(3):
            out["Z%d%d" % (s + 1, l + 1)] = slot.Z[s][l][:n[s]]
        out["F%d" % (s + 1)] = slot.F[s]
        out["dF%d" % (s + 1)] = slot.dF[s]
    if value:
        out["daction"] = slot.daction
    return {k: v.detach().cpu().clone() for k, v in out.items()}, n


@pytest.mark.parametrize("value", [False, True], ids=["policy_encoder", "value_encoder"])
def test_det_encoder_bitwise_across_grid_hints(value):
    prev = hip.get_option("deterministic")
    hip.set_option("deterministic", 1)
    try:
        a, na = _encoder_run(value, hint_live=False)
        b, nb = _encoder_run(value, hint_live=True)
    finally:
        hip.set_option("deterministic", prev)
    assert na == nb and na[0] > 0 and na[1] > 0
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, bad
    assert float(a["grad"].abs().max()) > 0 and float(a["dF1"].abs().max()) > 0


def test_det_forced_decision_gate_policy_step_B64():
    """tests/kink_forcing.py: the float64 oracle evaluated with the HIP pass's ReLU / max-pool decisions; one DDPG policy step at
    B = 64 in the mode, 0 violations of the float32 yardstick"""
    from tests.test_gpu_forced_decisions import test_step_gradients_with_forced_decisions as gate
    prev = hip.get_option("deterministic")
    hip.set_option("deterministic", 1)
    try:
        gate(64, 2, True, None)
    finally:
        hip.set_option("deterministic", prev)
