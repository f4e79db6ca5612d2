"""bench.py's own launcher (CPU part): `--gpus N` with N > 1 and no WORLD_SIZE in the environment re-executes the file under
torch.distributed.run with N ranks on 127.0.0.1 (the GPU part -- two ranks really running -- is tests/test_gpu_dp.py)."""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_flag_spawns_ranks(monkeypatch):
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 0
    import subprocess
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7", "--warmup", "3"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    rc = bench.launch_ranks(types.SimpleNamespace(gpus=4))
    assert rc == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "7", "--warmup", "3"]
    assert os.path.basename(cmd[cmd.index("--master-port") + 2]) == "bench.py"
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_main_dispatches_to_launcher(monkeypatch):
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(bench, "launch_ranks", lambda a: 17)
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 17
    else:
        raise AssertionError("main() did not hand over to the launcher")


def test_plain_run_is_lean_by_default(monkeypatch):
    """without --full a run measures the headline rate only; --dump-outputs is off unless a directory is given"""
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 5 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "5", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_float_arrays(tmp_path):
    """DIR/<name>.npy in float64 (losses) / float32 (tensors); a flat above the cap is a fixed, seeded sample of it"""
    sys.path.insert(0, ROOT)
    import importlib
    import numpy as np
    import torch
    bench = importlib.import_module("bench")
    big = torch.arange(bench.DUMP_CAP + 1000, dtype=torch.float32)
    tensors = {"pi": torch.ones(4, 6), "qf1": torch.ones(4, 9)[:, 0], "params_x": big}
    total = bench.dump_outputs(str(tmp_path / "a"), {"critic_loss": 1.5}, tensors)
    bench.dump_outputs(str(tmp_path / "b"), {"critic_loss": 1.5}, tensors)
    loss = np.load(tmp_path / "a" / "loss_critic_loss.npy")
    assert loss.dtype == np.float64 and loss.tolist() == [1.5]
    pi = np.load(tmp_path / "a" / "pi.npy")
    assert pi.dtype == np.float32 and pi.shape == (4, 6)
    p = np.load(tmp_path / "a" / "params_x.npy")
    assert p.dtype == np.float32 and p.size == bench.DUMP_CAP and len(np.unique(p)) == p.size
    assert np.array_equal(p, np.load(tmp_path / "b" / "params_x.npy"))
    assert total <= 64 * 1024 * 1024


def test_restore_training_state_puts_back_every_network():
    """--dump-outputs: the last timed step starts from the saved state -- parameters and Adam moments of every network, in place
    (the runtime's launch lists hold their addresses), followed by a re-pack of each"""
    sys.path.insert(0, ROOT)
    import importlib
    import torch
    bench = importlib.import_module("bench")

    class Flat(object):
        def __init__(self, v):
            self.master, self.exp_avg, self.exp_avg_sq = torch.full((5,), v), torch.full((5,), v + 1), torch.full((5,), v + 2)
            self.synced = 0

        def sync_packed(self):
            self.synced += 1
    rt = types.SimpleNamespace(**{n: types.SimpleNamespace(flat=Flat(float(k))) for k, n in enumerate(bench.STATE_FLATS)})
    saved = bench.training_state(rt)
    ptrs = {n: getattr(rt, n).flat.master.data_ptr() for n in bench.STATE_FLATS}
    for n in bench.STATE_FLATS:
        f = getattr(rt, n).flat
        for t in (f.master, f.exp_avg, f.exp_avg_sq):
            t.add_(100.0)
    bench.restore_training_state(rt, saved)
    for k, n in enumerate(bench.STATE_FLATS):
        f = getattr(rt, n).flat
        assert f.master.tolist() == [float(k)] * 5 and f.exp_avg.tolist() == [k + 1.0] * 5 and f.exp_avg_sq.tolist() == [k + 2.0] * 5
        assert f.master.data_ptr() == ptrs[n] and f.synced == 1
