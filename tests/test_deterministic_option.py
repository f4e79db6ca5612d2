"""The library option "deterministic" and its Python switches (no device needed: gad_set_option allocates nothing)."""
import ctypes as C
import os
import subprocess
import sys

import torch

from ga_ddpg_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_accepts_deterministic_option_and_abi_is_unchanged():
    L = hip.lib()
    assert L.gad_abi_version() == 12
    try:
        assert L.gad_set_option(b"deterministic", 1) == 0
        assert L.gad_set_option(b"deterministic", 0) == 0
    finally:
        hip._lib_det[0] = 0
        hip.sync_deterministic()


def test_set_option_round_trip_and_route_cache_cleared():
    try:
        hip.ROUTES["probe"] = "gemm_fwd(stream)"
        hip.set_option("deterministic", 1)
        assert hip.get_option("deterministic") == 1
        assert hip._lib_det[0] == 1
        assert "probe" not in hip.ROUTES
        hip.set_option("deterministic", 0)
        assert hip.get_option("deterministic") == 0
        assert hip._lib_det[0] == 0
    finally:
        hip.set_option("deterministic", hip.get_option_default("deterministic"))


def test_torch_flag_turns_the_mode_on_and_off():
    hip.set_option("deterministic", 0)
    prev = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
        assert hip.get_option("deterministic") == 1
        assert hip.sync_deterministic() == 1 and hip._lib_det[0] == 1
    finally:
        torch.use_deterministic_algorithms(prev)
    assert hip.get_option("deterministic") == 0
    assert hip.sync_deterministic() == 0 and hip._lib_det[0] == 0


def test_environment_override_reaches_get_option():
    code = ("from ga_ddpg_amd import hip; hip.lib(); "
            "print(hip.get_option('deterministic'), hip._lib_det[0])")
    for v in ("1", "0"):
        env = dict(os.environ, GAD_OPT_deterministic=v)
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert out.stdout.split() == [v, v]
