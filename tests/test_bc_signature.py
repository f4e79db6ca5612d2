"""BC.update_parameters takes `sync` like DDPG's: train_off_policy(run_ahead=True) and the run-ahead loops rely on it."""
import inspect

import pytest


def test_bc_update_parameters_takes_sync():
    from ga_ddpg_amd.core.bc import BC
    p = inspect.signature(BC.update_parameters).parameters
    assert list(p)[:4] == ["self", "batch_data", "updates", "k"]
    assert "sync" in p and p["sync"].default is True


def test_train_off_policy_run_ahead_refuses_an_agent_without_sync():
    """(it used to fall back to the synchronous loop without a word)"""
    from ga_ddpg_amd.core import train_test_offline as tto

    class Agent(object):
        update_step = 1

        def update_parameters(self, batch_data, updates, k):
            raise AssertionError("not reached")
    with pytest.raises(TypeError, match="sync"):
        tto.train_off_policy(Agent(), None, None, sample=lambda batch_size: {}, run_ahead=True, device_replay=False)
