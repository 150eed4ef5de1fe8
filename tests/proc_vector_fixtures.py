"""Scripted emulators for the process-pool tests.  The pool's workers resolve these factories by
name (``factory="tests.proc_vector_fixtures:<function>"``), so this module imports numpy and
``apex_amd.envs`` only, like the worker itself."""
import os
import sys
import time

from apex_amd.envs.core import Wrapper, make
from apex_amd.envs.proc_vector import worker_info

from .host_env_util import Shortened

TRIGGER = 5   # the action at which the failing emulators of worker 1 misbehave (no start sequence uses it)


def short(env_id):
    """Episodes of a few agent steps: a life every 7 raw frames, so each bank sees dones."""
    return Shortened(make(env_id), life_every=7, over_at=19)


class _Failing(Wrapper):
    """Misbehaves at the first ``TRIGGER`` action when it runs in worker 1 (in-process and in
    worker 0 it is the plain emulator), so the test chooses the agent step that fails."""

    def __init__(self, env, how):
        super().__init__(env)
        self.how = how
        info = worker_info()
        self.armed = info is not None and info[0] == 1

    def step(self, action):
        if self.armed and int(action) == TRIGGER:
            if self.how == "raise":
                raise ZeroDivisionError("scripted emulator failure")
            if self.how == "exit":
                os._exit(3)
            if self.how == "sleep":
                time.sleep(30.0)   # far past the pool's timeout; the pool kills the worker long before
        return self.env.step(action)


def raises(env_id):
    return _Failing(make(env_id), "raise")


def exits(env_id):
    return _Failing(make(env_id), "exit")


def sleeps(env_id):
    return _Failing(make(env_id), "sleep")


def checked(env_id):
    """Fails the worker's start-up if the worker loaded torch or is not single-threaded."""
    assert worker_info() is not None
    assert "torch" not in sys.modules, "a worker process imported torch"
    assert os.environ.get("OMP_NUM_THREADS") == "1" and os.environ.get("OPENBLAS_NUM_THREADS") == "1"
    return make(env_id)
