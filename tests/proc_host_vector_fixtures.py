"""Scripted envs for the host vector pool's tests.  The pool's workers resolve these factories by
name (``factory="tests.proc_host_vector_fixtures:<function>"``), so this module imports
``apex_amd.envs`` only, like the worker itself."""
import os
import sys

from apex_amd.envs.core import Wrapper, make
from apex_amd.envs.proc_vector import worker_info

FAIL_AT = 3   # the env step (1-based) at which the failing env of worker 1 raises


class _RaisesAtThirdStep(Wrapper):
    """Raises on its ``FAIL_AT``-th step when it runs in worker 1 (in-process and in worker 0 it is
    the plain env)."""

    def __init__(self, env):
        super().__init__(env)
        info = worker_info()
        self.armed = info is not None and info[0] == 1
        self.n = 0

    def step(self, action):
        self.n += 1
        if self.armed and self.n == FAIL_AT:
            raise ZeroDivisionError("scripted env failure")
        return self.env.step(action)


def raises_third(env_id):
    return _RaisesAtThirdStep(make(env_id))


def checked(env_id):
    """Fails the worker's start-up if the worker loaded torch or is not single-threaded."""
    assert worker_info() is not None
    assert "torch" not in sys.modules, "a worker process imported torch"
    assert os.environ.get("OMP_NUM_THREADS") == "1" and os.environ.get("OPENBLAS_NUM_THREADS") == "1"
    return make(env_id)
