"""Factories that fail in every worker, worker 0 last (``tests/test_host_eval_host.py``).  Imports
numpy-free modules only, like the worker itself."""
import time

from apex_amd.envs.proc_vector import worker_info


def all_fail_zero_last(env_id):
    w = worker_info()[0]
    if w == 0:
        time.sleep(0.3)   # the other workers' failures reach the parent first
    raise LookupError(f"scripted start-up failure in worker {w}")
